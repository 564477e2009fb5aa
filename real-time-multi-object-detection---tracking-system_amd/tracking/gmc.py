"""Camera-motion estimation for BoT-SORT on MI355X: the 2x3 similarity warp (rotation, uniform scale, translation) from the previous
frame to the current one, computed from the frames themselves on the GPU behind ``rtmodt_gmc_*`` (``include/rtmodt.h``,
``csrc/gmc.hip``), so that a caller with frames and no PTZ telemetry gets BoT-SORT's camera-motion compensation.

The rules are this project's own (an integer luma pyramid, a coarse translation, 16 x 16 block matching with a sub-pixel step, a
fixed sequence of two-point hypotheses, a similarity refitted from exact integer sums).  PINNED: the kernels equal the plain-Python
restatement ``tests/gmc_ref.py`` bit for bit.  PARITY UNPINNED: OpenCV and BoT-SORT's ``GMC`` (sparse optical flow / ORB / ECC, then
``estimateAffinePartial2D``) are installed nowhere this runs; ``DESIGN.md`` section 23 lists the deliberate differences.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi

OK, FIRST, FEW_BLOCKS, FEW_INLIERS, BAD_SCALE = 0, 1, 2, 3, 4
STATUS_NAMES = {OK: "estimated", FIRST: "first frame", FEW_BLOCKS: "too few valid blocks", FEW_INLIERS: "too few inliers",
                BAD_SCALE: "scale outside [0.5, 2]"}
MAX_HYP = 256
TABLE = 1089


def default_cfg() -> _ffi.GmcCfg:
    cfg = _ffi.GmcCfg()
    _ffi.lib().rtmodt_gmc_default_cfg(C.byref(cfg))
    return cfg


class CameraMotionEstimator(_ffi.Handle):
    """``estimate(frames, detections=None) -> (warp[n, 2, 3], status[n])`` for ``n_streams`` streams at once (a fixed number of
    launches).  The first frame of a stream after construction or :meth:`reset` returns the identity with status ``FIRST``; whenever
    the status is not ``OK`` the warp is exactly the identity.  ``detections``: per stream ``None`` or something with ``xyxy`` and
    ``confidence`` (a ``Detections``): the blocks those boxes meet take no part."""

    def __init__(self, downscale: int = 4, *, coarse_search: int | None = None, search: int | None = None, min_texture: int | None = None,
                 max_sad: int | None = None, mask_conf: float | None = None, n_hyp: int | None = None, seed: int | None = None,
                 min_sep: float | None = None, inlier_px: float | None = None, min_blocks: int | None = None, min_inliers: int | None = None,
                 max_boxes: int | None = None, n_streams: int = 1, device=0) -> None:
        cfg = default_cfg()
        cfg.downscale = int(downscale)
        for name, v in (("coarse_search", coarse_search), ("search", search), ("min_texture", min_texture), ("max_sad", max_sad), ("n_hyp", n_hyp),
                        ("seed", seed), ("min_blocks", min_blocks), ("min_inliers", min_inliers), ("max_boxes", max_boxes)):
            if v is not None:
                setattr(cfg, name, int(v))
        for name, v in (("mask_conf", mask_conf), ("min_sep", min_sep), ("inlier_px", inlier_px)):
            if v is not None:
                setattr(cfg, name, float(v))
        cfg.n_streams, cfg.device = int(n_streams), _ffi.device_ordinal(device)
        self.cfg, self.n_streams, self._device = cfg, int(n_streams), cfg.device
        self._geom = None
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_gmc_create(C.byref(cfg), C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def estimate(self, frames, detections=None, *, mem_kind=_ffi.MEM_HOST, height=0, width=0, stride=0):
        S, MB = self.n_streams, self.cfg.max_boxes
        if len(frames) != S:
            raise ValueError(f"{len(frames)} frames for {S} streams")
        fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        xy = cf = cnt = None
        if detections is not None:
            if len(detections) != S:
                raise ValueError(f"{len(detections)} detection sets for {S} streams")
            xy, cf, cnt = np.zeros((S, MB, 4), np.float32), np.zeros((S, MB), np.float32), np.zeros(S, np.int32)
            for s, d in enumerate(detections):
                if d is None:
                    continue
                b = np.asarray(d.xyxy, np.float32).reshape(-1, 4)
                if len(b) > MB:
                    raise ValueError(f"stream {s}: {len(b)} boxes > max_boxes {MB}")
                xy[s, :len(b)], cf[s, :len(b)], cnt[s] = b, np.asarray(d.confidence, np.float32).reshape(-1), len(b)
        warp, status = np.zeros((S, 2, 3), np.float32), np.zeros(S, np.int32)
        _ffi.check(_ffi.lib().rtmodt_gmc_estimate_batch(self._h, fp, int(height), int(width), int(stride), int(mem_kind), _ffi.ptr(xy), _ffi.ptr(cf),
                                                        _ffi.ptr(cnt), _ffi.ptr(warp), _ffi.ptr(status)))
        del keep
        self._geom = (int(height), int(width))
        return warp, status

    def estimate_from_detector(self, detector, frames, *, mem_kind=_ffi.MEM_HOST, height=0, width=0, stride=0) -> None:
        """The estimate for the frames of ``detector``'s last batch, masked with its device-resident detections, queued on the
        detector's stream: no host hop.  :meth:`result` fetches."""
        fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        _ffi.check(_ffi.lib().rtmodt_gmc_estimate_from_detector(self._h, detector.model.handle, fp, len(frames), int(height), int(width), int(stride),
                                                                int(mem_kind)))
        self._geom = (int(height), int(width))
        if keep:                                         # pageable host frames: the copy has been issued from them; wait before they may go
            _ffi.check(_ffi.lib().rtmodt_synchronize(self._device))

    def result(self):
        warp, status = np.zeros((self.n_streams, 2, 3), np.float32), np.zeros(self.n_streams, np.int32)
        _ffi.check(_ffi.lib().rtmodt_gmc_result(self._h, _ffi.ptr(warp), _ffi.ptr(status)))
        return warp, status

    def geometry(self) -> dict:
        """Level sizes and block counts of the last frame size."""
        if self._geom is None:
            raise ValueError("no frame has been estimated yet")
        h, w = self._geom
        d = self.cfg.downscale
        w0, h0 = w // d, h // d
        return dict(W0=w0, H0=h0, W1=w0 // 4, H1=h0 // 4, BX=w0 // 16, BY=h0 // 16, nb=(w0 // 16) * (h0 // 16))

    def debug(self, stream: int = 0) -> dict:
        """Every intermediate of the stream's last frame (``rtmodt_gmc_debug``), named as ``tests/gmc_ref.py`` names them."""
        g = self.geometry()
        nb, cs = g["nb"], self.cfg.coarse_search
        l0, l1 = np.zeros((g["H0"], g["W0"]), np.uint8), np.zeros((g["H1"], g["W1"]), np.uint8)
        table, coarse, blk, order = np.zeros(TABLE, np.int32), np.zeros(2, np.int32), np.zeros((6, nb), np.int32), np.zeros(nb, np.int32)
        scores, inl, sums, model = np.zeros(MAX_HYP, np.int32), np.zeros((2, nb), np.uint8), np.zeros((2, 8), np.int64), np.zeros((3, 4), np.float64)
        nv, bk = C.c_int32(0), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_gmc_debug(self._h, int(stream), _ffi.ptr(l0), _ffi.ptr(l1), _ffi.ptr(table), _ffi.ptr(coarse), _ffi.ptr(blk),
                                               _ffi.ptr(order), C.cast(C.byref(nv), C.c_void_p), _ffi.ptr(scores), C.cast(C.byref(bk), C.c_void_p),
                                               _ffi.ptr(inl), _ffi.ptr(sums), _ffi.ptr(model)))
        n = nv.value
        names = ("reason", "dx", "dy", "offx", "offy", "sad")
        return dict(l0=l0, l1=l1, table=table[:(2 * cs + 1) ** 2].reshape(2 * cs + 1, 2 * cs + 1), coarse=(int(coarse[0]), int(coarse[1])),
                    blk={k: blk[i].copy() for i, k in enumerate(names)}, order=order[:n].copy(), scores=scores, best_k=int(bk.value),
                    inl=inl[:, :n].copy(), sums=sums, model=model)

    def last_ms(self) -> float:
        return _ffi.last_ms("rtmodt_gmc_last_ms", self._h)

    def reset(self, stream: int = -1) -> None:
        _ffi.check(_ffi.lib().rtmodt_gmc_reset(self._h, int(stream)))

    _destroy = "rtmodt_gmc_destroy"
