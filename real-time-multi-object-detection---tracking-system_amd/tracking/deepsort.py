"""DeepSORT on MI355X: the tracker the reference's config offers (``tracking.algorithm: "deepsort"`` and its ``deepsort:`` block,
config/default.yaml:47-60) but never wired (src/tracking/tracker.py:212-214 raises -- and ``MultiObjectTracker("deepsort")`` here
raises the same error, as the reference does; this class is the way in).

The algorithm is the published one (Wojke et al.; deep_sort's tracker / linear_assignment / nn_matching / kalman_filter), with the
state resident on the GPU behind ``rtmodt_deepsort_*`` (``include/rtmodt.h``, ``csrc/deepsort.hip``).  PARITY UNPINNED:
``deep_sort_realtime`` is not installed anywhere this runs.  The appearance descriptor is the colour histogram of the reference's
design document (B.4), computed on the GPU from the frame, or -- with ``embedder="<file>.rtreid"`` -- the OSNet x0.25 network the
config's ``embedder`` names (``tracking.reid``, ``csrc/reid.hip``), also from the frame on the GPU; embeddings of a network that
runs elsewhere come in through ``embeddings=``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi
from ._common import TrailKeeper, pad_single_stream
from ..reid_weights import FEAT_DIM, SUFFIX
from .reid import check_weights_path
from .tracker import Track

TENTATIVE, CONFIRMED = 1, 2
DEFAULT_MAX_DETS = 1024
#: with an embedder network every detection slot holds the crop's 13 tap tensors and scratch: 2.9 MB of device memory
DEFAULT_MAX_DETS_NETWORK = 128
BUILTIN_EMBEDDER = "colorhist"
BUILTIN_DIM = 192


def _xyah_to_xyxy(m: np.ndarray) -> np.ndarray:
    """The tracker's own rule (csrc/track_dev.h: xyah_to_xyxy), float32 operation by operation."""
    m = np.asarray(m, np.float32).reshape(-1, 4)
    w = m[:, 2] * m[:, 3]
    x1 = m[:, 0] - w * np.float32(0.5)
    y1 = m[:, 1] - m[:, 3] * np.float32(0.5)
    return np.stack([x1, y1, x1 + w, y1 + m[:, 3]], 1).astype(np.float32)


class _DeepSortCore(_ffi.Handle):
    """Host face of the device tracker: ``n_streams`` independent states advanced by one call (a fixed number of launches)."""

    def __init__(self, max_dist=0.2, min_confidence=0.3, max_iou_distance=0.7, max_age=70, n_init=3, nn_budget=100, embedder=BUILTIN_EMBEDDER, *,
                 dim: int = 0, device=0, max_tracks: int = 256, max_dets: int = 1024, n_streams: int = 1) -> None:
        self.max_tracks, self.max_dets, self.n_streams, self.nn_budget = int(max_tracks), int(max_dets), int(n_streams), int(nn_budget)
        self.dim = int(dim) or (FEAT_DIM if embedder is not None and str(embedder).endswith(SUFFIX) else BUILTIN_DIM)
        self._device = _ffi.device_ordinal(device)
        emb = None if embedder is None else str(embedder).encode()
        cfg = _ffi.DeepSortCfg(float(max_dist), float(min_confidence), float(max_iou_distance), int(max_age), int(n_init), int(nn_budget), emb,
                               self.dim, self.max_tracks, self.max_dets, self.n_streams, self._device)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_deepsort_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def update_batch(self, xyxy, confidence, class_id, counts, frames=None, embeddings=None, *, mem_kind=_ffi.MEM_HOST, height=0, width=0,
                     stride=0) -> np.ndarray:
        """All streams at once: arrays shaped ``[n_streams, max_dets(, 4)]``, ``counts[n_streams]``, and either ``frames`` (one per
        stream: ``(h, w, 3)`` uint8 host arrays, or device addresses with ``mem_kind=MEM_DEVICE`` and the geometry given) or
        ``embeddings`` (``[n_streams, max_dets, dim]`` int8, see ``_ffi.appearance_quantize``).  Returns the number of confirmed
        tracks matched in this frame, per stream."""
        S, N = self.n_streams, self.max_dets
        xyxy = np.ascontiguousarray(xyxy, np.float32).reshape(S, N, 4)
        confidence = np.ascontiguousarray(confidence, np.float32).reshape(S, N)
        class_id = np.ascontiguousarray(class_id, np.int32).reshape(S, N)
        counts = np.ascontiguousarray(counts, np.int32).reshape(S)
        fp, keep = None, None
        if frames is not None:
            if len(frames) != S:
                raise ValueError(f"{len(frames)} frames for {S} streams")
            fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        if embeddings is not None:
            embeddings = np.ascontiguousarray(embeddings, np.int8).reshape(S, N, self.dim)
        ret = np.zeros(S, np.int32)
        _ffi.check(_ffi.lib().rtmodt_deepsort_update_batch(self._h, _ffi.ptr(xyxy), _ffi.ptr(confidence), _ffi.ptr(class_id), _ffi.ptr(counts), fp,
                                                           int(height), int(width), int(stride), int(mem_kind), _ffi.ptr(embeddings), _ffi.ptr(ret)))
        del keep
        return ret

    def update(self, xyxy, confidence, class_id, frame=None, embeddings=None, stream: int = 0) -> int:
        """One frame of a single-stream tracker."""
        if self.n_streams != 1 or stream != 0:
            raise ValueError("update() drives a single-stream tracker; use update_batch for several streams")
        bx, cf, cl, n = pad_single_stream(xyxy, confidence, class_id, self.max_dets)
        emb = None
        if embeddings is not None:
            emb = np.zeros((1, self.max_dets, self.dim), np.int8)
            emb[0, :n] = np.asarray(embeddings, np.int8).reshape(n, self.dim)
        return int(self.update_batch(bx, cf, cl, [n], None if frame is None else [frame], emb)[0])

    def update_from_detector(self, detector, frames, *, mem_kind=_ffi.MEM_HOST, height=0, width=0, stride=0) -> None:
        """Consume the detector's device-resident detections of its last batch (stream i <- frame i) and describe them on
        ``frames`` (the frames that batch was made of), asynchronously on the detector's stream: no host hop."""
        fp, keep, height, width, stride = _ffi.frame_pointers(frames, mem_kind, height, width, stride)
        _ffi.check(_ffi.lib().rtmodt_deepsort_update_from_detector(self._h, detector.model.handle, fp, len(frames), int(height), int(width),
                                                                   int(stride), int(mem_kind)))
        if keep:                                         # pageable host frames: the copy has been issued from them; wait before they may go
            _ffi.check(_ffi.lib().rtmodt_synchronize(self._device))

    def snapshot(self, stream: int = 0, gallery: bool = True) -> dict:
        """The parity surface (``rtmodt_deepsort_state``), list order."""
        M, B, D = self.max_tracks, self.nn_budget, self.dim
        ids = np.zeros(M, np.int64)
        state, hits, age, tsu, cls, gcnt = (np.zeros(M, np.int32) for _ in range(6))
        box, conf = np.zeros((M, 4), np.float32), np.zeros(M, np.float32)
        mean, cov = np.zeros((M, 8), np.float32), np.zeros((M, 12), np.float32)
        gal = np.zeros((M, B, D), np.int8) if gallery else None
        n, nid = C.c_int32(0), C.c_int64(0)
        _ffi.check(_ffi.lib().rtmodt_deepsort_state(self._h, stream, _ffi.ptr(ids), _ffi.ptr(state), _ffi.ptr(hits), _ffi.ptr(age), _ffi.ptr(tsu),
                                                    _ffi.ptr(box), _ffi.ptr(conf), _ffi.ptr(cls), _ffi.ptr(mean), _ffi.ptr(cov), _ffi.ptr(gcnt),
                                                    _ffi.ptr(gal), C.byref(n), C.byref(nid)))
        k = n.value
        out = {"ids": ids[:k].copy(), "state": state[:k].copy(), "hits": hits[:k].copy(), "age": age[:k].copy(), "tsu": tsu[:k].copy(),
               "xyxy": box[:k].copy(), "conf": conf[:k].copy(), "cls": cls[:k].copy(), "mean": mean[:k].copy(), "cov": cov[:k].copy(),
               "gallery_count": gcnt[:k].copy(), "next_id": int(nid.value)}
        if gallery:
            out["gallery"] = gal[:k].copy()
        return out

    def last_ms(self) -> tuple:
        """Device time (ms) of the last update: (descriptors, distance, update)."""
        return _ffi.last_ms("rtmodt_deepsort_last_ms", self._h, 3)

    def reset(self, stream: int = -1) -> None:
        _ffi.check(_ffi.lib().rtmodt_deepsort_reset(self._h, stream))

    _destroy = "rtmodt_deepsort_destroy"


class DeepSortTracker:
    """``update(detections, frame=...) -> list[Track]``: the confirmed tracks matched in this frame (deep_sort's
    ``is_confirmed() and time_since_update == 0``), ``xyxy`` = the posterior mean box, trails as ``MultiObjectTracker`` keeps them.

    ``max_dets`` (detections per frame the handle is sized for) defaults to 1024 with the built-in descriptor or caller descriptors,
    and to 128 with an embedder network: the network keeps 2.9 MB of device memory per detection slot (128 slots = 0.37 GB; 1024
    would be 3 GB for one stream).  A detector feeding ``update_from_detector`` must have ``max_det <= max_dets``."""

    #: ``pipeline.run`` hands the frame to a tracker that asks for it
    needs_frame = True

    def __init__(self, max_dist: float = 0.2, min_confidence: float = 0.3, max_iou_distance: float = 0.7, max_age: int = 70, n_init: int = 3,
                 nn_budget: int = 100, embedder: str = BUILTIN_EMBEDDER, *, embedding_dim: int = 0, device=0, max_tracks: int = 256,
                 max_dets: int | None = None) -> None:
        if embedder in (None, ""):
            embedder = BUILTIN_EMBEDDER
        if str(embedder).endswith(SUFFIX):
            embedder = check_weights_path(embedder)             # FileNotFoundError, as the detector words it
            if embedding_dim not in (0, FEAT_DIM):
                raise ValueError(f"embedding_dim {embedding_dim}: the network's descriptor has {FEAT_DIM} values")
        elif embedder != BUILTIN_EMBEDDER:
            raise NotImplementedError(
                f"embedder {embedder!r}: no embedding network runs here, only the built-in {BUILTIN_EMBEDDER!r} descriptor. Run the model "
                "yourself and pass its output per detection as update(..., embeddings=) on a tracker built with embedding_dim=<its dimension>. "
                f"An OSNet x0.25 checkpoint converted with tools/convert_weights.py --reid (a {SUFFIX} file) does run here.")
        if max_dets is None:
            max_dets = DEFAULT_MAX_DETS_NETWORK if embedder != BUILTIN_EMBEDDER else DEFAULT_MAX_DETS
        self.algorithm = "deepsort"
        self.embedder = embedder
        self._core = _DeepSortCore(max_dist, min_confidence, max_iou_distance, max_age, n_init, nn_budget, embedder, dim=embedding_dim,
                                   device=device, max_tracks=max_tracks, max_dets=max_dets)
        self._trails = TrailKeeper()

    @classmethod
    def from_config(cls, tracking_cfg: dict, **extra) -> "DeepSortTracker":
        """``cfg["tracking"]`` of the reference's YAML (config/default.yaml:46-60): reads its ``deepsort:`` block.  The block's
        ``embedder`` names an ``.onnx`` file, which is not read; it is refused as in the constructor unless ``embedder=`` overrides it
        (``"colorhist"``, or the ``.rtreid`` conversion of that model)."""
        p = dict(tracking_cfg.get("deepsort", {}))
        p.update(extra)
        known = ("max_dist", "min_confidence", "max_iou_distance", "max_age", "n_init", "nn_budget", "embedder", "embedding_dim", "device",
                 "max_tracks", "max_dets")
        return cls(**{k: v for k, v in p.items() if k in known})

    def update(self, detections, frame=None, embeddings=None) -> list:
        n = len(detections.confidence)
        if n and (frame is None) == (embeddings is None):
            raise ValueError("update() needs exactly one of frame= (built-in descriptor) or embeddings= (one row per detection)")
        if embeddings is not None and self.embedder != BUILTIN_EMBEDDER:
            raise ValueError("this tracker computes its descriptors with its embedder network: give frame=, not embeddings=")
        if embeddings is not None:
            embeddings = np.asarray(embeddings)
            if embeddings.dtype != np.int8:
                embeddings = _ffi.appearance_quantize(embeddings)
        ret = self._core.update(detections.xyxy, detections.confidence, detections.class_id, frame if n else None, embeddings if n else None)
        return self._tracks_out() if ret else []

    def update_from_detector(self, detector, frame=None, materialize: bool = True) -> list:
        """:meth:`update` fed from ``detector``'s device-resident detections of its last ``detect`` on ``frame``."""
        if frame is None:
            raise ValueError("update_from_detector() needs the frame the detector ran on")
        self._core.update_from_detector(detector, [frame])
        return self._tracks_out() if materialize else []

    def _tracks_out(self) -> list:
        st = self._core.snapshot(0, gallery=False)
        boxes = _xyah_to_xyxy(st["mean"][:, :4])
        self._trails.drop_dead(st["ids"])
        out = []
        for i in np.nonzero((st["state"] == CONFIRMED) & (st["tsu"] == 0))[0]:
            tid, b = int(st["ids"][i]), boxes[i]
            out.append(Track(track_id=tid, xyxy=b, confidence=float(st["conf"][i]), class_id=int(st["cls"][i]), age=int(st["age"][i]),
                             time_since_update=0, trail=self._trails.push(tid, b)))
        return out

    def close(self) -> None:
        self._core.close()
