"""What a tracked object LOOKED like, kept on MI355X: one best-shot thumbnail per track for the alert record and the review queue.

The reference's alert (``src/events/zone_engine.py``) carries ``bbox_xyxy`` and a ``frame_id`` and no picture; by the time an operator
reads ``events.jsonl`` the frame is gone.  ``SnapshotGallery`` decides per track, on the device, whether this frame's view is better
than the one kept (confidence x visible area, halved when the box is cut by the frame border or overlapped by another) and, if so,
resamples the crop -- exact area average, never enlarged, aspect ratio kept, grey padding -- into a fixed-size BGR24 slot in device
memory.  A call reports which thumbnails changed (``updated``) and which tracks ended (``retired``); a retired thumbnail stays intact
until the next call on its stream, which is the window to read or encode it.  The work runs in ``csrc/snapshot.hip`` (rules in its
header and in ``csrc/snapshot_rule.h``); there is no CPU implementation here.  ``tests/snapshot_ref.py`` restates the rules and the
kernels equal it exactly; parity with ``cv2.resize(INTER_AREA)``, Ultralytics' ``ObjectCropper`` and Frigate's snapshot choice is
unpinned, and every default is unvalidated on real footage.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Callable, Iterable, Optional, Sequence

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker

F_NEW, F_REWRITTEN, F_CUT, F_OCCLUDED = 1, 2, 4, 8


@dataclasses.dataclass
class SnapshotUpdate:
    """One thumbnail a call wrote.  ``track``: index into the list the call was given (or into the tracker's own list)."""
    track_id: int
    slot: int
    score: int
    flags: int
    track: int
    stream: int = 0

    @property
    def new(self) -> bool:
        return bool(self.flags & F_NEW)


@dataclasses.dataclass
class SnapshotRetired:
    """One track that ended: where its thumbnail lies until the next call on its stream, and the best shot's record."""
    track_id: int
    slot: int
    best_frame: int
    xyxy: np.ndarray
    confidence: float
    class_id: int
    first_seen: int
    last_seen: int
    n_rewrites: int
    stream: int = 0


class _AtlasView(_ffi.DeviceBuffer):
    """A stream's atlas as the ``DeviceBuffer`` the frame modules take; the gallery owns the memory."""

    def __init__(self, ptr: int, nbytes: int, device: int):
        self.device, self.nbytes, self.ptr = device, nbytes, ptr

    def free(self):
        self.ptr = None


class SnapshotGallery(_ffi.Handle):
    """Best-shot thumbnails of ``thumb = (h, w)`` pixels for ``n_streams`` streams of at most ``max_tracks`` tracks each."""

    def __init__(self, thumb=(96, 96), *, n_streams: int = 1, max_tracks: int = 256, margin_pm: Optional[int] = None, min_side: Optional[int] = None,
                 area_cap: Optional[int] = None, occl_iou_pm: Optional[int] = None, min_gain_pm: Optional[int] = None, retire_after: Optional[int] = None,
                 pad_bgr: Optional[Sequence[int]] = None, classes: Optional[Iterable[int]] = None, max_updated: Optional[int] = None,
                 max_retired: Optional[int] = None, device=0, on_retired: Optional[Callable] = None) -> None:
        L = _ffi.lib()
        cfg = _ffi.SnapshotCfg()
        L.rtmodt_snapshot_default_cfg(C.byref(cfg))
        cfg.thumb_h, cfg.thumb_w = int(thumb[0]), int(thumb[1])
        for name, v in (("margin_pm", margin_pm), ("min_side", min_side), ("area_cap", area_cap), ("occl_iou_pm", occl_iou_pm), ("min_gain_pm", min_gain_pm),
                        ("retire_after", retire_after), ("max_updated", max_updated), ("max_retired", max_retired)):
            if v is not None:
                setattr(cfg, name, int(v))
        if pad_bgr is not None:
            for k in range(3):
                cfg.pad_bgr[k] = int(pad_bgr[k])
        cfg.device = _ffi.device_ordinal(device)
        self._classes = None if classes is None else np.ascontiguousarray(list(classes), np.int32)
        if self._classes is not None:
            cfg.n_classes = len(self._classes)
            cfg.classes = self._classes.ctypes.data_as(C.POINTER(C.c_int32))
        self.cfg, self.n_streams, self.max_tracks = cfg, int(n_streams), int(max_tracks)
        self.thumb = (cfg.thumb_h, cfg.thumb_w)
        self.on_retired = on_retired
        self.updated: list = []          # of the last call
        self.retired: list = []
        self.n_rewritten = 0             # thumbnails of existing rows the last call replaced (all streams)
        self._slot_of: list = [dict() for _ in range(self.n_streams)]         # track id -> slot of the rows this object saw being written
        self._gone: list = [dict() for _ in range(self.n_streams)]            # ... of the rows the last call on the stream retired
        h = C.c_void_p()
        _ffi.check(L.rtmodt_snapshot_create(C.byref(cfg), self.n_streams, self.max_tracks, C.byref(h)))
        self._h = h
        self._upd = (_ffi.SnapshotUpdate * (self.n_streams * cfg.max_updated))()
        self._ret = (_ffi.SnapshotRetired * (self.n_streams * cfg.max_retired))()
        self._cnt = np.zeros((3, self.n_streams), np.int32)
        self._out = _ffi.SnapshotOut(C.addressof(self._upd), self._cnt[0].ctypes.data, C.addressof(self._ret), self._cnt[1].ctypes.data,
                                     self._cnt[2].ctypes.data)

    # ---- per frame -----------------------------------------------------------------------------------------------------
    def process(self, tracks, frame: np.ndarray, frame_id: int, stream: int = 0):
        """One stream: ``tracks`` is a list of objects with ``track_id`` / ``xyxy`` / ``class_id`` (and ``confidence``, when they have
        one) or a tuple ``(ids, xyxy[, conf], cls)``; ``frame`` an ``(h, w, 3)`` uint8 array.  Returns ``(updated, retired)``."""
        ids, xy, cf, cl = self._lists(tracks)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames([frame], 1, writable=False)
        rc = _ffi.lib().rtmodt_snapshot_process(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(xy), _ffi.ptr(cf), _ffi.ptr(cl), len(ids), C.c_void_p(ptrs[0]),
                                                h, w, st, mem, int(frame_id), C.byref(self._out))
        return self._collect(rc, [int(stream)], flat=True)

    def process_tracker(self, tracker, frames, frame_ids, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                        offset: int = 0):
        """Every stream of ``tracker`` straight on its device-resident state: the tracks the crossing counter's ``process_tracker``
        passes.  ``frames``: one per stream (host arrays or a ``DeviceBuffer``); ``frame_ids``: one per stream, or one for all.
        Dispatches on the tracker class; returns ``(updated, retired)``.  The gallery must hold at least the tracker's streams and
        ``max_tracks`` (a ``MultiObjectTracker`` holds 2048 by default): ``ValueError`` otherwise."""
        core, suffix, tsu = resolve_tracker(tracker, "process_tracker", "as a list: process(tracks, frame, frame_id)")
        n = core.n_streams
        if n > self.n_streams or core.max_tracks > self.max_tracks:
            raise ValueError(f"the tracker holds {n} stream(s) of up to {core.max_tracks} tracks, this gallery {self.n_streams} of {self.max_tracks}: "
                             f"make it with SnapshotGallery(n_streams={n}, max_tracks={core.max_tracks})")
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset, writable=False)
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        fid = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_ids, np.int64), (n,)))
        rc = getattr(_ffi.lib(), f"rtmodt_snapshot_process_{suffix}")(self._h, core._h, fp, h, w, st, mem, _ffi.ptr(fid), *tsu, C.byref(self._out))
        return self._collect(rc, list(range(n)), flat=False)

    # ---- reading -------------------------------------------------------------------------------------------------------
    def thumbnail(self, track_id: int, stream: int = 0) -> np.ndarray:
        """The kept thumbnail of a live (or just retired) track as an ``(h, w, 3)`` uint8 array."""
        return self.read([self._slots([track_id], stream)[0]], stream)[0]

    def read(self, slots, stream: int = 0) -> np.ndarray:
        """``(len(slots), h, w, 3)`` uint8: the thumbnails in ``slots``."""
        s = np.ascontiguousarray(slots, np.int32)
        out = np.empty((len(s), self.thumb[0], self.thumb[1], 3), np.uint8)
        _ffi.check(_ffi.lib().rtmodt_snapshot_read(self._h, int(stream), _ffi.ptr(s), len(s), _ffi.ptr(out)))
        return out

    def atlas(self, stream: int = 0):
        """``(DeviceBuffer view, slot_bytes, pitch)`` of one stream's atlas: slot s lies at ``s * slot_bytes``."""
        p, sb, pitch = C.c_void_p(), C.c_size_t(0), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_snapshot_atlas(self._h, int(stream), C.byref(p), C.byref(sb), C.byref(pitch)))
        return _AtlasView(p.value, sb.value * 2 * self.max_tracks, self.cfg.device), sb.value, pitch.value

    def jpeg(self, track_ids_or_slots, encoder, stream: int = 0, slots: bool = False) -> list:
        """JPEG files of thumbnails, encoded by ``encoder`` (a ``JpegEncoder``) on the atlas where it lies.  ``slots``: the first
        argument holds slot numbers, else track ids of live or just retired rows."""
        want = [int(v) for v in track_ids_or_slots]
        if not slots:
            want = self._slots(want, stream)
        view, sb, pitch = self.atlas(stream)
        return [encoder.encode_batch(view, height=self.thumb[0], width=self.thumb[1], stride=pitch, offset=s * sb, count=1)[0] for s in want]

    def snapshot(self, stream: int = 0) -> dict:
        """The ledger of one stream in ascending track id, and the slot bitmap."""
        cap = 2 * self.max_tracks
        ids, sc, bf, fs, ls = (np.zeros(cap, np.int64) for _ in range(5))
        xy, cf, ints, bm, n = np.zeros((cap, 4), np.float32), np.zeros(cap, np.float32), np.zeros((cap, 4), np.int32), np.zeros((cap + 31) // 32, np.uint32), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_snapshot_state(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(sc), _ffi.ptr(bf), _ffi.ptr(fs), _ffi.ptr(ls), _ffi.ptr(xy),
                                                   _ffi.ptr(cf), _ffi.ptr(ints), _ffi.ptr(bm), C.byref(n)))
        rows = [dict(track_id=int(ids[i]), slot=int(ints[i, 0]), best_score=int(sc[i]), best_frame=int(bf[i]), xyxy=xy[i].copy(), conf=cf[i],
                     cls=int(ints[i, 1]), first_seen=int(fs[i]), last_seen=int(ls[i]), n_rewrites=int(ints[i, 2]), flags=int(ints[i, 3])) for i in range(n.value)]
        return {"rows": rows, "bitmap": bm}

    # ---- stateless crops ----------------------------------------------------------------------------------------------
    def crop(self, frames, boxes, frame_index=None, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
             offset: int = 0):
        """Thumbnails of ``boxes`` (``(n, 4)`` xyxy) without a ledger: box i is cut from ``frames[frame_index[i]]`` (default frame 0).
        Returns ``(thumbnails (n, h, w, 3), sampled (n,) bool)``; the thumbnail of a box that is not sampled is zero."""
        xy = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        fi = np.zeros(len(xy), np.int32) if frame_index is None else np.ascontiguousarray(frame_index, np.int32)
        ptrs, h, w, st, mem, n = _ffi.batch_frames(frames, None, height=height, width=width, stride=stride, offset=offset, writable=False)
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        out = np.zeros((len(xy), self.thumb[0], self.thumb[1], 3), np.uint8)
        ok = np.zeros(len(xy), np.int32)
        _ffi.check(_ffi.lib().rtmodt_snapshot_crop(self._h, fp, n, h, w, st, mem, _ffi.ptr(xy), _ffi.ptr(fi), len(xy), _ffi.ptr(out), _ffi.MEM_HOST, _ffi.ptr(ok)))
        return out, ok.astype(bool)

    def crop_detector(self, detector, frames, conf_lo: float, conf_hi: float, max_out: Optional[int] = None, *, height: Optional[int] = None,
                      width: Optional[int] = None, stride: Optional[int] = None, offset: int = 0, count: Optional[int] = None):
        """The review queue (low-confidence detections for a human to label): thumbnails of the detections of ``detector``'s newest batch
        with ``conf_lo <= confidence < conf_hi``, at most ``max_out`` per frame (default: the detector's ``max_det``), in the detector's
        order.  The detections are read from the detector's device-resident outputs: no box crosses to the host.  ``frames``: the
        frames of that batch (host arrays or a ``DeviceBuffer``).  Returns one ``(thumbnails (k, h, w, 3), detection indices (k,),
        sampled (k,) bool)`` triple per frame; the thumbnail of a box that is not sampled is zero."""
        model = getattr(detector, "model", detector)
        n = int(count) if count is not None else (None if isinstance(frames, _ffi.DeviceBuffer) else len(frames))
        ptrs, h, w, st, mem, n = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset, writable=False)
        m = int(max_out) if max_out is not None else int(getattr(detector, "max_det", None) or model.max_det)
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        out = np.zeros((n, m, self.thumb[0], self.thumb[1], 3), np.uint8)
        index, ok, cnt = np.full((n, m), -1, np.int32), np.zeros((n, m), np.int32), np.zeros(n, np.int32)
        _ffi.check(_ffi.lib().rtmodt_snapshot_crop_detector(self._h, model.handle, fp, n, h, w, st, mem, float(conf_lo), float(conf_hi), m, _ffi.ptr(out),
                                                            _ffi.MEM_HOST, _ffi.ptr(index), _ffi.ptr(cnt), _ffi.ptr(ok)))
        return [(out[i, :cnt[i]], index[i, :cnt[i]], ok[i, :cnt[i]].astype(bool)) for i in range(n)]

    # ---- housekeeping ---------------------------------------------------------------------------------------------------
    def reset(self, stream: Optional[int] = None) -> None:
        """Empties the ledger of one stream (default: of every stream)."""
        for s in range(self.n_streams) if stream is None else [int(stream)]:
            _ffi.check(_ffi.lib().rtmodt_snapshot_reset(self._h, s))
            self._slot_of[s].clear()

    def last_kernel_ms(self) -> float:
        """Device time of the last call's launches (HIP events)."""
        return _ffi.last_ms("rtmodt_snapshot_last_ms", self._h)

    _destroy = "rtmodt_snapshot_destroy"

    # ---- internals -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _lists(tracks):
        if isinstance(tracks, tuple) and len(tracks) in (3, 4):
            ids, xy = tracks[0], tracks[1]
            cf, cl = (tracks[2], tracks[3]) if len(tracks) == 4 else (None, tracks[2])
        else:
            tracks = list(tracks)
            ids = [t.track_id for t in tracks]
            xy = [np.asarray(t.xyxy, np.float32) for t in tracks]
            cl = [t.class_id for t in tracks]
            cf = [t.confidence for t in tracks] if tracks and all(hasattr(t, "confidence") for t in tracks) else None
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 4)
        cl = np.ascontiguousarray(cl, np.int32).reshape(-1)
        cf = None if cf is None else np.ascontiguousarray(cf, np.float32).reshape(-1)
        return ids, xy, cf, cl

    def _slots(self, track_ids, stream: int) -> list:
        known = {**self._gone[stream], **self._slot_of[stream]}
        if any(int(t) not in known for t in track_ids):
            known.update({r["track_id"]: r["slot"] for r in self.snapshot(stream)["rows"]})
        missing = [int(t) for t in track_ids if int(t) not in known]
        if missing:
            raise KeyError(f"stream {stream} holds no thumbnail of track {missing[0]}")
        return [known[int(t)] for t in track_ids]

    def _collect(self, rc: int, streams, flat: bool):
        err = None if rc == _ffi.OK else _ffi.RtmodtError(rc, _ffi.lib().rtmodt_last_error().decode(errors="replace"))
        if err is not None and rc != _ffi.E_CAPACITY:
            raise err
        self.updated, self.retired, self.n_rewritten = [], [], 0
        for s in streams:
            d = 0 if flat else s
            known = self._slot_of[s]
            self._gone[s] = {}
            for k in range(int(self._cnt[0, d])):
                u = self._upd[d * self.cfg.max_updated + k]
                self.updated.append(SnapshotUpdate(u.track_id, u.slot, u.score, u.flags, u.track, s))
                known[u.track_id] = u.slot
            for k in range(int(self._cnt[1, d])):
                r = self._ret[d * self.cfg.max_retired + k]
                self.retired.append(SnapshotRetired(r.track_id, r.slot, r.best_frame, np.array(r.xyxy, np.float32), float(r.conf), r.cls, r.first_seen,
                                                    r.last_seen, r.n_rewrites, s))
                if known.get(r.track_id) == r.slot:
                    del known[r.track_id]
                self._gone[s][r.track_id] = r.slot                                   # readable until the next call on the stream
            self.n_rewritten += int(self._cnt[2, d])
        if self.on_retired is not None:
            for r in self.retired:
                self.on_retired(self, r)
        if err is not None:
            raise err
        return self.updated, self.retired
