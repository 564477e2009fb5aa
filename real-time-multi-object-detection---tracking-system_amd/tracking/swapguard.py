"""ByteTrack identities verified by appearance; ID swaps reverted online on the native engine.

The reference's design document names ID switching as risk number 1 and prescribes two cures.  The offline one
(``correct_id_switches``, G.2) is ``evaluation.stitch_tracks``.  This is the online one, which the document asks for three times
and the reference never builds: B.4 "Re-Identification Considerations" (use appearance as a post-processing filter only on
suspected ID swaps; keep a feature buffer per track, the average colour histogram of the last 5 frames; when two tracks swap
within 3 frames, compare histograms and revert if similarity > 0.85), B.4's failure table ("add appearance verification") and
G.1 row 1 ("add lightweight appearance hash verification").

``IdSwapGuard`` keeps, per stream and track id, the last ``history`` colour-histogram descriptors the track showed while it
touched no other track, and remembers which id it last touched.  On the first frames after two tracks part, each track's
descriptor is compared with both histories; when each resembles the *other* id's history (``min_similarity_pm``) and more than
its own (``min_gain_pm``), the two ids are exchanged back.  The per-frame work -- descriptors, the pairwise contact test, the
ledger, the decisions and the exchange of the ids inside the tracker's device-resident state -- runs in ``csrc/swapguard.hip`` (a
fixed number of launches per frame for all streams); there is no CPU implementation here.  ``tests/swapguard_ref.py`` states the
rules; DESIGN.md section 19 lists them, the parameters this project added (``min_history``, ``min_gain_pm``, ``contact_iou``) and
the known limits.  No default has been validated on real footage.

Two ways in: ``process(tracks, frame, frame_id)`` on a host list (the caller adopts the returned ids) and
``process_tracker(tracker, frames, frame_id)`` straight on a ``MultiObjectTracker`` / ``_ByteTrackCore``, whose ids are corrected
in place so that the zone engine, the crossing counter and the renderer read the corrected identity from that frame on.
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from typing import Sequence

import numpy as np

from .. import _ffi

log = logging.getLogger("rtmodt.tracker")

DIM = 192


@dataclass
class SwapEvent:
    """One reverted ID swap.  ``track_a`` < ``track_b`` index the list that was handed over; ``id_a`` / ``id_b`` are their ids
    before the exchange; ``similarities`` (per mille): a's descriptor against the history of ``id_a`` and of ``id_b``, then b's
    against ``id_b``'s and ``id_a``'s."""
    frame_id: int
    track_a: int
    track_b: int
    id_a: int
    id_b: int
    similarities: tuple
    stream: int = 0


class IdSwapGuard(_ffi.Handle):
    """Reverts ByteTrack ID swaps by appearance; ledgers live on the device, one per stream."""

    def __init__(self, *, history: int = 5, min_history: int = 3, window: int = 3, min_similarity: float = 0.85, min_gain_pm: int = 1,
                 contact_iou: float = 0.0, max_gap_frames: int = 30, max_tracks: int = 256, n_streams: int = 1, max_events: int = 64, device=0) -> None:
        self.history, self.min_history, self.window = int(history), int(min_history), int(window)
        self.min_similarity_pm, self.min_gain_pm = int(round(float(min_similarity) * 1000)), int(min_gain_pm)
        self.contact_iou, self.max_gap_frames = float(contact_iou), int(max_gap_frames)
        self.max_tracks, self.n_streams, self.max_events = int(max_tracks), int(n_streams), int(max_events)
        self._device = _ffi.device_ordinal(device)
        cfg = _ffi.SwapGuardCfg(self.history, self.min_history, self.window, self.min_similarity_pm, self.min_gain_pm, self.contact_iou,
                                self.max_gap_frames, self.max_tracks, self.n_streams, self.max_events, self._device)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_swapguard_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._ev = (_ffi.SwapEventRec * (self.n_streams * self.max_events))()
        self._n = np.zeros(self.n_streams, np.int32)
        #: the events of the most recent call, one list per stream -- also when that call raised E_CAPACITY
        self.last_events = [[] for _ in range(self.n_streams)]

    # ------------------------------------------------------------------ per frame
    def process(self, tracks: Sequence, frame, frame_id: int, *, stream: int = 0, height: int = 0, width: int = 0, stride: int = 0,
                mem_kind: int = _ffi.MEM_HOST):
        """One stream, a list duck-typed on ``track_id / xyxy``; ``frame`` is the BGR frame the detector read (an ``(h, w, 3)``
        uint8 array, or a device address with ``height`` / ``width`` / ``stride`` and ``mem_kind=MEM_DEVICE``).  Returns
        ``(ids, events)``: the ids after the reverts, in list order -- the caller's tracker must adopt them, otherwise the same
        pair is reverted again while the window lasts."""
        n = len(tracks)
        ids = np.fromiter((int(t.track_id) for t in tracks), np.int64, n)
        xyxy = np.ascontiguousarray([np.asarray(t.xyxy, np.float32) for t in tracks], np.float32).reshape(n, 4)
        return self.process_arrays(ids, xyxy, frame, frame_id, stream=stream, height=height, width=width, stride=stride, mem_kind=mem_kind)

    def process_arrays(self, ids, xyxy, frame, frame_id: int, *, stream: int = 0, height: int = 0, width: int = 0, stride: int = 0,
                       mem_kind: int = _ffi.MEM_HOST):
        """:meth:`process` on arrays: ``ids`` (n,) int64, ``xyxy`` (n, 4) float32."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        n = len(ids)
        xyxy = np.ascontiguousarray(xyxy, np.float32).reshape(n, 4)
        fp, keep, height, width, stride = _ffi.frame_pointers([frame], mem_kind, height, width, stride)
        out = np.empty(n, np.int64)
        ne = C.c_int32(0)
        rc = _ffi.lib().rtmodt_swapguard_process(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(xyxy), n, C.c_void_p(fp[0]), height, width, stride,
                                                 int(mem_kind), int(frame_id), _ffi.ptr(out), C.cast(self._ev, C.c_void_p), C.byref(ne))
        del keep
        events = [self._emit(self._ev[e], int(stream)) for e in range(ne.value)] if rc in (_ffi.OK, _ffi.E_CAPACITY) else []
        self.last_events = [events]
        _ffi.check(rc)
        return out, events

    def process_tracker(self, tracker, frames, frame_id: int, *, height: int = 0, width: int = 0, stride: int = 0, mem_kind: int = _ffi.MEM_HOST) -> list:
        """All streams of a ByteTrack ``tracker`` at once, on its device-resident state: ``frames[s]`` is the frame stream ``s``'s
        detections were read from.  Passed tracks are the ones ``tracker.report`` names (``"matched"``: matched or spawned this
        frame).  A revert exchanges the two ids inside the tracker's state.  Returns one event list per stream."""
        from .tracker import _ByteTrackCore
        core = getattr(tracker, "_core", tracker)
        if not isinstance(core, _ByteTrackCore):
            raise TypeError(f"process_tracker corrects the device-resident state of the ByteTrack tracker; hand the tracks of a "
                            f"{type(tracker).__name__} over as a list: process(tracks, frame, frame_id)")
        if isinstance(frames, np.ndarray) and frames.ndim == 3:
            frames = [frames]
        if len(frames) != core.n_streams:
            raise ValueError(f"{len(frames)} frames for a tracker of {core.n_streams} streams")
        fp, keep, height, width, stride = _ffi.frame_pointers(list(frames), mem_kind, height, width, stride)
        report = getattr(tracker, "report", "matched")
        rc = _ffi.lib().rtmodt_swapguard_process_tracker(self._h, core._h, fp, height, width, stride, int(mem_kind), int(frame_id),
                                                         1 if report == "matched" else 0, C.cast(self._ev, C.c_void_p), _ffi.ptr(self._n))
        del keep
        out = []
        if rc in (_ffi.OK, _ffi.E_CAPACITY):
            out = [[self._emit(self._ev[s * self.max_events + e], s) for e in range(int(self._n[s]))] for s in range(core.n_streams)]
        self.last_events = out
        _ffi.check(rc)
        return out

    # ------------------------------------------------------------------ state
    def state(self, stream: int = 0) -> list:
        """The ledger in the restatement's canonical form (``tests/swapguard_ref.py``: ``SwapGuardRef.snapshot``), rows in
        ascending id: ``[id, last frame, count, contact frame, contact id, the ring's bytes oldest first]``."""
        cap = 2 * self.max_tracks
        ids, last, cframe, cid = (np.empty(cap, np.int64) for _ in range(4))
        count = np.empty(cap, np.int32)
        ring = np.empty((cap, self.history, DIM), np.int8)
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_swapguard_state(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(last), _ffi.ptr(count), _ffi.ptr(cframe),
                                                     _ffi.ptr(cid), _ffi.ptr(ring), C.byref(n)))
        return [[int(ids[r]), int(last[r]), int(count[r]), int(cframe[r]), int(cid[r]), ring[r, :count[r]].tobytes()] for r in range(n.value)]

    def reverted(self, stream: int = 0) -> int:
        """Swaps reverted on ``stream`` since creation."""
        v = C.c_int64(0)
        _ffi.check(_ffi.lib().rtmodt_swapguard_counts(self._h, int(stream), C.byref(v)))
        return int(v.value)

    def last_ms(self) -> dict:
        """Device time of the last call: ``describe`` (the descriptor launches) and ``step`` (gather + decision kernel)."""
        d, s = _ffi.last_ms("rtmodt_swapguard_last_ms", self._h, 2)
        return {"describe": d, "step": s}

    _destroy = "rtmodt_swapguard_destroy"

    @staticmethod
    def _emit(r, stream) -> SwapEvent:
        evt = SwapEvent(frame_id=int(r.frame_id), track_a=int(r.track_a), track_b=int(r.track_b), id_a=int(r.id_a), id_b=int(r.id_b),
                        similarities=tuple(int(v) for v in r.sims), stream=stream)
        log.info("ID swap reverted: stream %d frame %d ids %d <-> %d (similarities %s)", stream, evt.frame_id, evt.id_a, evt.id_b, evt.similarities)
        return evt


def adopt(tracks: Sequence, events: Sequence) -> None:
    """Exchanges the ids of an already materialised track list (objects with ``track_id``) the way ``events`` exchanged them in
    the tracker's state."""
    for e in events:
        for t in tracks:
            if t.track_id == e.id_a:
                t.track_id = e.id_b
            elif t.track_id == e.id_b:
                t.track_id = e.id_a
