"""What the DeepSORT and OC-SORT front ends share: the padding of one frame's detections to a single-stream batch, and the trails."""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from .. import _ffi


def resolve_tracker(tracker, method=None, hint=""):
    """A tracker front end or core -> ``(core, suffix, tsu)``.  ``suffix`` ends the C symbol that reads that tracker's device-resident
    state (``rtmodt_<module>_<verb>_<suffix>``: ``tracker`` is ByteTrack) and ``tsu`` is the ``report_tsu`` argument that symbol takes,
    as a tuple to splice in: ByteTrack passes the tracks ``tracker.report`` names, DeepSORT its confirmed tracks matched this frame,
    the other two take none.  Anything else raises ``TypeError`` in the words of the caller's ``method`` with its ``hint`` of the list
    form; without a ``method`` the suffix is ``None`` and the caller refuses it itself."""
    from .botsort import _BotSortCore
    from .deepsort import _DeepSortCore
    from .ocsort import _OcSortCore
    from .tracker import _ByteTrackCore
    core = getattr(tracker, "_core", tracker)
    if isinstance(core, _ByteTrackCore):
        return core, "tracker", (1 if getattr(tracker, "report", "matched") == "matched" else 0,)
    if isinstance(core, _DeepSortCore):
        return core, "deepsort", (0,)
    if isinstance(core, _OcSortCore):
        return core, "ocsort", ()
    if isinstance(core, _BotSortCore):
        return core, "botsort", ()
    if method is None:
        return core, None, ()
    raise TypeError(f"{method} reads the device-resident state of the ByteTrack, the DeepSORT, the OC-SORT or the BoT-SORT tracker; hand the tracks of a "
                    f"{type(tracker).__name__} over {hint}")


def pad_single_stream(xyxy, confidence, class_id, max_dets: int):
    """One frame's detections as the ``[1, max_dets(, 4)]`` arrays ``update_batch`` takes: ``(bx, cf, cl, n)``."""
    xyxy = np.asarray(xyxy, np.float32).reshape(-1, 4)
    n = len(xyxy)
    if n > max_dets:
        raise _ffi.RtmodtError(_ffi.E_CAPACITY, f"{n} detections > max_dets {max_dets}")
    bx = np.zeros((1, max_dets, 4), np.float32); bx[0, :n] = xyxy
    cf = np.zeros((1, max_dets), np.float32); cf[0, :n] = np.asarray(confidence, np.float32).reshape(-1)
    cl = np.zeros((1, max_dets), np.int32); cl[0, :n] = np.asarray(class_id, np.int32).reshape(-1)
    return bx, cf, cl, n


class TrailKeeper:
    """The last ``maxlen`` centroids of every live track, as ``MultiObjectTracker`` draws them."""

    def __init__(self, maxlen: int = 30) -> None:
        self._map = defaultdict(list)
        self._maxlen = maxlen

    def drop_dead(self, ids) -> None:
        """ids are never reused: a dead track's trail is dead weight"""
        alive = set(int(i) for i in ids)
        for tid in [t for t in self._map if t not in alive]:
            del self._map[tid]

    def push(self, tid: int, b) -> list:
        """Appends the centroid of box ``b`` (float32 arithmetic, truncation) to ``tid``'s trail; returns a copy of the trail."""
        trail = self._map[tid]
        trail.append((int((b[0] + b[2]) / 2), int((b[1] + b[3]) / 2)))
        if len(trail) > self._maxlen:
            trail.pop(0)
        return list(trail)
