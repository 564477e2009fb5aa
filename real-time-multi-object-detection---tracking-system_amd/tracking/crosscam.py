"""Tracks linked across cameras to site-wide identities on the native engine.

Every tracker here numbers its tracks from 1 per stream, and the zone engine, the crossing counter, the speed estimator and the
snapshot gallery key on ``(stream, track_id)``: a person who walks from camera 0 into camera 3 is two unrelated objects to all of
them.  ``CrossCameraLinker`` keeps a device-resident table of site-wide identities (``gid`` from 1, never reused) and, per stream,
a ledger that binds local track ids to them, both updated once per frame set by ``csrc/crosscam.hip`` in a fixed number of launches
for all streams; there is no CPU implementation here.  The reference has no counterpart -- its ``Track`` has no global id and its
tracker sees one source.  ``tests/crosscam_ref.py`` restates the rules, DESIGN.md section 33 lists them with the choices this project
made.  No default (``min_similarity`` least of all) has been validated on real footage, and parity with a published multi-camera
tracker is unpinned: none is installed where this runs.

Three ways in: ``process(lists)`` on host lists ``(ids, classes, rows)`` per stream (ByteTrack and OC-SORT carry no descriptors and
enter this way, with rows of the caller's; float embeddings are quantised with ``quantize``), and ``process_tracker(tracker)``
straight on the device-resident state of a ``BotSortTracker`` or ``DeepSortTracker``, queued behind its last update.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _ffi
from ._common import resolve_tracker

NONE, BOUND, LINKED, JOINED, BORN, NO_DESCRIPTOR, DEFERRED, TABLE_FULL, UNBOUND = range(9)
STATUS_NAMES = ("none", "bound", "linked", "joined", "born", "no_descriptor", "deferred", "table_full", "unbound")
COUNTERS = ("call", "n_identities", "next_gid", "n_queries", "n_deferred", "n_table_full", "n_events", "n_retired")


@dataclass
class HandoffEvent:
    """A track taken over by an existing identity: ``local_id`` of ``stream`` is ``gid``, last seen in ``from_stream`` ``gap`` calls
    ago (0: in this very call, an overlapping view); ``sim`` per mille."""
    gid: int
    stream: int
    local_id: int
    from_stream: int
    gap: int
    sim: int


@dataclass
class RetiredIdentity:
    gid: int
    first_seen: int
    last_seen: int
    streams: tuple


@dataclass
class LinkResult:
    """Per stream and entry, in the order handed over: ``gid`` (0 none), ``status`` and ``sim``; the call's events, retired identities
    and counters."""
    gid: list
    status: list
    sim: list
    events: list
    retired: list
    counters: dict


def quantize(rows) -> np.ndarray:
    """Float embedding rows -> the int8 rows the linker takes (``rtmodt_appearance_quantize``)."""
    x = np.ascontiguousarray(rows, np.float32)
    x = x.reshape(-1, x.shape[-1])
    out = np.zeros(x.shape, np.int8)
    _ffi.check(_ffi.lib().rtmodt_appearance_quantize(_ffi.ptr(x), x.shape[0], x.shape[1], _ffi.ptr(out)))
    return out


def similarity(q, t, device=0):
    """The linker's GEMM alone: ``(dots, sim)`` of int8 rows ``q`` (nq, dim) against ``t`` (nt, dim), both int32 (nq, nt)."""
    q, t = np.ascontiguousarray(q, np.int8), np.ascontiguousarray(t, np.int8)
    dots, sim = np.zeros((len(q), len(t)), np.int32), np.zeros((len(q), len(t)), np.int32)
    dim = q.shape[1] if q.ndim == 2 else 0
    _ffi.check(_ffi.lib().rtmodt_crosscam_similarity(_ffi.device_ordinal(device), _ffi.ptr(q), len(q), _ffi.ptr(t), len(t), int(dim), _ffi.ptr(dots),
                                                     _ffi.ptr(sim)))
    return dots, sim


class CrossCameraLinker(_ffi.Handle):
    """Site-wide identities over ``n_streams`` cameras; the table and the ledgers live on the device."""

    def __init__(self, n_streams: int, dim: int, *, max_tracks: int = 256, max_identities: int = 4096, max_queries: int = 1024,
                 min_similarity: float = 0.7, max_age: int = 9000, bind_age: int | None = None, match_class: bool = True, device=0) -> None:
        self.n_streams, self.dim, self.max_tracks = int(n_streams), int(dim), int(max_tracks)
        self.max_identities, self.max_queries = int(max_identities), int(max_queries)
        self.min_sim_milli, self.max_age = int(round(float(min_similarity) * 1000)), int(max_age)
        self.bind_age, self.match_class = self.max_age if bind_age is None else int(bind_age), bool(match_class)
        self._device = _ffi.device_ordinal(device)
        cfg = _ffi.CrossCamCfg(self._device, self.n_streams, self.dim, self.max_tracks, self.max_identities, self.max_queries, self.min_sim_milli,
                               self.max_age, self.bind_age, 1 if self.match_class else 0)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_crosscam_create(C.byref(cfg), C.byref(h)))
        self._h = h
        S, M = self.n_streams, self.max_tracks
        self._gid, self._status, self._sim = np.zeros((S, M), np.int64), np.zeros((S, M), np.int32), np.zeros((S, M), np.int32)
        self._ev = (_ffi.CrossCamEventRec * (S * M))()
        self._ret = (_ffi.CrossCamRetiredRec * self.max_identities)()
        self._counters = np.zeros(8, np.int64)
        self._bound = [dict() for _ in range(S)]           # local id -> gid, read back from the ledgers when a call has changed them
        self._stale = False
        #: the hand-off events and the retired identities of the most recent call
        self.last_events: list = []
        self.last_retired: list = []

    # ------------------------------------------------------------------ configuration
    def set_transit(self, src: int, dst: int, min_calls: int, max_calls: int) -> None:
        """The camera topology, one ordered pair: a person last seen in ``src`` may appear in ``dst`` ``min_calls`` to
        ``max_calls`` calls later.  0 for overlapping views, > 0 for disjoint ones, ``max_calls < min_calls``: cannot get there."""
        _ffi.check(_ffi.lib().rtmodt_crosscam_set_transit(self._h, int(src), int(dst), int(min_calls), int(max_calls)))

    # ------------------------------------------------------------------ per frame set
    def _out(self):
        ne, nr = C.c_int32(0), C.c_int32(0)
        out = _ffi.CrossCamOut(_ffi.ptr(self._gid), _ffi.ptr(self._status), _ffi.ptr(self._sim), C.cast(self._ev, C.c_void_p), C.pointer(ne),
                               C.cast(self._ret, C.c_void_p), C.pointer(nr), _ffi.ptr(self._counters))
        return out, ne, nr

    def _result(self, counts, ne, nr) -> LinkResult:
        S = self.n_streams
        self.last_events = [HandoffEvent(int(e.gid), int(e.stream), int(e.local_id), int(e.from_stream), int(e.gap), int(e.sim))
                            for e in (self._ev[i] for i in range(ne.value))]
        self.last_retired = [RetiredIdentity(int(r.gid), int(r.first_seen), int(r.last_seen), tuple(s for s in range(S) if r.stream_mask >> s & 1))
                             for r in (self._ret[i] for i in range(nr.value))]
        self._stale = True
        return LinkResult([self._gid[s, :counts[s]].tolist() for s in range(S)], [self._status[s, :counts[s]].tolist() for s in range(S)],
                         [self._sim[s, :counts[s]].tolist() for s in range(S)], self.last_events, self.last_retired,
                         dict(zip(COUNTERS, (int(v) for v in self._counters))))

    def process(self, lists) -> LinkResult:
        """One call: ``lists[s] = (ids, classes, rows)`` of stream ``s`` -- local track ids (unique), class ids and int8 rows
        ``(n, dim)``; an empty stream is ``((), (), ())``."""
        S, D = self.n_streams, self.dim
        if len(lists) != S:
            raise ValueError(f"{len(lists)} lists for {S} streams")
        counts = np.asarray([len(np.asarray(l[0]).reshape(-1)) for l in lists], np.int32)
        stride = max(1, int(counts.max()))
        ids, cls, rows = np.zeros((S, stride), np.int64), np.zeros((S, stride), np.int32), np.zeros((S, stride, D), np.int8)
        for s, (i, k, r) in enumerate(lists):
            n = counts[s]
            if n:
                ids[s, :n], cls[s, :n] = np.asarray(i, np.int64).reshape(-1), np.asarray(k, np.int32).reshape(-1)
                rows[s, :n] = np.asarray(r, np.int8).reshape(n, D)
        out, ne, nr = self._out()
        _ffi.check(_ffi.lib().rtmodt_crosscam_process(self._h, _ffi.ptr(ids), _ffi.ptr(cls), _ffi.ptr(rows), _ffi.ptr(counts), stride, C.byref(out)))
        return self._result(counts, ne, nr)

    def process_tracker(self, tracker) -> LinkResult:
        """One call on the device-resident state of a ``BotSortTracker`` (tracked tracks matched this frame, each with its smoothed
        feature) or a ``DeepSortTracker`` (confirmed tracks matched this frame, each with the newest row of its gallery), queued on
        the HIP stream its last update ran on.  The entries come in the tracker's list order; ``global_id`` resolves them."""
        core, suffix, _ = resolve_tracker(tracker)
        if suffix not in ("botsort", "deepsort"):
            raise TypeError(f"{type(tracker).__name__} carries no descriptors on the device; hand its tracks over as lists: process(lists)")
        out, ne, nr = self._out()
        _ffi.check(getattr(_ffi.lib(), f"rtmodt_crosscam_process_{suffix}")(self._h, core._h, C.byref(out)))
        counts = [int(np.count_nonzero(self._status[s])) for s in range(self.n_streams)]
        return self._result(counts, ne, nr)

    # ------------------------------------------------------------------ look-up
    def global_id(self, track_id: int, stream: int = 0) -> int:
        """The site-wide id the local ``track_id`` of ``stream`` was bound to in the calls so far (0: none)."""
        if self._stale:
            self._bound = [{int(l): int(g) for l, g, _ in led} for led in self._ledgers()]
            self._stale = False
        return self._bound[int(stream)].get(int(track_id), 0)

    def label(self, track_id: int, stream: int = 0) -> str:
        """``"G17"`` for ``FrameRenderer`` labels; the empty string while the track has no identity."""
        g = self.global_id(track_id, stream)
        return f"G{g}" if g else ""

    # ------------------------------------------------------------------ state
    def _ledgers(self) -> list:
        S, I = self.n_streams, self.max_identities
        hdr, nb = np.zeros(3, np.int64), np.zeros(S, np.int32)
        bl, bg, bt = (np.zeros((S, I), np.int64) for _ in range(3))
        _ffi.check(_ffi.lib().rtmodt_crosscam_state(self._h, _ffi.ptr(hdr), None, None, None, None, None, None, _ffi.ptr(nb), _ffi.ptr(bl), _ffi.ptr(bg),
                                                    _ffi.ptr(bt)))
        return [np.stack([bl[s, :nb[s]], bg[s, :nb[s]], bt[s, :nb[s]]], 1) for s in range(S)]

    def snapshot(self) -> dict:
        """The whole table and every ledger (``tests/crosscam_ref.py``: ``CrossCamRef.snapshot``); ``load`` takes it back."""
        S, D, I = self.n_streams, self.dim, self.max_identities
        hdr = np.zeros(3, np.int64)
        gid, first, last = np.zeros(I, np.int64), np.zeros(I, np.int64), np.zeros((I, S), np.int64)
        cls, s16, s8 = np.zeros(I, np.int32), np.zeros((I, D), np.int16), np.zeros((I, D), np.int8)
        nb = np.zeros(S, np.int32)
        bl, bg, bt = (np.zeros((S, I), np.int64) for _ in range(3))
        _ffi.check(_ffi.lib().rtmodt_crosscam_state(self._h, _ffi.ptr(hdr), _ffi.ptr(gid), _ffi.ptr(cls), _ffi.ptr(first), _ffi.ptr(last), _ffi.ptr(s16),
                                                    _ffi.ptr(s8), _ffi.ptr(nb), _ffi.ptr(bl), _ffi.ptr(bg), _ffi.ptr(bt)))
        n = int(hdr[2])
        return {"call": int(hdr[0]), "next_gid": int(hdr[1]), "gid": gid[:n].copy(), "cls": cls[:n].copy(), "first_seen": first[:n].copy(),
                "last_seen": last[:n].copy(), "s16": s16[:n].copy(), "s8": s8[:n].copy(),
                "ledgers": [np.stack([bl[s, :nb[s]], bg[s, :nb[s]], bt[s, :nb[s]]], 1) for s in range(S)]}

    def load(self, snap: dict) -> None:
        """Replaces the state by a ``snapshot()`` of a linker of the same ``n_streams``, ``dim`` and ``max_identities``: a restart
        keeps its identities."""
        S, D, I = self.n_streams, self.dim, self.max_identities
        n = len(snap["gid"])
        if n > I or len(snap["ledgers"]) != S:
            raise ValueError(f"snapshot of {n} identities / {len(snap['ledgers'])} streams for a linker of {I} / {S}")
        hdr = np.asarray([snap["call"], snap["next_gid"], n], np.int64)
        gid, first = np.ascontiguousarray(snap["gid"], np.int64), np.ascontiguousarray(snap["first_seen"], np.int64)
        last, cls = np.ascontiguousarray(snap["last_seen"], np.int64).reshape(n, S), np.ascontiguousarray(snap["cls"], np.int32)
        s16, s8 = np.ascontiguousarray(snap["s16"], np.int16).reshape(n, D), np.ascontiguousarray(snap["s8"], np.int8).reshape(n, D)
        nb = np.asarray([len(l) for l in snap["ledgers"]], np.int32)
        bl, bg, bt = (np.zeros((S, I), np.int64) for _ in range(3))
        for s, led in enumerate(snap["ledgers"]):
            led = np.asarray(led, np.int64).reshape(-1, 3)
            if len(led) > I:
                raise ValueError(f"stream {s}: {len(led)} bindings for a table of {I}")
            bl[s, :len(led)], bg[s, :len(led)], bt[s, :len(led)] = led[:, 0], led[:, 1], led[:, 2]
        _ffi.check(_ffi.lib().rtmodt_crosscam_load(self._h, _ffi.ptr(hdr), _ffi.ptr(gid), _ffi.ptr(cls), _ffi.ptr(first), _ffi.ptr(last), _ffi.ptr(s16),
                                                   _ffi.ptr(s8), _ffi.ptr(nb), _ffi.ptr(bl), _ffi.ptr(bg), _ffi.ptr(bt)))
        self._stale = True

    def errors(self) -> list:
        """The sticky error per stream: 0 none, 2 a matching past the solver's contested limits (that call's queries stayed unbound)."""
        err = np.zeros(self.n_streams, np.int32)
        _ffi.check(_ffi.lib().rtmodt_crosscam_errors(self._h, _ffi.ptr(err)))
        return err.tolist()

    def clear_errors(self) -> None:
        _ffi.check(_ffi.lib().rtmodt_crosscam_clear_errors(self._h))

    def last_ms(self) -> float:
        """Device time (ms) of the last call."""
        return _ffi.last_ms("rtmodt_crosscam_last_ms", self._h)

    _destroy = "rtmodt_crosscam_destroy"
