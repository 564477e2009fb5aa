"""What COLOUR a tracked object is, kept on MI355X: names an operator can type ("red top, dark trousers", "the white van").

The reference's ``Track`` and its alert record carry ``bbox_xyxy``, a class and a ``frame_id``.  ``ColourAttributes`` samples the
inside of every track's box on a bounded grid, names each sample with one of the 12 names of ``NAMES`` by an all-integer rule, and
accumulates the counts of the UPPER and the LOWER part of the box in a per-track ledger on the device; it answers the dominant
and the second name of each part and of the WHOLE with their shares per mille, for live tracks and for the tracks a call retired.
The work runs in ``csrc/colour.hip`` (rules in its header and in ``csrc/colour_rule.h``); there is no CPU implementation here --
labels are computed by the library.  ``tests/colour_ref.py`` restates the rules and the kernels equal it exactly.  Unpinned:
agreement of the names with human colour naming or with any product's; every default, validated on no real footage; white
balance, night and IR frames (grey everywhere is the honest answer there).
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Callable, Iterable, Optional

import numpy as np

from .. import _ffi
from ..tracking._common import resolve_tracker

NAMES = ("black", "grey", "white", "red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown")
PARTS = ("upper", "lower", "whole")
F_NEW, F_MANY_OCCLUDERS, F_THIN = 1, 2, 4

LABEL_DTYPE = np.dtype([("name", "<i4"), ("share_pm", "<i4"), ("second", "<i4"), ("second_pm", "<i4"), ("samples", "<i4")])
ROW_DTYPE = np.dtype([("track_id", "<i8"), ("first_frame", "<i8"), ("last_frame", "<i8"), ("hist", "<u4", (2, 12)), ("cls", "<i4"), ("frames_used", "<i4"),
                      ("flags", "<i4"), ("track", "<i4"), ("frame_samples", "<i4"), ("reserved", "<i4", (2,)), ("label", LABEL_DTYPE, (3,))])
assert ROW_DTYPE.itemsize == C.sizeof(_ffi.ColourRow) == 208

PartColour = collections.namedtuple("PartColour", "name share_pm second second_pm samples")
PartColour.__doc__ = "One part's label: ``name`` / ``second`` are colour names (``None``: no samples / no second colour), shares per mille."
TrackColours = collections.namedtuple("TrackColours", "upper lower whole")


def _name(i: int) -> Optional[str]:
    return NAMES[i] if 0 <= i < len(NAMES) else None


def colours_of(row) -> TrackColours:
    """``TrackColours`` of one row (an element of ``ROW_DTYPE``), read off the labels the library computed."""
    return TrackColours(*(PartColour(_name(int(l["name"])), int(l["share_pm"]), _name(int(l["second"])), int(l["second_pm"]), int(l["samples"])) for l in row["label"]))


def label_of(row) -> str:
    """``"red / blue"``: the dominant names of the upper and the lower part (``-``: no samples)."""
    c = colours_of(row)
    return f"{c.upper.name or '-'} / {c.lower.name or '-'}"


class ColourAttributes(_ffi.Handle):
    """Colour attributes for ``n_streams`` streams of at most ``max_tracks`` tracks each; every keyword that is ``None`` keeps the
    library's default (``rtmodt_colour_default_cfg``)."""

    def __init__(self, *, n_streams: int = 1, max_tracks: int = 256, inset_x_pm: Optional[int] = None, top_pm: Optional[int] = None,
                 split_pm: Optional[int] = None, bottom_pm: Optional[int] = None, max_side: Optional[int] = None, skip_occluded: Optional[bool] = None,
                 min_samples: Optional[int] = None, retire_after: Optional[int] = None, classes: Optional[Iterable[int]] = None, thresholds: Optional[dict] = None,
                 device=0, on_retired: Optional[Callable] = None) -> None:
        L = _ffi.lib()
        cfg = _ffi.ColourCfg()
        L.rtmodt_colour_default_cfg(C.byref(cfg))
        for name, v in (("inset_x_pm", inset_x_pm), ("top_pm", top_pm), ("split_pm", split_pm), ("bottom_pm", bottom_pm), ("max_side", max_side),
                        ("skip_occluded", skip_occluded), ("min_samples", min_samples), ("retire_after", retire_after)):
            if v is not None:
                setattr(cfg, name, int(v))
        for name, v in (thresholds or {}).items():           # the per-pixel constants by their cfg names; "hue": the eight bounds
            if name == "hue":
                for k in range(8):
                    cfg.hue[k] = int(v[k])
            elif name in ("black_max", "chroma_min", "sat_split", "sat_hi_pm", "sat_lo_pm", "y_black", "y_white", "pink_mx", "red_brown_mx", "orange_brown_mx",
                          "yellow_brown_mx"):
                setattr(cfg, name, int(v))
            else:
                raise ValueError(f"unknown threshold {name!r}")
        cfg.device = _ffi.device_ordinal(device)
        self._classes = None if classes is None else np.ascontiguousarray(list(classes), np.int32)
        if self._classes is not None:
            cfg.n_classes = len(self._classes)
            cfg.classes = self._classes.ctypes.data_as(C.POINTER(C.c_int32))
        self.cfg, self.n_streams, self.max_tracks = cfg, int(n_streams), int(max_tracks)
        self.on_retired = on_retired
        self.updated = np.zeros(0, ROW_DTYPE)        # of the last call: this call's members, in list order, streams behind one another
        self.retired = np.zeros(0, ROW_DTYPE)        # ... the rows it retired, with their final labels
        self.updated_stream = np.zeros(0, np.int32)  # the stream of each row of `updated` / `retired`
        self.retired_stream = np.zeros(0, np.int32)
        h = C.c_void_p()
        _ffi.check(L.rtmodt_colour_create(C.byref(cfg), self.n_streams, self.max_tracks, C.byref(h)))
        self._h = h
        self._upd = np.zeros((self.n_streams, self.max_tracks), ROW_DTYPE)
        self._ret = np.zeros((self.n_streams, 2 * self.max_tracks), ROW_DTYPE)
        self._cnt = np.zeros((2, self.n_streams), np.int32)
        self._out = _ffi.ColourOut(self._upd.ctypes.data, self._cnt[0].ctypes.data, self._ret.ctypes.data, self._cnt[1].ctypes.data)

    # ---- per frame -----------------------------------------------------------------------------------------------------
    def process(self, tracks, frame: np.ndarray, frame_id: int, stream: int = 0):
        """One stream: ``tracks`` is a list of objects with ``track_id`` / ``xyxy`` / ``class_id`` or a tuple ``(ids, xyxy, cls)``;
        ``frame`` an ``(h, w, 3)`` uint8 array.  Returns ``(updated, retired)``, arrays of ``ROW_DTYPE``."""
        ids, xy, cl = self._lists(tracks)
        ptrs, h, w, st, mem, _ = _ffi.batch_frames([frame], 1, writable=False)
        rc = _ffi.lib().rtmodt_colour_process(self._h, int(stream), _ffi.ptr(ids), _ffi.ptr(xy), _ffi.ptr(cl), len(ids), C.c_void_p(ptrs[0]), h, w, st, mem,
                                              int(frame_id), C.byref(self._out))
        return self._collect(rc, [int(stream)], flat=True)

    def process_batch(self, tracks_per_stream, frames, frame_ids, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                      offset: int = 0):
        """Every stream in one call: one track list (as ``process`` takes it) and one frame per stream."""
        n = self.n_streams
        lists = [self._lists(t) for t in tracks_per_stream]
        if len(lists) != n:
            raise ValueError(f"{len(lists)} track lists for {n} streams")
        m = max([len(l[0]) for l in lists] + [1])
        ids, xy, cl, cnt = np.zeros((n, m), np.int64), np.zeros((n, m, 4), np.float32), np.zeros((n, m), np.int32), np.zeros(n, np.int32)
        for s, (i, b, c) in enumerate(lists):
            cnt[s] = len(i)
            ids[s, :len(i)], xy[s, :len(i)], cl[s, :len(i)] = i, b, c
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset, writable=False)
        fp = (C.c_void_p * n)(*ptrs)
        fid = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_ids, np.int64), (n,)))
        rc = _ffi.lib().rtmodt_colour_process_batch(self._h, _ffi.ptr(ids), _ffi.ptr(xy), _ffi.ptr(cl), _ffi.ptr(cnt), m, fp, h, w, st, mem, _ffi.ptr(fid),
                                                    C.byref(self._out))
        return self._collect(rc, list(range(n)), flat=False)

    def process_tracker(self, tracker, frames, frame_ids, *, height: Optional[int] = None, width: Optional[int] = None, stride: Optional[int] = None,
                        offset: int = 0):
        """Every stream of ``tracker`` straight on its device-resident state: the tracks the snapshot gallery's ``process_tracker``
        passes.  ``frames``: one per stream (host arrays or a ``DeviceBuffer``); ``frame_ids``: one per stream, or one for all.
        Dispatches on the tracker class; returns ``(updated, retired)``.  This object must hold at least the tracker's streams and
        ``max_tracks`` (a ``MultiObjectTracker`` holds 2048 by default): ``ValueError`` otherwise."""
        core, suffix, tsu = resolve_tracker(tracker, "process_tracker", "as a list: process(tracks, frame, frame_id)")
        n = core.n_streams
        if n > self.n_streams or core.max_tracks > self.max_tracks:
            raise ValueError(f"the tracker holds {n} stream(s) of up to {core.max_tracks} tracks, this object {self.n_streams} of {self.max_tracks}: "
                             f"make it with ColourAttributes(n_streams={n}, max_tracks={core.max_tracks})")
        ptrs, h, w, st, mem, _ = _ffi.batch_frames(frames, n, height=height, width=width, stride=stride, offset=offset, writable=False)
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        fid = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_ids, np.int64), (n,)))
        rc = getattr(_ffi.lib(), f"rtmodt_colour_process_{suffix}")(self._h, core._h, fp, h, w, st, mem, _ffi.ptr(fid), *tsu, C.byref(self._out))
        return self._collect(rc, list(range(n)), flat=False)

    # ---- reading -------------------------------------------------------------------------------------------------------
    def state(self, stream: int = 0) -> np.ndarray:
        """The whole ledger of one stream in ascending track id, labels included (an array of ``ROW_DTYPE``)."""
        rows, n = np.zeros(2 * self.max_tracks, ROW_DTYPE), C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_colour_state(self._h, int(stream), _ffi.ptr(rows), C.byref(n)))
        return rows[:n.value].copy()

    def load_state(self, rows, stream: int = 0) -> None:
        """Replaces one stream's ledger by ``rows`` (what ``state`` returned, of this or another object)."""
        r = np.ascontiguousarray(rows, ROW_DTYPE)
        _ffi.check(_ffi.lib().rtmodt_colour_load(self._h, int(stream), _ffi.ptr(r), len(r)))

    def attributes(self, track_id: int, stream: int = 0) -> TrackColours:
        """``TrackColours(upper, lower, whole)`` of a live track, or of one the last call retired; ``KeyError`` otherwise."""
        return colours_of(self._row(track_id, stream))

    def label(self, track_id: int, stream: int = 0) -> str:
        """``"red / blue"``: upper / lower."""
        return label_of(self._row(track_id, stream))

    def find(self, part: str, name: str, min_share_pm: int = 500, stream: Optional[int] = None) -> list:
        """``(stream, track_id)`` of the live tracks whose ``part`` (``"upper"``, ``"lower"``, ``"whole"``) is dominated by ``name``
        with at least ``min_share_pm`` thousandths, over ``state()`` of one stream (default: of every stream)."""
        p, k = PARTS.index(part), NAMES.index(name)
        hits = []
        for s in range(self.n_streams) if stream is None else [int(stream)]:
            st = self.state(s)
            lab = st["label"][:, p] if len(st) else st["label"].reshape(0)
            hits += [(s, int(t)) for t in st["track_id"][(lab["name"] == k) & (lab["share_pm"] >= int(min_share_pm))]]
        return hits

    # ---- housekeeping ---------------------------------------------------------------------------------------------------
    def reset(self, stream: Optional[int] = None) -> None:
        """Empties the ledger of one stream (default: of every stream)."""
        for s in range(self.n_streams) if stream is None else [int(stream)]:
            _ffi.check(_ffi.lib().rtmodt_colour_reset(self._h, s))

    def last_kernel_ms(self) -> float:
        """Device time of the last call's two launches (HIP events)."""
        return _ffi.last_ms("rtmodt_colour_last_ms", self._h)

    _destroy = "rtmodt_colour_destroy"

    # ---- internals -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _lists(tracks):
        if isinstance(tracks, tuple) and len(tracks) == 3:
            ids, xy, cl = tracks
        else:
            tracks = list(tracks)
            ids = [t.track_id for t in tracks]
            xy = [np.asarray(t.xyxy, np.float32) for t in tracks]
            cl = [t.class_id for t in tracks]
        return (np.ascontiguousarray(ids, np.int64).reshape(-1), np.ascontiguousarray(xy, np.float32).reshape(-1, 4),
                np.ascontiguousarray(cl, np.int32).reshape(-1))

    def _row(self, track_id: int, stream: int):
        st = self.state(stream)
        k = np.searchsorted(st["track_id"], int(track_id))
        if k < len(st) and st["track_id"][k] == int(track_id):
            return st[k]
        gone = self.retired[(self.retired_stream == int(stream)) & (self.retired["track_id"] == int(track_id))]
        if len(gone):
            return gone[0]
        raise KeyError(f"stream {stream} holds no colours of track {track_id}")

    def _collect(self, rc: int, streams, flat: bool):
        err = None if rc == _ffi.OK else _ffi.RtmodtError(rc, _ffi.lib().rtmodt_last_error().decode(errors="replace"))
        if err is not None and rc != _ffi.E_CAPACITY:
            raise err
        upd, ret, us, rs = [], [], [], []
        for s in streams:
            d = 0 if flat else s
            nu, nr = int(self._cnt[0, d]), int(self._cnt[1, d])
            upd.append(self._upd[d, :nu].copy()); us.append(np.full(nu, s, np.int32))
            ret.append(self._ret[d, :nr].copy()); rs.append(np.full(nr, s, np.int32))
        self.updated, self.updated_stream = np.concatenate(upd), np.concatenate(us)
        self.retired, self.retired_stream = np.concatenate(ret), np.concatenate(rs)
        if self.on_retired is not None:
            for r, s in zip(self.retired, self.retired_stream):
                self.on_retired(self, r, int(s))
        if err is not None:
            raise err
        return self.updated, self.retired
