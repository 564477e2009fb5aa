"""An archive of appearance descriptors searched by similarity on the native engine.

The tree makes descriptors (``appearance.hip``'s colour histogram, ``ReidEmbedder``'s int8[512], BoT-SORT's smoothed feature, the
site-wide identities of ``CrossCameraLinker``) and compares them exactly, but every one of these forgets: an identity the linker
retires takes its feature with it.  ``AppearanceIndex`` keeps them: a device-resident, append-only ring of int8 rows with metadata
(``rid`` from 1, never reused; the caller's ``key``; stream; class; time), and ``search`` answers "where else, and when, did this
one appear?" for up to 64 queries at a time with the exact, deterministic top-k under filters -- ``csrc/index.hip``, two launches
whatever the archive holds; there is no CPU implementation here.  The reference has no counterpart (its ``Track`` has no descriptor,
its web API answers with the detections of one image).  ``tests/index_ref.py`` restates the rules, DESIGN.md section 40 lists them.
Parity with a published vector index is unpinned: none is installed where this runs, and none ranks in integers.

Similarity is in parts per million: ``ppm = 10^6 <q, row> / isqrt(|q|^2 |row|^2)`` in integers (``ppm // 1000`` is the linker's
per-mille similarity); hits come best first, the newest row first on a tie.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _ffi

NO_KEY = -(1 << 63)
PPM = 1000000
T_MIN, T_MAX = -(1 << 63), (1 << 63) - 1
ALL_STREAMS = (1 << 64) - 1
_META = (("rid", np.int64), ("key", np.int64), ("t", np.int64), ("stream", np.int32), ("cls", np.int32), ("n2", np.int32), ("dead", np.int32))


@dataclass
class Hit:
    """One row of the archive that matched: ``rid`` its row id, ``key`` / ``stream`` / ``cls`` / ``t`` what it was added with."""
    rid: int
    key: int
    stream: int
    cls: int
    t: int
    similarity_ppm: int

    @property
    def similarity(self) -> float:
        return self.similarity_ppm / PPM


def stream_mask(streams) -> int:
    """``None`` (every stream) or an iterable of stream numbers 0..63 -> the 64-bit mask of a filter."""
    if streams is None:
        return ALL_STREAMS
    m = 0
    for s in streams:
        if not 0 <= int(s) < 64:
            raise ValueError(f"stream {s}: 0..63")
        m |= 1 << int(s)
    return m


def make_filter(min_ppm: int = PPM // 2, t_range=None, streams=None, cls=None, exclude_key=None) -> _ffi.IndexFilter:
    t0, t1 = (T_MIN, T_MAX) if t_range is None else (int(t_range[0]), int(t_range[1]))
    return _ffi.IndexFilter(t0, t1, stream_mask(streams), NO_KEY if exclude_key is None else int(exclude_key), -1 if cls is None else int(cls),
                            int(min_ppm))


class AppearanceIndex(_ffi.Handle):
    """A ring of ``capacity`` descriptor rows of ``dim`` int8 values on the device; a newer row overwrites the oldest."""

    def __init__(self, dim: int, capacity: int = 1 << 20, *, max_queries: int = 64, max_k: int = 64, max_add: int = 4096, chunk_rows: int = 0,
                 device=0) -> None:
        self.dim, self.capacity, self.max_queries, self.max_k = int(dim), int(capacity), int(max_queries), int(max_k)
        self.max_add, self.chunk_rows = int(max_add), int(chunk_rows)
        self._device = _ffi.device_ordinal(device)
        cfg = _ffi.IndexCfg(self._device, self.dim, self.capacity, self.max_queries, self.max_k, self.max_add, self.chunk_rows)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_index_create(C.byref(cfg), C.byref(h)))
        self._h = h
        #: (n_hits, every entry) of the most recent search as the library wrote them, the unused entries too
        self.last_raw = None

    # ------------------------------------------------------------------ append
    def _rows(self, rows) -> np.ndarray:
        r = np.asarray(rows)
        if r.dtype.kind == "f":                              # float embeddings: the quantisation of the DeepSORT gallery
            r = _ffi.appearance_quantize(r.reshape(-1, r.shape[-1]))
        r = np.ascontiguousarray(r, np.int8)
        r = r.reshape(-1, r.shape[-1]) if r.ndim else r.reshape(0, self.dim)
        if r.shape[1] != self.dim:
            raise _ffi.RtmodtError(_ffi.E_INVALID, f"rows of dim {r.shape[1]} for an index of dim {self.dim}")
        return r

    def add(self, rows, keys, streams, cls, t) -> int:
        """Appends ``rows`` ``(n, dim)`` -- int8, float embeddings (quantised first) or a ``DeviceBuffer`` holding n int8 rows -- with
        ``keys`` ``(n,)`` and ``streams`` / ``cls`` / ``t`` (``(n,)`` or one value for all).  -> the ``rid`` of the first row; the
        others follow in list order."""
        keys = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(-1))
        n = len(keys)
        streams, cls = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (n,))) for v in (streams, cls))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.int64), (n,)))
        if isinstance(rows, _ffi.DeviceBuffer):
            if rows.nbytes < n * self.dim:
                raise ValueError(f"{n} rows of {self.dim} bytes overrun the {rows.nbytes}-byte buffer")
            src, kind = C.c_void_p(rows.ptr), _ffi.MEM_DEVICE
        else:
            host = self._rows(rows)
            if len(host) != n:
                raise ValueError(f"{len(host)} rows, {n} keys")
            src, kind = _ffi.ptr(host), _ffi.MEM_HOST
        first = C.c_int64(0)
        _ffi.check(_ffi.lib().rtmodt_index_add(self._h, src, kind, _ffi.ptr(keys), _ffi.ptr(streams), _ffi.ptr(cls), _ffi.ptr(t), n, C.byref(first)))
        return first.value

    def add_from_linker(self, linker, t: int, every: int = 1) -> int:
        """Appends the identities ``linker`` (a ``CrossCameraLinker``) sighted in the call it just made, each every ``every``-th call
        of its life, as rows with ``key = gid``, read where they lie on the device and queued behind that call.  -> the count."""
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().rtmodt_index_add_crosscam(self._h, linker._h, int(t), int(every), C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ search
    def search(self, queries, k: int = 10, min_similarity: float = 0.5, t_range=None, streams=None, cls=None, exclude_keys=None, *,
               min_ppm: int | None = None, filters=None) -> list:
        """The ``k`` most similar eligible rows per query: one list of ``Hit`` per row of ``queries`` ``(nq, dim)``, best first.
        ``min_similarity`` (or ``min_ppm``, exact), ``t_range = (t0, t1)`` inclusive, ``streams`` (an iterable of stream numbers)
        and ``cls`` apply to every query; ``exclude_keys`` is one key for all or one per query (``None``: none).  ``filters``: one
        ``make_filter(...)`` per query instead of all of these."""
        q = self._rows(queries)
        nq, k = len(q), int(k)
        if filters is None:
            ppm = int(round(float(min_similarity) * PPM)) if min_ppm is None else int(min_ppm)
            ex = [None] * nq if exclude_keys is None else ([exclude_keys] * nq if np.ndim(exclude_keys) == 0 else list(exclude_keys))
            if len(ex) != nq:
                raise ValueError(f"{len(ex)} exclude_keys for {nq} queries")
            filters = [make_filter(ppm, t_range, streams, cls, e) for e in ex]
        if len(filters) != nq:
            raise ValueError(f"{len(filters)} filters for {nq} queries")
        fl = (_ffi.IndexFilter * max(1, nq))(*filters)
        hits = (_ffi.IndexHit * max(1, nq * max(k, 1)))()
        nh = np.zeros(max(1, nq), np.int32)
        _ffi.check(_ffi.lib().rtmodt_index_search(self._h, _ffi.ptr(q), nq, C.cast(fl, C.c_void_p), k, C.cast(hits, C.c_void_p), _ffi.ptr(nh)))
        raw = np.frombuffer(hits, np.dtype([("rid", "<i8"), ("key", "<i8"), ("t", "<i8"), ("stream", "<i4"), ("cls", "<i4"), ("ppm", "<i4"), ("r", "<i4")]))
        self.last_raw = (nh[:nq].copy(), raw[:nq * k].reshape(nq, k).copy())        # every entry, the unused ones too
        return [[Hit(int(h["rid"]), int(h["key"]), int(h["stream"]), int(h["cls"]), int(h["t"]), int(h["ppm"])) for h in self.last_raw[1][i, :nh[i]]]
                for i in range(nq)]

    def forget(self, keys) -> int:
        """Every live row whose key is among ``keys`` (4096 at most per call) is dead from now on: never a hit again, gone for good
        when the ring overwrites it.  -> how many rows that were."""
        keys = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(-1))
        n = C.c_int64(0)
        _ffi.check(_ffi.lib().rtmodt_index_forget(self._h, _ffi.ptr(keys), len(keys), C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ state
    def _header(self):
        hdr = np.zeros(2, np.int64)
        _ffi.check(_ffi.lib().rtmodt_index_state(self._h, _ffi.ptr(hdr), *([None] * 8)))
        return int(hdr[0]), int(hdr[1])

    @property
    def next_rid(self) -> int:
        return self._header()[0]

    def __len__(self) -> int:
        """Rows in the ring, the dead ones included."""
        return self._header()[1]

    def snapshot(self) -> dict:
        """The whole archive in slot order (``tests/index_ref.py``: ``IndexRef.snapshot``); ``load`` takes it back."""
        hdr = np.zeros(2, np.int64)
        out = {"rows": np.zeros((self.capacity, self.dim), np.int8)}
        out.update({k: np.zeros(self.capacity, d) for k, d in _META})
        _ffi.check(_ffi.lib().rtmodt_index_state(self._h, _ffi.ptr(hdr), _ffi.ptr(out["rows"]), *[_ffi.ptr(out[k]) for k, _ in _META]))
        out["next_rid"] = int(hdr[0])
        return out

    def load(self, snap: dict) -> None:
        """Replaces the archive by a ``snapshot()`` of an index of the same ``dim`` and ``capacity``: a restart keeps what it saw."""
        rows = np.ascontiguousarray(snap["rows"], np.int8)
        if rows.shape != (self.capacity, self.dim):
            raise ValueError(f"snapshot of shape {rows.shape} for an index of {(self.capacity, self.dim)}")
        a = {k: np.ascontiguousarray(snap[k], d).reshape(self.capacity) for k, d in _META if k != "n2"}
        _ffi.check(_ffi.lib().rtmodt_index_load(self._h, int(snap["next_rid"]), _ffi.ptr(rows), *[_ffi.ptr(a[k]) for k, _ in _META if k != "n2"]))

    def save(self, path) -> None:
        """The snapshot as one ``.npz`` file."""
        s = self.snapshot()
        np.savez(path, dim=self.dim, capacity=self.capacity, **s)

    @classmethod
    def restore(cls, path, **kw) -> "AppearanceIndex":
        """A new index with the archive ``save`` wrote; ``kw``: the constructor's other arguments."""
        with np.load(path) as z:
            snap = {k: z[k] for k in z.files}
        idx = cls(int(snap["dim"]), int(snap["capacity"]), **kw)
        try:
            idx.load(snap)
        except Exception:
            idx.close()
            raise
        return idx

    def last_ms(self) -> tuple:
        """Device time (ms) of the last add and of the last search (0.0: none yet)."""
        return _ffi.last_ms("rtmodt_index_last_ms", self._h, 2)

    _destroy = "rtmodt_index_destroy"
