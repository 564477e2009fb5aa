"""The appearance index restated in plain Python / NumPy: the rules ``csrc/index_rule.h`` and ``csrc/index.hip`` are pinned to.
``IndexRef`` mirrors the handle call for call (``add``, ``add_from_snapshot`` for ``rtmodt_index_add_crosscam``, ``search``,
``forget``, ``snapshot`` / ``load``); its state is compared with the handle's exactly.  No published vector index is restated
here: the reference has no descriptor to search, and none of the published ones ranks in integers.

  row         rid (from 1, never reused) in slot (rid - 1) % capacity, a newer row overwrites the oldest; key, stream 0..63, cls, t,
              n2 = sum v^2, dead
  similarity  dot = <q, row>; ppm = dot <= 0 ? 0 : min(10^6, 10^6 dot // max(1, isqrt(nq n2)))
  eligible    filled, not dead, t0 <= t <= t1, bit `stream` of the mask, cls_q < 0 or cls == cls_q, key != exclude_key (NO_KEY:
              none), ppm >= min_ppm
  rank        ppm << 40 | rid, descending; n_hits <= k entries, the unused ones zero
The choices the rule text leaves open, made here (DESIGN.md section 40 repeats them): a list longer than the ring keeps its last
``capacity`` rows (the rids of the others are used up all the same); ``forget`` counts rows, not keys, and a row already dead is not
counted again; a dead row keeps its slot until it is overwritten."""
from __future__ import annotations

import math

import numpy as np

from crosscam_ref import isqrt_vec

PPM = 1000000
RID_BITS = 40
NO_KEY = -(1 << 63)
T_MIN, T_MAX = -(1 << 63), (1 << 63) - 1
ALL_STREAMS = (1 << 64) - 1
MAX_CAPACITY, MAX_QUERIES, MAX_K, MAX_ADD, MAX_FORGET, MAX_CHUNKS = 1 << 22, 64, 64, 65536, 4096, 256
E_INVALID = -1
META = (("rid", np.int64), ("key", np.int64), ("t", np.int64), ("stream", np.int32), ("cls", np.int32), ("n2", np.int32), ("dead", np.int32))


def ppm_of(dot: int, nq: int, n2: int) -> int:
    dot, nq, n2 = int(dot), int(nq), int(n2)
    if dot <= 0:
        return 0
    return min(PPM, PPM * dot // max(1, math.isqrt(nq * n2)))


def ppm_matrix(dots, nq, n2):
    """ppm_of over a matrix of dots with the rows' (queries) and columns' (archive rows) squared norms."""
    dots = np.asarray(dots, np.int64)
    den = np.maximum(1, isqrt_vec(np.asarray(nq, np.int64)[:, None] * np.asarray(n2, np.int64)[None, :]))
    return np.where(dots <= 0, 0, np.minimum(PPM, PPM * np.maximum(dots, 0) // den))


def chunk_rows(capacity: int, requested: int = 0) -> int:
    """The rows of a chunk (0: the request is not allowed)."""
    if not 1 <= capacity <= MAX_CAPACITY or requested < 0:
        return 0
    if requested == 0:
        return (-(-capacity // MAX_CHUNKS) + 63) // 64 * 64
    if requested % 64 or -(-capacity // requested) > MAX_CHUNKS:
        return 0
    return requested


def filt(min_ppm=PPM // 2, t_range=None, streams=None, cls=None, exclude_key=None) -> dict:
    """One query's filter."""
    t0, t1 = (T_MIN, T_MAX) if t_range is None else t_range
    mask = ALL_STREAMS if streams is None else sum(1 << int(s) for s in set(streams))
    return dict(t0=int(t0), t1=int(t1), mask=mask, cls=-1 if cls is None else int(cls), excl=NO_KEY if exclude_key is None else int(exclude_key),
                min_ppm=int(min_ppm))


class IndexRef:
    def __init__(self, dim, capacity, max_queries=MAX_QUERIES, max_k=MAX_K, max_add=4096, chunk_rows_req=0):
        assert dim % 64 == 0 and 64 <= dim <= 512 and 1 <= capacity <= MAX_CAPACITY
        self.D, self.N, self.Q, self.K, self.A = dim, capacity, max_queries, max_k, max_add
        self.chunk = chunk_rows(capacity, chunk_rows_req)
        assert self.chunk > 0
        self.next_rid = 1
        self.rows = np.zeros((capacity, dim), np.int8)
        for k, d in META:
            setattr(self, k, np.zeros(capacity, d))

    def __len__(self):
        return min(self.next_rid - 1, self.N)

    # ---- append ----
    def add(self, rows, keys, streams, cls, t):
        """-> the first rid, or E_INVALID with nothing changed."""
        keys = np.asarray(keys, np.int64).reshape(-1)
        n = len(keys)
        rows = np.asarray(rows, np.int8).reshape(n, self.D)
        streams, cls = (np.broadcast_to(np.asarray(v, np.int32), (n,)) for v in (streams, cls))
        t = np.broadcast_to(np.asarray(t, np.int64), (n,))
        if n > self.A or ((streams < 0) | (streams > 63)).any():
            return E_INVALID
        first = self.next_rid
        for i in range(max(0, n - self.N), n):
            s = (first + i - 1) % self.N
            self.rows[s] = rows[i]
            self.rid[s], self.key[s], self.t[s], self.stream[s], self.cls[s], self.dead[s] = first + i, keys[i], t[i], streams[i], cls[i], 0
            r = rows[i].astype(np.int64)
            self.n2[s] = int((r * r).sum())
        self.next_rid += n
        return first

    def add_from_snapshot(self, snap, t, every=1):
        """rtmodt_index_add_crosscam on ``CrossCameraLinker.snapshot()`` / ``CrossCamRef.snapshot()`` taken after the call: the
        identities sighted in that call, every ``every``-th call of their life, in gid order.  -> the count."""
        c = int(snap["call"])
        if len(snap["gid"]) == 0:
            return 0
        last = np.asarray(snap["last_seen"], np.int64).reshape(len(snap["gid"]), -1)
        sel = [i for i in range(len(snap["gid"])) if last[i].max(initial=0) == c and (c - int(snap["first_seen"][i])) % every == 0]
        if sel:
            self.add(np.asarray(snap["s8"], np.int8)[sel], np.asarray(snap["gid"], np.int64)[sel], [int(np.argmax(last[i] == c)) for i in sel],
                     np.asarray(snap["cls"], np.int32)[sel], t)
        return len(sel)

    # ---- search ----
    def ranks(self, queries, filters):
        """(nq, capacity) int64: the rank of every slot for every query, 0 where the row is not eligible."""
        q = np.asarray(queries, np.int8).reshape(-1, self.D)
        dots = q.astype(np.int32) @ self.rows.astype(np.int32).T
        q64 = q.astype(np.int64)
        ppm = ppm_matrix(dots, (q64 * q64).sum(axis=1), self.n2)
        out = np.zeros(ppm.shape, np.int64)
        live = (self.rid > 0) & (self.dead == 0)
        sh = self.stream.astype(np.uint64)
        for i, f in enumerate(filters):
            ok = live & (self.t >= f["t0"]) & (self.t <= f["t1"]) & ((np.uint64(f["mask"]) >> sh) & np.uint64(1) == np.uint64(1))
            if f["cls"] >= 0:
                ok &= self.cls == f["cls"]
            if f["excl"] != NO_KEY:
                ok &= self.key != f["excl"]
            ok &= ppm[i] >= f["min_ppm"]
            out[i] = np.where(ok, (ppm[i] << RID_BITS) | self.rid, 0)
        return out

    def search(self, queries, filters, k):
        """-> per query the list of (rid, key, stream, cls, t, ppm), best first; or E_INVALID."""
        q = np.asarray(queries, np.int8).reshape(-1, self.D)
        if len(q) > self.Q or not 1 <= k <= self.K or len(filters) != len(q) or any(not 1 <= f["min_ppm"] <= PPM for f in filters):
            return E_INVALID
        res = []
        for r in self.ranks(q, filters):
            top = np.sort(r[r > 0])[::-1][:k]
            hits = []
            for v in top.tolist():
                rid, s = v & ((1 << RID_BITS) - 1), ((v & ((1 << RID_BITS) - 1)) - 1) % self.N
                hits.append((rid, int(self.key[s]), int(self.stream[s]), int(self.cls[s]), int(self.t[s]), v >> RID_BITS))
            res.append(hits)
        return res

    def forget(self, keys):
        keys = np.asarray(keys, np.int64).reshape(-1)
        if len(keys) > MAX_FORGET:
            return E_INVALID
        hit = (self.rid > 0) & (self.dead == 0) & np.isin(self.key, keys)
        self.dead[hit] = 1
        return int(hit.sum())

    # ---- the state as rtmodt_index_state hands it out ----
    def snapshot(self):
        out = {"next_rid": self.next_rid, "rows": self.rows.copy()}
        out.update({k: getattr(self, k).copy() for k, _ in META})
        return out

    def load(self, snap):
        """-> None, or E_INVALID with nothing changed (a rid that is not the one its slot holds at next_rid, ...)."""
        nxt = int(snap["next_rid"])
        rid = np.asarray(snap["rid"], np.int64)
        want = np.asarray([slot_rid(s, self.N, nxt) for s in range(self.N)], np.int64)
        st, dead = np.asarray(snap["stream"], np.int32), np.asarray(snap["dead"], np.int32)
        if nxt < 1 or not np.array_equal(rid, want) or ((st < 0) | (st > 63) | (dead < 0) | (dead > 1))[want > 0].any():
            return E_INVALID
        self.next_rid = nxt
        self.rows = np.asarray(snap["rows"], np.int8).reshape(self.N, self.D).copy()
        for k, d in META:
            setattr(self, k, np.asarray(snap[k], d).copy())
        r = self.rows.astype(np.int64)
        self.n2 = np.where(want > 0, (r * r).sum(axis=1), 0).astype(np.int32)
        return None


def slot_rid(slot, capacity, next_rid):
    """The rid slot holds when the next row gets next_rid (0: empty)."""
    newest = next_rid - 1
    if newest < 1:
        return 0
    r = newest - ((newest - 1) % capacity - slot) % capacity
    return r if r >= 1 else 0


def snapshots_equal(a: dict, b: dict):
    """-> None when equal, else the name of the first field that differs."""
    if int(a["next_rid"]) != int(b["next_rid"]):
        return "next_rid"
    for k in ("rows",) + tuple(k for k, _ in META):
        if np.asarray(a[k]).shape != np.asarray(b[k]).shape or not np.array_equal(a[k], b[k]):
            return k
    return None


def brute_force(ref: IndexRef, query, f, k):
    """One query by a double loop and sorted(): the definition the vectorised ``search`` is checked against."""
    q = [int(v) for v in np.asarray(query, np.int8)]
    nq = sum(v * v for v in q)
    cand = []
    for s in range(ref.N):
        if ref.rid[s] <= 0 or ref.dead[s]:
            continue
        row = [int(v) for v in ref.rows[s]]
        p = ppm_of(sum(a * b for a, b in zip(q, row)), nq, sum(v * v for v in row))
        if not f["t0"] <= int(ref.t[s]) <= f["t1"] or not (f["mask"] >> int(ref.stream[s])) & 1:
            continue
        if (f["cls"] >= 0 and int(ref.cls[s]) != f["cls"]) or (f["excl"] != NO_KEY and int(ref.key[s]) == f["excl"]) or p < f["min_ppm"]:
            continue
        cand.append((p, int(ref.rid[s]), s))
    return [(rid, int(ref.key[s]), int(ref.stream[s]), int(ref.cls[s]), int(ref.t[s]), p) for p, rid, s in sorted(cand, reverse=True)[:k]]
