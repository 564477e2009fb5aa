"""The cross-camera linker restated in plain Python / NumPy: the rules ``csrc/crosscam_rule.h`` and ``csrc/crosscam.hip`` are pinned
to.  ``CrossCamRef.process`` is one call of ``rtmodt_crosscam_process``; its state (``table``, ``ledgers``) is compared with the
handle's exactly.  No published multi-camera tracker is restated here: the reference has one source and no global id.

The choices the rule text of include/rtmodt.h leaves open, made here (DESIGN.md section 33 repeats them):
  * the call counter c is 1 in the first call; an identity retires when c - max(last_seen) > max_age, a binding is dropped when
    c - (call of its last sighting) > bind_age or when its identity retires; both are decided before anything else in the call;
  * entries are numbered in the caller's order; a stream's queries are its unbound entries with a non-zero row, in that order;
  * the matching of a stream takes the retired table ("start of call" = after step 1) and the liveness the bound pass left;
  * JOIN asks for equal classes whatever ``match_class`` says (the text says so); LINK asks for them when ``match_class`` is set;
  * with the table full a query may still JOIN; only a founder needs a row;
  * a stream past the solver's contested limits keeps NONE of its matches this call, its queries get status UNBOUND and take no
    part in the births; the sticky error 2 is per stream;
  * sim of an entry: LINKED against the identity's s8, JOINED against the founder's birth feature, every other status 0;
  * a JOINED event has from_stream = the founder's stream and gap 0 (the identity has no start-of-call sighting);
  * the feature of an identity sighted in several streams in one call is stepped once per stream, ascending; a founder's row is
    the birth, the joiners follow."""
from __future__ import annotations

import math

import numpy as np

import lap_ref as LR
from hota_ref import lap_solve

NONE, BOUND, LINKED, JOINED, BORN, NO_DESCRIPTOR, DEFERRED, TABLE_FULL, UNBOUND = range(9)
FEAT_NORM = 16256
MAX_STREAMS, MAX_DIM, MAX_TRACKS, MAX_IDENTITIES, MAX_QUERIES = 64, 512, 256, 4096, 1024
E_INVALID = -1


def sim_milli(dot: int, nq: int, ng: int) -> int:
    dot, nq, ng = int(dot), int(nq), int(ng)
    if dot <= 0:
        return 0
    return min(1000, 1000 * dot // max(1, math.isqrt(nq * ng)))


def norm2(row) -> int:
    r = np.asarray(row, np.int64)
    return int((r * r).sum())


def sim_rows(q, g) -> int:
    q, g = np.asarray(q, np.int64), np.asarray(g, np.int64)
    return sim_milli(int((q * g).sum()), norm2(q), norm2(g))


def isqrt_vec(p):
    """floor(sqrt(p)) of an int64 array, exactly (p < 2^53: the float64 root is off by one at most)."""
    p = np.asarray(p, np.int64)
    r = np.floor(np.sqrt(p.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > p, r - 1, r)
    return np.where((r + 1) * (r + 1) <= p, r + 1, r)


def sim_matrix(dots, nq, ng):
    """sim_milli over a matrix of dots with the rows' and columns' squared norms."""
    dots = np.asarray(dots, np.int64)
    den = np.maximum(1, isqrt_vec(np.asarray(nq, np.int64)[:, None] * np.asarray(ng, np.int64)[None, :]))
    return np.where(dots <= 0, 0, np.minimum(1000, 1000 * np.maximum(dots, 0) // den))


def feat_step(s16, f):
    """v = 9 s16 + 128 f (s16 None: a birth, 128 f) -> (s16, s8) as int lists; botsort_ref.feat_step states the same."""
    f = [int(v) for v in f]
    v = [128 * b for b in f] if s16 is None else [9 * int(a) + 128 * b for a, b in zip(s16, f)]
    r = math.isqrt(sum(x * x for x in v))
    if r == 0:
        return [0] * len(v), [0] * len(v)
    sg = lambda x: -1 if x < 0 else 1                      # noqa: E731
    return ([sg(x) * ((FEAT_NORM * abs(x) + r // 2) // r) for x in v],
            [sg(x) * min(127, (127 * abs(x) + r // 2) // r) for x in v])


def max_gain_rows(gain):
    """track_dev.h's assoc_sparse on a dense matrix of integer gains (0 = inadmissible): pairs whose row and column both have
    degree 1 are matched outright, the contested rows (lap_ref.contested) go to lap_solve in ascending row order with their
    edges in ascending column order.  -> (row -> column or -1, ok); ok False past lap.h's limits."""
    gain = np.asarray(gain, np.int64)
    nr, nc = gain.shape
    x = [-1] * nr
    if nr == 0 or nc == 0:
        return x, True
    adj = gain > 0
    hard, _, _ = LR.contested(adj)
    if not LR.within_limits(adj):
        return x, False
    hard = [int(r) for r in hard]
    hs = set(hard)
    for r in range(nr):
        if r not in hs and adj[r].sum() == 1:
            x[r] = int(np.argmax(adj[r]))
    colmap, estart, ecol, ecost = {}, [0], [], []
    for r in hard:
        for c in np.nonzero(adj[r])[0]:
            colmap.setdefault(int(c), len(colmap))
            ecol.append(colmap[int(c)])
            ecost.append(-int(gain[r, c]))
        estart.append(len(ecol))
    inv = {v: k for k, v in colmap.items()}
    for h, j in enumerate(lap_solve(estart, ecol, ecost, len(colmap))):
        if j >= 0:
            x[hard[h]] = inv[j]
    return x, True


class Identity:
    __slots__ = ("gid", "cls", "s16", "s8", "first_seen", "last_seen")

    def __init__(self, gid, cls, s16, s8, first_seen, last_seen):
        self.gid, self.cls, self.s16, self.s8, self.first_seen, self.last_seen = gid, cls, s16, s8, first_seen, last_seen


class CrossCamRef:
    def __init__(self, n_streams, dim, max_tracks=64, max_identities=256, max_queries=256, min_sim_milli=700, max_age=300, bind_age=None,
                 match_class=True):
        assert 1 <= n_streams <= MAX_STREAMS and dim % 64 == 0 and 64 <= dim <= MAX_DIM
        self.S, self.D, self.Mc, self.I, self.Q = n_streams, dim, max_tracks, max_identities, max_queries
        self.min_sim, self.max_age, self.bind_age, self.match_class = min_sim_milli, max_age, max_age if bind_age is None else bind_age, bool(match_class)
        self.tmin = [[0] * n_streams for _ in range(n_streams)]
        self.tmax = [[self.max_age] * n_streams for _ in range(n_streams)]
        self.c, self.next_gid = 0, 1
        self.table: list[Identity] = []                    # gid order
        self.ledgers = [dict() for _ in range(n_streams)]  # local id -> [gid, call of the last sighting]
        self.err = [0] * n_streams
        self.counters = {}

    def set_transit(self, src, dst, lo, hi):
        self.tmin[src][dst], self.tmax[src][dst] = int(lo), int(hi)

    def process(self, lists):
        """lists[s] = (ids, classes, rows int8 (n, dim)).  -> dict(gid, status, sim: per stream lists; events; retired) or E_INVALID."""
        S = self.S
        lists = [(np.asarray(i, np.int64).reshape(-1), np.asarray(k, np.int32).reshape(-1), np.asarray(r, np.int8).reshape(-1, self.D)) for i, k, r in lists]
        for ids, _, _ in lists:
            if len(set(ids.tolist())) != len(ids) or len(ids) > self.Mc:
                return E_INVALID
        self.c += 1
        c = self.c
        # 1. retire
        retired = []
        keep = []
        for g in self.table:
            if c - max(g.last_seen) > self.max_age:
                retired.append((g.gid, g.first_seen, max(g.last_seen), sum(1 << s for s in range(S) if g.last_seen[s] > 0)))
            else:
                keep.append(g)
        self.table = keep
        by_gid = {g.gid: g for g in self.table}
        for L in self.ledgers:
            for lid in [lid for lid, (gid, last) in L.items() if gid not in by_gid or c - last > self.bind_age]:
                del L[lid]
        start_last = {g.gid: list(g.last_seen) for g in self.table}
        # 2. bound pass
        gid = [[0] * len(l[0]) for l in lists]
        status = [[NONE] * len(l[0]) for l in lists]
        sim = [[0] * len(l[0]) for l in lists]
        live = [set() for _ in range(S)]
        sight = {}                                         # gid -> {stream: row}
        queries = []                                       # (stream, entry)
        n_deferred = 0
        for s, (ids, cls, rows) in enumerate(lists):
            for e in range(len(ids)):
                b = self.ledgers[s].get(int(ids[e]))
                if b is not None:
                    gid[s][e], status[s][e] = b[0], BOUND
                    b[1] = c
                    live[s].add(b[0])
                    if rows[e].any():
                        sight.setdefault(b[0], {})[s] = rows[e]
                    else:
                        by_gid[b[0]].last_seen[s] = c      # sighted, but no row to step the feature with
                elif not rows[e].any():
                    status[s][e] = NO_DESCRIPTOR
                elif len(queries) >= self.Q:
                    status[s][e] = DEFERRED
                    n_deferred += 1
                else:
                    queries.append((s, e))
        # 3 + 4. similarity and the matching of each stream against the table as the call found it
        events = {}
        unmatched = []
        T = self.table
        nT = len(T)
        T8 = np.asarray([g.s8 for g in T], np.int64).reshape(nT, self.D)
        ng = (T8 * T8).sum(axis=1)
        Tcls = np.asarray([g.cls for g in T], np.int64)
        Tlast = np.asarray([start_last[g.gid] for g in T], np.int64).reshape(nT, S)
        for s in range(S):
            qs = [(ss, e) for ss, e in queries if ss == s]
            if not qs:
                continue
            ids, cls, rows = lists[s]
            gain = np.zeros((len(qs), nT), np.int64)
            sims = np.zeros((len(qs), nT), np.int64)
            if nT:
                qr = rows[[e for _, e in qs]].astype(np.int64)
                sims = sim_matrix(qr @ T8.T, (qr * qr).sum(axis=1), ng)
                ok = sims >= self.min_sim
                if self.match_class:
                    ok &= cls[[e for _, e in qs]].astype(np.int64)[:, None] == Tcls[None, :]
                ok &= ~np.asarray([g.gid in live[s] for g in T], bool)[None, :]
                age = c - Tlast
                lo, hi = np.asarray(self.tmin, np.int64)[:, s], np.asarray(self.tmax, np.int64)[:, s]
                ok &= ((Tlast > 0) & (age >= lo[None, :]) & (age <= hi[None, :])).any(axis=1)[None, :]
                gain = np.where(ok, sims - self.min_sim + 1, 0)
            x, ok = max_gain_rows(gain)
            if not ok:
                self.err[s] = 2
                for _, e in qs:
                    status[s][e] = UNBOUND
                continue
            for r, (_, e) in enumerate(qs):
                if x[r] < 0:
                    unmatched.append((s, e))
                    continue
                g = T[x[r]]
                gid[s][e], status[s][e], sim[s][e] = g.gid, LINKED, int(sims[r, x[r]])
                for lid in [lid for lid, b in self.ledgers[s].items() if b[0] == g.gid]:
                    del self.ledgers[s][lid]               # the older binding of g in s (absent this call)
                self.ledgers[s][int(ids[e])] = [g.gid, c]
                sight.setdefault(g.gid, {})[s] = rows[e]
                sl = start_last[g.gid]
                f = max(range(S), key=lambda k: (sl[k], -k))
                events[(s, e)] = (g.gid, s, int(ids[e]), f, c - sl[f], sim[s][e])
        # 5. births, serially in query order
        born = []                                          # [gid, cls, birth s8, live streams (ordered), founder stream]
        n_full = 0
        B8, Bn = np.zeros((len(unmatched), self.D), np.int64), np.zeros(len(unmatched), np.int64)      # the founders' birth features
        for s, e in sorted(unmatched):
            ids, cls, rows = lists[s]
            best = None
            if born:
                q = rows[e].astype(np.int64)
                v = sim_matrix((q @ B8[:len(born)].T)[None, :], [int((q * q).sum())], Bn[:len(born)])[0]
                for k in np.nonzero(v >= self.min_sim)[0]:
                    b = born[int(k)]
                    if b[1] != int(cls[e]) or s in b[3] or not any(self.tmin[f][s] == 0 <= self.tmax[f][s] for f in b[3]):
                        continue
                    if best is None or v[k] > best[0]:
                        best = (int(v[k]), b)
            if best is not None:
                v, b = best
                b[3].append(s)
                gid[s][e], status[s][e], sim[s][e] = b[0], JOINED, v
                events[(s, e)] = (b[0], s, int(ids[e]), b[4], 0, v)
            elif len(self.table) + len(born) >= self.I:
                status[s][e] = TABLE_FULL
                n_full += 1
                continue
            else:
                b = [self.next_gid, int(cls[e]), feat_step(None, rows[e])[1], [s], s]
                self.next_gid += 1
                B8[len(born)] = b[2]
                Bn[len(born)] = norm2(b[2])
                born.append(b)
                gid[s][e], status[s][e] = b[0], BORN
            self.ledgers[s][int(ids[e])] = [b[0], c]
            sight.setdefault(b[0], {})[s] = rows[e]
        for b in born:
            g = Identity(b[0], b[1], None, None, c, [0] * S)
            self.table.append(g)
            by_gid[g.gid] = g
        # 6. feature update, ascending stream order
        for g_id, per in sight.items():
            g = by_gid[g_id]
            for s in sorted(per):
                g.s16, g.s8 = feat_step(g.s16, per[s])
                g.last_seen[s] = c
        ev = [events[k] for k in sorted(events)]
        self.counters = dict(call=c, n_identities=len(self.table), next_gid=self.next_gid, n_queries=len(queries), n_deferred=n_deferred,
                             n_table_full=n_full, n_events=len(ev), n_retired=len(retired))
        return dict(gid=gid, status=status, sim=sim, events=ev, retired=retired)

    # ---- the state as rtmodt_crosscam_state hands it out ----
    def load(self, snap):
        """The counterpart of rtmodt_crosscam_load: the call counter, next gid, table and ledgers of a snapshot; err is cleared."""
        S, D = self.S, self.D
        n = len(snap["gid"])
        assert n <= self.I and len(snap["ledgers"]) == S
        last = np.asarray(snap["last_seen"], np.int64).reshape(n, S)
        s16, s8 = np.asarray(snap["s16"], np.int64).reshape(n, D), np.asarray(snap["s8"], np.int64).reshape(n, D)
        self.c, self.next_gid = int(snap["call"]), int(snap["next_gid"])
        self.table = [Identity(int(snap["gid"][i]), int(snap["cls"][i]), s16[i].tolist(), s8[i].tolist(), int(snap["first_seen"][i]), last[i].tolist())
                      for i in range(n)]
        self.ledgers = [{int(l): [int(g), int(t)] for l, g, t in np.asarray(led, np.int64).reshape(-1, 3)} for led in snap["ledgers"]]
        self.err = [0] * S

    def snapshot(self):
        n = len(self.table)
        t = dict(call=self.c, next_gid=self.next_gid,
                 gid=np.asarray([g.gid for g in self.table], np.int64), cls=np.asarray([g.cls for g in self.table], np.int32),
                 first_seen=np.asarray([g.first_seen for g in self.table], np.int64),
                 last_seen=np.asarray([g.last_seen for g in self.table], np.int64).reshape(n, self.S),
                 s16=np.asarray([g.s16 for g in self.table], np.int16).reshape(n, self.D),
                 s8=np.asarray([g.s8 for g in self.table], np.int8).reshape(n, self.D))
        t["ledgers"] = [np.asarray([(lid, b[0], b[1]) for lid, b in sorted(L.items())], np.int64).reshape(-1, 3) for L in self.ledgers]
        return t


def snapshots_equal(a: dict, b: dict):
    """-> None when equal, else the name of the first field that differs."""
    for k in ("call", "next_gid"):
        if int(a[k]) != int(b[k]):
            return k
    for k in ("gid", "cls", "first_seen", "last_seen", "s16", "s8"):
        if np.asarray(a[k]).shape != np.asarray(b[k]).shape or not np.array_equal(a[k], b[k]):
            return k
    for s, (x, y) in enumerate(zip(a["ledgers"], b["ledgers"])):
        if x.shape != y.shape or not np.array_equal(x, y):
            return f"ledger {s}"
    return None


# ---- the generator of the random site (GPU case 3), checked on the restatement alone in test_crosscam_cpu.py ----
def person_rows(n_people, dim, seed):
    """One int8 base row per person: +-100 in a random sign pattern, so that two people's rows are nearly orthogonal."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, (n_people, dim)) * 200 - 100).astype(np.int8)


def noisy(base, rng, amp=12):
    return np.clip(base.astype(np.int32) + rng.integers(-amp, amp + 1, base.shape), -127, 127).astype(np.int8)


def random_site(seed=5, n_streams=3, calls=40, n_people=12, dim=64):
    """-> (frames, truth): frames[c][s] = (ids, classes, rows); truth[c][s] = the person behind each entry.  Every person walks
    through the cameras in turn: visible in one stream for a few calls, absent for 1..3, then in the next.  Local ids change
    when a track fragments (a new id in the same stream after a one-call gap).  Transit 0 -> 2 is restricted by the caller."""
    rng = np.random.default_rng(seed)
    base = person_rows(n_people, dim, seed + 1)
    next_id = [1] * n_streams
    plan = []                                              # per person: list of (stream, first call, last call, local id)
    for p in range(n_people):
        t = int(rng.integers(0, 6))
        s = int(rng.integers(0, n_streams))
        segs = []
        while t < calls:
            d = int(rng.integers(3, 8))
            segs.append([s, t, min(calls, t + d) - 1, next_id[s]])
            next_id[s] += 1
            t += d + int(rng.integers(1, 4))
            if rng.random() < 0.3:                         # a fragment: the same stream, a new local id
                continue
            s = (s + 1) % n_streams
        plan.append(segs)
    frames, truth = [], []
    for c in range(calls):
        fr, tr = [], []
        for s in range(n_streams):
            ids, rows, who = [], [], []
            for p, segs in enumerate(plan):
                for ss, t0, t1, lid in segs:
                    if ss == s and t0 <= c <= t1:
                        ids.append(lid)
                        rows.append(noisy(base[p], rng))
                        who.append(p)
            fr.append((np.asarray(ids, np.int64), np.zeros(len(ids), np.int32), np.asarray(rows, np.int8).reshape(-1, dim)))
            tr.append(who)
        frames.append(fr)
        truth.append(tr)
    return frames, truth, base
