"""Track stitching on the GPU: the fragments a tracker leaves behind an occlusion are merged back into one identity.

The reference's design document prescribes this step three times and never builds it (TECHNICAL_DESIGN_DOCUMENT.md B.4
"IDF1 Optimization" item 4, G.1 row 1, and G.2's ``correct_id_switches`` whose body is ``...``).  ``rtmodt_stitch_tracks``
(``csrc/stitch.hip``) does it for many sequences per call; DESIGN.md section 18 states the rules.

PARITY UNPINNED: the reference has no implementation and no third-party stitcher is installed anywhere this runs;
tests/stitch_ref.py restates the rules in plain Python and the GPU tests require equality with it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi


def _sequence_arrays(rows):
    """One sequence's ``(n, 6)`` rows -> (rows sorted by (id, frame), ids ascending, rows per id); the input checks."""
    a = np.asarray(rows, np.float64).reshape(-1, 6)
    if len(a):
        if not np.isfinite(a[:, :2]).all() or (a[:, 0] != np.floor(a[:, 0])).any():
            raise ValueError("stitch_tracks: a frame number is not an integer")
        if (a[:, 1] != np.floor(a[:, 1])).any():
            raise ValueError("stitch_tracks: a track id is not an integer")
    a = a[np.lexsort((a[:, 0], a[:, 1]))]
    if len(a) > 1 and ((a[1:, 0] == a[:-1, 0]) & (a[1:, 1] == a[:-1, 1])).any():      # sorted: a duplicate pair is adjacent
        raise ValueError("stitch_tracks: a (frame, id) pair occurs twice")
    ids, counts = np.unique(a[:, 1], return_counts=True)
    return a, ids.astype(np.int64), counts.astype(np.int64)


def stitch_tracks(sequences, *, max_gap=30, max_dist=20.0, velocity_window=0, interpolate=False, device="cuda:0",
                  return_candidates=False) -> list:
    """Merge fragmented tracks of many sequences in one call.  ``sequences``: ``(n, 6)`` arrays ``frame, id, x, y, w, h``
    (0-based boxes, as ``load_mot`` returns them; ids are arbitrary integers).

    A tracklet A (all rows of one id) is linked to a tracklet B when B starts 1..``max_gap`` frames after A ends and B's
    first centre lies less than ``max_dist`` px from A's exit point: A's last centre, moved along A's mean velocity over its
    last ``velocity_window`` steps when that is > 0.  Links are one-to-one; the chosen set has the most links and among
    those the smallest sum of squared distances.  Every chain of links takes the id of its first tracklet.
    ``interpolate`` adds linearly interpolated rows for the frames inside every linked gap.

    Returns one record per sequence: ``rows`` (the input rows with the new ids, then the fill rows, sorted by (frame, id)),
    ``id_map`` (old id -> new id), ``links`` (``(id_A, id_B, gap, d2)`` in id order), ``n_tracks_before`` and
    ``n_tracks_after``; ``fill`` holds the fill rows alone.  ``return_candidates`` adds ``candidates``: every admissible
    link ``(id_A, id_B, gap, d2, (p.x, p.y))``.  A duplicate (frame, id) or a non-integer frame raises ``ValueError``."""
    seqs = [_sequence_arrays(s) for s in sequences]
    if not seqs:
        return []
    n_seq = len(seqs)
    seq_trk_start = np.zeros(n_seq + 1, np.int32)
    seq_trk_start[1:] = np.cumsum([len(ids) for _, ids, _ in seqs])
    n_trk = int(seq_trk_start[-1])
    counts = np.concatenate([c for _, _, c in seqs]) if n_trk else np.zeros(0, np.int64)
    trk_row_start = np.zeros(n_trk + 1, np.int64)
    trk_row_start[1:] = np.cumsum(counts)
    if trk_row_start[-1] >= 2 ** 31:
        raise ValueError("stitch_tracks: more than 2^31 - 1 rows in one call")
    trk_row_start = trk_row_start.astype(np.int32)
    allrows = np.concatenate([a for a, _, _ in seqs]) if n_trk else np.zeros((0, 6))
    row_frame = np.ascontiguousarray(allrows[:, 0], np.int64)
    row_box = np.ascontiguousarray(allrows[:, 2:6], np.float64)
    # the fill rows' and the candidates' upper bounds: one call, never two
    first = row_frame[trk_row_start[:-1]] if n_trk else np.zeros(0, np.int64)
    last = row_frame[trk_row_start[1:] - 1] if n_trk else np.zeros(0, np.int64)
    gap = max(int(max_gap), 0)
    fill_cap = cand_cap = 0
    for s in range(n_seq):
        t0, t1 = int(seq_trk_start[s]), int(seq_trk_start[s + 1])
        if t1 == t0:
            continue
        if interpolate:
            fill_cap += int(np.maximum(np.minimum(gap, first[t0:t1].max() - last[t0:t1]) - 1, 0).sum())
        if return_candidates:
            st = np.sort(first[t0:t1])
            cand_cap += int((np.searchsorted(st, last[t0:t1] + gap, "right") - np.searchsorted(st, last[t0:t1], "right")).sum())
    succ = np.full(n_trk, -1, np.int32)
    root = np.arange(n_trk, dtype=np.int32)
    link_d2 = np.zeros(n_trk, np.float64)
    seq_links = np.zeros(n_seq, np.int64)
    seq_cost = np.zeros(n_seq, np.float64)
    fill_trk = np.zeros(fill_cap, np.int32)
    fill_frame = np.zeros(fill_cap, np.int64)
    fill_box = np.zeros((fill_cap, 4), np.float64)
    cand_a, cand_b = np.zeros(cand_cap, np.int32), np.zeros(cand_cap, np.int32)
    cand_d2, cand_p = np.zeros(cand_cap, np.float64), np.zeros((cand_cap, 2), np.float64)
    n_fill, n_cand = C.c_int64(0), C.c_int64(0)
    params = _ffi.StitchParams(int(max_gap), float(max_dist), int(velocity_window), int(bool(interpolate)))
    P = _ffi.ptr
    _ffi.check(_ffi.lib().rtmodt_stitch_tracks(_ffi.device_ordinal(device), C.byref(params), n_seq, P(seq_trk_start), P(trk_row_start),
                                               P(row_frame), P(row_box), P(succ), P(root), P(link_d2), P(seq_links), P(seq_cost),
                                               fill_cap, P(fill_trk), P(fill_frame), P(fill_box), C.byref(n_fill), cand_cap, P(cand_a),
                                               P(cand_b), P(cand_d2), P(cand_p), C.byref(n_cand) if return_candidates else None))
    nf, nc = int(n_fill.value), int(n_cand.value)
    trk_seq = np.repeat(np.arange(n_seq), np.diff(seq_trk_start))
    fill_seq, cand_seq = trk_seq[fill_trk[:nf]], trk_seq[cand_a[:nc]]
    out = []
    for s, (a, ids, cnt) in enumerate(seqs):
        t0, t1 = int(seq_trk_start[s]), int(seq_trk_start[s + 1])
        new_id = ids[root[t0:t1] - t0]
        rows = a.copy()
        rows[:, 1] = np.repeat(new_id, cnt)
        fsel = np.nonzero(fill_seq == s)[0]
        fill = np.empty((len(fsel), 6), np.float64)
        fill[:, 0] = fill_frame[fsel]
        fill[:, 1] = new_id[fill_trk[fsel] - t0]
        fill[:, 2:] = fill_box[fsel]
        rows = np.concatenate([rows, fill])
        rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
        links = [(int(ids[k]), int(ids[succ[t0 + k] - t0]), int(first[succ[t0 + k]] - last[t0 + k]), float(link_d2[t0 + k]))
                 for k in range(t1 - t0) if succ[t0 + k] >= 0]
        rec = {"rows": rows, "id_map": {int(i): int(n) for i, n in zip(ids, new_id)}, "links": links, "n_tracks_before": t1 - t0,
               "n_tracks_after": int(len(np.unique(new_id))), "fill": fill, "cost": float(seq_cost[s])}
        assert len(links) == int(seq_links[s])
        if return_candidates:
            rec["candidates"] = [(int(ids[cand_a[i] - t0]), int(ids[cand_b[i] - t0]), int(first[cand_b[i]] - last[cand_a[i]]),
                                  float(cand_d2[i]), (float(cand_p[i, 0]), float(cand_p[i, 1]))) for i in np.nonzero(cand_seq == s)[0]]
        out.append(rec)
    return out


def history_to_rows(tracks_history) -> np.ndarray:
    """``{track_id: [(frame, x, y, w, h), ...]}`` -> ``(n, 6)`` rows ``frame, id, x, y, w, h``."""
    rows = [[float(r[0]), float(tid), float(r[1]), float(r[2]), float(r[3]), float(r[4])] for tid, trail in tracks_history.items() for r in trail]
    return np.array(rows, np.float64).reshape(-1, 6)


def rows_to_history(rows) -> dict:
    """The inverse: ``{track_id: [(frame, x, y, w, h), ...]}``, every trail in frame order, frames and ids as ints."""
    rows = np.asarray(rows, np.float64).reshape(-1, 6)
    out: dict = {}
    for r in rows[np.lexsort((rows[:, 0], rows[:, 1]))]:
        out.setdefault(int(r[1]), []).append((int(r[0]), float(r[2]), float(r[3]), float(r[4]), float(r[5])))
    return out


def correct_id_switches(tracks_history, max_gap=30, max_dist=20, *, device="cuda:0") -> dict:
    """TECHNICAL_DESIGN_DOCUMENT.md G.2's signature, a thin adapter over :func:`stitch_tracks`: ``tracks_history`` maps
    ``{track_id: [(frame, x, y, w, h), ...]}``; the result has the same shape with the fragments merged under the
    surviving ids."""
    rec = stitch_tracks([history_to_rows(tracks_history)], max_gap=max_gap, max_dist=float(max_dist), device=device)[0]
    return rows_to_history(rec["rows"])
