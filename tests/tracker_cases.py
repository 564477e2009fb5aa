"""Deterministic scenes for the ByteTrack kernel's limit tests (NumPy only: no GPU, no package import).

tests/test_tracker_cases_cpu.py proves on the oracle that each scene reaches the condition it was built for (lane width,
tie and contention counts, more than 1024 tracks / detections, mixed expiry); tests/test_gpu_tracker_limits.py feeds the same
arrays to the kernel.  All coordinates are multiples of 1/4 px below 2^13, so the shifts and drifts below are exact in float32.
"""
import numpy as np

F32 = np.float32
TRACK_THRESH = 0.5            # the tracker's defaults (tracker.py:46-47)
DRIFT_X = np.array([1, 0, 1, 0], np.float32)
PITCH = 96.0                  # grid pitch: a box (<= 40 px) plus its in-cell offset (<= 4 px) stays below PITCH / 2

# the tie scenes of test A with the lane width each must produce, and the two column-bound shapes (rows, columns)
TIE_SIZES = (12, 30, 60, 120, 250, 500, 1000, 1500)
TIE_WIDTHS = (16, 32, 16, 8, 4, 2, 1, 1)
COLUMN_BOUND = ((5, 40, 64), (300, 3, 2))
TIE_SIZES_PASS2 = (30, 250, 1500)


def lane_width(n_rows, n_cols):
    """Lanes that share one row in an association pass.  Mirrors the choice in csrc/tracker.hip:assoc_pass and
    csrc/track_dev.h:assoc_sparse (1024 threads): if either changes, re-check that the scenes here still cover every width."""
    r = 64
    while r > 1 and (n_rows * r > 1024 or (r >> 1) >= n_cols):
        r >>= 1
    return r


def _quarter(a):
    return (np.round(np.asarray(a, np.float64) * 4) / 4).astype(F32)


def grid_boxes(m, rng, origin=(0.0, 0.0)):
    """m boxes of 28..40 px, one per cell of a PITCH-px grid: the IoU of two distinct boxes is exactly 0."""
    side = int(np.ceil(np.sqrt(m)))
    cell = rng.permutation(side * side)[:m]
    x = (cell % side) * PITCH + rng.uniform(0, 4, m) + origin[0]
    y = (cell // side) * PITCH + rng.uniform(0, 4, m) + origin[1]
    w, h = rng.uniform(28, 40, m), rng.uniform(28, 40, m)
    return _quarter(np.stack([x, y, x + w, y + h], axis=1))


def _confidences(n, rng, low_share):
    conf = rng.uniform(0.6, 0.95, n).astype(F32)
    low = rng.random(n) < low_share
    conf[low] = rng.uniform(0.1, 0.45, int(low.sum())).astype(F32)
    return conf


def tie_scene(m, rng, low_share=0.0):
    """(tracks, dets, conf).  The last m // 6 tracks are exact copies of the first ones: both rows of such a pair have the same
    arg-max column (a contested column; the smaller row must win it and the other stay unmatched).  The detections are the
    distinct tracks moved by exactly 0.5 px in x and y (IoU >= 0.8), plus m // 5 exact duplicates of some of them (a tie row:
    the row maximum sits in two columns and the lower column must win), in a random order.  With ``low_share`` that share of
    the detections falls below ``TRACK_THRESH``, so ties and contested columns also occur in the second pass."""
    dup_t, dup_d = m // 6, m // 5
    distinct = grid_boxes(m - dup_t, rng)
    tracks = np.concatenate([distinct, distinct[:dup_t]]).astype(F32)
    moved = distinct + F32(0.5)
    dets = np.concatenate([moved, moved[rng.permutation(len(moved))[:dup_d]]]).astype(F32)
    dets = dets[rng.permutation(len(dets))]
    return tracks, dets, _confidences(len(dets), rng, low_share)


def column_bound_scene(n_rows, n_cols, rng):
    """(tracks, dets, conf) with exactly n_rows tracks and n_cols detections, for the shapes whose lane width is set by the
    column count.  Track n_rows - 1 is a copy of track 0 (one contested column).  Few columns (< 8): every detection is the same
    moved copy of track 0, so row 0 ties over all columns.  Otherwise each of the first four tracks gets a moved detection and
    an exact duplicate of it, and the remaining detections lie on a far grid that overlaps no track."""
    distinct = grid_boxes(n_rows - 1, rng)
    tracks = np.concatenate([distinct, distinct[:1]]).astype(F32)
    if n_cols < 8:
        dets = np.repeat(distinct[:1] + F32(0.5), n_cols, axis=0)
    else:
        moved = distinct[:4] + F32(0.5)
        far = grid_boxes(n_cols - 8, rng, origin=(4096.0, 4096.0))
        dets = np.concatenate([moved, moved, far]).astype(F32)
        dets = dets[rng.permutation(n_cols)]
    return tracks, dets.astype(F32), _confidences(n_cols, rng, 0.0)


def two_populations(n, rng, frames=8, low_share=1.0 / 3):
    """``frames`` frames (boxes, conf, cls).  Two disjoint grids of n boxes, A and B = A + 45 px in x, are fed on alternate
    frames and drift by +1 px in x per frame (IoU with the box of two frames earlier >= 26/30), so from the second frame on the
    state holds 2 n live tracks while no frame carries more than n detections.  From the third frame on ``low_share`` of the
    detections are low-confidence: the second pass then sees more than n unmatched tracks."""
    a = grid_boxes(n, rng)
    cls = rng.integers(0, 80, n).astype(np.int32)
    out = []
    for f in range(frames):
        b = a + DRIFT_X * F32(f)
        if f % 2:
            b = b + np.array([45, 0, 45, 0], F32)
        out.append((b.astype(F32), _confidences(n, rng, low_share if f >= 2 else 0.0), cls.copy()))
    return out


def churn_mask(n, frames, rng, drop_frames=(4, 5, 6, 7), share=1.0 / 3):
    """[frames, n] keep masks: on ``drop_frames`` a random ``share`` of the detections is missing.  With track_buffer = 2 a track
    of :func:`two_populations` (seen every other frame) expires as soon as it misses one of its own frames, and returns as a
    new track at the end of the list: the expiry compaction keeps and drops tracks all over the list."""
    keep = np.ones((frames, n), bool)
    for f in drop_frames:
        if f < frames:
            keep[f] = rng.random(n) >= share
    return keep


def churn_frames(n, rng, frames=12):
    seq = two_populations(n, rng, frames)
    keep = churn_mask(n, frames, rng)
    return [(b[k], c[k], s[k]) for (b, c, s), k in zip(seq, keep)]


def big_frames(rng, n=2080, frames=4, swap=0.1):
    """``frames`` frames of n > 2048 boxes, exactly n / 2 (> 1024) high and n / 2 low in each, interleaved; every frame
    ``swap`` of each half changes sides and all boxes drift by +1 px.  The first frame spawns more than 1024 tracks; later ones
    spawn the newly high boxes and send the newly low ones to the second pass."""
    boxes = grid_boxes(n, rng)
    cls = rng.integers(0, 80, n).astype(np.int32)
    high = np.zeros(n, bool)
    high[rng.permutation(n)[:n // 2]] = True
    out = []
    for f in range(frames):
        if f:
            k = int(n // 2 * swap)
            up, down = rng.permutation(np.nonzero(~high)[0])[:k], rng.permutation(np.nonzero(high)[0])[:k]
            high[up], high[down] = True, False
        conf = np.where(high, rng.uniform(0.6, 0.95, n), rng.uniform(0.1, 0.45, n)).astype(F32)
        out.append(((boxes + F32(f)).astype(F32), conf, cls.copy()))
    return out


def drift_frames(n, frames, rng, low_share=0.3, drop=0.2):
    """A small scene: n grid boxes drifting by +1 px in x per frame, ``low_share`` of the detections low-confidence and ``drop`` of
    them missing, independently in every frame."""
    boxes = grid_boxes(n, rng)
    cls = rng.integers(0, 80, n).astype(np.int32)
    out = []
    for f in range(frames):
        keep = rng.random(n) >= drop
        out.append(((boxes + DRIFT_X * F32(f))[keep].astype(F32), _confidences(n, rng, low_share)[keep], cls[keep]))
    return out


def tie_rng(m, low_share=0.0):
    """The generator of each committed tie scene.  The seeds 1 (m = 60) and 2 (m = 30, two passes) were picked so that the small
    scene holds a tie inside one lane, or ties in both passes; test_tracker_cases_cpu.py asserts it."""
    if low_share:
        return np.random.default_rng(2 if m == 30 else 0)
    return np.random.default_rng(1 if m == 60 else 0)


# the smallest handle of the suite: odd capacities, so no state array's size is a multiple of 16 bytes
SMALL_TRACKS, SMALL_DETS, SMALL_STREAMS, SMALL_FRAMES, SMALL_BUFFER = 7, 5, 3, 12, 2


def small_handle_frames(stream):
    """SMALL_FRAMES frames of stream ``stream`` for a SMALL_TRACKS x SMALL_DETS handle with track_buffer = SMALL_BUFFER: 40 x 60
    boxes moving right by 1 + stream px a frame, events shifted by ``stream`` frames.  A is there throughout; a second detection one
    pixel beside it in one frame makes a contested row, then a contested column, and a track that expires; B misses one frame (re-matched
    at 1 or 2 px a frame, lost and born again at 3) and comes in below the confidence threshold once (second pass); C leaves for
    good (expiry); D is born after that.  At most 4 detections a frame and 4 live tracks."""
    v, t0 = 1.0 + stream, stream
    frames = []
    for f in range(SMALL_FRAMES):
        e = f - t0                                               # the event clock of this stream
        x = 16.0 + v * f
        dets = [((x, 16.0 + 80 * stream), 0.9, 1)]                                   # A
        if e == 2:
            dets.append(((x + 1.0, 16.0 + 80 * stream), 0.625, 1))                     # beside A
        if e != 4:
            dets.append(((x + 96.0, 24.0), 0.375 if e == 7 else 0.875, 2))              # B
        if e < 6:
            dets.append(((x + 192.0, 32.0), 0.75, 3))                                # C
        if e >= 8:
            dets.append(((x + 288.0, 40.0), 0.8125, 4))                              # D
        b = np.asarray([[px, py, px + 40.0, py + 60.0] for (px, py), _, _ in dets], F32)
        frames.append((b, np.asarray([c for _, c, _ in dets], F32), np.asarray([k for _, _, k in dets], np.int32)))
    return frames
