"""Sliced inference (csrc/slice.hip) restated in plain NumPy / Python: the definition the GPU tests hold
the kernels to, bit for bit.  Float operations are float32, one per line; loops, no vectorised cleverness.  Slow by design."""
import numpy as np

from oracle import yolo_oracle as Y

F32 = np.float32
MAX_TILES = 64
NMM, NMS = "nmm", "nms"
IOS, IOU = "ios", "iou"


# ------------------------------------------------------------------ grid
def axis(L, t, o):
    """Positions along one axis and the effective tile."""
    assert L >= 1 and t >= 1 and 0 <= o < t
    te = min(t, L)
    step = te - o
    if step <= 0:
        return [0], te
    pos = []
    k = 0
    while True:
        p = min(k * step, L - te)
        pos.append(p)
        if p + te >= L:
            break
        k += 1
    return pos, te


def grid(frame_w, frame_h, tile_w, tile_h, overlap_w, overlap_h):
    """([(x, y), ...] row-major: y outer, x inner), (te_w, te_h)."""
    xs, te_w = axis(frame_w, tile_w, overlap_w)
    ys, te_h = axis(frame_h, tile_h, overlap_h)
    tiles = [(x, y) for y in ys for x in xs]
    assert len(tiles) <= MAX_TILES
    return tiles, (te_w, te_h)


# ------------------------------------------------------------------ gather
def gather(frames, tile_w, tile_h, overlap_w, overlap_h, overview=True):
    """frames [n, H, W, 3] uint8 -> images [n * I, te_h, te_w, 3]: per frame its tiles, then the letterboxed overview."""
    out = []
    for f in frames:
        H, W = f.shape[:2]
        tiles, (te_w, te_h) = grid(W, H, tile_w, tile_h, overlap_w, overlap_h)
        for x, y in tiles:
            out.append(np.ascontiguousarray(f[y:y + te_h, x:x + te_w]))
        if overview:
            lb = Y.letterbox(np.ascontiguousarray(f), te_h, te_w)[0]
            assert lb.shape == (te_h, te_w, 3)
            out.append(lb)
    return np.stack(out)


# ------------------------------------------------------------------ to frame coordinates
def _clip(v, hi):
    v = F32(v)
    if v < F32(0):
        v = F32(0)
    if v > F32(hi):
        v = F32(hi)
    return v


def overview_geometry(frame_w, frame_h, te_w, te_h):
    """(gain, pad_x, pad_y) of scale_boxes (oracle/yolo_oracle.py:457-468): computed in double, used as float32."""
    gain = min(te_h / frame_h, te_w / frame_w)
    pad_x = Y._round_half_even((te_w - frame_w * gain) / 2 - 0.1)
    pad_y = Y._round_half_even((te_h - frame_h * gain) / 2 - 0.1)
    return F32(gain), F32(pad_x), F32(pad_y)


def to_frame(images, frame_w, frame_h, tile_w, tile_h, overlap_w, overlap_h, overview=True):
    """images: the I per-image detections (xyxy [k, 4], conf [k], cls [k]) of ONE frame -> candidates in frame coordinates:
    a list of (box float32[4], conf float32, cls int, image j, slot), in image-then-slot order."""
    tiles, (te_w, te_h) = grid(frame_w, frame_h, tile_w, tile_h, overlap_w, overlap_h)
    T = len(tiles)
    assert len(images) == T + (1 if overview else 0)
    gain, pad_x, pad_y = overview_geometry(frame_w, frame_h, te_w, te_h)
    cands = []
    for j, (xyxy, conf, cls) in enumerate(images):
        for slot in range(len(conf)):
            b = [F32(v) for v in xyxy[slot]]
            if j < T:
                ox = F32(tiles[j][0])
                oy = F32(tiles[j][1])
                b[0] = F32(b[0] + ox)
                b[2] = F32(b[2] + ox)
                b[1] = F32(b[1] + oy)
                b[3] = F32(b[3] + oy)
            else:
                b[0] = F32(b[0] - pad_x)
                b[2] = F32(b[2] - pad_x)
                b[1] = F32(b[1] - pad_y)
                b[3] = F32(b[3] - pad_y)
                b[0] = F32(b[0] / gain)
                b[1] = F32(b[1] / gain)
                b[2] = F32(b[2] / gain)
                b[3] = F32(b[3] / gain)
            b[0] = _clip(b[0], frame_w)
            b[2] = _clip(b[2], frame_w)
            b[1] = _clip(b[1], frame_h)
            b[3] = _clip(b[3], frame_h)
            cands.append((np.array(b, F32), F32(conf[slot]), int(cls[slot]), j, slot))
    return cands


# ------------------------------------------------------------------ merge
def _area(b):
    w = F32(b[2] - b[0])
    h = F32(b[3] - b[1])
    return F32(w * h)


def matches(a, b, metric, thresh):
    """The pair metric of boxes a, b (float32 [4]) is strictly above thresh, its denominator positive."""
    iw = F32(min(a[2], b[2]) - max(a[0], b[0]))
    ih = F32(min(a[3], b[3]) - max(a[1], b[1]))
    if iw < F32(0):
        iw = F32(0)
    if ih < F32(0):
        ih = F32(0)
    inter = F32(iw * ih)
    aa = _area(a)
    ab = _area(b)
    if metric == IOU:
        den = F32(aa + ab)
        den = F32(den - inter)
    else:
        den = min(aa, ab)
    if not den > F32(0):
        return False
    return bool(F32(inter / den) > F32(thresh))


def merge(cands, mode=NMM, metric=IOS, thresh=0.5, agnostic=False, max_out=300):
    """cands: to_frame's list for one frame -> (xyxy [k, 4], conf [k], cls [k], n_merged [k]) of the first max_out keepers."""
    order = sorted(range(len(cands)), key=lambda i: (-float(cands[i][1]), cands[i][3], cands[i][4]))
    live = [True] * len(order)
    out_b, out_c, out_k, out_n = [], [], [], []
    for pi, i in enumerate(order):
        if not live[pi]:
            continue
        if len(out_b) == max_out:
            break
        kb, kc, kk = cands[i][0], cands[i][1], cands[i][2]
        u = kb.copy()
        n = 0
        for pj in range(pi + 1, len(order)):
            if not live[pj]:
                continue
            b, _, ck = cands[order[pj]][:3]
            if not agnostic and ck != kk:
                continue
            if matches(kb, b, metric, thresh):                 # always against the keeper's ORIGINAL box
                live[pj] = False
                n += 1
                if mode == NMM:
                    if b[0] < u[0]:
                        u[0] = b[0]
                    if b[1] < u[1]:
                        u[1] = b[1]
                    if b[2] > u[2]:
                        u[2] = b[2]
                    if b[3] > u[3]:
                        u[3] = b[3]
        out_b.append(u if mode == NMM else kb.copy())
        out_c.append(kc)
        out_k.append(kk)
        out_n.append(n)
    k = len(out_b)
    return (np.array(out_b, F32).reshape(k, 4), np.array(out_c, F32).reshape(k), np.array(out_k, np.int32).reshape(k),
            np.array(out_n, np.int32).reshape(k))
