"""NumPy restatement of csrc/jpeg.hip: a baseline JPEG (T.81 sequential DCT, Huffman, 8-bit, YCbCr 4:2:0, JFIF) of one BGR24
frame, in the integer arithmetic the kernel's header comment states.  `encode` must equal the kernel's output byte for byte.

Stream: SOI, JFIF APP0, DQT (luminance), DQT (chrominance), SOF0 (Y 2x2, Cb 1x1, Cr 1x1), DHT x 4 (Annex K tables: DC0, AC0, DC1,
AC1), DRI (one MCU row), SOS, the interleaved scan with RSTm between MCU rows, EOI.

Rules (libjpeg's, so that libjpeg-turbo can be compared with bit for bit):
  quantisation tables  Annex K scaled by  s = q < 50 ? 5000 / q : 200 - 2q,  (base * s + 50) / 100  clamped to 1..255;
  colour               Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
                       Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
                       Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16;
  edges                a pixel right of or below the frame is the pixel at the clamped coordinate (last column / row replicated);
  chroma               2 x 2 box sum, (sum + bias) >> 2, bias 1, 2, 1, 2 ... along a row; a chroma row below ceil(h / 2) - 1 is a
                       copy of that row (libjpeg pads the down-sampled rows, not the pixels: it matters when h is even);
  forward DCT          Loeffler-Ligtenberg-Moschytz, 13-bit constants, 2 extra bits after the row pass, samples - 128, output x 8;
  quantisation         sign(c) * ((|c| + 4 q) / (8 q)), clamped to -1024..1023 (the clamp never acts on 8-bit samples);
  dummy blocks         a luminance block wholly outside ceil(w / 8) x ceil(h / 8) blocks has zero AC and the DC of the block
                       before it in its MCU (libjpeg's jccoefct.c): right edge DC1 = DC0, DC3 = DC2; bottom edge DC2 = DC3 = DC1;
  entropy coding       every restart interval (one MCU row) starts byte-aligned with DC predictors 0, is padded with 1-bits,
                       FF -> FF 00 inside it, RST(m mod 8) after interval m except the last.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                     99, 99] + [99] * 32)


def _run(*spans):
    out = []
    for a, b in spans:
        out += list(range(a, b + 1))
    return out


DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = list(bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f024336272820"
                                  "90a161718191a25262728292a3435363738393a")) + _run(
    (0x43, 0x4a), (0x53, 0x5a), (0x63, 0x6a), (0x73, 0x7a), (0x83, 0x8a), (0x92, 0x9a), (0xa2, 0xaa), (0xb2, 0xba), (0xc2, 0xca),
    (0xd2, 0xda), (0xe1, 0xea), (0xf1, 0xfa))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = list(bytes.fromhex("0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f1"
                                    "1718191a262728292a35363738393a".replace(" ", ""))) + _run(
    (0x43, 0x4a), (0x53, 0x5a), (0x63, 0x6a), (0x73, 0x7a), (0x82, 0x8a), (0x92, 0x9a), (0xa2, 0xaa), (0xb2, 0xba), (0xc2, 0xca),
    (0xd2, 0xda), (0xe2, 0xea), (0xf2, 0xfa))
assert len(AC_LUMA_VALS) == sum(AC_LUMA_BITS) == 162 and len(AC_CHROMA_VALS) == sum(AC_CHROMA_BITS) == 162


def quant_tables(quality):
    """(luminance, chrominance) in natural order, libjpeg's jpeg_set_quality."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255).astype(np.int64) for t in (LUMA_Q, CHROMA_Q))


def huff_table(bits, vals):
    """symbol -> (code, length) arrays of 256 entries (length 0: no code), T.81 Annex C."""
    code = np.zeros(256, np.int64)
    size = np.zeros(256, np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(quality, h, w):
    """Everything from SOI up to and including the SOS header (what rtmodt_jpeg_header returns)."""
    h, w = int(h), int(w)
    if not (1 <= h <= 8192 and 1 <= w <= 8192):
        raise ValueError(f"bad frame geometry {w}x{h}")
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist())) + _seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                           (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _seg(0xC4, bytes([tc]) + bytes(bits) + bytes(vals))
    out += _seg(0xDD, ((w + 15) // 16).to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


# ---- samples ----------------------------------------------------------------------------------------------------------------
def planes(frame_bgr):
    """BGR24 frame -> (Y [16 mh, 16 mw], Cb [8 mh, 8 mw], Cr), uint8 values as int64, padded to whole MCUs by clamping."""
    f = np.asarray(frame_bgr)
    if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
        raise ValueError("a frame is an H x W x 3 uint8 array")
    h, w = f.shape[:2]
    mh, mw = (h + 15) // 16, (w + 15) // 16
    yi = np.minimum(np.arange(16 * mh), h - 1)
    xi = np.minimum(np.arange(16 * mw), w - 1)
    p = f[yi][:, xi].astype(np.int64)
    B, G, R = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    bias = 1 + (np.arange(8 * mw) & 1)
    ci = np.minimum(np.arange(8 * mh), (h + 1) // 2 - 1)               # below the frame: the last chroma ROW again

    def down(c):
        return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias[None, :]) >> 2)[ci]
    return Y, down(Cb), down(Cr)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_1d(d, first):
    """One pass of jfdctint.c over the last axis of d [..., 8]."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def fdct_quant(plane, q):
    """plane [8 bh, 8 bw] of uint8 values, q [64] natural order -> quantised coefficients [bh, bw, 64] in zigzag order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128          # [bh, bw, row, col]
    r = _dct_1d(b, True)
    c = _dct_1d(r.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)                      # columns
    c = c.reshape(bh, bw, 64)
    d = 8 * q[None, None, :]
    v = np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    return np.clip(v, -1024, 1023)[..., ZIGZAG]


def coefficients(frame_bgr, quality):
    """[mh, mw, 6, 64]: per MCU the blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag order, dummy-block rule applied."""
    h, w = frame_bgr.shape[:2]
    ql, qc = quant_tables(quality)
    Y, Cb, Cr = planes(frame_bgr)
    mh, mw = Y.shape[0] // 16, Y.shape[1] // 16
    y = fdct_quant(Y, ql).reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64).copy()
    hb, wb = (h + 7) // 8, (w + 7) // 8
    if wb % 2:                                           # right edge: the second block column of the last MCU is outside
        y[:, -1, 1, 1:] = 0
        y[:, -1, 3, 1:] = 0
        y[:, -1, 1, 0] = y[:, -1, 0, 0]
        y[:, -1, 3, 0] = y[:, -1, 2, 0]
    if hb % 2:                                           # bottom edge: the second block row of the last MCU row is outside
        y[-1, :, 2:, 1:] = 0
        y[-1, :, 2, 0] = y[-1, :, 1, 0]
        y[-1, :, 3, 0] = y[-1, :, 1, 0]
    return np.concatenate([y, fdct_quant(Cb, qc)[:, :, None, :], fdct_quant(Cr, qc)[:, :, None, :]], axis=2)


# ---- entropy coding ---------------------------------------------------------------------------------------------------------
_HUFF = None


def _huff():
    global _HUFF
    if _HUFF is None:
        _HUFF = (huff_table(DC_LUMA_BITS, DC_VALS), huff_table(AC_LUMA_BITS, AC_LUMA_VALS), huff_table(DC_CHROMA_BITS, DC_VALS),
                 huff_table(AC_CHROMA_BITS, AC_CHROMA_VALS))
    return _HUFF


def _nbits(a):
    a = np.abs(a)
    n = np.zeros(a.shape, np.int64)
    for k in range(12):
        n += a >= (1 << k)
    return n


def _value_bits(v, n):
    return np.where(v < 0, v - 1, v) & ((1 << n) - 1)


def scan_intervals(coef):
    """coef [mh, mw, 6, 64] -> one bytes object per restart interval (padded with 1-bits, FF stuffed)."""
    mh, mw = coef.shape[:2]
    (dcl_c, dcl_s), (acl_c, acl_s), (dcc_c, dcc_s), (acc_c, acc_s) = _huff()
    nb = mw * 6
    blk = coef.reshape(mh, nb, 64).astype(np.int64)
    comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), mw)                       # component of each block of an interval
    chroma = comp > 0
    # DC differences: predictor = the previous block of the same component in the interval, 0 at its start
    dc = blk[:, :, 0]
    diff = np.zeros_like(dc)
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        d = dc[:, idx]
        diff[:, idx] = d - np.concatenate([np.zeros((mh, 1), np.int64), d[:, :-1]], axis=1)
    # tokens: every block owns 2 (DC) + 63 * 5 (3 ZRL, code, bits) + 1 (EOB) slots of (value, length); empty slots have length 0
    nblk = mh * nb
    ac = blk[:, :, 1:].reshape(nblk, 63)
    chroma_b = np.tile(chroma, mh)
    b_i, k_i = np.nonzero(ac)
    v = ac[b_i, k_i]
    first = np.ones(len(b_i), bool)
    first[1:] = b_i[1:] != b_i[:-1]
    prev = np.where(first, -1, np.concatenate([[0], k_i[:-1]]))
    run = k_i - prev - 1
    n = _nbits(v)
    sym = ((run & 15) << 4) | n
    ch = chroma_b[b_i]
    code = np.where(ch, acc_c[sym], acl_c[sym])
    size = np.where(ch, acc_s[sym], acl_s[sym])
    zrl_c, zrl_s = np.where(ch, acc_c[0xF0], acl_c[0xF0]), np.where(ch, acc_s[0xF0], acl_s[0xF0])
    SL = 2 + 63 * 5 + 1
    tv = np.zeros((nblk, SL), np.int32)
    tl = np.zeros((nblk, SL), np.uint8)
    base = 2 + 5 * k_i
    for z in range(3):
        m = (run >> 4) > z
        tv[b_i[m], base[m] + z] = zrl_c[m]
        tl[b_i[m], base[m] + z] = zrl_s[m]
    tv[b_i, base + 3], tl[b_i, base + 3] = code, size
    tv[b_i, base + 4], tl[b_i, base + 4] = _value_bits(v, n), n
    last = np.full(nblk, -1, np.int64)
    last[b_i] = k_i                                                          # (ascending k: the last write wins)
    eob = last < 62
    tv[eob, SL - 1] = np.where(chroma_b, acc_c[0], acl_c[0])[eob]
    tl[eob, SL - 1] = np.where(chroma_b, acc_s[0], acl_s[0])[eob]
    dflat = diff.reshape(nblk)
    dn = _nbits(dflat)
    tv[:, 0], tl[:, 0] = np.where(chroma_b, dcc_c[dn], dcl_c[dn]), np.where(chroma_b, dcc_s[dn], dcl_s[dn])
    tv[:, 1], tl[:, 1] = _value_bits(dflat, dn), dn
    out = []
    tv, tl = tv.reshape(mh, nb * SL), tl.reshape(mh, nb * SL)
    for r in range(mh):
        keep = tl[r] > 0
        val, ln = tv[r][keep].astype(np.int64), tl[r][keep].astype(np.int64)
        total = int(ln.sum())
        end = np.cumsum(ln)
        owner = np.repeat(np.arange(len(ln)), ln)                             # token of every bit
        shift = end[owner] - 1 - np.arange(total)                             # bit position inside its token, MSB first
        bits = ((val[owner] >> shift) & 1).astype(np.uint8)
        bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
        out.append(np.packbits(bits).tobytes().replace(b"\xff", b"\xff\x00"))
    return out


def scan(coef):
    """The entropy-coded segment: intervals joined by RST markers (no SOS header, no EOI)."""
    parts = scan_intervals(coef)
    out = bytearray()
    for m, p in enumerate(parts):
        out += p
        if m + 1 < len(parts):
            out += bytes([0xFF, 0xD0 + (m & 7)])
    return bytes(out)


def encode(frame_bgr, quality=95):
    """The complete JPEG file of one frame."""
    frame_bgr = np.asarray(frame_bgr)
    h, w = frame_bgr.shape[:2]
    return header(quality, h, w) + scan(coefficients(frame_bgr, quality)) + b"\xff\xd9"


# ---- helpers for tests ------------------------------------------------------------------------------------------------------
def split(jpeg):
    """(header up to and including SOS, entropy-coded bytes, number of RST markers) of a baseline JPEG with one scan."""
    d = bytes(jpeg)
    assert d[:2] == b"\xff\xd8" and d[-2:] == b"\xff\xd9"
    i = 2
    while True:
        assert d[i] == 0xFF, i
        m, L = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        i += 2 + L
        if m == 0xDA:
            break
    body = d[i:-2]
    a = np.frombuffer(body, np.uint8)
    pos = np.nonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7))[0]
    return d[:i], body, [int(a[p + 1]) - 0xD0 for p in pos]


def segments(jpeg):
    """[(marker, payload)] of the header segments up to and including SOS."""
    d = bytes(jpeg)
    i, out = 2, []
    while True:
        m, L = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        out.append((m, d[i + 4:i + 2 + L]))
        i += 2 + L
        if m == 0xDA:
            return out
