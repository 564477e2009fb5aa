"""NumPy / plain-Python restatement of the baseline JPEG decoder in csrc/jpeg_dec_core.h (stream rules) and csrc/jpeg_dec.hip
(pixels).  ``parse`` / ``coefficients`` / ``decode`` must equal the library for every stream, accepted or rejected; ``decode``
equals libjpeg-turbo's default decoder (Pillow) byte for byte on accepted streams (tests/test_jpeg_dec_cpu.py).

Stream rules
  accepted     SOF0, 8-bit samples, 8-bit quantisation tables, 1 or 3 components, one interleaved scan over all components
               (Ss 0, Se 63, Ah = Al = 0), luminance sampling 1x1 / 2x1 / 2x2 with 1x1 chrominance, at most four distinct Huffman
               tables in the scan, any DRI, sides 1..8192.  A single component is decoded as 1x1 whatever its factors say.
               A scan that names a Huffman table no DHT defined uses the Annex K table of that class and number (0 / 1): AVI MJPG.
  UNSUPPORTED  every other SOF, DAC, 12-bit or other precisions, 16-bit quantisation tables, 4 or 2 components, other
               sampling, several scans (SOS with fewer components than the frame), spectral selection / approximation, sides
               above 8192, Adobe APP14 with transform 0 on three components.
  CORRUPT      broken marker structure, bad segment lengths, a DHT that is no prefix code, undefined quantisation table, missing SOF.
  TRUNCATED    the file ends inside the header.
  scan         [end of the SOS header, end of file), without a closing FF D9.  Every FF D0..D7 pair inside it ends a restart
               interval; their number must be ceil(MCUs / Ri) - 1 (0 without DRI) and the m-th must be RST(m mod 8): else CORRUPT.
  interval     decoded by itself, DC predictors 0 at its start.  Its bits are its bytes with FF 00 -> FF, up to the first FF that is
               not followed by 00 (or its end); behind them the reader supplies zero bits.  A Huffman code that does not resolve in
               16 bits, a DC category above 11, an AC category above 10 or a coefficient index above 63 stops the interval: CORRUPT.
               An interval that consumed a supplied zero bit is TRUNCATED.  The frame's status is the largest of its intervals'.
Pixels: libjpeg's jidctint.c (islow), jdsample.c with fancy upsampling, jdcolor.c -- see the functions below.
"""
import numpy as np

OK, UNSUPPORTED, CORRUPT, TRUNCATED, SIZE_MISMATCH = 0, 1, 2, 3, 4
STATUS_NAMES = ["OK", "UNSUPPORTED", "CORRUPT", "TRUNCATED", "SIZE_MISMATCH"]
MAX_DIM = 8192

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]


def _run(*spans):
    out = []
    for a, b in spans:
        out += list(range(a, b + 1))
    return out


# T.81 Annex K.3 (what libjpeg installs when a scan names a table no DHT defined)
_AC_TAIL = [(0x43, 0x4a), (0x53, 0x5a), (0x63, 0x6a), (0x73, 0x7a)]
STD_TABLES = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
             list(bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a"
                                "3435363738393a")) + _run(*_AC_TAIL, (0x83, 0x8a), (0x92, 0x9a), (0xa2, 0xaa), (0xb2, 0xba), (0xc2, 0xca),
                                                          (0xd2, 0xda), (0xe1, 0xea), (0xf1, 0xfa))),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             list(bytes.fromhex("0001020311040521310612415107617113223281081442" "91a1b1c109233352f0156272d10a162434e125f1"
                                "1718191a262728292a35363738393a")) + _run(*_AC_TAIL, (0x82, 0x8a), (0x92, 0x9a), (0xa2, 0xaa), (0xb2, 0xba),
                                                                        (0xc2, 0xca), (0xd2, 0xda), (0xe2, 0xea), (0xf2, 0xfa))),
}
assert all(sum(b) == len(v) for b, v in STD_TABLES.values())


class JpegError(Exception):
    """A stream the decoder rejects; ``status`` is one of the codes above."""

    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES[status]}: {message}")
        self.status = status
        self.message = message


class Header:
    """What ``parse`` returns: geometry, per-component sampling / table numbers, tables, restart interval, the scan's byte range."""


def valid_prefix_code(bits):
    """libjpeg's jdhuff.c test: while codes are handed out in order, a code of length l must stay below 2^l."""
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            return False
        code <<= 1
    return True


def parse(file):
    d = bytes(file)
    n = len(d)
    if n < 2:
        raise JpegError(TRUNCATED, "no SOI")
    if d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError(CORRUPT, "no SOI")
    H = Header()
    H.qt = [None] * 4                                 # natural order
    H.huff = {}                                       # (class, id) -> (bits[16], vals)
    H.ri = 0
    H.comps = None
    adobe_transform = -1
    i = 2
    while True:
        if i >= n:
            raise JpegError(TRUNCATED, "the file ends before SOS")
        if d[i] != 0xFF:
            raise JpegError(CORRUPT, f"byte {i}: no marker")
        while i < n and d[i] == 0xFF:                 # fill bytes
            i += 1
        if i >= n:
            raise JpegError(TRUNCATED, "the file ends before SOS")
        m = d[i]
        i += 1
        if m == 0x00 or m == 0x01 or 0xD0 <= m <= 0xD9:
            raise JpegError(CORRUPT, f"marker FF {m:02X} in the header")
        if i + 2 > n:
            raise JpegError(TRUNCATED, "the file ends inside a segment")
        L = d[i] << 8 | d[i + 1]
        if L < 2:
            raise JpegError(CORRUPT, f"segment FF {m:02X} of length {L}")
        if i + L > n:
            raise JpegError(TRUNCATED, "the file ends inside a segment")
        p = d[i + 2:i + L]
        i += L
        if m == 0xC0:
            if H.comps is not None:
                raise JpegError(CORRUPT, "two SOF segments")
            if len(p) < 6:
                raise JpegError(CORRUPT, "short SOF")
            prec, H.h, H.w, nc = p[0], p[1] << 8 | p[2], p[3] << 8 | p[4], p[5]
            if prec != 8:
                raise JpegError(UNSUPPORTED, f"{prec}-bit samples")
            if nc == 4:
                raise JpegError(UNSUPPORTED, "4 components")
            if nc not in (1, 3):
                raise JpegError(UNSUPPORTED, f"{nc} components")
            if len(p) != 6 + 3 * nc:
                raise JpegError(CORRUPT, "SOF length")
            if H.h == 0 or H.w == 0:
                raise JpegError(CORRUPT, "empty frame")
            if H.h > MAX_DIM or H.w > MAX_DIM:
                raise JpegError(UNSUPPORTED, f"frame {H.w}x{H.h} above {MAX_DIM}")
            comps = []
            for c in range(nc):
                cid, hv, tq = p[6 + 3 * c:9 + 3 * c]
                hs, vs = hv >> 4, hv & 15
                if not (1 <= hs <= 4 and 1 <= vs <= 4):
                    raise JpegError(CORRUPT, "sampling factor outside 1..4")
                if tq > 3:
                    raise JpegError(CORRUPT, "quantisation table number")
                comps.append([cid, hs, vs, tq, 0, 0])
            if nc == 1:
                comps[0][1] = comps[0][2] = 1
            elif (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any(c[1] != 1 or c[2] != 1 for c in comps[1:]):
                raise JpegError(UNSUPPORTED, "sampling " + " ".join(f"{c[1]}x{c[2]}" for c in comps))
            H.comps = comps
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            kind = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xCC: "arithmetic coding"}.get(
                m, "arithmetic-coded" if m > 0xC8 else "differential")
            raise JpegError(UNSUPPORTED, f"{kind} (FF {m:02X})")
        elif m == 0xDB:
            k = 0
            while k < len(p):
                pq, tq = p[k] >> 4, p[k] & 15
                if pq == 1:
                    raise JpegError(UNSUPPORTED, "16-bit quantisation table")
                if pq > 1 or tq > 3 or k + 65 > len(p):
                    raise JpegError(CORRUPT, "DQT")
                t = [0] * 64
                for z in range(64):
                    t[ZIGZAG[z]] = p[k + 1 + z]
                H.qt[tq] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(p):
                tc, th = p[k] >> 4, p[k] & 15
                if tc > 1 or th > 3 or k + 17 > len(p):
                    raise JpegError(CORRUPT, "DHT")
                bits = list(p[k + 1:k + 17])
                cnt = sum(bits)
                if cnt > 256 or k + 17 + cnt > len(p):
                    raise JpegError(CORRUPT, "DHT")
                if not valid_prefix_code(bits):
                    raise JpegError(CORRUPT, "DHT is no prefix code")
                H.huff[(tc, th)] = (bits, list(p[k + 17:k + 17 + cnt]))
                k += 17 + cnt
        elif m == 0xDD:
            if len(p) != 2:
                raise JpegError(CORRUPT, "DRI")
            H.ri = p[0] << 8 | p[1]
        elif m == 0xEE:
            if len(p) >= 12 and p[:5] == b"Adobe":
                adobe_transform = p[11]
        elif m == 0xDA:
            if H.comps is None:
                raise JpegError(CORRUPT, "SOS before SOF")
            nc = len(H.comps)
            if len(p) < 1:
                raise JpegError(CORRUPT, "SOS")
            ns = p[0]
            if ns < 1 or ns > 4 or len(p) != 4 + 2 * ns:
                raise JpegError(CORRUPT, "SOS")
            if ns != nc:
                raise JpegError(UNSUPPORTED, "multiple scans")
            for c in range(nc):
                cid, t = p[1 + 2 * c], p[2 + 2 * c]
                if cid != H.comps[c][0]:
                    raise JpegError(UNSUPPORTED, "scan component order")
                if (t >> 4) > 3 or (t & 15) > 3:
                    raise JpegError(CORRUPT, "Huffman table number")
                H.comps[c][4], H.comps[c][5] = t >> 4, t & 15
            if p[1 + 2 * ns] != 0 or p[2 + 2 * ns] != 63 or p[3 + 2 * ns] != 0:
                raise JpegError(UNSUPPORTED, "spectral selection / successive approximation")
            if nc == 3 and adobe_transform == 0:
                raise JpegError(UNSUPPORTED, "Adobe transform 0 (RGB)")
            slots = []
            for c in H.comps:
                if H.qt[c[3]] is None:
                    raise JpegError(CORRUPT, "undefined quantisation table")
                for key in ((0, c[4]), (1, c[5])):
                    if key in slots:
                        continue
                    if key not in H.huff:
                        if key not in STD_TABLES:
                            raise JpegError(CORRUPT, "undefined Huffman table")
                        H.huff[key] = STD_TABLES[key]
                    if len(slots) == 4:
                        raise JpegError(UNSUPPORTED, "more than four Huffman tables in one scan")
                    slots.append(key)
            H.slots = slots
            break
        # every other segment (APPn, COM, DNL ...) is skipped
    H.ncomp = len(H.comps)
    H.hs, H.vs = H.comps[0][1], H.comps[0][2]
    H.mcus_x, H.mcus_y = -(-H.w // (8 * H.hs)), -(-H.h // (8 * H.vs))
    H.scan_off = i
    H.scan_end = n - 2 if n - 2 >= i and d[n - 2:] == b"\xff\xd9" else n
    mcus = H.mcus_x * H.mcus_y
    H.intervals = -(-mcus // H.ri) if H.ri else 1
    return H


_LOOK = {}


def _lookup(bits, vals):
    """16-bit peek -> (length, symbol); length 0 where no code of up to 16 bits matches."""
    key = (tuple(bits), tuple(vals))
    if key not in _LOOK:
        ln = np.zeros(65536, np.uint8)
        sy = np.zeros(65536, np.uint8)
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                lo = code << (16 - length)
                ln[lo:lo + (1 << (16 - length))] = length
                sy[lo:lo + (1 << (16 - length))] = vals[k]
                code += 1
                k += 1
            code <<= 1
        _LOOK[key] = (ln.tolist(), sy.tolist())
    return _LOOK[key]


def _decode_interval(data, H, tabs, first_mcu, n_mcus, out):
    """One restart interval -> its status; nonzero coefficients go to out[c][by, bx, natural index]."""
    # the interval's bits: bytes up to the first FF that is not followed by 00, unstuffed
    raw = bytearray()
    k, n = 0, len(data)
    while k < n:
        b = data[k]
        if b == 0xFF:
            if k + 1 < n and data[k + 1] == 0:
                raw.append(0xFF)
                k += 2
                continue
            break
        raw.append(b)
        k += 1
    avail = 8 * len(raw)
    total = avail + 64
    val = int.from_bytes(bytes(raw) + b"\0" * 8, "big")
    pos = 0
    pred = [0] * H.ncomp
    status = OK

    def finish(st):
        return max(st, TRUNCATED if pos > avail else OK)

    for mcu in range(first_mcu, first_mcu + n_mcus):
        my, mx = divmod(mcu, H.mcus_x)
        for c, comp in enumerate(H.comps):
            (dl, ds), (al, as_) = tabs[c]
            for v in range(comp[2]):
                for h in range(comp[1]):
                    if pos > avail:                    # (only zero bits from here on)
                        return TRUNCATED
                    blk = out[c][my * comp[2] + v, mx * comp[1] + h]
                    peek = (val >> (total - pos - 16)) & 0xFFFF if pos + 16 <= total else 0
                    ln = dl[peek]
                    if ln == 0:
                        return finish(CORRUPT)
                    s = ds[peek]
                    pos += ln
                    if s > 11:
                        return finish(CORRUPT)
                    if s:
                        r = (val >> (total - pos - s)) & ((1 << s) - 1) if pos + s <= total else 0
                        pos += s
                        diff = r if r >= (1 << (s - 1)) else r - (1 << s) + 1
                        pred[c] = ((pred[c] + diff + 32768) & 0xFFFF) - 32768
                    blk[0] = pred[c]
                    kk = 1
                    while kk < 64:
                        peek = (val >> (total - pos - 16)) & 0xFFFF if pos + 16 <= total else 0
                        ln = al[peek]
                        if ln == 0:
                            return finish(CORRUPT)
                        rs = as_[peek]
                        pos += ln
                        r, s = rs >> 4, rs & 15
                        if s:
                            kk += r
                            if kk > 63 or s > 10:
                                return finish(CORRUPT)
                            x = (val >> (total - pos - s)) & ((1 << s) - 1) if pos + s <= total else 0
                            pos += s
                            blk[ZIGZAG[kk]] = x if x >= (1 << (s - 1)) else x - (1 << s) + 1
                            kk += 1
                        elif r == 15:
                            kk += 16
                        else:
                            break
    return finish(status)


def entropy_decode(file):
    """(header, per-component int16 [block rows, block cols, 64] natural order, status).  Raises ``JpegError`` for header errors only."""
    d = bytes(file)
    H = parse(d)
    out = [np.zeros((H.mcus_y * c[2], H.mcus_x * c[1], 64), np.int16) for c in H.comps]
    a = np.frombuffer(d, np.uint8)[H.scan_off:H.scan_end]
    marks = (np.nonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7))[0] + H.scan_off).tolist() if len(a) > 1 else []
    if len(marks) != H.intervals - 1:
        return H, out, CORRUPT
    tabs = [(_lookup(*H.huff[(0, c[4])]), _lookup(*H.huff[(1, c[5])])) for c in H.comps]
    mcus = H.mcus_x * H.mcus_y
    per = H.ri if H.ri else mcus
    status = OK
    for j in range(H.intervals):
        start = H.scan_off if j == 0 else marks[j - 1] + 2
        end = H.scan_end if j == H.intervals - 1 else marks[j]
        if j and (d[marks[j - 1] + 1] & 7) != (j - 1) & 7:
            status = max(status, CORRUPT)
            continue
        status = max(status, _decode_interval(d[start:end], H, tabs, j * per, min(per, mcus - j * per), out))
    return H, out, status


def coefficients(file):
    """Per component the int16 coefficients [block rows, block cols, 64] (whole MCUs), natural order, not dequantised."""
    H, out, status = entropy_decode(file)
    if status != OK:
        raise JpegError(status, "damaged scan")
    return out


def coefficient_hash(coefs):
    """sum over i of (uint16(v_i) + 1) * ((i + 1) * 0x9E3779B97F4A7C15) mod 2^64, i running over the int16 coefficients component after
    component: what jpeg_dec_check prints."""
    v = np.concatenate([np.ascontiguousarray(c, np.int16).reshape(-1) for c in coefs]).view(np.uint16).astype(np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        w = (np.arange(1, len(v) + 1, dtype=np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
        return int((v * w).sum(dtype=np.uint64))


def status_of(file):
    try:
        return entropy_decode(file)[2]
    except JpegError as e:
        return e.status


# ---- pixels -------------------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + np.int32(1 << (n - 1))) >> np.int32(n)


def _idct_1d(d, shift):
    """One pass of jidctint.c (islow) over the last axis of d [..., 8], int32 with wrap-around."""
    i32 = np.int32
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * i32(4433)
    tmp2 = z1 + z3 * i32(-15137)
    tmp3 = z1 + z2 * i32(6270)
    z2, z3 = d[..., 0], d[..., 4]
    tmp0, tmp1 = (z2 + z3) << i32(13), (z2 - z3) << i32(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * i32(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * i32(2446), tmp1 * i32(16819), tmp2 * i32(25172), tmp3 * i32(12299)
    z1, z2, z3, z4 = z1 * i32(-7373), z2 * i32(-20995), z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([_descale(tmp10 + tmp3, shift), _descale(tmp11 + tmp2, shift), _descale(tmp12 + tmp1, shift),
                     _descale(tmp13 + tmp0, shift), _descale(tmp13 - tmp0, shift), _descale(tmp12 - tmp1, shift),
                     _descale(tmp11 - tmp2, shift), _descale(tmp10 - tmp3, shift)], axis=-1)


def idct_raw(coef, qt):
    """coef [br, bc, 64] int16, qt [64] natural order -> int32 [br, bc, 8, 8] before the range limit (dequantise, islow IDCT)."""
    br, bc = coef.shape[:2]
    with np.errstate(over="ignore"):
        x = (coef.astype(np.int32) * np.asarray(qt, np.int32)[None, None, :]).reshape(br, bc, 8, 8)     # [.., row, col]
        ws = _idct_1d(x.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)                                 # columns: pass 1
        return _idct_1d(ws, 18)                                                                          # rows: pass 2


def idct_plane(coef, qt):
    """-> uint8 plane [8 br, 8 bc]: the result as a 10-bit two's-complement number, + 128, clamped to 0..255."""
    br, bc = coef.shape[:2]
    px = ((idct_raw(coef, qt) + 512) & 1023) - 512
    return np.clip(px + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(8 * br, 8 * bc)


def upsample(plane, ch, cw, hs, vs, h, w):
    """jdsample.c with do_fancy_upsampling: the component's real extent ch x cw -> h x w int64.  A component of real width <= 2 is
    replicated in both directions."""
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p[:h, :w]
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)[:h, :w]
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    if vs == 1:                                                                    # h2v1
        even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
        even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
        out = np.empty((ch, 2 * cw), np.int64)
        out[:, 0::2], out[:, 1::2] = even, odd
        return out[:h, :w]
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for par, nb in ((0, up), (1, down)):
        c = 3 * p + nb
        cl = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        cr = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        even, odd = (3 * c + cl + 8) >> 4, (3 * c + cr + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * c[:, 0] + 8) >> 4, (4 * c[:, -1] + 7) >> 4
        out[par::2, 0::2], out[par::2, 1::2] = even, odd
    return out[:h, :w]


def pixels(H, coefs):
    """uint8 [h, w, 3] BGR, or [h, w] for one component."""
    h, w = H.h, H.w
    planes = [idct_plane(coefs[c], H.qt[comp[3]]) for c, comp in enumerate(H.comps)]
    if H.ncomp == 1:
        return planes[0][:h, :w].copy()
    y = planes[0][:h, :w].astype(np.int64)
    ch, cw = -(-h // H.vs), -(-w // H.hs)
    cb = upsample(planes[1], ch, cw, H.hs, H.vs, h, w) - 128
    cr = upsample(planes[2], ch, cw, H.hs, H.vs, h, w) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def decode(file):
    H, coefs, status = entropy_decode(file)
    if status != OK:
        raise JpegError(status, "damaged scan")
    return pixels(H, coefs)
