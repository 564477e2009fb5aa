"""NumPy restatement of the 4:2:0 -> BGR conversion the engine implements (csrc/preprocess.hip: letterbox_yuv420_kernel):
OpenCV's integer BT.601 limited-range conversion as cv2.cvtColor(x, COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420) computes it,
chroma sample (x // 2, y // 2), no chroma interpolation.  Parity with cv2 itself is unpinned (no OpenCV to run against); this
restatement is the contract the tests hold the kernel to."""
import numpy as np

SHIFT = 20
CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527

# (Y, U, V) -> (B, G, R): the known answers of the spec
KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (0, 0, 254)),
         ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255))]


def yuv_to_bgr(y, u, v) -> np.ndarray:
    """Per-pixel conversion of same-shaped Y, U, V arrays -> (..., 3) uint8 BGR."""
    y, u, v = (np.asarray(a, np.int64) for a in (y, u, v))
    uu, vv = u - 128, v - 128
    yv = np.maximum(0, y - 16) * CY + (1 << (SHIFT - 1))
    sat = lambda a: np.clip(a >> SHIFT, 0, 255).astype(np.uint8)      # arithmetic shift, then clamp
    return np.stack([sat(yv + CUB * uu), sat(yv + CVG * vv + CUG * uu), sat(yv + CVR * vv)], axis=-1)


def planes(buf, h: int, w: int, fmt: str, pitch: int = 0, chroma_pitch: int = 0, u_offset: int = 0, v_offset: int = 0):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) of one frame held in the flat byte buffer `buf`, laid out as rtmodt_frame_format says
    (zeros = the packed defaults)."""
    b = np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8)
    nv12 = fmt == "nv12"
    pitch = pitch or w
    cp = chroma_pitch or (pitch if nv12 else pitch // 2)
    uo = u_offset or pitch * h
    rows = lambda off, p, n, k: np.stack([b[off + r * p: off + r * p + k] for r in range(n)])
    Y = rows(0, pitch, h, w)
    if nv12:
        uv = rows(uo, cp, h // 2, w)
        return Y, uv[:, 0::2], uv[:, 1::2]
    vo = v_offset or uo + cp * (h // 2)
    return Y, rows(uo, cp, h // 2, w // 2), rows(vo, cp, h // 2, w // 2)


def to_bgr(buf, h: int, w: int, fmt: str, **layout) -> np.ndarray:
    """One 4:2:0 frame -> (h, w, 3) uint8 BGR, per the spec."""
    Y, U, V = planes(buf, h, w, fmt, **layout)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    return yuv_to_bgr(Y, up(U), up(V))


def relayout(frame, h: int, w: int, fmt: str, pitch: int, rows_alloc: int, chroma_pitch: int = 0):
    """A packed frame re-laid out the way a decoder surface is: Y pitch `pitch`, the chroma plane(s) after `rows_alloc` rows
    (e.g. 1088 for 1080p), chroma pitch `chroma_pitch` (0 = the default).  Returns (flat buffer, layout kwargs); padding bytes are
    filled with 0xA5 so that a kernel that reads them shows."""
    Y, U, V = planes(frame, h, w, fmt)
    nv12 = fmt == "nv12"
    cp = chroma_pitch or (pitch if nv12 else pitch // 2)
    uo = pitch * rows_alloc
    vo = 0 if nv12 else uo + cp * (h // 2)
    size = (vo if not nv12 else uo) + cp * (h // 2) + 64
    out = np.full(size, 0xA5, np.uint8)
    for r in range(h):
        out[r * pitch: r * pitch + w] = Y[r]
    for r in range(h // 2):
        if nv12:
            row = np.empty(w, np.uint8)
            row[0::2], row[1::2] = U[r], V[r]
            out[uo + r * cp: uo + r * cp + w] = row
        else:
            out[uo + r * cp: uo + r * cp + w // 2] = U[r]
            out[vo + r * cp: vo + r * cp + w // 2] = V[r]
    kw = dict(pitch=pitch, chroma_pitch=chroma_pitch, u_offset=uo)
    if not nv12:
        kw["v_offset"] = vo
    return out, kw
