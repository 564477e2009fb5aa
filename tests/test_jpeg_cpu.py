"""CPU: the JPEG rules of csrc/jpeg.hip as tests/jpeg_ref.py restates them, judged by libjpeg itself (Pillow 12 on libjpeg-turbo 3.1),
plus the host-only pieces: rtmodt_jpeg_header, MjpegWriter / multipart_chunk and the pipeline's recorder hook.

Against libjpeg: PARITY PINNED.  For every size, quality and content below, the entropy-coded scan of jpeg_ref.encode equals, byte for
byte, the scan Pillow writes from the same pixels with quality=q, subsampling=2 (4:2:0), optimize=False, restart_marker_rows=1 -- and
so do the quantisation tables Pillow reports and the DHT segments.  Two rules had to be libjpeg's exactly to get there, and both are
stated in jpeg.hip's header: a luminance block that lies wholly outside the frame's blocks is not coded from replicated pixels but as
"zero AC, DC of the block before it in the MCU" (jccoefct.c), and below an even-height frame the chroma rows repeat the last
DOWN-SAMPLED row, not the down-sampling of the repeated last pixel row (jcprepct.c pads after down-sampling).  With pixel replication
alone the scans differed at 8 x 8 and 1080 x 1920 (and any even h that is not a multiple of 16) by up to 14 chroma levels after
decoding; with the two rules no byte differs.  Players for the AVI files are not available: parity with them is unpinned."""
import ctypes as C
import io
import struct
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as J
import render_ref as R

SIZES = [(1, 1), (8, 8), (16, 16), (37, 53), (64, 100), (640, 640), (1080, 1920)]
QUALITIES = [1, 25, 50, 75, 95, 100]
CONTENTS = ["flat", "gradient", "rendered", "noise"]
_FRAMES = {}


def frame_of(kind, h, w):
    key = (kind, h, w)
    if key in _FRAMES:
        return _FRAMES[key]
    rng = np.random.default_rng(h * 3 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) % 256], -1).astype(np.uint8)
    if kind == "flat":
        f = np.full((h, w, 3), (10, 200, 90), np.uint8)
    elif kind == "gradient":
        f = grad
    elif kind == "noise":
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        tracks = []
        for i in range(12):
            x1, y1 = rng.uniform(-5, w), rng.uniform(-5, h)
            bw, bh = rng.uniform(2, max(w / 3, 3)), rng.uniform(2, max(h / 3, 3))
            cx, cy = int(x1 + bw / 2), int(y1 + bh / 2)
            tracks.append(SimpleNamespace(track_id=i * 7, xyxy=np.array([x1, y1, x1 + bw, y1 + bh], np.float32), confidence=np.float32(0.5 + i / 30),
                                          class_name="person", trail=[(cx - 3 * k, cy - 2 * k) for k in range(10)]))
        zones = [("zone", np.array([[w // 8, h // 8], [w // 2, h // 6], [w // 3, h // 2]], np.int32))]
        f = R.render(grad, tracks, zones, 30.0, 5.0)
    _FRAMES[key] = f
    return f


def pillow_encode(frame_bgr, q):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(b, "JPEG", quality=q, subsampling=2, optimize=False, restart_marker_rows=1)
    return b.getvalue()


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_streams_decode_and_equal_libjpeg(h, w, kind):
    f = frame_of(kind, h, w)
    for q in QUALITIES:
        mine = J.encode(f, q)
        # 1. any decoder reads it: right size, no warning, ceil(h / 16) - 1 restart markers in cycling order
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            im = Image.open(io.BytesIO(mine))
            im.load()
        assert im.size == (w, h) and im.mode == "RGB"
        hdr, body, rst = J.split(mine)
        assert hdr == J.header(q, h, w)
        assert rst == [m % 8 for m in range((h + 15) // 16 - 1)], (q, rst)
        # 2. against libjpeg: the tables first, then the scan, byte for byte
        theirs = pillow_encode(f, q)
        qt = Image.open(io.BytesIO(theirs)).quantization
        ql, qc = J.quant_tables(q)
        assert list(qt[0]) == ql.tolist() and list(qt[1]) == qc.tolist(), q
        assert [s for s in J.segments(theirs) if s[0] == 0xC4] == [s for s in J.segments(mine) if s[0] == 0xC4]
        assert (0xDD, ((w + 15) // 16).to_bytes(2, "big")) in J.segments(theirs)
        _, body_t, rst_t = J.split(theirs)
        assert rst_t == rst
        assert body == body_t, f"{kind} {w}x{h} q{q}: scans differ ({len(body)} / {len(body_t)} bytes)"


def test_dummy_block_and_chroma_row_rules_matter():
    """The two edge rules are not decoration: without either, the restatement would not equal libjpeg at these sizes."""
    f = frame_of("noise", 24, 24)
    c = J.coefficients(f, 90)
    assert not c[-1, :, 2:4, 1:].any() and not c[:, -1, 1, 1:].any() and not c[:, -1, 3, 1:].any()
    assert (c[-1, :, 2, 0] == c[-1, :, 1, 0]).all() and (c[-1, :, 3, 0] == c[-1, :, 1, 0]).all()
    assert (c[0, -1, 1, 0] == c[0, -1, 0, 0]) and (c[0, -1, 3, 0] == c[0, -1, 2, 0])
    _, cb, _ = J.planes(f)
    assert np.array_equal(cb[12:], np.repeat(cb[11:12], 4, axis=0))


def test_header_from_the_library(pkg):
    """rtmodt_jpeg_header needs no device; it returns the restatement's bytes."""
    L, E = pkg._ffi.lib(), pkg._ffi
    need = C.c_size_t(0)
    for q, h, w in [(95, 1080, 1920), (1, 1, 1), (50, 37, 53), (100, 8192, 8192), (85, 16, 4099), (49, 640, 640)]:
        want = J.header(q, h, w)
        assert L.rtmodt_jpeg_header(q, h, w, None, 0, C.byref(need)) == 0 and need.value == len(want)       # null buffer: the size
        short = np.full(len(want) - 1, 0xA5, np.uint8)
        assert L.rtmodt_jpeg_header(q, h, w, E.ptr(short), short.nbytes, C.byref(need)) == 0 and need.value == len(want)
        assert np.all(short == 0xA5), "a short buffer was written"
        buf = np.full(len(want) + 8, 0xA5, np.uint8)
        assert L.rtmodt_jpeg_header(q, h, w, E.ptr(buf), buf.nbytes, C.byref(need)) == 0
        assert buf[:len(want)].tobytes() == want and np.all(buf[len(want):] == 0xA5)
        assert pkg.visualization.jpeg.header(q, h, w) == want
    for q, h, w in [(0, 8, 8), (101, 8, 8), (-1, 8, 8), (95, 0, 8), (95, 8, 0), (95, 8193, 8), (95, 8, 8193)]:
        assert L.rtmodt_jpeg_header(q, h, w, None, 0, C.byref(need)) == E.E_INVALID, (q, h, w)
    assert L.rtmodt_jpeg_header(95, 8, 8, None, 0, None) == E.E_INVALID
    assert b"null" in L.rtmodt_last_error()


def riff_tree(data, at, end):
    """[(fourcc, list type or None, payload offset, payload size)] of the chunks in data[at:end]."""
    out = []
    while at < end:
        cc, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        kind = data[at + 8:at + 12] if cc in (b"RIFF", b"LIST") else None
        out.append((cc, kind, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end, "chunk sizes do not add up"
    return out


def test_mjpeg_writer_avi(pkg, tmp_path):
    V = pkg.visualization.jpeg
    rng = np.random.default_rng(2)
    jpegs = [J.encode(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) >> s, 80) for s in (0, 2, 4, 6, 7)]
    jpegs[1] += b""                                              # (lengths differ; make sure one is odd)
    if all(len(j) % 2 == 0 for j in jpegs):
        jpegs[2] = jpegs[2][:-2] + b"\x00\xff\xd9"               # a padding byte before EOI keeps the file decodable
    assert any(len(j) % 2 for j in jpegs) and len({len(j) for j in jpegs}) == 5
    path = str(tmp_path / "clip.avi")
    wr = V.MjpegWriter(path, 29.97, (64, 48))
    assert wr.isOpened()
    for j in jpegs:
        wr.write(j)
    wr.release()
    wr.release()                                                  # idempotent, like cv2's
    with pytest.raises(ValueError):
        wr.write(jpegs[0])
    data = open(path, "rb").read()
    top = riff_tree(data, 0, len(data))
    assert len(top) == 1 and top[0][:2] == (b"RIFF", b"AVI ") and top[0][3] == len(data) - 8
    chunks = riff_tree(data, 12, len(data))
    assert [(c[0], c[1]) for c in chunks] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl, movi, idx1 = chunks
    inner = riff_tree(data, hdrl[2] + 4, hdrl[2] + hdrl[3])
    assert [(c[0], c[1]) for c in inner] == [(b"avih", None), (b"LIST", b"strl")]
    avih = struct.unpack("<14I", data[inner[0][2]:inner[0][2] + inner[0][3]])
    assert avih[4] == 5 and avih[6] == 1 and avih[8:10] == (64, 48) and avih[3] & 0x10 and avih[0] == round(1e6 / 29.97)
    strl = riff_tree(data, inner[1][2] + 4, inner[1][2] + inner[1][3])
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][3] == 56 and strl[1][3] == 40
    strh = data[strl[0][2]:strl[0][2] + 56]
    assert strh[:8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack("<4I", strh[20:36])
    assert abs(rate / scale - 29.97) < 1e-9 and length == 5
    strf = struct.unpack("<IiiHH4sI", data[strl[1][2]:strl[1][2] + 24])
    assert strf[:6] == (40, 64, 48, 1, 24, b"MJPG")
    frames = riff_tree(data, movi[2] + 4, movi[2] + movi[3])
    assert [c[0] for c in frames] == [b"00dc"] * 5
    assert idx1[3] == 16 * 5
    for i, j in enumerate(jpegs):
        cc, flags, off, ln = struct.unpack("<4sIII", data[idx1[2] + 16 * i:idx1[2] + 16 * i + 16])
        assert cc == b"00dc" and flags & 0x10 and ln == len(j)
        at = movi[2] + off                                       # offsets count from the 'movi' fourcc
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == ln and at + 8 == frames[i][2]
        assert data[at + 8:at + 8 + ln] == j
        assert at % 2 == 0
        im = Image.open(io.BytesIO(data[at + 8:at + 8 + ln]))
        im.load()
        assert im.size == (64, 48)


def test_mjpeg_writer_other_containers_and_limits(pkg, tmp_path, monkeypatch):
    V = pkg.visualization.jpeg
    jpegs = [J.encode(np.full((16, 16, 3), v, np.uint8), 50) + b"" for v in (0, 100, 200)]
    for ext in (".mjpeg", ".MJPG"):
        p = str(tmp_path / ("s" + ext))
        with V.MjpegWriter(p, 10, (16, 16)) as wr:
            for j in jpegs:
                wr.write(j)
            assert wr.frames == 3
        assert open(p, "rb").read() == b"".join(jpegs)
    for bad in ("x.mp4", "x", "x.avi.txt"):
        with pytest.raises(ValueError):
            V.MjpegWriter(str(tmp_path / bad), 10, (16, 16))
    with pytest.raises(ValueError):
        V.MjpegWriter(str(tmp_path / "f.avi"), 0, (16, 16))
    # the 2 GiB refusal, with the limit patched down: the frame that would cross it raises and the file stays a valid AVI
    p = str(tmp_path / "full.avi")
    one = 8 + len(jpegs[0]) + (len(jpegs[0]) & 1)
    monkeypatch.setattr(V, "AVI_MAX_BYTES", V.MjpegWriter._MOVI_AT + 12 + 2 * one + 8 + 16 * 2 + 10)
    wr = V.MjpegWriter(p, 10, (16, 16))
    wr.write(jpegs[0])
    wr.write(jpegs[0])
    with pytest.raises(ValueError, match="frame 2"):
        wr.write(jpegs[0])
    wr.release()
    data = open(p, "rb").read()
    assert len(data) <= V.AVI_MAX_BYTES and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    chunks = riff_tree(data, 12, len(data))
    assert [c[1] or c[0] for c in chunks] == [b"hdrl", b"movi", b"idx1"] and chunks[2][3] == 32
    # multipart framing
    part = V.multipart_chunk(jpegs[1])
    assert part == b"--frame\r\nContent-Type: image/jpeg\r\nContent-Length: %d\r\n\r\n" % len(jpegs[1]) + jpegs[1] + b"\r\n"
    assert V.multipart_chunk(b"ab", boundary=b"xyz").startswith(b"--xyz\r\n")
    assert pkg.MjpegWriter is V.MjpegWriter and pkg.visualization.multipart_chunk is V.multipart_chunk


class _Det:
    def detect(self, frame):
        return type("D", (), {"__len__": lambda self: 1})()


class _Trk:
    def update(self, detections):
        return []


def test_pipeline_recorder_hook(pkg):
    log = []

    class Prof(pkg.profiling.LatencyProfiler):
        def tick(self, stage):
            log.append(("tick", stage))
            return super().tick(stage)

        def end_frame(self):
            log.append(("end_frame",))
            return super().end_frame()

    class Renderer:
        def render(self, frame, tracks, zones=None, fps=0.0, latency_ms=0.0):
            frame[0, 0] = (1, 2, 3)                              # "annotated"
            return frame

    class Recorder:
        def __init__(self):
            self.frames = []

        def write(self, frame):
            log.append(("write",))
            self.frames.append(frame.copy())

    frames = np.full((2, 8, 8, 3), 77, np.uint8)
    mk = lambda: Prof(gpu_sync=False, warmup_frames=0, log_interval=1000)
    run = lambda **kw: pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), mk(), max_frames=4, device_stages=False,
                                        renderer=Renderer(), **kw)
    base = run()
    plain_log, log[:] = list(log), []
    rec = Recorder()
    out = run(recorder=rec)
    assert len(rec.frames) == 4 and all(tuple(f[0, 0]) == (1, 2, 3) and f[1, 1, 0] == 77 for f in rec.frames)
    per_frame = [e for e in log if e[0] in ("end_frame", "write")]
    assert per_frame == [("end_frame",), ("write",)] * 4, "recorder.write must follow profiler.end_frame, once per frame"
    assert [e for e in log if e[0] != "write"] == plain_log                   # the stages are ticked exactly as without a recorder
    assert sorted(out) == sorted(base) and not any("record" in k for k in out)
    assert {k for k in out if k.endswith("_mean_ms")} == {k for k in base if k.endswith("_mean_ms")}
