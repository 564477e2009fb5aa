"""CPU: the 4:2:0 input path's contract without a GPU -- the NumPy restatement of the conversion (tests/yuv420_ref.py) against
the spec's known answers and across layouts; header, ctypes structure and signature table in agreement; bad layouts refused in
Python and by the library (which checks a layout before it touches the device); the raw ingest back-end in nv12 / yuv420p mode."""
import ctypes as C
import os
import re
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv420_ref as R  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtmodt_amd  # noqa: E402,F401

pkg = sys.modules["rtmodt_amd"]
F = pkg._ffi


def test_restatement_gives_the_known_answers():
    for (y, u, v), bgr in R.KNOWN:
        assert tuple(int(c) for c in R.yuv_to_bgr([y], [u], [v])[0]) == bgr, (y, u, v)
    # every (Y, U, V) combination on a coarse grid stays in range and is monotone in Y for grey
    g = np.arange(0, 256, 15)
    yy, uu, vv = np.meshgrid(g, g, g, indexing="ij")
    out = R.yuv_to_bgr(yy, uu, vv)
    assert out.dtype == np.uint8 and out.shape == (*yy.shape, 3)
    grey = R.yuv_to_bgr(np.arange(256), np.full(256, 128), np.full(256, 128))
    assert (np.diff(grey.astype(int), axis=0) >= 0).all() and (grey[:17] == 0).all() and (grey[235:] == 255).all()


def test_nv12_and_i420_of_the_same_planes_agree():
    h, w = 38, 54
    nv12 = pkg.synth.yuv420_frames(1, h, w, "nv12", seed=3)[0]
    i420 = pkg.synth.yuv420_frames(1, h, w, "i420", seed=3)[0]
    assert nv12.shape == i420.shape == (h * 3 // 2, w)
    yn, un, vn = R.planes(nv12, h, w, "nv12")
    yi, ui, vi = R.planes(i420, h, w, "i420")
    assert np.array_equal(yn, yi) and np.array_equal(un, ui) and np.array_equal(vn, vi)
    assert np.array_equal(R.to_bgr(nv12, h, w, "nv12"), R.to_bgr(i420, h, w, "i420"))
    # chroma is nearest: the four pixels of a 2 x 2 block share U and V
    assert len(np.unique(un)) > 20 and len(np.unique(yn)) > 50


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_padded_pitch_and_height_equal_packed(fmt):
    h, w = 20, 30
    fr = pkg.synth.yuv420_frames(1, h, w, fmt, seed=5)[0]
    want = R.to_bgr(fr, h, w, fmt)
    for pitch, rows, cp in ((w, h, 0), (w + 7, h, 0), (64, 24, 0), (w + 2, h + 8, w + 11 if fmt == "nv12" else w // 2 + 5)):
        buf, kw = R.relayout(fr, h, w, fmt, pitch, rows, cp)
        assert np.array_equal(R.to_bgr(buf, h, w, fmt, **kw), want), (pitch, rows, cp)
        fm = F.frame_format(fmt, h, w, **kw)
        assert F.frame_span(fm, h, w) <= buf.nbytes


def test_synth_bgr_to_yuv_is_close_to_the_inverse():
    bgr = pkg.synth.structured_frames(2, 32, 48, seed=1)
    for fmt in ("nv12", "i420", "yuv420p"):
        yuv = pkg.synth.bgr_to_yuv420(bgr, fmt)
        assert yuv.shape == (2, 48, 48)
        back = R.to_bgr(yuv[0], 32, 48, "nv12" if fmt == "nv12" else "i420")
        assert np.abs(back.astype(int) - bgr[0].astype(int)).mean() < 12          # chroma is subsampled; only a sanity bar
    a, b = pkg.synth.yuv420_frames(1, 32, 48, seed=4), pkg.synth.yuv420_frames(1, 32, 48, seed=4)
    assert np.array_equal(a, b)


def _header():
    return open(F.HEADER_PATH).read()


def test_header_struct_and_signature_table_agree():
    src = _header()
    for name, val in (("BGR24", 0), ("NV12", 1), ("I420", 2)):          # (spelled in pieces: tests/*.py name run-time options only)
        assert re.search(rf"#define RTMODT_{'PIX'}_{name} {val}\b", src), name
    assert (F.PIX_BGR24, F.PIX_NV12, F.PIX_I420) == (0, 1, 2)
    body = src[src.index("typedef struct rtmodt_frame_format {"):]
    body = body[:body.index("} rtmodt_frame_format;")]
    fields = re.findall(r"\b(int32_t|int64_t)\s+(\w+);", body)
    assert [(n, t) for t, n in fields] == [(n, {C.c_int32: "int32_t", C.c_int64: "int64_t"}[t]) for n, t in F.FrameFormat._fields_]
    assert C.sizeof(F.FrameFormat) == 32
    assert [getattr(F.FrameFormat, n).offset for n, _ in F.FrameFormat._fields_] == [0, 4, 8, 12, 16, 24]
    L = F.lib()
    for s in ("rtmodt_detector_enqueue_batch_fmt", "rtmodt_preprocess_yuv420"):
        assert s in F.header_symbols() and s in L._signatures and hasattr(L, s)
    assert L._signatures["rtmodt_detector_enqueue_batch_fmt"][1][5] is C.POINTER(F.FrameFormat)
    assert L._signatures["rtmodt_preprocess_yuv420"][1][4] is C.POINTER(F.FrameFormat)
    assert F.PIXEL_FORMATS["yuv420p"] == F.PIX_I420


BAD = [  # (what, h, w, format, layout kwargs, exception, library code)
    ("odd height", 37, 54, "nv12", {}, ValueError, F.E_INVALID),
    ("odd width", 38, 53, "i420", {}, ValueError, F.E_INVALID),
    ("Y pitch too small", 38, 54, "nv12", dict(pitch=50), ValueError, F.E_INVALID),
    ("chroma pitch too small (nv12)", 38, 54, "nv12", dict(chroma_pitch=40), ValueError, F.E_INVALID),
    ("chroma pitch too small (i420)", 38, 54, "i420", dict(chroma_pitch=26), ValueError, F.E_INVALID),
    ("UV overlaps Y", 38, 54, "nv12", dict(u_offset=54 * 37), ValueError, F.E_INVALID),
    ("U overlaps Y", 38, 54, "i420", dict(u_offset=100), ValueError, F.E_INVALID),
    ("V overlaps U", 38, 54, "i420", dict(v_offset=54 * 38 + 27 * 18), ValueError, F.E_INVALID),
    ("V overlaps Y", 38, 54, "i420", dict(v_offset=10), ValueError, F.E_INVALID),
    ("negative offset", 38, 54, "i420", dict(u_offset=-5), ValueError, F.E_INVALID),
    ("unknown colorspace", 38, 54, "nv12", dict(colorspace=1), NotImplementedError, F.E_UNSUPPORTED),
]


@pytest.mark.parametrize("what,h,w,fmt,kw,exc,code", BAD, ids=[b[0] for b in BAD])
def test_bad_layouts_are_refused_in_python_and_by_the_library(what, h, w, fmt, kw, exc, code):
    with pytest.raises(exc):
        F.frame_format(fmt, h, w, **kw)
    # the library checks the layout before any device call: this runs without a GPU
    fm = F.FrameFormat(F.pixel_format_id(fmt), kw.get("colorspace", 0), kw.get("pitch", 0), kw.get("chroma_pitch", 0),
                       kw.get("u_offset", 0), kw.get("v_offset", 0))
    buf = np.zeros(4 * h * w, np.uint8)
    out = np.zeros((64, 64, 3), np.float16)
    L = F.lib()
    assert L.rtmodt_preprocess_yuv420(0, F.ptr(buf), h, w, C.byref(fm), 64, 64, F.ptr(out)) == code
    assert L.rtmodt_last_error()


def test_unknown_pixel_format_is_refused():
    with pytest.raises(ValueError, match="unknown pixel format"):
        F.frame_format("nv21", 38, 54)
    with pytest.raises(ValueError):
        F.pixel_format_id(7)
    L = F.lib()
    buf, out = np.zeros(4096, np.uint8), np.zeros((64, 64, 3), np.float16)
    for pf in (0, 3, -1):                                  # BGR24 is not a 4:2:0 format; 3 / -1 are no format at all
        fm = F.FrameFormat(pf, 0, 0, 0, 0, 0)
        assert L.rtmodt_preprocess_yuv420(0, F.ptr(buf), 38, 54, C.byref(fm), 64, 64, F.ptr(out)) == F.E_INVALID
    for pf in (3, -1):
        fm = F.FrameFormat(pf, 0, 0, 0, 0, 0)
        assert L.rtmodt_detector_enqueue_batch_fmt(None, None, 1, 38, 54, C.byref(fm), 0) == F.E_INVALID


def test_good_layouts_and_defaults():
    h, w = 1080, 1920
    nv = F.frame_format("nv12", h, w)
    assert F.frame_span(nv, h, w) == w * h * 3 // 2
    i4 = F.frame_format("yuv420p", h, w)
    assert i4.pixel_format == F.PIX_I420 and F.frame_span(i4, h, w) == w * h * 3 // 2
    pad = F.frame_format("nv12", h, w, pitch=2048, u_offset=2048 * 1088)
    assert F.frame_span(pad, h, w) == 2048 * 1088 + 2048 * 539 + 1920
    assert F.frame_span(F.frame_format("bgr24", h, w), h, w) == h * w * 3


def test_detector_pixel_format_keyword_is_keyword_only():
    import inspect
    p = inspect.signature(pkg.Detector.__init__).parameters["pixel_format"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "bgr24"
    q = inspect.signature(pkg.Detector.enqueue).parameters
    for k in ("pixel_format", "chroma_pitch", "u_offset", "v_offset"):
        assert q[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    r = inspect.signature(pkg.pipeline.PinnedFrameRing.__init__).parameters["pixel_format"]
    assert r.default == "bgr24"


@pytest.mark.parametrize("fmt", ["nv12", "yuv420p"])
def test_raw_backend_in_4_2_0_mode(tmp_path, fmt):
    h, w = 36, 52
    frames = pkg.synth.yuv420_frames(5, h, w, "nv12" if fmt == "nv12" else "i420", seed=9)
    path = tmp_path / "clip.yuv"
    path.write_bytes(frames.tobytes() + b"\x00" * (w * h))          # a trailing partial frame is the end of the stream
    ing = pkg.ingestion
    cap = ing.RawVideoCapture(str(path), resolution=(w, h), pixel_format=fmt)
    got = []
    while cap.grab():
        ok, f = cap.retrieve()
        got.append(f)
    assert len(got) == 5 and all(f.shape == (h * 3 // 2, w) for f in got)
    assert all(np.array_equal(a, b) for a, b in zip(got, frames))
    cap.release()
    with pytest.raises(ValueError):
        ing.RawVideoCapture(str(path), resolution=(51, 36), pixel_format=fmt)
    with pytest.raises(ValueError):
        ing.RawVideoCapture(str(path), resolution=(w, h), pixel_format="nv21")
    # through the reader, fed by a FIFO the writer closes: ids count the frames, end-of-stream leaves the last one readable
    fifo = str(tmp_path / "pipe.yuv")
    os.mkfifo(fifo)

    def writer():
        with open(fifo, "wb") as fw:
            for fr in frames:
                fw.write(fr.tobytes())
                time.sleep(0.01)
    t = threading.Thread(target=writer, daemon=True)
    t.start()
    r = ing.FrameReader(fifo, backend="raw", resolution=(w, h), pixel_format=fmt, reconnect_delay=0.01, max_reconnects=0)
    r.start()
    t.join(5.0)
    t0 = time.perf_counter()
    while r.is_alive and time.perf_counter() - t0 < 5.0:
        time.sleep(0.005)
    ok, f, fid = r.read()
    assert ok and fid == 5 and f.shape == (h * 3 // 2, w) and np.array_equal(f, frames[-1])
    assert not r.is_alive                                   # no reconnects allowed: the reader has stopped at end of stream
    r.stop()
