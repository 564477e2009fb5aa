"""GPU: csrc/jpeg_dec.hip against tests/jpeg_dec_ref.py, byte for byte -- pixels and, one stage earlier, the entropy decoder's
coefficients -- at the smallest shapes where each mechanism can break: one block, one MCU, partial MCUs and odd extents (edge
replication on the component's real extent), chroma widths 1, 2 and 3 (the replication rule), every subsampling with no DRI, a
restart per MCU row and per 1 and 3 MCUs (intervals across row ends, RST0..7 wrapping), 70 intervals (more than one wave);
optimised tables, qualities 5 / 75 / 100, noise / smooth / flat / checkerboard content.  Then batches of unlike files, padded rows
with guard bytes, host and device destinations, the encoder round trip, one batch with a truncated and a corrupt file (the streams
the sanitised native program has passed on the CPU), the API's edges, and FrameReader(backend="mjpeg") feeding pipeline.run.
jpeg_dec_ref itself equals libjpeg-turbo (tests/test_jpeg_dec_cpu.py)."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import jpeg_dec_cases as K
import jpeg_dec_ref as D
import jpeg_ref as J

pytestmark = pytest.mark.gpu

_REF = {}


def ref_of(file):
    """(pixels as [h, w, 3] BGR, coefficients) of the restatement, computed once per file"""
    if file not in _REF:
        H, coefs, st = D.entropy_decode(file)
        assert st == D.OK
        px = D.pixels(H, coefs)
        _REF[file] = (px if px.ndim == 3 else np.repeat(px[..., None], 3, axis=2), coefs)
    return _REF[file]


@pytest.fixture(scope="module")
def dec(pkg):
    d = pkg.ingestion.JpegDecoder(max_height=64, max_width=1120, max_batch=128, max_file_bytes=1 << 18)
    yield d
    d.close()


def check_batch(dec, files, h, w, what=""):
    out, status = dec.decode_batch(files, out=np.full((len(files), h, w, 3), 0x5A, np.uint8))
    assert status.tolist() == [D.OK] * len(files), (what, status.tolist())
    for i, f in enumerate(files):
        px, coefs = ref_of(f)
        for c, want in enumerate(coefs):                                   # a mismatch is placed before or after the IDCT
            got = dec.coefficients(i, c)
            assert got.shape == want.shape and np.array_equal(got, want), f"{what} file {i} component {c}: coefficients differ"
        assert np.array_equal(out[i], px), f"{what} file {i}: {int(np.count_nonzero(out[i] != px))} pixel bytes differ"


VARIATIONS = [("noise", 75, "none"), ("smooth", 5, "none"), ("checker", 100, "none"), ("noise", 75, "optimised"), ("flat", 75, "none")]


def files_for(h, w, subsamplings, markers, variations=VARIATIONS):
    out = []
    for ss in subsamplings:
        for marker in markers:
            for kind, q, opt in variations:
                if opt == "optimised" and marker != "none":
                    continue                                               # (Pillow's options: a file is optimised or has restart markers here)
                out.append(K.pillow_file(K.frame(kind, h, w), q, ss, opt if opt != "none" else marker))
    return out


@pytest.mark.parametrize("h,w,subsamplings,markers", [
    (8, 8, ["gray"], ["none"]),                                            # one block
    (16, 16, ["420"], ["none"]),                                           # one MCU
    (17, 33, K.SUBSAMPLINGS, ["none", "row"]),                             # partial MCUs, odd extents
    (31, 15, K.SUBSAMPLINGS, ["none", "mcu1"]),
    (40, 2, ["444", "422", "420"], ["none", "mcu1"]),                      # chroma width 1
    (20, 4, ["444", "422", "420"], ["none", "mcu1"]),                      # chroma width 2
    (7, 5, ["444", "422", "420"], ["none", "mcu1"]),                       # chroma width 3
    (33, 1, ["444", "422", "420"], ["none", "mcu1"]),
    (48, 64, K.SUBSAMPLINGS, ["none", "row", "mcu1", "mcu3"]),             # intervals across row ends, RST0..7 wrapping
], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_shapes_and_mechanisms(dec, h, w, subsamplings, markers):
    files = files_for(h, w, subsamplings, markers)
    check_batch(dec, files, h, w, f"{h}x{w}")


def test_seventy_intervals_span_two_waves(dec):
    files = [K.pillow_file(K.frame(kind, 16, 1120), q, "420", "mcu1") for kind, q in (("noise", 75), ("smooth", 5), ("checker", 100))]
    assert all(D.parse(f).intervals == 70 for f in files)
    check_batch(dec, files, 16, 1120, "16x1120")


@pytest.mark.parametrize("lanes", [64, 4])
def test_intervals_packed_into_waves(pkg, monkeypatch, lanes):
    """The entropy kernel spreads few intervals one per wave; RTMODT_JPEGDEC_LANES forces the packing a large call gets: 64 lanes (70
    intervals: two waves, the second partly filled) and 4."""
    monkeypatch.setenv("RTMODT_JPEGDEC_LANES", str(lanes))
    d = pkg.ingestion.JpegDecoder(max_height=48, max_width=1120, max_batch=32, max_file_bytes=1 << 18)
    monkeypatch.delenv("RTMODT_JPEGDEC_LANES")
    files = [K.pillow_file(K.frame(kind, 16, 1120), q, "420", "mcu1") for kind, q in (("noise", 75), ("smooth", 5), ("checker", 100))]
    check_batch(d, files, 16, 1120, f"16x1120, {lanes} lanes")
    check_batch(d, files_for(48, 64, K.SUBSAMPLINGS, ["mcu1", "mcu3", "row"], VARIATIONS[:2]), 48, 64, f"48x64, {lanes} lanes")
    d.close()


def mixed_three(h, w):
    return [K.pillow_file(K.frame("noise", h, w), 40, "420", "row"), K.pillow_file(K.frame("smooth", h, w, seed=1), 97, "444", "optimised"),
            K.pillow_file(K.frame("noise", h, w, seed=2), 80, "gray", "mcu3")]


def test_mixed_batch_padded_rows_host_and_device(pkg, dec):
    h, w, stride, lead = 37, 53, 3 * 53 + 11, 29
    files = mixed_three(h, w)
    want = [ref_of(f)[0] for f in files]
    # host: rows padded, guard bytes before, between (the padding of every row) and after the frames
    buf = np.full(lead + 3 * h * stride + 64, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[lead:], (3, h, w, 3), (h * stride, stride, 3, 1))
    _, status = dec.decode_batch(files, out=view)
    assert status.tolist() == [0, 0, 0]
    guard = np.ones(buf.shape, bool)
    for i in range(3):
        assert np.array_equal(view[i], want[i]), i
        for y in range(h):
            at = lead + i * h * stride + y * stride
            guard[at:at + 3 * w] = False
    assert np.all(buf[guard] == 0xA5), "a byte outside the frames' rows was written"
    # device: the same layout inside a DeviceBuffer
    dev = pkg._ffi.DeviceBuffer(buf.nbytes)
    dev.upload(np.full(buf.nbytes, 0xA5, np.uint8))
    _, status = dec.decode_batch(files, out=dev, height=h, width=w, stride=stride, offset=lead)
    assert status.tolist() == [0, 0, 0]
    assert np.array_equal(dev.download(), buf), "device frames differ from the host frames, guard bytes included"
    dev.free()


@pytest.mark.parametrize("h,w", [(48, 64), (136, 250)])
def test_encoder_round_trip(pkg, dec, h, w):
    frames = [K.frame("noise", h, w), K.frame("smooth", h, w), pkg.synth.frames(1, h, w, seed=3)[0]]
    enc = pkg.JpegEncoder(90, max_height=h, max_width=w, max_batch=3)
    files = enc.encode_batch(frames)
    enc.close()
    assert files[0] == J.encode(frames[0], 90)
    check_batch(dec, files, h, w, "encoder round trip")


def test_damaged_stream_batch(dec):
    """Input validation with bounded reads: one batch, frame 1 truncated, frame 2 with a flipped scan byte that makes it CORRUPT --
    two of the streams tests/test_jpeg_dec_cpu.py runs through the sanitised native program."""
    from test_jpeg_dec_cpu import damaged_files
    files = damaged_files()
    good = K.pillow_file(K.frame("noise", 33, 49), 90, "444", "none")              # the CPU test's second base file
    cut = files[5 + 2]                                                               # ... cut half-way through its scan
    assert cut == K.truncated(good, 0.5) and D.status_of(cut) == D.TRUNCATED
    flipped = next(f for i, f in enumerate(files[20:220]) if i % 4 == 1 and D.status_of(f) == D.CORRUPT)
    other = K.pillow_file(K.frame("smooth", 33, 49), 60, "420", "row")
    h, w, stride = 33, 49, 3 * 49 + 5
    buf = np.full(16 + 4 * h * stride, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[16:], (4, h, w, 3), (h * stride, stride, 3, 1))
    _, status = dec.decode_batch([good, cut, flipped, other], out=view)
    assert status.tolist() == [D.status_of(f) for f in (good, cut, flipped, other)] == [D.OK, D.TRUNCATED, D.CORRUPT, D.OK]
    assert np.array_equal(view[0], ref_of(good)[0]) and np.array_equal(view[3], ref_of(other)[0])
    guard = np.ones(buf.shape, bool)
    for i in range(4):
        for y in range(h):
            at = 16 + i * h * stride + y * stride
            guard[at:at + 3 * w] = False
    assert np.all(buf[guard] == 0xA5)


def test_api_edges(pkg):
    E = pkg._ffi
    L = E.lib()

    def create(max_h, max_w, max_batch, max_file):
        hd = C.c_void_p()
        cfg = E.JpegDecCfg(max_h, max_w, max_batch, max_file)
        assert L.rtmodt_jpegdec_create(0, C.byref(cfg), C.byref(hd)) == 0, L.rtmodt_last_error()
        return hd

    a, b = create(32, 48, 2, 2048), create(64, 64, 4, 1 << 16)
    small = K.pillow_file(K.frame("smooth", 24, 40), 50, "420", "row")
    big = K.pillow_file(K.frame("noise", 24, 40), 100, "444")
    assert len(small) <= 2048 < len(big)

    def call(hd, files, h, w, stride=None, mem=E.MEM_HOST, n=None, null=None):
        n = len(files) if n is None else n
        arrs = [np.frombuffer(f, np.uint8) for f in files]
        fp = (C.c_void_p * max(len(files), 1))(*[x.ctypes.data for x in arrs])
        sizes = (C.c_size_t * max(len(files), 1))(*[len(f) for f in files])
        out = np.full((max(len(files), 1), h, w, 3), 0x33, np.uint8)
        dp = (C.c_void_p * max(len(files), 1))(*[out[i].ctypes.data for i in range(len(files))])
        status = np.full(max(len(files), 1), -7, np.int32)
        args = [hd, fp, sizes, n, dp, h, w, 3 * w if stride is None else stride, mem, E.ptr(status)]
        if null is not None:
            args[null] = None
        return L.rtmodt_jpegdec_decode_batch(*args), out, status

    ms = C.c_float(0)
    assert L.rtmodt_jpegdec_last_ms(a, C.byref(ms)) == E.E_INVALID                 # nothing has run
    # capacity and argument errors launch nothing: status and frames stay as they were, no kernel time exists
    for rc_want, kw in ((E.E_CAPACITY, dict(files=[small] * 3, h=24, w=40)), (E.E_CAPACITY, dict(files=[small], h=33, w=40)),
                        (E.E_CAPACITY, dict(files=[small], h=24, w=49)), (E.E_CAPACITY, dict(files=[big], h=24, w=40)),
                        (E.E_INVALID, dict(files=[small], h=24, w=40, stride=3 * 40 - 1)), (E.E_INVALID, dict(files=[small], h=24, w=40, mem=7)),
                        (E.E_INVALID, dict(files=[small], h=24, w=40, null=1)), (E.E_INVALID, dict(files=[small], h=24, w=40, null=9)),
                        (E.E_INVALID, dict(files=[small], h=0, w=40)), (E.E_INVALID, dict(files=[small], h=24, w=40, n=-1))):
        rc, out, status = call(a, **kw)
        assert rc == rc_want and L.rtmodt_last_error(), kw
        assert np.all(out == 0x33) and np.all(status == -7), kw
        assert L.rtmodt_jpegdec_last_ms(a, C.byref(ms)) == E.E_INVALID
    rc, out, status = call(a, [], 24, 40)                                            # n = 0 succeeds, nothing launched
    assert rc == 0 and L.rtmodt_jpegdec_last_ms(a, C.byref(ms)) == E.E_INVALID
    # two handles side by side, and geometry changes between calls
    want_small, want_big = ref_of(small)[0], ref_of(big)[0]
    tiny = K.pillow_file(K.frame("noise", 9, 11), 75, "422", "mcu1")
    for _ in range(2):
        rc, out, status = call(a, [small, small], 24, 40)
        assert rc == 0 and status.tolist() == [0, 0] and np.array_equal(out[0], want_small) and np.array_equal(out[1], want_small)
        rc, out, status = call(b, [big, small, big], 24, 40)
        assert rc == 0 and status.tolist() == [0, 0, 0] and np.array_equal(out[0], want_big) and np.array_equal(out[1], want_small)
        rc, out, status = call(a, [tiny], 9, 11)
        assert rc == 0 and status.tolist() == [0] and np.array_equal(out[0], ref_of(tiny)[0])
        assert L.rtmodt_jpegdec_last_ms(a, C.byref(ms)) == 0 and ms.value > 0
    rc, out, status = call(b, [small, tiny], 24, 40)                                 # a sound file of another size
    assert rc == 0 and status.tolist() == [D.OK, D.SIZE_MISMATCH] and np.all(out[1] == 0x33)
    L.rtmodt_jpegdec_destroy(a)
    L.rtmodt_jpegdec_destroy(b)
    L.rtmodt_jpegdec_destroy(None)


def test_decoder_class(pkg):
    M = pkg.ingestion
    d = M.JpegDecoder(max_height=8, max_width=8, max_batch=1)                         # grows by itself
    f = K.pillow_file(K.frame("noise", 24, 40), 80, "420", "row")
    g = K.pillow_file(K.frame("noise", 24, 40), 80, "gray")
    assert np.array_equal(d.decode(f), ref_of(f)[0])
    assert np.array_equal(d.decode(g), ref_of(g)[0]) and np.array_equal(d.decode(g, gray_plane=True), ref_of(g)[0][..., 0])
    out, status = d.decode_batch([f, g, f])
    assert out.shape == (3, 24, 40, 3) and status.tolist() == [0, 0, 0] and np.array_equal(out[1], ref_of(g)[0])
    assert d.last_kernel_ms() > 0
    with pytest.raises(M.JpegDecodeError) as e:
        d.decode(f[:100])
    assert e.value.status == D.TRUNCATED
    assert d.decode_batch([])[1].shape == (0,)
    d.close()
    d.close()


class _Stepped:
    """A FIFO fed one piece per frame the consumer asks for: the latest-frame reader then hands over every frame, in order."""

    def __init__(self, path, pieces):
        self.path, self.pieces, self.sem, self.reader, self.fids, self.want = path, pieces, threading.Semaphore(0), None, [], 0
        os.mkfifo(path)
        self.thread = threading.Thread(target=self._feed, daemon=True)
        self.thread.start()

    def _feed(self):
        with open(self.path, "wb", buffering=0) as f:
            for p in self.pieces:
                self.sem.acquire()
                f.write(p)

    def read(self):
        self.want += 1
        self.sem.release()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 20.0:
            ok, frame, fid = self.reader.read()
            if ok and fid >= self.want:
                self.fids.append(fid)
                return ok, frame, fid
            time.sleep(0)
        raise AssertionError(f"frame {self.want} never arrived")


class _Logged:
    def __init__(self, det):
        self.det, self.log = det, []

    def detect(self, frame):
        d = self.det.detect(frame)
        self.log.append((d.xyxy.copy(), d.confidence.copy(), d.class_id.copy()))
        return d


def test_mjpeg_reader_feeds_the_pipeline(pkg, tmp_path):
    h, w, n = 48, 64, 10
    frames = pkg.synth.frames(n, h, w, seed=11)
    enc = pkg.JpegEncoder(90, max_height=h, max_width=w, max_batch=n)
    jpegs = enc.encode_batch(list(frames))
    enc.close()
    decoded = [ref_of(j)[0] for j in jpegs]
    avi = str(tmp_path / "clip.avi")
    with pkg.MjpegWriter(avi, 25, (w, h)) as wr:
        for j in jpegs:
            wr.write(j)
    data = open(avi, "rb").read()
    at, cuts = pkg.MjpegWriter._MOVI_AT + 12, []
    for j in jpegs:                                                          # the file, cut behind every 00dc chunk
        at += 8 + len(j) + (len(j) & 1)
        cuts.append(at)
    avi_pieces = [data[a:b] for a, b in zip([0] + cuts[:-1], cuts[:-1] + [len(data)])]
    wpath = str(tmp_path / "w.rtw")
    pkg.weights.save(wpath, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(wpath, input_size=(320, 320), confidence=0.02, max_det=100, warmup=False, autotune=False)
    runs = {}
    for name, pieces, kw in (("mjpeg", avi_pieces, {}), ("raw", [d.tobytes() for d in decoded], {})):
        src = _Stepped(str(tmp_path / (name + ".avi")), pieces)
        ring = pkg.pipeline.PinnedFrameRing(3, h, w)
        log = _Logged(det)
        with pkg.ingestion.FrameReader(src.path, backend=name, resolution=(w, h), ring=ring, reconnect_delay=0.01, max_reconnects=0, **kw) as reader:
            src.reader = reader
            prof = pkg.profiling.LatencyProfiler(gpu_sync=True, warmup_frames=0, log_interval=1000)
            pkg.pipeline.run(src, log, pkg.MultiObjectTracker("bytetrack"), prof, max_frames=n, device_stages=False, device_handoff=False)
        src.thread.join(timeout=5)
        ring.close()
        runs[name] = (src.fids, log.log)
    det.close()
    assert runs["mjpeg"][0] == runs["raw"][0] == list(range(1, n + 1))
    assert sum(len(d[0]) for d in runs["raw"][1]) > 0
    for a, b in zip(runs["mjpeg"][1], runs["raw"][1]):
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
