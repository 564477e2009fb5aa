"""GPU: the JPEG encoder (csrc/jpeg.hip) byte for byte against the NumPy restatement of its rules (tests/jpeg_ref.py, itself pinned
to libjpeg-turbo by tests/test_jpeg_cpu.py), through JpegEncoder and the C ABI: frame sizes and row strides, qualities, batches,
host and device frames, render -> encode on one device buffer, untouched sources and guards, capacity errors, handles side by
side, and the pipeline's recorder."""
import ctypes as C
import io
import struct
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as J
import render_ref as R

pytestmark = pytest.mark.gpu

ZONES = [("entrance", np.array([[100, 100], [400, 120], [380, 360], [120, 300]], np.int32)),
         ("loading bay", np.array([[300, 200], [600, 180], [610, 500], [320, 520], [450, 350]], np.int32))]


def content(rng, i, h, w):
    """Frame i of a batch: noise, a gradient, or a flat field with a noisy patch."""
    if i % 3 == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if i % 3 == 1:
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy + 16 * i) % 256], -1).astype(np.uint8)
    f = np.full((h, w, 3), (255, 0, 128 + i), np.uint8)
    f[h // 4:h // 2 + 1, w // 4:w // 2 + 1] = rng.integers(0, 256, (h // 2 + 1 - h // 4, w // 2 + 1 - w // 4, 3), dtype=np.uint8)
    return f


def strided_batch(rng, n, h, w, stride):
    """n frames in one padded buffer (random padding); returns (buffer [n, h * stride], views)."""
    buf = rng.integers(0, 256, (n, h * stride), dtype=np.uint8)
    views = [np.lib.stride_tricks.as_strided(buf[i], (h, w, 3), (stride, 3, 1), writeable=True) for i in range(n)]
    for i, v in enumerate(views):
        v[...] = content(rng, i, h, w)
    return buf, views


def first_diff(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return f"lengths {len(a)} / {len(b)}, first difference at byte {int(d[0]) if len(d) else n}"


@pytest.mark.parametrize("quality", [1, 50, 95, 100])
@pytest.mark.parametrize("h,w,stride", [(640, 640, 1920), (1080, 1920, 5760), (37, 53, 3 * 53 + 7), (64, 100, 304), (1, 1, 3),
                                        (16, 4099, 3 * 4099 + 1)])
def test_bit_exact(pkg, h, w, stride, quality):
    """Batches of 1, 3 and 8, host frames and a DeviceBuffer with an offset: every file equals jpeg_ref.encode's."""
    rng = np.random.default_rng(h * 31 + w + quality)
    buf, views = strided_batch(rng, 8, h, w, stride)
    want = [J.encode(v, quality) for v in views]
    enc = pkg.JpegEncoder(quality, max_height=h, max_width=w, max_batch=8)
    dev = pkg._ffi.DeviceBuffer(buf.nbytes + 96)
    dev.upload(buf, offset=32)
    for n in (1, 3, 8):
        got = enc.encode_batch(views[:n])
        assert len(got) == n
        for i in range(n):
            assert got[i] == want[i], f"host, batch {n}, frame {i}: {first_diff(got[i], want[i])}"
        got = enc.encode_batch(dev, height=h, width=w, stride=stride, offset=32, count=n)
        assert len(got) == n
        for i in range(n):
            assert got[i] == want[i], f"device, batch {n}, frame {i}: {first_diff(got[i], want[i])}"
    assert enc.encode(views[5]) == want[5]
    assert enc.last_kernel_ms() > 0
    dev.free()
    enc.close()


def make_tracks(rng, n, h, w):
    out = []
    for i in range(n):
        x1, y1 = rng.uniform(-20, w - 20), rng.uniform(-10, h - 20)
        bw, bh = rng.uniform(5, 200), rng.uniform(5, 200)
        cx, cy = int(x1 + bw / 2), int(y1 + bh / 2)
        trail = [(cx + int(rng.integers(-40, 41)), cy + int(rng.integers(-40, 41))) for _ in range(int(rng.integers(0, 20)))]
        out.append(SimpleNamespace(track_id=int(rng.integers(0, 500)), xyxy=np.array([x1, y1, x1 + bw, y1 + bh], np.float32),
                                   confidence=np.float32(rng.uniform(0, 1)), class_name=["person", "car", "dog"][i % 3], trail=trail))
    return out


def test_render_then_encode_on_one_device_buffer(pkg):
    rng = np.random.default_rng(21)
    n, h, w = 3, 540, 700
    frames = [content(rng, i + 1, h, w) for i in range(n)]
    lists = [make_tracks(rng, 30, h, w) for _ in range(n)]
    dev = pkg._ffi.DeviceBuffer(n * h * w * 3)
    dev.upload(np.stack(frames))
    pkg.FrameRenderer().render_batch(dev, lists, zones=ZONES, fps=30.0, latency_ms=7.5, height=h, width=w)
    got = pkg.JpegEncoder(90).encode_batch(dev, height=h, width=w)
    assert len(got) == n
    for i in range(n):
        drawn = R.render(frames[i], lists[i], ZONES, 30.0, 7.5)
        want = J.encode(drawn, 90)
        assert got[i] == want, f"frame {i}: {first_diff(got[i], want)}"
        im = Image.open(io.BytesIO(got[i]))
        im.load()
        assert im.size == (w, h)
    dev.free()


def raw_call(pkg, enc, ptrs, n, h, w, stride, mem, slot, guard=64):
    """rtmodt_jpeg_encode_batch into a 0xA5-filled buffer with `guard` bytes behind the last slot; -> (rc, out, sizes)."""
    out = np.full(n * slot + guard, 0xA5, np.uint8)
    sizes = np.zeros(max(n, 1), np.uint32)
    fp = (C.c_void_p * max(n, 1))(*ptrs)
    rc = pkg._ffi.lib().rtmodt_jpeg_encode_batch(enc._h, fp, n, h, w, stride, mem, pkg._ffi.ptr(out), slot, pkg._ffi.ptr(sizes))
    return rc, out, sizes


@pytest.mark.parametrize("device_frames", [False, True])
def test_sources_padding_and_guards_untouched(pkg, device_frames):
    rng = np.random.default_rng(33)
    n, h, w, stride = 3, 37, 53, 3 * 53 + 7
    buf, views = strided_batch(rng, n, h, w, stride)
    before = buf.copy()
    enc = pkg.JpegEncoder(75, max_height=h, max_width=w, max_batch=n)
    slot = 8192
    if device_frames:
        dev = pkg._ffi.DeviceBuffer(buf.nbytes + 64)
        dev.upload(np.full(buf.nbytes + 64, 0x5A, np.uint8))
        dev.upload(buf, offset=32)
        ptrs = [dev.ptr + 32 + i * h * stride for i in range(n)]
        rc, out, sizes = raw_call(pkg, enc, ptrs, n, h, w, stride, pkg._ffi.MEM_DEVICE, slot)
        after = dev.download()
        assert np.all(after[:32] == 0x5A) and np.all(after[-32:] == 0x5A)
        assert np.array_equal(after[32:-32].reshape(n, -1), before), "the device frames or their padding were written"
        dev.free()
    else:
        rc, out, sizes = raw_call(pkg, enc, [v.ctypes.data for v in views], n, h, w, stride, pkg._ffi.MEM_HOST, slot)
        assert np.array_equal(buf, before), "the host frames or their padding were written"
    assert rc == 0
    for i in range(n):
        want = J.encode(views[i], 75)
        assert out[i * slot:i * slot + sizes[i]].tobytes() == want
        assert np.all(out[i * slot + sizes[i]:(i + 1) * slot] == 0xA5), f"bytes behind file {i} were written"
    assert np.all(out[n * slot:] == 0xA5)


def test_capacity(pkg):
    E = pkg._ffi
    rng = np.random.default_rng(44)
    h = w = 640
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flat = np.full((h, w, 3), 90, np.uint8)
    enc = pkg.JpegEncoder(100, max_height=h, max_width=w, max_batch=3)
    hdr = len(J.header(100, h, w))
    slot = hdr + 1024
    need = len(J.encode(noise, 100))
    rc, out, sizes = raw_call(pkg, enc, [noise.ctypes.data], 1, h, w, 3 * w, E.MEM_HOST, slot)
    msg = E.lib().rtmodt_last_error().decode()
    assert rc == E.E_CAPACITY and "frame 0" in msg and str(need) in msg, msg
    assert sizes[0] == need
    assert np.all(out == 0xA5), "a file that does not fit left bytes behind"
    # [flat, noise, flat]: the flat files are complete, the slot of the noise frame and every guard are untouched
    flat_jpeg = J.encode(flat, 100)
    slot = len(flat_jpeg) + 100
    rc, out, sizes = raw_call(pkg, enc, [flat.ctypes.data, noise.ctypes.data, flat.ctypes.data], 3, h, w, 3 * w, E.MEM_HOST, slot)
    msg = E.lib().rtmodt_last_error().decode()
    assert rc == E.E_CAPACITY and "frame 1" in msg and str(need) in msg, msg
    assert sizes.tolist() == [len(flat_jpeg), need, len(flat_jpeg)]
    for i in (0, 2):
        assert out[i * slot:i * slot + sizes[i]].tobytes() == flat_jpeg
        assert np.all(out[i * slot + sizes[i]:(i + 1) * slot] == 0xA5)
        Image.open(io.BytesIO(out[i * slot:i * slot + sizes[i]].tobytes())).load()
    assert np.all(out[slot:2 * slot] == 0xA5) and np.all(out[3 * slot:] == 0xA5)
    # the wrapper retries with the size the library reported
    got = enc.encode_batch([flat, noise, flat], slot_bytes=slot)
    assert got == [flat_jpeg, J.encode(noise, 100), flat_jpeg]
    got = enc.encode_batch([noise])                       # default slot (header + 1.5 bytes per pixel) is too small for noise at 100
    assert len(got[0]) == need and got[0] == J.encode(noise, 100)
    # a frame larger than the handle: refused before anything runs
    big = np.zeros((h + 1, w, 3), np.uint8)
    rc, out, sizes = raw_call(pkg, enc, [big.ctypes.data], 1, h + 1, w, 3 * w, E.MEM_HOST, 1 << 20)
    assert rc == E.E_CAPACITY and np.all(out == 0xA5)
    rc, out, sizes = raw_call(pkg, enc, [flat.ctypes.data] * 4, 4, h, w, 3 * w, E.MEM_HOST, 1 << 16)
    assert rc == E.E_CAPACITY and np.all(out == 0xA5)
    # argument errors, and n = 0
    assert raw_call(pkg, enc, [flat.ctypes.data], 1, h, w, 3 * w - 1, E.MEM_HOST, 1 << 16)[0] == E.E_INVALID
    assert raw_call(pkg, enc, [0], 1, h, w, 3 * w, E.MEM_HOST, 1 << 16)[0] == E.E_INVALID
    assert raw_call(pkg, enc, [], 0, h, w, 3 * w, E.MEM_HOST, 1 << 16)[0] == 0
    hd = C.c_void_p()
    for cfg, code in ((E.JpegCfg(101, 0, 64, 64, 1), E.E_INVALID), (E.JpegCfg(95, 1, 64, 64, 1), E.E_UNSUPPORTED),
                      (E.JpegCfg(95, 0, 8193, 64, 1), E.E_INVALID), (E.JpegCfg(95, 0, 64, 64, 0), E.E_INVALID)):
        assert E.lib().rtmodt_jpeg_create(0, C.byref(cfg), C.byref(hd)) == code and not hd.value


def test_handles_side_by_side_and_geometry_changes(pkg):
    rng = np.random.default_rng(55)
    a, b = pkg.JpegEncoder(30, max_height=64, max_width=64, max_batch=1), pkg.JpegEncoder(97)
    f1, f2, f3 = content(rng, 0, 200, 310), content(rng, 1, 96, 80), content(rng, 2, 721, 1283)
    for _ in range(2):
        assert a.encode(f1) == J.encode(f1, 30)            # (a's handle is re-made for the larger frame)
        assert b.encode(f1) == J.encode(f1, 97)
        assert b.encode(f2) == J.encode(f2, 97)
        assert a.encode_batch([f3, f3]) == [J.encode(f3, 30)] * 2
        assert a.encode(f2) == J.encode(f2, 30)
    assert pkg.JpegEncoder().quality == 95
    assert a.encode_batch([]) == []


class _Det:
    def detect(self, frame):
        return type("D", (), {"__len__": lambda self: 1})()


class _Trk:
    def update(self, detections):
        return [SimpleNamespace(track_id=4, xyxy=np.array([2, 12, 30, 40], np.float32), confidence=0.9, class_name="person",
                                trail=[(5, 5), (16, 26)])]


def test_recorder_through_the_pipeline(pkg, tmp_path):
    frames = np.random.default_rng(6).integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    path = str(tmp_path / "out.avi")
    rec = pkg.MjpegRecorder(path, 25.0, pkg.JpegEncoder(85))
    prof = pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof, max_frames=5, device_stages=False,
                     renderer=pkg.FrameRenderer(show_fps=False), recorder=rec)
    rec.release()
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    at = data.index(b"idx1")
    n = struct.unpack("<I", data[at + 4:at + 8])[0] // 16
    assert n == 5
    movi = data.index(b"movi")
    for i in range(n):
        _, _, off, ln = struct.unpack("<4sIII", data[at + 8 + 16 * i:at + 24 + 16 * i])
        payload = data[movi + off + 8:movi + off + 8 + ln]
        drawn = R.render(frames[i % 2], _Trk().update(None), None, show_fps=False)
        assert payload == J.encode(drawn, 85), i
        got = np.asarray(Image.open(io.BytesIO(payload)).convert("RGB"))
        want = np.asarray(Image.open(io.BytesIO(J.encode(drawn, 85))).convert("RGB"))
        assert got.shape == (48, 64, 3) and np.array_equal(got, want)
