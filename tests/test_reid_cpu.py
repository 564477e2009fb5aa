"""CPU: the re-identification embedder's restatement (tests/reid_ref.py), its weight module (reid_weights) and the argument checks
of rtmodt_reid_create / DeepSortTracker that run before any device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reid_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def RW(pkg):
    return pkg.reid_weights


@pytest.fixture(scope="module")
def synth(RW):
    return RW.synthetic(0)


# ------------------------------------------------------------------------------------------------------------- resize
def test_resize_identity_constant_single_pixel_and_monotone_ramp():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (256, 128, 3), dtype=np.uint8)
    assert np.array_equal(R.resize(img), img[..., ::-1])                       # a 128 x 256 rectangle: the identity (BGR -> RGB)
    for h, w in ((1, 1), (3, 7), (300, 200), (1, 50), (77, 1)):
        const = np.empty((h, w, 3), np.uint8)
        const[...] = (7, 130, 255)
        assert (R.resize(const) == np.asarray([255, 130, 7], np.uint8)).all()  # constant stays constant; 1 x 1 replicates its pixel
    for w in (2, 5, 64, 128, 300):
        ramp = np.repeat(np.round(np.linspace(0, 255, w)).astype(np.uint8)[None, :, None], 9, 0).repeat(3, 2)
        out = R.resize(ramp).astype(int)
        assert (np.diff(out, axis=1) >= 0).all() and (out == out[:1]).all() and out.min() >= 0 and out.max() <= 255
        assert w > 128 or (out[0, 0, 0] == 0 and out[0, -1, 0] == 255)             # upscaling replicates the edge pixels
    # the weights of every axis map sum to 2048 and the indices stay inside the source
    for n_out, shift in ((256, 4), (128, 8)):
        for n in (1, 2, 3, 127, 128, 129, 1000, 16384):
            lo, hi, w0, w1 = R.axis_map(n_out, n, shift)
            assert ((w0 + w1) == 2048).all() and lo.min() >= 0 and hi.max() <= n - 1 and (w1 >= 0).all()


def test_crop_box_rule_is_the_histogram_descriptors():
    frame = np.random.default_rng(1).integers(0, 256, (47, 33, 3), dtype=np.uint8)
    assert R.crop(frame, [5, 5, 5, 20]) is None and R.crop(frame, [float("nan"), 0, 9, 9]) is None and R.crop(frame, [-9, -9, -1, -1]) is None
    assert np.array_equal(R.crop(frame, [-1e9, -1e9, 1e9, 1e9]), R.resize(frame))
    assert np.array_equal(R.crop(frame, [3.99, 4.01, 20.5, 31.999]), R.resize(frame[4:31, 3:20]))


def test_normalisation_table_is_exact(RW):
    t = RW.norm_table()
    assert t.dtype == np.float16 and t.shape == (256, 3) and np.array_equal(t.view(np.uint16), R.norm_table().view(np.uint16))
    exact = (np.arange(256)[:, None] / 255.0 - np.asarray(RW.MEAN)) / np.asarray(RW.STD)
    assert np.abs(t.astype(np.float64) - exact).max() <= 2.0 ** -11 * np.abs(exact).max() * 1.001       # one fp16 rounding of the float64 value


def test_the_librarys_host_table_is_the_restatements_bit_for_bit(pkg):
    ffi = pkg._ffi
    got = np.full((256, 3), np.nan, np.float32)
    assert ffi.lib().rtmodt_reid_norm_table(ffi.ptr(got), got.nbytes) == ffi.OK       # no device, no handle
    want = R.norm_table()
    assert np.array_equal(got.astype(np.float16).astype(np.float32), got)          # float32 carriers of fp16 values
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert ffi.lib().rtmodt_reid_norm_table(ffi.ptr(got), got.nbytes - 1) == ffi.E_INVALID
    assert ffi.lib().rtmodt_reid_norm_table(None, got.nbytes) == ffi.E_INVALID


# ------------------------------------------------------------------------------------------------------------ weights
def _unfolded_torch_graph(sd, x):
    """torchreid's osnet_x0_25 forward in eval mode, written with unfolded BatchNorm straight from its state_dict, float64."""
    import torch
    import torch.nn.functional as F
    T = lambda k: torch.from_numpy(np.asarray(sd[k])).double()  # noqa: E731

    def bn(p, t):
        return F.batch_norm(t, T(p + ".running_mean"), T(p + ".running_var"), T(p + ".weight"), T(p + ".bias"), False, 0.0, 1e-5)

    def convbn(p, t, relu=True, **kw):
        y = bn(p + ".bn", F.conv2d(t, T(p + ".conv.weight"), **kw))
        return F.relu(y) if relu else y

    def light(p, t):
        w2 = T(p + ".conv2.weight")
        return F.relu(bn(p + ".bn", F.conv2d(F.conv2d(t, T(p + ".conv1.weight")), w2, padding=1, groups=w2.shape[0])))

    def gate(p, t):
        g = F.adaptive_avg_pool2d(t, 1)
        g = F.relu(F.conv2d(g, T(p + ".fc1.weight"), T(p + ".fc1.bias")))
        return t * torch.sigmoid(F.conv2d(g, T(p + ".fc2.weight"), T(p + ".fc2.bias")))

    def block(p, t):
        x1 = convbn(p + ".conv1", t)
        a = light(p + ".conv2a", x1)
        b = light(p + ".conv2b.1", light(p + ".conv2b.0", x1))
        c = light(p + ".conv2c.2", light(p + ".conv2c.1", light(p + ".conv2c.0", x1)))
        d = light(p + ".conv2d.3", light(p + ".conv2d.2", light(p + ".conv2d.1", light(p + ".conv2d.0", x1))))
        x2 = gate(p + ".gate", a) + gate(p + ".gate", b) + gate(p + ".gate", c) + gate(p + ".gate", d)
        idn = convbn(p + ".downsample", t, relu=False) if (p + ".downsample.conv.weight") in sd else t
        return F.relu(convbn(p + ".conv3", x2, relu=False) + idn)

    t = F.max_pool2d(convbn("conv1", x, stride=2, padding=3), 3, 2, 1)
    t = F.avg_pool2d(convbn("conv2.2.0", block("conv2.1", block("conv2.0", t))), 2)
    t = F.avg_pool2d(convbn("conv3.2.0", block("conv3.1", block("conv3.0", t))), 2)
    t = convbn("conv5", block("conv4.1", block("conv4.0", t)))
    v = F.adaptive_avg_pool2d(t, 1).flatten(1)
    v = F.linear(v, T("fc.0.weight"), T("fc.0.bias"))
    return F.relu(F.batch_norm(v, T("fc.1.running_mean"), T("fc.1.running_var"), T("fc.1.weight"), T("fc.1.bias"), False, 0.0, 1e-5))


def test_from_state_dict_equals_the_unfolded_graph_in_float64(RW):
    import torch
    sd = RW.synthetic_state_dict(3)
    assert any(k.startswith("classifier.") for k in sd)
    fused = RW.from_state_dict({"module." + k: v for k, v in sd.items()})          # DataParallel prefix accepted, classifier dropped
    assert set(fused) == set(RW.layer_shapes()) and not any("classifier" in k for k in fused)
    x = torch.from_numpy(np.ascontiguousarray(RW.normalize(RW.calibration_crops(2)).transpose(0, 3, 1, 2))).double()
    want = _unfolded_torch_graph(sd, x).numpy()
    assert want.max() > 1.0
    exact = RW.from_state_dict(sd, dtype=np.float64)                               # the fold itself, before its one cast
    assert all(w.dtype == b.dtype == np.float64 for w, b in exact.values())
    got = RW.torch_forward(x, exact, torch.float64)["feat"].numpy()
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    # the default is that fold cast once to float32, the form round_stored() and save() take
    assert all(fused[k][i].dtype == np.float32 and np.array_equal(fused[k][i], exact[k][i].astype(np.float32)) for k in exact for i in (0, 1))
    with pytest.raises(KeyError):
        RW.from_state_dict({k: v for k, v in sd.items() if k != "conv3.0.gate.fc1.bias"})


def test_save_load_round_trip_and_digest(RW, synth, tmp_path):
    path = str(tmp_path / "a.rtreid")
    d = RW.save(path, synth)
    back, d2 = RW.load(path)
    assert d == d2 == RW.digest(synth) and len(d) == 8
    assert list(back) == list(RW.layer_shapes())
    assert all(np.array_equal(synth[k][0], back[k][0]) and np.array_equal(synth[k][1], back[k][1]) for k in synth)
    other = dict(synth)
    other["fc"] = (synth["fc"][0], synth["fc"][1] + np.float32(1))
    assert RW.digest(other) != d
    raw = bytearray(open(path, "rb").read())
    raw[len(raw) // 2] ^= 1
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="digest"):
        RW.load(path)
    with pytest.raises(ValueError, match="osnet_x0_25 has"):
        RW.save(path, {**synth, "conv5": (np.zeros((64, 128), np.float32), np.zeros(64, np.float32))})


def test_converter_cli_reads_a_torch_checkpoint(RW, tmp_path):
    import torch
    sd = RW.synthetic_state_dict(5, calibrate=False)
    pt, out = str(tmp_path / "osnet_x0_25.pth"), str(tmp_path / "osnet_x0_25.rtreid")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, pt)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--reid", pt, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, dg = RW.load(out)
    want = RW.round_stored(RW.from_state_dict(sd))
    assert dg in r.stdout and all(np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]) for k in want)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--reid", pt, str(tmp_path / "x.onnx")], capture_output=True, text=True)
    assert r.returncode != 0 and ".rtreid" in r.stderr


def test_synthetic_tap_range_and_determinism(RW, synth):
    import torch
    assert RW.digest(RW.synthetic(0)) == RW.digest(synth) != RW.digest(RW.synthetic(1))
    x = torch.from_numpy(np.ascontiguousarray(RW.normalize(RW.calibration_crops()).transpose(0, 3, 1, 2)))
    taps = RW.torch_forward(x, synth, torch.float64)
    lo, hi = RW.SYNTHETIC_TAP_STD
    assert list(taps) == list(RW.TAPS[1:])
    for k, t in taps.items():
        assert lo <= float(t.std()) <= hi, (k, float(t.std()))
        assert float(t.abs().max()) < 1000.0                                      # nowhere near fp16's range
    for k, (w, b) in synth.items():                                               # stored values: fp16 except the gate
        assert RW.is_fp32(k) or np.array_equal(w, w.astype(np.float16).astype(np.float32)), k


def test_emulator_without_roundings_equals_float64_and_the_restatement(RW, synth):
    import torch
    crops = RW.calibration_crops(2)
    x = torch.from_numpy(np.ascontiguousarray(RW.normalize(crops).transpose(0, 3, 1, 2)))
    a = RW.torch_forward(x, synth, torch.float64, emulate=False)
    ref = R.forward(crops, synth)                                                 # the NumPy restatement: other code, same network
    emu_t = RW.torch_forward(x, synth, torch.float32, emulate=True)
    emu_n = R.forward(crops, synth, emulate=True)
    for k in RW.TAPS[1:]:
        t = a[k].numpy()
        t = t.transpose(0, 2, 3, 1) if t.ndim == 4 else t
        assert np.abs(t - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), k
        e = emu_t[k].numpy().astype(np.float64)
        e = e.transpose(0, 2, 3, 1) if e.ndim == 4 else e
        err = np.abs(e - ref[k]).max() / np.abs(ref[k]).max()
        assert 0 < err < 1e-2 or k == "maxpool", (k, err)                         # the roundings are really inserted, and are fp16-sized
        assert np.abs(e - emu_n[k]).max() <= 4e-3 * np.abs(ref[k]).max(), k       # float32 against exact accumulation: a few fp16 flips


def test_mutations_move_the_restatement(RW, synth):
    crops = RW.calibration_crops(2)
    ref = R.forward(crops, synth)
    w3 = RW.round_stored(RW.from_state_dict(RW.synthetic_state_dict(0), eps=1e-3))
    for m in R.MUTATIONS:
        k = R.FIRST_TAP[m]
        mut = R.forward(crops, w3 if m == "eps1e-3" else synth, mutate=m)
        before = R.TAPS[1:R.TAPS.index(k)]
        assert all(np.array_equal(mut[b], ref[b]) for b in before), m
        assert np.abs(mut[k] - ref[k]).max() > 5 * max(R.TOL_TAP[k], R.TOL_CONV) * np.abs(mut[k]).max(), m


def test_lsb_bound_covers_a_perturbed_feature():
    rng = np.random.default_rng(4)
    f = np.maximum(rng.normal(0, 3, (6, 512)), 0)
    eps = R.TOL_FEAT * np.abs(f).max()
    n = R.lsb_bound(f, eps)
    worst = 0
    for _ in range(20):
        g = f + rng.choice([-eps, eps], f.shape)
        worst = max(worst, int(np.abs(R.quantize_rows(g).astype(int) - R.quantize_rows(f).astype(int)).max()))
    assert 1 <= worst <= n <= 3


# ----------------------------------------------------------------------------------------------------- argument checks
def test_reid_create_refuses_bad_arguments_before_the_device(pkg, RW, synth, tmp_path):
    ffi = pkg._ffi
    L = ffi.lib()
    good = str(tmp_path / "g.rtreid")
    RW.save(good, synth)
    h = C.c_void_p()

    def rc(path, frames=2, boxes=8, device=0):
        cfg = ffi.ReidCfg(None if path is None else str(path).encode(), device, frames, boxes)
        r = L.rtmodt_reid_create(C.byref(cfg), C.byref(h))
        assert not h.value
        return r

    assert rc(tmp_path / "missing.rtreid") == ffi.E_INVALID and "not found" in L.rtmodt_last_error().decode()
    assert rc(None) == ffi.E_INVALID
    raw = bytearray(open(good, "rb").read())
    raw[-5] ^= 0x40
    bad = tmp_path / "bad.rtreid"
    bad.write_bytes(bytes(raw))
    assert rc(bad) == ffi.E_INVALID and "digest" in L.rtmodt_last_error().decode()
    junk = tmp_path / "junk.rtreid"
    junk.write_bytes(b"RTMODTW1" + bytes(200))
    assert rc(junk) == ffi.E_INVALID
    # a crafted file: the digest is right, a record's offset is not -- near 2^64 (offset + size wraps), and just past the end
    import struct
    import zlib
    for field, value in ((72, 2 ** 64 - 64), (80, 2 ** 64 - 4), (72, len(raw) - 4), (80, len(raw))):
        forged = bytearray(open(good, "rb").read())
        struct.pack_into("<Q", forged, 24 + 3 * 96 + field, value)                     # record 3: w_offset at +72, b_offset at +80
        struct.pack_into("<I", forged, 16, zlib.crc32(bytes(forged[24:])) & 0xFFFFFFFF)
        forged_path = tmp_path / "forged.rtreid"
        forged_path.write_bytes(bytes(forged))
        assert rc(forged_path) == ffi.E_INVALID and "outside the file" in L.rtmodt_last_error().decode(), (field, value)
    assert rc(good, frames=0) == ffi.E_INVALID and rc(good, boxes=0) == ffi.E_INVALID
    assert rc(good, frames=64, boxes=1024) == ffi.E_CAPACITY and "65536 crops" in L.rtmodt_last_error().decode()      # the size asked for is named
    assert rc(good, frames=65) == ffi.E_CAPACITY and rc(good, boxes=1025) == ffi.E_CAPACITY and rc(good, frames=64, boxes=1024) == ffi.E_CAPACITY
    assert L.rtmodt_reid_create(None, C.byref(h)) == ffi.E_INVALID
    # the file save() writes is the file the C reader accepts: a good file gets past every check, up to the device (absent here: E_HIP)
    cfg = ffi.ReidCfg(good.encode(), 0, 2, 8)
    r = L.rtmodt_reid_create(C.byref(cfg), C.byref(h))
    assert r in (ffi.OK, ffi.E_HIP), L.rtmodt_last_error().decode()
    if r == ffi.OK:
        L.rtmodt_reid_destroy(h)
        h.value = None
    # the tracker's embedder field: the same checks, still before the device; an .onnx stays unsupported
    def ds(emb, dim=0):
        cfg = ffi.DeepSortCfg(0.2, 0.3, 0.7, 70, 3, 100, emb, dim, 32, 16, 1, 0)
        r = L.rtmodt_deepsort_create(C.byref(cfg), C.byref(h))
        assert not h.value
        return r
    assert ds(str(tmp_path / "missing.rtreid").encode()) == ffi.E_INVALID
    assert ds(str(bad).encode()) == ffi.E_INVALID
    assert ds(good.encode(), dim=192) == ffi.E_INVALID
    assert ds(b"weights/osnet_x0_25.onnx") == ffi.E_UNSUPPORTED and "--reid" in L.rtmodt_last_error().decode()


def test_tracker_with_a_missing_rtreid_file_raises_file_not_found(pkg, tmp_path):
    with pytest.raises(FileNotFoundError, match="No Re-ID model found at"):
        pkg.DeepSortTracker(embedder=str(tmp_path / "missing.rtreid"))
    with pytest.raises(FileNotFoundError, match="No Re-ID model found at"):
        pkg.DeepSortTracker.from_config({"deepsort": {"embedder": str(tmp_path / "missing.rtreid")}})
    with pytest.raises(FileNotFoundError):
        pkg.tracking.ReidEmbedder(str(tmp_path / "missing.rtreid"))
    with pytest.raises(ValueError, match=".rtreid"):
        pkg.tracking.ReidEmbedder("weights/osnet_x0_25.onnx")
    with pytest.raises(NotImplementedError, match="convert_weights.py --reid"):
        pkg.DeepSortTracker(embedder="weights/osnet_x0_25.onnx")
