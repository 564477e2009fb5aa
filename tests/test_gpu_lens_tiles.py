"""GPU: the lens corrector (``csrc/lens.hip``) past one tile, one wave and at its size limits, with the cases of
``tests/lens_cases.py`` (``tests/test_lens_cases_cpu.py`` proves that each reaches what it is here for): two to 64 tile columns, one
to 4096 row bands, the partial run at a row's end in a tile other than the first, full waves, the 12-byte store and the byte path per
destination pitch and base address, sources of 1 x 1 and 2 x 2, 16384 pixels in each axis, a hostile map in every tile column; 70
frames of three lenses in one launch; both store paths from one handle.  Table and bytes equal ``tests/lens_ref.py`` (``==`` on
integers), guard bytes around every row included.  One test compares the kernel with a float64 bilinear reference that shares nothing
with the restatement's rules 2 and 3, under a derived bound; one runs decoder -> lens -> detector on device memory alone."""
import os

import numpy as np
import pytest

import jpeg_dec_cases as K
import jpeg_dec_ref as D
import lens_cases as L
import lens_ref as R
from lens_cases import BORDER, SENT, image, random_frames, rectify
from oracle import yolo_oracle as Y

pytestmark = pytest.mark.gpu

IDS = [c.name for c in L.CASES]
ALL_KINDS = ("three_tiles_odd", "wide_260")                                    # every combination of host and device memory


def set_case(lc, stream, case):
    if case.lens is not None:
        return lc.set_model(stream, case.lens.K, case.lens.k, case.lens.new_K, case.lens.r2_limit)
    return lc.set_map(stream, *case.map)


# ---------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("case", L.CASES, ids=IDS)
def test_case_table_and_bytes_equal_restatement(pkg, case):
    want_table = L.table(case.name)
    lc = pkg.ingestion.LensCorrector(1, case.src, case.out, border=BORDER)
    assert set_case(lc, 0, case) == int(want_table[2].sum())
    got_table = lc.map(0)
    assert len(got_table) == 3 and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got_table, want_table))
    n = 3 if case.name in L.MAX_CASES else 2
    frames = random_frames(n, case.src, 300 + case.out[1])
    want = [R.sample(f, want_table, BORDER) for f in frames]
    kinds = [("host", "host"), ("device", "device")] + ([("host", "device"), ("device", "host")] if case.name in ALL_KINDS else [])
    for src_kind, dst_kind in kinds:
        for offset in (0, 1):
            for dextra in case.dextras:
                got = rectify(lc, pkg, frames, [0] * n, case.out, src_kind=src_kind, dst_kind=dst_kind, spitch=3 * case.src[1] + 5,
                              dpitch=3 * case.out[1] + dextra, offset=offset)
                for i in range(n):
                    bad = np.argwhere((got[i] != want[i]).any(axis=2))
                    assert len(bad) == 0, (case.name, src_kind, dst_kind, offset, dextra, i, len(bad), bad[:8].tolist())     # (row, column) of wrong pixels
    lc.close()


# ---------------------------------------------------------------------------------------------------------------- batch and streams
def test_seventy_frames_of_three_lenses_in_one_launch(pkg):
    """gridDim.y = 70 (more slots than a wave has lanes, a 2240-byte command block), every frame through the lens of its stream."""
    case = L.BY_NAME["two_tiles_plus_1"]
    src, out = case.src, case.out
    lenses = [case.lens, L.axis_lens("pincushion", src, out, 1.0, 1.6), L.axis_lens("rational", src, out, 0.9, 2.1, dcx=-2.0)]
    tables = [L.table(case.name)] + [R.build_model(m, src, out) for m in lenses[1:]]
    lc = pkg.ingestion.LensCorrector(3, src, out, border=BORDER)
    for s, m in enumerate(lenses):
        assert lc.set_model(s, m.K, m.k, m.new_K) == int(tables[s][2].sum())
    streams = [i % 3 for i in range(70)]
    frames = random_frames(70, src, 70)
    want = [R.sample(f, tables[s], BORDER) for f, s in zip(frames, streams)]
    assert not np.array_equal(R.sample(frames[0], tables[1], BORDER), want[0])                   # the lenses differ where it shows
    for kind in ("device", "host"):
        got = rectify(lc, pkg, frames, streams, out, src_kind=kind, dst_kind=kind, spitch=3 * src[1] + 5, dpitch=3 * out[1] + 7, offset=1)
        assert len(got) == 70
        for i in range(70):
            assert np.array_equal(got[i], want[i]), (kind, i, streams[i])
    lc.close()


# ---------------------------------------------------------------------------------------------------------------- both store paths
def test_wide_and_narrow_stores_from_one_handle(pkg):
    """The same device destination at an offset that is a multiple of 4 (12-byte stores), at offset 1 (bytes) and back: the kernel is
    chosen per call."""
    F = pkg._ffi
    case = L.BY_NAME["wide_260"]
    (sh, sw), (oh, ow) = case.src, case.out
    dpitch = 3 * ow
    assert dpitch % 4 == 0
    lc = pkg.ingestion.LensCorrector(1, case.src, case.out, border=BORDER)
    set_case(lc, 0, case)
    frames = random_frames(2, case.src, 41)
    want = [R.sample(f, L.table(case.name), BORDER) for f in frames]
    src = F.DeviceBuffer(2 * sh * 3 * sw)
    src.upload(np.concatenate([f.ravel() for f in frames]))
    dst = F.DeviceBuffer(8 + 2 * oh * dpitch + 8)
    for offset in (8, 1, 4, 3):
        dst.upload(np.full(dst.nbytes, SENT, np.uint8))
        assert lc.process(src, [0, 0], dst, out_offset=offset) is dst
        expect = np.full(dst.nbytes, SENT, np.uint8)
        expect[:offset + 2 * oh * dpitch + 8] = image(want, dpitch, offset)
        assert np.array_equal(dst.download(), expect), offset
    lc.close()


# ---------------------------------------------------------------------------------------------------------------- float64 reference
@pytest.mark.parametrize("name", ["three_tiles_odd", "wide_260", "exact_tiles"])
def test_float64_bilinear_bound(pkg, name):
    """|kernel - float64 bilinear interpolation at the unquantised position| <= 0.5 + G / 32 on every pixel whose taps are on the source
    with a pixel to spare (L.float64_bound has the derivation; G = 7 for the ramps used), and every pixel off the source is the border
    colour.  The reference uses R.lens_map alone: neither the quantisation nor the integer blend of the restatement."""
    case = L.BY_NAME[name]
    frame, G = L.smooth_frame(case.src)
    lc = pkg.ingestion.LensCorrector(1, case.src, case.out, border=BORDER)
    set_case(lc, 0, case)
    out = lc.process([frame])[0]
    lc.close()
    worst, n_inner, n_off = L.float64_check(case.lens, case.src, case.out, frame, G, out, BORDER)
    print(f"{name}: worst |kernel - float64| {worst:.4f} over {n_inner} pixels, bound {L.float64_bound(G):.4f} (G = {G}); {n_off} pixels off the source are border")
    assert n_inner >= 500 and n_off >= 100


# ---------------------------------------------------------------------------------------------------------------- the device ingest chain
def test_decoded_frames_rectified_on_the_device_reach_the_detector(pkg, tmp_path):
    """JpegDecoder -> LensCorrector -> Detector on device memory alone: three handles, three streams, no host hop.  The detector's
    letterboxed fp16 input equals the oracle's preprocessing of the restated rectification of the restated decode, bit for bit."""
    F = pkg._ffi
    src, out, size = (24, 530), (20, 521), 320
    (sh, sw), (oh, ow) = src, out
    files = [K.pillow_file(K.frame(kind, sh, sw, seed=s), 90, "420", "row") for s, kind in enumerate(("noise", "smooth"))]
    pixels = []
    for f in files:
        H, coefs, st = D.entropy_decode(f)
        assert st == D.OK and (H.h, H.w) == src
        pixels.append(D.pixels(H, coefs))
    lenses = [L.axis_lens("barrel", src, out, 1.05, 1.3), L.axis_lens("tangential", src, out, 0.95, 1.5, dcx=-3.0)]
    tables = [R.build_model(m, src, out) for m in lenses]
    want = [Y.preprocess(R.sample(pixels[i], tables[i], BORDER), size, size).astype(np.float16) for i in range(2)]

    path = os.path.join(str(tmp_path), f"yolov8n_{size}.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=size), "n")
    det = pkg.Detector(path, input_size=(size, size), confidence=0.02, max_det=20, batch=2, warmup=False, autotune=False)
    dec = pkg.ingestion.JpegDecoder(max_height=32, max_width=544, max_batch=2, max_file_bytes=1 << 18)
    lc = pkg.ingestion.LensCorrector(2, src, out, border=BORDER)
    for s, m in enumerate(lenses):
        lc.set_model(s, m.K, m.k, m.new_K)
    dev_a, dev_b = F.DeviceBuffer(2 * sh * 3 * sw), F.DeviceBuffer(2 * oh * 3 * ow)
    for _ in range(2):                                                        # the second round runs over buffers the first one left in use
        _, status = dec.decode_batch(files, out=dev_a, height=sh, width=sw)
        assert status.tolist() == [D.OK, D.OK]
        assert lc.process(dev_a, out=dev_b) is dev_b
        det.enqueue([dev_b.ptr + i * oh * 3 * ow for i in range(2)], height=oh, width=ow)
        det.fetch()
        for i in range(2):
            inp = det.debug_fetch(i, want_heads=False, want_pred=False)[0]
            assert inp.shape == want[i].shape and np.array_equal(inp.view(np.uint16), want[i].view(np.uint16)), i
    assert not np.array_equal(want[0].view(np.uint16), want[1].view(np.uint16))
    lc.close(); dec.close(); det.close()
