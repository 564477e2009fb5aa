"""CPU: the JPEG decoder's rules as tests/jpeg_dec_ref.py restates them, judged by libjpeg-turbo itself (through Pillow), and the
host-only pieces of the decoder: csrc/jpeg_dec_core.h run natively (plain and under the address / undefined-behaviour sanitizers) on
valid and damaged streams, rtmodt_jpeg_probe, and MjpegCapture's container splitting.

Against libjpeg: PARITY PINNED.  jpeg_dec_ref.decode equals Pillow's pixels byte for byte on 1 600 files (sizes 1 x 1 .. 50 x 70 with
partial MCUs and chroma widths 1, 2 and 3; 4:4:4, 4:2:2, 4:2:0, grayscale; qualities 30 .. 100; noise and smooth content; with and
without restart markers, optimised tables) plus this tree's own encoder's files, flat frames and a saturated checkerboard.
Missing DHT (AVI MJPG): Pillow on libjpeg-turbo decodes a file whose DHT segments were removed with the Annex K tables, to the same
pixels as the complete file -- test_missing_dht_uses_annex_k asserts it -- so the decoder ACCEPTS such files and does the same.
Behaviour on damaged streams is this decoder's own (statuses, no concealment): unpinned against libjpeg."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_dec_cases as K
import jpeg_dec_ref as D
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "real-time-multi-object-detection---tracking-system_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "jpeg_dec_check.cpp")

MAIN_SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (31, 15), (40, 2), (24, 24), (33, 49), (50, 70)]
NARROW_SIZES = [(40, 2), (5, 3), (20, 4), (7, 5), (3, 6), (2, 40), (33, 1)]
GRID_MARKERS = ["none", "row", "mcu3", "optimised"]


def check_against_pillow(file, what):
    want = K.pillow_pixels(file)
    got = D.decode(file)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {int(np.count_nonzero(got != want))} bytes differ from libjpeg-turbo's"


@pytest.mark.parametrize("ss", K.SUBSAMPLINGS)
@pytest.mark.parametrize("h,w", MAIN_SIZES)
def test_restatement_equals_libjpeg_main_sweep(h, w, ss):
    for q in (30, 75, 95, 100):
        for kind in ("noise", "smooth"):
            for marker in GRID_MARKERS:
                check_against_pillow(K.pillow_file(K.frame(kind, h, w), q, ss, marker), (h, w, ss, q, kind, marker))


@pytest.mark.parametrize("ss", K.SUBSAMPLINGS)
@pytest.mark.parametrize("h,w", NARROW_SIZES)
def test_restatement_equals_libjpeg_narrow_sweep(h, w, ss):
    for q in (30, 95):
        for kind in ("noise", "smooth"):
            for marker in GRID_MARKERS:
                check_against_pillow(K.pillow_file(K.frame(kind, h, w), q, ss, marker), (h, w, ss, q, kind, marker))


def test_restatement_equals_libjpeg_on_other_files():
    for h, w in ((1, 1), (16, 16), (37, 53), (48, 64)):                     # this tree's own encoder (jpeg_ref restates it)
        for q in (5, 85, 100):
            check_against_pillow(J.encode(K.frame("noise", h, w), q), ("jpeg_ref.encode", h, w, q))
    for ss in K.SUBSAMPLINGS:
        for h, w in ((17, 33), (48, 64)):
            check_against_pillow(K.pillow_file(K.frame("flat", h, w), 75, ss), ("flat", h, w, ss))
            for marker in ("none", "mcu1"):                                     # the range-limit wrap
                f = K.pillow_file(K.frame("checker", h, w), 100, ss, marker)
                check_against_pillow(f, ("checker", h, w, ss, marker))
    f = K.pillow_file(K.frame("checker", 48, 64), 100, "444")
    raw = D.idct_raw(D.coefficients(f)[0], D.parse(f).qt[0])
    assert raw.min() + 128 < 0 and raw.max() + 128 > 255, "the checkerboard stays inside 0..255: the range limit is not exercised"


def test_missing_dht_uses_annex_k():
    """AVI MJPG frames carry no DHT.  libjpeg-turbo installs the Annex K tables for them; so does this decoder."""
    for ss in K.SUBSAMPLINGS:
        whole = K.pillow_file(K.frame("noise", 31, 45), 80, ss, "row")
        bare = K.without_segments(whole, 0xC4)
        assert len(bare) < len(whole) and b"\xff\xc4" not in bare[:D.parse(bare).scan_off]
        assert np.array_equal(K.pillow_pixels(bare), K.pillow_pixels(whole)), "Pillow does not decode a file without DHT: the rule would be UNSUPPORTED"
        assert np.array_equal(D.decode(bare), K.pillow_pixels(whole))
        assert D.coefficient_hash(D.coefficients(bare)) == D.coefficient_hash(D.coefficients(whole))


# ---- rtmodt_jpeg_probe ----------------------------------------------------------------------------------------------------------
def probe(pkg, file):
    info = pkg._ffi.JpegInfo()
    buf = np.frombuffer(bytes(file), np.uint8)
    assert pkg._ffi.lib().rtmodt_jpeg_probe(pkg._ffi.ptr(buf) if len(buf) else None, len(buf), C.byref(info)) == 0
    return info


def patched(file, marker, offset, value):
    """byte `offset` of the first `marker` segment's payload set to `value`"""
    d = bytearray(file)
    at = next(a for m, a, _ in K.segments(file) if m == marker)
    d[at + 4 + offset] = value
    return bytes(d)


def unsupported_files():
    base = K.pillow_file(K.frame("smooth", 24, 40), 80, "420")
    sof = next(a for m, a, _ in K.segments(base) if m == 0xC0)
    sos, sos_len = next((a, ln) for m, a, ln in K.segments(base) if m == 0xDA)
    out = {}
    b = io.BytesIO()
    Image.fromarray(K.frame("smooth", 24, 40)).save(b, "JPEG", progressive=True)
    out["progressive"] = (b.getvalue(), "progressive")
    for name, m in (("extended", 0xC1), ("lossless", 0xC3), ("arithmetic", 0xC9)):
        d = bytearray(base)
        d[sof + 1] = m
        out[name] = (bytes(d), name)
    out["12-bit"] = (patched(base, 0xC0, 0, 12), "12-bit")
    out["4 components"] = (patched(base, 0xC0, 5, 4), "4 components")
    out["sampling 1x2"] = (patched(base, 0xC0, 7, 0x12), "sampling")
    out["sampling 4x1"] = (patched(base, 0xC0, 7, 0x41), "sampling")
    out["chroma 2x1"] = (patched(K.pillow_file(K.frame("smooth", 24, 40), 80, "444"), 0xC0, 10, 0x21), "sampling")
    one = bytes([0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0])
    out["multiple scans"] = (base[:sos] + one + base[sos + sos_len:], "multiple scans")
    adobe = bytes([0xFF, 0xEE, 0, 14]) + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0])
    out["adobe rgb"] = (base[:2] + adobe + base[2:], "Adobe")
    return out


def test_probe(pkg):
    E = pkg._ffi
    for ss, (hs, vs, nc) in {"444": (1, 1, 3), "422": (2, 1, 3), "420": (2, 2, 3), "gray": (1, 1, 1)}.items():
        for marker, h, w in (("none", 17, 33), ("row", 48, 64), ("mcu3", 31, 15)):
            f = K.pillow_file(K.frame("noise", h, w), 75, ss, marker)
            i, H = probe(pkg, f), D.parse(f)
            assert (i.status, i.h, i.w, i.components, i.h_samp, i.v_samp, i.restart_interval) == (D.OK, h, w, nc, hs, vs, H.ri), (ss, marker)
            assert H.ri == {"none": 0, "row": H.mcus_x, "mcu3": 3}[marker]
    i = probe(pkg, J.encode(K.frame("noise", 37, 53), 90))
    assert (i.status, i.h, i.w, i.components, i.h_samp, i.v_samp, i.restart_interval) == (D.OK, 37, 53, 3, 2, 2, 4)
    for name, (f, word) in unsupported_files().items():
        i = probe(pkg, f)
        assert i.status == D.UNSUPPORTED == D.status_of(f), (name, i.status, D.status_of(f))
        assert word.lower() in i.message.decode().lower(), (name, i.message)
    good = K.pillow_file(K.frame("noise", 24, 40), 80, "420", "row")
    for f in (b"", b"\xff", b"\xff\xd8", good[:40], good[:D.parse(good).scan_off - 1], b"\x00" + good, good[:2] + b"\x12" + good[2:],
              K.oversubscribed_dht(good), K.without_segments(good, 0xDB), K.without_segments(good, 0xC0)):
        assert probe(pkg, f).status == D.status_of(f) != D.OK, f[:8]
    assert probe(pkg, good[:D.parse(good).scan_off]).status == D.OK            # the header is all the probe reads
    info = E.JpegInfo()
    assert E.lib().rtmodt_jpeg_probe(None, 4, C.byref(info)) == E.E_INVALID
    assert E.lib().rtmodt_jpeg_probe(E.ptr(np.frombuffer(good, np.uint8)), len(good), None) == E.E_INVALID


# ---- the native program ---------------------------------------------------------------------------------------------------------
def rocm_root():
    for r in (os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"):
        if r and os.path.isfile(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return r
    raise AssertionError("no ROCm headers (hip/hip_runtime.h) found")


def build(tmp_path, sanitize):
    rocm = rocm_root()
    clang = [p for p in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.isfile(p)]
    gxx = [p for p in (shutil.which("g++"),) if p]
    exe = str(tmp_path / ("jpeg_dec_check_san" if sanitize else "jpeg_dec_check"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    errors = []
    for cxx in (clang + gxx if sanitize else gxx + clang):
        cmd = [cxx, "-x", "c++", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(rocm, "include"), SRC, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    raise AssertionError("no host compiler built jpeg_dec_check" + (" with the sanitizers" if sanitize else "") + ":\n" + "\n".join(errors))


def damaged_files():
    rng = np.random.default_rng(20240917)
    bases = [K.pillow_file(K.frame("noise", 48, 64), 75, "420", "row"), K.pillow_file(K.frame("noise", 33, 49), 90, "444", "none"),
             K.pillow_file(K.frame("smooth", 31, 45), 60, "422", "mcu3"), K.pillow_file(K.frame("noise", 40, 40), 85, "gray", "optimised")]
    out = []
    for b in bases:
        out += [K.truncated(b, f) for f in (0.02, 0.25, 0.5, 0.75, 0.98)]
    for i in range(200):
        out.append(K.flipped(bases[i % len(bases)], rng))
    for b in (bases[0], bases[2]):
        out += [K.without_restart(b, 1), K.renumbered_restart(b, 1), K.renumbered_restart(b, 0)]
    out += [K.oversubscribed_dht(b) for b in bases]
    out += [b[:n] for b in bases[:2] for n in (0, 1, 2, 3, 20, 100, 200)]          # cuts inside the header
    return out


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    """(list file, [(status, hash)] from the restatement): the valid grid (one content and quality per cell), files without DHT, damaged streams"""
    files = []
    for ss in K.SUBSAMPLINGS:
        for h, w in MAIN_SIZES + NARROW_SIZES:
            for marker in GRID_MARKERS + ["mcu1"]:
                files.append(K.pillow_file(K.frame("noise" if (h + w) % 2 else "smooth", h, w), 95 if h % 2 else 30, ss, marker))
        files.append(K.without_segments(K.pillow_file(K.frame("noise", 31, 45), 80, ss, "row"), 0xC4))
        files.append(K.pillow_file(K.frame("checker", 48, 64), 100, ss, "mcu3"))
    files.append(J.encode(K.frame("noise", 136, 250), 95))
    n_valid = len(files)
    files += damaged_files()
    files += [f for f, _ in unsupported_files().values()]
    d = tmp_path_factory.mktemp("jpegdec")
    ref = []
    with open(d / "list.txt", "w") as lst:
        for i, f in enumerate(files):
            (d / f"{i}.jpg").write_bytes(f)
            try:
                _, coefs, st = D.entropy_decode(f)
            except D.JpegError as e:
                st, coefs = e.status, None
            ref.append((st, D.coefficient_hash(coefs) if st == D.OK else 0))
            lst.write(f"{d / f'{i}.jpg'} {st}\n")
    assert all(st == D.OK for st, _ in ref[:n_valid])
    seen = {st for st, _ in ref[n_valid:]}
    assert {D.OK, D.UNSUPPORTED, D.CORRUPT, D.TRUNCATED} <= seen, seen            # (a flipped byte can leave a decodable stream)
    return str(d / "list.txt"), ref


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_core_on_the_host(tmp_path, streams, sanitize):
    path, ref = streams
    exe = build(tmp_path, sanitize)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = [(int(l.split()[1]), int(l.split()[2], 16)) for l in out.stdout.splitlines()]
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (i, g, r)


# ---- containers -----------------------------------------------------------------------------------------------------------------
def test_container_round_trip(pkg, tmp_path):
    V, M = pkg.visualization.jpeg, pkg.ingestion
    jpegs = [J.encode(K.frame("noise", 48, 64, seed=s) >> (s % 5), 80) for s in range(7)] + [K.pillow_file(K.frame("smooth", 48, 64), 70, "444")]
    assert any(len(j) % 2 for j in jpegs) and any(len(j) % 2 == 0 for j in jpegs)
    for name in ("clip.avi", "clip.mjpeg", "clip.multipart"):
        path = str(tmp_path / name)
        if name.endswith(".multipart"):
            with open(path, "wb") as f:
                for j in jpegs:
                    f.write(V.multipart_chunk(j))
        else:
            with V.MjpegWriter(path, 25, (64, 48)) as wr:
                for j in jpegs:
                    wr.write(j)
        cap = M.MjpegCapture(path, resolution=(64, 48))
        assert cap.opened
        back = []
        while cap.grab():
            back.append(cap.jpeg)
        cap.release()
        assert not cap.opened and not cap.grab()
        assert len(back) == len(jpegs) and back == jpegs, name
    with pytest.raises(ConnectionError):
        M.MjpegCapture(str(tmp_path / "missing.avi"))
    assert M.reader._BACKENDS["mjpeg"] is M.MjpegCapture and pkg.ingestion.JpegDecoder is pkg.ingestion.jpeg_decode.JpegDecoder
