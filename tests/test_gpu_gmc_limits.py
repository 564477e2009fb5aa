"""GPU: the camera-motion estimator (csrc/gmc.hip) against its restatement (tests/gmc_ref.py) on the cases of tests/gmc_cases.py: the
default downscale of 4 at every row and frame alignment, host and device frames; downscale 8; the widest level 1; 4096 blocks; mask
boxes past one wave, at their limit and on their float edges; every block reason; the FEW_INLIERS exits pixels can reach; early
returns beside a full fit; a host frame that ends on its buffer's last byte.  Every comparison is tests/gmc_run.py's: every
intermediate rtmodt_gmc_debug returns, the warp's bits and the status, after every frame.  tests/test_gmc_cases_cpu.py proves that
each case reaches what it is named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmc_cases as K  # noqa: E402
import gmc_ref as G  # noqa: E402
from gmc_run import _est, _same  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _run_case(pkg, name, ref_name=None):
    """The case's frames through one estimator, every frame and stream compared with the restatement's stored result."""
    c, ref = K.case(name), K.reference(ref_name or name)
    est = _est(pkg, n_streams=len(c.streams), **c.cfg)
    seen = []
    for f in range(len(ref)):
        warp, status = est.estimate([st[f] for st in c.streams], c.masks)
        for s in range(len(c.streams)):
            _same(est, s, warp[s], status[s], ref[f][s], (name, f, s))
        seen.append(status.tolist())
    est.close()
    return seen


@pytest.mark.parametrize("name", [n for n in K.NAMES if not n.startswith("crop")])
def test_case_equals_the_restatement(pkg, name):
    seen = _run_case(pkg, name)
    assert seen == [[st for _, st, _ in row] for row in K.reference(name)]


def test_crop_view_and_contiguous_copy_give_the_same_result(pkg):
    """A frame whose last pixel is its buffer's last byte, rows at the parent's pitch, and a contiguous copy of its pixels: both equal
    ONE stored result of the restatement, so they equal each other in every intermediate."""
    assert _run_case(pkg, "crop-view", "crop-copy") == _run_case(pkg, "crop-copy", "crop-copy")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("name", K.D4_NAMES)
def test_d4_device_frames_at_every_byte_alignment(pkg, name, off):
    """The d = 4 cases with frames that already stand on the device, stream s at an address that is (off + s) mod 4: the same bits, and
    neither the frames nor the bytes around them are written."""
    F = pkg._ffi
    c, ref = K.case(name), K.reference(name)
    S = len(c.streams)
    h, w = c.streams[0][0].shape[:2]
    pitch = c.streams[0][0].strides[0]
    own = (h - 1) * pitch + 3 * w
    slot = (own + 3) // 4 * 4 + 32
    at = [32 + s * slot + (off + s) % 4 for s in range(S)]
    dev = F.DeviceBuffer(32 + S * slot + 32)
    est = _est(pkg, n_streams=S, **c.cfg)
    for f in range(len(ref)):
        image = np.full(dev.nbytes, K.GUARD, np.uint8)
        for s in range(S):
            image[at[s]:at[s] + own] = K.frame_bytes(c.streams[s][f])
        dev.upload(image)
        assert [(dev.ptr + a) % 4 for a in at] == [(off + s) % 4 for s in range(S)]
        warp, status = est.estimate([dev.ptr + a for a in at], mem_kind=F.MEM_DEVICE, height=h, width=w, stride=pitch)
        for s in range(S):
            _same(est, s, warp[s], status[s], ref[f][s], (name, off, f, s))
        assert np.array_equal(dev.download(), image), "the device frames or the bytes around them were written"
    est.close()
    dev.free()


def _raw_estimate(pkg, est, frame, n_boxes):
    """rtmodt_gmc_estimate_batch itself, one stream, n_boxes boxes that meet nothing -> its return code."""
    F = pkg._ffi
    fp, keep, h, w, pitch = F.frame_pointers([frame], F.MEM_HOST)
    xy, cf, cnt = np.full((1, n_boxes, 4), -5, F32), np.ones((1, n_boxes), F32), np.asarray([n_boxes], np.int32)
    warp, status = np.zeros((1, 2, 3), F32), np.zeros(1, np.int32)
    return F.lib().rtmodt_gmc_estimate_batch(est.handle, fp, h, w, pitch, F.MEM_HOST, F.ptr(xy), F.ptr(cf), F.ptr(cnt), F.ptr(warp), F.ptr(status))


@pytest.mark.parametrize("name,too_large", [("widest", (160, 3841)), ("blocks-4096-d1", (1024, 1040))])
def test_one_past_a_limit_is_refused_and_the_handle_gives_the_next_result(pkg, name, too_large):
    """3840 x 160 and 1024 x 1024 run; one column more than 3840 (2400 blocks), one block column more than 4096 blocks and one box more
    than 1024 are E_CAPACITY, the last from rtmodt_gmc_estimate_batch itself; after each the next frame gives the restatement's next
    result."""
    F = pkg._ffi
    c, ref = K.case(name), K.reference(name)
    frames = c.streams[0]
    d = c.cfg["downscale"]
    assert (too_large[1] > G.MAX_W) != ((too_large[1] // d // 16) * (too_large[0] // d // 16) > G.MAX_BLOCKS)      # one limit at a time
    est = _est(pkg, **c.cfg)
    assert est.cfg.max_boxes == 1024

    def step(f):
        warp, status = est.estimate([frames[f]])
        _same(est, 0, warp[0], status[0], ref[f][0], (name, f))
    step(0)
    with pytest.raises(F.RtmodtError) as e:
        est.estimate([np.zeros(too_large + (3,), np.uint8)])
    assert e.value.code == F.E_CAPACITY
    step(1)
    assert _raw_estimate(pkg, est, frames[2], 1025) == F.E_CAPACITY
    assert _raw_estimate(pkg, est, frames[2], 1024) == 0                                   # the limit itself: frame 2 with 1024 boxes that meet nothing
    warp, status = est.result()
    _same(est, 0, warp[0], status[0], ref[2][0], (name, 2))
    est.close()


def test_estimate_from_detector_with_more_than_64_boxes_equals_the_same_boxes_from_the_host(pkg, tmp_path):
    """The detector-fed path takes its box stride from max_det: at max_det = 300 the synthetic detector returns 300 boxes a frame, and
    the estimate masked with them on the device equals estimate() fed the fetched boxes, block for block.  (Those noise boxes are
    large: measured, no block is met by a box past the 64th alone, so what this pins beyond 64 boxes is the count and the stride; a
    hit that only a later pass of the lane loop sees is masks-200 and masks-1024.)"""
    path = os.path.join(str(tmp_path), "yolov8n_320_noise.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    det = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=300, batch=1, warmup=False, autotune=False)
    a, b = _est(pkg, downscale=2, mask_conf=0.0), _est(pkg, downscale=2, mask_conf=0.0, max_boxes=300)
    frames = G.pan_sequence(320, 320, 60, [(6, -4), (-10, 8)], margin=48)
    masked = 0
    for f, frame in enumerate(frames):
        det.enqueue([frame])
        a.estimate_from_detector(det, [frame])
        wa, sa = a.result()
        got = det.fetch()
        assert len(got[0]) > 64
        wb, sb = b.estimate([frame], got)
        assert np.array_equal(wa.view(np.int32), wb.view(np.int32)) and sa.tolist() == sb.tolist(), f
        if f:
            da, db = a.debug(0), b.debug(0)
            assert all(np.array_equal(da["blk"][k], db["blk"][k]) for k in da["blk"]) and np.array_equal(da["order"], db["order"])
            masked += int((da["blk"]["reason"] == G.R_MASK).sum())
    assert masked > 0
    a.close(); b.close(); det.close()
