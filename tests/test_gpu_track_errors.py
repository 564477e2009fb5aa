"""GPU: the error surface the three trackers share (csrc/track_host.h): a stream whose meta row carries a sticky error answers
E_CAPACITY from the update that raised it and from every later read of the state, with the text each tracker has always used --
ByteTrack alone names its solver ("lapjv assignment too dense").  The expected strings are written out here, not read from
the library."""
import numpy as np
import pytest

import deepsort_ref
import ocsort_ref
from oracle import tracker_oracle as T

pytestmark = pytest.mark.gpu

TOO_MANY = "stream 0: more than max_tracks=4 live tracks"
DENSE = "too dense (more than 256 contested rows/columns or 2048 contested pairs)"
TOO_DENSE = {"bytetrack": "stream 0: lapjv assignment " + DENSE, "deepsort": "stream 0: assignment " + DENSE, "ocsort": "stream 0: assignment " + DENSE}


def make(pkg, name, **kw):
    t = pkg.tracking
    if name == "bytetrack":
        return t.tracker._ByteTrackCore(**kw)
    return t.deepsort._DeepSortCore(**{"nn_budget": 4, **kw}) if name == "deepsort" else t.ocsort._OcSortCore(**kw)


def feed(core, name, xy, cf, cl, desc=None):
    if name == "deepsort":
        return core.update(xy, cf, cl, embeddings=np.zeros((len(xy), core.dim), np.int8) if desc is None else desc)
    return core.update(xy, cf, cl)


def overflow(pkg, name):
    """six separate confident boxes into a 4-track x 8-detection handle: six births"""
    core = make(pkg, name, max_tracks=4, max_dets=8)
    xy = np.asarray([[8 + 64 * k, 8, 48 + 64 * k, 68] for k in range(6)], np.float32)
    return core, lambda: feed(core, name, xy, np.full(6, 0.9, np.float32), np.zeros(6, np.int32))


def dense(pkg, name):
    """the 2049-pair frames of the restatements' limit scenes (test_gpu_ocsort.py / test_gpu_deepsort.py use them at the same
    capacities); ByteTrack takes OC-SORT's with match_thresh = 0.3, OC-SORT's IoU threshold, and its lapjv branch"""
    if name == "deepsort":
        params, frames = deepsort_ref.pair_limit_frames(True)
    else:
        frames = ocsort_ref.pair_limit_frames(True)
        params = dict(match_thresh=0.3, assign_mode=pkg._ffi.ASSIGN_LAPJV) if name == "bytetrack" else ocsort_ref.SEQUENCES["limit"][0]
        iou = T.batch_iou(frames[0][0], frames[1][0])
        assert int(((np.float32(1) - iou).astype(np.float64) < 1.0 - float(np.float32(0.3))).sum()) == 2049
    core = make(pkg, name, max_tracks=128, max_dets=64, **params)
    feed(core, name, *frames[0])
    assert len(core.snapshot(0)["ids"]) == 33
    return core, lambda: feed(core, name, *frames[1])


@pytest.mark.parametrize("name", ["bytetrack", "deepsort", "ocsort"])
@pytest.mark.parametrize("scene,want", [(overflow, {k: TOO_MANY for k in TOO_DENSE}), (dense, TOO_DENSE)], ids=["too_many_tracks", "too_dense"])
def test_sticky_error_code_and_text(pkg, name, scene, want):
    ffi = pkg._ffi
    core, step = scene(pkg, name)
    try:
        with pytest.raises(ffi.RtmodtError) as e:
            step()
        assert (e.value.code, e.value.msg) == (ffi.E_CAPACITY, want[name])
        with pytest.raises(ffi.RtmodtError) as e:              # sticky: the state read says the same
            core.snapshot(0)
        assert (e.value.code, e.value.msg) == (ffi.E_CAPACITY, want[name])
        assert ("lapjv" in e.value.msg) == (name == "bytetrack" and scene is dense)
        core.reset()
        assert len(core.snapshot(0)["ids"]) == 0                # the handle answers again
    finally:
        core.close()
