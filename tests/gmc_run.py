"""The bit-for-bit comparison of the camera-motion estimator (csrc/gmc.hip) with its restatement (tests/gmc_ref.py), shared by
``tests/test_gpu_gmc.py`` and ``tests/test_gpu_gmc_limits.py``: after a frame every intermediate rtmodt_gmc_debug returns, the warp's
bits and the status are the restatement's."""
import numpy as np

import gmc_ref as G

F32 = np.float32


def _est(pkg, **kw):
    from importlib import import_module
    return import_module(pkg.__name__ + ".tracking.gmc").CameraMotionEstimator(**kw)


def _bits(a):
    return np.ascontiguousarray(a, F32).reshape(-1).view(np.int32).tolist()


def _same(est, s, warp, status, ref_out, tag):
    rw, rs, dbg = ref_out
    assert int(status) == rs and _bits(warp) == _bits(rw), (tag, int(status), rs, warp, rw)
    got = est.debug(s)
    assert np.array_equal(got["l0"], dbg["l0"]) and np.array_equal(got["l1"], dbg["l1"]), tag
    if rs == G.FIRST:
        return
    assert np.array_equal(got["table"], dbg["table"]) and got["coarse"] == tuple(dbg["coarse"]), (tag, got["coarse"], dbg["coarse"])
    for k in ("reason", "dx", "dy", "offx", "offy", "sad"):
        assert np.array_equal(got["blk"][k], dbg["blk"][k]), (tag, k)
    assert np.array_equal(got["order"], dbg["order"]), tag
    assert np.array_equal(got["scores"], dbg["scores"]) and got["best_k"] == dbg["best_k"], (tag, got["best_k"], dbg["best_k"])
    assert np.array_equal(got["inl"], dbg["inl"]) and np.array_equal(got["sums"], dbg["sums"]), tag
    assert np.array_equal(got["model"].view(np.int64), dbg["model"].view(np.int64)), (tag, got["model"], dbg["model"])


def _run(pkg, streams, n_frames=6, masks=None, reset_at=None, **cfg):
    """streams: one list of frames per stream.  Returns the statuses seen."""
    S = len(streams)
    est = _est(pkg, n_streams=S, **cfg)
    refs = [G.GmcRef(**cfg) for _ in range(S)]
    seen = []
    for f in range(n_frames):
        if reset_at and f == reset_at[1]:
            est.reset(reset_at[0])
            refs[reset_at[0]].reset()
        fr = [streams[s][f] for s in range(S)]
        dets = None if masks is None else [masks[s] for s in range(S)]
        warp, status = est.estimate(fr, dets)
        for s in range(S):
            m = None if masks is None or masks[s] is None else masks[s]
            _same(est, s, warp[s], status[s], refs[s].estimate(fr[s], None if m is None else m.xyxy, None if m is None else m.confidence), (f, s))
        seen.append(status.tolist())
    est.close()
    return seen
