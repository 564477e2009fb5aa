"""CPU: the DeepSORT restatement (tests/deepsort_ref.py) against independent forms, the host-only quantiser of the library
against the restatement, the uniqueness of every assignment optimum on the GPU suite's sequences, and the behaviour the tracker
exists for (no identity switch where boxes cross).  PARITY UNPINNED: deep_sort_realtime is not installed; nothing here runs it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deepsort_ref as R  # noqa: E402
import eval_ref  # noqa: E402
from oracle import kalman_oracle as K  # noqa: E402
from oracle.tracker_oracle import TrackerOracle  # noqa: E402


def _run(name, record=None):
    if name in R.EMBEDDED:
        params, dim, frames = R.embedded_inputs(name)
        trk = R.DeepSortRef(record=record, dim=dim, **params)
        outs = []
        for x, xy, cf, cl, _ in frames:
            outs.append(trk.tracks_out(trk.update(xy, cf, cl, R.quantize_rows(x))))
        return trk, outs, frames
    params, frames = R.sequence_inputs(name)
    trk = R.DeepSortRef(record=record, **params)
    outs = []
    for img, xy, cf, cl, _ in frames:
        desc, _ = R.describe(img, xy)
        idx = trk.update(xy, cf, cl, desc)
        outs.append(trk.tracks_out(idx))
    return trk, outs, frames


def test_kalman_and_gating_block_form_equals_textbook_float64():
    """The block-diagonal float32 filter + diagonal gating distance against the 8x8 float64 filter + a Cholesky-solved Mahalanobis
    distance, on a walk with updates and coasting; the bound is the one tests/test_oracle_kalman.py uses for the same filter."""
    rng = np.random.default_rng(0)
    full = K.KalmanFull64()
    z = np.array([200.0, 150.0, 0.5, 80.0])
    m32, c32 = K.kf_initiate(z[None].astype(np.float32))
    m64, c64 = full.initiate(z)
    for step in range(60):
        m32, c32 = K.kf_predict(m32, c32)
        m64, c64 = full.predict(m64, c64)
        z = z + np.array([1.5, -0.7, 0.0, 0.2]) + rng.normal(0, [0.5, 0.5, 0.002, 0.3])
        probe = (z[None] + rng.normal(0, [3, 3, 0.01, 2], (5, 4))).astype(np.float32)
        d2 = R.gating_d2(m32, c32, probe)[0]
        h = m64[3]
        S = full.H @ c64 @ full.H.T + np.diag(np.square([full.wp * h, full.wp * h, 1e-1, full.wp * h]))
        L = np.linalg.cholesky(S)
        y = np.linalg.solve(L, (probe.astype(np.float64) - m64[:4]).T)
        ref = (y * y).sum(0)
        assert np.allclose(d2, ref, rtol=1e-4, atol=1e-4), (step, d2, ref)
        if step % 4 != 3:                                  # every fourth frame coasts
            m32, c32 = K.kf_update(m32, c32, z[None].astype(np.float32))
            m64, c64 = full.update(m64, c64, z)
        blocks = c32.reshape(4, 3)
        for k in range(4):
            assert np.allclose([blocks[k, 0], blocks[k, 1], blocks[k, 2]], [c64[k, k], c64[k, 4 + k], c64[4 + k, 4 + k]], rtol=1e-4, atol=1e-6)
        assert np.allclose(m32[0], m64, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("name", sorted(R.SEQUENCES) + sorted(R.EMBEDDED))
def test_matching_equals_scipy_and_every_optimum_is_unique(name):
    """Every matching problem of every frame: (a) equals scipy.optimize.linear_sum_assignment run the way deep_sort's
    min_cost_matching runs it -- dense matrix, inadmissible entries set to max_distance + 1e-5, matched pairs above max_distance
    rejected; (b) is the UNIQUE optimum: forbidding any matched pair makes the total gain drop.  No frame is left out, of any
    sequence the GPU suite feeds from the host (the two detector-fed GPU tests have no CPU form: deepsort_ref.py says which)."""
    from scipy.optimize import linear_sum_assignment
    record = []
    trk, _, frames = _run(name, record)
    assert len(record) >= len(frames) // 2
    not_unique = 0
    for rec in record:
        gain, cost = rec["gain"], rec["cost"]
        m, n = len(gain), len(gain[0])
        if rec["kind"] == "appearance":
            maxd = trk.max_dist
            dense = np.asarray([[cost[r, c] / float(R.DOT_ONE) if gain[r][c] is not None else maxd + 1e-5 for c in range(n)] for r in range(m)])
        else:
            maxd = trk.max_iou_distance
            dense = np.asarray([[cost[r, c] if gain[r][c] is not None else maxd + 1e-5 for c in range(n)] for r in range(m)])
        rr, cc = linear_sum_assignment(dense)
        ref = sorted((int(r), int(c)) for r, c in zip(rr, cc) if dense[r, c] <= maxd)
        assert ref == rec["pairs"], (name, rec["kind"], ref, rec["pairs"])
        if not R.unique_optimum(gain, rec["pairs"], rec["total"]):
            not_unique += 1
    assert not_unique == 0


def test_pair_limit_frame_has_2048_pairs_equals_scipy_and_its_optimum_is_unique():
    """The IoU-stage frame of the GPU suite that sits exactly at lap.h's 2048 contested pairs (deepsort_ref.pair_limit_frames):
    32 tentative tracks x 64 detections, every pair admissible; the restatement's matching equals scipy's run the way
    min_cost_matching runs it, and forbidding any matched pair makes scipy's best total rise, so the optimum is unique.  With
    the extra track there are 2049 admissible pairs, the extra row's only one in a contested column."""
    from scipy.optimize import linear_sum_assignment
    for extra in (False, True):
        params, frames = R.pair_limit_frames(extra)
        record = []
        trk = R.DeepSortRef(record=record, **params)
        for xy, cf, cl, desc in frames:
            trk.update(xy, cf, cl, desc)
        assert [r["kind"] for r in record] == ["iou"]
        gain, cost, pairs = record[0]["gain"], record[0]["cost"], record[0]["pairs"]
        adm = np.asarray([[g is not None for g in row] for row in gain])
        assert adm.shape == (32 + extra, 64) and int(adm.sum()) == 2048 + extra and adm[:32].all()
        if extra:
            assert adm[32].tolist() == [False] * 63 + [True]
        maxd = trk.max_iou_distance
        dense = np.where(adm, cost, maxd + 1e-5)
        rr, cc = linear_sum_assignment(dense)
        assert sorted((int(r), int(c)) for r, c in zip(rr, cc) if dense[r, c] <= maxd) == pairs and len(pairs) == 32 + extra
        best = dense[rr, cc].sum()
        for r, c in pairs:                                     # gain = limit - cost and every optimum matches all rows: least cost = most gain
            d = dense.copy()
            d[r, c] = 10.0
            r2, c2 = linear_sum_assignment(d)
            assert d[r2, c2].sum() > best + 1e-9, (r, c)


def test_descriptor_equals_per_pixel_loop_and_quantiser_properties():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    boxes = [[3.7, 2.2, 40.9, 30.5], [-5, -5, 100, 100], [10, 10, 11, 11], [20, 5, 10, 30], [7, 7, 7, 20], [0, 0, 53, 37], [50.2, 33.9, 60, 40],
             [4, 4, 9, 7], [float("nan"), 0, 10, 10]]
    desc, counts = R.describe(frame, boxes)
    for b, cnt in zip(boxes, counts):
        brute = np.zeros(192, np.int64)
        if not any(v != v for v in b):
            x0, y0, x1, y1 = (min(max(int(v), 0), lim) for v, lim in zip(b, (53, 37, 53, 37)))
            H = y1 - y0
            for y in range(y0, y1):
                s = next(k for k in range(4) if y0 + (k * H) // 4 <= y < y0 + ((k + 1) * H) // 4) if x1 > x0 else 0
                for x in range(x0, x1):
                    for c in range(3):
                        brute[s * 48 + c * 16 + (int(frame[y, x, c]) >> 4)] += 1
        assert np.array_equal(brute, cnt), b
    assert not counts[3].any() and not counts[4].any() and not counts[8].any() and counts[2].sum() == 3 and counts[5].sum() == 3 * 53 * 37
    assert not R.quantize_counts(np.zeros(192, np.int32)).any()
    one = np.zeros(192, np.int32); one[17] = 123456
    q = R.quantize_counts(one)
    assert q[17] == 127 and q.sum() == 127
    for cnt in counts:
        q = R.quantize_counts(cnt).astype(np.int64)
        assert q.min() >= 0 and q.max() <= 127 and (q > 0).sum() == (cnt > 0).sum() - ((cnt > 0) & (q == 0)).sum()


def test_library_quantize_equals_restatement_without_a_device(pkg):
    """rtmodt_appearance_quantize is host code: it runs where no GPU is, and equals the restatement byte for byte."""
    L = pkg._ffi.lib()
    rng = np.random.default_rng(9)
    for dim in (64, 128, 192, 256, 320, 512):
        x = (rng.normal(0, 1, (23, dim)) * rng.uniform(1e-3, 1e3, (23, 1))).astype(np.float32)
        x[3] = 0
        x[5] = 0; x[5, 7] = -2.5
        x[6, ::2] = 0
        got = pkg._ffi.appearance_quantize(x)
        assert got.dtype == np.int8 and np.array_equal(got, R.quantize_rows(x)), dim
        assert not got[3].any() and got[5, 7] == -127
    out = np.zeros(100, np.int8)
    x = np.zeros(100, np.float32)
    for dim in (0, 32, 100, 576):
        assert L.rtmodt_appearance_quantize(pkg._ffi.ptr(x), 1, dim, pkg._ffi.ptr(out)) == pkg._ffi.E_INVALID
    assert b"64..512" in L.rtmodt_last_error()


def _mot_rows(per_frame):
    rows = []
    for f, items in enumerate(per_frame):
        for oid, b in items:
            rows.append([f + 1, oid, b[0], b[1], b[2] - b[0], b[3] - b[1]])
    return np.asarray(rows, np.float64).reshape(-1, 6)


def test_no_identity_switch_where_boxes_cross_but_iou_only_tracking_has_one():
    """Pairs of differently coloured boxes cross at equal size and speed (the far one hidden while they coincide).  DeepSORT's
    output has 0 identity switches; the IoU-only ByteTrack restatement, fed the same detections, has at least 1 (counted with
    the project's CLEAR MOT restatement, tests/eval_ref.py)."""
    trk, outs, frames = _run("crossing")
    gt = _mot_rows([[(int(o), b) for o, b in zip(ids, xy)] for _, xy, _, _, ids in frames])
    ds = eval_ref.mot_ref(gt, _mot_rows(outs))
    assert ds["num_matches"] > 0.8 * ds["num_objects"], ds
    assert ds["num_switches"] == 0, ds["num_switches"]
    bt = TrackerOracle()
    hyp = []
    for _, xy, cf, cl, _ in frames:
        bt.update(xy, cf, cl)
        s = bt.snapshot()
        hyp.append([(int(s["ids"][i]), s["xyxy"][i]) for i in np.nonzero(s["tsu"] == 1)[0]])
    assert eval_ref.mot_ref(gt, _mot_rows(hyp))["num_switches"] >= 1


def test_reference_behaviour_is_unchanged_and_the_new_class_is_exported(pkg):
    with pytest.raises(NotImplementedError, match="DeepSORT adapter not yet wired. Use bytetrack."):
        pkg.MultiObjectTracker("deepsort")
    assert pkg.DeepSortTracker is pkg.tracking.DeepSortTracker and pkg.DeepSortTracker.needs_frame is True
    with pytest.raises(NotImplementedError, match="embeddings="):
        pkg.DeepSortTracker(embedder="weights/osnet_x0_25.onnx")
    with pytest.raises(NotImplementedError, match="embeddings="):
        pkg.DeepSortTracker.from_config({"algorithm": "deepsort", "deepsort": {"max_dist": 0.2, "embedder": "weights/osnet_x0_25.onnx"}})
    h = C.c_void_p()
    cfg = pkg._ffi.DeepSortCfg(0.2, 0.3, 0.7, 70, 3, 100, b"weights/osnet_x0_25.onnx", 0, 256, 1024, 1, 0)
    assert pkg._ffi.lib().rtmodt_deepsort_create(C.byref(cfg), C.byref(h)) == pkg._ffi.E_UNSUPPORTED and not h.value
    for bad, code in (((0.2, 0.3, 0.7, 70, 3, 129, None, 0, 256, 1024, 1, 0), pkg._ffi.E_CAPACITY), ((0.2, 0.3, 0.7, 70, 3, 100, None, 0, 257, 1024, 1, 0), pkg._ffi.E_CAPACITY),
                      ((0.2, 0.3, 0.7, 70, 3, 100, None, 0, 256, 1025, 1, 0), pkg._ffi.E_CAPACITY), ((0.2, 0.3, 0.7, 70, 3, 100, None, 100, 256, 1024, 1, 0), pkg._ffi.E_INVALID),
                      ((0.2, 0.3, 0.7, 0, 3, 100, None, 0, 256, 1024, 1, 0), pkg._ffi.E_INVALID)):
        assert pkg._ffi.lib().rtmodt_deepsort_create(C.byref(pkg._ffi.DeepSortCfg(*bad)), C.byref(h)) == code and not h.value, bad


def test_every_host_fed_gpu_sequence_is_in_the_tables():
    """The GPU suite takes its host-fed sequences from deepsort_ref.SEQUENCES / EMBEDDED and nowhere else."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_deepsort.py")).read()
    assert "R.random_scene(" not in src and "R.crossing_scene(" not in src and "R.embedded_scene(" not in src and "default_rng" not in src.split("# sequences")[1]
    assert "R.sequence_inputs(" in src and "R.embedded_inputs(" in src


def test_pipeline_keeps_a_frame_hungry_tracker_off_the_device_event_path(pkg):
    """pipeline.run with a tracker that sets needs_frame: the frame is passed, the tracks are materialised, and the event engine gets
    them through process() -- never through process_tracker(), which reads a ByteTrack handle; the ByteTrack loop is unchanged."""
    class Det:
        model = type("M", (), {"names": {}})()

        def detect(self, frame):
            return "dets"

    class Trk:
        def __init__(self, needs_frame):
            self.calls = []
            if needs_frame:
                self.needs_frame = True
                self.update_from_detector = lambda det, frame=None, materialize=True: self.calls.append(("dev", frame is not None, materialize)) or ["t"]
                self.update = lambda dets, frame=None: self.calls.append(("host", frame is not None)) or ["t"]
            else:
                self.update_from_detector = lambda det, materialize=True: self.calls.append(("dev", materialize)) or []
                self.update = lambda dets: self.calls.append(("host",)) or []

    class Eng:
        def __init__(self):
            self.calls = []

        def process(self, tracks, fid):
            self.calls.append(("process", list(tracks)))
            return []

        def process_tracker(self, tracker, fid, class_names=None):
            self.calls.append(("process_tracker",))
            return [[]]

    src = pkg.pipeline.SyntheticSource(np.zeros((1, 8, 8, 3), np.uint8))
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    for handoff in (True, False):
        trk, eng = Trk(True), Eng()
        pkg.pipeline.run(src, Det(), trk, prof(), max_frames=2, device_stages=False, event_engine=eng, device_handoff=handoff)
        assert trk.calls == ([("dev", True, True)] if handoff else [("host", True)]) * 2
        assert eng.calls == [("process", ["t"])] * 2
    trk, eng = Trk(False), Eng()
    pkg.pipeline.run(src, Det(), trk, prof(), max_frames=2, device_stages=False, event_engine=eng)
    assert trk.calls == [("dev", False)] * 2 and eng.calls == [("process_tracker",)] * 2
    with pytest.raises(ValueError, match="packed pixels"):                     # a BGRA view would change its pitch under a silent copy
        pkg._ffi.frame_pointers([np.zeros((4, 4, 4), np.uint8)[:, :, :3]], pkg._ffi.MEM_HOST)
    with pytest.raises(ValueError, match="packed pixels"):
        pkg._ffi.frame_pointers([np.zeros((4, 4, 3), np.float32)], pkg._ffi.MEM_HOST)
    padded = np.lib.stride_tricks.as_strided(np.zeros((4, 20), np.uint8), (4, 5, 3), (20, 3, 1))
    assert pkg._ffi.frame_pointers([padded], pkg._ffi.MEM_HOST)[2:] == (4, 5, 20)
