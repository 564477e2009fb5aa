"""bench.py's `roofline.traffic` is measured in separate rocprofv3 PMC passes and kept in profiles/traffic_current.json; the line may only carry it
while it still describes the kernels that ran: the JSON is stamped with a digest of csrc/, a changed kernel source yields null."""
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_digest import CSRC, csrc_digest, load_traffic      # noqa: E402


def test_traffic_is_null_when_the_kernels_changed(tmp_path):
    csrc = tmp_path / "csrc"
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("build", "*.o", ".pytest_cache"))
    d0 = csrc_digest(str(csrc))
    assert d0 == csrc_digest(str(csrc)) and len(d0) == 64
    tj = tmp_path / "traffic.json"
    json.dump({"workload_key": "s-640-8x4", "csrc_sha256": d0, "hbm_bytes_per_step": 123, "source": "pmc"}, open(tj, "w"))
    assert load_traffic(str(tj), "s-640-8x4", d0) == (123, "pmc")
    v, why = load_traffic(str(tj), "s-640-8x2", d0)
    assert v is None and "workload" in why
    with open(csrc / "conv.hip", "a") as f:                      # any change to a kernel source
        f.write("\n// touched\n")
    d1 = csrc_digest(str(csrc))
    assert d1 != d0
    v, why = load_traffic(str(tj), "s-640-8x4", d1)
    assert v is None and why.startswith("stale")
    v, why = load_traffic(str(tmp_path / "missing.json"), "s-640-8x4", d1)
    assert v is None


def test_committed_stamp_is_well_formed():
    tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_current.json")))
    assert "workload_key" in tj and "hbm_bytes_per_step" in tj
    v, why = load_traffic(os.path.join(ROOT, "profiles", "traffic_current.json"), tj["workload_key"], csrc_digest())
    assert (v is None and why.startswith("stale")) or v == tj["hbm_bytes_per_step"]


def test_library_carries_the_digest_of_the_sources_it_was_built_from(pkg):
    """the stamp must describe the LIBRARY that runs, not the working tree -- the Makefile compiles tools/kernel_digest.py's value into
    build_info.o, which is rebuilt whenever any kernel source changes; after `make` the two agree, and bench.py reads the library's."""
    info = dict(kv.split("=", 1) for kv in pkg._ffi.lib().rtmodt_build_info().decode().split())
    assert info["diag"] == "0"
    assert info["csrc_sha256"] == csrc_digest(), "librtmodt_hip.so is stale: run make in csrc/ (or __graft_entry__.build())"


def test_workload_label_follows_the_arguments():
    """bench.py's config.workload named "config 4 shard" whatever --model / --size / --streams were."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "config 4" in b.workload_label("s", 640, 8)
    assert "config 5" in b.workload_label("m", 1280, 1)
    assert "config 2/3" in b.workload_label("s", 640, 1)
    for other in (("s", 640, 16), ("m", 640, 8), ("n", 640, 8), ("s", 1280, 1)):
        assert b.workload_label(*other) == "not a BASELINE configuration"
    assert "120 ms" in b.live_stream_cost(4) and "no batching" in b.live_stream_cost(1)


def test_dump_outputs_have_fixed_shapes_and_float_dtypes(tmp_path):
    """--dump-outputs: what the last timed step returned, padded to max_det / max_tracks rows so that two runs with the same
    arguments compare element for element; float32 / float64 only, integers stored exactly."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)

    class Det:
        def __init__(self, k):
            self.xyxy = np.arange(4 * k, dtype=np.float32).reshape(k, 4)
            self.confidence = np.full(k, 0.5, np.float32)
            self.class_id = np.arange(k, dtype=np.int32)

        def __len__(self):
            return len(self.confidence)

    class Trk:
        def snapshot(self, s):
            k = 2 * s
            return {"ids": np.arange(k, dtype=np.int64) + (1 << 40), "xyxy": np.ones((k, 4), np.float32), "conf": np.ones(k, np.float32),
                    "cls": np.full(k, 3, np.int32), "age": np.full(k, 7, np.int32), "tsu": np.zeros(k, np.int32), "next_id": k + 1}

    out = b.step_outputs([Det(3), Det(0), Det(5)], Trk(), 3, max_det=6, max_tracks=8)
    b.write_outputs(str(tmp_path), out)
    got = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert set(got) == set(out) and all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["det_count"].tolist() == [3, 0, 5] and got["det_xyxy"].shape == (3, 6, 4) and got["det_confidence"].shape == (3, 6)
    assert np.array_equal(got["det_xyxy"][2, :5], Det(5).xyxy) and not got["det_xyxy"][2, 5:].any()
    assert got["trk_count"].tolist() == [0, 2, 4] and got["trk_xyxy"].shape == (3, 8, 4) and got["trk_next_id"].tolist() == [1, 3, 5]
    assert got["trk_id"].dtype == np.float64 and got["trk_id"][2, 3] == (1 << 40) + 3
