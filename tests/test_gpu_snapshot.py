"""GPU: the snapshot gallery (csrc/snapshot.hip) against the NumPy restatement of its rules (tests/snapshot_ref.py), through the C
ABI: every thumbnail byte of the whole atlas, every ``updated`` / ``retired`` entry, the whole ledger and the slot bitmap are
compared with == after every call -- no case is exempted.  Small frames with a padded pitch and an odd base address in host and
device memory, every box case, a crop wider than one tile, 300 tracks in one stream, three streams in one call, a churn sequence
with a retirement whose slot is reused one call later, capacity of the rows and of both output lists, refusals, the device-state
forms of the four trackers (ids exchanged by the swap guard included), stateless crops, the review queue read from the detector's
device-resident outputs, the JPEG encoder on atlas slots in place, and the pipeline's snapshots stage on a list and on the tracker's state."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as J  # noqa: E402
import snapshot_ref as R  # noqa: E402
from test_gpu_privacy import FH, FW, S, _trackers, detector, run_scripted, scripted  # noqa: E402,F401

pytestmark = pytest.mark.gpu


class Frame:
    """An h x w BGR frame inside a buffer with a padded pitch, `lead` bytes into it (1: an odd base address), on the host or the device."""

    def __init__(self, pkg, h, w, stride, seed, device, lead=1):
        self.h, self.w, self.stride, self.lead = h, w, stride, lead
        self.buf = np.random.default_rng(seed).integers(0, 256, lead + h * stride, dtype=np.uint8)
        self.view = np.lib.stride_tricks.as_strided(self.buf[lead:], (h, w, 3), (stride, 3, 1), writeable=False)
        self.keep = self.buf.copy()
        self.dev = None
        if device:
            self.dev = pkg._ffi.DeviceBuffer(len(self.buf))
            self.dev.upload(self.buf)
        self.mem = pkg._ffi.MEM_DEVICE if device else pkg._ffi.MEM_HOST
        self.ptr = (self.dev.ptr if device else self.buf.ctypes.data) + lead

    def unchanged(self):
        now = self.dev.download() if self.dev is not None else self.buf
        return np.array_equal(now, self.keep)

    def free(self):
        if self.dev is not None:
            self.dev.free()


class Dev:
    """The C ABI of one gallery, and the restatement beside it."""

    def __init__(self, pkg, cfg: R.Cfg, n_streams, max_tracks):
        self.F, self.L = pkg._ffi, pkg._ffi.lib()
        F = self.F
        c = F.SnapshotCfg()
        self.L.rtmodt_snapshot_default_cfg(C.byref(c))
        for k in ("thumb_h", "thumb_w", "margin_pm", "min_side", "area_cap", "occl_iou_pm", "min_gain_pm", "retire_after", "max_updated", "max_retired"):
            setattr(c, k, getattr(cfg, k))
        for k in range(3):
            c.pad_bgr[k] = cfg.pad_bgr[k]
        self._classes = None if cfg.classes is None else np.ascontiguousarray(cfg.classes, np.int32)
        if self._classes is not None:
            c.n_classes, c.classes = len(self._classes), self._classes.ctypes.data_as(C.POINTER(C.c_int32))
        self.cfg, self.c, self.S, self.M, self.cap = cfg, c, n_streams, max_tracks, 2 * max_tracks
        h = C.c_void_p()
        F.check(self.L.rtmodt_snapshot_create(C.byref(c), n_streams, max_tracks, C.byref(h)))
        self.h = h
        self.ref = [R.Stream(cfg, max_tracks) for _ in range(n_streams)]
        self.upd = (F.SnapshotUpdate * (n_streams * cfg.max_updated))()
        self.ret = (F.SnapshotRetired * (n_streams * cfg.max_retired))()
        self.cnt = np.zeros((3, n_streams), np.int32)
        self.out = F.SnapshotOut(C.addressof(self.upd), self.cnt[0].ctypes.data, C.addressof(self.ret), self.cnt[1].ctypes.data, self.cnt[2].ctypes.data)

    def close(self):
        self.L.rtmodt_snapshot_destroy(self.h)

    # ---- what came back, as the restatement's tuples ----
    def results(self, d):
        u = [(x.track_id, x.score, x.slot, x.flags, x.track) for x in self.upd[d * self.cfg.max_updated:d * self.cfg.max_updated + int(self.cnt[0, d])]]
        r = [(x.track_id, x.slot, x.best_frame, tuple(np.float32(list(x.xyxy)).view(np.uint32)), np.float32(x.conf).view(np.uint32), x.cls, x.first_seen,
              x.last_seen, x.n_rewrites) for x in self.ret[d * self.cfg.max_retired:d * self.cfg.max_retired + int(self.cnt[1, d])]]
        return u, r, int(self.cnt[2, d])

    def expect(self, s, ids, xy, conf, cls, frame, fid, selected=None):
        code, u, r, nrw = self.ref[s].process(ids, xy, conf, cls, frame, fid, selected)
        r = [(x.track_id, x.slot, x.best_frame, tuple(np.float32(x.xyxy).view(np.uint32)), np.float32(x.conf).view(np.uint32), x.cls, x.first_seen, x.last_seen,
              x.n_rewrites) for x in r]
        return code, u[:self.cfg.max_updated], r[:self.cfg.max_retired], nrw

    def process(self, s, ids, xy, conf, cls, fr: Frame, fid, want_out=True):
        """One stream through rtmodt_snapshot_process and through the restatement; asserts the results, then the whole state."""
        ids, xy, cls = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(xy, np.float32).reshape(-1, 4), np.ascontiguousarray(cls, np.int32)
        cf = None if conf is None else np.ascontiguousarray(conf, np.float32)
        rc = self.L.rtmodt_snapshot_process(self.h, s, self.F.ptr(ids), self.F.ptr(xy), self.F.ptr(cf), self.F.ptr(cls), len(ids), C.c_void_p(fr.ptr), fr.h, fr.w,
                                            fr.stride, fr.mem, fid, C.byref(self.out) if want_out else None)
        code, u, r, nrw = self.expect(s, ids, xy, cf, cls, fr.view, fid)
        if want_out:
            assert rc == code, (rc, code, self.L.rtmodt_last_error())
            if code != R.E_INVALID:
                assert self.results(0) == (u, r, nrw)
        else:
            assert rc == (code if code == R.E_INVALID else 0)
        self.same(s)
        assert fr.unchanged()
        return code, u, r

    def state(self, s):
        cap = self.cap
        ids, sc, bf, fs, ls = (np.zeros(cap, np.int64) for _ in range(5))
        xy, cf, ints, bm, n = np.zeros((cap, 4), np.float32), np.zeros(cap, np.float32), np.zeros((cap, 4), np.int32), np.zeros((cap + 31) // 32, np.uint32), C.c_int32(-1)
        P = self.F.ptr
        rc = self.L.rtmodt_snapshot_state(self.h, s, P(ids), P(sc), P(bf), P(fs), P(ls), P(xy), P(cf), P(ints), P(bm), C.byref(n))
        k = max(n.value, 0)
        rows = [(int(ids[i]), int(ints[i, 0]), int(sc[i]), int(bf[i]), tuple(xy[i].view(np.uint32)), cf[i].view(np.uint32), int(ints[i, 1]), int(fs[i]), int(ls[i]),
                 int(ints[i, 2]), int(ints[i, 3])) for i in range(k)]
        return rc, rows, bm

    def atlas(self, s):
        slots = np.arange(self.cap, dtype=np.int32)
        out = np.empty((self.cap, self.cfg.thumb_h, self.cfg.thumb_w, 3), np.uint8)
        self.F.check(self.L.rtmodt_snapshot_read(self.h, s, self.F.ptr(slots), self.cap, self.F.ptr(out)))
        return out

    def same(self, s):
        """The whole atlas, the ledger and the bitmap of stream s equal the restatement's."""
        ref = self.ref[s]
        got, want = self.atlas(s), ref.atlas
        bad = np.nonzero((got != want).reshape(self.cap, -1).any(1))[0]
        assert len(bad) == 0, f"stream {s}: thumbnails of slots {bad[:8].tolist()} differ"
        rc, rows, bm = self.state(s)                                    # (a stream in error still hands its rows out, with the error code)
        assert rc == (R.E_CAPACITY if ref.err else 0), self.L.rtmodt_last_error()
        want_rows = [(r.track_id, r.slot, r.best_score, r.best_frame, tuple(np.float32(r.xyxy).view(np.uint32)), np.float32(r.conf).view(np.uint32), r.cls,
                      r.first_seen, r.last_seen, r.n_rewrites, r.flags) for r in ref.ledger()]
        assert rows == want_rows
        assert np.array_equal(bm, ref.bitmap())


BOXES = np.float32([
    [0, 0, 96, 60],                      # the full frame
    [30, 20, 30, 20],                    # 1 x 1
    [-10, 5, 9.5, 14],                   # partly outside
    [80, 40, 120, 90],                   # partly outside, the far corner
    [-40, -40, -30, -30],                # fully outside
    [np.nan, 5, 20, 20],                 # NaN
    [5, 5, np.inf, 20],                  # inf
    [40, 30, 47, 35],                    # smaller than the thumbnail
    [10, 10, 73, 41],                    # 64 x 32: exactly 2 : 1
    [3, 7, 59, 50],                      # 57 x 44: no integer ratio
    [50, 2, 52, 58],                     # a tall sliver
    [20, 50, 10, 55],                    # inverted
])


@pytest.mark.parametrize("thumb", [(16, 16), (24, 40)], ids=["16x16", "40x24"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_small_frame_every_box_case(pkg, device, thumb):
    cfg = R.Cfg(thumb_h=thumb[0], thumb_w=thumb[1], margin_pm=100, min_side=1, occl_iou_pm=300, min_gain_pm=50, retire_after=5, classes=(0, 1, 2))
    d = Dev(pkg, cfg, 1, 16)
    fr = Frame(pkg, 61, 97, 3 * 97 + 7, 1, device)                      # padded pitch 298 (not a multiple of 4), odd base
    n = len(BOXES)
    ids = np.arange(100, 100 + n)[::-1].copy()                          # the list is not in id order
    cls = (np.arange(n) % 4).astype(np.int32)                           # class 3 is filtered
    conf = np.linspace(0.3, 0.9, n).astype(np.float32)
    code, u, r = d.process(0, ids, BOXES, conf, cls, fr, 10)
    assert code == 0 and len(u) >= 6 and all(x[3] & R.F_NEW for x in u)
    assert [x[2] for x in u] == list(range(len(u)))                     # free slots in ascending order, in list order
    d.process(0, ids, BOXES, conf, cls, fr, 11)                         # the same again: nothing is rewritten
    conf2 = conf.copy()
    conf2[::2] = 0.95
    conf2[1::2] = 0.1
    code, u, r = d.process(0, ids, BOXES + np.float32([1, 0, 1, 0]), conf2, cls, fr, 12)       # shifted by a pixel; some better, some worse
    assert any(x[3] & R.F_REWRITTEN for x in u) and len(u) < n
    d.process(0, ids[:3], BOXES[:3], None, cls[:3], fr, 13, want_out=False)                    # no confidences, no outputs
    fr2 = Frame(pkg, 61, 97, 3 * 97 + 1, 2, device, lead=0)             # aligned base, pitch 292: the dword path
    d.process(0, ids, BOXES, conf2, cls, fr2, 20)                       # every row retires and is born again
    d.close(); fr.free(); fr2.free()


@pytest.mark.parametrize("lead,stride", [(0, 1536 * 3), (1, 1536 * 3 + 2), (0, 1536 * 3 + 4)], ids=["dwords", "bytes", "dwords-padded"])
def test_wide_crop_past_one_tile(pkg, lead, stride):
    cfg = R.Cfg(thumb_h=16, thumb_w=16, margin_pm=0, min_side=1, occl_iou_pm=0)
    d = Dev(pkg, cfg, 1, 8)
    fr = Frame(pkg, 40, 1536, stride, 3, True, lead)
    boxes = np.float32([[18, 0, 1517, 39], [0, 3, 1535, 33], [1365, 0, 1535, 39], [1, 1, 1366, 2]])      # 1500 wide; the whole width; across the tile seam
    code, u, r = d.process(0, [1, 2, 3, 4], boxes, [0.5] * 4, [0] * 4, fr, 0)
    assert len(u) == 4
    d.close(); fr.free()
    cfg = R.Cfg(thumb_h=8, thumb_w=512, margin_pm=0, min_side=1, occl_iou_pm=0)                          # every thread owns six bytes of the row
    d = Dev(pkg, cfg, 1, 2)
    fr = Frame(pkg, 40, 1536, stride, 4, False, lead)
    d.process(0, [1, 2], boxes[:2], None, [0, 0], fr, 0)
    d.close(); fr.free()


def test_many_tracks_new_kept_rewritten(pkg):
    cfg = R.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=2, occl_iou_pm=400, min_gain_pm=0, retire_after=100)
    d = Dev(pkg, cfg, 1, 320)
    fr = Frame(pkg, 128, 160, 3 * 160, 5, True, 0)
    rng = np.random.default_rng(6)
    n = 300
    x0, y0 = rng.integers(0, 150, n), rng.integers(0, 118, n)
    boxes = np.stack([x0, y0, x0 + rng.integers(2, 12, n), y0 + rng.integers(2, 12, n)], 1).astype(np.float32)
    ids = rng.permutation(1000)[:n].astype(np.int64)
    conf = rng.uniform(0.2, 0.6, n).astype(np.float32)
    cls = np.zeros(n, np.int32)
    code, u, r = d.process(0, ids[:200], boxes[:200], conf[:200], cls[:200], fr, 0)
    assert len(u) == 200
    conf2 = conf.copy()
    conf2[0:200:2] += 0.3                                               # every second old track gets a better shot, the others are kept
    code, u, r = d.process(0, ids, boxes, conf2, cls, fr, 1)            # 100 births among them
    kinds = [x[3] & 3 for x in u]
    assert kinds.count(R.F_NEW) == 100 and kinds.count(R.F_REWRITTEN) >= 50 and len(u) < 300
    order = rng.permutation(n)
    conf3 = conf2.copy()
    conf3[1:200:2] += 0.35
    code, u, r = d.process(0, ids[order], boxes[order], conf3[order], cls[order], fr, 2)
    assert 0 < len(u) < 150 and all(x[3] & R.F_REWRITTEN for x in u)
    d.close(); fr.free()


def test_three_streams_in_one_call(pkg):
    cfg = R.Cfg(thumb_h=16, thumb_w=16, margin_pm=50, min_side=2, retire_after=0)
    d = Dev(pkg, cfg, 3, 8)
    F, L = d.F, d.L
    frames = [Frame(pkg, 61, 97, 3 * 97 + 7, 10 + s, True, 0) for s in range(3)]
    one = pkg._ffi.DeviceBuffer(3 * len(frames[0].buf))
    for s in range(3):
        one.upload(frames[s].buf, s * len(frames[s].buf))
    stride_t = 8
    for call in range(3):
        ids, xy = np.zeros((3, stride_t), np.int64), np.zeros((3, stride_t, 4), np.float32)
        conf, cls, n = np.zeros((3, stride_t), np.float32), np.zeros((3, stride_t), np.int32), np.int32([5, 0, 3])
        fid = np.int64([call, 7 * call + 1, 100 + 3 * call])
        for s in range(3):
            for i in range(n[s]):
                ids[s, i] = 10 * s + (i + call) % 6
                xy[s, i] = [5 + 9 * i + call, 4 + 3 * s, 30 + 11 * i - call, 40 + 2 * i]
                conf[s, i] = 0.3 + 0.1 * ((i + 2 * call) % 5)
                cls[s, i] = i
        fp = (C.c_void_p * 3)(*[one.ptr + s * len(frames[s].buf) for s in range(3)])
        rc = L.rtmodt_snapshot_process_batch(d.h, F.ptr(ids), F.ptr(xy), F.ptr(conf), F.ptr(cls), F.ptr(n), stride_t, fp, 61, 97, frames[0].stride, F.MEM_DEVICE,
                                             F.ptr(fid), C.byref(d.out))
        assert rc == 0, L.rtmodt_last_error()
        for s in range(3):
            code, u, r, nrw = d.expect(s, ids[s, :n[s]], xy[s, :n[s]], conf[s, :n[s]], cls[s, :n[s]], frames[s].view, int(fid[s]))
            assert code == 0 and d.results(s) == (u, r, nrw), (call, s)
            d.same(s)
    assert any(len(d.ref[s].rows) for s in range(3))
    for s in range(3):
        assert np.array_equal(one.download(len(frames[s].buf), s * len(frames[s].buf)), frames[s].keep)
        frames[s].free()
    one.free(); d.close()


def test_churn_births_occlusion_retirement_and_slot_reuse(pkg):
    cfg = R.Cfg(thumb_h=16, thumb_w=16, margin_pm=100, min_side=4, occl_iou_pm=250, min_gain_pm=100, retire_after=2)
    d = Dev(pkg, cfg, 1, 6)
    fr = [Frame(pkg, 61, 97, 3 * 97 + 3, 20 + k, k % 2 == 1) for k in range(3)]
    reused = retired = occluded = 0
    gone_slots = {}
    for f in range(12):
        tr = []
        tr.append((1, [5 + 2 * f, 10, 25 + 2 * f, 40], 0.5 + 0.03 * f))                        # walks right, keeps improving
        tr.append((2, [60 - 3 * f, 12, 80 - 3 * f, 44], 0.8 - 0.02 * f))                       # walks left into track 1: an occlusion pair
        if f < 4:
            tr.append((3, [40, 30, 60, 55], 0.6))                                              # leaves after frame 3: retires at frame 6
        if f >= 5:
            born = [70, 5 + f, 90, 30 + f] if f % 2 else [7 + 2 * f, 12, 27 + 2 * f, 42]       # a birth in every call from frame 5 on, each seen
            tr.append((4 + f, born, 0.4))                                                      # once; every second one on top of track 1
        ids, xy, cf = [t[0] for t in tr], [t[1] for t in tr], [t[2] for t in tr]
        code, u, r = d.process(0, ids, xy, cf, [0] * len(tr), fr[f % 3], f)
        assert code == 0
        for x in u:
            if x[3] & R.F_NEW and x[2] in gone_slots:
                assert f > gone_slots.pop(x[2]), "a slot was reused in the call that freed it"
                reused += 1
            occluded += bool(x[3] & R.F_OCCLUDED)
        for x in r:
            gone_slots[x[1]] = f
            retired += 1
    assert retired >= 3 and reused >= 1 and occluded >= 1
    d.close()
    for k in fr:
        k.free()


def test_capacity_of_rows_and_of_both_lists(pkg):
    box = lambda i: [4 + 6 * (i % 12), 4 + 8 * (i // 12), 12 + 6 * (i % 12), 14 + 8 * (i // 12)]
    fr = Frame(pkg, 61, 97, 3 * 97, 30, False, 0)
    cfg = R.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=2, occl_iou_pm=0, retire_after=1000)
    d = Dev(pkg, cfg, 2, 4)                                             # 8 rows
    for call in range(2):
        ids = [4 * call + i for i in range(4)]
        assert d.process(0, ids, [box(i) for i in ids], None, [0] * 4, fr, call)[0] == 0
    ids = [8, 9, 10]
    code, u, r = d.process(0, ids, [box(i) for i in ids], None, [0] * 3, fr, 2)              # 3 + 8 idle rows > 8
    assert code == R.E_CAPACITY and b"ledger full" in d.L.rtmodt_last_error() and [x[2] for x in u] == [0, 1, 2]
    assert d.process(0, ids, [box(i) for i in ids], None, [0] * 3, fr, 3)[0] == R.E_CAPACITY  # the stream stays in error ...
    assert d.process(1, ids, [box(i) for i in ids], None, [0] * 3, fr, 0)[0] == 0             # ... its neighbour does not ...
    d.F.check(d.L.rtmodt_snapshot_reset(d.h, 0))                                               # ... until it is reset
    d.ref[0] = R.Stream(cfg, 4)
    d.ref[0].atlas[:] = d.atlas(0)                                                             # (the atlas bytes stay as they are)
    assert d.process(0, ids, [box(i) for i in ids], None, [0] * 3, fr, 0)[0] == 0
    d.close()
    # a slot shortage: six rows retire in the call that brings three births, and their slots are free from the next call only
    cfg = R.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=2, occl_iou_pm=0, retire_after=1)
    d = Dev(pkg, cfg, 1, 4)
    assert d.process(0, [0, 1, 2, 3], [box(i) for i in range(4)], None, [0] * 4, fr, 0)[0] == 0
    assert d.process(0, [4, 5, 0, 1], [box(i) for i in (4, 5, 0, 1)], None, [0] * 4, fr, 1)[0] == 0
    code, u, r = d.process(0, [6, 7, 8], [box(i) for i in (6, 7, 8)], None, [0] * 3, fr, 5)
    assert code == R.E_CAPACITY and len(r) == 6 and len(u) == 3
    d.close()
    cfg = R.Cfg(thumb_h=8, thumb_w=8, margin_pm=0, min_side=2, occl_iou_pm=0, retire_after=0, max_updated=2, max_retired=1)
    d = Dev(pkg, cfg, 1, 8)
    ids = [0, 1, 2, 3, 4]
    code, u, r = d.process(0, ids, [box(i) for i in ids], None, [0] * 5, fr, 0)              # 5 thumbnails, room for 2 entries: all are written
    assert code == R.E_CAPACITY and len(u) == 2 and b"max_updated" in d.L.rtmodt_last_error()
    code, u, r = d.process(0, [7], [box(7)], None, [0], fr, 5)                                # 5 rows retire, room for 1 entry
    assert code == R.E_CAPACITY and len(r) == 1 and b"max_retired" in d.L.rtmodt_last_error()
    assert d.process(0, [7], [box(7)], None, [0], fr, 6)[0] == 0                              # the stream goes on
    d.close(); fr.free()


def test_refusals_leave_the_state_alone(pkg):
    cfg = R.Cfg(thumb_h=16, thumb_w=16, min_side=2)
    d = Dev(pkg, cfg, 1, 4)
    F, L = d.F, d.L
    fr = Frame(pkg, 61, 97, 3 * 97 + 7, 40, True)
    d.process(0, [5, 6], [[5, 5, 40, 40], [30, 10, 90, 50]], [0.5, 0.6], [0, 0], fr, 10)
    for fid in (10, 9, -1):
        assert d.process(0, [5, 9], [[5, 5, 50, 50], [1, 1, 30, 30]], [0.9, 0.9], [0, 0], fr, fid)[0] == R.E_INVALID      # (same() inside: nothing changed)
    ids, xy, cls = np.int64([5, 5]), np.float32([[5, 5, 40, 40]] * 2), np.int32([0, 0])
    call = lambda ids, xy, cls, n, ptr, h, w, st, mem, fid: L.rtmodt_snapshot_process(d.h, 0, F.ptr(ids), F.ptr(xy), None, F.ptr(cls), n, C.c_void_p(ptr), h, w, st,
                                                                                     mem, fid, C.byref(d.out))
    assert call(ids, xy, cls, 2, fr.ptr, 61, 97, fr.stride, fr.mem, 11) == F.E_INVALID and b"twice" in L.rtmodt_last_error()
    assert call(ids, xy, cls, 1, None, 61, 97, fr.stride, fr.mem, 11) == F.E_INVALID
    assert call(ids, xy, cls, 1, fr.ptr, 61, 97, 3 * 97 - 1, fr.mem, 11) == F.E_INVALID
    assert call(ids, xy, cls, 1, fr.ptr, 61, 97, fr.stride, 7, 11) == F.E_INVALID
    assert call(ids, xy, cls, 1, fr.ptr, 0, 97, fr.stride, fr.mem, 11) == F.E_INVALID
    big = np.arange(5, dtype=np.int64)
    assert call(big, np.zeros((5, 4), np.float32), np.zeros(5, np.int32), 5, fr.ptr, 61, 97, fr.stride, fr.mem, 11) == F.E_CAPACITY
    assert L.rtmodt_snapshot_process(d.h, 1, F.ptr(ids), F.ptr(xy), None, F.ptr(cls), 1, C.c_void_p(fr.ptr), 61, 97, fr.stride, fr.mem, 11, None) == F.E_INVALID
    d.same(0)
    assert d.process(0, [5], [[5, 5, 50, 50]], [0.9], [0], fr, 11)[0] == 0                     # and the stream goes on from where it was
    d.close(); fr.free()


@pytest.mark.parametrize("which", ["bytetrack", "deepsort", "ocsort", "botsort"])
def test_tracker_forms_equal_the_list_form_on_the_passed_tracks(pkg, which):
    make, with_frames, passed = _trackers(pkg)[which]
    core = make()
    frames = run_scripted(core, with_frames)
    cfg = R.Cfg(thumb_h=16, thumb_w=16, margin_pm=100, min_side=4, occl_iou_pm=300, retire_after=0, classes=(0, 1))
    d = Dev(pkg, cfg, S, 32)
    F, L = d.F, d.L
    fp = (C.c_void_p * S)(*[f.ctypes.data for f in frames])
    n_pass = 0
    for call in range(2):
        if call == 1:                                                   # one more update: the frame-2-only track is lost, boxes move on
            xyxy = np.zeros((S, 16, 4), np.float32); conf = np.zeros((S, 16), np.float32); cls = np.zeros((S, 16), np.int32); cnt = np.zeros(S, np.int32)
            for s in range(S):
                xy, cf, cl = scripted(3, s)
                xyxy[s, :len(cf)], conf[s, :len(cf)], cls[s, :len(cf)], cnt[s] = xy, cf * np.float32(0.9 + 0.02 * s), cl, len(cf)
            core.update_batch(xyxy, conf, cls, cnt, **({"frames": frames} if with_frames else {}))
        fid = np.int64([call, 10 + call])
        args = (d.h, core._h, fp, FH, FW, 3 * FW, F.MEM_HOST, F.ptr(fid))
        if which == "bytetrack":
            rc = L.rtmodt_snapshot_process_tracker(*args, 1, C.byref(d.out))
        elif which == "deepsort":
            rc = L.rtmodt_snapshot_process_deepsort(*args, 0, C.byref(d.out))
        elif which == "ocsort":
            rc = L.rtmodt_snapshot_process_ocsort(*args, C.byref(d.out))
        else:
            rc = L.rtmodt_snapshot_process_botsort(*args, C.byref(d.out))
        assert rc == 0, L.rtmodt_last_error()
        for s in range(S):
            st = core.snapshot(s)
            sel = np.zeros(len(st["ids"]), bool)
            sel[passed(core, st)] = True
            n_pass += int(sel.sum())
            code, u, r, nrw = d.expect(s, st["ids"], st["xyxy"], st["conf"], st["cls"], frames[s], int(fid[s]), sel)
            assert code == 0 and d.results(s) == (u, r, nrw), (call, s)
            d.same(s)
    assert n_pass > 0 and any(len(d.ref[s].rows) for s in range(S))
    d.close(); core.close()


def test_stateless_crops(pkg):
    cfg = R.Cfg(thumb_h=24, thumb_w=40, margin_pm=100, min_side=1)
    d = Dev(pkg, cfg, 1, 2)
    F, L = d.F, d.L
    frames = [Frame(pkg, 61, 97, 3 * 97 + 7, 50 + k, True, 0) for k in range(2)]
    one = F.DeviceBuffer(2 * len(frames[0].buf))
    for k in range(2):
        one.upload(frames[k].buf, k * len(frames[k].buf))
    fp = (C.c_void_p * 2)(one.ptr, one.ptr + len(frames[0].buf))
    idx = (np.arange(len(BOXES)) % 2).astype(np.int32)
    want, ok = R.crop(cfg, [f.view for f in frames], BOXES, idx)
    got, sampled = np.zeros_like(want), np.zeros(len(BOXES), np.int32)
    F.check(L.rtmodt_snapshot_crop(d.h, fp, 2, 61, 97, frames[0].stride, F.MEM_DEVICE, F.ptr(BOXES), F.ptr(idx), len(BOXES), F.ptr(got), F.MEM_HOST, F.ptr(sampled)))
    assert np.array_equal(sampled, ok) and 0 < ok.sum() < len(BOXES) and np.array_equal(got, want)
    out = F.DeviceBuffer(want.nbytes)                                   # host frames, thumbnails left in device memory
    out.upload(np.zeros(want.nbytes, np.uint8))
    hp = (C.c_void_p * 2)(frames[0].buf.ctypes.data, frames[1].buf.ctypes.data)
    F.check(L.rtmodt_snapshot_crop(d.h, hp, 2, 61, 97, frames[0].stride, F.MEM_HOST, F.ptr(BOXES), F.ptr(idx), len(BOXES), C.c_void_p(out.ptr), F.MEM_DEVICE, None))
    assert np.array_equal(out.download().reshape(want.shape), want)
    bad = idx.copy()
    bad[3] = 2
    assert L.rtmodt_snapshot_crop(d.h, fp, 2, 61, 97, frames[0].stride, F.MEM_DEVICE, F.ptr(BOXES), F.ptr(bad), len(BOXES), F.ptr(got), F.MEM_HOST, None) == F.E_INVALID
    g = pkg.visualization.SnapshotGallery((24, 40), margin_pm=100, min_side=1)             # the same through the Python class
    t, s = g.crop([frames[0].view.copy(), frames[1].view.copy()], BOXES, idx)
    assert np.array_equal(t, want) and np.array_equal(s, ok.astype(bool))
    g.close(); out.free(); one.free(); d.close()
    for f in frames:
        f.free()


def test_crop_detector_confidence_band(pkg, detector):
    """The review queue on a synthetic detector at its smallest input: the detections of a confidence band, at most max_out per frame,
    in the detector's order, read from the detector's device-resident outputs and cut by the stateless resampler."""
    frames = [f.copy() for f in pkg.synth.frames(2, 320, 320, seed=11)]
    dets = detector.detect_batch(frames)                                      # (the host's copy: what the restatement is fed with)
    conf = np.concatenate([d.confidence for d in dets])
    lo, hi = float(np.float32(np.quantile(conf, 0.25))), float(np.float32(np.quantile(conf, 0.75)))
    g = pkg.visualization.SnapshotGallery((24, 40), min_side=2)
    cfg = R.Cfg(thumb_h=24, thumb_w=40, min_side=2)
    dev = pkg._ffi.DeviceBuffer(2 * 320 * 320 * 3)
    dev.upload(np.stack(frames))
    n = 0
    for max_out in (5, None):
        for where in (frames, dev):
            kw = dict(height=320, width=320, count=2) if where is dev else {}
            got = g.crop_detector(detector, where, lo, hi, max_out, **kw)
            assert len(got) == 2
            for i, (thumbs, idx, ok) in enumerate(got):
                c32 = np.asarray(dets[i].confidence, np.float32)
                want_idx = np.nonzero((c32 >= np.float32(lo)) & (c32 < np.float32(hi)))[0][:max_out]
                assert np.array_equal(idx, want_idx), (max_out, i)
                want, wok = R.crop(cfg, [frames[i]], dets[i].xyxy[want_idx], np.zeros(len(want_idx), np.int32))
                assert np.array_equal(ok, wok.astype(bool)) and np.array_equal(thumbs, want)
                n += int(ok.sum())
    assert n > 0
    assert all(len(t) == 0 for t, _, _ in g.crop_detector(detector, frames, 2.0, 3.0))                 # an empty band
    with pytest.raises(pkg._ffi.RtmodtError) as e:
        g.crop_detector(detector, frames + [frames[0]], lo, hi)                                       # more frames than the batch held
    assert e.value.code == pkg._ffi.E_INVALID
    with pytest.raises(pkg._ffi.RtmodtError):
        g.crop_detector(detector, frames, lo, hi, max_out=0)
    assert np.array_equal(dev.download(), np.stack(frames).reshape(-1))
    dev.free(); g.close()


def test_ledger_follows_ids_the_swap_guard_exchanged(pkg):
    """ByteTrack exchanges the ids of two objects that pass each other and the swap guard exchanges them back inside the tracker's state,
    which leaves the tracker's list out of id order: the rows are then placed by counting, and stay with their ids."""
    import swapguard_ref as SG
    frames, h, w = SG.s1_frames()
    core = pkg.tracking.tracker._ByteTrackCore(0.5, 30, 0.8, n_streams=1, max_tracks=32, max_dets=16)
    guard = pkg.tracking.IdSwapGuard(n_streams=1, max_tracks=32)
    cfg = R.Cfg(thumb_h=16, thumb_w=16, margin_pm=100, min_side=2, occl_iou_pm=300, min_gain_pm=0, retire_after=3)
    d = Dev(pkg, cfg, 1, 32)
    F, L = d.F, d.L
    tracker = SimpleNamespace(_core=core, report="matched")
    reverted, out_of_order = 0, False
    for f, (img, xy, cf, cl) in enumerate(frames):
        xyxy = np.zeros((1, 16, 4), np.float32); conf = np.zeros((1, 16), np.float32); cls = np.zeros((1, 16), np.int32)
        xyxy[0, :len(xy)], conf[0, :len(xy)], cls[0, :len(xy)] = xy, cf, cl
        core.update_batch(xyxy, conf, cls, np.array([len(xy)], np.int32))
        reverted += len(guard.process_tracker(tracker, [img], f)[0])
        st = core.snapshot(0)
        out_of_order |= bool(np.any(np.diff(st["ids"]) <= 0))
        img = np.ascontiguousarray(img)
        fp, fid = (C.c_void_p * 1)(img.ctypes.data), np.int64([f])
        rc = L.rtmodt_snapshot_process_tracker(d.h, core._h, fp, img.shape[0], img.shape[1], img.strides[0], F.MEM_HOST, F.ptr(fid), 1, C.byref(d.out))
        assert rc == 0, L.rtmodt_last_error()
        code, u, r, nrw = d.expect(0, st["ids"], st["xyxy"], st["conf"], st["cls"], img, f, st["tsu"] == 1)
        assert code == 0 and d.results(0) == (u, r, nrw), f
        d.same(0)
    assert reverted == 1 and out_of_order and len(d.ref[0].rows) >= 2
    d.close(); guard.close(); core.close()


def test_jpeg_encoder_on_atlas_slots_in_place(pkg):
    frame = np.random.default_rng(60).integers(0, 256, (61, 97, 3), dtype=np.uint8)
    frame = (frame // 4 + np.arange(97, dtype=np.uint8)[None, :, None]).astype(np.uint8)    # some structure, so that the files differ
    for thumb in ((16, 16), (24, 40)):
        cfg = R.Cfg(thumb_h=thumb[0], thumb_w=thumb[1], margin_pm=100, min_side=4, retire_after=1)
        ref = R.Stream(cfg, 8)
        retired = []
        g = pkg.visualization.SnapshotGallery(thumb, max_tracks=8, margin_pm=100, min_side=4, retire_after=1, on_retired=lambda gal, r: retired.append(r.track_id))
        enc = pkg.visualization.JpegEncoder(90, max_height=64, max_width=64, max_batch=4)
        ids, xy, cf, cl = np.int64([3, 1, 2]), np.float32([[5, 5, 60, 50], [40, 10, 90, 30], [0, 0, 96, 60]]), np.float32([0.5, 0.6, 0.7]), np.int32([0, 0, 0])
        upd, ret = g.process((ids, xy, cf, cl), frame, 0)
        ref.process(ids, xy, cf, cl, frame, 0)
        files = g.jpeg([1, 2, 3], enc)
        for tid, f in zip([1, 2, 3], files):
            assert f == J.encode(ref.atlas[ref.rows[tid].slot], 90), (thumb, tid)
            assert np.array_equal(g.thumbnail(tid), ref.atlas[ref.rows[tid].slot])
        assert len(set(files)) == 3
        slots = sorted(r.slot for r in ref.rows.values())
        assert g.jpeg(slots, enc, slots=True) == [J.encode(ref.atlas[s], 90) for s in slots]
        upd, ret = g.process((ids[:1], xy[:1], cf[:1], cl[:1]), frame, 1)
        assert ret == [] and retired == []
        upd, ret = g.process((ids[:1], xy[:1], cf[:1], cl[:1]), frame, 2)                     # 1 and 2 retire: still readable now
        assert sorted(retired) == [1, 2] and [r.track_id for r in ret] == [1, 2]
        assert g.jpeg([1], enc)[0] == files[0]
        assert [r["track_id"] for r in g.snapshot()["rows"]] == [3]
        enc.close(); g.close()


class _Det:
    model = type("M", (), {"names": {0: "person"}})()

    def detect(self, frame):
        return type("D", (), {"xyxy": np.zeros((1, 4), np.float32), "confidence": np.ones(1, np.float32), "class_id": np.zeros(1, np.int32),
                              "__len__": lambda self: 1})()


def _script(f):
    tr = [SimpleNamespace(track_id=4, xyxy=np.float32([2 + f, 12, 30 + 2 * f, 40]), confidence=0.5 + 0.1 * (f % 3), class_name="person", class_id=0, trail=[])]
    if f < 2:
        tr.append(SimpleNamespace(track_id=9, xyxy=np.float32([30, 5, 60, 45]), confidence=0.7, class_name="person", class_id=0, trail=[]))
    return tr


class _Trk:
    def __init__(self):
        self.f = -1

    def update(self, detections):
        self.f += 1
        return _script(self.f)


def test_pipeline_snapshots_stage(pkg):
    frames = np.random.default_rng(9).integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof(), max_frames=6, device_stages=False, device_handoff=False)
    g = pkg.visualization.SnapshotGallery((16, 16), max_tracks=8, retire_after=1, min_side=4)
    mask = pkg.visualization.PrivacyMask(mode="fill")
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(frames), _Det(), _Trk(), prof(), max_frames=6, device_stages=False, device_handoff=False, snapshots=g,
                           privacy=mask)
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"snapshots_mean_ms", "privacy_mean_ms"}
    assert "snapshots_rewritten" not in base and "snapshots_retired" not in base
    assert pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking", "events", "visualization", "total"]
    ref = R.Stream(R.Cfg(thumb_h=16, thumb_w=16, retire_after=1, min_side=4), 8)
    n_rw = n_rt = 0
    src = pkg.pipeline.SyntheticSource(frames)
    for f in range(6):
        ok, frame, fid = src.read()
        tr = _script(f)
        code, u, r, nrw = ref.process([t.track_id for t in tr], [t.xyxy for t in tr], [t.confidence for t in tr], [0] * len(tr), frame, fid)
        n_rw, n_rt = n_rw + nrw, n_rt + len(r)
    assert (out["snapshots_rewritten"], out["snapshots_retired"]) == (n_rw, n_rt) and n_rw > 0 and n_rt == 1
    assert np.array_equal(g.thumbnail(4), ref.atlas[ref.rows[4].slot])           # the clean pixels: the stage runs before privacy
    mask.close(); g.close()


class _Spy:
    """A recorder that notes, after every frame of the loop, the tracker's own state and the frame the stages saw."""

    def __init__(self, core):
        self.core, self.seen = core, []

    def write(self, frame):
        self.seen.append((self.core.snapshot(0), frame.copy()))


def test_pipeline_snapshots_stage_on_the_tracker_state(pkg, detector):
    """No materialised track list: the stage reads the ByteTrack handle's device-resident state, as the speed stage would.  The ledger,
    every thumbnail and the summary's counts equal the restatement fed with the tracker's own snapshot after every frame."""
    trk = pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    trk.report = "matched"
    src = pkg.synth.frames(2, 320, 320, seed=11)
    with pytest.raises(ValueError, match="max_tracks=2048"):                  # the gallery's default is smaller than the tracker's
        small = pkg.visualization.SnapshotGallery((32, 32))
        try:
            small.process_tracker(trk, [src[0]], 0)
        finally:
            small.close()
    g = pkg.visualization.SnapshotGallery((32, 32), max_tracks=2048, min_side=2, min_gain_pm=0)
    prof = pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    spy = _Spy(trk._core)
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(src), detector, trk, prof, max_frames=4, snapshots=g, recorder=spy)
    assert "snapshots_mean_ms" in out and len(spy.seen) == 4
    ref = R.Stream(R.Cfg(thumb_h=32, thumb_w=32, min_side=2, min_gain_pm=0), 2048)
    fids, probe = [], pkg.pipeline.SyntheticSource(src)
    for _ in range(4):
        fids.append(probe.read()[2])
    n_rw = n_rt = 0
    for (st, frame), fid in zip(spy.seen, fids):
        code, u, r, nrw = ref.process(st["ids"], st["xyxy"], st["conf"], st["cls"], frame, fid, st["tsu"] == 1)
        assert code == 0
        n_rw, n_rt = n_rw + nrw, n_rt + len(r)
    assert (out["snapshots_rewritten"], out["snapshots_retired"]) == (n_rw, n_rt)
    rows = g.snapshot()["rows"]
    want = ref.ledger()
    assert len(want) > 0 and [(r["track_id"], r["slot"], r["best_score"], r["best_frame"], r["n_rewrites"], r["flags"]) for r in rows] == \
        [(r.track_id, r.slot, r.best_score, r.best_frame, r.n_rewrites, r.flags) for r in want]
    slots = [r.slot for r in want]
    assert np.array_equal(g.read(slots), ref.atlas[slots])
    g.close()
