"""GPU: one handle across calls of changing size (csrc/frame_stage.h: the staging buffer grows, then is reused by a smaller call).
Every frame-taking module makes three calls on ONE handle, small -> large -> small (frames of 37 x 53 at pitch 3 * 53 + 7, of
64 x 100 at pitch 304, of 37 x 53 again; batches of 1, 3 and 2), first on host frames, then the same three on a DeviceBuffer from
offset 32.  Every result equals the module's own reference bit for bit, and every byte outside the frames' rows -- the padding of
each row, the 32 bytes before the first frame and the 32 behind the last -- comes back as the random byte it was.  Where a handle
fixes the batch to its stream count, only the frame size changes; where it fixes the geometry, only the batch and the padding."""
import os
import sys
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deepsort_ref as DS  # noqa: E402
import heatmap_ref as HR  # noqa: E402
import jpeg_dec_cases as K  # noqa: E402
import jpeg_dec_ref as JD  # noqa: E402
import jpeg_ref as J  # noqa: E402
import privacy_ref as PR  # noqa: E402
import reid_ref as RR  # noqa: E402
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CALLS = [(1, 37, 53, 3 * 53 + 7), (3, 64, 100, 304), (2, 37, 53, 3 * 53 + 7)]       # (batch, h, w, pitch): small, large, small
LEAD = 32


def batch(seed, n, h, stride):
    """n frames of h rows in one buffer [n, h * stride] of random bytes (the padding included)."""
    return np.random.default_rng(seed).integers(0, 256, (n, h * stride), dtype=np.uint8)


def views(buf, h, w, stride):
    return [np.lib.stride_tricks.as_strided(b, (h, w, 3), (stride, 3, 1), writeable=buf.flags.writeable) for b in buf]


def outside_rows(n, h, w, stride):
    pad = np.ones((n, h, stride), bool)
    pad[:, :, :3 * w] = False
    return pad.reshape(n, h * stride)


def same(got, want, what):
    bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at {bad[:6].tolist()}"


class OnDevice:
    """``buf`` inside a DeviceBuffer, LEAD random bytes before it and LEAD behind it."""

    def __init__(self, pkg, buf, seed):
        self.host = np.concatenate([np.random.default_rng(seed).integers(0, 256, LEAD, dtype=np.uint8), buf.reshape(-1),
                                    np.random.default_rng(seed + 1).integers(0, 256, LEAD, dtype=np.uint8)])
        self.dev = pkg._ffi.DeviceBuffer(self.host.nbytes)
        self.dev.upload(self.host)
        self.shape = buf.shape

    def addresses(self):
        return [self.dev.ptr + LEAD + i * self.shape[1] for i in range(self.shape[0])]

    def finish(self, want, what):
        """The buffer equals ``want`` and the bytes around it are untouched; frees the buffer."""
        got = self.dev.download()
        self.dev.free()
        same(got[LEAD:-LEAD], want, what)
        assert np.array_equal(got[:LEAD], self.host[:LEAD]) and np.array_equal(got[-LEAD:], self.host[-LEAD:]), f"{what}: bytes around the frames were written"


def in_place(pkg, what, reference, on_host, on_device, calls=CALLS):
    """An in-place module: reference(call, view, i) -> the frame afterwards; on_host(call, views) / on_device(call, buffer, kw) run it."""
    for kind in ("host", "device"):
        for c, (n, h, w, stride) in enumerate(calls):
            buf = batch(1000 * c + n, n, h, stride)
            want = buf.copy()
            for i, (src, dst) in enumerate(zip(views(buf, h, w, stride), views(want, h, w, stride))):
                dst[:] = reference(c, src, i)
            assert not np.array_equal(want, buf), "the scene changes nothing"
            assert np.array_equal(want[outside_rows(n, h, w, stride)], buf[outside_rows(n, h, w, stride)])
            if kind == "host":
                got = buf.copy()
                on_host(c, views(got, h, w, stride))
                same(got, want, f"{what}, host, call {c}")
            else:
                d = OnDevice(pkg, buf, c)
                on_device(c, d.dev, dict(height=h, width=w, stride=stride, offset=LEAD))
                d.finish(want, f"{what}, device, call {c}")


def boxes_in(seed, k, h, w):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.uniform(0, w - 6, k), rng.uniform(0, h - 6, k)
    return np.stack([x0, y0, x0 + rng.uniform(3, w / 2, k), y0 + rng.uniform(3, h / 2, k)], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ in place
def test_renderer(pkg):
    zones = [("z", np.array([[5, 4], [40, 6], [30, 30], [8, 25]], np.int32))]

    def tracks(c, i):
        _, h, w, _ = CALLS[c]
        return [SimpleNamespace(track_id=10 * c + i + k, xyxy=b, confidence=np.float32(0.5), class_name="car", trail=[(3 + k, 4), (20, 9 + k), (w - 2, h - 3)])
                for k, b in enumerate(boxes_in(31 * c + i, 4, h, w))]

    r = pkg.FrameRenderer()
    handle = r._h
    in_place(pkg, "renderer", lambda c, v, i: R.render(v, tracks(c, i), zones, 25.0, 8.0),
             lambda c, vs: r.render_batch(vs, [tracks(c, i) for i in range(len(vs))], zones=zones, fps=25.0, latency_ms=8.0),
             lambda c, dev, kw: r.render_batch(dev, [tracks(c, i) for i in range(CALLS[c][0])], zones=zones, fps=25.0, latency_ms=8.0, **kw))
    assert r._h is handle, "the calls went to more than one handle"
    r.close()


@pytest.mark.parametrize("m", [dict(mode="pixelate", cell=3), dict(mode="blur", radius=5, passes=2)], ids=lambda m: m["mode"])
def test_privacy(pkg, m):
    def boxes(c, i):
        return boxes_in(7 * c + i, 3, CALLS[c][1], CALLS[c][2]), np.zeros(3, np.int32)

    mask = pkg.visualization.PrivacyMask(**m)
    handle = mask._h
    in_place(pkg, f"privacy {m['mode']}", lambda c, v, i: PR.apply(v, *boxes(c, i), **m),
             lambda c, vs: mask.apply_batch(vs, [boxes(c, i) for i in range(len(vs))]),
             lambda c, dev, kw: mask.apply_batch(dev, [boxes(c, i) for i in range(CALLS[c][0])], **kw))
    assert mask._h is handle
    mask.close()


def test_heatmap_overlay(pkg):
    """The handle pins the frame size: the batch (1, 3, 2 of its 3 streams) and the row padding (7, 145, 7 bytes) change."""
    h, w, cell, S = 37, 53, 4, 3
    calls = [(n, h, w, 3 * w + pad) for n, pad in ((1, 7), (3, 145), (2, 7))]
    streams = [[2], [0, 1, 2], [1, 0]]
    gh, gw = HR.grid_shape(h, w, cell)
    grids = [np.random.default_rng(50 + s).integers(0, 90, (gh, gw)).astype(np.uint32) for s in range(S)]
    hm = pkg.visualization.Heatmap(S, h, w, cell=cell)
    for s in range(S):
        hm.load(grids[s], s)
    in_place(pkg, "heatmap overlay", lambda c, v, i: HR.overlay(v, grids[streams[c][i]], cell),
             lambda c, vs: hm.overlay(vs, streams=streams[c]),
             lambda c, dev, kw: hm.overlay(dev, streams=streams[c], stride=kw["stride"], offset=kw["offset"]), calls=calls)
    hm.close()


# ------------------------------------------------------------------------------------------------------------ read only
def test_jpeg_encode(pkg):
    enc = pkg.JpegEncoder(80, max_height=64, max_width=100, max_batch=3)          # (made for the largest call: a larger one would re-make the handle)
    handle = enc._h
    for kind in ("host", "device"):
        for c, (n, h, w, stride) in enumerate(CALLS):
            buf = batch(2000 * c + n, n, h, stride)
            want = [J.encode(v, 80) for v in views(buf, h, w, stride)]
            if kind == "host":
                src = buf.copy()
                got = enc.encode_batch(views(src, h, w, stride))
                same(src, buf, f"jpeg encode, host, call {c}: the frames")
            else:
                d = OnDevice(pkg, buf, c)
                got = enc.encode_batch(d.dev, height=h, width=w, stride=stride, offset=LEAD, count=n)
                d.finish(buf, f"jpeg encode, device, call {c}: the frames")
            assert got == want, (kind, c, [len(g) for g in got], [len(x) for x in want])
    assert enc._h is handle
    enc.close()


def test_jpeg_decode(pkg):
    dec = pkg.ingestion.JpegDecoder(max_height=64, max_width=100, max_batch=3, max_file_bytes=1 << 16)
    handle = dec._h
    for kind in ("host", "device"):
        for c, (n, h, w, stride) in enumerate(CALLS):
            files = [K.pillow_file(K.frame(("noise", "smooth", "checker")[i], h, w, seed=c), (40, 97, 80)[i], ("420", "444", "422")[i], ("row", "none", "mcu3")[i])
                     for i in range(n)]
            buf = batch(3000 * c + n, n, h, stride)
            want = buf.copy()
            for f, dst in zip(files, views(want, h, w, stride)):
                hd, coefs, st = JD.entropy_decode(f)
                assert st == JD.OK
                dst[:] = JD.pixels(hd, coefs)
            if kind == "host":
                got = buf.copy()
                out = np.lib.stride_tricks.as_strided(got, (n, h, w, 3), (h * stride, stride, 3, 1))
                status = dec.decode_batch(files, out=out)[1]
                same(got, want, f"jpeg decode, host, call {c}")
            else:
                d = OnDevice(pkg, buf, c)
                status = dec.decode_batch(files, out=d.dev, height=h, width=w, stride=stride, offset=LEAD)[1]
                d.finish(want, f"jpeg decode, device, call {c}")
            assert status.tolist() == [JD.OK] * n
    assert dec._h is handle
    dec.close()


def test_reid_embed(pkg, tmp_path):
    """What checks the staging: the crops the network is fed equal reid_ref.crop bit for bit (the kernel read the right bytes at the
    right pitch), and device frames give the descriptors host frames gave.  The descriptor against the quantisation of the handle's own
    feature is a consistency check only (not independent of the code under test); the network itself is tests/test_gpu_reid.py's."""
    path = str(tmp_path / "osnet_synth.rtreid")
    pkg.reid_weights.save(path, pkg.reid_weights.synthetic(0))
    eng = pkg.tracking.ReidEmbedder(path, max_boxes=4, max_frames=3)
    descs = {}
    for kind in ("host", "device"):
        for c, (n, h, w, stride) in enumerate(CALLS):
            buf = batch(4000 * c + n, n, h, stride)
            vs = views(buf, h, w, stride)
            xy = np.stack([boxes_in(11 * c + i, 4, h, w) for i in range(n)])
            if kind == "host":
                src = buf.copy()
                feat, desc = eng.embed(views(src, h, w, stride), xy, [4] * n)
                same(src, buf, f"reid, host, call {c}: the frames")
            else:
                d = OnDevice(pkg, buf, c)
                feat, desc = eng.embed(d.addresses(), xy, [4] * n, mem_kind=pkg._ffi.MEM_DEVICE, height=h, width=w, stride=stride)
            crops = eng.tap("crop")
            if kind == "device":
                d.finish(buf, f"reid, device, call {c}: the frames")
            for i in range(n):
                for b in range(4):
                    want = RR.crop(vs[i], xy[i, b])
                    assert want is not None and np.array_equal(crops[i, b], want), (kind, c, i, b)
            assert np.array_equal(desc, RR.quantize_rows(feat.reshape(-1, feat.shape[-1])).reshape(desc.shape)) and desc.any()
            assert np.array_equal(descs.setdefault(c, desc), desc), f"call {c}: device frames give other descriptors than host frames"
    eng.close()


def test_deepsort_update_batch_with_frames(pkg):
    """The handle fixes the batch to its two streams: the frame size changes.  State against deepsort_ref after every call."""
    S, max_dets = 2, 4
    core = import_module(pkg.__name__ + ".tracking.deepsort")._DeepSortCore(n_streams=S, max_tracks=16, max_dets=max_dets)
    refs = [DS.DeepSortRef() for _ in range(S)]
    for kind in ("host", "device"):
        for c, (_, h, w, stride) in enumerate(CALLS):
            buf = batch(5000 * c + S, S, h, stride)
            vs = views(buf, h, w, stride)
            xy = np.stack([boxes_in(13 * c + s, max_dets, h, w) for s in range(S)])
            cf, cl = np.full((S, max_dets), 0.9, np.float32), np.zeros((S, max_dets), np.int32)
            want = [refs[s].tracks_out(refs[s].update(xy[s], cf[s], cl[s], DS.describe(vs[s], xy[s])[0])) for s in range(S)]
            if kind == "host":
                src = buf.copy()
                ret = core.update_batch(xy, cf, cl, [max_dets] * S, frames=views(src, h, w, stride))
                same(src, buf, f"deepsort, host, call {c}: the frames")
            else:
                d = OnDevice(pkg, buf, c)
                ret = core.update_batch(xy, cf, cl, [max_dets] * S, frames=d.addresses(), mem_kind=pkg._ffi.MEM_DEVICE, height=h, width=w, stride=stride)
                d.finish(buf, f"deepsort, device, call {c}: the frames")
            for s in range(S):
                diff = DS.snapshots_equal(core.snapshot(s), refs[s].snapshot())
                assert diff is None, (kind, c, s, diff)
                assert ret[s] == len(want[s])
    assert len(refs[0].ids) > 0
    core.close()
