"""GPU: ``csrc/compose.hip`` against ``tests/compose_ref.py``.  EVERY byte of every destination is compared, the bytes a run must
not touch included: destinations are pre-filled with a guard pattern and the expectation is the same guard with only the rows'
own bytes replaced.  The layouts are those of ``tests/compose_cases.py`` (the smallest that reach every path: the three kinds of
axis and their mix, 1 x 1 cells, the 16384 limits, the band walk, tile seams, painting order, 64 cells, 16 outputs, NV12 / I420);
their expected pictures are computed once per session and shared."""
from types import SimpleNamespace

import numpy as np
import pytest

import compose_cases as CC
import compose_ref as R
import jpeg_ref as J
import render_ref as RR

pytestmark = pytest.mark.gpu
GUARD = 0xA5
FMT = {R.BGR24: "bgr24", R.NV12: "nv12", R.I420: "i420"}


def layout(pkg, name):
    VC = pkg.visualization.compose
    sources, outputs, cells, _ = CC.CASES[name]
    return (sources, [VC.Output((o.h, o.w), FMT[o.fmt], o.background) for o in outputs],
            [VC.Cell(c.output, c.source, c.rect, c.crop, c.fit, c.pad, c.offline) for c in cells])


@pytest.fixture(scope="module")
def compositors(pkg):
    made = {}

    def get(name):
        if name not in made:
            made[name] = pkg.visualization.Compositor(*layout(pkg, name))
        return made[name]
    yield get
    for c in made.values():
        c.close()


def geometry(o, mode):
    """Placement of one output's planes: ``tight`` (all defaults), ``odd`` (pitches that are no multiple of 4, planes pushed apart by
    odd gaps), ``wide`` (pitches that are multiples of 16)."""
    if mode == "tight":
        return {}
    if o.fmt == R.BGR24:
        return {"pitch": 3 * o.w + (5 if mode == "odd" else (-3 * o.w) % 16 + 16)}
    pitch = o.w + 3 if mode == "odd" else o.w + (-o.w) % 16 + 16
    cp = (o.w if o.fmt == R.NV12 else o.w // 2) + (7 if mode == "odd" else 9 + (-(o.w if o.fmt == R.NV12 else o.w // 2) - 9) % 16)
    uo = pitch * o.h + (11 if mode == "odd" else 32)
    g = {"pitch": pitch, "chroma_pitch": cp, "u_offset": uo}
    if o.fmt == R.I420:
        g["v_offset"] = uo + cp * (o.h // 2) + (13 if mode == "odd" else 16)
    return g


def expected_buffer(name, i, geo, tail=9):
    o = CC.CASES[name][1][i]
    span = R.resolve_format(o.fmt, o.h, o.w, **geo)[4]
    buf = np.full(span + tail, GUARD, np.uint8)
    R.write_output(buf, CC.expected(name)[i], o.fmt, **geo)
    return buf


def first_diff(a, b):
    d = np.flatnonzero(a != b)
    return f"{d.size} bytes differ, first at {int(d[0])}: got {int(a[d[0]])}, want {int(b[d[0]])}" if d.size else "equal"


def fmt_of(pkg, o, geo):
    return pkg._ffi.frame_format(FMT[o.fmt], o.h, o.w, **geo)


# ---------------------------------------------------------------------------------------------------------------- every case, host to host
@pytest.mark.parametrize("name", list(CC.CASES))
def test_every_case_host_to_host(pkg, compositors, name):
    """Axis kinds, limits and ratios, tile seams, painting order (top-most cell, a covered cell, a camera that is down, a source in two
    cells), 64 cells, 16 outputs, 4:2:0 -- padded rows and the gaps between the planes keep their guard bytes."""
    comp = compositors(name)
    outputs = CC.CASES[name][1]
    geos = [geometry(o, "odd") for o in outputs]
    want = [expected_buffer(name, i, g) for i, g in enumerate(geos)]
    bufs = [np.full(w.size, GUARD, np.uint8) for w in want]
    comp.run(list(CC.frames(name)), [(b, fmt_of(pkg, o, g)) for b, o, g in zip(bufs, outputs, geos)])
    for i, (b, w) in enumerate(zip(bufs, want)):
        assert np.array_equal(b, w), f"{name}: output {i}: {first_diff(b, w)}"
    assert comp.last_ms() > 0


def test_default_run_returns_packed_arrays(pkg, compositors):
    for name in ("order", "nv12", "i420"):
        got = compositors(name).run(list(CC.frames(name)))
        for o, g, w in zip(CC.CASES[name][1], got, CC.expected(name)):
            if o.fmt == R.BGR24:
                assert np.array_equal(g, w), name
            else:
                want = np.zeros(o.h * o.w * 3 // 2, np.uint8)
                R.write_output(want, w, o.fmt)
                assert g.shape == (o.h * 3 // 2, o.w) and np.array_equal(g.reshape(-1), want), name


# ---------------------------------------------------------------------------------------------------------------- alignment, device to device
def device_run(pkg, comp, name, soff, spad, doff, mode):
    """Sources and destinations in device memory: source i at an address that is ``soff`` modulo 256 with rows ``3w + spad`` bytes
    apart, destination i at ``doff`` modulo 256 with the planes of ``geometry(mode)``.  Returns (got, want) buffers per output."""
    F = pkg._ffi
    sources, outputs = CC.CASES[name][0], CC.CASES[name][1]
    frames = CC.frames(name)
    sp = [3 * w + spad for _, w in sources]
    so = np.cumsum([0] + [(h * p + 511) // 256 * 256 for (h, _), p in zip(sources, sp)])
    sbuf = F.DeviceBuffer(int(so[-1]) + 256)
    src = []
    for i, f in enumerate(frames):
        if f is None:
            src.append(None)
            continue
        h, w = sources[i]
        rows = np.full((h, sp[i]), 0x3C, np.uint8)
        rows[:, :3 * w] = f.reshape(h, 3 * w)
        sbuf.upload(rows, int(so[i]) + soff)
        src.append((sbuf, int(so[i]) + soff, sp[i]))
    geos = [geometry(o, mode) for o in outputs]
    want = [expected_buffer(name, i, g) for i, g in enumerate(geos)]
    do = np.cumsum([0] + [(w.size + doff + 511) // 256 * 256 for w in want])
    dbuf = F.DeviceBuffer(int(do[-1]) + 256)
    dbuf.upload(np.full(dbuf.nbytes, GUARD, np.uint8))
    comp.run(src, [(dbuf, int(do[i]) + doff, fmt_of(pkg, o, g)) for i, (o, g) in enumerate(zip(outputs, geos))])
    got = [dbuf.download(w.size, int(do[i]) + doff) for i, w in enumerate(want)]
    before = [dbuf.download(doff, int(do[i])) for i in range(len(want))] if doff else []
    sbuf.free(); dbuf.free()
    assert all((b == GUARD).all() for b in before)
    return got, want


@pytest.mark.parametrize("soff,spad,doff,mode", [(1, 7, 3, "odd"), (5, 1, 1, "tight"), (0, 0, 0, "wide"), (16, 13, 32, "wide"), (2, 2, 0, "tight")])
@pytest.mark.parametrize("name", ["seams", "enlarge", "band", "nv12", "i420"])
def test_alignment_device_to_device(pkg, compositors, name, soff, spad, doff, mode):
    """Odd base addresses and pitches that are no multiple of 16 or 4 on both sides (the ragged ends of the 16-byte loads and stores),
    and fully aligned ones (whole rows as 16-byte blocks)."""
    got, want = device_run(pkg, compositors(name), name, soff, spad, doff, mode)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"{name}: output {i}: {first_diff(g, w)}"


# ---------------------------------------------------------------------------------------------------------------- 4:2:0 plane placement
@pytest.mark.parametrize("name", ["nv12", "i420"])
@pytest.mark.parametrize("mode", ["tight", "odd", "wide"])
def test_yuv_plane_placement_host(pkg, compositors, name, mode):
    """Default and explicit chroma pitch and plane offsets; the guard bytes between the planes stay."""
    o = CC.CASES[name][1][0]
    geo = geometry(o, mode)
    want = expected_buffer(name, 0, geo)
    buf = np.full(want.size, GUARD, np.uint8)
    compositors(name).run(list(CC.frames(name)), [(buf, fmt_of(pkg, o, geo))])
    assert np.array_equal(buf, want), first_diff(buf, want)
    if mode != "tight":
        pitch, cp, uo, vo, _ = R.resolve_format(o.fmt, o.h, o.w, **geo)
        assert (want[pitch * (o.h - 1) + o.w:uo] == GUARD).all() and uo > pitch * (o.h - 1) + o.w          # a gap there is, and it is kept


# ---------------------------------------------------------------------------------------------------------------- memory kinds
def test_mixed_memory_kinds(pkg, compositors):
    F, name = pkg._ffi, "order"
    comp, (sources, outputs, _, _) = compositors(name), CC.CASES[name]
    o = outputs[0]
    want = expected_buffer(name, 0, {}, tail=0)
    # host sources -> device destination
    dbuf = F.DeviceBuffer(want.size + 64)
    dbuf.upload(np.full(dbuf.nbytes, GUARD, np.uint8))
    comp.run(list(CC.frames(name)), [(dbuf, 32, None)])
    assert np.array_equal(dbuf.download(want.size, 32), want) and (dbuf.download(32, 0) == GUARD).all() and (dbuf.download(32, 32 + want.size) == GUARD).all()
    # device sources -> host destination
    sbuf = F.DeviceBuffer(sum(h * w * 3 for h, w in sources))
    src, off = [], 0
    for (h, w), f in zip(sources, CC.frames(name)):
        if f is not None:
            sbuf.upload(f, off)
        src.append(None if f is None else (sbuf, off, None))
        off += h * w * 3
    got = comp.run(src)[0]
    assert np.array_equal(got, CC.expected(name)[0])
    sbuf.free(); dbuf.free()


def test_own_buffer_feeds_renderer_and_jpeg(pkg, compositors):
    """The wall stays in the compositor's own device buffer; FrameRenderer draws on it and JpegEncoder encodes it where it lies."""
    name = "seams"
    comp, o = compositors(name), CC.CASES[name][1][0]
    views = comp.run(list(CC.frames(name)), "device")
    view, pitch = comp.output(0)
    assert views[0].ptr == view.ptr and pitch % 16 == 0 and pitch >= 3 * o.w
    wall = CC.expected(name)[0]
    rows = view.download(pitch * o.h).reshape(o.h, pitch)
    assert np.array_equal(rows[:, :3 * o.w].reshape(o.h, o.w, 3), wall)
    enc = pkg.JpegEncoder(90, max_height=o.h, max_width=o.w, max_batch=1)
    assert enc.encode_batch(view, height=o.h, width=o.w, stride=pitch, count=1)[0] == J.encode(wall, 90)
    # a track of source 1, carried onto the wall through cell 1's plan, drawn by the renderer on the buffer
    box = comp.map_boxes(1, [[20, 5, 50, 30]])[0]
    p = R.plan(CC.CASES[name][0][1], CC.CASES[name][2][1], False)
    assert np.allclose(box, np.concatenate([R.map_points(p, [[20, 5]])[0], R.map_points(p, [[50, 30]])[0]]))
    track = SimpleNamespace(track_id=7, xyxy=box.astype(np.float32), confidence=np.float32(0.5), class_name="car", trail=[])
    pkg.FrameRenderer(show_fps=False).render_batch(view, [[track]], height=o.h, width=o.w, stride=pitch)
    drawn = view.download(pitch * o.h).reshape(o.h, pitch)[:, :3 * o.w].reshape(o.h, o.w, 3)
    assert np.array_equal(drawn, RR.render(wall.copy(), [track], None, 0.0, 0.0, show_fps=False)) and not np.array_equal(drawn, wall)
    assert enc.encode_batch(view, height=o.h, width=o.w, stride=pitch, count=1)[0] == J.encode(drawn, 90)


# ---------------------------------------------------------------------------------------------------------------- other behaviour
def test_set_crop_between_runs(pkg):
    """Follow-zoom: an inset on top of the full view is re-planned between runs, to crops of every kind of axis; the rest stays."""
    VC = pkg.visualization.compose
    src = (60, 90)
    f = CC.frame(60, 90, 3)
    comp = pkg.visualization.Compositor([src], [VC.Output((40, 64))], [VC.Cell(0, 0, (0, 0, 64, 40), fit="stretch")])
    k = comp.add_inset(0, (10, 10, 12, 8), (37, 3, 24, 16), fit="stretch")
    cells = [R.Cell(0, 0, (0, 0, 64, 40), fit=R.STRETCH), R.Cell(0, 0, (37, 3, 24, 16), (10, 10, 12, 8), R.STRETCH)]
    for crop in [(10, 10, 12, 8), (0, 0, 90, 60), (66, 44, 24, 16), (5, 5, 80, 5), (0, 0, 0, 0), (89, 59, 1, 1)]:
        comp.set_crop(k, crop)
        cells[1] = R.Cell(0, 0, (37, 3, 24, 16), crop, R.STRETCH)
        assert np.array_equal(comp.run([f])[0], R.compose([src], [R.Output(40, 64)], cells, [f])[0]), crop
        assert comp.plans[k].crop == R.plan(src, cells[1], False).crop
    with pytest.raises(pkg._ffi.RtmodtError, match="crop") as e:
        comp.set_crop(k, (80, 0, 20, 5))
    assert e.value.code == pkg._ffi.E_INVALID
    assert np.array_equal(comp.run([f])[0], R.compose([src], [R.Output(40, 64)], cells, [f])[0])             # the refused crop changed nothing
    # a rejected layout leaves the previous one in force
    with pytest.raises(pkg._ffi.RtmodtError, match="leaves"):
        comp.set_layout([src], [VC.Output((40, 64))], [VC.Cell(0, 0, (60, 0, 10, 10))])
    assert np.array_equal(comp.run([f])[0], R.compose([src], [R.Output(40, 64)], cells, [f])[0])
    comp.close()


def test_refusals_launch_nothing(pkg, compositors):
    F, name = pkg._ffi, "shrink"
    comp = compositors(name)
    (h, w), o = CC.CASES[name][0][0], CC.CASES[name][1][0]
    f = CC.frames(name)[0]
    buf = F.DeviceBuffer(h * w * 3 + o.h * o.w * 3 + 64)
    fill = np.full(buf.nbytes, GUARD, np.uint8)
    fill[:h * w * 3] = f.reshape(-1)
    buf.upload(fill)
    src = [(buf, 0, None)]
    bad = [[(buf, h * w * 3 - 1, None)],                                            # the destination's first byte is the source's last
           [(buf, 0, None)],
           [(buf, h * w * 3, F.FrameFormat(F.PIX_BGR24, 0, 3 * o.w - 1, 0, 0, 0))],  # pitch below 3w
           [(buf, h * w * 3, F.FrameFormat(F.PIX_NV12, 0, 0, 0, 0, 0))]]              # not the layout's format
    for out in bad:
        with pytest.raises((F.RtmodtError, ValueError)) as e:
            comp.run(src, out)
        assert not isinstance(e.value, F.RtmodtError) or e.value.code == F.E_INVALID
        assert np.array_equal(buf.download(), fill)
    # straight through the C ABI: Python's own checks aside
    import ctypes as C
    sp, pitches, dp = (C.c_void_p * 1)(buf.ptr), (C.c_int32 * 1)(3 * w), (C.c_void_p * 1)(buf.ptr + 3 * w * (h - 1))
    L = F.lib()
    assert L.rtmodt_compose_run(comp._h, sp, pitches, F.MEM_DEVICE, dp, None, F.MEM_DEVICE) == F.E_INVALID and "overlaps source 0" in L.rtmodt_last_error().decode()
    assert L.rtmodt_compose_run(comp._h, sp, pitches, 2, dp, None, F.MEM_DEVICE) == F.E_INVALID
    pitches[0] = 3 * w - 1
    assert L.rtmodt_compose_run(comp._h, sp, pitches, F.MEM_DEVICE, None, None, F.MEM_DEVICE) == F.E_INVALID and "pitch" in L.rtmodt_last_error().decode()
    own, _ = comp.output(0)                                                     # the handle's own buffer may not be a source of a run that writes it
    sp[0], pitches[0] = own.ptr, 3 * w
    assert L.rtmodt_compose_run(comp._h, sp, pitches, F.MEM_DEVICE, None, None, F.MEM_DEVICE) == F.E_INVALID and "own buffer" in L.rtmodt_last_error().decode()
    assert np.array_equal(buf.download(), fill)
    # two destinations that share bytes
    two = pkg.visualization.Compositor([(4, 4)], [pkg.visualization.Output((4, 4)), pkg.visualization.Output((4, 4))],
                                       [pkg.visualization.Cell(0, 0, (0, 0, 4, 4)), pkg.visualization.Cell(1, 0, (0, 0, 4, 4))])
    with pytest.raises(F.RtmodtError, match="overlaps destination 0"):
        two.run([CC.frame(4, 4, 1)], [(buf, h * w * 3, None), (buf, h * w * 3 + 47, None)])
    assert np.array_equal(buf.download(), fill)
    two.close(); buf.free()


class _Recorder:
    def __init__(self):
        self.frames = []

    def write(self, frame):
        self.frames.append(frame.copy())


def test_pipeline_compose_stage(pkg, tmp_path):
    import os
    path = os.path.join(str(tmp_path), "yolov8n_320.rtw")
    pkg.weights.save(path, pkg.weights.synthetic("n", input_size=320), "n")
    detector = pkg.Detector(path, input_size=(320, 320), confidence=0.02, max_det=20, warmup=False, autotune=False)
    size, sub = (77, 131), (22, 40)
    frames = [CC.frame(size[0], size[1], 50 + i) for i in range(4)]
    prof = lambda: pkg.profiling.LatencyProfiler(gpu_sync=False, warmup_frames=0, log_interval=1000)
    tracker = lambda: pkg.MultiObjectTracker("bytetrack", track_thresh=0.05)
    base_p = prof()
    base = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), base_p, max_frames=4)
    comp = pkg.visualization.Compositor.substream(size, sub)
    rec, p = _Recorder(), prof()
    out = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=4, compose=comp, recorder=rec)
    want = [R.resample(f, sub[0], sub[1]) for f in frames]
    assert len(rec.frames) == 4 and all(np.array_equal(a, b) for a, b in zip(rec.frames, want))              # the recorder receives the sub-stream
    rows = lambda d: {k for k in d if k.endswith("_mean_ms")}
    assert rows(out) - rows(base) == {"compose_mean_ms"} and rows(base) <= rows(out)
    order = list(p.STAGE_ORDER)
    assert order.index("compose") == order.index("visualization") + 1
    # compose=None: the parent's stage table and summary keys, and the recorder receives the full frame
    rec, p = _Recorder(), prof()
    none = pkg.pipeline.run(pkg.pipeline.SyntheticSource(np.stack(frames)), detector, tracker(), p, max_frames=4, compose=None, recorder=rec)
    assert set(none) == set(base) and "compose_mean_ms" not in none
    assert list(p.STAGE_ORDER) == list(base_p.STAGE_ORDER) == pkg.profiling.LatencyProfiler.STAGE_ORDER == ["decode", "preprocess", "inference", "nms", "tracking",
                                                                                                           "events", "visualization", "total"]
    assert all(np.array_equal(a, b) for a, b in zip(rec.frames, frames))
    comp.close()
    detector.close()
