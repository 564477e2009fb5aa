"""Video-wall mosaics, sub-streams and zoom insets on MI355X: BGR24 sources are scaled and placed into one or more outputs -- BGR24,
NV12 or I420 -- in one launch (``csrc/compose.hip``; rules: ``csrc/compose_rule.h``); there is no CPU implementation here.  The
reference has no such step (its web page shows one image and ``tools/run_pipeline.py`` writes the full frame).
``tests/compose_ref.py`` restates every rule and every output byte equals it exactly.  Unpinned: ``cv2.resize`` (INTER_AREA /
INTER_LINEAR), ``cv2.cvtColor(..., COLOR_BGR2YUV_I420)`` (whose chroma comes from one pixel of the block) and any encoder's reading
of the NV12; shrinking by integer factors whose product is a power of two equals Pillow's ``Image.reduce``.

Sizes are ``(height, width)``; rectangles are ``(x, y, w, h)``; colours are ``(b, g, r)``; points are ``(x, y)`` with pixel centres
at integers.  A LAYOUT is static: sources, outputs, and cells painted in list order (a later cell lies on top: picture in picture).
Text and borders are the renderer's: ``FrameRenderer`` draws on an output, with ``map_points`` / ``map_boxes`` carrying tracks over.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Sequence

import numpy as np

from .. import _ffi

FITS = {"stretch": 0, "fit": 1, "fill": 2}
KINDS = ("shrink", "copy", "enlarge")


def _fit_id(fit) -> int:
    if isinstance(fit, (int, np.integer)) and int(fit) in FITS.values():
        return int(fit)
    if str(fit).lower() not in FITS:
        raise ValueError(f"unknown fit mode {fit!r}; one of {sorted(FITS)}")
    return FITS[str(fit).lower()]


@dataclasses.dataclass
class Output:
    """One output picture: ``size`` (h, w), ``fmt`` ``"bgr24" | "nv12" | "i420"`` (4:2:0: even sizes), the colour no cell covers."""
    size: tuple
    fmt: object = "bgr24"
    background: tuple = (0, 0, 0)


@dataclasses.dataclass
class Cell:
    """``source``'s ``crop`` (zeros: all of it -- the digital zoom) shown in ``rect`` of ``output``.  ``fit``: ``"stretch"``,
    ``"fit"`` (aspect kept, bars in ``pad``) or ``"fill"`` (aspect kept, the crop cut centrally).  ``offline``: the colour of the
    whole rectangle in a run whose source is ``None`` (the camera is down)."""
    output: int
    source: int
    rect: tuple
    crop: tuple = (0, 0, 0, 0)
    fit: object = "fit"
    pad: tuple = (0, 0, 0)
    offline: tuple = (0, 0, 0)


@dataclasses.dataclass
class CellPlan:
    """What the library planned for a cell: the effective ``crop`` in the source, the ``inner`` picture in the output, the axes."""
    crop: tuple
    inner: tuple
    kind_x: str
    kind_y: str


class _OutputView(_ffi.DeviceBuffer):
    """An output in the compositor's own device buffer as the ``DeviceBuffer`` the frame modules take; the compositor owns the memory."""

    def __init__(self, ptr: int, nbytes: int, device: int):
        self.device, self.nbytes, self.ptr = device, nbytes, ptr

    def free(self):
        self.ptr = None


def _c_layout(sources, outputs, cells):
    cs = (_ffi.ComposeSource * max(len(sources), 1))()
    for i, (h, w) in enumerate(sources):
        cs[i].h, cs[i].w = int(h), int(w)
    co = (_ffi.ComposeOutput * max(len(outputs), 1))()
    for i, o in enumerate(outputs):
        co[i].h, co[i].w = int(o.size[0]), int(o.size[1])
        co[i].pixel_format = _ffi.pixel_format_id(o.fmt)
        co[i].background_bgr = (C.c_uint8 * 3)(*[int(v) for v in o.background])
    cc = (_ffi.ComposeCell * max(len(cells), 1))()
    for i, c in enumerate(cells):
        cc[i].output, cc[i].source = int(c.output), int(c.source)
        cc[i].x, cc[i].y, cc[i].w, cc[i].h = (int(v) for v in c.rect)
        cc[i].crop_x, cc[i].crop_y, cc[i].crop_w, cc[i].crop_h = (int(v) for v in c.crop)
        cc[i].fit = _fit_id(c.fit)
        cc[i].pad_bgr = (C.c_uint8 * 3)(*[int(v) for v in c.pad])
        cc[i].offline_bgr = (C.c_uint8 * 3)(*[int(v) for v in c.offline])
    return cs, co, cc


def plan_layout(sources, outputs, cells) -> list:
    """The plans of a layout without a GPU (``rtmodt_compose_plan``): the library's own checks, then one ``CellPlan`` per cell."""
    cs, co, cc = _c_layout(sources, outputs, cells)
    out = (_ffi.ComposePlan * max(len(cells), 1))()
    _ffi.check(_ffi.lib().rtmodt_compose_plan(cs, len(sources), co, len(outputs), cc, len(cells), out))
    return [CellPlan(tuple(out[i].crop), tuple(out[i].inner), KINDS[out[i].kind_x], KINDS[out[i].kind_y]) for i in range(len(cells))]


class Compositor(_ffi.Handle):
    """A layout on the device and the runs over it.  ``sources``: ``[(h, w)]``; ``outputs``: ``[Output]``; ``cells``: ``[Cell]`` in
    painting order.  The layout is checked and planned by the library when it is set; a rejected one raises and changes nothing."""

    def __init__(self, sources: Sequence, outputs: Sequence[Output], cells: Sequence[Cell], device=0) -> None:
        self._h = None
        c = _ffi.ComposeCfg()
        _ffi.lib().rtmodt_compose_default_cfg(C.byref(c))
        c.device = _ffi.device_ordinal(device)
        self._device = c.device
        h = C.c_void_p()
        _ffi.check(_ffi.lib().rtmodt_compose_create(C.byref(c), C.byref(h)))
        self._h = h
        self.sources, self.outputs, self.cells, self.plans = [], [], [], []
        self.set_layout(sources, outputs, cells)

    # ---- layouts ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def grid_cells(n: int, out_size, cols: Optional[int] = None, gap: int = 0, fit="fit", output: int = 0, even: bool = False, pad=(0, 0, 0),
                   offline=(0, 0, 0)) -> list:
        """The cells of an ``n``-camera wall on one output: ``cols`` columns (default: ceil(sqrt(n))), ``gap`` pixels between cells and
        to the border; source i in cell i, row-major.  ``even``: rectangles on even coordinates (a 4:2:0 output)."""
        n, gap = int(n), int(gap)
        cols = int(cols) if cols else max(1, math.ceil(math.sqrt(n)))
        rows = (n + cols - 1) // cols
        oh, ow = int(out_size[0]), int(out_size[1])
        cw, ch = (ow - gap * (cols + 1)) // cols, (oh - gap * (rows + 1)) // rows
        if even:
            cw, ch = cw & ~1, ch & ~1
        if n < 1 or cw < 1 or ch < 1:
            raise ValueError(f"{n} cells in {cols} columns with gap {gap} do not fit a {ow}x{oh} output")
        cells = []
        for i in range(n):
            x, y = gap + (i % cols) * (cw + gap), gap + (i // cols) * (ch + gap)
            if even:
                x, y = x + (x & 1), y + (y & 1)
            cells.append(Cell(output, i, (x, y, cw, ch), fit=fit, pad=pad, offline=offline))
        return cells

    @classmethod
    def grid(cls, n: int, src_size, out_size, cols: Optional[int] = None, gap: int = 0, fit="fit", fmt="bgr24", background=(0, 0, 0), device=0):
        """The video wall: ``n`` sources of ``src_size`` in one output of ``out_size``."""
        yuv = _ffi.pixel_format_id(fmt) != _ffi.PIX_BGR24
        return cls([tuple(src_size)] * int(n), [Output(tuple(out_size), fmt, background)], cls.grid_cells(n, out_size, cols, gap, fit, even=yuv), device)

    @classmethod
    def substream(cls, src_size, out_size, fmt="bgr24", fit="stretch", device=0):
        """One source scaled into one output: the low-bitrate preview of a camera."""
        return cls([tuple(src_size)], [Output(tuple(out_size), fmt)], [Cell(0, 0, (0, 0, int(out_size[1]), int(out_size[0])), fit=fit)], device)

    def set_layout(self, sources, outputs, cells) -> None:
        sources, outputs, cells = [tuple(int(v) for v in s) for s in sources], list(outputs), list(cells)
        cs, co, cc = _c_layout(sources, outputs, cells)
        _ffi.check(_ffi.lib().rtmodt_compose_set_layout(self._h, cs, len(sources), co, len(outputs), cc, len(cells)))
        self.sources, self.outputs, self.cells = sources, outputs, cells
        self.plans = plan_layout(sources, outputs, cells)

    def add_inset(self, source: int, crop, rect, output: int = 0, fit="fill", pad=(0, 0, 0), offline=(0, 0, 0)) -> int:
        """A zoomed inset on top of everything painted so far: ``source``'s ``crop`` enlarged into ``rect`` of ``output``.  Returns the
        cell's index (for ``set_crop``: follow-zoom)."""
        self.set_layout(self.sources, self.outputs, self.cells + [Cell(int(output), int(source), tuple(rect), tuple(crop), fit, pad, offline)])
        return len(self.cells) - 1

    def set_crop(self, cell: int, crop) -> None:
        """Re-plans one cell with a new crop (zeros: the whole source); the rest of the layout is left alone."""
        x, y, w, h = (int(v) for v in crop)
        _ffi.check(_ffi.lib().rtmodt_compose_set_crop(self._h, int(cell), x, y, w, h))
        self.cells[cell] = dataclasses.replace(self.cells[cell], crop=(x, y, w, h))
        self.plans = plan_layout(self.sources, self.outputs, self.cells)

    # ---- point mapping ------------------------------------------------------------------------------------------------------
    def map_points(self, cell: int, xy) -> np.ndarray:
        """Source pixel coordinates -> coordinates in the cell's output (float64, from the plan): a pixel's area maps onto its area.
        Points outside the crop land outside the inner picture; nothing is clipped."""
        p = self.plans[cell]
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        (cx, cy, cw, ch), (ix, iy, iw, ih) = p.crop, p.inner
        return np.stack([(xy[:, 0] + 0.5 - cx) * (iw / cw) - 0.5 + ix, (xy[:, 1] + 0.5 - cy) * (ih / ch) - 0.5 + iy], 1)

    def map_boxes(self, cell: int, xyxy) -> np.ndarray:
        """``(n, 4)`` xyxy boxes of the source -> the cell's output: ``FrameRenderer`` then draws the tracks on the wall."""
        b = np.asarray(xyxy, np.float64).reshape(-1, 4)
        return np.concatenate([self.map_points(cell, b[:, :2]), self.map_points(cell, b[:, 2:])], 1)

    # ---- runs ---------------------------------------------------------------------------------------------------------------
    def _host_out(self, i: int, a, fmt):
        o = self.outputs[i]
        h, w = o.size
        pf = _ffi.pixel_format_id(o.fmt)
        if fmt is not None:
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 1 and a.strides[0] == 1 and a.flags.writeable):
                raise ValueError(f"output {i}: with a FrameFormat the destination is a flat writable uint8 buffer")
            if a.nbytes < _ffi.frame_span(fmt, h, w):
                raise ValueError(f"output {i}: the buffer holds {a.nbytes} bytes, the layout spans {_ffi.frame_span(fmt, h, w)}")
            return a.ctypes.data, fmt
        if pf == _ffi.PIX_BGR24:
            hh, ww, pitch = _ffi._host_frames([a], writable=True)
            if (hh, ww) != (h, w):
                raise ValueError(f"output {i}: a {ww}x{hh} array for a {w}x{h} output")
            return a.ctypes.data, _ffi.frame_format(pf, h, w, pitch=pitch)
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (h * 3 // 2, w) and a.strides[1] == 1 and a.strides[0] >= w
                and a.flags.writeable):
            raise ValueError(f"output {i}: a packed 4:2:0 destination is a writable (h * 3 // 2, w) uint8 array with contiguous rows")
        return a.ctypes.data, _ffi.frame_format(pf, h, w, pitch=a.strides[0])

    def run(self, frames, out=None):
        """One run.  ``frames``: one entry per source -- a host array (``(h, w, 3)`` uint8, rows may be padded), a
        ``(DeviceBuffer, offset, pitch)`` triple, or ``None`` for a camera that is down; host and device may not be mixed.
        ``out``: ``None`` -- new host arrays are returned (BGR24: ``(h, w, 3)``; 4:2:0: the packed ``(h * 3 // 2, w)`` array of cv2 /
        ffmpeg); ``"device"`` -- the outputs stay in the compositor's own device buffers and ``[self.output(i)]`` is returned; or a
        list with one entry per output: a host array as above, ``(flat uint8 host buffer, FrameFormat)``, ``(DeviceBuffer, offset,
        FrameFormat or None)`` written in place, or ``None`` for the own buffer.  Returns ``out`` (the new arrays for ``None``)."""
        ns, no = len(self.sources), len(self.outputs)
        frames = list(frames)
        if len(frames) != ns:
            raise ValueError(f"{len(frames)} frames, the layout has {ns} sources")
        dev = [isinstance(f, tuple) for f in frames if f is not None]
        if any(dev) and not all(dev):
            raise ValueError("host and device sources may not be mixed in one run")
        smem = _ffi.MEM_DEVICE if any(dev) else _ffi.MEM_HOST
        sp, pitches, keep = (C.c_void_p * ns)(), (C.c_int32 * ns)(), []
        for i, f in enumerate(frames):
            h, w = self.sources[i]
            if f is None:
                sp[i], pitches[i] = None, 3 * w
            elif smem == _ffi.MEM_DEVICE:
                buf, off, pitch = f
                pitch = 3 * w if pitch is None else int(pitch)
                if off < 0 or pitch < 3 * w or off + (h - 1) * pitch + 3 * w > buf.nbytes:
                    raise ValueError(f"source {i}: a {w}x{h} frame (pitch {pitch}) at offset {off} overruns the {buf.nbytes}-byte buffer")
                sp[i], pitches[i] = buf.ptr + int(off), pitch
            else:
                hh, ww, pitch = _ffi._host_frames([f], writable=False)
                if (hh, ww) != (h, w):
                    raise ValueError(f"source {i}: a {ww}x{hh} frame, the layout says {w}x{h}")
                keep.append(f)
                sp[i], pitches[i] = f.ctypes.data, pitch
        ret = out
        if out is None:
            out = [np.zeros(tuple(o.size) + (3,) if _ffi.pixel_format_id(o.fmt) == _ffi.PIX_BGR24 else (o.size[0] * 3 // 2, o.size[1]), np.uint8)
                   for o in self.outputs]
            ret = out
        elif isinstance(out, str):
            if out != "device":
                raise ValueError(f"out={out!r}: None, 'device' or a list with one entry per output")
            out = [None] * no
        out = list(out)
        if len(out) != no:
            raise ValueError(f"{len(out)} destinations, the layout has {no} outputs")
        ddev = [isinstance(d, tuple) and isinstance(d[0], _ffi.DeviceBuffer) for d in out if d is not None]
        if any(ddev) and not all(ddev):
            raise ValueError("host and device destinations may not be mixed in one run")
        dmem = _ffi.MEM_DEVICE if any(ddev) else _ffi.MEM_HOST
        dp, fmts = (C.c_void_p * no)(), (_ffi.FrameFormat * no)()
        for i, d in enumerate(out):
            o = self.outputs[i]
            fmts[i] = _ffi.FrameFormat(_ffi.pixel_format_id(o.fmt), 0, 0, 0, 0, 0)
            if d is None:
                dp[i] = None
            elif dmem == _ffi.MEM_DEVICE:
                buf, off, fmt = d
                fmt = fmt if fmt is not None else fmts[i]
                if off < 0 or off + _ffi.frame_span(fmt, *o.size) > buf.nbytes:
                    raise ValueError(f"output {i}: the layout at offset {off} overruns the {buf.nbytes}-byte buffer")
                dp[i], fmts[i] = buf.ptr + int(off), fmt
            else:
                a, fmt = d if isinstance(d, tuple) else (d, None)
                dp[i], fmts[i] = self._host_out(i, a, fmt)
        _ffi.check(_ffi.lib().rtmodt_compose_run(self._h, sp, pitches, smem, dp, fmts, dmem))
        if isinstance(ret, str):
            return [self.output(i)[0] for i in range(no)]
        return ret

    def output(self, i: int = 0):
        """``(DeviceBuffer view, pitch)`` of output ``i`` in the compositor's own device buffer: a BGR24 output goes to
        ``FrameRenderer.render_batch`` / ``JpegEncoder.encode_batch`` with ``height``, ``width`` and ``stride=pitch``; a 4:2:0 output's
        chroma follows the Y plane with ``frame_format``'s defaults for that pitch.  Valid until the layout changes."""
        p, pitch = C.c_void_p(), C.c_size_t(0)
        _ffi.check(_ffi.lib().rtmodt_compose_output(self._h, int(i), C.byref(p), C.byref(pitch)))
        o = self.outputs[i]
        rows = o.size[0] if _ffi.pixel_format_id(o.fmt) == _ffi.PIX_BGR24 else o.size[0] * 3 // 2
        return _OutputView(p.value, pitch.value * rows, self._device), pitch.value

    def last_ms(self) -> float:
        """Device time of the last run's launch (HIP events)."""
        return _ffi.last_ms("rtmodt_compose_last_ms", self._h)

    _destroy = "rtmodt_compose_destroy"
