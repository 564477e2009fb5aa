"""CPU: ``_ffi.batch_frames``, the one place that turns "a list of host arrays or a DeviceBuffer" into the frame argument block
``(addresses, height, width, row stride, mem_kind, n)`` of the batched calls.  No GPU: the device branch runs on a stand-in."""
import numpy as np
import pytest


def padded(n, h, w, stride, writeable=True):
    buf = np.zeros((n, h * stride), np.uint8)
    return buf, [np.lib.stride_tricks.as_strided(b, (h, w, 3), (stride, 3, 1), writeable=writeable) for b in buf]


@pytest.fixture
def stand_in(pkg):
    """Makes DeviceBuffers that own nothing: the address is made up, and it is gone again before any of them can be freed, whether the
    test passes or not."""
    made = []

    def make(nbytes, ptr=0x7000_0000):
        d = pkg._ffi.DeviceBuffer.__new__(pkg._ffi.DeviceBuffer)
        d.device, d.nbytes, d.ptr = 0, nbytes, ptr
        made.append(d)
        return d

    yield make
    for d in made:
        d.ptr = None                                        # free() and __del__ see no pointer


def test_host_frames_with_padded_rows(pkg):
    F = pkg._ffi
    buf, views = padded(3, 37, 53, 3 * 53 + 7)
    ptrs, h, w, st, mem, n = F.batch_frames(views)
    assert (h, w, st, mem, n) == (37, 53, 166, F.MEM_HOST, 3)
    assert ptrs == [buf[i].ctypes.data for i in range(3)]
    assert F.batch_frames(views, 3)[5] == 3
    tight = [np.zeros((4, 5, 3), np.uint8)]
    assert F.batch_frames(tight)[1:] == (4, 5, 15, F.MEM_HOST, 1)
    one_row = [np.lib.stride_tricks.as_strided(np.zeros(12, np.uint8), (1, 4, 3), (5, 3, 1))]      # a single row with a meaningless pitch:
    assert F.batch_frames(one_row, writable=False, strict=True)[1:4] == (1, 4, 12)                 # the JPEG encoder reads it as 3w,
    with pytest.raises(ValueError):                                                                # everyone else refuses it
        F.batch_frames(one_row)
    with pytest.raises(ValueError):
        F.frame_pointers(one_row, F.MEM_HOST)
    # frame_pointers (the trackers' form) reads the same geometry through the same check
    fp, keep, h2, w2, st2 = F.frame_pointers(views, F.MEM_HOST)
    assert (h2, w2, st2) == (37, 53, 166) and list(fp) == ptrs and len(keep) == 3


def test_refused_host_frames(pkg):
    F = pkg._ffi
    _, views = padded(2, 8, 6, 24)
    bgra = np.zeros((8, 6, 4), np.uint8)[:, :, :3]                                # pixels 4 bytes apart
    for bad in ([bgra], [views[0], bgra], [np.zeros((8, 6, 3), np.float32)], [np.zeros((8, 6), np.uint8)], [views[0][:, ::-1]], [views[0][::-1]],
                [views[0].transpose(1, 0, 2)], ["frame"]):
        with pytest.raises(ValueError):
            F.batch_frames(bad)
        with pytest.raises(ValueError):
            F.frame_pointers(bad, F.MEM_HOST)
    _, frozen = padded(2, 8, 6, 24, writeable=False)
    with pytest.raises(ValueError):
        F.batch_frames(frozen, writable=True)
    with pytest.raises(ValueError):
        F.batch_frames(frozen)                                                    # writable is the default: most callers draw in place
    assert F.batch_frames(frozen, writable=False)[5] == 2
    # mixed shapes, mixed pitches
    with pytest.raises(ValueError):
        F.batch_frames([views[0], views[1][:7]])
    with pytest.raises(ValueError):
        F.batch_frames([views[0], views[1][:, :5]])
    with pytest.raises(ValueError):
        F.batch_frames([views[0], np.zeros((8, 6, 3), np.uint8)])                 # pitch 24 and pitch 18
    # n mismatch
    with pytest.raises(ValueError):
        F.batch_frames(views, 3)
    with pytest.raises(ValueError):
        F.batch_frames(views, 1)
    # strict (the JPEG codecs): an empty frame is refused here
    with pytest.raises(ValueError):
        F.batch_frames([np.zeros((0, 6, 3), np.uint8)], strict=True)


def test_empty_batch(pkg, stand_in):
    F = pkg._ffi
    assert F.batch_frames([]) == ([], 0, 0, 0, F.MEM_HOST, 0)
    assert F.batch_frames([], 0) == ([], 0, 0, 0, F.MEM_HOST, 0)
    assert F.batch_frames([], 0, strict=True)[5] == 0
    d = stand_in(100)
    assert F.batch_frames(d, 0, height=4, width=5) == ([], 4, 5, 15, F.MEM_DEVICE, 0)
    assert F.batch_frames(d, 0, height=4, width=5, offset=-1)[5] == 0             # no frame, nothing to overrun ...
    with pytest.raises(ValueError):
        F.batch_frames(d, 0, height=4, width=5, offset=-1, strict=True)           # ... except for the codecs, which always refused it


def test_device_buffer_addresses_and_overrun(pkg, stand_in):
    F = pkg._ffi
    h, w, st, n, off = 37, 53, 3 * 53 + 7, 3, 32
    last = off + (n - 1) * h * st + (h - 1) * st + 3 * w                          # one past the last byte of the last row
    d = stand_in(last)
    ptrs, h2, w2, st2, mem, n2 = F.batch_frames(d, n, height=h, width=w, stride=st, offset=off)
    assert (h2, w2, st2, mem, n2) == (h, w, st, F.MEM_DEVICE, n)
    assert ptrs == [d.ptr + off + i * h * st for i in range(n)]
    assert F.batch_frames(d, height=h, width=w, stride=st, offset=off)[5] == n    # n None: the frames that fit behind the offset
    d.nbytes = last - 1                                                           # the last byte is missing
    with pytest.raises(ValueError):
        F.batch_frames(d, n, height=h, width=w, stride=st, offset=off)
    assert F.batch_frames(d, height=h, width=w, stride=st, offset=off)[5] == n - 1
    assert F.batch_frames(d, n - 1, height=h, width=w, stride=st, offset=off)[5] == n - 1
    d.nbytes = last
    with pytest.raises(ValueError):
        F.batch_frames(d, n, height=h, width=w, stride=st, offset=off + 1)        # one byte past the end
    with pytest.raises(ValueError):
        F.batch_frames(d, n, height=h, width=w, stride=st, offset=-1)
    with pytest.raises(ValueError):
        F.batch_frames(d, n, width=w)                                             # device frames need height and width
    assert F.batch_frames(d, 1, height=h, width=w)[3] == 3 * w                    # stride defaults to 3w
    # a stride below 3w or an empty frame: refused here when the frame count has to be derived or with strict, else the library's to refuse
    assert F.batch_frames(d, 1, height=h, width=w, stride=3 * w - 1)[3] == 3 * w - 1
    for kw in (dict(n=1, strict=True), dict(n=None)):
        with pytest.raises(ValueError):
            F.batch_frames(d, height=h, width=w, stride=3 * w - 1, **kw)
        with pytest.raises(ValueError):
            F.batch_frames(d, height=0, width=w, **kw)
