"""Every Python class that owns a library handle, created on a device ordinal that cannot exist: the create fails at ``hipSetDevice``
inside the shared open (``csrc/handle_host.h``), the half-built handle is released, the error text of that first failing call
survives the release, and what is left of the Python object closes, closes again and is collected without a sound.  This needs no
GPU and behaves the same on a machine that has some.  The file and line of the message name the shared header (as they always named
``track_host.h`` for the trackers), so the call's name is matched, not its location."""
import gc

import pytest

NO_DEVICE = 1 << 20


def _reid_weights(pkg, tmp_path):
    path = str(tmp_path / "osnet_synth.rtreid")
    pkg.reid_weights.save(path, pkg.reid_weights.synthetic(0))
    return path


# name -> constructor at the smallest valid arguments; (pkg, tmp_path, device)
CASES = {
    "PrivacyMask": lambda p, t, d: p.PrivacyMask(device=d),
    "FrameRenderer": lambda p, t, d: p.FrameRenderer(device=d),
    "JpegEncoder": lambda p, t, d: p.JpegEncoder(device=d, max_height=16, max_width=16, max_batch=1),
    "JpegDecoder": lambda p, t, d: p.JpegDecoder(device=d, max_height=16, max_width=16, max_batch=1),
    "SnapshotGallery": lambda p, t, d: p.visualization.snapshots.SnapshotGallery((8, 8), max_tracks=1, device=d),
    "CrossingCounter": lambda p, t, d: p.CrossingCounter(device=d, max_tracks=1),
    "SpeedEstimator": lambda p, t, d: p.SpeedEstimator(mm_per_pixel=1.0, device=d, max_tracks=1),
    "IdSwapGuard": lambda p, t, d: p.IdSwapGuard(max_tracks=1, device=d),
    "CameraMotionEstimator": lambda p, t, d: p.CameraMotionEstimator(device=d),
    "ByteTrackCore": lambda p, t, d: p.tracking.tracker._ByteTrackCore(device=d, max_tracks=1, max_dets=1),
    "DeepSortCore": lambda p, t, d: p.tracking.deepsort._DeepSortCore(device=d, max_tracks=1, max_dets=1),
    "OcSortCore": lambda p, t, d: p.tracking.ocsort._OcSortCore(device=d, max_tracks=1, max_dets=1),
    "BotSortCore": lambda p, t, d: p.tracking.botsort._BotSortCore(device=d, max_tracks=1, max_dets=1),
    "Heatmap": lambda p, t, d: p.Heatmap(1, 8, 8, device=d),
    "LensCorrector": lambda p, t, d: p.ingestion.lens.LensCorrector(1, (8, 8), device=d),
    "Stabilizer": lambda p, t, d: p.ingestion.stabilizer.Stabilizer(1, (8, 8), device=d),
    "CameraHealth": lambda p, t, d: p.ingestion.health.CameraHealth(1, 8, 8, device=d),
    "MotionDetector": lambda p, t, d: p.MotionDetector(1, 8, 8, device=d),
    "LeftObjectDetector": lambda p, t, d: p.LeftObjectDetector(1, 8, 8, device=d),
    "ZoneEventEngine": lambda p, t, d: p.ZoneEventEngine([], log_path=str(t / "events.jsonl"), device=d, max_tracks=1),
    "CrossCameraLinker": lambda p, t, d: p.tracking.crosscam.CrossCameraLinker(1, 64, max_tracks=1, max_identities=1, max_queries=1, device=d),
    "ReidEmbedder": lambda p, t, d: p.tracking.reid.ReidEmbedder(_reid_weights(p, t), device=d, max_boxes=1, max_frames=1),
    # opens its device lazily, in the set_layout of its constructor (cp_ensure_device): the handle exists by then and close() releases it
    "Compositor": lambda p, t, d: p.visualization.compose.Compositor([(8, 8)], [p.visualization.compose.Output((8, 8))],
                                                                     [p.visualization.compose.Cell(0, 0, (0, 0, 8, 8))], device=d),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_create_on_a_device_that_cannot_exist(pkg, tmp_path, name):
    E = pkg._ffi.RtmodtError
    shell = None
    with pytest.raises(E) as info:
        try:
            CASES[name](pkg, tmp_path, NO_DEVICE)
        except E as e:
            tb = e.__traceback__
            while tb is not None:                              # the object whose __init__ raised
                me = tb.tb_frame.f_locals.get("self")
                if isinstance(me, pkg._ffi.Handle):
                    shell = me
                tb = tb.tb_next
            raise
    assert info.value.code == pkg._ffi.E_HIP == -3, str(info.value)
    assert "hipSetDevice" in info.value.msg, info.value.msg
    assert shell is not None, "no handle object was under construction"
    assert not getattr(shell, "_h", None) or name == "Compositor"
    shell.close()
    assert shell._h is None
    shell.close()
    del shell, info
    gc.collect()


def test_base_class_closes_once_and_in_order(pkg):
    calls = []

    class Fake(pkg._ffi.Handle):
        _destroy = "rtmodt_version"                            # any symbol: the stand-in below is what gets called

    f = Fake()
    f.close()                                                  # no handle: nothing is looked up
    f._h = 7
    lib = pkg._ffi.lib()
    real = lib.rtmodt_version
    try:
        lib.rtmodt_version = lambda h: calls.append(h)
        f.close()
        f.close()
        f.__del__()
    finally:
        lib.rtmodt_version = real
    assert calls == [7] and f._h is None
