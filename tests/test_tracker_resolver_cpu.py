"""``tracking/_common.resolve_tracker`` -- the one place that tells which of the four trackers an object is -- with stand-in objects
(no handle is created, no GPU is touched): for every core and every front end that wraps one, the suffix of the C symbol and the
``report_tsu`` tuple to splice into its arguments; for anything else, every consumer's ``TypeError`` in its own words."""
import types

import pytest

READS = "reads the device-resident state of the ByteTrack, the DeepSORT, the OC-SORT or the BoT-SORT tracker; hand the tracks of a"


def _cores(pkg):
    T = pkg.tracking
    return {"tracker": (T.tracker._ByteTrackCore, T.tracker.MultiObjectTracker), "deepsort": (T.deepsort._DeepSortCore, T.deepsort.DeepSortTracker),
            "ocsort": (T.ocsort._OcSortCore, T.ocsort.OcSortTracker), "botsort": (T.botsort._BotSortCore, T.botsort.BotSortTracker)}


def _blank(cls, **attrs):
    o = object.__new__(cls)                                   # no __init__: no library call
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("suffix", ["tracker", "deepsort", "ocsort", "botsort"])
def test_cores_and_front_ends(pkg, suffix):
    resolve = pkg.tracking._common.resolve_tracker
    core_cls, front_cls = _cores(pkg)[suffix]
    tsu = {"tracker": (1,), "deepsort": (0,), "ocsort": (), "botsort": ()}[suffix]
    core = _blank(core_cls)
    assert resolve(core) == (core, suffix, tsu)
    assert resolve(core, "process_tracker", "as a list: process(tracks, frame_id)") == (core, suffix, tsu)
    front = _blank(front_cls, _core=core)                     # MultiObjectTracker.report defaults to "reference": not "matched"
    assert resolve(front) == (core, suffix, (0,) if suffix == "tracker" else tsu)
    for report, want in (("matched", 1), ("reference", 0)):   # only ByteTrack's front end has a say in what is reported
        front = _blank(front_cls, _core=core, report=report)
        assert resolve(front) == (core, suffix, (want,) if suffix == "tracker" else tsu)
    assert resolve(types.SimpleNamespace(_core=core, report="all"))[1] == suffix


class Stranger:
    n_streams = 1


def test_other_types(pkg):
    resolve = pkg.tracking._common.resolve_tracker
    s = Stranger()
    assert resolve(s) == (s, None, ())
    wrapped = types.SimpleNamespace(_core=s)
    assert resolve(wrapped) == (s, None, ())
    with pytest.raises(TypeError) as e:
        resolve(wrapped, "process_tracker", "as a list: process(tracks, t_us)")
    assert str(e.value) == f"process_tracker {READS} SimpleNamespace over as a list: process(tracks, t_us)"


# (class path, method, call) -> the message, copied from each module as it stood before the resolver
CONSUMERS = [
    ("events.crossing.CrossingCounter", lambda o, t: o.process_tracker(t, 0), f"process_tracker {READS} Stranger over as a list: process(tracks, frame_id)"),
    ("events.speed.SpeedEstimator", lambda o, t: o.process_tracker(t, 0), f"process_tracker {READS} Stranger over as a list: process(tracks, t_us)"),
    ("visualization.privacy.PrivacyMask", lambda o, t: o.apply_tracker(t, []), f"apply_tracker {READS} Stranger over as a list: apply(frame, tracks)"),
    ("visualization.heatmap.Heatmap", lambda o, t: o.accumulate_tracker(t), f"accumulate_tracker {READS} Stranger over as lists: accumulate([tracks])"),
    ("visualization.snapshots.SnapshotGallery", lambda o, t: o.process_tracker(t, [], 0),
     f"process_tracker {READS} Stranger over as a list: process(tracks, frame, frame_id)"),
    ("detection.left_objects.LeftObjectDetector", lambda o, t: o._tracks(1, None, t),
     "tracker: the ByteTrack, the DeepSORT, the OC-SORT or the BoT-SORT tracker (their state is read on the device); hand any other tracker's tracks over as lists"),
    ("tracking.crosscam.CrossCameraLinker", lambda o, t: o.process_tracker(t), "Stranger carries no descriptors on the device; hand its tracks over as lists: process(lists)"),
]


@pytest.mark.parametrize("path,call,message", CONSUMERS, ids=[c[0].rsplit(".", 1)[1] for c in CONSUMERS])
def test_each_consumer_refuses_in_its_own_words(pkg, path, call, message):
    mod = pkg
    for part in path.split("."):
        mod = getattr(mod, part)
    obj = _blank(mod)
    with pytest.raises(TypeError) as e:
        call(obj, Stranger())
    assert str(e.value) == message


def test_crosscam_takes_only_the_trackers_with_descriptors(pkg):
    link = _blank(pkg.tracking.crosscam.CrossCameraLinker)
    for suffix in ("tracker", "ocsort"):
        core = _blank(_cores(pkg)[suffix][0])
        with pytest.raises(TypeError) as e:
            link.process_tracker(core)
        assert str(e.value) == f"{type(core).__name__} carries no descriptors on the device; hand its tracks over as lists: process(lists)"
