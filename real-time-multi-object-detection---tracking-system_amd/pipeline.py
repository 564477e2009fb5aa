"""The hot loop of the reference's ``tools/run_pipeline.py:121-158`` around the native
detector and tracker: read frame -> ``detector.detect`` ->
``tracker.update`` -> ``profiler.end_frame``, every stage bracketed by the sync-ing
profiler exactly as the reference does.  The zone engine (``event_engine``) and the renderer
(``renderer``, a ``FrameRenderer``) are optional; without them their stages are absent from the table.

On top of the reference's three wall-clock stages (``decode``, ``inference``, ``tracking``)
the loop records what the engine measured with HIP events inside ``inference``:
``preprocess`` (letterbox), ``nms`` and the forward pass itself -- the sub-stages the
reference's ``STAGE_ORDER`` names but its loop never ticks.
"""
from __future__ import annotations

from typing import Iterable, Optional

import numpy as np

from .profiling import LatencyProfiler


class SyntheticSource:
    """Stand-in for ``RTSPReader.read()`` (src/ingestion/rtsp_reader.py:74-79): returns
    ``(ok, frame, frame_id)`` from a pre-generated ring of frames (copied, like the reader)."""

    def __init__(self, frames: np.ndarray):
        self._frames = frames
        self._i = 0

    def read(self):
        f = self._frames[self._i % len(self._frames)].copy()
        self._i += 1
        return True, f, self._i


class PinnedFrameRing:
    """The frame ring between a decoder and the detector: ``slots`` page-locked H x W x 3
    uint8 images (``pixel_format="bgr24"``), or packed ``(H * 3 // 2, W)`` 4:2:0 frames (``"nv12"`` / ``"i420"`` /
    ``"yuv420p"``: half the bytes).  ``write(i, frame)`` is what a capture thread does with a decoded frame; ``frame(i)`` is the
    view handed to ``Detector.enqueue`` -- its upload is then a true asynchronous DMA on the engine's copy stream."""

    def __init__(self, slots: int, height: int, width: int, device=0, *, pixel_format: str = "bgr24"):
        from . import _ffi
        pix = _ffi.pixel_format_id(pixel_format)
        if pix == _ffi.PIX_BGR24:
            shape = (slots, height, width, 3)
        else:
            if height % 2 or width % 2:
                raise ValueError(f"4:2:0 frames need an even width and height, got {width}x{height}")
            shape = (slots, height * 3 // 2, width)
        self._mem = _ffi.PinnedArray(shape, np.uint8, _ffi.device_ordinal(device))
        self.slots = slots
        self.pixel_format = pixel_format

    def write(self, i: int, frame: np.ndarray) -> np.ndarray:
        dst = self._mem.array[i % self.slots]
        np.copyto(dst, frame)
        return dst

    def frame(self, i: int) -> np.ndarray:
        return self._mem.array[i % self.slots]

    def close(self) -> None:
        self._mem.free()


def run(source, detector, tracker, profiler: Optional[LatencyProfiler] = None, max_frames: int = 200,
        device_stages: bool = True, event_engine=None, device_handoff: bool = True, renderer=None, recorder=None,
        crossing_counter=None, swap_guard=None, privacy=None, heatmap=None, motion=None, speed=None, lens=None, snapshots=None, compose=None,
        left_objects=None, stabilize=None, health=None, enhance=None, colours=None, denoise=None) -> dict:
    """Runs ``max_frames`` iterations of the reference loop; returns ``profiler.summary(p50=True)``
    plus the last frame's detections and tracks.

    ``device_handoff`` (default): the tracker consumes the detector's detections where they are, on the device, and the
    zone engine the tracker's device-resident state (``tracker.update_from_detector`` / ``event_engine.process_tracker``);
    the host receives the detections (as the reference's ``Detector._parse`` does) and the events, never the track arrays.
    ``False``: the reference's literal data flow -- ``tracker.update(detections)`` on host arrays, ``process(tracks)``.

    ``renderer``: each frame is annotated in place after the event stage, inside a ``visualization`` stage, as the reference
    does (tools/run_pipeline.py:149-156).  It draws the materialised track list, so the event stage then takes that list too
    (no device-only hand-off of the tracks).

    ``recorder``: ``recorder.write(frame)`` is called with the (annotated) frame after ``profiler.end_frame()``, where the
    reference calls ``video_writer.write(annotated)`` (tools/run_pipeline.py:160-161) -- outside every profiler stage.  A
    ``visualization.MjpegRecorder`` encodes it on the GPU and appends it to an AVI.

    ``crossing_counter``: an ``events.CrossingCounter``, called where the event engine is called, inside a ``crossings`` stage: on
    the tracker's device-resident state when the track list was not materialised (ByteTrack, DeepSORT and OC-SORT alike), else on the list.
    The summary then carries ``crossings``, the number of crossing events of stream 0.

    ``swap_guard``: a ``tracking.IdSwapGuard``, called right after ``tracker.update`` and before events, crossings and rendering,
    inside a ``swap_guard`` stage: it verifies the ByteTrack identities by appearance on the frame the detector read and exchanges
    the ids of a swapped pair back inside the tracker's device-resident state, so every later stage reads the corrected identity
    (a track list that was already materialised has its ids exchanged too).  The summary then carries ``id_swaps_reverted``.

    ``privacy``: a ``visualization.PrivacyMask``, called inside a ``privacy`` stage after the swap guard, the events and the crossings
    and directly before ``visualization``: the masker is the last reader of the clean pixels, and labels and boxes are drawn on top
    of the mask.  It masks the materialised track list when there is one, else the tracker's device-resident tracks (no box crosses
    to the host); the recorder then receives the masked frame.  ``None``: the stage table and every output are unchanged.

    ``heatmap``: a one-stream ``visualization.Heatmap`` of the frames' size, called inside a ``heatmap`` stage after ``privacy`` and
    directly before ``visualization``, so that boxes and labels are drawn over the heat.  Every frame is accumulated -- the
    materialised track list when there is one, else the tracker's device-resident tracks -- and the heat is blended onto the frame
    only if the object's ``overlay_enabled`` is set.  ``None``: the stage table and every output are unchanged.

    ``motion``: a one-stream ``detection.MotionDetector`` of the frames' size, called inside a ``motion`` stage directly after
    ``decode``.  On a frame it calls ``STILL`` the ``inference``, ``tracking`` and ``swap_guard`` stages are skipped -- unless
    ``motion.max_still`` consecutive frames were already skipped (0: never forced), or the detector has not run yet -- and every
    later stage runs on what the last detector frame left: the held detections, the held track list or the tracker's
    device-resident state.  Dwell events keep counting on a person who stands still and the heatmap keeps heating under a parked
    car.  The summary then carries ``motion_frames``, ``still_frames`` and ``scene_changes``, the frames of each status.  ``None``:
    today's loop exactly.

    ``speed``: an ``events.SpeedEstimator`` (fixed camera, one ground plane), called inside a ``speed`` stage directly after
    ``crossings`` -- so after the swap guard: its ledger follows the corrected ids -- with the timestamp
    ``speed.frame_time_us(frame_id)``.  It reads the tracker's device-resident state when the crossings stage would, else the
    materialised list, and runs on the held tracks of a motion-gated still frame (a parked car's STOPPED alarm still fires).  The
    summary then carries ``speed_events``, the number of alarms of stream 0.  ``None``: the stage is absent.

    ``lens``: a one-stream ``ingestion.LensCorrector`` for the frames' size with its lens set, called inside an ``undistort`` stage
    directly after ``decode`` and before ``motion``: the frame is replaced by the rectified one for every later stage and for the
    recorder, so zones, tripwires, privacy polygons and the ground plane are given in rectified coordinates
    (``LensCorrector.undistort_points`` carries them over).  ``None``: the loop, the stage table and the summary are unchanged.

    ``snapshots``: a ``visualization.SnapshotGallery``, called inside a ``snapshots`` stage directly BEFORE ``privacy``: the gallery reads
    the clean pixels, so its thumbnails are not redacted -- a deployment that wants redacted thumbnails leaves this argument out and
    calls the gallery itself after ``privacy``.  Like ``speed`` it reads the tracker's device-resident state when the crossings stage
    would, else the materialised list, and it runs on the held tracks of a motion-gated still frame.  For the device-resident form
    the gallery must be made with at least the tracker's ``max_tracks`` (2048 for a default ``MultiObjectTracker``; the gallery's own
    default is 256): ``process_tracker`` raises ``ValueError`` otherwise.  The summary then carries
    ``snapshots_rewritten`` (thumbnails of existing tracks that a better shot replaced) and ``snapshots_retired`` for stream 0.
    ``None``: the loop, the stage table and the summary are unchanged.

    ``left_objects``: a one-stream ``detection.LeftObjectDetector`` of the frames' size, called inside a ``left_objects`` stage directly
    before ``snapshots`` (else before ``privacy``, else before ``visualization``): after the swap guard, on clean pixels.  It runs on
    every frame, motion-gated still frames included (a left bag IS a still scene), on the held tracks; like ``speed`` it reads the
    tracker's device-resident state when the crossings stage would, else the materialised list.  The summary then carries
    ``left_object_alarms`` and ``left_objects_retired`` for stream 0.  ``None``: the loop, the stage table and the summary are
    unchanged.

    ``compose``: a one-source ``visualization.Compositor`` for the frames' size (``Compositor.substream(...)``, or any layout of one
    source whose output 0 is BGR24), called inside a ``compose`` stage directly after ``visualization``: the annotated frame is
    scaled on the GPU and the recorder receives output 0 -- the sub-stream -- instead of the full frame.  ``None``: the loop, the
    stage table and the summary are unchanged.

    ``stabilize``: a one-stream ``ingestion.Stabilizer`` of the frames' size (with ``gmc=`` it estimates the camera motion from the
    frames themselves; without, the path stays the identity), called inside a ``stabilize`` stage directly after ``undistort`` (else
    directly after ``decode``) and before ``motion``: the frame is replaced by the stabilised one for every later stage and for the
    recorder, so the fixed-camera stages work on a camera that is mounted firmly but not rigidly.  The summary then carries
    ``stabilize_holds``, ``stabilize_clamped`` and ``stabilize_resets``, the frames of each status.  ``None``: the loop, the stage
    table and the summary are unchanged.

    ``health``: a one-stream ``ingestion.CameraHealth`` of the frames' size, called inside a ``health`` stage directly after ``decode``
    and before ``undistort``: it judges the picture the camera delivered -- covered, re-aimed, defocused, dark, dazzled, frozen -- and
    its events carry the source's frame ids.  It gates nothing: what to do with an alarm is the caller's decision.  The summary then
    carries ``health_alarms``, the RAISED events, and ``health_flags``, the OR of the active masks.  ``None``: the loop, the stage
    table and the summary are unchanged.

    ``enhance``: a one-stream ``ingestion.FrameEnhancer`` of the frames' size, called inside an ``enhance`` stage directly before
    ``motion`` and after ``decode``, ``health``, ``undistort`` and ``stabilize`` -- health judges the raw picture and the lens table
    samples unaltered pixels: a dark or flat frame is replaced by the enhanced one for every later stage and for the recorder.  The
    summary then carries ``enhance_mean_eff``, the mean effective strength (0..256) over the frames.  ``None``: the loop, the stage
    table and the summary are unchanged.

    ``denoise``: a one-stream ``ingestion.FrameDenoiser`` of the frames' size, called inside a ``denoise`` stage directly before
    ``enhance`` -- the enhancer should equalise the clean picture, not the noise -- and, without an enhancer, where ``enhance`` would
    stand: directly after the last present of ``stabilize``, ``undistort``, ``health`` and ``decode`` (a temporal filter needs
    registered frames).  The filtered frame goes into a fresh array and replaces the frame for every later stage and for the
    recorder.  The summary then carries ``denoise_mean_noise_q8``, the mean over the frames of the noise figure
    (``DenoiseResult.noise_q8``).  ``None``: the loop, the stage table and the summary are unchanged.

    ``colours``: an ``events.ColourAttributes``, called inside a ``colours`` stage directly before ``left_objects`` (else before
    ``snapshots``, else ``privacy``, else ``visualization``): after the swap guard, so its ledger follows the corrected ids, and on clean
    pixels.  Like ``snapshots`` it reads the tracker's device-resident state when the crossings stage would, else the materialised
    list, and it runs on the held tracks of a motion-gated still frame; for the device-resident form the object must be made with at
    least the tracker's ``max_tracks``.  The summary then carries ``colours_retired``, the rows of stream 0 that left with their final
    label.  ``None``: the loop, the stage table and the summary are unchanged."""
    profiler = profiler or LatencyProfiler(gpu_sync=True, warmup_frames=50, log_interval=100)
    detections = tracks = None
    n_events = n_crossings = n_reverted = 0
    if privacy is not None and "privacy" not in profiler.STAGE_ORDER:          # this profiler's table gains the row (the class's order stays)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("visualization"), "privacy")
        profiler.STAGE_ORDER = order
    if heatmap is not None and "heatmap" not in profiler.STAGE_ORDER:          # likewise, between privacy and visualization
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("visualization"), "heatmap")
        profiler.STAGE_ORDER = order
    if motion is not None and "motion" not in profiler.STAGE_ORDER:            # likewise, directly after decode
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("decode") + 1, "motion")
        profiler.STAGE_ORDER = order
    if speed is not None and "speed" not in profiler.STAGE_ORDER:              # likewise, directly after events (crossings has no row)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("events") + 1, "speed")
        profiler.STAGE_ORDER = order
    if lens is not None and "undistort" not in profiler.STAGE_ORDER:           # likewise, directly after decode (and so before motion)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("decode") + 1, "undistort")
        profiler.STAGE_ORDER = order
    if stabilize is not None and "stabilize" not in profiler.STAGE_ORDER:      # likewise, directly after undistort (else: decode), before motion
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("undistort" if "undistort" in order else "decode") + 1, "stabilize")
        profiler.STAGE_ORDER = order
    if health is not None and "health" not in profiler.STAGE_ORDER:            # likewise, directly after decode, after the three above: before undistort
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("decode") + 1, "health")
        profiler.STAGE_ORDER = order
    if enhance is not None and "enhance" not in profiler.STAGE_ORDER:          # likewise, after the four above and directly before motion
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index(next(k for k in ("stabilize", "undistort", "health", "decode") if k in order)) + 1, "enhance")
        profiler.STAGE_ORDER = order
    if denoise is not None and "denoise" not in profiler.STAGE_ORDER:          # likewise, directly before enhance (else: where enhance would stand)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("enhance") if "enhance" in order else
                     order.index(next(k for k in ("stabilize", "undistort", "health", "decode") if k in order)) + 1, "denoise")
        profiler.STAGE_ORDER = order
    if snapshots is not None and "snapshots" not in profiler.STAGE_ORDER:      # likewise, directly before privacy (else: visualization)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("privacy" if "privacy" in order else "visualization"), "snapshots")
        profiler.STAGE_ORDER = order
    if left_objects is not None and "left_objects" not in profiler.STAGE_ORDER:    # likewise, directly before snapshots (else: privacy, visualization)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index(next(k for k in ("snapshots", "privacy", "visualization") if k in order)), "left_objects")
        profiler.STAGE_ORDER = order
    if colours is not None and "colours" not in profiler.STAGE_ORDER:          # likewise, directly before left_objects (else: snapshots, privacy, visualization)
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index(next(k for k in ("left_objects", "snapshots", "privacy", "visualization") if k in order)), "colours")
        profiler.STAGE_ORDER = order
    if compose is not None and "compose" not in profiler.STAGE_ORDER:          # likewise, directly after visualization
        order = list(profiler.STAGE_ORDER)
        order.insert(order.index("visualization") + 1, "compose")
        profiler.STAGE_ORDER = order
    n_speed = n_snap_rewritten = n_snap_retired = n_left_alarms = n_left_retired = n_colours_retired = 0
    n_status = [0, 0, 0, 0]                                                    # frames per motion status
    n_stab = [0, 0, 0, 0]                                                      # frames per stabiliser status
    still_run = 0                                                              # consecutive frames whose detector pass was skipped
    n_health_alarms = health_flags = 0
    n_enhanced = enhance_eff = 0
    n_denoised = denoise_noise = 0
    for _ in range(max_frames):
        profiler.tick("decode")
        ok, frame, fid = source.read()
        profiler.tock("decode")
        if not ok or frame is None:
            continue
        if health is not None:
            profiler.tick("health")
            verdict = health.process([frame], frame_ids=[int(fid)])[0]
            profiler.tock("health")
            n_health_alarms += sum(1 for e in verdict.events if e.kind == 1)   # 1: RAISED
            health_flags |= verdict.active
        if lens is not None:
            profiler.tick("undistort")
            frame = lens.process([frame])[0]
            profiler.tock("undistort")
        if stabilize is not None:
            profiler.tick("stabilize")
            frame = stabilize.process([frame])[0]
            n_stab[stabilize.result()[0].status] += 1
            profiler.tock("stabilize")
        if denoise is not None:
            profiler.tick("denoise")
            clean = np.empty_like(frame)                                       # (there is no in-place form, and the source's frame is not written)
            denoise_noise += denoise.process([frame], out=[clean])[0].noise_q8
            frame = clean
            n_denoised += 1
            profiler.tock("denoise")
        if enhance is not None:
            profiler.tick("enhance")
            enhanced = np.empty_like(frame)                                    # (the source may hand out a slot of its ring: it is not written)
            enhance_eff += enhance.process([frame], out=[enhanced])[0].eff
            frame = enhanced
            n_enhanced += 1
            profiler.tock("enhance")
        skip = False
        if motion is not None:
            profiler.tick("motion")
            status = motion.process([frame])[0].status
            profiler.tock("motion")
            n_status[status] += 1
            skip = status == 1 and detections is not None and (motion.max_still == 0 or still_run < motion.max_still)      # 1: STILL
            still_run = still_run + 1 if skip else 0
        if not skip:
            profiler.tick("inference")
            detections = detector.detect(frame)
            total_inf = profiler.tock("inference")
            if device_stages and hasattr(detector, "stage_times"):
                pre, fwd, nms = detector.stage_times()
                # split the wall-clock "inference" stage the way the reference's STAGE_ORDER intends:
                # preprocess + inference (forward+decode, host overhead included) + nms == the bracketed time
                profiler.record("preprocess", pre)
                profiler.record("nms", nms)
                profiler.record("inference", max(total_inf - pre - nms, 0.0))
        handoff = device_handoff and hasattr(tracker, "update_from_detector") and hasattr(detector, "model")
        # the track list stays on the device only when the event stage can read it there; an engine with the reference's
        # host API alone (`process(tracks, fid)`) must be handed the materialised list, trails included
        # (and only a ByteTrack handle can be read there: the DeepSORT and OC-SORT trackers hand their tracks over as a list, through
        # process(); OcSortTracker says so with zone_events_on_device = False, DeepSortTracker by asking for the frame)
        needs_frame = bool(getattr(tracker, "needs_frame", False))
        events_on_device = (handoff and not needs_frame and getattr(tracker, "zone_events_on_device", True) and renderer is None and event_engine is not None
                            and hasattr(event_engine, "process_tracker"))
        # the crossing counter reads either tracker's state; alone (no event engine, no renderer) it too leaves the list on the device
        crossings_on_device = events_on_device
        if (crossing_counter is not None or speed is not None or snapshots is not None or left_objects is not None or colours is not None) and event_engine is None and renderer is None and handoff:
            events_on_device = crossings_on_device = True
        if not skip:
            profiler.tick("tracking")
            if needs_frame:                                # a tracker that describes its detections on the frame (DeepSortTracker) or estimates the camera motion from it (BotSortTracker(gmc=))
                tracks = tracker.update_from_detector(detector, frame=frame, materialize=not events_on_device) if handoff else tracker.update(detections, frame=frame)
            else:
                tracks = tracker.update_from_detector(detector, materialize=not events_on_device) if handoff else tracker.update(detections)
            profiler.tock("tracking")
        if swap_guard is not None and not skip:
            profiler.tick("swap_guard")
            reverted = swap_guard.process_tracker(tracker, [frame], fid)[0]
            if reverted and tracks:
                from .tracking.swapguard import adopt
                adopt(tracks, reverted)
            n_reverted += len(reverted)
            profiler.tock("swap_guard")
        if event_engine is not None:                       # tools/run_pipeline.py:141-146
            profiler.tick("events")
            if events_on_device:
                n_events += len(event_engine.process_tracker(tracker, fid, class_names=getattr(detector.model, "names", None))[0])
            else:
                n_events += len(event_engine.process(tracks, fid))
            profiler.tock("events")
        if crossing_counter is not None:
            profiler.tick("crossings")
            if crossings_on_device:
                n_crossings += len(crossing_counter.process_tracker(tracker, fid, class_names=getattr(detector.model, "names", None))[0])
            else:
                n_crossings += len(crossing_counter.process(tracks, fid))
            profiler.tock("crossings")
        if speed is not None:
            profiler.tick("speed")
            if crossings_on_device:
                n_speed += len(speed.process_tracker(tracker, speed.frame_time_us(fid), class_names=getattr(detector.model, "names", None))[0])
            else:
                n_speed += len(speed.process(tracks, speed.frame_time_us(fid)))
            profiler.tock("speed")
        if colours is not None:
            profiler.tick("colours")
            if crossings_on_device:
                _, gone = colours.process_tracker(tracker, [frame], fid)
            else:
                _, gone = colours.process(tracks or [], frame, fid)
            n_colours_retired += len(gone)
            profiler.tock("colours")
        if left_objects is not None:
            profiler.tick("left_objects")
            if crossings_on_device:
                left = left_objects.process([frame], tracker=tracker, frame_id=fid)[0]
            else:
                held = tracks or []
                left = left_objects.process([frame], frame_id=fid, tracks=[([t.track_id for t in held], [t.xyxy for t in held], [t.class_id for t in held])])[0]
            n_left_alarms += len(left.events)
            n_left_retired += len(left.retired)
            profiler.tock("left_objects")
        if snapshots is not None:
            profiler.tick("snapshots")
            if crossings_on_device:
                _, gone = snapshots.process_tracker(tracker, [frame], fid)
            else:
                _, gone = snapshots.process(tracks or [], frame, fid)
            n_snap_rewritten += snapshots.n_rewritten
            n_snap_retired += len(gone)
            profiler.tock("snapshots")
        if privacy is not None:
            profiler.tick("privacy")
            if tracks is None or events_on_device:
                privacy.apply_tracker(tracker, [frame])
            else:
                privacy.apply(frame, tracks)
            profiler.tock("privacy")
        if heatmap is not None:
            profiler.tick("heatmap")
            if tracks is None or events_on_device:
                heatmap.accumulate_tracker(tracker)
            else:
                heatmap.accumulate([tracks])
            if heatmap.overlay_enabled:
                heatmap.overlay([frame])
            profiler.tock("heatmap")
        if renderer is not None:                           # tools/run_pipeline.py:149-156
            profiler.tick("visualization")
            zones = event_engine.get_zone_polygons() if event_engine is not None else None
            renderer.render(frame, tracks, zones=zones, fps=profiler.current_fps,
                            latency_ms=sum(profiler._frame_ms.values()) if profiler._frame_ms else 0)
            profiler.tock("visualization")
        shown = frame
        if compose is not None:
            profiler.tick("compose")
            shown = compose.run([frame])[0]
            profiler.tock("compose")
        profiler.end_frame()
        if recorder is not None:                           # tools/run_pipeline.py:160-161
            recorder.write(shown)
    out = profiler.summary(p50=True)
    out["frames"] = max_frames
    out["last_detections"] = 0 if detections is None else len(detections)
    if device_handoff and hasattr(tracker, "_core") and getattr(tracker, "report", "") == "matched":
        out["last_tracks"] = int((tracker._core.snapshot(0)["tsu"] == 1).sum())      # read back once, after the loop
    else:
        out["last_tracks"] = 0 if tracks is None else len(tracks)
    out["events"] = n_events
    if crossing_counter is not None:
        out["crossings"] = n_crossings
    if speed is not None:
        out["speed_events"] = n_speed
    if snapshots is not None:
        out["snapshots_rewritten"], out["snapshots_retired"] = n_snap_rewritten, n_snap_retired
    if colours is not None:
        out["colours_retired"] = n_colours_retired
    if left_objects is not None:
        out["left_object_alarms"], out["left_objects_retired"] = n_left_alarms, n_left_retired
    if swap_guard is not None:
        out["id_swaps_reverted"] = n_reverted
    if stabilize is not None:
        out["stabilize_holds"], out["stabilize_clamped"], out["stabilize_resets"] = n_stab[1], n_stab[2], n_stab[3]
    if health is not None:
        out["health_alarms"], out["health_flags"] = n_health_alarms, health_flags
    if enhance is not None:
        out["enhance_mean_eff"] = enhance_eff / max(n_enhanced, 1)
    if denoise is not None:
        out["denoise_mean_noise_q8"] = denoise_noise / max(n_denoised, 1)
    if motion is not None:
        out["motion_frames"], out["still_frames"], out["scene_changes"] = n_status[2], n_status[1], n_status[3]
    return out
