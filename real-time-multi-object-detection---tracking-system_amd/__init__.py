"""MI355X-native detect + track hot path (drop-in for the reference's
``src/detection/detector.py`` and ``src/tracking/tracker.py``).

The directory name is not a Python identifier; import it through the alias
module at the repo root (``import rtmodt_amd``) or with
``importlib.import_module("real-time-multi-object-detection---tracking-system_amd")``.

Sub-modules (imported lazily so that ``synth``/``weights`` work without the HIP
library being built):

* ``detection.detector`` -- ``Detector`` / ``Detections``  (reference: src/detection/detector.py:29-135)
* ``detection.sliced``   -- ``SlicedDetector``: overlapping tiles plus an overview per frame, cut and merged on the GPU (the SAHI
                            scheme; the cure for the design document's "Missed small objects", B.4)
* ``detection.motion``   -- ``MotionDetector``: a background model per stream on the GPU tells still frames from moving ones, so that
                            ``pipeline.run(motion=...)`` keeps the detector off still scenes (the reference drops frames blind to content)
* ``detection.left_objects`` -- ``LeftObjectDetector``: static foreground the detector has no class for (a bag left behind, an exhibit
                            taken away) found, followed in a device-resident ledger and told from standing people by the tracks
* ``tracking.tracker``   --``MultiObjectTracker`` / ``Track`` (reference: src/tracking/tracker.py:27-259)
* ``tracking.deepsort``  -- ``DeepSortTracker``: DeepSORT with appearance matching on the GPU (reference: config/default.yaml:53-60)
* ``tracking.ocsort``    -- ``OcSortTracker``: OC-SORT, the motion-only tracker of the design document's H.2 comparison, on the GPU
* ``tracking.botsort``   -- ``BotSortTracker``: BoT-SORT, the comparison's best row (Re-ID fusion, camera-motion compensation), on the GPU
* ``tracking.gmc``       -- ``CameraMotionEstimator``: the camera-motion warp BoT-SORT compensates with, estimated from the frames on the GPU
* ``tracking.swapguard`` -- ``IdSwapGuard``: ByteTrack identities verified by appearance, ID swaps reverted online on the GPU (the
                            design document's B.4 / G.1 appearance verification, which the reference does not implement)
* ``tracking.reid``      -- ``ReidEmbedder``: the OSNet x0.25 re-identification network on the GPU (reference: config/default.yaml:60)
* ``reid_weights``       -- its ``.rtreid`` weight file, synthetic weights, torchreid ``state_dict`` conversion
* ``_ffi``               -- ctypes binding of ``include/rtmodt.h`` (librtmodt_hip.so)
* ``weights``            -- flat fused-conv weight format, synthetic weights, BN folding
* ``synth``              -- deterministic synthetic frames / box sequences
* ``streams``            -- stream sharding across GPUs + barrier / max-time / stats reduce (RCCL or gloo)
* ``profiling``          -- ``LatencyProfiler`` (reference: src/profiling/latency_profiler.py:35-143)
* ``events``             -- ``ZoneEventEngine`` on device-resident tracks (reference: src/events/zone_engine.py:64-157);
                            ``CrossingCounter``: directional line / gate counts (what config/default.yaml:73-77 promises);
                            ``SpeedEstimator``: track speed, alarms and proximity pairs on a world ground plane;
                            ``ColourAttributes``: the colour names of every track's upper and lower part, for attribute search
* ``pipeline``           -- the reference's per-frame loop (tools/run_pipeline.py:121-158) around the native classes
* ``visualization``      -- ``FrameRenderer``: boxes, labels, trails, zones and HUD drawn into frames on the GPU
                            (reference: src/visualization/renderer.py:28-96); ``JpegEncoder`` / ``MjpegWriter``: the annotated
                            frames as JPEG / Motion-JPEG, encoded on the GPU (reference: tools/run_pipeline.py:112-117,160-161);
                            ``PrivacyMask``: tracked objects and fixed privacy zones filled, pixelated or blurred on the GPU before a
                            frame is recorded or served (the reference has no redaction); ``Heatmap``: occupancy heatmaps
                            accumulated from boxes or device-resident tracks, blended onto frames and summed per zone on the GPU
                            (the reference accumulates nothing over time)
* ``ingestion``          -- ``FrameReader`` / ``RTSPReader``: latest-frame reader thread with pluggable capture back-ends,
                            decoding into a page-locked ring (reference: src/ingestion/rtsp_reader.py:27-158); ``JpegDecoder`` /
                            ``MjpegCapture``: JPEG / Motion-JPEG files, AVI and multipart streams decoded on the GPU; ``Stabilizer``:
                            frames of a shaking camera steadied on the GPU ahead of every fixed-camera stage; ``CameraHealth``:
                            covered, re-aimed, defocused, dark, dazzled and frozen cameras told from healthy ones on the GPU;
                            ``FrameEnhancer``: low-light and low-contrast frames lifted by temporally smoothed CLAHE on the GPU
                            ahead of motion detection and the detector; ``FrameDenoiser``: sensor noise removed by a
                            motion-adaptive temporal and spatial filter on the GPU ahead of the enhancer
* ``evaluation``         -- COCO bbox AP and CLEAR MOT / IDF1 evaluated on the GPU, plus writers of the project's outputs
                            in COCO results / MOTChallenge form (reference: src/evaluation/metrics.py); ``stitch_tracks`` /
                            ``correct_id_switches``: fragmented tracks merged and their gaps filled on the GPU (the design
                            document's B.4 / G.1 / G.2 post-processing step, which the reference does not implement)
"""
import importlib as _importlib

__all__ = ["Detector", "Detections", "SlicedDetector", "MotionDetector", "LeftObjectDetector", "MultiObjectTracker", "Track", "DeepSortTracker", "OcSortTracker", "BotSortTracker"]

_LAZY = {
    "Detector": ".detection.detector",
    "Detections": ".detection.detector",
    "SlicedDetector": ".detection.sliced",
    "MotionDetector": ".detection.motion",
    "MotionResult": ".detection.motion",
    "LeftObjectDetector": ".detection.left_objects",
    "LeftObjectEvent": ".detection.left_objects",
    "LeftObjectResult": ".detection.left_objects",
    "MultiObjectTracker": ".tracking.tracker",
    "Track": ".tracking.tracker",
    "DeepSortTracker": ".tracking.deepsort",
    "OcSortTracker": ".tracking.ocsort",
    "BotSortTracker": ".tracking.botsort",
    "CameraMotionEstimator": ".tracking.gmc",
    "IdSwapGuard": ".tracking.swapguard",
    "SwapEvent": ".tracking.swapguard",
    "ZoneEventEngine": ".events.zone_engine",
    "CrossingCounter": ".events.crossing",
    "SpeedEstimator": ".events.speed",
    "ColourAttributes": ".events.colours",
    "FrameReader": ".ingestion.reader",
    "RTSPReader": ".ingestion.reader",
    "JpegDecoder": ".ingestion.jpeg_decode",
    "MjpegCapture": ".ingestion.mjpeg",
    "FrameEnhancer": ".ingestion.enhance",
    "FrameDenoiser": ".ingestion.denoise",
    "FrameRenderer": ".visualization.renderer",
    "PrivacyMask": ".visualization.privacy",
    "Heatmap": ".visualization.heatmap",
    "JpegEncoder": ".visualization.jpeg",
    "MjpegWriter": ".visualization.jpeg",
    "MjpegRecorder": ".visualization.jpeg",
}


def __getattr__(name):
    if name in _LAZY:
        mod = _importlib.import_module(_LAZY[name], __name__)
        return getattr(mod, name)
    if name in ("synth", "weights", "reid_weights", "_ffi", "detection", "tracking", "yolo_spec", "streams", "profiling", "pipeline", "events", "ingestion",
                "visualization", "evaluation"):
        return _importlib.import_module("." + name, __name__)
    raise AttributeError(name)
