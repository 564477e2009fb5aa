"""ctypes binding of ``include/rtmodt.h`` (``lib/librtmodt_hip.so``).

Thin by design: argument marshalling and error translation only.  There is NO CPU
fallback -- if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librtmodt_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "rtmodt.h")

OK, E_INVALID, E_IO, E_HIP, E_CAPACITY, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5
MEM_HOST, MEM_DEVICE = 0, 1
PIX_BGR24, PIX_NV12, PIX_I420 = 0, 1, 2
JPEG_OK, JPEG_UNSUPPORTED, JPEG_CORRUPT, JPEG_TRUNCATED, JPEG_SIZE_MISMATCH = 0, 1, 2, 3, 4
PIXEL_FORMATS = {"bgr24": PIX_BGR24, "nv12": PIX_NV12, "i420": PIX_I420, "yuv420p": PIX_I420}
ASSIGN_GREEDY, ASSIGN_LAPJV = 0, 1
SLICE_MERGE_NMM, SLICE_MERGE_NMS = 0, 1
SLICE_METRIC_IOS, SLICE_METRIC_IOU = 0, 1


class RtmodtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[rtmodt {code}] {msg}")
        self.code = code
        self.msg = msg


class DetCfg(C.Structure):
    _fields_ = [("weight_path", C.c_char_p), ("in_w", C.c_int32), ("in_h", C.c_int32), ("conf", C.c_float),
                ("iou", C.c_float), ("classes", C.POINTER(C.c_int32)), ("n_classes", C.c_int32), ("half", C.c_int32),
                ("device", C.c_int32), ("max_det", C.c_int32), ("agnostic", C.c_int32), ("batch", C.c_int32),
                ("max_src_w", C.c_int32), ("max_src_h", C.c_int32), ("use_graph", C.c_int32), ("autotune", C.c_int32), ("chains", C.c_int32), ("rect", C.c_int32)]


class FrameFormat(C.Structure):                      # struct rtmodt_frame_format
    _fields_ = [("pixel_format", C.c_int32), ("colorspace", C.c_int32), ("pitch", C.c_int32), ("chroma_pitch", C.c_int32),
                ("u_offset", C.c_int64), ("v_offset", C.c_int64)]


def pixel_format_id(name) -> int:
    """``"bgr24" | "nv12" | "i420" | "yuv420p"`` (or an ``RTMODT_PIX_*`` value) -> the ``RTMODT_PIX_*`` value."""
    if isinstance(name, (int, np.integer)) and int(name) in PIXEL_FORMATS.values():
        return int(name)
    key = str(name).lower()
    if key not in PIXEL_FORMATS:
        raise ValueError(f"unknown pixel format {name!r}; one of {sorted(PIXEL_FORMATS)}")
    return PIXEL_FORMATS[key]


def frame_format(pixel_format, h: int, w: int, pitch: int = 0, chroma_pitch: int = 0, u_offset: int = 0, v_offset: int = 0,
                 colorspace: int = 0) -> FrameFormat:
    """A checked ``rtmodt_frame_format`` for ``h x w`` frames: the library's own rules (csrc/engine.hip: resolve_frame_format),
    applied here first so that a bad layout raises ``ValueError`` before any call.  Zeros mean the packed defaults."""
    pf = pixel_format_id(pixel_format)
    fmt = FrameFormat(pf, int(colorspace), int(pitch), int(chroma_pitch), int(u_offset), int(v_offset))
    frame_span(fmt, h, w)
    return fmt


def frame_span(fmt: FrameFormat, h: int, w: int) -> int:
    """Bytes from the frame pointer to the end of the last plane (what one host frame stages); raises ``ValueError`` on a layout the
    library rejects with ``RTMODT_E_INVALID`` and ``NotImplementedError`` on one it rejects with ``RTMODT_E_UNSUPPORTED``."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"bad frame geometry {w}x{h}")
    pf = pixel_format_id(fmt.pixel_format)
    if pf == PIX_BGR24:
        pitch = fmt.pitch or 3 * w
        if pitch < 3 * w:
            raise ValueError(f"BGR pitch {pitch} < {3 * w}")
        return h * pitch
    if fmt.colorspace != 0:
        raise NotImplementedError(f"colorspace {fmt.colorspace}: only 0 (BT.601 limited range) is implemented")
    if h % 2 or w % 2:
        raise ValueError(f"a 4:2:0 frame needs an even width and height, got {w}x{h}")
    nv12 = pf == PIX_NV12
    pitch = fmt.pitch or w
    crow = w if nv12 else w // 2
    cp = fmt.chroma_pitch or (pitch if nv12 else pitch // 2)
    if pitch < w:
        raise ValueError(f"Y pitch {pitch} < width {w}")
    if cp < crow:
        raise ValueError(f"chroma pitch {cp} < {crow} bytes per chroma row")
    uo = fmt.u_offset or pitch * h
    vo = 0 if nv12 else (fmt.v_offset or uo + cp * (h // 2))
    if uo <= 0 or vo < 0:
        raise ValueError(f"negative plane offset (u {uo}, v {vo})")
    planes = [("Y", 0, pitch * (h - 1) + w), ("UV" if nv12 else "U", uo, uo + cp * (h // 2 - 1) + crow)]
    if not nv12:
        planes.append(("V", vo, vo + cp * (h // 2 - 1) + crow))
    for i in range(len(planes)):
        for j in range(i):
            a, b = planes[i], planes[j]
            if not (a[2] <= b[1] or b[2] <= a[1]):
                raise ValueError(f"the {a[0]} plane [{a[1]}, {a[2]}) overlaps the {b[0]} plane [{b[1]}, {b[2]})")
    return max(p[2] for p in planes)


class ZoneCfg(C.Structure):                          # struct rtmodt_zone_cfg
    _fields_ = [("polygon_xy", C.POINTER(C.c_int32)), ("n_points", C.c_int32), ("dwell_time_sec", C.c_double),
                ("cooldown_sec", C.c_double), ("key", C.c_int32)]


class LineCfg(C.Structure):                          # struct rtmodt_line_cfg
    _fields_ = [("ax", C.c_int32), ("ay", C.c_int32), ("bx", C.c_int32), ("by", C.c_int32), ("direction", C.c_int32)]


class GateCfg(C.Structure):                          # struct rtmodt_gate_cfg
    _fields_ = [("polygon_xy", C.POINTER(C.c_int32)), ("n_points", C.c_int32), ("direction", C.c_int32)]


class CrossingEventRec(C.Structure):                 # struct rtmodt_crossing_event
    _fields_ = [("track_id", C.c_int64), ("frames", C.c_int64), ("xyxy", C.c_float * 4), ("centroid", C.c_int32 * 2), ("prev", C.c_int32 * 2),
                ("track", C.c_int32), ("kind", C.c_int32), ("index", C.c_int32), ("direction", C.c_int32), ("cls", C.c_int32),
                ("reserved", C.c_int32)]


class SpeedCfg(C.Structure):                         # struct rtmodt_speed_cfg
    _fields_ = [("anchor", C.c_int32), ("window", C.c_int32), ("min_samples", C.c_int32), ("hold", C.c_int32), ("max_gap_us", C.c_int64),
                ("stop_us", C.c_int64), ("min_step_mm", C.c_int32), ("limit_mm_s", C.c_int32), ("stop_mm_s", C.c_int32),
                ("wrong_way_min_mm_s", C.c_int32), ("allowed_dir", C.c_int32 * 2), ("bins", C.c_int32), ("bin_mm_s", C.c_int32),
                ("proximity_mm", C.c_int32), ("max_pairs", C.c_int32), ("max_events", C.c_int32), ("n_classes", C.c_int32),
                ("classes", C.POINTER(C.c_int32))]


class SpeedRow(C.Structure):                         # struct rtmodt_speed_row
    _fields_ = [("track_id", C.c_int64), ("odometer_mm", C.c_int64), ("track", C.c_int32), ("cls", C.c_int32), ("world", C.c_int32 * 2),
                ("speed_mm_s", C.c_int32), ("peak_mm_s", C.c_int32), ("heading", C.c_int32 * 2), ("flags", C.c_int32), ("n_samples", C.c_int32)]


class SpeedEventRec(C.Structure):                    # struct rtmodt_speed_event
    _fields_ = [("track_id", C.c_int64), ("t_us", C.c_int64), ("xyxy", C.c_float * 4), ("world", C.c_int32 * 2), ("kind", C.c_int32),
                ("value", C.c_int32), ("cls", C.c_int32), ("track", C.c_int32)]


class SpeedPair(C.Structure):                        # struct rtmodt_speed_pair
    _fields_ = [("track_a", C.c_int64), ("track_b", C.c_int64), ("a", C.c_int32), ("b", C.c_int32), ("dist_mm", C.c_int32), ("reserved", C.c_int32)]


class SpeedOut(C.Structure):                         # struct rtmodt_speed_out
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_void_p), ("events", C.c_void_p), ("n_events", C.c_void_p), ("pairs", C.c_void_p),
                ("n_pairs", C.c_void_p), ("total_pairs", C.c_void_p)]


class SnapshotCfg(C.Structure):                      # struct rtmodt_snapshot_cfg
    _fields_ = [("thumb_h", C.c_int32), ("thumb_w", C.c_int32), ("margin_pm", C.c_int32), ("min_side", C.c_int32), ("area_cap", C.c_int32),
                ("occl_iou_pm", C.c_int32), ("min_gain_pm", C.c_int32), ("retire_after", C.c_int32), ("pad_bgr", C.c_uint8 * 4),
                ("max_updated", C.c_int32), ("max_retired", C.c_int32), ("device", C.c_int32), ("n_classes", C.c_int32),
                ("classes", C.POINTER(C.c_int32))]


class SnapshotUpdate(C.Structure):                   # struct rtmodt_snapshot_update
    _fields_ = [("track_id", C.c_int64), ("score", C.c_int64), ("slot", C.c_int32), ("flags", C.c_int32), ("track", C.c_int32), ("reserved", C.c_int32)]


class SnapshotRetired(C.Structure):                  # struct rtmodt_snapshot_retired
    _fields_ = [("track_id", C.c_int64), ("best_frame", C.c_int64), ("first_seen", C.c_int64), ("last_seen", C.c_int64), ("xyxy", C.c_float * 4),
                ("conf", C.c_float), ("slot", C.c_int32), ("cls", C.c_int32), ("n_rewrites", C.c_int32)]


class SnapshotOut(C.Structure):                      # struct rtmodt_snapshot_out
    _fields_ = [("updated", C.c_void_p), ("n_updated", C.c_void_p), ("retired", C.c_void_p), ("n_retired", C.c_void_p), ("n_rewritten", C.c_void_p)]


class SnapshotPlan(C.Structure):                     # struct rtmodt_snapshot_plan_out
    _fields_ = [("sampled", C.c_int32), ("raw", C.c_int32 * 4), ("box", C.c_int32 * 4), ("crop", C.c_int32 * 4), ("sw", C.c_int32), ("sh", C.c_int32),
                ("dw", C.c_int32), ("dh", C.c_int32), ("ox", C.c_int32), ("oy", C.c_int32), ("cut", C.c_int32), ("area", C.c_int32)]


class ColourCfg(C.Structure):                        # struct rtmodt_colour_cfg
    _fields_ = [("black_max", C.c_int32), ("chroma_min", C.c_int32), ("sat_split", C.c_int32), ("sat_hi_pm", C.c_int32), ("sat_lo_pm", C.c_int32),
                ("y_black", C.c_int32), ("y_white", C.c_int32), ("hue", C.c_int32 * 8), ("pink_mx", C.c_int32), ("red_brown_mx", C.c_int32),
                ("orange_brown_mx", C.c_int32), ("yellow_brown_mx", C.c_int32), ("inset_x_pm", C.c_int32), ("top_pm", C.c_int32), ("split_pm", C.c_int32),
                ("bottom_pm", C.c_int32), ("max_side", C.c_int32), ("skip_occluded", C.c_int32), ("min_samples", C.c_int32), ("retire_after", C.c_int32),
                ("device", C.c_int32), ("n_classes", C.c_int32), ("classes", C.POINTER(C.c_int32))]


class ColourLabel(C.Structure):                      # struct rtmodt_colour_label
    _fields_ = [("name", C.c_int32), ("share_pm", C.c_int32), ("second", C.c_int32), ("second_pm", C.c_int32), ("samples", C.c_int32)]


class ColourRow(C.Structure):                        # struct rtmodt_colour_row
    _fields_ = [("track_id", C.c_int64), ("first_frame", C.c_int64), ("last_frame", C.c_int64), ("hist", (C.c_uint32 * 12) * 2), ("cls", C.c_int32),
                ("frames_used", C.c_int32), ("flags", C.c_int32), ("track", C.c_int32), ("frame_samples", C.c_int32), ("reserved", C.c_int32 * 2),
                ("label", ColourLabel * 3)]


class ColourOut(C.Structure):                        # struct rtmodt_colour_out
    _fields_ = [("updated", C.c_void_p), ("n_updated", C.c_void_p), ("retired", C.c_void_p), ("n_retired", C.c_void_p)]


class ColourPlan(C.Structure):                       # struct rtmodt_colour_plan_out
    _fields_ = [("sampled", C.c_int32), ("raw", C.c_int32 * 4), ("box", C.c_int32 * 4), ("rect", C.c_int32 * 4), ("split_row", C.c_int32), ("sx", C.c_int32),
                ("sy", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32)]


class RenderCfg(C.Structure):                        # struct rtmodt_render_cfg
    _fields_ = [("show_boxes", C.c_int32), ("show_ids", C.c_int32), ("show_trails", C.c_int32), ("show_zones", C.c_int32),
                ("show_fps", C.c_int32), ("trail_length", C.c_int32), ("palette_bgr", C.POINTER(C.c_uint8)), ("n_palette", C.c_int32)]


class RenderTrack(C.Structure):                      # struct rtmodt_render_track
    _fields_ = [("track_id", C.c_int64), ("xyxy", C.c_float * 4), ("label", C.c_char_p), ("trail_xy", C.POINTER(C.c_int32)),
                ("n_trail", C.c_int32)]


class RenderList(C.Structure):                       # struct rtmodt_render_list
    _fields_ = [("tracks", C.POINTER(RenderTrack)), ("n_tracks", C.c_int32)]


class JpegCfg(C.Structure):                          # struct rtmodt_jpeg_cfg
    _fields_ = [("quality", C.c_int32), ("subsampling", C.c_int32), ("max_h", C.c_int32), ("max_w", C.c_int32), ("max_batch", C.c_int32)]


class JpegInfo(C.Structure):                         # struct rtmodt_jpeg_info
    _fields_ = [("status", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("components", C.c_int32), ("h_samp", C.c_int32),
                ("v_samp", C.c_int32), ("restart_interval", C.c_int32), ("reserved", C.c_int32), ("message", C.c_char * 96)]


class JpegDecCfg(C.Structure):                       # struct rtmodt_jpegdec_cfg
    _fields_ = [("max_h", C.c_int32), ("max_w", C.c_int32), ("max_batch", C.c_int32), ("max_file_bytes", C.c_int64)]


class DeepSortCfg(C.Structure):                     # struct rtmodt_deepsort_cfg
    _fields_ = [("max_dist", C.c_double), ("min_confidence", C.c_float), ("max_iou_distance", C.c_double), ("max_age", C.c_int32),
                ("n_init", C.c_int32), ("nn_budget", C.c_int32), ("embedder", C.c_char_p), ("dim", C.c_int32), ("max_tracks", C.c_int32),
                ("max_dets", C.c_int32), ("n_streams", C.c_int32), ("device", C.c_int32)]


class OcSortCfg(C.Structure):                       # struct rtmodt_ocsort_cfg
    _fields_ = [("det_thresh", C.c_float), ("low_thresh", C.c_float), ("iou_threshold", C.c_float), ("inertia", C.c_double),
                ("max_age", C.c_int32), ("min_hits", C.c_int32), ("delta_t", C.c_int32), ("use_byte", C.c_int32), ("max_tracks", C.c_int32),
                ("max_dets", C.c_int32), ("n_streams", C.c_int32), ("device", C.c_int32)]


class BotSortCfg(C.Structure):                      # struct rtmodt_botsort_cfg
    _fields_ = [("track_high_thresh", C.c_float), ("track_low_thresh", C.c_float), ("new_track_thresh", C.c_float), ("track_buffer", C.c_int32),
                ("match_thresh", C.c_double), ("proximity_thresh", C.c_double), ("appearance_thresh", C.c_double), ("fuse_score", C.c_int32),
                ("embedder", C.c_char_p), ("dim", C.c_int32), ("max_tracks", C.c_int32), ("max_dets", C.c_int32), ("n_streams", C.c_int32),
                ("device", C.c_int32)]


class GmcCfg(C.Structure):                          # struct rtmodt_gmc_cfg
    _fields_ = [("downscale", C.c_int32), ("coarse_search", C.c_int32), ("search", C.c_int32), ("min_texture", C.c_int32), ("max_sad", C.c_int32),
                ("mask_conf", C.c_float), ("n_hyp", C.c_int32), ("seed", C.c_uint32), ("min_sep", C.c_float), ("inlier_px", C.c_float),
                ("min_blocks", C.c_int32), ("min_inliers", C.c_int32), ("max_boxes", C.c_int32), ("n_streams", C.c_int32), ("device", C.c_int32)]


class ReidCfg(C.Structure):                         # struct rtmodt_reid_cfg
    _fields_ = [("weight_path", C.c_char_p), ("device", C.c_int32), ("max_frames", C.c_int32), ("max_boxes", C.c_int32)]


class MotCounts(C.Structure):                        # struct rtmodt_mot_counts
    _fields_ = [(n, C.c_int64) for n in ("num_frames", "num_objects", "num_predictions", "num_matches", "num_switches", "num_misses",
                                         "num_false_positives", "mostly_tracked", "mostly_lost", "num_unique_objects", "idtp", "idfp",
                                         "idfn")] + [("dist_sum", C.c_double)]


class HotaCounts(C.Structure):                       # struct rtmodt_hota_counts
    _fields_ = [(n, C.c_int64) for n in ("tp", "fn", "fp")] + [(n, C.c_double) for n in ("loc_sum", "ass_a_sum", "ass_re_sum", "ass_pr_sum")]


class ErrorParams(C.Structure):                      # struct rtmodt_error_params
    _fields_ = [("conf_thr", C.c_double), ("iou_fg", C.c_double), ("iou_bg", C.c_double), ("cm_iou", C.c_double), ("max_det", C.c_int32),
                ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("reserved", C.c_int32)]


class StitchParams(C.Structure):                     # struct rtmodt_stitch_params
    _fields_ = [("max_gap", C.c_int32), ("max_dist", C.c_double), ("velocity_window", C.c_int32), ("interpolate", C.c_int32)]


class SwapGuardCfg(C.Structure):                     # struct rtmodt_swapguard_cfg
    _fields_ = [("history", C.c_int32), ("min_history", C.c_int32), ("window", C.c_int32), ("min_similarity_pm", C.c_int32),
                ("min_gain_pm", C.c_int32), ("contact_iou", C.c_float), ("max_gap_frames", C.c_int64), ("max_tracks", C.c_int32),
                ("n_streams", C.c_int32), ("max_events", C.c_int32), ("device", C.c_int32)]


class SliceCfg(C.Structure):                        # struct rtmodt_slice_cfg
    _fields_ = [("device", C.c_int32), ("frame_w", C.c_int32), ("frame_h", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32),
                ("overlap_w", C.c_int32), ("overlap_h", C.c_int32), ("overview", C.c_int32), ("merge", C.c_int32), ("metric", C.c_int32),
                ("match_thresh", C.c_float), ("agnostic", C.c_int32), ("max_out", C.c_int32), ("max_frames", C.c_int32)]


class PrivacyCfg(C.Structure):                      # struct rtmodt_privacy_cfg
    _fields_ = [("mode", C.c_int32), ("fill_bgr", C.c_uint8 * 4), ("cell", C.c_int32), ("radius", C.c_int32), ("passes", C.c_int32),
                ("region", C.c_int32), ("head_pm", C.c_int32), ("expand_px", C.c_int32), ("classes", C.POINTER(C.c_int32)),
                ("n_classes", C.c_int32), ("max_regions", C.c_int32), ("device", C.c_int32)]


class HeatmapCfg(C.Structure):                      # struct rtmodt_heatmap_cfg
    _fields_ = [("n_streams", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("cell", C.c_int32), ("footprint", C.c_int32),
                ("foot_radius", C.c_int32), ("weight", C.c_int32), ("decay_shift", C.c_int32), ("decay_every", C.c_int32),
                ("classes", C.POINTER(C.c_int32)), ("n_classes", C.c_int32), ("device", C.c_int32)]


class MotionCfg(C.Structure):                       # struct rtmodt_motion_cfg
    _fields_ = [(n, C.c_int32) for n in ("streams", "height", "width", "scale", "learn_shift", "learn_shift_fg", "threshold", "dev_gain",
                                         "min_neighbors", "dilate", "warmup", "scene_pm", "min_area", "max_regions", "block", "device")]


class MotionResult(C.Structure):                    # struct rtmodt_motion_result
    _fields_ = [("status", C.c_int32), ("stream", C.c_int32), ("frames_seen", C.c_int32), ("n_raw", C.c_uint32), ("n_fg", C.c_uint32),
                ("n_regions", C.c_int32), ("n_regions_total", C.c_int32), ("bbox", C.c_int32 * 4), ("reserved", C.c_int32),
                ("luma_sum", C.c_uint64)]


class LeftObjCfg(C.Structure):                      # struct rtmodt_leftobj_cfg
    _fields_ = ([(n, C.c_int32) for n in ("streams", "height", "width", "scale", "warmup", "warm_shift", "learn_shift", "threshold", "stable",
                                          "cand_shift", "occlusion", "static_frames", "min_neighbors", "min_area", "max_area", "max_regions",
                                          "scene_pm", "max_objects", "miss_frames", "alarm_frames", "absorb_frames", "covered_pm", "attend_margin",
                                          "max_tracks")] +
                [("n_owner_classes", C.c_int32), ("owner_classes", C.c_int32 * 8), ("n_report_classes", C.c_int32), ("report_classes", C.c_int32 * 8),
                 ("device", C.c_int32)])


class LeftObjResult(C.Structure):                   # struct rtmodt_leftobj_result
    _fields_ = [("status", C.c_int32), ("stream", C.c_int32), ("frames_seen", C.c_int32), ("n_fg", C.c_uint32), ("n_static", C.c_uint32),
                ("n_regions", C.c_int32), ("n_regions_total", C.c_int32), ("n_objects", C.c_int32), ("n_events", C.c_int32),
                ("n_retired", C.c_int32), ("dropped", C.c_int32), ("next_oid", C.c_int32)]


class LeftObjRegion(C.Structure):                   # struct rtmodt_leftobj_region
    _fields_ = [("box", C.c_int32 * 4), ("cells", C.c_int32 * 4), ("area", C.c_int32), ("kind", C.c_int32), ("age_min", C.c_int32),
                ("age_max", C.c_int32), ("covered", C.c_int32), ("attended", C.c_int32), ("oid", C.c_int32), ("root", C.c_int32)]


class LeftObjObject(C.Structure):                   # struct rtmodt_leftobj_object
    _fields_ = [("first_frame", C.c_int64), ("owner", C.c_int64), ("oid", C.c_int32), ("kind", C.c_int32), ("area", C.c_int32), ("idle", C.c_int32),
                ("unmatched", C.c_int32), ("alarmed", C.c_int32), ("cells", C.c_int32 * 4), ("box", C.c_int32 * 4)]


class LeftObjEvent(C.Structure):                    # struct rtmodt_leftobj_event
    _fields_ = [("first_frame", C.c_int64), ("frame_id", C.c_int64), ("owner", C.c_int64), ("oid", C.c_int32), ("kind", C.c_int32),
                ("area", C.c_int32), ("reserved", C.c_int32), ("box", C.c_int32 * 4)]


class LeftObjRetired(C.Structure):                  # struct rtmodt_leftobj_retired
    _fields_ = [("oid", C.c_int32), ("reason", C.c_int32), ("alarmed", C.c_int32), ("reserved", C.c_int32)]


class LeftObjTracks(C.Structure):                   # struct rtmodt_leftobj_tracks
    _fields_ = [("source", C.c_int32), ("stride", C.c_int32), ("ids", C.c_void_p), ("xyxy", C.c_void_p), ("cls", C.c_void_p), ("n", C.c_void_p),
                ("tracker", C.c_void_p), ("report_tsu", C.c_int32), ("reserved", C.c_int32)]


class LeftObjOut(C.Structure):                      # struct rtmodt_leftobj_out
    _fields_ = [("results", C.c_void_p), ("regions", C.c_void_p), ("events", C.c_void_p), ("retired", C.c_void_p), ("objects", C.c_void_p)]


class LensCfg(C.Structure):                         # struct rtmodt_lens_cfg
    _fields_ = [("device", C.c_int32), ("streams", C.c_int32), ("src_h", C.c_int32), ("src_w", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("border_bgr", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class LensParams(C.Structure):                      # struct rtmodt_lens_params
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 8), ("nfx", C.c_double),
                ("nfy", C.c_double), ("ncx", C.c_double), ("ncy", C.c_double), ("r2_limit", C.c_double)]


class StabCfg(C.Structure):                         # struct rtmodt_stab_cfg
    _fields_ = [(k, C.c_int32) for k in ("device", "streams", "h", "w", "leak_shift", "max_shift_px", "max_rot_milli", "max_zoom_milli",
                                         "crop_zoom_milli", "reset_after")] + [("border_bgr", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class StabStreamResult(C.Structure):                # struct rtmodt_stab_stream_result
    _fields_ = [("status", C.c_int32), ("hold", C.c_int32), ("j", C.c_double * 4), ("coef", C.c_int64 * 4)]


class HealthCfg(C.Structure):                       # struct rtmodt_health_cfg
    _fields_ = [(k, C.c_int32) for k in ("streams", "height", "width", "scale", "edge_threshold", "ref_shift", "warmup", "dark_level", "dark_pm",
                                         "bright_level", "bright_pm", "retain_pm", "cover_pm", "defocus_pm", "min_ref_edges", "hold_frames",
                                         "clear_frames", "freeze_frames", "freeze_cells", "relearn_frames", "device")]


class HealthResult(C.Structure):                    # struct rtmodt_health_result
    _fields_ = [("stream", C.c_int32), ("frames_seen", C.c_int32), ("raw", C.c_uint32), ("active", C.c_uint32), ("n_dark", C.c_uint32),
                ("n_bright", C.c_uint32), ("n_changed", C.c_uint32), ("n_edge", C.c_uint32), ("n_ref_edge", C.c_uint32), ("n_kept", C.c_uint32),
                ("n_events", C.c_int32), ("learned", C.c_int32), ("luma_sum", C.c_uint64), ("sharp", C.c_uint64), ("ref_sharp", C.c_uint64)]


class HealthEvent(C.Structure):                     # struct rtmodt_health_event
    _fields_ = [("frame_id", C.c_int64), ("condition", C.c_int32), ("kind", C.c_int32)]


class HealthState(C.Structure):                     # struct rtmodt_health_state
    _fields_ = [("ref_sharp", C.c_uint64), ("frames_seen", C.c_int32), ("active", C.c_uint32), ("pending", C.c_uint32), ("reserved", C.c_int32),
                ("run", C.c_int32 * 6), ("off", C.c_int32 * 6)]


class EnhanceCfg(C.Structure):                      # struct rtmodt_enhance_cfg
    _fields_ = [(k, C.c_int32) for k in ("streams", "height", "width", "tiles_y", "tiles_x", "clip_q8", "strength", "smooth_shift", "auto_lo",
                                         "auto_hi", "colour", "device")]


class EnhanceResult(C.Structure):                   # struct rtmodt_enhance_result
    _fields_ = [("stream", C.c_int32), ("frames_seen", C.c_int32), ("eff", C.c_uint32), ("clipped", C.c_uint32), ("luma_sum", C.c_uint64)]


class DenoiseCfg(C.Structure):                      # struct rtmodt_denoise_cfg
    _fields_ = [(k, C.c_int32) for k in ("streams", "height", "width", "motion_lo", "motion_hi", "temporal_shift", "spatial", "spatial_thr", "device")]


class DenoiseResult(C.Structure):                   # struct rtmodt_denoise_result
    _fields_ = [("stream", C.c_int32), ("frames_seen", C.c_int32), ("n_static", C.c_uint32), ("n_moving", C.c_uint32), ("absdiff_static", C.c_uint64)]


class SwapEventRec(C.Structure):                     # struct rtmodt_swap_event
    _fields_ = [("frame_id", C.c_int64), ("id_a", C.c_int64), ("id_b", C.c_int64), ("track_a", C.c_int32), ("track_b", C.c_int32),
                ("sims", C.c_int32 * 4)]


class CrossCamCfg(C.Structure):                      # struct rtmodt_crosscam_cfg
    _fields_ = [(k, C.c_int32) for k in ("device", "n_streams", "dim", "max_tracks", "max_identities", "max_queries", "min_sim_milli", "max_age",
                                         "bind_age", "match_class")]


class CrossCamEventRec(C.Structure):                 # struct rtmodt_crosscam_event
    _fields_ = [("gid", C.c_int64), ("local_id", C.c_int64), ("stream", C.c_int32), ("from_stream", C.c_int32), ("gap", C.c_int32), ("sim", C.c_int32)]


class CrossCamRetiredRec(C.Structure):               # struct rtmodt_crosscam_retired
    _fields_ = [("gid", C.c_int64), ("first_seen", C.c_int64), ("last_seen", C.c_int64), ("stream_mask", C.c_uint64)]


class CrossCamOut(C.Structure):                      # struct rtmodt_crosscam_out
    _fields_ = [("gid", C.c_void_p), ("status", C.c_void_p), ("sim", C.c_void_p), ("events", C.c_void_p), ("n_events", C.POINTER(C.c_int32)),
                ("retired", C.c_void_p), ("n_retired", C.POINTER(C.c_int32)), ("counters", C.c_void_p)]


class IndexCfg(C.Structure):                         # struct rtmodt_index_cfg
    _fields_ = [(k, C.c_int32) for k in ("device", "dim", "capacity", "max_queries", "max_k", "max_add", "chunk_rows")]


class IndexFilter(C.Structure):                      # struct rtmodt_index_filter
    _fields_ = [("t0", C.c_int64), ("t1", C.c_int64), ("stream_mask", C.c_uint64), ("exclude_key", C.c_int64), ("cls", C.c_int32), ("min_ppm", C.c_int32)]


class IndexHit(C.Structure):                         # struct rtmodt_index_hit
    _fields_ = [("rid", C.c_int64), ("key", C.c_int64), ("t", C.c_int64), ("stream", C.c_int32), ("cls", C.c_int32), ("ppm", C.c_int32),
                ("reserved", C.c_int32)]


class ComposeCfg(C.Structure):                      # struct rtmodt_compose_cfg
    _fields_ = [(k, C.c_int32) for k in ("device", "max_sources", "max_outputs", "max_cells", "max_dim")]


class ComposeSource(C.Structure):                   # struct rtmodt_compose_src_desc
    _fields_ = [("h", C.c_int32), ("w", C.c_int32)]


class ComposeOutput(C.Structure):                   # struct rtmodt_compose_out_desc
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("pixel_format", C.c_int32), ("background_bgr", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class ComposeCell(C.Structure):                     # struct rtmodt_compose_cell
    _fields_ = [("output", C.c_int32), ("source", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32), ("fit", C.c_int32),
                ("pad_bgr", C.c_uint8 * 3), ("reserved0", C.c_uint8), ("offline_bgr", C.c_uint8 * 3), ("reserved1", C.c_uint8)]


class ComposePlan(C.Structure):                     # struct rtmodt_compose_plan_out
    _fields_ = [("crop", C.c_int32 * 4), ("inner", C.c_int32 * 4), ("kind_x", C.c_int32), ("kind_y", C.c_int32)]


_lib = None


def header_symbols() -> list[str]:
    """Every function name ``include/rtmodt.h`` declares."""
    txt = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"\b(rtmodt_[a-z0-9_]+)\s*\(", txt)))


def lib() -> C.CDLL:
    """Loads the library (once).  Raises ``RtmodtError`` if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtmodtError(E_IO, f"{LIB_PATH} not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, i64 = C.c_void_p, C.c_int32, C.c_float, C.c_int64
    sig = {
        "rtmodt_last_error": (C.c_char_p, []),
        "rtmodt_version": (C.c_char_p, []),
        "rtmodt_build_info": (C.c_char_p, []),
        "rtmodt_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p)]),
        "rtmodt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "rtmodt_synchronize": (C.c_int, [C.c_int]),
        "rtmodt_device_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(vp)]),
        "rtmodt_device_free": (C.c_int, [C.c_int, vp]),
        "rtmodt_host_alloc": (C.c_int, [C.c_int, C.c_size_t, C.POINTER(vp)]),
        "rtmodt_host_free": (C.c_int, [C.c_int, vp]),
        "rtmodt_memcpy_h2d": (C.c_int, [C.c_int, vp, vp, C.c_size_t]),
        "rtmodt_memcpy_d2h": (C.c_int, [C.c_int, vp, vp, C.c_size_t]),
        "rtmodt_detector_create": (C.c_int, [C.POINTER(DetCfg), C.POINTER(vp)]),
        "rtmodt_detector_destroy": (None, [vp]),
        "rtmodt_detector_detect": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
        "rtmodt_detector_detect_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
        "rtmodt_detector_enqueue_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_detector_fetch": (C.c_int, [vp, vp, vp, vp, vp]),
        "rtmodt_detector_enqueue_batch_fmt": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(FrameFormat), C.c_int]),
        "rtmodt_detector_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                           C.POINTER(i64), C.POINTER(i64)]),
        "rtmodt_detector_chains": (C.c_int, [vp, C.POINTER(i32)]),
        "rtmodt_detector_stages": (C.c_int, [vp, C.POINTER(i32)]),
        "rtmodt_detector_debug_fetch": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "rtmodt_detector_debug_layer": (C.c_int, [vp, C.c_char_p, C.c_int, vp, C.POINTER(i32)]),
        "rtmodt_detector_profile": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(f32),
                                              C.POINTER(i64), C.POINTER(i32)]),
        "rtmodt_detector_last_timing": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_detector_stage_times": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_detector_clock_enable": (C.c_int, [vp, C.c_int]),
        "rtmodt_detector_clock_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
        "rtmodt_nms_pred": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, f32, f32, vp, C.c_int, C.c_int, C.c_int,
                                      vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_preprocess": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "rtmodt_preprocess_yuv420": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.POINTER(FrameFormat), C.c_int, C.c_int, vp]),
        "rtmodt_tracker_create": (C.c_int, [C.c_int, f32, C.c_int, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "rtmodt_tracker_destroy": (None, [vp]),
        "rtmodt_tracker_set_cost_limit": (C.c_int, [vp, C.c_double]),
        "rtmodt_tracker_update": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(i32)]),
        "rtmodt_tracker_update_batch": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "rtmodt_tracker_update_from_detector": (C.c_int, [vp, vp]),
        "rtmodt_tracker_update_from_detector_frames": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "rtmodt_tracker_update_from_detector_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]),
        "rtmodt_tracker_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i64)]),
        "rtmodt_tracker_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_tracker_enable_kalman": (C.c_int, [vp]),
        "rtmodt_tracker_kalman_state": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(i32)]),
        "rtmodt_iou_matrix": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, vp]),
        "rtmodt_assign_greedy": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, f32, vp, vp]),
        "rtmodt_assign_lapjv": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_double, vp, vp]),
        "rtmodt_deepsort_create": (C.c_int, [C.POINTER(DeepSortCfg), C.POINTER(vp)]),
        "rtmodt_deepsort_destroy": (None, [vp]),
        "rtmodt_deepsort_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_appearance_describe": (C.c_int, [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
        "rtmodt_appearance_quantize": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "rtmodt_appearance_dotmax": (C.c_int, [C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
        "rtmodt_deepsort_update_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "rtmodt_deepsort_update_from_detector": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_deepsort_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i64)]),
        "rtmodt_deepsort_last_ms": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_ocsort_create": (C.c_int, [C.POINTER(OcSortCfg), C.POINTER(vp)]),
        "rtmodt_ocsort_destroy": (None, [vp]),
        "rtmodt_ocsort_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_ocsort_update_batch": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "rtmodt_ocsort_update_from_detector": (C.c_int, [vp, vp]),
        "rtmodt_ocsort_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]),
        "rtmodt_ocsort_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_botsort_create": (C.c_int, [C.POINTER(BotSortCfg), C.POINTER(vp)]),
        "rtmodt_botsort_destroy": (None, [vp]),
        "rtmodt_botsort_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_botsort_check_warp": (C.c_int, [vp, C.c_int]),
        "rtmodt_botsort_update_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "rtmodt_botsort_update_from_detector": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "rtmodt_botsort_state": (C.c_int, [vp, C.c_int] + [vp] * 13 + [C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]),
        "rtmodt_botsort_last_ms": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_botsort_update_from_detector_gmc": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_gmc_default_cfg": (None, [C.POINTER(GmcCfg)]),
        "rtmodt_gmc_create": (C.c_int, [C.POINTER(GmcCfg), C.POINTER(vp)]),
        "rtmodt_gmc_destroy": (None, [vp]),
        "rtmodt_gmc_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_gmc_estimate_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
        "rtmodt_gmc_estimate_from_detector": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_gmc_result": (C.c_int, [vp, vp, vp]),
        "rtmodt_gmc_debug": (C.c_int, [vp, C.c_int] + [vp] * 12),
        "rtmodt_gmc_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_reid_create": (C.c_int, [C.POINTER(ReidCfg), C.POINTER(vp)]),
        "rtmodt_reid_destroy": (None, [vp]),
        "rtmodt_reid_embed": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
        "rtmodt_reid_tap": (C.c_int, [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "rtmodt_reid_last_ms": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_reid_norm_table": (C.c_int, [vp, C.c_size_t]),
        "rtmodt_zones_create": (C.c_int, [C.c_int, C.POINTER(ZoneCfg), C.c_int, C.c_int, C.c_int, C.c_int, i64, C.POINTER(vp)]),
        "rtmodt_zones_destroy": (None, [vp]),
        "rtmodt_zones_process": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, C.c_double, i64, vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_zones_process_tracker": (C.c_int, [vp, vp, C.c_double, i64, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
        "rtmodt_zones_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_crossing_create": (C.c_int, [C.c_int, C.POINTER(LineCfg), C.c_int, C.POINTER(GateCfg), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             i64, C.POINTER(vp)]),
        "rtmodt_crossing_destroy": (None, [vp]),
        "rtmodt_crossing_process": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, i64, vp, C.POINTER(i32)]),
        "rtmodt_crossing_process_tracker": (C.c_int, [vp, vp, i64, C.c_int, vp, vp]),
        "rtmodt_crossing_process_deepsort": (C.c_int, [vp, vp, i64, C.c_int, vp, vp]),
        "rtmodt_crossing_process_ocsort": (C.c_int, [vp, vp, i64, vp, vp]),
        "rtmodt_crossing_process_botsort": (C.c_int, [vp, vp, i64, vp, vp]),
        "rtmodt_crossing_counts": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "rtmodt_crossing_reset_counts": (C.c_int, [vp]),
        "rtmodt_crossing_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_speed_create": (C.c_int, [C.c_int, C.POINTER(SpeedCfg), C.c_int, C.c_int, C.POINTER(vp)]),
        "rtmodt_speed_destroy": (None, [vp]),
        "rtmodt_speed_set_plane": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_speed_set_scale": (C.c_int, [vp, C.c_int, C.c_double]),
        "rtmodt_speed_fit_plane": (C.c_int, [vp, vp, C.c_int, vp, C.POINTER(C.c_double)]),
        "rtmodt_speed_process": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, i64, C.POINTER(SpeedOut)]),
        "rtmodt_speed_process_batch": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(SpeedOut)]),
        "rtmodt_speed_process_tracker": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(SpeedOut)]),
        "rtmodt_speed_process_deepsort": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(SpeedOut)]),
        "rtmodt_speed_process_ocsort": (C.c_int, [vp, vp, vp, C.POINTER(SpeedOut)]),
        "rtmodt_speed_process_botsort": (C.c_int, [vp, vp, vp, C.POINTER(SpeedOut)]),
        "rtmodt_speed_histogram": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "rtmodt_speed_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_swapguard_create": (C.c_int, [C.POINTER(SwapGuardCfg), C.POINTER(vp)]),
        "rtmodt_swapguard_destroy": (None, [vp]),
        "rtmodt_swapguard_process": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, vp, vp, C.POINTER(i32)]),
        "rtmodt_swapguard_process_tracker": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, C.c_int, vp, vp]),
        "rtmodt_swapguard_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_swapguard_counts": (C.c_int, [vp, C.c_int, C.POINTER(i64)]),
        "rtmodt_swapguard_last_ms": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_slice_grid": (C.c_int, [C.c_int] * 6 + [vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "rtmodt_slicer_create": (C.c_int, [C.POINTER(SliceCfg), C.c_int, C.POINTER(vp)]),
        "rtmodt_slicer_destroy": (None, [vp]),
        "rtmodt_slicer_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "rtmodt_slicer_gather": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "rtmodt_slice_merge": (C.c_int, [C.c_int, C.POINTER(SliceCfg), C.c_int, C.c_int] + [vp] * 9 + [C.POINTER(f32)]),
        "rtmodt_slicer_enqueue": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int]),
        "rtmodt_slicer_fetch": (C.c_int, [vp, vp] + [vp] * 9),
        "rtmodt_slicer_last_ms": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_tracker_update_from_slicer": (C.c_int, [vp, vp]),
        "rtmodt_privacy_default_cfg": (None, [C.POINTER(PrivacyCfg)]),
        "rtmodt_privacy_create": (C.c_int, [C.POINTER(PrivacyCfg), C.POINTER(vp)]),
        "rtmodt_privacy_destroy": (None, [vp]),
        "rtmodt_privacy_set_polygons": (C.c_int, [vp, vp, vp, C.c_int]),
        "rtmodt_privacy_regions": (C.c_int, [C.POINTER(PrivacyCfg), vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(i32)]),
        "rtmodt_privacy_apply": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "rtmodt_privacy_apply_tracker": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_privacy_apply_deepsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_privacy_apply_ocsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_privacy_apply_botsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_privacy_apply_detector": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_privacy_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_heatmap_default_cfg": (None, [C.POINTER(HeatmapCfg)]),
        "rtmodt_heatmap_create": (C.c_int, [C.POINTER(HeatmapCfg), C.POINTER(vp)]),
        "rtmodt_heatmap_destroy": (None, [vp]),
        "rtmodt_heatmap_footprint": (C.c_int, [C.POINTER(HeatmapCfg), vp, i32, vp, C.c_int, C.POINTER(i32)]),
        "rtmodt_heatmap_accumulate": (C.c_int, [vp, vp, vp, vp]),
        "rtmodt_heatmap_accumulate_tracker": (C.c_int, [vp, vp, C.c_int]),
        "rtmodt_heatmap_accumulate_deepsort": (C.c_int, [vp, vp, C.c_int]),
        "rtmodt_heatmap_accumulate_ocsort": (C.c_int, [vp, vp]),
        "rtmodt_heatmap_accumulate_botsort": (C.c_int, [vp, vp]),
        "rtmodt_heatmap_accumulate_detector": (C.c_int, [vp, vp]),
        "rtmodt_heatmap_overlay": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]),
        "rtmodt_heatmap_set_colormap": (C.c_int, [vp, vp]),
        "rtmodt_heatmap_zone_sums": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp]),
        "rtmodt_heatmap_read": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_heatmap_load": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_heatmap_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_heatmap_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_motion_default_cfg": (None, [C.POINTER(MotionCfg)]),
        "rtmodt_motion_create": (C.c_int, [C.POINTER(MotionCfg), C.POINTER(vp)]),
        "rtmodt_motion_destroy": (None, [vp]),
        "rtmodt_motion_process": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "rtmodt_motion_read_mask": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_motion_read_blocks": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_motion_read_state": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(i32)]),
        "rtmodt_motion_load_state": (C.c_int, [vp, C.c_int, vp, vp, i32]),
        "rtmodt_motion_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_motion_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_motion_cell": (C.c_int, [C.POINTER(MotionCfg), C.c_uint32, i32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(i32)]),
        "rtmodt_leftobj_default_cfg": (None, [C.POINTER(LeftObjCfg)]),
        "rtmodt_leftobj_create": (C.c_int, [C.POINTER(LeftObjCfg), C.POINTER(vp)]),
        "rtmodt_leftobj_destroy": (None, [vp]),
        "rtmodt_leftobj_process": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LeftObjTracks), C.POINTER(LeftObjOut)]),
        "rtmodt_leftobj_read_state": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(i32)]),
        "rtmodt_leftobj_load_state": (C.c_int, [vp, C.c_int, vp, vp, i32]),
        "rtmodt_leftobj_read_mask": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_leftobj_load_mask": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_leftobj_read_ledger": (C.c_int, [vp, C.c_int, vp, C.POINTER(i32), C.POINTER(i32)]),
        "rtmodt_leftobj_load_ledger": (C.c_int, [vp, C.c_int, vp, C.c_int, i32]),
        "rtmodt_leftobj_set_ignore": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_leftobj_read_ignore": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_leftobj_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_leftobj_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_leftobj_cell": (C.c_int, [C.POINTER(LeftObjCfg), C.c_uint32, i32, C.POINTER(C.c_uint64), C.POINTER(i32), C.POINTER(i32)]),
        "rtmodt_lens_default_cfg": (None, [C.POINTER(LensCfg)]),
        "rtmodt_lens_create": (C.c_int, [C.POINTER(LensCfg), C.POINTER(vp)]),
        "rtmodt_lens_destroy": (None, [vp]),
        "rtmodt_lens_set_model": (C.c_int, [vp, C.c_int, C.POINTER(LensParams), C.POINTER(i32)]),
        "rtmodt_lens_set_map": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(i32)]),
        "rtmodt_lens_read_map": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "rtmodt_lens_process": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int]),
        "rtmodt_lens_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_lens_distort_points": (C.c_int, [C.POINTER(LensParams), vp, C.c_int, vp, vp]),
        "rtmodt_lens_undistort_points": (C.c_int, [C.POINTER(LensParams), vp, C.c_int, vp, vp]),
        "rtmodt_lens_build_map": (C.c_int, [C.POINTER(LensParams), C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "rtmodt_lens_quantise_map": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "rtmodt_stab_default_cfg": (None, [C.POINTER(StabCfg)]),
        "rtmodt_stab_create": (C.c_int, [C.POINTER(StabCfg), C.POINTER(vp)]),
        "rtmodt_stab_destroy": (None, [vp]),
        "rtmodt_stab_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_stab_process": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
        "rtmodt_stab_process_gmc": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]),
        "rtmodt_stab_result": (C.c_int, [vp, C.POINTER(StabStreamResult)]),
        "rtmodt_stab_state": (C.c_int, [vp, C.c_int, vp, C.POINTER(i32)]),
        "rtmodt_stab_load_state": (C.c_int, [vp, C.c_int, vp, i32]),
        "rtmodt_stab_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_stab_points": (C.c_int, [C.POINTER(StabCfg), vp, C.c_int, vp, C.c_int, vp]),
        "rtmodt_stab_step": (C.c_int, [C.POINTER(StabCfg), vp, C.POINTER(i32), vp, C.c_int, C.POINTER(i32), vp]),
        "rtmodt_health_default_cfg": (None, [C.POINTER(HealthCfg)]),
        "rtmodt_health_create": (C.c_int, [C.POINTER(HealthCfg), C.POINTER(vp)]),
        "rtmodt_health_destroy": (None, [vp]),
        "rtmodt_health_process": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "rtmodt_health_read_state": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(HealthState)]),
        "rtmodt_health_load_state": (C.c_int, [vp, C.c_int, vp, vp, C.POINTER(HealthState)]),
        "rtmodt_health_rebase": (C.c_int, [vp, C.c_int]),
        "rtmodt_health_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_health_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_health_decide": (C.c_int, [C.POINTER(HealthCfg), i64, i64, C.POINTER(HealthResult), C.POINTER(HealthState), vp]),
        "rtmodt_enhance_default_cfg": (None, [C.POINTER(EnhanceCfg)]),
        "rtmodt_enhance_create": (C.c_int, [C.POINTER(EnhanceCfg), C.POINTER(vp)]),
        "rtmodt_enhance_destroy": (None, [vp]),
        "rtmodt_enhance_process": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
        "rtmodt_enhance_read_state": (C.c_int, [vp, C.c_int, vp, C.POINTER(i32)]),
        "rtmodt_enhance_load_state": (C.c_int, [vp, C.c_int, vp, i64, i32]),
        "rtmodt_enhance_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_enhance_histograms": (C.c_int, [vp, C.c_int, vp]),
        "rtmodt_enhance_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_enhance_curve": (C.c_int, [vp, i64, i32, vp, C.POINTER(C.c_uint32)]),
        "rtmodt_enhance_axis": (C.c_int, [i32, i32, vp, vp, vp]),
        "rtmodt_denoise_default_cfg": (None, [C.POINTER(DenoiseCfg)]),
        "rtmodt_denoise_create": (C.c_int, [C.POINTER(DenoiseCfg), C.POINTER(vp)]),
        "rtmodt_denoise_destroy": (None, [vp]),
        "rtmodt_denoise_process": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
        "rtmodt_denoise_read_state": (C.c_int, [vp, C.c_int, vp, C.POINTER(i32)]),
        "rtmodt_denoise_load_state": (C.c_int, [vp, C.c_int, vp, i64, i32]),
        "rtmodt_denoise_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_denoise_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_denoise_pixel": (C.c_int, [C.POINTER(DenoiseCfg), vp, vp, C.c_uint32, i32, vp, vp, C.POINTER(i32), C.POINTER(i32)]),
        "rtmodt_snapshot_default_cfg": (None, [C.POINTER(SnapshotCfg)]),
        "rtmodt_snapshot_create": (C.c_int, [C.POINTER(SnapshotCfg), C.c_int, C.c_int, C.POINTER(vp)]),
        "rtmodt_snapshot_destroy": (None, [vp]),
        "rtmodt_snapshot_process": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, C.POINTER(SnapshotOut)]),
        "rtmodt_snapshot_process_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(SnapshotOut)]),
        "rtmodt_snapshot_process_tracker": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(SnapshotOut)]),
        "rtmodt_snapshot_process_deepsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(SnapshotOut)]),
        "rtmodt_snapshot_process_ocsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(SnapshotOut)]),
        "rtmodt_snapshot_process_botsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(SnapshotOut)]),
        "rtmodt_snapshot_atlas": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(i32)]),
        "rtmodt_snapshot_read": (C.c_int, [vp, C.c_int, vp, C.c_int, vp]),
        "rtmodt_snapshot_state": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]),
        "rtmodt_snapshot_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_snapshot_plan": (C.c_int, [C.POINTER(SnapshotCfg), vp, C.c_int, C.c_int, C.POINTER(SnapshotPlan)]),
        "rtmodt_snapshot_crop": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]),
        "rtmodt_snapshot_crop_detector": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, C.c_int, vp, vp, vp]),
        "rtmodt_snapshot_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_colour_default_cfg": (None, [C.POINTER(ColourCfg)]),
        "rtmodt_colour_create": (C.c_int, [C.POINTER(ColourCfg), C.c_int, C.c_int, C.POINTER(vp)]),
        "rtmodt_colour_destroy": (None, [vp]),
        "rtmodt_colour_process": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, i64, C.POINTER(ColourOut)]),
        "rtmodt_colour_process_batch": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(ColourOut)]),
        "rtmodt_colour_process_tracker": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(ColourOut)]),
        "rtmodt_colour_process_deepsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(ColourOut)]),
        "rtmodt_colour_process_ocsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(ColourOut)]),
        "rtmodt_colour_process_botsort": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(ColourOut)]),
        "rtmodt_colour_state": (C.c_int, [vp, C.c_int, vp, C.POINTER(i32)]),
        "rtmodt_colour_load": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "rtmodt_colour_reset": (C.c_int, [vp, C.c_int]),
        "rtmodt_colour_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_colour_name": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(ColourCfg)]),
        "rtmodt_colour_plan": (C.c_int, [C.POINTER(ColourCfg), vp, C.c_int, C.c_int, C.POINTER(ColourPlan)]),
        "rtmodt_crosscam_default_cfg": (None, [C.POINTER(CrossCamCfg)]),
        "rtmodt_crosscam_create": (C.c_int, [C.POINTER(CrossCamCfg), C.POINTER(vp)]),
        "rtmodt_crosscam_destroy": (None, [vp]),
        "rtmodt_crosscam_set_transit": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_crosscam_process": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.POINTER(CrossCamOut)]),
        "rtmodt_crosscam_process_botsort": (C.c_int, [vp, vp, C.POINTER(CrossCamOut)]),
        "rtmodt_crosscam_process_deepsort": (C.c_int, [vp, vp, C.POINTER(CrossCamOut)]),
        "rtmodt_crosscam_state": (C.c_int, [vp] * 12),
        "rtmodt_crosscam_load": (C.c_int, [vp] * 12),
        "rtmodt_crosscam_errors": (C.c_int, [vp, vp]),
        "rtmodt_crosscam_clear_errors": (C.c_int, [vp]),
        "rtmodt_crosscam_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_crosscam_similarity": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp]),
        "rtmodt_index_default_cfg": (None, [C.POINTER(IndexCfg)]),
        "rtmodt_index_create": (C.c_int, [C.POINTER(IndexCfg), C.POINTER(vp)]),
        "rtmodt_index_destroy": (None, [vp]),
        "rtmodt_index_add": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.POINTER(i64)]),
        "rtmodt_index_add_crosscam": (C.c_int, [vp, vp, i64, C.c_int, C.POINTER(i32)]),
        "rtmodt_index_search": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, vp]),
        "rtmodt_index_forget": (C.c_int, [vp, vp, C.c_int, C.POINTER(i64)]),
        "rtmodt_index_state": (C.c_int, [vp] * 10),
        "rtmodt_index_load": (C.c_int, [vp, i64] + [vp] * 7),
        "rtmodt_index_last_ms": (C.c_int, [vp, C.POINTER(f32), C.POINTER(f32)]),
        "rtmodt_compose_default_cfg": (None, [C.POINTER(ComposeCfg)]),
        "rtmodt_compose_create": (C.c_int, [C.POINTER(ComposeCfg), C.POINTER(vp)]),
        "rtmodt_compose_destroy": (None, [vp]),
        "rtmodt_compose_set_layout": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int]),
        "rtmodt_compose_set_crop": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "rtmodt_compose_run": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_int]),
        "rtmodt_compose_output": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "rtmodt_compose_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_compose_plan": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]),
        "rtmodt_renderer_create": (C.c_int, [C.c_int, C.POINTER(RenderCfg), C.POINTER(vp)]),
        "rtmodt_renderer_destroy": (None, [vp]),
        "rtmodt_renderer_set_zones": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "rtmodt_render_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RenderList), C.c_int,
                                          C.c_double, C.c_double]),
        "rtmodt_renderer_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_render_pack": (C.c_int, [C.POINTER(RenderCfg), C.POINTER(RenderList), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                         C.c_double, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "rtmodt_jpeg_create": (C.c_int, [C.c_int, C.POINTER(JpegCfg), C.POINTER(vp)]),
        "rtmodt_jpeg_destroy": (None, [vp]),
        "rtmodt_jpeg_encode_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]),
        "rtmodt_jpeg_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_jpeg_header": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "rtmodt_jpeg_probe": (C.c_int, [vp, C.c_size_t, C.POINTER(JpegInfo)]),
        "rtmodt_jpegdec_create": (C.c_int, [C.c_int, C.POINTER(JpegDecCfg), C.POINTER(vp)]),
        "rtmodt_jpegdec_destroy": (None, [vp]),
        "rtmodt_jpegdec_decode_batch": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "rtmodt_jpegdec_last_ms": (C.c_int, [vp, C.POINTER(f32)]),
        "rtmodt_jpegdec_coefficients": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "rtmodt_coco_eval": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                       vp, vp, vp, vp, vp, vp]),
        "rtmodt_mot_eval": (C.c_int, [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(MotCounts)]),
        "rtmodt_hota_eval": (C.c_int, [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(HotaCounts)]),
        "rtmodt_detection_errors": (C.c_int, [C.c_int, C.POINTER(ErrorParams), C.c_int, C.c_int] + [vp] * 20),
        "rtmodt_stitch_tracks": (C.c_int, [C.c_int, C.POINTER(StitchParams), C.c_int] + [vp] * 9 + [i64, vp, vp, vp, C.POINTER(i64), i64, vp, vp, vp,
                                                                                                 vp, C.POINTER(i64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here == header/library drift
        fn.restype = res
        fn.argtypes = args
    L._signatures = sig
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != OK:
        raise RtmodtError(rc, lib().rtmodt_last_error().decode(errors="replace"))


class Handle:
    """Base of a class that owns one library handle: ``_h`` and ``_destroy``, the name of the symbol that releases it.  A class that
    has more to close in a fixed order overrides ``close()`` and calls this one."""
    _h = None
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_ms(symbol: str, h, k: int = 1):
    """``rtmodt_X_last_ms`` with ``k`` float outputs: the milliseconds as a float, or as a tuple when ``k > 1``."""
    out = [C.c_float(0) for _ in range(k)]
    check(getattr(lib(), symbol)(h, *[C.byref(v) for v in out]))
    return out[0].value if k == 1 else tuple(v.value for v in out)


def ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    """GPUs visible to this process (``rtmodt_device_count``)."""
    n = C.c_int(0)
    check(lib().rtmodt_device_count(C.byref(n)))
    return n.value


def device_ordinal(device) -> int:
    """``"cuda:1"`` / ``"1"`` / ``1`` -> 1 (ROCm keeps the ``cuda`` spelling, detector.py:66)."""
    if isinstance(device, int):
        return device
    s = str(device)
    if s in ("cuda", "hip", "gpu", ""):
        return 0
    if ":" in s:
        s = s.split(":", 1)[1]
    return int(s)


# ---- small functional wrappers used by tests / bench ----------------------------------
def iou_matrix(a: np.ndarray, b: np.ndarray, device: int = 0) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 4)
    out = np.empty((a.shape[0], b.shape[0]), np.float32)
    check(lib().rtmodt_iou_matrix(device, ptr(a), a.shape[0], ptr(b), b.shape[0], ptr(out)))
    return out


def assign_greedy(iou: np.ndarray, thresh: float, device: int = 0):
    iou = np.ascontiguousarray(iou, np.float32)
    m, n = iou.shape
    r2c = np.empty(m, np.int32)
    used = np.empty(n, np.int32)
    check(lib().rtmodt_assign_greedy(device, ptr(iou), m, n, float(thresh), ptr(r2c), ptr(used)))
    mr = [int(i) for i in range(m) if r2c[i] >= 0]
    return mr, [int(r2c[i]) for i in mr], [int(i) for i in range(m) if r2c[i] < 0], [int(j) for j in range(n) if not used[j]]


def assign_lapjv(iou: np.ndarray, thresh: float, device: int = 0):
    """tracker.py:168-181: ``lap.lapjv(1 - iou, extend_cost=True, cost_limit=1 - thresh)`` -> the four lists."""
    iou = np.ascontiguousarray(iou, np.float32)
    m, n = iou.shape
    r2c = np.empty(m, np.int32)
    used = np.empty(n, np.int32)
    check(lib().rtmodt_assign_lapjv(device, ptr(iou), m, n, float(1 - thresh), ptr(r2c), ptr(used)))
    mr = [int(i) for i in range(m) if r2c[i] >= 0]
    return mr, [int(r2c[i]) for i in mr], [int(i) for i in range(m) if r2c[i] < 0], [int(j) for j in range(n) if not used[j]]


def nms_pred(pred: np.ndarray, conf=0.35, iou=0.45, classes=None, agnostic=False, max_det=100, device: int = 0):
    pred = np.ascontiguousarray(pred, np.float32)
    nc, A = pred.shape[0] - 4, pred.shape[1]
    cl = None if classes is None else np.ascontiguousarray(classes, np.int32)
    xy = np.empty((max_det, 4), np.float32)
    cf = np.empty(max_det, np.float32)
    ci = np.empty(max_det, np.int32)
    an = np.empty(max_det, np.int32)
    n = C.c_int32(0)
    check(lib().rtmodt_nms_pred(device, ptr(pred), nc, A, float(conf), float(iou), ptr(cl), 0 if cl is None else len(cl),
                                int(bool(agnostic)), int(max_det), ptr(xy), ptr(cf), ptr(ci), ptr(an), C.byref(n)))
    k = n.value
    return xy[:k].copy(), cf[:k].copy(), ci[:k].copy(), an[:k].copy()


def preprocess(frame: np.ndarray, in_w: int = 640, in_h: int = 640, device: int = 0) -> np.ndarray:
    frame = np.ascontiguousarray(frame, np.uint8)
    h, w = frame.shape[:2]
    out = np.empty((in_h, in_w, 3), np.float16)
    check(lib().rtmodt_preprocess(device, ptr(frame), h, w, frame.strides[0], in_w, in_h, ptr(out)))
    return out


def preprocess_yuv420(frame: np.ndarray, fmt="nv12", in_w: int = 640, in_h: int = 640, device: int = 0, *, height: int = 0,
                      width: int = 0) -> np.ndarray:
    """One 4:2:0 host frame -> the letterboxed network input (``rtmodt_preprocess_yuv420``, the kernel alone).  ``frame``: the
    packed ``(h * 3 // 2, w)`` uint8 array of cv2 / ffmpeg (``fmt`` a format name), or any uint8 buffer with ``fmt`` a
    ``FrameFormat`` and ``height`` / ``width`` given."""
    frame = np.ascontiguousarray(frame, np.uint8)
    if isinstance(fmt, FrameFormat):
        h, w = int(height), int(width)
    else:
        if frame.ndim != 2 or frame.shape[0] % 3:
            raise ValueError(f"a packed 4:2:0 frame is a (h * 3 // 2, w) array, got shape {frame.shape}")
        h, w = frame.shape[0] * 2 // 3, frame.shape[1]
        fmt = frame_format(fmt, h, w, pitch=frame.strides[0])
    if pixel_format_id(fmt.pixel_format) == PIX_BGR24:
        raise ValueError("preprocess_yuv420 takes NV12 / I420 frames (BGR24: preprocess)")
    if frame.nbytes < frame_span(fmt, h, w):
        raise ValueError(f"the buffer holds {frame.nbytes} bytes, the layout spans {frame_span(fmt, h, w)}")
    out = np.empty((in_h, in_w, 3), np.float16)
    check(lib().rtmodt_preprocess_yuv420(device, ptr(frame), h, w, C.byref(fmt), in_w, in_h, ptr(out)))
    return out


def appearance_quantize(x: np.ndarray) -> np.ndarray:
    """Float embedding rows ``(n, dim)`` -> the int8 rows the DeepSORT gallery stores (``rtmodt_appearance_quantize``, host only)."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2:
        raise ValueError(f"embeddings are a (n, dim) array, got shape {x.shape}")
    out = np.zeros(x.shape, np.int8)
    check(lib().rtmodt_appearance_quantize(ptr(x), x.shape[0], x.shape[1], ptr(out)))
    return out


def frame_pointers(frames, mem_kind: int, height: int = 0, width: int = 0, stride: int = 0):
    """``frames`` -> (``uint8_t *[n]`` array, keep-alive list, height, width, row pitch).  Device frames (``mem_kind == MEM_DEVICE``) are
    addresses and the geometry is the caller's.  Host frames are ``(h, w, 3)`` uint8 arrays whose pixels are 3 contiguous bytes (rows may
    be padded); the geometry is read from the arrays, which must agree.  Anything else (another dtype, a BGRA view, a negative
    stride) is refused: a silent copy would change the pitch under the caller's feet."""
    if mem_kind == MEM_DEVICE:
        return (C.c_void_p * len(frames))(*[int(p) for p in frames]), [], int(height), int(width), int(stride)
    keep = list(frames)
    h, w, pitch = _host_frames(keep, writable=False)
    return (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep]), keep, h, w, pitch


def _host_frames(frames, writable: bool, one_row_any_pitch: bool = False):
    """The one check of a list of host frames -> their common (height, width, row pitch); (0, 0, 0) for an empty list.
    ``one_row_any_pitch`` (the JPEG encoder): the pitch NumPy reports for a single row means nothing and is read as at least 3w."""
    geo = (0, 0, 0)
    for i, f in enumerate(frames):
        ok = isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3 and f.strides[2] == 1 and f.strides[1] == 3
        pitch = 0 if not ok else max(f.strides[0], 3 * f.shape[1]) if one_row_any_pitch and f.shape[0] == 1 else f.strides[0]
        if not ok or pitch < 3 * f.shape[1]:
            raise ValueError(f"frame {i}: a host frame is an (h, w, 3) uint8 array with packed pixels and a row pitch >= 3w "
                             f"(got {getattr(f, 'dtype', type(f))}, shape {getattr(f, 'shape', None)}, strides {getattr(f, 'strides', None)})")
        if writable and not f.flags.writeable:
            raise ValueError(f"frame {i} is read-only; it is written in place")
        g = (f.shape[0], f.shape[1], pitch)
        if i and g != geo:
            raise ValueError("the frames of one call share their size and row pitch")
        geo = g
    return geo


def batch_frames(frames, n: int | None = None, *, height: int | None = None, width: int | None = None, stride: int | None = None,
                 offset: int = 0, writable: bool = True, strict: bool = False):
    """The frame argument block of the batched calls: ``frames`` -> ``(addresses, height, width, row stride, mem_kind, n)``.

    ``frames`` is a list of ``n`` host arrays (``(h, w, 3)`` uint8, packed pixels, rows may be padded, one shape and row stride; writable
    when ``writable``), whose geometry is read from the arrays, or a ``DeviceBuffer`` that holds the frames one after another: frame i at
    ``offset + i * height * stride`` (``stride`` defaults to ``3 * width``), checked against the buffer's size to its last byte.
    ``n`` None: ``len(frames)``, or as many frames as fit behind ``offset``.  ``strict``: an empty frame or a device stride below
    ``3 * width`` is refused here; otherwise the library refuses it.  Anything else than these two forms is refused: a silent copy would
    change the pitch under the caller's feet."""
    if isinstance(frames, DeviceBuffer):
        if height is None or width is None:
            raise ValueError("device frames need height and width")
        h, w = int(height), int(width)
        st = 3 * w if stride is None else int(stride)
        if (strict or n is None) and (h < 1 or w < 1 or st < 3 * w):
            raise ValueError(f"bad frame geometry {w}x{h}, stride {st}")
        n = (frames.nbytes - offset + st - 3 * w) // (h * st) if n is None else int(n)
        if ((strict or n) and offset < 0) or n < 0 or (n and offset + (n - 1) * h * st + (h - 1) * st + 3 * w > frames.nbytes):
            raise ValueError(f"{n} frames of {w}x{h} (stride {st}) from offset {offset} overrun the {frames.nbytes}-byte buffer")
        return [frames.ptr + offset + i * h * st for i in range(n)], h, w, st, MEM_DEVICE, n
    frames = list(frames)
    if n is not None and len(frames) != n:
        raise ValueError(f"{len(frames)} frames, {n} expected")
    h, w, st = _host_frames(frames, writable, one_row_any_pitch=strict and not writable)
    if strict and frames and (h < 1 or w < 1):
        raise ValueError(f"empty frames {h}x{w}")
    return [f.ctypes.data for f in frames], h, w, st, MEM_HOST, len(frames)


def appearance_describe(frames, boxes, *, height: int = 0, width: int = 0, stride: int = 0, mem_kind: int = MEM_HOST, device: int = 0,
                        want_counts: bool = False):
    """Descriptors of ``boxes[i]`` (an ``(n_i, 4)`` xyxy array) on ``frames[i]`` (``rtmodt_appearance_describe``): a list of
    ``(n_i, 192)`` int8 arrays, and the int32 counts too with ``want_counts``.  Host frames are ``(h, w, 3)`` uint8 arrays (row
    pitch = ``strides[0]``); device frames are addresses with ``height`` / ``width`` / ``stride`` given."""
    n = len(frames)
    boxes = [np.ascontiguousarray(b, np.float32).reshape(-1, 4) for b in boxes]
    fp, keep, height, width, stride = frame_pointers(frames, mem_kind, height, width, stride)
    mb = max(1, max(len(b) for b in boxes))
    xy = np.zeros((n, mb, 4), np.float32)
    for i, b in enumerate(boxes):
        xy[i, :len(b)] = b
    cnt = np.asarray([len(b) for b in boxes], np.int32)
    desc = np.zeros((n, mb, 192), np.int8)
    counts = np.zeros((n, mb, 192), np.int32) if want_counts else None
    check(lib().rtmodt_appearance_describe(device, fp, n, int(height), int(width), int(stride), mem_kind, ptr(xy), ptr(cnt), mb, ptr(desc),
                                           ptr(counts)))
    d = [desc[i, :len(b)].copy() for i, b in enumerate(boxes)]
    return (d, [counts[i, :len(b)].copy() for i, b in enumerate(boxes)]) if want_counts else d


def appearance_dotmax(gallery: np.ndarray, counts, dets: np.ndarray, device: int = 0) -> np.ndarray:
    """``gallery (T, budget, dim)`` int8 with ``counts[T]`` valid rows, ``dets (N, dim)`` int8 -> ``(T, N)`` int32 (``rtmodt_appearance_dotmax``)."""
    gallery = np.ascontiguousarray(gallery, np.int8)
    dets = np.ascontiguousarray(dets, np.int8)
    counts = np.ascontiguousarray(counts, np.int32)
    T, budget, dim = gallery.shape
    out = np.zeros((T, dets.shape[0]), np.int32)
    check(lib().rtmodt_appearance_dotmax(device, ptr(gallery), ptr(counts), T, budget, ptr(dets), dets.shape[0], dim, ptr(out)))
    return out


class DeviceBuffer:
    """A raw device allocation owned by the library (frame rings for the bench)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = device, nbytes
        p = C.c_void_p()
        check(lib().rtmodt_device_alloc(device, nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, host: np.ndarray, offset: int = 0):
        host = np.ascontiguousarray(host)
        assert offset + host.nbytes <= self.nbytes
        check(lib().rtmodt_memcpy_h2d(self.device, C.c_void_p(self.ptr + offset), ptr(host), host.nbytes))

    def download(self, nbytes: int | None = None, offset: int = 0) -> np.ndarray:
        """``nbytes`` bytes from ``offset`` (default: the rest of the buffer) as a new host uint8 array."""
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        if offset < 0 or nbytes < 0 or offset + nbytes > self.nbytes:
            raise ValueError(f"[{offset}, {offset + nbytes}) outside the {self.nbytes}-byte buffer")
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            check(lib().rtmodt_memcpy_d2h(self.device, ptr(out), C.c_void_p(self.ptr + offset), nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().rtmodt_device_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """A NumPy view over page-locked host memory owned by the library: frames written here (by a decoder,
    a capture thread, ...) reach the GPU by asynchronous DMA underneath the previous batch's compute."""

    def __init__(self, shape, dtype=np.uint8, device: int = 0):
        self.device = device
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check(lib().rtmodt_host_alloc(device, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p.value
        buf = (C.c_uint8 * self.nbytes).from_address(self.ptr)
        buf._owner = self                                 # every NumPy view of the memory keeps its owner (and so the allocation) alive
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().rtmodt_host_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
