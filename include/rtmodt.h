/* rtmodt.h -- C ABI of librtmodt_hip.so, the MI355X (gfx950) detect + track hot path.
 *
 * Drop-in boundary for the reference's two hot-path classes:
 *   src/detection/detector.py:54-135   class Detector          -> rtmodt_detector_*
 *   src/tracking/tracker.py:43-194     class _ByteTrackCore    -> rtmodt_tracker_*
 * The Python classes of the same names in the package call these entry points through
 * ctypes; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain C, opaque handles, host pointers unless a parameter says "device".
 * Every function returns 0 on success or a negative RTMODT_E_* code; the message for the
 * calling thread's last failure is rtmodt_last_error().  No exceptions cross the ABI.
 * The library owns all device memory (one static arena per handle).  Handles are not
 * thread-safe: one Detector + one tracker per stream group, used from one thread
 * (as the reference's single main loop does, tools/run_pipeline.py:121-166).
 */
#ifndef RTMODT_H
#define RTMODT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTMODT_OK 0
#define RTMODT_E_INVALID (-1)   /* bad argument / unsupported configuration            */
#define RTMODT_E_IO (-2)        /* weight file missing or malformed                    */
#define RTMODT_E_HIP (-3)       /* HIP runtime failure (message carries hipGetErrorString) */
#define RTMODT_E_CAPACITY (-4)  /* more tracks / detections than the handle was sized for */
#define RTMODT_E_UNSUPPORTED (-5)

#define RTMODT_MEM_HOST 0
#define RTMODT_MEM_DEVICE 1

#define RTMODT_ASSIGN_GREEDY 0  /* tracker.py:182-194 (the branch taken when `lap` is absent) */
#define RTMODT_ASSIGN_LAPJV 1   /* tracker.py:168-181 (the branch taken when `lap` is importable): exact optimal assignment
                                 * under cost_limit = 1 - match_thresh; PARITY UNPINNED (no `lap` to run against) */

typedef struct rtmodt_detector rtmodt_detector;
typedef struct rtmodt_tracker rtmodt_tracker;
typedef struct rtmodt_zones rtmodt_zones;
typedef struct rtmodt_renderer rtmodt_renderer;
typedef struct rtmodt_jpeg rtmodt_jpeg;
typedef struct rtmodt_jpegdec rtmodt_jpegdec;
typedef struct rtmodt_deepsort rtmodt_deepsort;
typedef struct rtmodt_ocsort rtmodt_ocsort;
typedef struct rtmodt_botsort rtmodt_botsort;
typedef struct rtmodt_gmc rtmodt_gmc;
typedef struct rtmodt_reid rtmodt_reid;

/* ---- library / device ------------------------------------------------------------- */
const char *rtmodt_last_error(void);
const char *rtmodt_version(void);
/* "csrc_sha256=<digest of the kernel sources this binary was built from> diag=<0|1>": bench.py attaches a measured
 * roofline.traffic only to a library whose digest equals the one the counters were collected on */
const char *rtmodt_build_info(void);
/* The value of the run-time option RTMODT_<name> exactly as the library reads it (NULL when unset).  Options are read at
 * detector-create / autotune time only, from ONE table (csrc/common.h); a name outside it is RTMODT_E_INVALID -- never an abort. */
int rtmodt_option(const char *name, const char **value);
int rtmodt_device_count(int *count);
int rtmodt_synchronize(int device);                 /* replaces torch.cuda.synchronize() (latency_profiler.py:63,69) */
int rtmodt_device_alloc(int device, size_t bytes, void **out);
int rtmodt_device_free(int device, void *ptr);
/* Page-locked host memory for the frame source (the ring RTSPReader.read() copies out of,
 * src/ingestion/rtsp_reader.py:74-79): enqueue_batch copies host frames on its own HIP stream into a
 * per-slot staging area, so frames that live in such memory upload underneath the previous
 * batch's forward pass; pageable frames still work but their copy blocks the calling thread. */
int rtmodt_host_alloc(int device, size_t bytes, void **out);
int rtmodt_host_free(int device, void *ptr);
int rtmodt_memcpy_h2d(int device, void *dst_device, const void *src_host, size_t bytes);
int rtmodt_memcpy_d2h(int device, void *dst_host, const void *src_device, size_t bytes);

/* ---- detector: replaces Detector.__init__/detect/_parse (detector.py:59-129) ------- */
typedef struct rtmodt_det_cfg {
    const char *weight_path;   /* RTMODTW1 file (package weights.py); model scale/nc come from its header */
    int32_t in_w, in_h;        /* network input = letterbox target; multiples of 32 (detector.py:61, :102) */
    float conf;                /* detector.py:62  confidence=0.35  (strict >, float32)                      */
    float iou;                 /* detector.py:63  iou=0.45         (strict >)                               */
    const int32_t *classes;    /* detector.py:64  class filter, NULL = all                                 */
    int32_t n_classes;
    int32_t half;              /* detector.py:65,76  must be 1: the engine stores activations in fp16       */
    int32_t device;            /* detector.py:66  ordinal of "cuda:N"                                      */
    int32_t max_det;           /* detector.py:67  max_det=100                                              */
    int32_t agnostic;          /* detector.py:68  agnostic_nms                                             */
    int32_t batch;             /* frames per detect_batch call (streams batched on this GPU), >= 1         */
    int32_t max_src_w, max_src_h; /* largest source frame accepted (staging), 0 = in_w/in_h                */
    int32_t use_graph;         /* 1: replay the forward pass as one captured hipGraph                      */
    int32_t autotune;          /* 1: time every conv tile configuration at create and keep the fastest      */
    int32_t chains;            /* sub-batches that run as independent chains (stem -> graph -> decode) on their own streams;
                                * -1 / -2 = STAGED with S = 2 / 3 stages: the whole batch per launch, the net cut into S
                                * stages on S streams, stage 1 of batch t + 1 overlapping stage 2 of batch t (S arena
                                * copies; keep S + 1 batches in flight: enqueue t + S before fetching t).  Three stages
                                * take every hardware queue of the process: use them when the frames are already in
                                * device memory, two when they come from the host through the engine's copy stream;
                                * 0 = automatic: two stages for batch >= 2, the plain single-stream engine for batch 1;
                                * 1 = plain engine; n > 1 = n sub-batch chains */
    int32_t rect;              /* 1: minimal-rectangle letterbox of `predict` on a .pt model (LetterBox auto=True): the scale is
                                * min(S/h, S/w) with S = max(in_w, in_h) and in_w x in_h is the rectangle (1080p: 640 x 384) */
} rtmodt_det_cfg;

int rtmodt_detector_create(const rtmodt_det_cfg *cfg, rtmodt_detector **out);
void rtmodt_detector_destroy(rtmodt_detector *det);

/* One frame, synchronous: letterbox -> forward -> decode -> NMS -> rescale -> D2H.
 * bgr: H x W x 3 uint8, row pitch stride_bytes (host).  Outputs caller-allocated:
 * xyxy[max_det*4], conf[max_det], cls[max_det]; *n_out = number of detections. */
int rtmodt_detector_detect(rtmodt_detector *det, const uint8_t *bgr, int h, int w, int stride_bytes,
                           float *xyxy, float *conf, int32_t *cls, int32_t *n_out);

/* n <= cfg.batch frames of identical size in one pass (BASELINE configs 4-5: streams
 * batched per GPU).  frames[i] is a host or device pointer per mem_kind.  Outputs are
 * [n][max_det] blocks; n_out[n]. */
int rtmodt_detector_detect_batch(rtmodt_detector *det, const uint8_t *const *frames, int n, int h, int w,
                                 int stride_bytes, int mem_kind, float *xyxy, float *conf, int32_t *cls,
                                 int32_t *n_out);

/* Asynchronous halves of detect_batch for the throughput path: enqueue leaves the
 * detections on the device (consumable by rtmodt_tracker_update_from_detector on the same
 * HIP stream, no host round trip) and starts their copy to pinned host memory; fetch waits
 * for the OLDEST batch in flight and hands it out.  Up to two batches may be in flight
 * (enqueue t+1, then fetch t), which hides the host's per-step work behind the GPU. */
int rtmodt_detector_enqueue_batch(rtmodt_detector *det, const uint8_t *const *frames, int n, int h, int w,
                                  int stride_bytes, int mem_kind);
int rtmodt_detector_fetch(rtmodt_detector *det, float *xyxy, float *conf, int32_t *cls, int32_t *n_out);

/* Pixel formats of the frames enqueue_batch_fmt / preprocess_yuv420 take.  The 4:2:0 formats are converted on the GPU with
 * OpenCV's integer BT.601 limited-range conversion (cv2.cvtColor COLOR_YUV2BGR_NV12 / _I420, restated in DESIGN.md section 3;
 * PARITY UNPINNED: no OpenCV to run against) and then letterboxed exactly as BGR24 frames are. */
#define RTMODT_PIX_BGR24 0      /* packed B, G, R                                                         */
#define RTMODT_PIX_NV12 1       /* Y plane, then ONE interleaved U, V plane at half resolution (U first)  */
#define RTMODT_PIX_I420 2       /* Y plane, then a U plane and a V plane at half resolution (yuv420p)     */
typedef struct rtmodt_frame_format {
    int32_t pixel_format;  /* RTMODT_PIX_*                                                                            */
    int32_t colorspace;    /* 0 = BT.601 limited range (the only one); anything else RTMODT_E_UNSUPPORTED (4:2:0 only)  */
    int32_t pitch;         /* bytes per row of the BGR image / of the Y plane; 0 = 3w / w                                */
    int32_t chroma_pitch;  /* bytes per chroma row; 0 = pitch (NV12) or pitch / 2 (I420)                                  */
    int64_t u_offset;      /* frame pointer -> UV (NV12) or U (I420) plane; 0 = pitch * h (decoders often pad: pitch * 1088) */
    int64_t v_offset;      /* I420 only: frame pointer -> V plane; 0 = u_offset + chroma_pitch * h / 2                     */
} rtmodt_frame_format;
/* enqueue_batch for frames in the layout `fmt` describes (NULL = BGR24 with pitch 3w).  BGR24 is enqueue_batch exactly.  4:2:0
 * frames: h and w even, every plane inside [frame, frame + span) and no two planes overlapping, else RTMODT_E_INVALID with
 * nothing launched; host frames are staged as that one span per frame (RTMODT_E_CAPACITY beyond max_src's BGR bytes).  They
 * take the letterbox kernel of resized BGR frames (never the stem's byte source or the in-place read of RTMODT_ZERO_COPY);
 * results come out of rtmodt_detector_fetch and feed rtmodt_tracker_update_from_detector* as usual. */
int rtmodt_detector_enqueue_batch_fmt(rtmodt_detector *det, const uint8_t *const *frames, int n, int h, int w,
                                      const rtmodt_frame_format *fmt, int mem_kind);

/* Introspection used by the parity tests and bench.py */
int rtmodt_detector_info(rtmodt_detector *det, int32_t *scale_id, int32_t *nc, int32_t *n_anchors,
                         int32_t *n_convs, int64_t *conv_flops_per_frame, int64_t *arena_bytes);
/* Number of sub-batch chains this detector runs its batch as (see rtmodt_det_cfg.chains). */
int rtmodt_detector_chains(rtmodt_detector *det, int32_t *n_chains);
/* Stages the detector runs as (rtmodt_det_cfg.chains = -1 / -2 and a hardware queue found for each): 2 or 3, else 1. */
int rtmodt_detector_stages(rtmodt_detector *det, int32_t *n_stages);
/* Copies out, for frame `img` of the last batch: the letterboxed network input as fp16 NHWC(3)
 * [in_h*in_w*3] (may be NULL), the three Detect maps as fp16 [A_i*(64+nc)] concatenated
 * P3,P4,P5 (may be NULL) and the decoded pre-NMS tensor pred[(4+nc)*A] float32 (may be NULL). */
int rtmodt_detector_debug_fetch(rtmodt_detector *det, int img, uint16_t *input_f16, uint16_t *heads_f16, float *pred);
/* Output of fused conv `name` ("4.cv2", "22.cv3.0.1", ...) for frame img as fp16 NHWC [H*W*C];
 * shape returned through hwc[3]; out may be NULL to query the shape. */
int rtmodt_detector_debug_layer(rtmodt_detector *det, const char *name, int img, uint16_t *out, int32_t *hwc);
/* Per-launch device time of the last `iters` eager (non-graph) forwards, measured with HIP
 * events on the detector's stream: names[i] points into handle-owned storage. */
int rtmodt_detector_profile(rtmodt_detector *det, int iters, int max_entries, const char **names, float *ms,
                            int64_t *flops, int32_t *n_entries);
/* Device time (ms, HIP events on the detector's stream) of the batch the last fetch returned:
 * whole pass, and the letterbox + forward-graph part alone. */
int rtmodt_detector_last_timing(rtmodt_detector *det, float *total_ms, float *forward_ms);
/* The same batch split into the stages the reference's profiler names (latency_profiler.py:38):
 * preprocess = letterbox, inference = forward pass + decode, nms = NMS + rescale (device ms). */
int rtmodt_detector_stage_times(rtmodt_detector *det, float *preprocess_ms, float *inference_ms, float *nms_ms);
/* In-kernel shader clock (measurement aid, no reference counterpart): while enabled, one wave behind every batch's NMS reads the
 * shader-cycle counter against the constant 100 MHz counter for ~20 us; _read waits for the post-processing stream and returns
 * mean / min / max GHz over the samples since it was enabled (or read last).  The MFMA peak at THAT clock, not at the 2.4 GHz of
 * the data sheet, is what the matrix cores could have delivered during the run. */
int rtmodt_detector_clock_enable(rtmodt_detector *det, int on);
int rtmodt_detector_clock_read(rtmodt_detector *det, double *ghz_mean, double *ghz_min, double *ghz_max, int32_t *n_samples);

/* decode-free NMS on a caller-supplied pre-NMS tensor pred[(4+nc)*A] float32 (the layout
 * ultralytics' non_max_suppression receives): BASELINE config 2's
 * "NMS correctness" case.  dets out: xyxy in the tensor's own coordinates (no rescale). */
int rtmodt_nms_pred(int device, const float *pred, int nc, int n_anchors, float conf, float iou,
                    const int32_t *classes, int n_classes, int agnostic, int max_det,
                    float *xyxy, float *conf_out, int32_t *cls, int32_t *anchor_idx, int32_t *n_out);

/* letterbox + BGR->RGB + /255 alone (ultralytics LetterBox + cv2.resize INTER_LINEAR restated):
 * out fp16 NHWC [in_h*in_w*3]. */
int rtmodt_preprocess(int device, const uint8_t *bgr, int h, int w, int stride_bytes, int in_w, int in_h,
                      uint16_t *out_f16);
/* The same for one 4:2:0 host frame (fmt: RTMODT_PIX_NV12 / RTMODT_PIX_I420): conversion + letterbox, the kernel alone. */
int rtmodt_preprocess_yuv420(int device, const uint8_t *frame, int h, int w, const rtmodt_frame_format *fmt,
                             int in_w, int in_h, uint16_t *out_f16);

/* ---- tracker: replaces _ByteTrackCore (tracker.py:43-194) ---------------------------- */
/* n_streams independent tracker states updated by ONE launch (one workgroup per stream). */
int rtmodt_tracker_create(int device, float track_thresh, int track_buffer, float match_thresh,
                          int assign_mode, int max_tracks, int max_dets, int n_streams, rtmodt_tracker **out);
void rtmodt_tracker_destroy(rtmodt_tracker *trk);
/* RTMODT_ASSIGN_LAPJV only: the reference evaluates `cost_limit = 1 - thresh` in Python doubles
 * (tracker.py:170); match_thresh above is a float, so a caller that wants the identical limit
 * passes it here.  Default: 1.0 - (double)match_thresh. */
int rtmodt_tracker_set_cost_limit(rtmodt_tracker *trk, double cost_limit);

/* One frame for one stream (tracker.py:58-141).  *n_active_out = tracks with
 * time_since_update == 0 after the update -- always 0, as in the reference (SURVEY finding 4). */
int rtmodt_tracker_update(rtmodt_tracker *trk, int stream, const float *xyxy, const float *conf,
                          const int32_t *cls, int n, int32_t *n_active_out);
/* One frame for every stream: xyxy[n_streams][max_dets][4], conf/cls[n_streams][max_dets], n[n_streams]. */
int rtmodt_tracker_update_batch(rtmodt_tracker *trk, const float *xyxy, const float *conf, const int32_t *cls,
                                const int32_t *n, int32_t *n_active_out);
/* Consumes the device-resident detections of det's last enqueue_batch (stream i <- frame i),
 * asynchronously on det's HIP stream. */
int rtmodt_tracker_update_from_detector(rtmodt_tracker *trk, rtmodt_detector *det);
/* The same for frames [first_frame, first_frame + n_frames) of det's batch (stream i <- frame first_frame + i):
 * a batch that holds several CONSECUTIVE frames of every stream (frame-major: image f * n_streams + s) is
 * tracked by calling this once per f, in order -- tracker.py:58-141 still sees each stream's frames one at a time. */
int rtmodt_tracker_update_from_detector_frames(rtmodt_tracker *trk, rtmodt_detector *det, int first_frame, int n_frames);
/* A frame-major batch (image f * n_streams + s, starting at first_frame) of n_frames consecutive frames of n_streams streams
 * in ONE launch: stream s's workgroup walks over its n_frames detection slots in order, so every stream still sees
 * tracker.py:58-141 one frame at a time; state after the call == n_frames calls of _update_from_detector_frames. */
int rtmodt_tracker_update_from_detector_batch(rtmodt_tracker *trk, rtmodt_detector *det, int first_frame, int n_streams, int n_frames);
/* List-order snapshot of a stream's state = the reference's _core._tracks + _core._next_id
 * (the parity surface).  Arrays sized max_tracks; any may be NULL. */
int rtmodt_tracker_state(rtmodt_tracker *trk, int stream, int64_t *ids, float *xyxy, float *conf,
                         int32_t *cls, int32_t *age, int32_t *tsu, int32_t *n, int64_t *next_id);
/* Empties one stream -- no tracks, ids start again at 1, a sticky RTMODT_E_CAPACITY is cleared -- and leaves the others as they
 * are.  ANY negative stream means all streams (-1 by convention); stream >= n_streams is RTMODT_E_INVALID. */
int rtmodt_tracker_reset(rtmodt_tracker *trk, int stream);
/* OPT-IN, no reference counterpart (the reference overwrites a matched track's box, tracker.py:99-104, and has no motion
 * model): ByteTrack's published 8-state constant-velocity Kalman filter over (cx, cy, a, h), batched inside the same
 * launch -- every track is predicted at the start of a frame, association runs on the predicted boxes, a matched track
 * is corrected with its detection, a new track is initiated from it.  `xyxy` in rtmodt_tracker_state keeps the
 * reference's meaning (the last matched detection).  Call before the first update.  oracle/kalman_oracle.py. */
int rtmodt_tracker_enable_kalman(rtmodt_tracker *trk);
/* Filter state in list order: mean[n][8] = (cx, cy, a, h, vx, vy, va, vh); cov[n][12] = per coordinate the (a, b, c)
 * entries of its 2x2 covariance block [[a, b], [b, c]] (the 8x8 covariance is block-diagonal by construction). */
int rtmodt_tracker_kalman_state(rtmodt_tracker *trk, int stream, float *mean, float *cov, int32_t *n);

/* _ByteTrackCore._batch_iou (tracker.py:150-161) alone: out[m*n] float32, bit-exact. */
int rtmodt_iou_matrix(int device, const float *a, int m, const float *b, int n, float *out);
/* _linear_assignment greedy branch (tracker.py:182-194) alone on a caller-supplied matrix:
 * row_to_col[m] (-1 = unmatched), col_used[n]. */
int rtmodt_assign_greedy(int device, const float *iou, int m, int n, float thresh, int32_t *row_to_col,
                         int32_t *col_used);
/* _linear_assignment lap.lapjv branch (tracker.py:168-181) alone: the optimal assignment of
 * cost = 1 - iou (float32) extended with cost_limit, i.e. the maximum-gain matching over pairs
 * with cost < cost_limit.  RTMODT_E_CAPACITY when more than 256 rows / 256 columns / 2048 pairs
 * are contested (share a row or column with another candidate pair). */
int rtmodt_assign_lapjv(int device, const float *iou, int m, int n, double cost_limit, int32_t *row_to_col,
                        int32_t *col_used);

/* ---- DeepSORT: the tracker config/default.yaml:47 offers as `algorithm: "deepsort"` and src/tracking/tracker.py:212-214 never wired ---- */
/* The published algorithm (Wojke et al.; deep_sort's tracker.py, linear_assignment.py, nn_matching.py, kalman_filter.py) with the
 * state resident on the device: csrc/deepsort.hip states the rules, tests/deepsort_ref.py restates them.  PARITY UNPINNED:
 * deep_sort_realtime is installed nowhere this runs.  Limits: 256 tracks and 1024 detections per stream, nn_budget <= 128, 64
 * streams, and the contested-pair limits of rtmodt_assign_lapjv; beyond them RTMODT_E_CAPACITY, never a fault. */
typedef struct rtmodt_deepsort_cfg {
    double max_dist;            /* default.yaml:54  0.2: a pair is admissible when max(0, 16129 - dotmax) <= floor(max_dist * 16129) */
    float min_confidence;       /* default.yaml:55  0.3: detections below it are dropped (float32 >=)                            */
    double max_iou_distance;    /* default.yaml:56  0.7: IoU stage, 1 - iou <= max_iou_distance                                  */
    int32_t max_age;            /* default.yaml:57  70: an unmatched confirmed track dies when time_since_update > max_age       */
    int32_t n_init;             /* default.yaml:58  3: hits before a tentative track is confirmed                                */
    int32_t nn_budget;          /* default.yaml:59  100: descriptors kept per track (a ring of the last nn_budget since birth)    */
    const char *embedder;       /* default.yaml:60: NULL, "" or "colorhist" = the built-in descriptor; a path ending in ".rtreid" =
                                 * the OSNet x0.25 network of rtmodt_reid_* on that weight file, built inside the tracker (frames are
                                 * then described by the network, caller descriptors are refused, RTMODT_E_INVALID when the file is
                                 * missing or damaged); any other model file (".onnx" included) is RTMODT_E_UNSUPPORTED: convert the
                                 * checkpoint with tools/convert_weights.py --reid, or bring its output as caller descriptors      */
    int32_t dim;                /* descriptor dimension: 0 = 192 (built-in) or 512 (network); 64..512 in multiples of 64 for caller
                                 * descriptors; with a network 0 or 512                                                          */
    int32_t max_tracks, max_dets, n_streams, device;
} rtmodt_deepsort_cfg;
int rtmodt_deepsort_create(const rtmodt_deepsort_cfg *cfg, rtmodt_deepsort **out);
void rtmodt_deepsort_destroy(rtmodt_deepsort *ds);
int rtmodt_deepsort_reset(rtmodt_deepsort *ds, int stream);   /* stream < 0: all */

/* The built-in appearance descriptor (the "colour histogram per track" of TECHNICAL_DESIGN_DOCUMENT.md B.4, standing in for
 * default.yaml:60's embedder) of max_boxes box slots per frame: frames as in rtmodt_render_batch (BGR24, h x w, pitch
 * stride_bytes >= 3w, host or device pointers, only read), xyxy[n_frames][max_boxes][4], n_boxes[n_frames].  Outputs (host):
 * desc[n_frames][max_boxes][192] int8 and, when not NULL, counts[n_frames][max_boxes][192] int32 -- rows past n_boxes are zero.
 * Rules: csrc/appearance.hip.  Two launches whatever the number of boxes.  At most 64 frames and 1024 boxes per frame. */
int rtmodt_appearance_describe(int device, const uint8_t *const *frames, int n_frames, int h, int w, int stride_bytes, int mem_kind,
                               const float *xyxy, const int32_t *n_boxes, int max_boxes, int8_t *desc, int32_t *counts);
/* Host only, no device needed: float rows x[n][dim] of an embedder that runs elsewhere (default.yaml:60) -> int8 rows,
 * rint(127 * x / ||x||) in float64 (norm by sequential summation), a zero row gives zeros.  dim 64..512 in multiples of 64. */
int rtmodt_appearance_quantize(const float *x, int n, int dim, int8_t *out);
/* The gallery distance alone (default.yaml:54, :59), as rtmodt_iou_matrix exposes the IoU alone: gallery[n_tracks][budget][dim]
 * int8 with counts[n_tracks] valid rows each, dets[n_dets][dim]; out[n_tracks][n_dets] = the maximum over a track's rows of the
 * int8 dot product with the detection (exact, int32), INT32_MIN for a track without rows.  v_mfma_i32_16x16x64_i8. */
int rtmodt_appearance_dotmax(int device, const int8_t *gallery, const int32_t *counts, int n_tracks, int budget, const int8_t *dets,
                             int n_dets, int dim, int32_t *out);

/* One frame for every stream (default.yaml:53-60): xyxy[n_streams][max_dets][4], conf / cls[n_streams][max_dets], n[n_streams],
 * plus EITHER frames[n_streams] (the frame each stream's boxes lie on; descriptors are computed on the GPU) OR
 * desc[n_streams][max_dets][dim] int8 caller descriptors -- never both; neither is needed when every n is 0.
 * n_returned_out[n_streams] (may be NULL) = confirmed tracks matched in this frame (what update() returns). */
int rtmodt_deepsort_update_batch(rtmodt_deepsort *ds, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                                 const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind, const int8_t *desc,
                                 int32_t *n_returned_out);
/* The same on the device-resident detections of det's last enqueue_batch (stream i <- frame i; frames[n_frames] are the frames
 * that batch was made of), queued on det's HIP stream behind its NMS: the detections never visit the host.  With
 * RTMODT_MEM_DEVICE frames the call is asynchronous; the frames must stay valid and unchanged until the work is done
 * (rtmodt_deepsort_state, rtmodt_deepsort_last_ms and rtmodt_synchronize all wait for it).  With RTMODT_MEM_HOST frames they are
 * first copied to a staging area on that stream: the copy of pageable memory blocks the calling thread, the frames must stay
 * valid until a synchronisation, and a call that has to grow the staging area (the first one, or larger frames) waits for the
 * stream first.  Use device frames (where the detector read them) for the asynchronous path. */
int rtmodt_deepsort_update_from_detector(rtmodt_deepsort *ds, rtmodt_detector *det, const uint8_t *const *frames, int n_frames, int h,
                                         int w, int stride_bytes, int mem_kind);
/* A stream's tracks in list order (creation order, deletions compacted); arrays sized max_tracks, any may be NULL.  state: 1
 * tentative, 2 confirmed; xyxy / conf / cls: the last matched detection; mean[n][8], cov[n][12] as rtmodt_tracker_kalman_state;
 * gallery_count[n] = stored descriptors, gallery[n][nn_budget][dim] = those rows oldest first (the rest zero). */
int rtmodt_deepsort_state(rtmodt_deepsort *ds, int stream, int64_t *ids, int32_t *state, int32_t *hits, int32_t *age, int32_t *tsu,
                          float *xyxy, float *conf, int32_t *cls, float *mean, float *cov, int32_t *gallery_count, int8_t *gallery,
                          int32_t *n, int64_t *next_id);
/* Device time (ms, HIP events) of the last update's three parts: descriptors (0 with caller descriptors), distance, update. */
int rtmodt_deepsort_last_ms(rtmodt_deepsort *ds, float *describe_ms, float *distance_ms, float *update_ms);

/* ---- OC-SORT: the motion-only tracker of TECHNICAL_DESIGN_DOCUMENT.md H.2 (row 4, "Req. Re-ID Model: No") ---- */
/* Observation-Centric SORT (Cao et al., CVPR 2023) with the state resident on the device: csrc/ocsort.hip states the rules (split,
 * SORT's 7-state filter, direction-consistent first association, BYTE stage, recovery on the last observation, re-update across
 * an occlusion), tests/ocsort_ref.py restates them and the kernel equals that restatement bit for bit.  PARITY UNPINNED: ocsort,
 * boxmot and filterpy are installed nowhere this runs.  Class-agnostic, as published: a track carries the class of its last matched
 * detection.  One launch per call whatever the counts.  Limits: 256 tracks and 1024 detections per stream, 64 streams, delta_t <= 8,
 * and the contested-pair limits of rtmodt_assign_lapjv; beyond them RTMODT_E_CAPACITY, never a fault. */
typedef struct rtmodt_ocsort_cfg {
    float det_thresh;           /* 0.6: high detections have conf > det_thresh (float32, strict)                                 */
    float low_thresh;           /* 0.1: low detections have low_thresh < conf < det_thresh; used only with use_byte              */
    float iou_threshold;        /* 0.3: a pair is admissible when iou >= iou_threshold (float32).  Must exceed inertia / 2 (our
                                 * rule, RTMODT_E_INVALID otherwise): it makes every admissible pair's gain positive             */
    double inertia;             /* 0.2: weight of the direction-consistency term of the first association; 0 turns it off        */
    int32_t max_age;            /* 30: an unmatched track dies when time_since_update > max_age                                  */
    int32_t min_hits;           /* 3: a matched track is returned once hit_streak >= min_hits (or while frame_count <= min_hits) */
    int32_t delta_t;            /* 3: frames back to the reference observation of a track's direction; 1..8 (8 is our limit)     */
    int32_t use_byte;           /* 0: non-zero adds the BYTE stage on the low detections                                         */
    int32_t max_tracks, max_dets, n_streams, device;
} rtmodt_ocsort_cfg;
int rtmodt_ocsort_create(const rtmodt_ocsort_cfg *cfg, rtmodt_ocsort **out);
void rtmodt_ocsort_destroy(rtmodt_ocsort *oc);
int rtmodt_ocsort_reset(rtmodt_ocsort *oc, int stream);       /* stream < 0: all */
/* One frame for every stream: xyxy[n_streams][max_dets][4], conf / cls[n_streams][max_dets], n[n_streams].
 * n_returned_out[n_streams] (may be NULL) = the tracks returned this frame (what update() returns). */
int rtmodt_ocsort_update_batch(rtmodt_ocsort *oc, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                               int32_t *n_returned_out);
/* The same on the device-resident detections of det's last enqueue_batch (stream i <- frame i), queued on det's HIP stream behind
 * its NMS: asynchronous, the detections never visit the host (rtmodt_ocsort_state, rtmodt_ocsort_last_ms and rtmodt_synchronize
 * wait for it). */
int rtmodt_ocsort_update_from_detector(rtmodt_ocsort *oc, rtmodt_detector *det);
/* A stream's tracks in list order (creation order, deletions compacted); arrays sized max_tracks, any may be NULL.  xyxy / conf /
 * cls: the last observation (before a track's first match: its birth detection; hits > 0 <=> it has an observation);
 * mean[n][8] = (x, y, s, r, vx, vy, vs, 0), cov[n][12] as rtmodt_tracker_kalman_state; direction[n][2] = the stored unit direction
 * (dy, dx), zero when none.  A track is returned this frame when tsu == 0 and (hit_streak >= min_hits or frame_count <= min_hits).
 * On a stream in (sticky) error the outputs are still filled in before RTMODT_E_CAPACITY is returned. */
int rtmodt_ocsort_state(rtmodt_ocsort *oc, int stream, int64_t *ids, int32_t *hits, int32_t *hit_streak, int32_t *age, int32_t *tsu,
                        float *xyxy, float *conf, int32_t *cls, float *mean, float *cov, float *direction, int32_t *n,
                        int64_t *next_id, int64_t *frame_count);
/* Device time (ms, HIP events) of the last update's single launch. */
int rtmodt_ocsort_last_ms(rtmodt_ocsort *oc, float *update_ms);

/* ---- BoT-SORT: the tracker TECHNICAL_DESIGN_DOCUMENT.md H.2 ranks best (row 3, IDF1 0.83, 38 switches, "Req. Re-ID Model: Yes") ---- */
/* BoT-SORT (Aharon et al., 2022) with the state resident on the device: csrc/botsort.hip states the rules (split, the 8-state filter
 * on width and height with its two 4x4 covariance blocks, camera-motion compensation by a caller-supplied warp, IoU fused with the
 * detection score and with appearance, the second association on the low detections, new / tracked / lost life cycle, duplicate
 * removal), tests/botsort_ref.py restates them and the kernel equals that restatement bit for bit.  PARITY UNPINNED: BoT-SORT and
 * boxmot are installed nowhere this runs.  Class-agnostic.  A fixed number of launches per call whatever the counts.  Limits: 256
 * tracks and 1024 detections per stream, 64 streams, descriptors of at most 512 values, and the contested-pair limits of
 * rtmodt_assign_lapjv; beyond them RTMODT_E_CAPACITY, never a fault.  The warp comes from whoever has it (PTZ telemetry) or from
 * the estimator below (rtmodt_gmc_*), which computes it from the frames themselves. */
typedef struct rtmodt_botsort_cfg {
    float track_high_thresh;    /* H.2 row 3  0.6: high detections have conf > track_high_thresh (float32, strict)               */
    float track_low_thresh;     /* 0.1: low detections have track_low_thresh < conf < track_high_thresh                          */
    float new_track_thresh;     /* 0.7: an unmatched high detection becomes a track when conf >= new_track_thresh                */
    int32_t track_buffer;       /* 30: a lost track dies when frame_count - last_frame > track_buffer                            */
    double match_thresh;        /* 0.8: the first association admits a pair when its cost <= match_thresh                        */
    double proximity_thresh;    /* 0.5: appearance is ignored for a pair with 1 - iou > proximity_thresh                         */
    double appearance_thresh;   /* 0.25: ... and when (1 - cos) / 2 > appearance_thresh                                          */
    int32_t fuse_score;         /* 1: the IoU cost is 1 - iou * conf (the published `not mot20`)                                 */
    const char *embedder;       /* NULL, "" or "none" = motion only; "colorhist" = the built-in descriptor (or, with dim != 192,
                                 * caller descriptors); a path ending in ".rtreid" = the OSNet x0.25 network of rtmodt_reid_*;
                                 * anything else is RTMODT_E_UNSUPPORTED, as rtmodt_deepsort_create words it                     */
    int32_t dim;                /* descriptor dimension: 0 = 192 (built-in) or 512 (network); 64..512 in multiples of 64 for caller
                                 * descriptors; must be 0 without an embedder                                                    */
    int32_t max_tracks, max_dets, n_streams, device;
} rtmodt_botsort_cfg;
int rtmodt_botsort_create(const rtmodt_botsort_cfg *cfg, rtmodt_botsort **out);                    /* H.2 row 3 */
void rtmodt_botsort_destroy(rtmodt_botsort *bot);
int rtmodt_botsort_reset(rtmodt_botsort *bot, int stream);    /* stream < 0: all */
/* Host only, no device needed: RTMODT_OK for warp[n_streams][6] (row-major 2x3 [R | t] per stream, NULL = identity) whose entries
 * are all finite and whose |det R| >= 1e-6, RTMODT_E_INVALID otherwise.  The update calls apply it before anything is launched. */
int rtmodt_botsort_check_warp(const float *warp, int n_streams);
/* One frame for every stream (H.2 row 3): detections as rtmodt_ocsort_update_batch takes them, then frames + geometry OR desc as
 * rtmodt_deepsort_update_batch takes them (neither on a motion-only handle), then warp[n_streams][6] (host; row-major 2x3 per stream,
 * the image motion from the previous frame to this one; NULL = identity).  n_returned_out[n_streams] (may be NULL) = the tracks
 * with flag 2 after the frame. */
int rtmodt_botsort_update_batch(rtmodt_botsort *bot, const float *xyxy, const float *conf, const int32_t *cls, const int32_t *n,
                                const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind, const int8_t *desc,
                                const float *warp, int32_t *n_returned_out);
/* The same on the device-resident detections of det's last enqueue_batch (H.2 row 3; stream i <- frame i), queued on det's HIP
 * stream behind its NMS as rtmodt_deepsort_update_from_detector is; frames = NULL on a motion-only handle.  warp[n_frames][6]
 * travels in the kernel's arguments: it is read before the call returns and never blocks that stream. */
int rtmodt_botsort_update_from_detector(rtmodt_botsort *bot, rtmodt_detector *det, const uint8_t *const *frames, int n_frames, int h,
                                        int w, int stride_bytes, int mem_kind, const float *warp);
/* A stream's tracks in list order (H.2 row 3; creation order, deletions compacted); arrays sized max_tracks, any may be NULL.
 * flag: 1 new, 2 tracked, 3 lost; xyxy / conf / cls: the last matched detection; mean[n][8] = (cx, cy, w, h, vx, vy, vw, vh);
 * cov[n][20] = the upper triangle, row-major ((0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)), of the covariance block
 * of (cx, cy, vx, vy), then that of (w, h, vw, vh); feat16[n][dim] / feat8[n][dim] = the smoothed feature at norm 16256 / 127
 * (untouched on a motion-only handle).  A track is returned when flag == 2.  On a stream in (sticky) error the outputs are still
 * filled in before RTMODT_E_CAPACITY is returned. */
int rtmodt_botsort_state(rtmodt_botsort *bot, int stream, int64_t *ids, int32_t *flag, int32_t *age, int32_t *tsu, int32_t *start_frame,
                         int32_t *last_frame, float *xyxy, float *conf, int32_t *cls, float *mean, float *cov, int16_t *feat16,
                         int8_t *feat8, int32_t *n, int64_t *next_id, int64_t *frame_count);
/* Device time (ms, HIP events) of the last update's three parts (H.2 row 3): descriptors (0 without frames), distance, update. */
int rtmodt_botsort_last_ms(rtmodt_botsort *bot, float *describe_ms, float *distance_ms, float *update_ms);

/* ---- camera-motion estimation for BoT-SORT: the warp of rtmodt_botsort_update_*, computed from two consecutive frames on the device ---- */
/* csrc/gmc.hip states the rules (integer luma pyramid, coarse translation by SAD on level 1, 16 x 16 block matching on level 0 with a
 * parabolic sub-pixel step, a fixed sequence of two-point hypotheses, a similarity refitted twice from exact integer sums),
 * tests/gmc_ref.py restates them and the kernels equal that restatement bit for bit.  PARITY UNPINNED: OpenCV and BoT-SORT's GMC
 * (sparse optical flow / ORB / ECC + estimateAffinePartial2D) are installed nowhere this runs; DESIGN.md section 23 lists the deliberate
 * differences.  Six launches per call whatever the counts.  Limits: 64 streams, 4096 blocks per stream, frames up to 3840 x 2160,
 * 1024 mask boxes per stream; beyond them RTMODT_E_CAPACITY, never a fault.  The smallest frame accepted has a level 1 of
 * (2 coarse_search + 4) pixels each way, i.e. w, h >= 4 downscale (2 coarse_search + 4); below that RTMODT_E_INVALID.  BGR24 only. */
typedef struct rtmodt_gmc_cfg {
    int32_t downscale;        /* 4: level 0 is the d x d box average of the luma, d in {1, 2, 4, 8}                                  */
    int32_t coarse_search;    /* 8: the coarse translation is searched over |dx|, |dy| <= coarse_search level-1 pixels, 0..16: it
                               * reaches 4 downscale coarse_search pixels a frame                                                     */
    int32_t search;           /* 4: a block is searched over |dx|, |dy| <= search level-0 pixels around the coarse shift, 1..8        */
    int32_t min_texture;      /* 256: both gradient sums of a 16 x 16 block must reach it                                            */
    int32_t max_sad;          /* 4096: the best SAD of a block must not exceed it                                                    */
    float mask_conf;          /* 0.1: a box with conf >= mask_conf masks the blocks it meets                                         */
    int32_t n_hyp;            /* 128: two-point hypotheses drawn, 1..256                                                             */
    uint32_t seed;            /* 1: of the stated generator; the same inputs give the same warp, call after call                     */
    float min_sep;            /* 32: a hypothesis whose two block centres are closer than this (pixels) is rejected                   */
    float inlier_px;          /* 1.5: a correspondence within this residual (pixels) of the model is an inlier                        */
    int32_t min_blocks;       /* 16: fewer valid blocks give the identity (status 2), >= 2                                           */
    int32_t min_inliers;      /* 12: fewer inliers give the identity (status 3), >= 2                                                */
    int32_t max_boxes;        /* mask boxes per stream of rtmodt_gmc_estimate_batch, 0..1024                                         */
    int32_t n_streams, device;
} rtmodt_gmc_cfg;
/* Host only: the defaults above, max_boxes 1024, one stream, device 0.  PARITY UNPINNED (no OpenCV / GMC here). */
void rtmodt_gmc_default_cfg(rtmodt_gmc_cfg *cfg);
/* PARITY UNPINNED (no OpenCV / GMC here).  The pyramid buffers are carved at the first estimate, for its frame size. */
int rtmodt_gmc_create(const rtmodt_gmc_cfg *cfg, rtmodt_gmc **out);
void rtmodt_gmc_destroy(rtmodt_gmc *gmc);
/* Forgets the previous frame of a stream (stream < 0: all): its next frame returns the identity with status 1.  Once every stream is
 * reset the frame size may change. */
int rtmodt_gmc_reset(rtmodt_gmc *gmc, int stream);
/* One BGR24 frame for every stream, as rtmodt_deepsort_update_batch takes frames (PARITY UNPINNED).  mask_xyxy[n_streams][max_boxes][4],
 * mask_conf[n_streams][max_boxes], mask_n[n_streams]: host arrays, all may be NULL (no mask).  warp_out[n_streams][6]: row-major 2x3
 * [a, -b, tx; b, a, ty], previous frame to this one, full-resolution pixels; status_out[n_streams]: 0 estimated, 1 first frame,
 * 2 too few valid blocks, 3 too few inliers, 4 scale outside [0.5, 2]; with a status other than 0 the warp is exactly the identity,
 * so the output always passes rtmodt_botsort_check_warp.  A frame size other than the previous call's without a reset of every
 * stream, or a frame below the smallest accepted, is RTMODT_E_INVALID; beyond a limit RTMODT_E_CAPACITY; both before any launch. */
int rtmodt_gmc_estimate_batch(rtmodt_gmc *gmc, const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind,
                              const float *mask_xyxy, const float *mask_conf, const int32_t *mask_n, float *warp_out, int32_t *status_out);
/* The same for the frames of det's last enqueue_batch (stream i <- frame i), masked with its device-resident detections, queued on
 * det's HIP stream behind its NMS: no copy of the detections, no wait (PARITY UNPINNED).  rtmodt_gmc_result fetches. */
int rtmodt_gmc_estimate_from_detector(rtmodt_gmc *gmc, rtmodt_detector *det, const uint8_t *const *frames, int n_frames, int h, int w,
                                      int stride_bytes, int mem_kind);
/* Waits for the last estimate and copies warp_out[n_streams][6] / status_out[n_streams] (either may be NULL). */
int rtmodt_gmc_result(rtmodt_gmc *gmc, float *warp_out, int32_t *status_out);
/* Every intermediate of a stream's last frame the tests compare with tests/gmc_ref.py; any pointer may be NULL.  With W0 = w / d,
 * H0 = h / d, W1 = W0 / 4, H1 = H0 / 4, nb = (W0 / 16) (H0 / 16): l0[H0][W0], l1[H1][W1] of the current frame; coarse_table[1089]
 * ((2 cs + 1)^2 entries used, [dy + cs][dx + cs]); coarse_shift[2] = (dx, dy); blk[6][nb] = reason, dx, dy, offx, offy, sad;
 * order[nb] (n_valid used); hyp_score[256] (-1: rejected or not drawn); best_k; inliers[2][nb] (bytes, compacted order, both rounds);
 * sums[2][8] = N, SPx, SPy, SQx, SQy, S(P.Q), S(PxQ), S|P|^2; model[3][4] = a, b, tx, ty (1/16 pixel) of the winning hypothesis and
 * of both refits.  After a first frame only l0 and l1 are defined.  Stages not reached leave zeros (best_k -1). */
int rtmodt_gmc_debug(rtmodt_gmc *gmc, int stream, uint8_t *l0, uint8_t *l1, int32_t *coarse_table, int32_t *coarse_shift, int32_t *blk,
                     int32_t *order, int32_t *n_valid, int32_t *hyp_score, int32_t *best_k, uint8_t *inliers, int64_t *sums, double *model);
/* Device time (ms, HIP events) of the last estimate's six launches. */
int rtmodt_gmc_last_ms(rtmodt_gmc *gmc, float *estimate_ms);
/* rtmodt_botsort_update_from_detector with the warp estimated by gmc from the same frames (PARITY UNPINNED): the estimate and the
 * update are queued on det's stream, botsort_update reads the six floats of stream s from the estimator's device buffer, nothing
 * crosses the host.  frames are required (the estimator reads them; a handle with an embedder describes the detections on them). */
int rtmodt_botsort_update_from_detector_gmc(rtmodt_botsort *bot, rtmodt_detector *det, rtmodt_gmc *gmc, const uint8_t *const *frames,
                                            int n_frames, int h, int w, int stride_bytes, int mem_kind);

/* ---- the embedder of default.yaml:60 (`tracking.deepsort.embedder: "weights/osnet_x0_25.onnx"`): OSNet x0.25 on the GPU ---- */
/* csrc/reid.hip states the crop rule, the rounding contract and the launches; tests/reid_ref.py restates them.  PINNED: the crop
 * and the int8 quantiser exactly, the network within a measured fp16 bound of float64 (profiles/reid/README.md).  PARITY
 * UNPINNED: torchreid, cv2.resize and deep_sort_realtime are installed nowhere this runs.  The weight file is the project's
 * .rtreid (reid_weights.py; tools/convert_weights.py --reid converts a torchreid checkpoint); an .onnx file is not read. */
typedef struct rtmodt_reid_cfg {
    const char *weight_path;    /* default.yaml:60: the .rtreid file                                                             */
    int32_t device;
    int32_t max_frames;         /* frames per call, 1..64                                                                        */
    int32_t max_boxes;          /* boxes per frame, 1..1024; max_frames * max_boxes <= 8192 (2.9 MB of device memory per crop)   */
} rtmodt_reid_cfg;
/* default.yaml:60.  A missing, foreign or damaged file (CRC-32 digest) and non-positive sizes are RTMODT_E_INVALID, sizes past
 * the limits RTMODT_E_CAPACITY -- all before the device is touched. */
int rtmodt_reid_create(const rtmodt_reid_cfg *cfg, rtmodt_reid **out);
/* default.yaml:60.  Frames and boxes as rtmodt_appearance_describe: xyxy[n_frames][max_boxes][4], n_boxes[n_frames].  Outputs
 * (host): desc[n_frames][max_boxes][512] int8 and, when not NULL, feat[n_frames][max_boxes][512] float32 (the network's
 * feature after fc); rows past n_boxes and rows of empty boxes are zero.  n_frames > max_frames, max_boxes or n_boxes past the
 * handle's: RTMODT_E_CAPACITY before anything is launched.  The number of launches does not depend on the boxes. */
int rtmodt_reid_embed(rtmodt_reid *r, const uint8_t *const *frames, int n_frames, int h, int w, int stride_bytes, int mem_kind,
                      const float *xyxy, const int32_t *n_boxes, int max_boxes, float *feat, int8_t *desc);
/* default.yaml:60.  One of the 13 tensors the last embed left in HBM, for every crop slot of the handle ([max_frames][max_boxes]
 * rows): "crop" uint8 [256][128][3] RGB; "conv1" [128][64][16], "maxpool" [64][32][16], "conv2.0" / "conv2.1" [64][32][64],
 * "conv2.2" [32][16][64], "conv3.0" / "conv3.1" [32][16][96], "conv3.2" [16][8][96], "conv4.0" / "conv4.1" / "conv5"
 * [16][8][128], all fp16 NHWC; "feat" float32 [512].  *needed = the size in bytes; copied when out is not NULL and out_bytes
 * suffices (else RTMODT_E_CAPACITY).  Rows of slots without a box, or with an empty one, hold stale bytes (feat: zeros). */
int rtmodt_reid_tap(rtmodt_reid *r, const char *name, void *out, size_t out_bytes, size_t *needed);
/* default.yaml:60.  Device time (ms, HIP events) of the last embed: the crop kernel, and everything after it. */
int rtmodt_reid_last_ms(rtmodt_reid *r, float *crop_ms, float *net_ms);
void rtmodt_reid_destroy(rtmodt_reid *r);   /* default.yaml:60 */
/* default.yaml:60.  The network's input values as the library builds them on the host: out[v][c] = RNE16((v / 255 - mean_c) /
 * std_c) evaluated in float32, as float32[256][3] (c in R, G, B; ImageNet mean and std).  Needs no device and no handle; a
 * buffer smaller than 3072 bytes is RTMODT_E_INVALID. */
int rtmodt_reid_norm_table(float *out, size_t out_bytes);

/* ---- zone events: replaces ZoneEventEngine.process (src/events/zone_engine.py:82-132) -------- */
/* One polygon zone (zone_engine.py:50-58, :142-151).  `key` = index of the FIRST zone carrying the
 * same name: the reference keys its occupancy and cooldown dicts by zone name (:98-100, :105), so
 * same-named zones share their timers; distinct names -> key == own index. */
typedef struct rtmodt_zone_cfg {
    const int32_t *polygon_xy;  /* n_points x (x, y), int32 like np.array(cfg["polygon"], dtype=np.int32) (:143) */
    int32_t n_points;
    double dwell_time_sec;      /* default 2.0  (:147) */
    double cooldown_sec;        /* default 10.0 (:148) */
    int32_t key;
} rtmodt_zone_cfg;
/* n_streams independent ledgers (occupancy + cooldown per track id and zone), at most 32 zones /
 * 2048 polygon points.  max_idle_frames: a track id not passed for more than this many frames loses
 * its cooldown entries (the reference never drops them, zone_engine.py:76; pass INT64_MAX/2 to
 * mirror that until the 2 x max_tracks ledger fills -> RTMODT_E_CAPACITY).  "More than": an id
 * passed at frame_id f with f - (frame_id it was last passed at) > max_idle_frames has lost them,
 * whether or not a call was made in between; with 0 no cooldown entry outlives a frame.
 * A frame passes while its tracks + the retained idle rows <= 2 x max_tracks.  The frame that
 * exceeds it, and one with more than max_events events, returns RTMODT_E_CAPACITY and leaves that
 * stream in error for good: every later _process, _process_tracker and _state that touches the
 * stream returns RTMODT_E_CAPACITY again (the idle rows were dropped to make room, so its cooldown
 * ledger is no longer what the caller built up).  Destroy the handle and create a larger one. */
int rtmodt_zones_create(int device, const rtmodt_zone_cfg *zones, int n_zones, int n_streams, int max_tracks,
                        int max_events, int64_t max_idle_frames, rtmodt_zones **out);
void rtmodt_zones_destroy(rtmodt_zones *z);
/* process(tracks, frame_id) for one stream on a caller-supplied track list (any order, unique ids);
 * `now` = the reference's time.time() (:84).  Events come back in the reference's order (track
 * order, then zone order): ev_track = index into the caller's list, ev_zone = zone index,
 * ev_dwell = now - first_seen (the reference rounds it to 2 decimals when it builds the record,
 * :113), ev_centroid[2] = int((x1+x2)/2), int((y1+y2)/2) (:91-92).  Outputs sized max_events. */
int rtmodt_zones_process(rtmodt_zones *z, int stream, const int64_t *track_ids, const float *xyxy,
                         const int32_t *cls, int n, double now, int64_t frame_id, int32_t *ev_track,
                         int32_t *ev_zone, double *ev_dwell, int32_t *ev_centroid, int32_t *n_events);
/* The same for every stream of `trk` at once, straight on its device-resident state and on the
 * HIP stream its last update ran on (no host round trip for the tracks).  The tracks "passed" are
 * those with time_since_update == report_tsu after the update (1 = matched or spawned this frame;
 * 0 = what the reference's tracker returns, i.e. none -- SURVEY finding 4).  Outputs are
 * [n_streams][max_events] (+ [4] / [2] for xyxy / centroid), n_events[n_streams]. */
int rtmodt_zones_process_tracker(rtmodt_zones *z, rtmodt_tracker *trk, double now, int64_t frame_id,
                                 int report_tsu, int64_t *ev_track_id, int32_t *ev_zone, double *ev_dwell,
                                 float *ev_xyxy, int32_t *ev_centroid, int32_t *ev_cls, int32_t *n_events);
/* Ledger snapshot of one stream, rows in ascending track id (= _occupancy and _cooldown, :74-76):
 * occ_mask bit k <=> zone key k is in _occupancy[track]; first_seen / last_alert are
 * [rows][n_zones] indexed by key (last_alert 0.0 = no entry).  Arrays sized 2 x max_tracks rows. */
int rtmodt_zones_state(rtmodt_zones *z, int stream, int64_t *ids, uint32_t *occ_mask, double *first_seen,
                       double *last_alert, int32_t *n);

/* ---- crossing counter: directional line and gate counts on device-resident tracks ----------- */
/* Completes what config/default.yaml:73-77 offers (`exit_gate`: trigger "crossing", direction "left_to_right") and the
 * reference never implements: zone_engine.py:150 parses `direction` and nothing reads it, so its "crossing" zone is an intrusion
 * zone under another name.  csrc/crossing.hip, one launch per frame for all streams; tests/crossing_ref.py states the rules and the
 * kernel equals it exactly ("Crossing counter").  PARITY UNPINNED against any third-party counter.
 * Centroid = the zone engine's (int((x1+x2)/2), int((y1+y2)/2) in float32), clamped to [-2^20, 2^20]; a track whose box has a
 * non-finite coordinate is not passed that frame.  Line endpoints and gate vertices outside that range are RTMODT_E_INVALID. */
#define RTMODT_LINE_BOTH 0
#define RTMODT_LINE_POS 1   /* the crossing ends on the side where (B - A) x (P - A) > 0 */
#define RTMODT_LINE_NEG 2
#define RTMODT_GATE_ANY 0   /* no direction: every exit fires */
#define RTMODT_GATE_LEFT_TO_RIGHT 1
#define RTMODT_GATE_RIGHT_TO_LEFT 2
#define RTMODT_GATE_TOP_TO_BOTTOM 3
#define RTMODT_GATE_BOTTOM_TO_TOP 4
#define RTMODT_CROSSING_LINE 0
#define RTMODT_CROSSING_GATE 1
typedef struct rtmodt_crossing rtmodt_crossing;
/* A tripwire: the directed segment A -> B.  A passed track with centroid P crosses it when P is off the infinite line, the last
 * non-zero side stored for the track differs from P's, and the path from the previous passed centroid to P meets the closed
 * segment.  `direction` selects which crossings are counted and reported (RTMODT_LINE_*). */
typedef struct rtmodt_line_cfg {
    int32_t ax, ay, bx, by;
    int32_t direction;
} rtmodt_line_cfg;
/* A gate: a polygon (the zone engine's inside-or-on test) and an optional direction (RTMODT_GATE_*): the zone of default.yaml:73-77.
 * It fires when a track leaves it and the displacement from the centroid it entered at agrees with the direction (dominant axis,
 * ties included: left_to_right is dx > 0 and dx >= |dy|). */
typedef struct rtmodt_gate_cfg {
    const int32_t *polygon_xy;  /* n_points x (x, y) */
    int32_t n_points;
    int32_t direction;
} rtmodt_gate_cfg;
/* One crossing.  `track`: index into the caller's list (rtmodt_crossing_process) or into the tracker's list.  `direction`:
 * RTMODT_LINE_POS / _NEG for a line, the gate's own direction for a gate.  `prev`: the previous passed centroid (line) or the entry
 * centroid (gate); `frames`: frame_id minus the frame of that point. */
typedef struct rtmodt_crossing_event {
    int64_t track_id;
    int64_t frames;
    float xyxy[4];
    int32_t centroid[2];
    int32_t prev[2];
    int32_t track, kind, index, direction, cls, reserved;
} rtmodt_crossing_event;
/* n_streams independent ledgers and count sets; at most 32 lines, 32 gates, 2048 gate vertices, n_classes in 1..256 (a crossing
 * whose class id lies outside [0, n_classes) enters the totals only).  A ledger row (per track id: last passed frame, previous
 * centroid, last non-zero side per line, inside bit + entry centroid and frame per gate) is dropped once frame_id - (the frame it
 * was last passed at) > max_gap_frames; the id then starts fresh and causes no crossing on the frame it returns.  Within the gap the
 * row is kept as it is.  A ledger holds 2 x max_tracks rows: the frame that needs more returns RTMODT_E_CAPACITY, the idle rows are
 * dropped to make room, and the stream stays in error for good (every later _process*, and _state, of that stream returns
 * RTMODT_E_CAPACITY; the counts remain readable, and passed tracks that cross keep entering them).  Destroy the handle and create a larger
 * one.  Track ids are taken to name one object for the handle's lifetime: after rtmodt_tracker_reset / rtmodt_deepsort_reset / rtmodt_ocsort_reset, or with a new
 * tracker handle, ids start again at 1, so create a new counter with it (rows kept within the gap would be taken for the new tracks). */
int rtmodt_crossing_create(int device, const rtmodt_line_cfg *lines, int n_lines, const rtmodt_gate_cfg *gates, int n_gates,
                           int n_classes, int n_streams, int max_tracks, int max_events, int64_t max_gap_frames,
                           rtmodt_crossing **out);
/* Waits for the work queued on the handle's own stream, then frees the ledgers, the counts and the handle; null is allowed. */
void rtmodt_crossing_destroy(rtmodt_crossing *c);
/* One stream, a caller-supplied track list (any order, unique ids, at most max_tracks); every listed track is passed.  Events come
 * back in (list order, lines in order, gates in order); `events` holds max_events records.  A frame with more events returns
 * RTMODT_E_CAPACITY with the first max_events of them delivered and the counts complete; the stream goes on working. */
int rtmodt_crossing_process(rtmodt_crossing *c, int stream, const int64_t *track_ids, const float *xyxy, const int32_t *cls,
                            int n, int64_t frame_id, rtmodt_crossing_event *events, int32_t *n_events);
/* default.yaml:73-77 on every stream of a ByteTrack handle at once, straight on its device-resident state and on the HIP stream its
 * last update ran on.  Passed = time_since_update == report_tsu (1 = matched or spawned this frame, as rtmodt_zones_process_tracker).
 * events is [n_streams][max_events], n_events[n_streams]. */
int rtmodt_crossing_process_tracker(rtmodt_crossing *c, rtmodt_tracker *trk, int64_t frame_id, int report_tsu,
                                    rtmodt_crossing_event *events, int32_t *n_events);
/* The same on a DeepSORT handle (zone_engine.py:150 never reached any tracker's state): passed = confirmed and
 * time_since_update == report_tsu (0 = matched this frame); the box is the matched detection's (rtmodt_deepsort_state: xyxy). */
int rtmodt_crossing_process_deepsort(rtmodt_crossing *c, rtmodt_deepsort *ds, int64_t frame_id, int report_tsu,
                                     rtmodt_crossing_event *events, int32_t *n_events);
/* The same on an OC-SORT handle: passed = the tracks that handle returns this frame (rtmodt_ocsort_state); the box is the matched
 * detection's. */
int rtmodt_crossing_process_ocsort(rtmodt_crossing *c, rtmodt_ocsort *oc, int64_t frame_id, rtmodt_crossing_event *events,
                                   int32_t *n_events);
/* The same on a BoT-SORT handle (H.2 row 3): passed = the returned tracks (flag 2) matched this frame (tsu == 0); the box is the
 * matched detection's. */
int rtmodt_crossing_process_botsort(rtmodt_crossing *c, rtmodt_botsort *bot, int64_t frame_id, rtmodt_crossing_event *events,
                                    int32_t *n_events);
/* One stream's counts since creation or the last reset (default.yaml:73-77): line_total [n_lines][2] (pos, neg),
 * line_class [n_lines][2][n_classes], gate_total [n_gates], gate_class [n_gates][n_classes]; any pointer may be null. */
int rtmodt_crossing_counts(rtmodt_crossing *c, int stream, int64_t *line_total, int64_t *line_class, int64_t *gate_total,
                           int64_t *gate_class);
/* Zeroes the counts of every stream; the ledgers stay (a track halfway through a gate still fires on exit). */
int rtmodt_crossing_reset_counts(rtmodt_crossing *c);
/* Ledger snapshot of one stream, rows in ascending track id (the parity surface of tests/crossing_ref.py): side_pos / side_neg bit l
 * <=> the side stored for line l is +1 / -1; inside bit g <=> the track is in gate g, and then entry_xy[row][g] / entry_frame[row][g]
 * hold where and when it entered (other cells are unspecified).  Arrays sized 2 x max_tracks rows. */
int rtmodt_crossing_state(rtmodt_crossing *c, int stream, int64_t *ids, int64_t *last_frame, int32_t *prev_xy, uint32_t *side_pos,
                          uint32_t *side_neg, uint32_t *inside, int32_t *entry_xy, int64_t *entry_frame, int32_t *n);

/* ---- speed estimator: track speed and proximity on a ground plane ---------------------------- */
/* How fast tracked objects move in real units, and which two are closer than d metres: the speeding / stopped-vehicle / wrong-way
 * alarms, the speed histogram (85th percentile) and the near-miss pairs that traffic and site-safety deployments ask for.  The
 * reference has nothing of the kind (its Track carries no velocity).  csrc/speed.hip: one launch per call for the ledgers and alarms
 * of all streams, one more for the pairs when proximity_mm > 0; csrc/ground_plane.h states the per-point rules (anchor, projection,
 * integer distance and speed), the header of speed.hip the ledger rules; tests/speed_ref.py restates both and the kernels equal it
 * exactly.  PARITY UNPINNED against Ultralytics' SpeedEstimator / DistanceCalculation.
 * A FIXED camera and ONE ground plane per stream: no PTZ, no camera-motion compensation, no lens model (rectify the frames first: the
 * lens correction section at the end of this header).
 * Every call carries a timestamp in microseconds per stream, strictly increasing per stream (else RTMODT_E_INVALID, nothing
 * changes).  A box is SAMPLED when its class passes the filter, its coordinates are finite and its anchor projects onto the plane
 * (ground_plane.h); only sampled tracks touch the ledger. */
#define RTMODT_SPEED_FOOT 0     /* anchor ((x1 + x2) / 2, y2): the point on the ground (default) */
#define RTMODT_SPEED_CENTRE 1   /* anchor ((x1 + x2) / 2, (y1 + y2) / 2) */
#define RTMODT_SPEED_EV_SPEEDING 0
#define RTMODT_SPEED_EV_STOPPED 1
#define RTMODT_SPEED_EV_WRONG_WAY 2
/* row flags: bits 0..2 = the alarm of that kind has fired and not re-armed; bit 3 = the stop timer runs; bit 4 = the row was
 * created by this call */
#define RTMODT_SPEED_F_TIMER 8
#define RTMODT_SPEED_F_NEW 16
typedef struct rtmodt_speed rtmodt_speed;
typedef struct rtmodt_speed_cfg {
    int32_t anchor;             /* RTMODT_SPEED_FOOT | RTMODT_SPEED_CENTRE */
    int32_t window;             /* 2..32: ring of the last `window` samples (X, Y, t_us) per track */
    int32_t min_samples;        /* 2..window: speed is -1 (unknown) with fewer samples in the ring */
    int32_t hold;               /* >= 1: SPEEDING / WRONG_WAY need this many consecutive samples */
    int64_t max_gap_us;         /* >= 0: a row not sampled for longer is dropped, the id starts fresh */
    int64_t stop_us;            /* >= 0: STOPPED needs the speed below stop_mm_s for this long */
    int32_t min_step_mm;        /* >= 0: the odometer gains a step only when it is at least this long (dead band against box jitter) */
    int32_t limit_mm_s;         /* SPEEDING: speed > limit; 0 = off */
    int32_t stop_mm_s;          /* STOPPED: 0 <= speed < stop_mm_s; 0 = off */
    int32_t wrong_way_min_mm_s; /* WRONG_WAY needs at least this speed */
    int32_t allowed_dir[2];     /* WRONG_WAY: world direction of travel, |.| <= 2^20; (0, 0) = off */
    int32_t bins, bin_mm_s;     /* speed histogram: bins 0..256 (0 = none) of bin_mm_s >= 1 each, the last one open-ended */
    int32_t proximity_mm;       /* 0..2^30: pairs closer than this are reported; 0 = off */
    int32_t max_pairs;          /* >= 1 */
    int32_t max_events;         /* >= 1 */
    int32_t n_classes;          /* with `classes`: only these class ids are sampled (at most 256); classes == NULL: all */
    const int32_t *classes;
} rtmodt_speed_cfg;
/* One sampled track of this call, in list order.  `track`: index into the caller's list, or into the tracker's list.  speed_mm_s:
 * the chord from the oldest ring sample to the newest over their time difference, -1 while unknown; heading: that chord (dx, dy) in
 * mm, (0, 0) while unknown; peak_mm_s: the largest speed of the row so far (-1: none). */
typedef struct rtmodt_speed_row {
    int64_t track_id;
    int64_t odometer_mm;
    int32_t track, cls;
    int32_t world[2];
    int32_t speed_mm_s, peak_mm_s;
    int32_t heading[2];
    int32_t flags, n_samples;
} rtmodt_speed_row;
/* One alarm.  `value`: the speed in mm/s at the moment it fired; `track` as in the row. */
typedef struct rtmodt_speed_event {
    int64_t track_id;
    int64_t t_us;
    float xyxy[4];
    int32_t world[2];
    int32_t kind, value, cls, track;
} rtmodt_speed_event;
/* Two sampled tracks closer than proximity_mm (compared on the squared integers); a < b index the rows of this call. */
typedef struct rtmodt_speed_pair {
    int64_t track_a, track_b;
    int32_t a, b;
    int32_t dist_mm;            /* isqrt of the squared distance */
    int32_t reserved;
} rtmodt_speed_pair;
/* What one call hands back; the struct pointer and every member may be null.  With none given nothing crosses to the host and the
 * call does not wait for the device; otherwise the streams' result blocks come back in one copy.  One-stream calls: rows
 * [max_tracks], events [max_events], pairs [max_pairs], counts [1]; all-stream calls: [n_streams][...] and counts [n_streams].
 * n_pairs is the number delivered (<= max_pairs), total_pairs the number that exist. */
typedef struct rtmodt_speed_out {
    rtmodt_speed_row *rows;
    int32_t *n_rows;
    rtmodt_speed_event *events;
    int32_t *n_events;
    rtmodt_speed_pair *pairs;
    int32_t *n_pairs;
    int32_t *total_pairs;
} rtmodt_speed_out;
/* n_streams independent ledgers, histograms and planes; max_tracks <= 4096.  A ledger holds 2 x max_tracks rows, sorted by track
 * id, with the crossing counter's capacity behaviour: the call that needs more returns RTMODT_E_CAPACITY, the idle rows are dropped
 * to make room and the stream stays in error for good (every later call that asks for output, and _state, returns
 * RTMODT_E_CAPACITY).  More alarms than max_events or more pairs than max_pairs in one call: RTMODT_E_CAPACITY with the first ones
 * delivered and the counts reported; the stream goes on working.  A call made without outputs cannot report either; a ledger it
 * filled surfaces in the next call that asks for output.  The rules per sampled track, in this order:
 *   ring    the sample (X, Y, t_us) enters the ring (the oldest leaves once `window` are held);
 *   odo     the step from the odometer's anchor point (the first sample, then every sample that moved it) is isqrt of the squared
 *           distance; if step >= min_step_mm the odometer gains it and the anchor moves here;
 *   speed   as in rtmodt_speed_row; the histogram bin min(speed / bin_mm_s, bins - 1) gains one whenever the speed is known;
 *   SPEEDING   speed > limit_mm_s on `hold` consecutive samples fires once; re-arms when speed <= limit_mm_s (or unknown);
 *   STOPPED    0 <= speed < stop_mm_s starts a timer at this sample; fires once when t_us - start >= stop_us; anything else stops
 *              the timer and re-arms;
 *   WRONG_WAY  speed >= wrong_way_min_mm_s and heading . allowed_dir < 0 on `hold` consecutive samples fires once; re-arms when the
 *              condition fails.
 * Events leave in list order, kinds in the order above. */
int rtmodt_speed_create(int device, const rtmodt_speed_cfg *cfg, int n_streams, int max_tracks, rtmodt_speed **out);
/* Waits for the handle's queued work, frees everything; null is allowed. */
void rtmodt_speed_destroy(rtmodt_speed *h);
/* The image-pixel -> world-millimetre homography of one stream, row-major.  Non-finite entries or a singular matrix:
 * RTMODT_E_INVALID.  A stream without a plane makes every _process* that touches it return RTMODT_E_INVALID. */
int rtmodt_speed_set_plane(rtmodt_speed *h, int stream, const double H[9]);
/* The Ultralytics-style shorthand: H = diag(s, s, 1), s = mm_per_pixel, finite and > 0. */
int rtmodt_speed_set_scale(rtmodt_speed *h, int stream, double mm_per_pixel);
/* Host only, no device needed: fits H to n >= 4 correspondences image (u, v) -> world (x, y) mm by a normalised DLT (float64,
 * Gaussian elimination with partial pivoting).  *max_residual_mm (may be null) = the largest reprojection residual, so that a bad
 * survey shows.  Degenerate input (n < 4, three of four points collinear, repeated points): RTMODT_E_INVALID. */
int rtmodt_speed_fit_plane(const double *img_xy, const double *world_xy, int n, double H_out[9], double *max_residual_mm);
/* One stream, a caller-supplied track list (any order, unique ids, at most max_tracks). */
int rtmodt_speed_process(rtmodt_speed *h, int stream, const int64_t *track_ids, const float *xyxy, const int32_t *cls, int n,
                         int64_t t_us, const rtmodt_speed_out *out);
/* Every stream in one call: track_ids / cls [n_streams][stride], xyxy [n_streams][stride][4], n [n_streams], t_us [n_streams]. */
int rtmodt_speed_process_batch(rtmodt_speed *h, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n,
                               int stride, const int64_t *t_us, const rtmodt_speed_out *out);
/* Every stream of a ByteTrack handle, straight on its device-resident state and on the HIP stream its last update ran on: exactly
 * the tracks and boxes rtmodt_crossing_process_tracker passes.  t_us [n_streams of the tracker]. */
int rtmodt_speed_process_tracker(rtmodt_speed *h, rtmodt_tracker *trk, const int64_t *t_us, int report_tsu, const rtmodt_speed_out *out);
/* The same on a DeepSORT handle: the tracks rtmodt_crossing_process_deepsort passes. */
int rtmodt_speed_process_deepsort(rtmodt_speed *h, rtmodt_deepsort *ds, const int64_t *t_us, int report_tsu, const rtmodt_speed_out *out);
/* The same on an OC-SORT handle: the tracks rtmodt_crossing_process_ocsort passes. */
int rtmodt_speed_process_ocsort(rtmodt_speed *h, rtmodt_ocsort *oc, const int64_t *t_us, const rtmodt_speed_out *out);
/* The same on a BoT-SORT handle: the tracks rtmodt_crossing_process_botsort passes. */
int rtmodt_speed_process_botsort(rtmodt_speed *h, rtmodt_botsort *bot, const int64_t *t_us, const rtmodt_speed_out *out);
/* One stream's speed histogram, hist [bins]; reset != 0 zeroes it after the read (hist may be null then). */
int rtmodt_speed_histogram(rtmodt_speed *h, int stream, int64_t *hist, int reset);
/* Ledger snapshot of one stream, rows in ascending track id (the parity surface of tests/speed_ref.py); any array may be null.
 * ring_xy [rows][window][2] and ring_t [rows][window] are the ring's slots as stored: ints[row] = {n_samples, head (slot of the newest
 * sample), speed, peak, cls, flags, speeding run, wrong-way run}; the samples are the slots head - n_samples + 1 .. head (mod
 * window), other slots are unspecified.  odo_anchor_xy [rows][2], heading [rows][2], stop_since [rows] (valid while the timer
 * runs).  Arrays sized 2 x max_tracks rows. */
int rtmodt_speed_state(rtmodt_speed *h, int stream, int64_t *ids, int64_t *last_t_us, int64_t *odometer_mm, int64_t *stop_since,
                       int32_t *ring_xy, int64_t *ring_t, int32_t *odo_anchor_xy, int32_t *heading, int32_t *ints, int32_t *n);

/* ---- frame renderer: replaces FrameRenderer.render (src/visualization/renderer.py) ---------- */
/* Annotates BGR24 frames in place, one launch per batch (csrc/render.hip, whose header comment states the paint rules; they
 * restate cv2's drawing calls -- PARITY UNPINNED: no OpenCV to run against).  Per frame, in this order: zone tint (the
 * zone engine's inside-or-on test) blended 0.25 / 0.75 with the frame, zone names drawn into the frame before the blend;
 * then per track in list order: box outline, label box + label text, trail; then the HUD.  Strokes are "every pixel whose
 * centre lies within distance 1 of the segment"; text uses the bundled bitmap fonts of csrc/font_atlas.h. */
typedef struct rtmodt_render_cfg {
    int32_t show_boxes, show_ids, show_trails, show_zones, show_fps;   /* renderer.py:32-38, all 1 by default      */
    int32_t trail_length;           /* 1..1024: a trail draws its last trail_length points (renderer.py:87)             */
    const uint8_t *palette_bgr;     /* n_palette x (B, G, R); NULL = the reference's 20 colours                          */
    int32_t n_palette;              /* 1..256 when palette_bgr is given                                                  */
} rtmodt_render_cfg;
/* One track of a draw list (duck-typed Track: track_id / xyxy / label / trail). */
typedef struct rtmodt_render_track {
    int64_t track_id;               /* colour = palette[track_id mod n_palette], the mod taken as Python's % does          */
    float xyxy[4];                  /* corners int(v) (truncation), clamped to +-2^20; NaN is RTMODT_E_INVALID           */
    const char *label;              /* show_ids: the text above the box (the reference formats "ID:{id} {class_name}
                                     * {conf:.2f}"), NUL-terminated, at most 255 bytes; bytes outside 32..126 draw as '?' */
    const int32_t *trail_xy;        /* n_trail x (x, y), oldest first, each clamped to +-2^20                             */
    int32_t n_trail;
} rtmodt_render_track;
typedef struct rtmodt_render_list {
    const rtmodt_render_track *tracks;
    int32_t n_tracks;               /* at most 65536 per frame                                                           */
} rtmodt_render_list;

int rtmodt_renderer_create(int device, const rtmodt_render_cfg *cfg, rtmodt_renderer **out);
void rtmodt_renderer_destroy(rtmodt_renderer *r);
/* The zones later batches tint (ZoneEventEngine.get_zone_polygons(): name + int32 polygon), uploaded once and cached;
 * n_zones = 0 clears them.  At most 32 zones / 2048 points / 255-byte names, else RTMODT_E_CAPACITY.  A name is drawn at
 * (int(m10 / m00) - 30, int(m01 / m00)) of the polygon's contour moments (float64), nothing when m00 == 0. */
int rtmodt_renderer_set_zones(rtmodt_renderer *r, const int32_t *const *polygons_xy, const int32_t *n_points,
                              const char *const *names, int n_zones);
/* Draws lists[i] onto frames[i] (n frames of h x w, row pitch stride_bytes >= 3w; the bytes past 3w of a row are never
 * touched).  mem_kind RTMODT_MEM_DEVICE: frames are device pointers, drawn in place; RTMODT_MEM_HOST: uploaded, drawn and
 * copied back.  draw_zones = 1: the cached zones are drawn first (when show_zones).  fps / latency_ms feed the HUD
 * ("FPS: %.1f | Latency: %.1fms").  All draw lists travel in one command buffer (one host-to-device copy); returns when
 * the frames are final. */
int rtmodt_render_batch(rtmodt_renderer *r, uint8_t *const *frames, int n, int h, int w, int stride_bytes, int mem_kind,
                        const rtmodt_render_list *lists, int draw_zones, double fps, double latency_ms);
/* Device time (ms, HIP events) of the last render_batch's kernel. */
int rtmodt_renderer_last_ms(rtmodt_renderer *r, float *kernel_ms);
/* The command buffer render_batch would send for these lists (host only, no device needed; frame pointers left 0):
 * *needed = its size; written to out when out_bytes >= *needed.  Layout: csrc/render.hip, "command buffer". */
int rtmodt_render_pack(const rtmodt_render_cfg *cfg, const rtmodt_render_list *lists, int n, int h, int w, int draw_zones,
                       double fps, double latency_ms, void *out, size_t out_bytes, size_t *needed);

/* ---- JPEG / Motion-JPEG encoder: replaces cv2.VideoWriter on the annotated frame (tools/run_pipeline.py:112-117,160-161) ---- */
/* Batches of BGR24 frames (the renderer's frame convention, so render_batch's output is encoded where it lies) become complete
 * baseline JPEG files: JFIF, YCbCr 4:2:0, the Annex K Huffman tables, one restart interval per MCU row (csrc/jpeg.hip, whose
 * header comment states the stream and the integer arithmetic; tests/jpeg_ref.py restates both).  The rules are libjpeg's:
 * PARITY PINNED -- the files equal libjpeg-turbo 3.1's (Pillow, restart_marker_rows=1, optimize=False) byte for byte. */
typedef struct rtmodt_jpeg_cfg {
    int32_t quality;        /* 1..100; 0 = 95 (cv2.imencode's default)                      */
    int32_t subsampling;    /* 0 = 4:2:0, the only one; anything else RTMODT_E_UNSUPPORTED  */
    int32_t max_h, max_w;   /* largest frame the handle is sized for (<= 8192 each)         */
    int32_t max_batch;      /* frames per call                                              */
} rtmodt_jpeg_cfg;
/* Scratch: 768 bytes per MCU of max_batch frames of max_h x max_w (6.3 MB per 1080p frame). */
int rtmodt_jpeg_create(int device, const rtmodt_jpeg_cfg *cfg, rtmodt_jpeg **out);
void rtmodt_jpeg_destroy(rtmodt_jpeg *j);
/* video_writer.write(annotated) (run_pipeline.py:160-161) for n frames of h x w, row pitch stride_bytes >= 3w, mem_kind as in
 * rtmodt_render_batch; the frames are only read.  Frame i's file (SOI .. EOI) is written to out + i * slot_bytes (host memory)
 * and sizes[i] is its length.  RTMODT_E_CAPACITY when n, h or w exceed the handle (nothing launched), and when a file does not
 * fit slot_bytes: the message names the first such frame and the bytes it needs, sizes[i] holds the needed size of every
 * frame, the frames that fit are complete, and no byte past any slot's sizes[i] is touched.  n = 0: success, nothing launched. */
int rtmodt_jpeg_encode_batch(rtmodt_jpeg *j, const uint8_t *const *frames, int n, int h, int w, int stride_bytes, int mem_kind,
                             uint8_t *out, size_t slot_bytes, uint32_t *sizes);
/* Device time (ms, HIP events) of the last encode_batch's kernels. */
int rtmodt_jpeg_last_ms(rtmodt_jpeg *j, float *kernel_ms);
/* Host only, no device needed: everything from SOI up to and including the SOS header of an h x w file at `quality` (1..100).
 * *needed = its size; written to out when out_bytes >= *needed. */
int rtmodt_jpeg_header(int quality, int h, int w, uint8_t *out, size_t out_bytes, size_t *needed);

/* ---- JPEG / Motion-JPEG decoder: replaces `cap.read()` of src/ingestion/rtsp_reader.py (cv2.VideoCapture on an MJPEG camera) and
 * the image upload of web/server.py (cv2.imdecode) ---------------------------------------------------------------------------- */
/* Baseline JPEG files (SOF0, 8 bit, 1 or 3 components, one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0 / gray, any Huffman tables, any
 * DRI; files without DHT use the Annex K tables) become BGR24 frames (csrc/jpeg_dec.hip; the stream rules are in
 * csrc/jpeg_dec_core.h; tests/jpeg_dec_ref.py restates both).  The arithmetic is libjpeg's (islow IDCT, fancy upsampling):
 * PARITY PINNED -- the pixels equal libjpeg-turbo 3.1's default decoder's (Pillow) byte for byte on accepted streams.  UNPINNED: parity
 * with cv2's / cameras' decoders, and everything about damaged streams (statuses below; libjpeg's concealment is not reproduced). */
#define RTMODT_JPEG_OK 0
#define RTMODT_JPEG_UNSUPPORTED 1    /* progressive, extended, lossless, arithmetic, 12 bit, several scans, 4 components, other sampling */
#define RTMODT_JPEG_CORRUPT 2        /* broken structure; a restart marker missing, surplus or misnumbered; an impossible code        */
#define RTMODT_JPEG_TRUNCATED 3      /* the file ends inside the header, or a restart interval ends before its last MCU               */
#define RTMODT_JPEG_SIZE_MISMATCH 4  /* a sound file whose h x w is not the call's                                                    */
typedef struct rtmodt_jpeg_info {
    int32_t status;                  /* RTMODT_JPEG_*; the other fields are valid as far as the header was read                       */
    int32_t h, w, components;
    int32_t h_samp, v_samp;          /* luminance sampling factors: 1x1 (4:4:4, gray), 2x1 (4:2:2), 2x2 (4:2:0)                       */
    int32_t restart_interval;        /* MCUs, 0: none -- such a stream is decoded by ONE GPU lane per frame (slow)                    */
    int32_t reserved;
    char message[96];                /* what is unsupported / wrong, "" when OK                                                       */
} rtmodt_jpeg_info;
/* What `cap.read()` / cv2.imdecode would be asked to decode: reads the header of file[0, bytes) up to and including SOS.  Host only,
 * no device.  Returns RTMODT_OK whenever info was filled (whatever info->status says); RTMODT_E_INVALID for null pointers. */
int rtmodt_jpeg_probe(const uint8_t *file, size_t bytes, rtmodt_jpeg_info *info);
typedef struct rtmodt_jpegdec_cfg {
    int32_t max_h, max_w;            /* largest frame the handle accepts (<= 8192 each)                                               */
    int32_t max_batch;               /* files per call                                                                                */
    int64_t max_file_bytes;          /* largest file; 0 = max_h * max_w * 3 / 4 + 65536.  Page-locked staging: max_batch x this        */
} rtmodt_jpegdec_cfg;
/* The handle behind an MJPEG `cap.read()` (rtsp_reader.py) / the web server's image upload.  Device scratch grows with the calls:
 * 192 bytes per 8x8 block (coefficients + planes) and 4 bytes per restart interval. */
int rtmodt_jpegdec_create(int device, const rtmodt_jpegdec_cfg *cfg, rtmodt_jpegdec **out);
void rtmodt_jpegdec_destroy(rtmodt_jpegdec *dec);
/* `ok, frame = cap.read()` (rtsp_reader.py) / cv2.imdecode of an upload (web/server.py) for n files: files[i][0, sizes[i]) (host
 * memory) is decoded into frames[i], n frames of h x w BGR24 with row pitch stride_bytes >= 3w; only the 3w bytes of a row are
 * written.  mem_kind as in rtmodt_render_batch: RTMODT_MEM_DEVICE frames are device pointers -- directly what
 * rtmodt_detector_enqueue_batch(..., RTMODT_MEM_DEVICE) and rtmodt_render_batch take; RTMODT_MEM_HOST frames are copied back.
 * status[i] (host) = RTMODT_JPEG_*; a frame whose status is not OK has unspecified pixels inside its own rows (here: untouched).
 * The call succeeds when individual files fail.  RTMODT_E_CAPACITY, nothing launched, when n, h, w or a file's size exceeds the
 * handle; RTMODT_E_INVALID for null pointers, stride_bytes < 3w or a bad mem_kind; n = 0: success, nothing launched.  Four
 * launches per call whatever n is; returns when the frames are final. */
int rtmodt_jpegdec_decode_batch(rtmodt_jpegdec *dec, const uint8_t *const *files, const size_t *sizes, int n, uint8_t *const *frames,
                                int h, int w, int stride_bytes, int mem_kind, int32_t *status);
/* Device time (ms, HIP events) of the last decode_batch's kernels (the `cap.read()` cost that moved to the GPU). */
int rtmodt_jpegdec_last_ms(rtmodt_jpegdec *dec, float *kernel_ms);
/* Diagnostics of `cap.read()`'s replacement: the entropy decoder's output for one component of one frame of the last decode_batch,
 * int16 [rows][cols][64] in natural order, not dequantised (whole MCUs).  *rows / *cols are always set; out is written when
 * out_elems >= rows * cols * 64. */
int rtmodt_jpegdec_coefficients(rtmodt_jpegdec *dec, int frame, int component, int16_t *out, size_t out_elems, int *rows, int *cols);

/* ---- offline evaluation: replaces src/evaluation/metrics.py's pycocotools / motmetrics calls --------------------- */
/* PARITY UNPINNED: neither library is installed anywhere this runs.  The rules are restated in csrc/eval.hip's header and
 * INTEGRATION.md section 9 (pycocotools >= 2.0.7 COCOeval bbox, motmetrics >= 1.4.0 CLEAR MOT + IDF1, 'iou' distance);
 * tests/eval_ref.py restates them in NumPy.  Device scratch is allocated and freed inside each call. */

/* COCO bbox evaluate() + accumulate(), float64 throughout.  Thresholds are the caller's arrays, used as given (the
 * Python side builds iouThrs / recThrs with np.linspace, so linspace(.5, .95, 10)[8] == 0.8999999999999999):
 * iou_thrs[T], rec_thrs[R], max_dets[M] (ascending, max_dets[M-1] <= 1024), area_rng[A][2] (lo, hi; A * T <= 256).
 * Cells: the non-empty (category, image) pairs, grouped by category index (cell_cat[n_cells], ascending) and, inside a
 * category, in image order.  gt_start / dt_start[n_cells + 1] are CSR offsets into the GT and detection rows, each
 * cell's rows in file order; boxes are x, y, w, h.  gt_area is the annotation's `area` field (the area-range test), the
 * ignore flag is gt_crowd; gt_id == 0 makes a match count as unmatched (pycocotools' dtm > 0 test).  At most 1024 GTs and
 * 4096 detections per cell, else RTMODT_E_CAPACITY before anything is launched.  Outputs (host):
 * precision[T][R][K][A][M] and recall[T][K][A][M], -1 where a category has no cell or no non-ignored GT -- bit-identical
 * to COCOeval.eval['precision'] / ['recall'] computed in float64 by the stated rules. */
int rtmodt_coco_eval(int device, const double *iou_thrs, int T, const double *rec_thrs, int R, const int32_t *max_dets, int M,
                     const double *area_rng, int A, int K, int n_cells, const int32_t *cell_cat, const int32_t *gt_start,
                     const double *gt_box, const double *gt_area, const int32_t *gt_crowd, const int64_t *gt_id,
                     const int32_t *dt_start, const double *dt_box, const double *dt_score, double *precision, double *recall);

/* One sequence's CLEAR MOT / identity counts (motmetrics' compare_to_groundtruth(..., 'iou', distth=0.5)). */
typedef struct rtmodt_mot_counts {
    int64_t num_frames, num_objects, num_predictions;        /* frames = the union of both files' frame ids          */
    int64_t num_matches, num_switches, num_misses, num_false_positives;
    int64_t mostly_tracked, mostly_lost, num_unique_objects;  /* tracked / present >= 0.8, < 0.2 (float64)            */
    int64_t idtp, idfp, idfn;                                 /* IDTP = max-weight one-to-one pairing of ids (exact)   */
    double dist_sum;                                          /* sum of d = 1 - IoU over MATCH + SWITCH; motp = dist_sum
                                                               * / (num_matches + num_switches)                       */
} rtmodt_mot_counts;
/* A batch of sequences in one launch.  seq_frame_start[n_seq + 1]: CSR into the frames, each sequence's frames ascending
 * (frame_id[] only names a frame in error messages).  gt_start / hyp_start[n_frames + 1]: CSR into the GT / hypothesis
 * rows, boxes x, y, w, h (the MOT file's corner minus 1); gt_oid / hyp_hid are dense ids within the sequence
 * (0..seq_n_oid-1, 0..seq_n_hid-1), unique inside a frame.  Per frame: continuation of last frame's matches, then an
 * assignment of maximum cardinality and, among those, minimum sum of d over pairs with d <= 0.5 (lap.h, lexicographic
 * costs); MATCH / SWITCH / MISS / FP as motmetrics counts them.  Limits: 1024 rows per frame and side (checked before
 * launch); 2^28 valid pairs (d <= 0.5) per call (checked after the count pass, before any pair is written); a frame whose
 * contested remainder exceeds 256 rows / 256 columns / 2048 pairs fails with RTMODT_E_CAPACITY naming the sequence and
 * frame.  The pairs are kept as a per-frame CSR and the IDF1 counts as a sparse (sequence, o, h) table: memory follows
 * the valid pairs, not |O| x |H| or the id counts. */
int rtmodt_mot_eval(int device, int n_seq, const int32_t *seq_frame_start, const int64_t *frame_id, const int32_t *gt_start,
                    const int32_t *hyp_start, const int32_t *gt_oid, const double *gt_box, const int32_t *hyp_hid, const double *hyp_box,
                    const int32_t *seq_n_oid, const int32_t *seq_n_hid, rtmodt_mot_counts *out);

/* HOTA (Luiten et al., IJCV 2021) beside CLEAR MOT and IDF1: csrc/hota.hip restates TrackEval's trackeval/metrics/hota.py.
 * PARITY UNPINNED: TrackEval is installed nowhere this runs; the rules are in csrc/hota.hip's header and INTEGRATION.md
 * section 17, tests/hota_ref.py restates them in plain Python / NumPy (its per-frame matching pinned to
 * scipy.optimize.linear_sum_assignment, the solver TrackEval calls) and the GPU tests require bit identity with it.
 * One sequence's sums at one alpha; DetA = tp / (tp + fn + fp), AssA = ass_a_sum / tp, LocA = loc_sum / tp,
 * HOTA = sqrt(DetA * AssA) with TrackEval's guards are built by the caller. */
typedef struct rtmodt_hota_counts {
    int64_t tp, fn, fp;                 /* matches with S >= alpha - eps; GT rows - tp; hypothesis rows - tp              */
    double loc_sum;                     /* sum of S over those matches, in ascending frame, then ascending GT row         */
    double ass_a_sum, ass_re_sum, ass_pr_sum;   /* sums over the (o, h) with mc > 0, ascending (o, h), of
                                                 * mc * (mc / (gtc + trc - mc)), mc * (mc / max(1, gtc)), mc * (mc / max(1, trc)) */
} rtmodt_hota_counts;
/* rtmodt_mot_eval's input (n_seq = 0 is an empty call) plus alphas[n_alpha]: ascending, used as given, n_alpha <= 32 (the
 * Python side passes np.arange(0.05, 0.99, 0.05)).  out[n_seq][n_alpha].  Similarity S = the float64 IoU that mot_eval's
 * distance is 1 - of; only pairs with S > 0 are stored and memory follows them, never |O| x |H|.  Pass 1 builds the global
 * alignment score gas(o, h) of every co-occurring id pair, pass 2 matches every frame on its own (maximum weight of
 * gas * S; lap.h's solver on the contested remainder), the finish runs on the host from the sparse (sequence, o, h, mc)
 * table.  Limits: mot_eval's (1024 rows per frame and side, checked before launch; 2^28 stored pairs per call; a contested
 * remainder above 256 rows / 256 columns / 2048 pairs fails with RTMODT_E_CAPACITY naming the sequence and frame, before
 * anything is counted). */
int rtmodt_hota_eval(int device, int n_seq, const int32_t *seq_frame_start, const int64_t *frame_id, const int32_t *gt_start,
                     const int32_t *hyp_start, const int32_t *gt_oid, const double *gt_box, const int32_t *hyp_hid, const double *hyp_box,
                     const int32_t *seq_n_oid, const int32_t *seq_n_hid, const double *alphas, int n_alpha, rtmodt_hota_counts *out);

/* ---- detection error analysis: what the detector gets wrong ---------------------------------------------------- */
/* TECHNICAL_DESIGN_DOCUMENT.md D.5 defines five error types (localization, classification, duplicate, background false
 * positive, missed) to be clustered by image region and object size, D.4 asks for the per-class breakdown and D.6 step 4
 * plots a confusion matrix from a GT and a predictions file; the reference implements only build_confusion_matrix
 * (src/evaluation/metrics.py:110-123) on label pairs that nothing produces.  csrc/errors.hip, one launch for all images;
 * the rules are INTEGRATION.md section 14 and tests/errors_ref.py restates them in NumPy.  PARITY UNPINNED: neither tidecv
 * nor ultralytics is installed anywhere this runs. */
#define RTMODT_ERR_TP 0             /* detection types 0..5 are also the histogram columns 0..5 */
#define RTMODT_ERR_LOCALIZATION 1
#define RTMODT_ERR_CLASSIFICATION 2
#define RTMODT_ERR_BOTH 3
#define RTMODT_ERR_DUPLICATE 4
#define RTMODT_ERR_BACKGROUND 5
#define RTMODT_ERR_MISSED 6         /* histogram column 6: MISSED_COVERED + MISSED ground truths */
#define RTMODT_ERR_IGNORED 6        /* detection type: matched to a crowd GT; counted nowhere */
#define RTMODT_ERR_NOT_EVALUATED 7  /* detection type: below conf_thr or behind the max_det cut; counted nowhere */
#define RTMODT_GT_CROWD 0
#define RTMODT_GT_MATCHED 1
#define RTMODT_GT_MISSED_COVERED 2  /* unmatched, but a LOCALIZATION / CLASSIFICATION detection points at it */
#define RTMODT_GT_MISSED 3
typedef struct rtmodt_error_params {
    double conf_thr;        /* detections with score >= conf_thr are ranked by (-score, file index)        (0.25) */
    double iou_fg, iou_bg;  /* foreground / background IoU, iou_bg <= iou_fg                           (0.5, 0.1) */
    double cm_iou;          /* IoU of the class-agnostic matching behind the confusion matrix              (0.45) */
    int32_t max_det;        /* kept detections per image, 1..1024                                           (100) */
    int32_t grid_x, grid_y; /* by_cell columns and rows, 1..64 each                                        (8, 8) */
    int32_t reserved;       /* 0 */
} rtmodt_error_params;
/* Images are CSR slices: gt_start / dt_start[n_img + 1] into the GT / detection rows, each image's rows in file order;
 * gt_cat / dt_cat are dense category indices 0..K-1; boxes are x, y, w, h, float64; img_wh[n_img][2] is every image's
 * width and height (> 0).  Every IoU threshold is used as min(t, 1 - 1e-10) and compared with >=.  Outputs (host): per
 * detection row dt_type (RTMODT_ERR_*) and dt_gt (the GT row that decided the type, -1 none); per GT row gt_state
 * (RTMODT_GT_*) and gt_dt (the detection row matched to it, -1 none); int64 histograms by_class[K][7], by_size[3][7]
 * (area < 32^2, < 96^2, the rest; a detection's area is w * h, a GT's its `area` field), by_cell[grid_y][grid_x][7] (the
 * cell of the box centre in the image's own frame), missed_uncovered[K], the confusion matrix cm[K + 1][K + 1] (rows
 * ground truth, columns prediction, index K background) and cm_dropped[K] (free detections on a crowd GT of their class).
 * Every argument check runs before the first HIP call: RTMODT_E_INVALID for a null pointer, a NaN threshold, score, area
 * or a non-finite box, iou_bg > iou_fg, max_det or grid out of range, a non-positive image size, a category index outside
 * 0..K-1; RTMODT_E_CAPACITY for an image with more than 1024 GTs or 4096 detections (the message names the image), with
 * nothing launched.  Device scratch is allocated and freed inside the call. */
int rtmodt_detection_errors(int device, const rtmodt_error_params *params, int K, int n_img, const double *img_wh,
                            const int32_t *gt_start, const int32_t *gt_cat, const double *gt_box, const double *gt_area,
                            const int32_t *gt_crowd, const int32_t *dt_start, const int32_t *dt_cat, const double *dt_box,
                            const double *dt_score, int32_t *dt_type, int32_t *dt_gt, int32_t *gt_state, int32_t *gt_dt,
                            int64_t *by_class, int64_t *by_size, int64_t *by_cell, int64_t *missed_uncovered, int64_t *cm,
                            int64_t *cm_dropped);

/* ---- track stitching: the post-processing step the design document prescribes and never builds ---------------------- */
/* TECHNICAL_DESIGN_DOCUMENT.md B.4 "IDF1 Optimization" item 4 ("post-process merging -- merge tracks with overlapping time
 * windows and similar positions (< 20 px centroid distance)"), G.1 row 1 ("post-process merge tracks within 20 px and
 * 30-frame gap") and G.2's correct_id_switches(tracks_history, max_gap=30, max_dist=20), whose body is `...`.  PARITY
 * UNPINNED: the reference has no implementation and no third-party stitcher is installed anywhere this runs; the rules are
 * stated in csrc/stitch.hip's header and DESIGN.md section 18, and tests/stitch_ref.py restates them in plain Python. */
typedef struct rtmodt_stitch_params {
    int32_t max_gap;         /* a link A -> B needs 1 <= first frame of B - last frame of A <= max_gap; 1..1<<20        (30) */
    double max_dist;         /* ... and a squared centre distance < max_dist * max_dist (strict); finite, > 0        (20.0) */
    int32_t velocity_window; /* >= 0; 0 = A's exit point is its last centre; w = extrapolated over the gap with the mean
                              * velocity of A's last min(w, rows - 1) steps                                             (0) */
    int32_t interpolate;     /* 0 / 1: emit linearly interpolated rows for the frames inside every linked gap            (0) */
} rtmodt_stitch_params;
/* A batch of sequences in a fixed number of launches.  seq_trk_start[n_seq + 1]: CSR into the tracklets (one per id, any
 * order; indices below are positions in this list); trk_row_start[n_trk + 1]: CSR into the rows, every tracklet at least one
 * row, frames strictly ascending (|frame| <= 2^53); row_box[n][4] x, y, w, h, float64.  The chosen links are one-to-one, the
 * maximum number of admissible links and among those the minimum sum of d2 (lap.h, lexicographic costs): isolated candidate
 * pairs directly, the contested remainder per connected component, all components of all sequences concurrently.  Candidate
 * links are found by a binary-searched window over the tracklets ordered by first frame (work follows tracklets x window
 * population) and kept as a CSR (memory follows the admissible links, at most 2^28 a call).  Outputs (host): per tracklet
 * trk_succ (the tracklet it is linked to, -1 none), trk_root (the head of its chain: its rows take that tracklet's id) and
 * trk_link_d2 (the cost of its link, 0 without one); per sequence seq_links and seq_cost (the sum of d2, added in tracklet
 * order).  interpolate: for a link A -> B over a gap g the rows k = 1..g-1 at frame e_A + k with the box a + (b - a) * (k / g)
 * come back as fill_trk (A), fill_frame, fill_box[.][4], ordered by (sequence, A, k); *n_fill is their number.  When they do
 * not fit fill_cap the call returns RTMODT_E_CAPACITY, *n_fill holds the need, the per-tracklet and per-sequence outputs are
 * complete, the first fill_cap rows are written and nothing past them.  n_cand != NULL also returns the admissible links in
 * (A, first frame of B, B) order: cand_a, cand_b, cand_d2 and (when non-null) the exit point cand_p[.][2]; more than cand_cap
 * is RTMODT_E_CAPACITY with the need in *n_cand and no other output valid.  A contested component of more than 256 rows, 256
 * columns or 2048 links is RTMODT_E_CAPACITY naming the sequence and a tracklet of the component (its position within the
 * sequence); no output is valid.  Every argument check runs before the first HIP call: RTMODT_E_INVALID, naming sequence and
 * row, for a null pointer, a parameter out of range, a non-finite box, frames not strictly ascending inside a tracklet, a CSR
 * that is not monotone.  n_seq = 0, or no tracklet at all, is success with nothing launched.  Device scratch is allocated and
 * freed inside the call. */
int rtmodt_stitch_tracks(int device, const rtmodt_stitch_params *params, int n_seq, const int32_t *seq_trk_start,
                         const int32_t *trk_row_start, const int64_t *row_frame, const double *row_box, int32_t *trk_succ,
                         int32_t *trk_root, double *trk_link_d2, int64_t *seq_links, double *seq_cost, int64_t fill_cap,
                         int32_t *fill_trk, int64_t *fill_frame, double *fill_box, int64_t *n_fill, int64_t cand_cap, int32_t *cand_a,
                         int32_t *cand_b, double *cand_d2, double *cand_p, int64_t *n_cand);

/* ---- ID-swap guard: ByteTrack identities verified by appearance, swaps reverted online --------------------------------- */
/* TECHNICAL_DESIGN_DOCUMENT.md B.4 "Re-Identification Considerations" ("use appearance as a post-processing filter only on
 * suspected ID swaps; keep a feature buffer per track, the average colour histogram of the last 5 frames; when two tracks swap
 * within 3 frames, compare histograms and revert if similarity > 0.85"), B.4's failure table ("add appearance verification") and
 * G.1 row 1 ("add lightweight appearance hash verification").  PARITY UNPINNED: the reference has no code for any of it; the
 * rules are stated in csrc/swapguard.hip's header and DESIGN.md section 19, and tests/swapguard_ref.py restates them in plain
 * Python, which the kernel equals exactly.  The document gives 5, 3 and 0.85; min_history, min_gain_pm and contact_iou are this
 * project's additions, and no default has been validated on real footage.  The descriptor is csrc/appearance.hip's 192-bin int8
 * colour histogram; all arithmetic is integer except the IoU (the tracker's, float32). */
typedef struct rtmodt_swapguard rtmodt_swapguard;
typedef struct rtmodt_swapguard_cfg {
    int32_t history;            /* 1..8: descriptors kept per track id (B.4: 5)                                              */
    int32_t min_history;        /* 1..history: a track with fewer stored descriptors is never part of a revert         (3) */
    int32_t window;             /* >= 0: a revert needs frame_id - (last frame the two touched) <= window (B.4: 3)            */
    int32_t min_similarity_pm;  /* 0..1000: both cross similarities must reach it, per mille (B.4: 850)                       */
    int32_t min_gain_pm;        /* >= 0: ... and exceed the track's similarity to its own history by at least this     (1) */
    float contact_iou;          /* two tracks touch when their IoU is > contact_iou (strict; not NaN)                   (0.0) */
    int64_t max_gap_frames;     /* >= 0: a row not passed for more than this many frames is dropped (as the crossing counter) */
    int32_t max_tracks;         /* 1..1024 tracks handed over per stream and frame; a ledger holds 2 x max_tracks rows        */
    int32_t n_streams;          /* 1..64 independent ledgers                                                                  */
    int32_t max_events;         /* 1..1<<20 events per stream and frame                                                       */
    int32_t device;
} rtmodt_swapguard_cfg;
/* One reverted swap (B.4 step 3).  track_a < track_b: indices into the list handed over (the caller's, or the tracker's);
 * id_a / id_b: their ids BEFORE the exchange; sims: per mille, a's descriptor against the history of id_a and of id_b, then b's
 * against id_b's and id_a's (the revert needed sims[1] and sims[3] high, above sims[0] and sims[2]). */
typedef struct rtmodt_swap_event {
    int64_t frame_id, id_a, id_b;
    int32_t track_a, track_b;
    int32_t sims[4];
} rtmodt_swap_event;
/* B.4 step 2, the feature buffer: n_streams ledgers keyed by track id.  RTMODT_E_INVALID for a parameter outside the ranges
 * above; nothing is launched.  PARITY UNPINNED. */
int rtmodt_swapguard_create(const rtmodt_swapguard_cfg *cfg, rtmodt_swapguard **out);
/* Ends B.4 step 2's buffers: waits for the work queued on the handle's own stream, then frees the ledgers and the handle; null
 * is allowed.  PARITY UNPINNED. */
void rtmodt_swapguard_destroy(rtmodt_swapguard *g);
/* B.4 steps 1 and 3 on a caller-supplied list of one stream (any order, unique ids else RTMODT_E_INVALID, at most max_tracks
 * else RTMODT_E_CAPACITY): every listed track is passed, described on `frame` (BGR24, h x w, row pitch stride_bytes, host or
 * device memory by mem_kind).  ids_out[n] receives the ids after the reverts; the caller's tracker must adopt them, as the
 * tracker form below does for ByteTrack -- otherwise the pair fires again while the window lasts.  Events in ascending track_a;
 * `events` holds max_events records; a frame with more returns RTMODT_E_CAPACITY with the first max_events delivered and every
 * revert applied.  A ledger that would pass 2 x max_tracks rows drops its idle rows and the stream stays in RTMODT_E_CAPACITY
 * for good (as rtmodt_crossing_create describes); never a fault.  PARITY UNPINNED. */
int rtmodt_swapguard_process(rtmodt_swapguard *g, int stream, const int64_t *track_ids, const float *xyxy, int n,
                             const uint8_t *frame, int h, int w, int stride_bytes, int mem_kind, int64_t frame_id,
                             int64_t *ids_out, rtmodt_swap_event *events, int32_t *n_events);
/* G.1 row 1 on every stream of a ByteTrack handle at once, on its device-resident state and on the HIP stream its last update
 * ran on: passed = time_since_update == report_tsu (1 = matched or spawned this frame, as rtmodt_crossing_process_tracker);
 * frames[n_streams of the tracker] are the frames the detector read.  A revert exchanges the two ids inside the tracker's state
 * and nothing else, so everything that reads that state afterwards sees the corrected identity.  More passed tracks than
 * max_tracks in a stream is RTMODT_E_CAPACITY for that stream from then on.  events is [n_streams][max_events],
 * n_events[n_streams].  The launch count is fixed: one gather, the two descriptor launches, one step.  PARITY UNPINNED. */
int rtmodt_swapguard_process_tracker(rtmodt_swapguard *g, rtmodt_tracker *trk, const uint8_t *const *frames, int h, int w,
                                     int stride_bytes, int mem_kind, int64_t frame_id, int report_tsu,
                                     rtmodt_swap_event *events, int32_t *n_events);
/* Ledger snapshot of one stream (B.4 step 2; the parity surface of tests/swapguard_ref.py), rows in ascending id: last passed
 * frame, stored descriptors, the frame of the last contact and the id touched then (-1 none), and ring[row][history][192] with
 * the stored descriptors oldest first (the rest zero).  Arrays sized 2 x max_tracks rows; any may be NULL.  PARITY UNPINNED. */
int rtmodt_swapguard_state(rtmodt_swapguard *g, int stream, int64_t *ids, int64_t *last_frame, int32_t *count,
                           int64_t *contact_frame, int64_t *contact_id, int8_t *ring, int32_t *n);
/* Swaps reverted on one stream since creation (G.1 row 1's count of corrected switches).  PARITY UNPINNED. */
int rtmodt_swapguard_counts(rtmodt_swapguard *g, int stream, int64_t *n_reverted);
/* Device time of the last _process / _process_tracker call, from HIP events around its launches: the descriptor launches, then
 * gather + step (B.4 calls the check "lightweight"; this is where that is measured).  PARITY UNPINNED. */
int rtmodt_swapguard_last_ms(rtmodt_swapguard *g, float *describe_ms, float *step_ms);

/* ---- sliced inference: the cure for config/default.yaml:24-26, 34 (1920 x 1080 frames into a 640 x 640 detector) --------------- */
/* The reference shrinks every object three times before the network sees it; its design document lists "Missed small objects"
 * (B.4's failure table, mitigation "lower track_thresh or use YOLOv8m") and marks conf 0.40 "Misses small objects" (B.3's
 * threshold table).  The standard cure that keeps the model is the SAHI scheme: cut the frame into overlapping tiles at native
 * resolution, detect in every tile plus one down-scaled overview, merge the boxes back in frame coordinates.  Here the cut and
 * the merge run on the GPU around an ordinary detector handle (csrc/slice.hip states the rules, DESIGN.md section 25 the
 * layouts).  PINNED against tests/slice_ref.py, bit for bit: the tile bytes, the per-image detections, the merge.  PARITY
 * UNPINNED: the `sahi` package is installed nowhere this runs.  UNPINNED as well: any accuracy gain on real footage -- no trained
 * checkpoint exists offline, so the small-object claim rests on the published method, not on a measurement here.
 *
 * Grid: along an axis of length L with tile t and overlap o (0 <= o < t): te = min(t, L), step = te - o (one position, 0, when
 * step <= 0), p_k = min(k * step, L - te) up to and including the first with p_k + te >= L -- every tile is full size, the last
 * one shifted inward.  Tiles are ordered row-major (y outer, x inner); at most 64 per frame, else RTMODT_E_CAPACITY.  With T
 * tiles and the overview on, a frame is I = T + 1 images; a batch of n frames is n * I images of te_w x te_h BGR24 with pitch
 * 3 * te_w, frame-major (image f * I + j; j == T is the overview: the whole frame letterboxed with 114 padding). */
#define RTMODT_SLICE_MERGE_NMM 0   /* greedy non-maximum merging: a keeper absorbs its matches into a min / max union box */
#define RTMODT_SLICE_MERGE_NMS 1   /* a keeper drops its matches                                                          */
#define RTMODT_SLICE_METRIC_IOS 0  /* inter / min(area_a, area_b)                                                         */
#define RTMODT_SLICE_METRIC_IOU 1  /* inter / (area_a + area_b - inter)                                                   */
typedef struct rtmodt_slicer rtmodt_slicer;
typedef struct rtmodt_slice_cfg {
    int32_t device;
    int32_t frame_w, frame_h;     /* the source frames (config/default.yaml:24-26: 1920 x 1080)                              */
    int32_t tile_w, tile_h;       /* requested tile = the detector's input (config/default.yaml:34: 640); effective min(t, L) */
    int32_t overlap_w, overlap_h; /* pixels, 0 <= overlap < tile                                                            */
    int32_t overview;             /* 1: one more image per frame, the whole frame letterboxed into the effective tile       */
    int32_t merge;                /* RTMODT_SLICE_MERGE_*  (SAHI's default: NMM)                                            */
    int32_t metric;               /* RTMODT_SLICE_METRIC_* (SAHI's default: IoS)                                            */
    float match_thresh;           /* a pair matches when the metric is > match_thresh (strict, float32; SAHI's default 0.5)  */
    int32_t agnostic;             /* 0: only boxes of one class match                                                       */
    int32_t max_out;              /* merged detections kept per frame (1..4096), the first in (conf, image, slot) order     */
    int32_t max_frames;           /* frames per sliced batch; max_frames * I <= 64 (a detector batch)                       */
} rtmodt_slice_cfg;
/* The grid alone, host only (no device is touched): xs / ys[64] (may be NULL) receive the tile origins, *n_tiles their count,
 * *te_w / *te_h the effective tile.  RTMODT_E_INVALID for a bad argument, RTMODT_E_CAPACITY for more than 64 tiles. */
int rtmodt_slice_grid(int frame_w, int frame_h, int tile_w, int tile_h, int overlap_w, int overlap_h, int32_t *xs, int32_t *ys,
                      int32_t *n_tiles, int32_t *te_w, int32_t *te_h);
/* A slicer for detectors built with `max_det` detections per image.  The merge sorts a frame's candidates in LDS: I * max_det
 * above 8192 is RTMODT_E_CAPACITY, as is max_frames * I above 64; bad arguments (overlap >= tile among them) are
 * RTMODT_E_INVALID; nothing is allocated in either case. */
int rtmodt_slicer_create(const rtmodt_slice_cfg *cfg, int max_det, rtmodt_slicer **out);
/* Waits for the work queued on behalf of the handle (its own stream, the merges on a detector's stream), then frees it; null is
 * allowed.  Destroy the slicer before the detector it was last used with. */
void rtmodt_slicer_destroy(rtmodt_slicer *s);
int rtmodt_slicer_info(rtmodt_slicer *s, int32_t *n_tiles, int32_t *images_per_frame, int32_t *te_w, int32_t *te_h);
/* slice_gather alone: n frames (frame_h x frame_w BGR24, row pitch >= 3 * frame_w, host or device memory by mem_kind) are cut in
 * ONE launch and the n * I images copied out to tiles_out_host.  Not while a sliced batch is in flight (RTMODT_E_INVALID). */
int rtmodt_slicer_gather(rtmodt_slicer *s, const uint8_t *const *frames, int n, int pitch, int mem_kind, uint8_t *tiles_out_host);
/* slice_merge alone on caller-supplied per-image detections (host arrays, the layout rtmodt_detector_fetch hands out for a batch of
 * n_frames * I images: det_xyxy[n_frames * I][max_det][4] in image coordinates, det_conf / det_cls[n_frames * I][max_det],
 * det_n[n_frames * I]); cfg->device and cfg->max_frames are not used.  One workgroup per frame.  Outputs (host):
 * xyxy[n_frames][max_out][4], conf / cls / n_merged[n_frames][max_out] (n_merged: boxes the keeper absorbed or dropped),
 * n_out[n_frames]; *kernel_ms (may be NULL) the launch's device time from HIP events. */
int rtmodt_slice_merge(int device, const rtmodt_slice_cfg *cfg, int max_det, int n_frames, const float *det_xyxy, const float *det_conf,
                       const int32_t *det_cls, const int32_t *det_n, float *xyxy, float *conf, int32_t *cls, int32_t *n_merged,
                       int32_t *n_out, float *kernel_ms);
/* One sliced batch, asynchronous: slice_gather on the slicer's stream (host frames are staged by the handle; the stream is idle
 * before the detector sees the tile pointers), rtmodt_detector_enqueue_batch on the n * I images as device frames, slice_merge on
 * the detector's post-processing stream behind its NMS -- no host round trip.  det must be on the same device, built with the
 * slicer's max_det (else RTMODT_E_INVALID), with batch >= n * I and max_src >= the effective tile (else RTMODT_E_CAPACITY), and
 * must have no batch in flight that is not this slicer's.  Two sliced batches may be in flight (enqueue t+1, then fetch t); a
 * third is RTMODT_E_INVALID.  A refusal launches nothing. */
int rtmodt_slicer_enqueue(rtmodt_slicer *s, rtmodt_detector *det, const uint8_t *const *frames, int n, int pitch, int mem_kind);
/* The OLDEST sliced batch in flight: drains det's oldest batch through rtmodt_detector_fetch (its in-flight accounting stays
 * right) and hands out the merged detections, xyxy[n][max_out][4], conf / cls / n_merged[n][max_out], n_out[n]; any but n_out may
 * be NULL.  tile_xyxy[n * I][max_det][4], tile_conf / tile_cls[n * I][max_det], tile_n[n * I] (each may be NULL) receive the
 * per-image detections they were merged from, in image coordinates. */
int rtmodt_slicer_fetch(rtmodt_slicer *s, rtmodt_detector *det, float *xyxy, float *conf, int32_t *cls, int32_t *n_merged, int32_t *n_out,
                        float *tile_xyxy, float *tile_conf, int32_t *tile_cls, int32_t *tile_n);
/* Device time (ms, HIP events) of slice_gather of the last enqueue / gather and of slice_merge of the last fetched batch. */
int rtmodt_slicer_last_ms(rtmodt_slicer *s, float *gather_ms, float *merge_ms);
/* rtmodt_tracker_update_from_detector on the MERGED detections of the slicer's newest batch (stream i <- frame i), queued on the
 * same HIP stream behind slice_merge; the tracker needs max_dets >= max_out. */
int rtmodt_tracker_update_from_slicer(rtmodt_tracker *trk, rtmodt_slicer *s);

/* ---- privacy masking: people, objects and fixed privacy zones redacted before a frame leaves the box ------------------------ */
/* The reference records and streams every frame in the clear; it has no code for redaction (PARITY UNPINNED throughout: no
 * counterpart in the reference, no OpenCV to run cv2.blur / GaussianBlur against, no camera's privacy mask to compare with).
 * PINNED, byte for byte, against tests/privacy_ref.py: the regions, the mask and the three modes.  csrc/privacy_regions.h states
 * how a box becomes a rectangle (truncated corners clamped to +-2^20, BOX or HEAD rows, expansion, clip, class filter),
 * csrc/privacy.hip's header the paint rules; all of it is integer arithmetic.  A pixel is masked when it lies in a region
 * rectangle of its frame or inside or on a privacy polygon (the zone engine's test).  Unmasked pixels and the bytes past 3w of a
 * row are never written.  Frames as in rtmodt_render_batch: BGR24, h x w, row pitch stride_bytes >= 3w, host or device memory
 * by mem_kind.  At most 32 polygons / 2048 points / 65536 regions per frame, else RTMODT_E_CAPACITY with nothing launched. */
#define RTMODT_PRIVACY_FILL 0       /* masked pixels become fill_bgr                                                            */
#define RTMODT_PRIVACY_PIXELATE 1   /* ... the rounded mean (sum + n/2) / n of their cell x cell cell, grid anchored at (0, 0)    */
#define RTMODT_PRIVACY_BLUR 2       /* ... `passes` box filters of (2 radius + 1)^2, each rounded to u8, windows clipped to the frame */
#define RTMODT_PRIVACY_REGION_BOX 0   /* the whole box                                                                          */
#define RTMODT_PRIVACY_REGION_HEAD 1  /* its top max(1, (H * head_pm + 999) / 1000) rows                                        */
typedef struct rtmodt_privacy rtmodt_privacy;
typedef struct rtmodt_privacy_cfg {
    int32_t mode;               /* RTMODT_PRIVACY_*                                                                             */
    uint8_t fill_bgr[4];        /* FILL's colour, B G R (the fourth byte is ignored)                                            */
    int32_t cell;               /* 2..64                                                                                        */
    int32_t radius;             /* 1..16                                                                                        */
    int32_t passes;             /* 1..3                                                                                         */
    int32_t region;             /* RTMODT_PRIVACY_REGION_*                                                                      */
    int32_t head_pm;            /* 1..1000 per mille of the box height                                                          */
    int32_t expand_px;          /* 0..256 pixels added on all four sides                                                        */
    const int32_t *classes;     /* NULL: every class; else only boxes of these n_classes (0..256) class ids yield a region      */
    int32_t n_classes;
    int32_t max_regions;        /* 1..65536 regions per frame the handle accepts                                                */
    int32_t device;
} rtmodt_privacy_cfg;
/* Host only: pixelate, black fill colour, cell 16, radius 8, passes 2, whole boxes, head_pm 300, no expansion, every class,
 * 65536 regions, device 0.  PARITY UNPINNED. */
void rtmodt_privacy_default_cfg(rtmodt_privacy_cfg *cfg);
/* Every parameter is checked whatever the mode: one outside its range is RTMODT_E_INVALID and nothing is launched or
 * allocated.  The class list is copied.  PARITY UNPINNED. */
int rtmodt_privacy_create(const rtmodt_privacy_cfg *cfg, rtmodt_privacy **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  PARITY UNPINNED. */
void rtmodt_privacy_destroy(rtmodt_privacy *p);
/* The fixed privacy zones (a camera's "privacy masks"), int32 polygons as rtmodt_renderer_set_zones takes them, uploaded once and
 * cached by the handle; n = 0 clears them.  More than 32 polygons or 2048 points is RTMODT_E_CAPACITY.  PARITY UNPINNED. */
int rtmodt_privacy_set_polygons(rtmodt_privacy *p, const int32_t *const *polygons_xy, const int32_t *n_points, int n);
/* Host only, no device needed: the rectangles (x0, y0, x1, y1 inclusive, in box order, skipped boxes left out) that n_boxes
 * boxes xyxy[n_boxes][4] of classes cls[n_boxes] (may be NULL without a class list) yield in an h x w frame under cfg's region
 * kind, head_pm, expand_px and classes.  *needed = their count; written to rects when cap_rects >= *needed (the two-call
 * protocol of rtmodt_render_pack).  A NaN or infinite coordinate is RTMODT_E_INVALID.  The parity surface of
 * csrc/privacy_regions.h.  PARITY UNPINNED. */
int rtmodt_privacy_regions(const rtmodt_privacy_cfg *cfg, const float *xyxy, const int32_t *cls, int n_boxes, int h, int w,
                           int32_t *rects, int cap_rects, int32_t *needed);
/* Masks n frames with the boxes handed over: xyxy[i] points at n_boxes[i] boxes of frame i (4 floats each), cls[i] at their
 * classes (cls, or cls[i], may be NULL without a class list).  dst_frames == NULL: in place.  Otherwise dst_frames[i] receives
 * the whole masked frame (its bytes past 3w of a row stay as they are) and src_frames[i] is left untouched; dst_frames[i] must
 * equal src_frames[i] (that frame is masked in place) or not overlap it, else RTMODT_E_INVALID.  A NaN or infinite coordinate is
 * RTMODT_E_INVALID, more regions in a frame than max_regions RTMODT_E_CAPACITY; a refusal launches nothing and leaves every
 * frame untouched.  Every output is a function of the frame as it was before the call: in-place BLUR goes through a scratch
 * buffer of the handle.  At most three launches, whatever the number of regions.  Synchronous.  PARITY UNPINNED. */
int rtmodt_privacy_apply(rtmodt_privacy *p, uint8_t *const *src_frames, uint8_t *const *dst_frames, int n, int h, int w,
                         int stride_bytes, int mem_kind, const float *const *xyxy, const int32_t *const *cls,
                         const int32_t *n_boxes);
/* Masks, in place, frames[n_streams of the tracker] with the ByteTrack handle's device-resident tracks, on the HIP stream its
 * last update ran on: exactly the tracks rtmodt_crossing_process_tracker passes (time_since_update == report_tsu, finite box;
 * a non-finite box is skipped).  No box crosses to the host.  The tracker's max_tracks must not exceed max_regions
 * (RTMODT_E_CAPACITY).  PARITY UNPINNED. */
int rtmodt_privacy_apply_tracker(rtmodt_privacy *p, rtmodt_tracker *trk, uint8_t *const *frames, int h, int w, int stride_bytes,
                                 int mem_kind, int report_tsu);
/* The same on a DeepSORT handle: the tracks rtmodt_crossing_process_deepsort passes (confirmed, time_since_update ==
 * report_tsu).  PARITY UNPINNED. */
int rtmodt_privacy_apply_deepsort(rtmodt_privacy *p, rtmodt_deepsort *ds, uint8_t *const *frames, int h, int w, int stride_bytes,
                                  int mem_kind, int report_tsu);
/* The same on an OC-SORT handle: the tracks rtmodt_crossing_process_ocsort passes (the returned ones).  PARITY UNPINNED. */
int rtmodt_privacy_apply_ocsort(rtmodt_privacy *p, rtmodt_ocsort *oc, uint8_t *const *frames, int h, int w, int stride_bytes,
                                int mem_kind);
/* The same on a BoT-SORT handle: the tracks rtmodt_crossing_process_botsort passes (tracked and matched this frame).  PARITY
 * UNPINNED. */
int rtmodt_privacy_apply_botsort(rtmodt_privacy *p, rtmodt_botsort *bot, uint8_t *const *frames, int h, int w, int stride_bytes,
                                 int mem_kind);
/* Masks, in place, the first n frames of the detector's newest batch with EVERY detection of that batch, read from its
 * device-resident outputs on its post-processing stream behind the NMS (a tracker reports an object only once it is confirmed;
 * masking the detections closes that gap).  n above the batch's frame count is RTMODT_E_INVALID, the detector's max_det above
 * max_regions RTMODT_E_CAPACITY.  PARITY UNPINNED. */
int rtmodt_privacy_apply_detector(rtmodt_privacy *p, rtmodt_detector *det, uint8_t *const *frames, int n, int h, int w,
                                  int stride_bytes, int mem_kind);
/* Device time (ms, HIP events around the launches) of the last apply call that launched.  PARITY UNPINNED. */
int rtmodt_privacy_last_ms(rtmodt_privacy *p, float *kernel_ms);

/* ---- occupancy heatmaps: where objects have been, accumulated from boxes or device-resident tracks ------------------------- */
/* The reference has nothing that accumulates presence over time (its heat-map plot is the confusion matrix); PARITY UNPINNED
 * throughout: no counterpart in the reference, no Ultralytics Heatmap solution, no cv2 colormap or addWeighted to compare with, no
 * default tuned on real footage.  PINNED, exactly, against tests/heatmap_ref.py: the footprints, decay, saturation, the overlay and
 * the zone sums.  csrc/heatmap_stamp.h states which cells a box stamps, csrc/heatmap.hip's header the other rules; all of it is
 * integer arithmetic.  A handle holds one uint32 grid of ceil(height / cell) x ceil(width / cell) cells per stream, zero at
 * creation, edge cells clipped to the frame.  At most 65536 boxes per frame, 32 polygons / 2048 points, else RTMODT_E_CAPACITY
 * with nothing launched; a refused call leaves the grid and the frames as they were. */
#define RTMODT_HEATMAP_BOX 0        /* every cell the box's rectangle (clipped to the frame) touches                             */
#define RTMODT_HEATMAP_DISC 1       /* of those, the cells whose centre lies within min(W, H) / 2 of the box centre, and the centre pixel's */
#define RTMODT_HEATMAP_FOOT 2       /* the cells within foot_radius of the bottom-centre (ground contact) pixel, and that pixel's  */
typedef struct rtmodt_heatmap rtmodt_heatmap;
typedef struct rtmodt_heatmap_cfg {
    int32_t n_streams;          /* 1..1024 grids                                                                                */
    int32_t height, width;      /* the frame size, 1..32768 each; n_streams * cells at most 2^30                                */
    int32_t cell;               /* 1, 2, 4, 8 or 16 pixels per cell side                                                        */
    int32_t footprint;          /* RTMODT_HEATMAP_*                                                                             */
    int32_t foot_radius;        /* 0..256 pixels (FOOT)                                                                         */
    int32_t weight;             /* 1..1024 added per footprint covering a cell                                                  */
    int32_t decay_shift;        /* 0: no decay; 1..16: heat -= heat >> decay_shift ...                                          */
    int32_t decay_every;        /* ... in every decay_every-th accumulate call (1..65536)                                       */
    const int32_t *classes;     /* NULL: every class; else only boxes of these n_classes (0..256) class ids leave a footprint   */
    int32_t n_classes;
    int32_t device;
} rtmodt_heatmap_cfg;
/* Host only: 1 stream, height and width 0 (the caller sets them), cell 4, DISC, foot_radius 0, weight 1, no decay (shift 0, every
 * 1), every class, device 0.  PARITY UNPINNED. */
void rtmodt_heatmap_default_cfg(rtmodt_heatmap_cfg *cfg);
/* Every parameter is checked before anything is allocated: one outside its range is RTMODT_E_INVALID.  The class list is copied;
 * the colour table starts as the closed-form jet (rtmodt_heatmap_set_colormap).  PARITY UNPINNED. */
int rtmodt_heatmap_create(const rtmodt_heatmap_cfg *cfg, rtmodt_heatmap **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  PARITY UNPINNED. */
void rtmodt_heatmap_destroy(rtmodt_heatmap *h);
/* Host only, no device needed: the cells (cx, cy pairs, row by row) the one box xyxy[4] of class cls stamps on the grid of cfg's
 * height x width frame under cfg's cell, footprint, foot_radius and classes.  *needed = their count; written to cells_xy when
 * cap_cells >= *needed (the two-call protocol of rtmodt_privacy_regions).  A NaN or infinite coordinate is RTMODT_E_INVALID.  The
 * parity surface of csrc/heatmap_stamp.h.  PARITY UNPINNED. */
int rtmodt_heatmap_footprint(const rtmodt_heatmap_cfg *cfg, const float *xyxy, int32_t cls, int32_t *cells_xy, int cap_cells,
                             int32_t *needed);
/* One frame of every stream: xyxy[s] points at n_boxes[s] boxes of stream s (4 floats each), cls[s] at their classes (cls, or
 * cls[s], may be NULL without a class list).  Calls are numbered from 1 per handle (refused calls are not counted): if decay_shift
 * != 0 and call % decay_every == 0 every cell first becomes heat - (heat >> decay_shift); then heat = min(heat + weight * count,
 * 2^32 - 1) with count the number of this frame's footprints covering the cell.  No atomics: saturation is exact, the order of
 * the boxes does not matter.  A NaN or infinite coordinate is RTMODT_E_INVALID, more than 65536 boxes in a frame
 * RTMODT_E_CAPACITY.  One launch, whatever the number of boxes.  Synchronous.  PARITY UNPINNED. */
int rtmodt_heatmap_accumulate(rtmodt_heatmap *h, const float *const *xyxy, const int32_t *const *cls, const int32_t *n_boxes);
/* The same with the ByteTrack handle's device-resident tracks (stream s of the tracker -> grid s), on the HIP stream its last
 * update ran on: exactly the tracks rtmodt_privacy_apply_tracker masks (time_since_update == report_tsu, finite box; a non-finite
 * box is skipped).  No box crosses to the host; two launches.  A stream count other than the handle's is RTMODT_E_INVALID.  PARITY
 * UNPINNED. */
int rtmodt_heatmap_accumulate_tracker(rtmodt_heatmap *h, rtmodt_tracker *trk, int report_tsu);
/* The same on a DeepSORT handle: confirmed tracks with time_since_update == report_tsu.  PARITY UNPINNED. */
int rtmodt_heatmap_accumulate_deepsort(rtmodt_heatmap *h, rtmodt_deepsort *ds, int report_tsu);
/* The same on an OC-SORT handle: the returned tracks.  PARITY UNPINNED. */
int rtmodt_heatmap_accumulate_ocsort(rtmodt_heatmap *h, rtmodt_ocsort *oc);
/* The same on a BoT-SORT handle: tracked and matched this frame.  PARITY UNPINNED. */
int rtmodt_heatmap_accumulate_botsort(rtmodt_heatmap *h, rtmodt_botsort *bot);
/* The same with EVERY detection of the detector's newest batch (frame i -> grid i), read from its device-resident outputs on its
 * post-processing stream behind the NMS.  A batch whose frame count is not the handle's stream count is RTMODT_E_INVALID.  PARITY
 * UNPINNED. */
int rtmodt_heatmap_accumulate_detector(rtmodt_heatmap *h, rtmodt_detector *det);
/* Blends the heat onto n BGR24 frames in place (height x width as created, else RTMODT_E_INVALID; row pitch stride_bytes >= 3w;
 * host or device memory by mem_kind).  Frame i shows grid streams[i]; streams == NULL: grid i, and n must be the stream count.
 * m = scale_max (colours stable over time), or with scale_max == 0 the grid's maximum now; m == 0 leaves the frame untouched.
 * Level v = min(255, (heat * 255 + m / 2) / m); pixel (x, y) reads cell (x / cell, y / cell) (nearest sampling); v < min_level
 * (1..255): the pixel keeps its bytes; else each channel becomes (p * (256 - alpha) + lut[v][c] * alpha + 128) >> 8, alpha
 * 0..256.  The bytes past 3w of a row are never written.  Two launches at most.  Synchronous.  PARITY UNPINNED (cv2.addWeighted,
 * cv2.applyColorMap). */
int rtmodt_heatmap_overlay(rtmodt_heatmap *h, uint8_t *const *frames, const int32_t *streams, int n, int height, int width,
                           int stride_bytes, int mem_kind, int alpha, int min_level, uint32_t scale_max);
/* The colour table, 256 x 3 bytes B G R, copied.  NULL restores the default, a closed-form jet: channel = clamp(max(0, 765 -
 * |8v - 510k|) >> 1, 0, 255) with k = 3, 2, 1 for R, G, B; its parity with cv2.COLORMAP_JET is UNPINNED.  PARITY UNPINNED. */
int rtmodt_heatmap_set_colormap(rtmodt_heatmap *h, const uint8_t *lut_bgr);
/* sums[z] = the sum of heat over the cells of polygon z (int32 polygons as rtmodt_renderer_set_zones takes them) of one stream's
 * grid; a cell belongs to a polygon when its centre pixel (min(cx * cell + cell / 2, width - 1), likewise y) is inside or on it
 * (the zone engine's test).  With weight 1 and FOOT radius 0 that is the object-frames spent in the zone.  More than 32 polygons
 * or 2048 points is RTMODT_E_CAPACITY.  One launch.  PARITY UNPINNED. */
int rtmodt_heatmap_zone_sums(rtmodt_heatmap *h, int stream, const int32_t *const *polygons_xy, const int32_t *n_points, int n,
                             uint64_t *sums);
/* One stream's grid to host memory, uint32[gh][gw].  PARITY UNPINNED. */
int rtmodt_heatmap_read(rtmodt_heatmap *h, int stream, uint32_t *out);
/* Replaces one stream's grid with a saved one (uint32[gh][gw]), so that a map survives a restart.  PARITY UNPINNED. */
int rtmodt_heatmap_load(rtmodt_heatmap *h, int stream, const uint32_t *in);
/* Zeroes one stream's grid, or every grid with stream == -1; the call numbering goes on.  PARITY UNPINNED. */
int rtmodt_heatmap_reset(rtmodt_heatmap *h, int stream);
/* Device time (ms, HIP events around the launches) of the last accumulate or overlay call that launched.  PARITY UNPINNED. */
int rtmodt_heatmap_last_ms(rtmodt_heatmap *h, float *kernel_ms);

/* ---- motion detection: a background model per stream tells still frames from moving ones ------------------------------------ */
/* The reference drops frames blind to content (design document B.1) and offers a smaller model or input against a low frame rate
 * (G.1 row 2, G.3); it has nothing that looks at the pixels.  PARITY UNPINNED throughout: no counterpart in the reference, no
 * OpenCV BackgroundSubtractorMOG2 and no Frigate to compare with, no default validated on real footage.  PINNED, exactly, against
 * tests/motion_ref.py: the model, the mask, every count, the regions and the status.  csrc/motion_model.h states the per-cell
 * rules, csrc/motion.hip's header the mask and the regions; all of it is integer arithmetic.  A handle holds, per stream, bg and
 * dev (unsigned 8.8 fixed point) for each cell of a ceil(height / scale) x ceil(width / scale) luma grid, frames_seen, the last
 * mask and the last block grid. */
#define RTMODT_MOTION_WARMUP 0          /* frames_seen < warmup at entry: the model learns, nothing is foreground                  */
#define RTMODT_MOTION_STILL 1           /* no region                                                                               */
#define RTMODT_MOTION_MOTION 2          /* at least one region                                                                     */
#define RTMODT_MOTION_SCENE_CHANGE 3    /* 1000 * n_raw >= scene_pm * cells: covered, moved, lights switched; the model restarts   */
typedef struct rtmodt_motion rtmodt_motion;
typedef struct rtmodt_motion_cfg {
    int32_t streams;            /* 1..1024                                                                                      */
    int32_t height, width;      /* the frame size, 1..32768 each; the grid at most 2^24 cells, all streams 2^28                 */
    int32_t scale;              /* 1, 2, 4 or 8 pixels per cell side                                                            */
    int32_t learn_shift;        /* 1..8: bg += (Yc * 256 - bg) >> learn_shift for the cells that are not raw foreground         */
    int32_t learn_shift_fg;     /* 0: raw foreground never updates the model; else learn_shift..12                              */
    int32_t threshold;          /* 1..255 luma levels                                                                           */
    int32_t dev_gain;           /* 0..8: raw = |d| > threshold * 256 + dev_gain * dev                                           */
    int32_t min_neighbors;      /* 1..9 raw cells in the 3 x 3 neighbourhood (the cell included) for a raw cell to be kept      */
    int32_t dilate;             /* 0..3 cells (Chebyshev)                                                                       */
    int32_t warmup;             /* 1..255 frames                                                                                */
    int32_t scene_pm;           /* 1..1000 per mille of the cells                                                               */
    int32_t min_area;           /* >= 1 cells for a component to be a region                                                    */
    int32_t max_regions;        /* 1..256 regions stored per frame                                                              */
    int32_t block;              /* 4, 8, 16 or 32 cells per side of a block of the activity grid                                */
    int32_t device;
} rtmodt_motion_cfg;
typedef struct rtmodt_motion_result {
    int32_t status;             /* RTMODT_MOTION_*                                                                              */
    int32_t stream;
    int32_t frames_seen;        /* after the call: 0 after a SCENE_CHANGE                                                       */
    uint32_t n_raw, n_fg;       /* raw foreground cells; mask cells                                                             */
    int32_t n_regions;          /* stored: min(n_regions_total, max_regions)                                                    */
    int32_t n_regions_total;
    int32_t bbox[4];            /* of the mask, pixels x0, y0, x1, y1 (x1, y1 exclusive); all zero when the mask is empty       */
    int32_t reserved;
    uint64_t luma_sum;          /* the sum of the cells' luma                                                                   */
} rtmodt_motion_result;
/* Host only: 1 stream, height and width 0 (the caller sets them), scale 4, learn_shift 4, learn_shift_fg 8, threshold 12, dev_gain
 * 2, min_neighbors 3, dilate 1, warmup 8, scene_pm 600, min_area 4, max_regions 32, block 16, device 0.  No default has been
 * validated on real footage.  PARITY UNPINNED. */
void rtmodt_motion_default_cfg(rtmodt_motion_cfg *cfg);
/* Every parameter is checked before anything is allocated: one outside its range is RTMODT_E_INVALID, a grid above 2^24 cells (or
 * 2^28 over all streams) RTMODT_E_CAPACITY.  Every model starts with frames_seen 0.  PARITY UNPINNED. */
int rtmodt_motion_create(const rtmodt_motion_cfg *cfg, rtmodt_motion **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  PARITY UNPINNED. */
void rtmodt_motion_destroy(rtmodt_motion *m);
/* One frame for each of n distinct streams: frame i (BGR24, height x width as created, row pitch stride_bytes >= 3w, host or
 * device memory by mem_kind, read only) updates the model of streams[i] (streams == NULL: stream i, and n must be the stream
 * count).  results[i] and regions[i][max_regions][5] (x0, y0, x1, y1 in pixels, area in cells; the entries past n_regions are zero)
 * describe it.  A frame size other than the handle's, a stream outside 0..streams - 1 or named twice, a null frame and n above the
 * stream count are RTMODT_E_INVALID with nothing launched.  Seven launches, whatever the frames show; all results come back in one
 * copy.  Streams the call does not name keep their state.  Synchronous.  PARITY UNPINNED. */
int rtmodt_motion_process(rtmodt_motion *m, const uint8_t *const *frames, const int32_t *streams, int n, int height, int width,
                          int stride_bytes, int mem_kind, rtmodt_motion_result *results, int32_t *regions);
/* The mask of the stream's last frame, uint8[gh][gw] of 0 / 1 (all zero before the first).  PARITY UNPINNED. */
int rtmodt_motion_read_mask(rtmodt_motion *m, int stream, uint8_t *out);
/* The mask cells per block x block group of cells, uint32[ceil(gh / block)][ceil(gw / block)].  PARITY UNPINNED. */
int rtmodt_motion_read_blocks(rtmodt_motion *m, int stream, uint32_t *out);
/* One stream's model to host memory: bg and dev as uint16[gh][gw] each, and frames_seen.  PARITY UNPINNED. */
int rtmodt_motion_read_state(rtmodt_motion *m, int stream, uint16_t *bg, uint16_t *dev, int32_t *frames_seen);
/* Replaces one stream's model (frames_seen 0..2^30), so that it survives a restart.  PARITY UNPINNED. */
int rtmodt_motion_load_state(rtmodt_motion *m, int stream, const uint16_t *bg, const uint16_t *dev, int32_t frames_seen);
/* Forgets one stream's model, mask and block grid (frames_seen 0), or every stream's with stream == -1.  PARITY UNPINNED. */
int rtmodt_motion_reset(rtmodt_motion *m, int stream);
/* Device time (ms, HIP events around the launches) of the last process call that launched.  PARITY UNPINNED. */
int rtmodt_motion_last_ms(rtmodt_motion *m, float *kernel_ms);
/* Host only, no device needed: csrc/motion_model.h's rule on one cell of luma yc (0..255) of a stream that has seen frames_seen
 * frames: *bg and *dev are updated, *raw is 1 for raw foreground.  Only the five rule fields of cfg are read (learn_shift,
 * learn_shift_fg, threshold, dev_gain, warmup).  The parity surface of csrc/motion_model.h.  PARITY UNPINNED. */
int rtmodt_motion_cell(const rtmodt_motion_cfg *cfg, uint32_t yc, int32_t frames_seen, uint16_t *bg, uint16_t *dev, int32_t *raw);

/* ---- left / removed objects: static foreground the detector has no class for ------------------------------------------------- */
/* A bag left on a platform, a car in a no-parking bay, an exhibit taken away: things that stop moving (the motion detector folds
 * them into its background) and that the 80 classes do not name.  The reference fires on tracked objects only (zone_engine.py) and
 * has no counterpart: PARITY UNPINNED throughout, no default validated on real footage.  PINNED, exactly, against
 * tests/leftobj_ref.py: the cell state, the mask, the regions, the ledger, the events and every count.  csrc/leftobj_rule.h states
 * the rules, csrc/leftobj.hip's header the mask, the regions and the launches; all of it is integer arithmetic.  DELIBERATE LIMITS:
 * a fixed camera (no camera-motion compensation), one luma channel, each handle reads its frames itself (no pixel pass shared with
 * the motion detector).  A handle holds, per stream, the 8-byte cell state of a ceil(height / scale) x ceil(width / scale) grid
 * (bg | cand << 16, unsigned 8.8 fixed point; age << 32; miss << 48; flags << 56, bit 0 = ignore), frames_seen, the last luma grid,
 * the last mask and the object ledger. */
#define RTMODT_LEFTOBJ_WARMUP 0         /* frames_seen < warmup at entry                                                            */
#define RTMODT_LEFTOBJ_CLEAR 1          /* no region                                                                                */
#define RTMODT_LEFTOBJ_STATIC 2         /* at least one region of static foreground                                                 */
#define RTMODT_LEFTOBJ_SCENE_CHANGE 3   /* 1000 * n_fg >= scene_pm * cells: the model restarts, every ledger entry retires RESET    */
#define RTMODT_LEFTOBJ_UNKNOWN 0        /* kinds                                                                                    */
#define RTMODT_LEFTOBJ_ABANDONED 1      /* the region's edge is in the picture                                                      */
#define RTMODT_LEFTOBJ_REMOVED 2        /* the region's edge is in the background model                                             */
#define RTMODT_LEFTOBJ_TRACKED_STATIC 3 /* covered by a track of a report class                                                     */
#define RTMODT_LEFTOBJ_CLEARED 1        /* retirement reasons: unmatched for more than miss_frames calls                            */
#define RTMODT_LEFTOBJ_ABSORBED 2       /* older than absorb_frames: folded into the background                                     */
#define RTMODT_LEFTOBJ_RESET 3          /* a scene change                                                                           */
#define RTMODT_LEFTOBJ_TRACKS_NONE 0    /* track sources                                                                            */
#define RTMODT_LEFTOBJ_TRACKS_LIST 1    /* host lists, one per frame of the call                                                    */
#define RTMODT_LEFTOBJ_TRACKS_BYTETRACK 2
#define RTMODT_LEFTOBJ_TRACKS_DEEPSORT 3
#define RTMODT_LEFTOBJ_TRACKS_OCSORT 4
#define RTMODT_LEFTOBJ_TRACKS_BOTSORT 5
typedef struct rtmodt_leftobj rtmodt_leftobj;
typedef struct rtmodt_leftobj_cfg {
    int32_t streams;            /* 1..1024                                                                                      */
    int32_t height, width;      /* the frame size, 1..32768 each; the grid at most 2^24 cells, all streams 2^28                 */
    int32_t scale;              /* 1, 2, 4 or 8 pixels per cell side                                                            */
    int32_t warmup;             /* 1..255 frames that only learn                                                                */
    int32_t warm_shift;         /* 1..8: bg += (t - bg) >> warm_shift during the warm-up                                        */
    int32_t learn_shift;        /* 1..12: the same for background cells afterwards                                              */
    int32_t threshold;          /* 1..255 luma levels: fg = |t - bg| > threshold << 8                                           */
    int32_t stable;             /* 1..255 luma levels: a foreground cell is stable while |t - cand| <= stable << 8              */
    int32_t cand_shift;         /* 1..8: cand += (t - cand) >> cand_shift on a stable cell                                      */
    int32_t occlusion;          /* 0..254 frames a candidate survives something else in front of it                             */
    int32_t static_frames;      /* 1..65535: static = age >= static_frames                                                      */
    int32_t min_neighbors;      /* 1..9 static cells in the 3 x 3 neighbourhood (the cell included) for a mask cell             */
    int32_t min_area, max_area; /* 1 <= min_area <= max_area cells for a component to be a region                               */
    int32_t max_regions;        /* 1..256 regions stored per frame                                                              */
    int32_t scene_pm;           /* 1..1000 per mille of foreground cells                                                        */
    int32_t max_objects;        /* 1..256 ledger entries per stream                                                             */
    int32_t miss_frames;        /* 0..65535 unmatched calls an entry survives                                                   */
    int32_t alarm_frames;       /* 1..2^30 idle calls until the event                                                           */
    int32_t absorb_frames;      /* 0: never; else 1..2^30 frames after first_frame                                              */
    int32_t covered_pm;         /* 1..1000 per mille of the region's pixel box                                                  */
    int32_t attend_margin;      /* 0..32768 pixels                                                                              */
    int32_t max_tracks;         /* 1..4096 tracks per list                                                                      */
    int32_t n_owner_classes;    /* 0..8                                                                                         */
    int32_t owner_classes[8];
    int32_t n_report_classes;   /* 0..8                                                                                         */
    int32_t report_classes[8];
    int32_t device;
} rtmodt_leftobj_cfg;
typedef struct rtmodt_leftobj_result {
    int32_t status;             /* RTMODT_LEFTOBJ_WARMUP .. SCENE_CHANGE                                                        */
    int32_t stream;
    int32_t frames_seen;        /* after the call: 0 after a SCENE_CHANGE                                                       */
    uint32_t n_fg, n_static;    /* foreground cells; mask cells                                                                 */
    int32_t n_regions;          /* stored: min(n_regions_total, max_regions)                                                    */
    int32_t n_regions_total;
    int32_t n_objects;          /* ledger entries after the call                                                                */
    int32_t n_events, n_retired;
    int32_t dropped;            /* births of this call that found the ledger full                                               */
    int32_t next_oid;           /* the oid the next birth takes                                                                 */
} rtmodt_leftobj_result;
typedef struct rtmodt_leftobj_region {
    int32_t box[4];             /* pixels x0, y0, x1, y1 (x1, y1 exclusive)                                                     */
    int32_t cells[4];           /* cx0, cy0, cx1, cy1 (inclusive)                                                               */
    int32_t area;               /* cells                                                                                        */
    int32_t kind;               /* UNKNOWN, ABANDONED or REMOVED by the edge test                                               */
    int32_t age_min, age_max;
    int32_t covered;            /* bit 0: by a selected track; bit 1: by one of a report class                                  */
    int32_t attended;
    int32_t oid;                /* the ledger entry it matched or bore; 0: none (dropped, or a scene change)                    */
    int32_t root;               /* the region's first cell in raster order                                                      */
} rtmodt_leftobj_region;
typedef struct rtmodt_leftobj_object {
    int64_t first_frame;
    int64_t owner;              /* the last attending track id, -1: none yet                                                    */
    int32_t oid, kind, area, idle, unmatched, alarmed;
    int32_t cells[4];
    int32_t box[4];
} rtmodt_leftobj_object;
typedef struct rtmodt_leftobj_event {
    int64_t first_frame, frame_id, owner;
    int32_t oid, kind, area, reserved;
    int32_t box[4];
} rtmodt_leftobj_event;
typedef struct rtmodt_leftobj_retired { int32_t oid, reason, alarmed, reserved; } rtmodt_leftobj_retired;
typedef struct rtmodt_leftobj_tracks {
    int32_t source;             /* RTMODT_LEFTOBJ_TRACKS_*                                                                      */
    int32_t stride;             /* LIST: entries per row of the arrays below                                                    */
    const int64_t *ids;         /* LIST: [n][stride]                                                                            */
    const float *xyxy;          /*       [n][stride][4]                                                                         */
    const int32_t *cls;         /*       [n][stride]                                                                            */
    const int32_t *n;           /*       [n] entries used, each 0..min(stride, max_tracks)                                      */
    void *tracker;              /* BYTETRACK .. BOTSORT: the handle; its stream s is this handle's stream s                     */
    int32_t report_tsu;         /* BYTETRACK, DEEPSORT: the time_since_update that selects a track (csrc/track_select_dev.h)    */
    int32_t reserved;
} rtmodt_leftobj_tracks;
typedef struct rtmodt_leftobj_out {          /* any pointer may be NULL; all NULL (or out == NULL): nothing is copied back      */
    rtmodt_leftobj_result *results;          /* [n]                                                                             */
    rtmodt_leftobj_region *regions;          /* [n][max_regions]                                                                */
    rtmodt_leftobj_event *events;            /* [n][2 * max_objects]: old rows that alarm, then births that alarm               */
    rtmodt_leftobj_retired *retired;         /* [n][max_objects]                                                                */
    rtmodt_leftobj_object *objects;          /* [n][max_objects]: the ledger after the call                                     */
} rtmodt_leftobj_out;
/* Host only: 1 stream, no frame size, scale 4, warmup 8, warm_shift 2, learn_shift 6, threshold 16, stable 10, cand_shift 3,
 * occlusion 50, static_frames 100, min_neighbors 4, min_area 4, max_area 2^24, max_regions 32, scene_pm 600, max_objects 64,
 * miss_frames 50, alarm_frames 250, absorb_frames 0, covered_pm 500, attend_margin 32, max_tracks 256, owner class 0, no report
 * class.  No default has been validated on real footage.  PARITY UNPINNED. */
void rtmodt_leftobj_default_cfg(rtmodt_leftobj_cfg *cfg);
/* Every parameter is checked before anything is allocated: one outside its range is RTMODT_E_INVALID, a grid above 2^24 cells (or
 * 2^28 over all streams) RTMODT_E_CAPACITY.  PARITY UNPINNED. */
int rtmodt_leftobj_create(const rtmodt_leftobj_cfg *cfg, rtmodt_leftobj **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  PARITY UNPINNED. */
void rtmodt_leftobj_destroy(rtmodt_leftobj *p);
/* One frame for each of n distinct streams, as rtmodt_motion_process takes them; frame_ids[i] is the frame's number (first_frame
 * and the absorb timer count in it).  tracks == NULL: no tracks.  A frame size other than the handle's, a null frame, a stream out
 * of range or named twice, n above the stream count, a list longer than max_tracks and a tracker whose stream count differs from
 * the handle's are RTMODT_E_INVALID with nothing launched.  Nine launches and one memset, whatever the frames show; everything out
 * asks for comes back in one copy.  Streams the call does not name keep their state.  Synchronous.  PARITY UNPINNED. */
int rtmodt_leftobj_process(rtmodt_leftobj *p, const uint8_t *const *frames, const int32_t *streams, const int64_t *frame_ids, int n, int height,
                           int width, int stride_bytes, int mem_kind, const rtmodt_leftobj_tracks *tracks, const rtmodt_leftobj_out *out);
/* One stream's model: the cells as uint64[gh][gw] (layout above), the last luma grid uint8[gh][gw], frames_seen.  cells or luma
 * may be NULL.  PARITY UNPINNED. */
int rtmodt_leftobj_read_state(rtmodt_leftobj *p, int stream, uint64_t *cells, uint8_t *luma, int32_t *frames_seen);
/* Replaces one stream's model (frames_seen 0..2^30), the ignore bits included, so that it survives a restart.  PARITY UNPINNED. */
int rtmodt_leftobj_load_state(rtmodt_leftobj *p, int stream, const uint64_t *cells, const uint8_t *luma, int32_t frames_seen);
/* The mask of the stream's last frame, uint8[gh][gw] of 0 / 1.  PARITY UNPINNED. */
int rtmodt_leftobj_read_mask(rtmodt_leftobj *p, int stream, uint8_t *out);
/* Replaces it (entries 0 / 1), so that a restarted handle answers as the one it was saved from.  PARITY UNPINNED. */
int rtmodt_leftobj_load_mask(rtmodt_leftobj *p, int stream, const uint8_t *mask);
/* The ledger: *n entries in oid order (objects holds max_objects), and the oid the next birth takes.  PARITY UNPINNED. */
int rtmodt_leftobj_read_ledger(rtmodt_leftobj *p, int stream, rtmodt_leftobj_object *objects, int32_t *n, int32_t *next_oid);
/* Replaces the ledger: n <= max_objects entries with oids ascending, each below next_oid, next_oid >= 1.  PARITY UNPINNED. */
int rtmodt_leftobj_load_ledger(rtmodt_leftobj *p, int stream, const rtmodt_leftobj_object *objects, int n, int32_t next_oid);
/* The ignore grid, uint8[gh][gw]: a cell whose entry is not 0 is never static.  The rest of the cell state stays.  PARITY UNPINNED. */
int rtmodt_leftobj_set_ignore(rtmodt_leftobj *p, int stream, const uint8_t *grid);
int rtmodt_leftobj_read_ignore(rtmodt_leftobj *p, int stream, uint8_t *grid);
/* Forgets one stream's model, mask and ledger (frames_seen 0, next oid 1; the ignore grid stays), or every stream's with
 * stream == -1.  PARITY UNPINNED. */
int rtmodt_leftobj_reset(rtmodt_leftobj *p, int stream);
/* Device time (ms, HIP events around the launches) of the last process call that launched.  PARITY UNPINNED. */
int rtmodt_leftobj_last_ms(rtmodt_leftobj *p, float *kernel_ms);
/* Host only, no device needed: csrc/leftobj_rule.h's rule on one cell of luma yc (0..255) of a stream that has seen frames_seen
 * frames: *state (the 8-byte cell) is updated, *fg is 1 for foreground, *is_static 1 for a static cell.  Only the eight rule fields
 * of cfg are read (warmup .. static_frames).  The parity surface of csrc/leftobj_rule.h.  PARITY UNPINNED. */
int rtmodt_leftobj_cell(const rtmodt_leftobj_cfg *cfg, uint32_t yc, int32_t frames_seen, uint64_t *state, int32_t *fg, int32_t *is_static);

/* ---- lens correction: frames are undistorted once, directly after decode ------------------------------------------------------ */
/* Every geometric module of this library (zones, crossings, privacy polygons, heatmap zone sums, the ground-plane speed estimator)
 * assumes a pinhole picture; a short surveillance lens bows straight lines by tens of pixels.  This module produces the rectified
 * picture those modules assume.  The reference has no counterpart: src/ingestion/rtsp_reader.py hands cap.read()'s frame straight
 * to the detector and cv2.undistort appears nowhere in it.  csrc/lens_model.h states the rules (the map of OpenCV's pinhole +
 * Brown-Conrady / rational model, 5 fractional bits, four integer-weighted taps, (sum + 512) >> 10); tests/lens_ref.py restates
 * them and the table and every output byte equal it exactly.  PARITY UNPINNED against cv2.undistort /
 * initUndistortRectifyMap / remap (cv2's table rounds differently and is not installed where this is tested) and on real footage.
 * No fisheye model (its atan cannot be pinned across libm, NumPy and the device): such a lens enters through rtmodt_lens_set_map. */
typedef struct rtmodt_lens rtmodt_lens;
typedef struct rtmodt_lens_cfg {
    int32_t device;
    int32_t streams;            /* 1..1024 lenses                                                                               */
    int32_t src_h, src_w;       /* the source frame size, 1..16384 each                                                         */
    int32_t out_h, out_w;       /* the rectified frame size, 1..16384 each                                                      */
    uint8_t border_bgr[3];      /* what a tap off the source, and a pixel OUTSIDE the map, reads                                 */
    uint8_t reserved;
} rtmodt_lens_cfg;
typedef struct rtmodt_lens_params {
    double fx, fy, cx, cy;      /* source intrinsics; integer pixel coordinates are pixel centres                               */
    double k[8];                /* k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order); all zero: no distortion                            */
    double nfx, nfy, ncx, ncy;  /* output intrinsics; nfx == 0: all four are copied from the source intrinsics                  */
    double r2_limit;            /* 0: none; else an output pixel whose normalised r^2 exceeds it is OUTSIDE                     */
} rtmodt_lens_params;
/* Host only: device 0, 1 stream, every size 0 (the caller sets them), a black border.  No reference counterpart (rtsp_reader.py
 * hands cap.read()'s frame straight to the detector).  PARITY UNPINNED. */
void rtmodt_lens_default_cfg(rtmodt_lens_cfg *cfg);
/* Allocates one table of 8 bytes per output pixel for each stream; no stream has a lens yet.  streams outside 1..1024 or a size
 * outside 1..16384 is RTMODT_E_INVALID.  No reference counterpart (as above).  PARITY UNPINNED. */
int rtmodt_lens_create(const rtmodt_lens_cfg *cfg, rtmodt_lens **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  No reference counterpart.  PARITY UNPINNED. */
void rtmodt_lens_destroy(rtmodt_lens *l);
/* Builds one stream's table on the host from the model (csrc/lens_model.h rules 1 and 2) and uploads it: once per lens, not per
 * frame.  *n_outside (may be null) = the output pixels that are border, so that a caller can choose nfx (zoom) knowingly.  fx, fy,
 * nfx or nfy not finite or not > 0 is RTMODT_E_INVALID and the stream keeps the lens it had.  No reference counterpart.  PARITY
 * UNPINNED. */
int rtmodt_lens_set_model(rtmodt_lens *l, int stream, const rtmodt_lens_params *params, int32_t *n_outside);
/* The same from a caller's map: map_x, map_y float32[out_h][out_w], the source position of each output pixel, the form cv2.remap
 * takes (rule 2 of csrc/lens_model.h; a NaN, an infinity or a position at or beyond +-2^20 is OUTSIDE).  The door for fisheye and
 * any other lens.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_lens_set_map(rtmodt_lens *l, int stream, const float *map_x, const float *map_y, int32_t *n_outside);
/* One stream's table as the device holds it, in canonical form whatever the packing: qx, qy int32[out_h][out_w] (5 fractional
 * bits; 0 where outside), outside uint8[out_h][out_w] of 0 / 1; any array may be null.  A stream without a lens is
 * RTMODT_E_INVALID.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_lens_read_map(rtmodt_lens *l, int stream, int32_t *qx, int32_t *qy, uint8_t *outside);
/* Rectifies n frames in ONE launch: dst[i] (BGR24 out_h x out_w, row pitch dst_stride >= 3 out_w) is src[i] (BGR24 src_h x src_w,
 * row pitch src_stride >= 3 src_w) seen through the lens of streams[i] (streams == NULL: stream i).  Source and destination memory
 * kinds are independent (host -> device is the ingest path: upload and rectify).  Bytes beyond 3 out_w of a destination row are
 * never written.  RTMODT_E_INVALID with nothing launched: a stream without a lens or outside 0..streams - 1, a pitch below 3 w, a
 * null frame, a destination range that overlaps any source range of the call (a gather cannot work in place); more than 65535
 * frames is RTMODT_E_CAPACITY.  The geometry is the handle's.  n == 0 is a no-op.  Synchronous.  No reference counterpart
 * (rtsp_reader.py hands cap.read()'s frame straight to the detector).  PARITY UNPINNED. */
int rtmodt_lens_process(rtmodt_lens *l, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                        int dst_mem_kind, const int32_t *streams, int n);
/* Device time (ms, HIP events around the launch) of the last process call that launched.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_lens_last_ms(rtmodt_lens *l, float *kernel_ms);
/* Host only, float64, no device needed: n points xy[n][2] of the RECTIFIED picture -> the original picture (rule 4's closed form): a
 * rectified box is drawn back on an original frame.  residual is not written (pass null).  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_lens_distort_points(const rtmodt_lens_params *params, const double *xy, int n, double *out_xy, double *residual);
/* Host only: n points of the ORIGINAL picture -> the rectified picture by 20 fixed iterations of OpenCV's fixed-point scheme; zones,
 * tripwires, privacy polygons and the surveyed points of rtmodt_speed_fit_plane are carried over once.  residual[n] (may be null):
 * |distort(undistort(p)) - p| (largest axis) in pixels, +infinity when not a number.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_lens_undistort_points(const rtmodt_lens_params *params, const double *xy, int n, double *out_xy, double *residual);
/* Host only: the canonical table of a model without a device (read_map's arrays, none may be null).  No reference counterpart.
 * PARITY UNPINNED. */
int rtmodt_lens_build_map(const rtmodt_lens_params *params, int src_h, int src_w, int out_h, int out_w, int32_t *qx, int32_t *qy,
                          uint8_t *outside);
/* Host only: the canonical table of a caller's map (set_map's rule) without a device.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_lens_quantise_map(const float *map_x, const float *map_y, int src_h, int src_w, int out_h, int out_w, int32_t *qx, int32_t *qy,
                             uint8_t *outside);

/* ---- snapshot gallery: the best-shot thumbnail of every track, kept on the device ----------------------------------------------- */
/* What the object LOOKED like, for the alert record and the review queue: the reference's alert carries bbox_xyxy and a frame_id and
 * no picture.  Per track the gallery decides on the device whether this frame's view is better than the one kept and, if so,
 * resamples the crop into a fixed-size BGR24 thumbnail slot in device memory; it reports which thumbnails changed and which tracks
 * ended.  csrc/snapshot_rule.h states the per-box rules (crop rectangle, fit, exact area average, score, replacement), the header
 * of csrc/snapshot.hip the ledger rules; tests/snapshot_ref.py restates both and the kernels equal it exactly (DESIGN.md section
 * 32).  No reference counterpart.  PARITY UNPINNED against cv2.resize INTER_AREA, Ultralytics' ObjectCropper and Frigate's
 * snapshot choice; every default is unvalidated on real footage; sharpness is no term of the score.
 * Two launches per call whatever the tracks do: the decision (selection, score, occlusion pairs, ledger merge, slot assignment, a
 * device-side work list) and the resampler, which walks the work list and costs nothing for a track whose thumbnail is kept.
 * Every call carries a frame_id per stream, strictly increasing per stream (else RTMODT_E_INVALID, nothing changes).  Frames are
 * BGR24, h x w at a row pitch of stride_bytes >= 3 w, in host or device memory, and are only read.  A box is SAMPLED when its class
 * passes the filter, its coordinates are finite and its clipped crop has at least min_side pixels on both sides; only sampled
 * tracks touch the ledger. */
#define RTMODT_SNAPSHOT_F_NEW 1        /* the row was created by this call (it always takes its shot) */
#define RTMODT_SNAPSHOT_F_REWRITTEN 2  /* the row's thumbnail was replaced by this call */
#define RTMODT_SNAPSHOT_F_CUT 4        /* the kept shot's box reaches the frame border */
#define RTMODT_SNAPSHOT_F_OCCLUDED 8   /* the kept shot overlapped another sampled box of its list */
typedef struct rtmodt_snapshot rtmodt_snapshot;
typedef struct rtmodt_snapshot_cfg {
    int32_t thumb_h, thumb_w;   /* 8..512 each: the slot */
    int32_t margin_pm;          /* 0..1000: the box grows by this many thousandths of its own width / height on each side */
    int32_t min_side;           /* >= 1: a clipped crop narrower or lower than this is not sampled */
    int32_t area_cap;           /* 1..2^28: the area term of the score saturates here */
    int32_t occl_iou_pm;        /* 0..1000: another sampled box with IoU above this many thousandths halves the score; 0 = off */
    int32_t min_gain_pm;        /* 0..10000: a new shot must beat the kept one by more than this many thousandths */
    int32_t retire_after;       /* >= 0: a row whose track was last sampled more than this many frame ids ago is retired */
    uint8_t pad_bgr[4];         /* the slot around the image (3 used) */
    int32_t max_updated;        /* >= 1: entries of `updated` per stream and call */
    int32_t max_retired;        /* >= 1: entries of `retired` per stream and call */
    int32_t device;
    int32_t n_classes;          /* with `classes`: only these class ids are sampled (at most 256); classes == NULL: all */
    const int32_t *classes;
} rtmodt_snapshot_cfg;
/* One thumbnail this call wrote, in list order.  `track`: index into the caller's list, or into the tracker's list. */
typedef struct rtmodt_snapshot_update {
    int64_t track_id;
    int64_t score;
    int32_t slot, flags, track, reserved;
} rtmodt_snapshot_update;
/* One row this call retired, in ascending track id: the best shot's frame id, box, confidence and class. */
typedef struct rtmodt_snapshot_retired {
    int64_t track_id;
    int64_t best_frame, first_seen, last_seen;
    float xyxy[4];
    float conf;
    int32_t slot, cls, n_rewrites;
} rtmodt_snapshot_retired;
/* What one call hands back; the struct pointer and every member may be null.  With none given nothing crosses to the host and the
 * call does not wait for the device; otherwise the streams' result blocks come back in one copy.  One-stream calls: updated
 * [max_updated], retired [max_retired], counts [1]; all-stream calls: [n_streams][...] and counts [n_streams].  n_updated /
 * n_retired are the numbers delivered; n_rewritten counts the thumbnails of EXISTING rows this call replaced (new rows excluded). */
typedef struct rtmodt_snapshot_out {
    rtmodt_snapshot_update *updated;
    int32_t *n_updated;
    rtmodt_snapshot_retired *retired;
    int32_t *n_retired;
    int32_t *n_rewritten;
} rtmodt_snapshot_out;
/* The plan of one box (the parity surface of csrc/snapshot_rule.h): rectangles are inclusive x0, y0, x1, y1. */
typedef struct rtmodt_snapshot_plan_out {
    int32_t sampled;            /* 0: the box is skipped, nothing else is written */
    int32_t raw[4];             /* truncated corners, neither grown nor clipped */
    int32_t box[4];             /* raw clipped to the frame (x1 < x0 or y1 < y0: empty) */
    int32_t crop[4];            /* grown by the margin and clipped: the pixels that are read */
    int32_t sw, sh;             /* the crop's size */
    int32_t dw, dh, ox, oy;     /* size and place of the image in the slot */
    int32_t cut, area;          /* the raw rectangle reaches the frame border; min(area of box, area_cap) */
} rtmodt_snapshot_plan_out;
/* thumb 96 x 96, margin 100, min_side 8, area_cap 2^16, occl_iou_pm 300, min_gain_pm 100, retire_after 30, pad 114 114 114 (the
 * letterbox's grey), max_updated / max_retired 1024, device 0, every class. */
void rtmodt_snapshot_default_cfg(rtmodt_snapshot_cfg *cfg);
/* n_streams independent ledgers and thumbnail atlases; max_tracks <= 4096.  A ledger holds 2 x max_tracks rows sorted by track id,
 * and a stream's atlas one BGR24 slot of thumb_h x thumb_w per row at a row pitch of align_up(3 thumb_w, 16).  The rules, per call
 * and stream, in this order:
 *   retire   a row with frame_id - last_seen > retire_after leaves the ledger and is reported in `retired` (a track of the same id
 *            sampled in this call starts a new row).  Its slot is free from the NEXT call on that stream: until then the
 *            thumbnail stays intact, which is the host's window to read or encode it;
 *   score    every sampled box gets its score (snapshot_rule.h);
 *   keep     a sampled track with a row: last_seen = frame_id; its thumbnail is rewritten iff score * 1000 > best_score * (1000 +
 *            min_gain_pm), and then best_score / best_frame / box / conf / cls / flags follow and n_rewrites gains one;
 *   birth    a sampled track without a row takes its shot at once; the new rows of a call take the slots that were free when the
 *            call began, in ascending slot index, in list order.
 * Capacity, as the crossing counter's: the call that needs more than 2 x max_tracks rows, or more free slots than there are,
 * returns RTMODT_E_CAPACITY, the idle rows are dropped (their slots, and those of the rows retired by that call, are reused at once)
 * and the stream stays in error for good (every later call that asks for output, and _state, returns RTMODT_E_CAPACITY) until
 * rtmodt_snapshot_reset.  More updated or retired entries than the maxima: RTMODT_E_CAPACITY with the first ones delivered and the
 * counts reported; every thumbnail is written all the same and the stream goes on working.  A call made without outputs cannot
 * report either.  The error message names the atlas bytes when the allocation fails. */
int rtmodt_snapshot_create(const rtmodt_snapshot_cfg *cfg, int n_streams, int max_tracks, rtmodt_snapshot **out);
/* Waits for the handle's queued work, frees everything; null is allowed. */
void rtmodt_snapshot_destroy(rtmodt_snapshot *h);
/* One stream, a caller-supplied track list (any order, unique ids, at most max_tracks) and its frame.  conf may be null: every
 * entry then scores as confidence 1. */
int rtmodt_snapshot_process(rtmodt_snapshot *h, int stream, const int64_t *track_ids, const float *xyxy, const float *conf,
                            const int32_t *cls, int n, const uint8_t *frame, int fh, int fw, int stride_bytes, int mem_kind,
                            int64_t frame_id, const rtmodt_snapshot_out *out);
/* Every stream in one call: track_ids / conf / cls [n_streams][stride], xyxy [n_streams][stride][4], n [n_streams], frames
 * [n_streams] of one geometry, frame_id [n_streams]. */
int rtmodt_snapshot_process_batch(rtmodt_snapshot *h, const int64_t *track_ids, const float *xyxy, const float *conf, const int32_t *cls,
                                  const int32_t *n, int stride, const uint8_t *const *frames, int fh, int fw, int stride_bytes,
                                  int mem_kind, const int64_t *frame_id, const rtmodt_snapshot_out *out);
/* Every stream of a ByteTrack handle, straight on its device-resident state (box, conf, cls) and on the HIP stream its last update
 * ran on: exactly the tracks rtmodt_crossing_process_tracker passes.  frames / frame_id [n_streams of the tracker]. */
int rtmodt_snapshot_process_tracker(rtmodt_snapshot *h, rtmodt_tracker *trk, const uint8_t *const *frames, int fh, int fw,
                                    int stride_bytes, int mem_kind, const int64_t *frame_id, int report_tsu, const rtmodt_snapshot_out *out);
/* The same on a DeepSORT handle: the tracks rtmodt_crossing_process_deepsort passes. */
int rtmodt_snapshot_process_deepsort(rtmodt_snapshot *h, rtmodt_deepsort *ds, const uint8_t *const *frames, int fh, int fw,
                                     int stride_bytes, int mem_kind, const int64_t *frame_id, int report_tsu, const rtmodt_snapshot_out *out);
/* The same on an OC-SORT handle: the tracks rtmodt_crossing_process_ocsort passes. */
int rtmodt_snapshot_process_ocsort(rtmodt_snapshot *h, rtmodt_ocsort *oc, const uint8_t *const *frames, int fh, int fw, int stride_bytes,
                                   int mem_kind, const int64_t *frame_id, const rtmodt_snapshot_out *out);
/* The same on a BoT-SORT handle: the tracks rtmodt_crossing_process_botsort passes. */
int rtmodt_snapshot_process_botsort(rtmodt_snapshot *h, rtmodt_botsort *bot, const uint8_t *const *frames, int fh, int fw, int stride_bytes,
                                    int mem_kind, const int64_t *frame_id, const rtmodt_snapshot_out *out);
/* The device address of one stream's atlas: slot s begins at dev_ptr + s * slot_bytes, rows `pitch` bytes apart, so that the JPEG
 * encoder takes slots where they lie (frame pointers dev_ptr + slot * slot_bytes, h = thumb_h, w = thumb_w, stride = pitch,
 * RTMODT_MEM_DEVICE).  Waits for the handle's queued work. */
int rtmodt_snapshot_atlas(rtmodt_snapshot *h, int stream, void **dev_ptr, size_t *slot_bytes, int32_t *pitch);
/* n thumbnails of one stream to the host, tight thumb_h * thumb_w * 3 bytes each, in the order of slots[n]. */
int rtmodt_snapshot_read(rtmodt_snapshot *h, int stream, const int32_t *slots, int n, uint8_t *out);
/* Ledger snapshot of one stream, rows in ascending track id (the parity surface of tests/snapshot_ref.py); any array may be null.
 * ints[row] = {slot, cls, n_rewrites, flags}; xyxy / conf / cls are the best shot's; bitmap [(2 max_tracks + 31) / 32] words, bit
 * s set while slot s belongs to a row.  Arrays sized 2 x max_tracks rows.  A stream in error fills them all the same (the rows of
 * the overflowing call and of the calls since) and returns RTMODT_E_CAPACITY. */
int rtmodt_snapshot_state(rtmodt_snapshot *h, int stream, int64_t *ids, int64_t *best_score, int64_t *best_frame, int64_t *first_seen,
                          int64_t *last_seen, float *xyxy, float *conf, int32_t *ints, uint32_t *bitmap, int32_t *n);
/* Empties one stream's ledger and bitmap, forgets its last frame_id and its error; the atlas bytes stay as they are. */
int rtmodt_snapshot_reset(rtmodt_snapshot *h, int stream);
/* Host only, no device needed: the crop rectangle, the fit and the placement of one box xyxy[4] of any class in an h x w frame. */
int rtmodt_snapshot_plan(const rtmodt_snapshot_cfg *cfg, const float *xyxy, int h, int w, rtmodt_snapshot_plan_out *out);
/* Stateless, the same resampler without a ledger: box i, xyxy[i] of frames[frame_idx[i]], becomes thumbnail i of `out`, tight
 * thumb_h * thumb_w * 3 bytes each, in host or device memory (out_mem_kind).  sampled[i] (may be null) = 1 when the box was
 * sampled; the thumbnail of a box that is not is left untouched.  The class filter does not apply.  Synchronous. */
int rtmodt_snapshot_crop(rtmodt_snapshot *h, const uint8_t *const *frames, int n_frames, int fh, int fw, int stride_bytes, int mem_kind,
                         const float *xyxy, const int32_t *frame_idx, int n_boxes, uint8_t *out, int out_mem_kind, int32_t *sampled);
/* The review queue (low-confidence detections for a human to label), stateless: the detections of the detector's newest batch with
 * conf_lo <= confidence < conf_hi, read from its device-resident outputs behind the NMS on its post-processing stream -- no box
 * crosses to the host.  Per frame the first max_out of them (1..max_det) in slot order: thumbnail [frame][k] of `out` ([n][max_out],
 * tight thumb_h * thumb_w * 3 bytes each, host or device memory), index [n][max_out] = the detection's slot (-1 past the frame's
 * count), counts [n], sampled [n][max_out] (may be null) = 1 when the box was sampled; other thumbnails are left untouched.
 * frames [n <= the batch's frames]: the frames the batch was detected on.  The class filter does not apply.  Synchronous. */
int rtmodt_snapshot_crop_detector(rtmodt_snapshot *h, rtmodt_detector *det, const uint8_t *const *frames, int n, int fh, int fw,
                                  int stride_bytes, int mem_kind, float conf_lo, float conf_hi, int max_out, uint8_t *out,
                                  int out_mem_kind, int32_t *index, int32_t *counts, int32_t *sampled);
/* Device time (ms, HIP events around the two launches) of the last _process*, _crop or _crop_detector call. */
int rtmodt_snapshot_last_ms(rtmodt_snapshot *h, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Cross-camera linker (csrc/crosscam.hip; the per-pair rules in csrc/crosscam_rule.h): the tracks of n_streams cameras are linked
 * to site-wide identities.  The reference has no counterpart (its Track has no global id, its tracker sees one source).  PARITY
 * UNPINNED: no published multi-camera tracker is installed where this runs; every default is validated on no real footage.
 *
 * An ENTRY is (local track id, class, int8 row of dim values).  An IDENTITY holds gid (from 1, never reused), class, the smoothed
 * feature s16 / s8, first_seen and last_seen[n_streams] (the call of the last sighting per stream, 0 never); the table is in gid
 * order.  Per stream a ledger binds local ids to gids.  The call counter c is 1 in the first call.  Per call, in order:
 *   1. retire   an identity with c - max(last_seen) > max_age leaves with its bindings and is reported; a binding not sighted for
 *               more than bind_age calls is dropped;
 *   2. bound    an entry whose local id is in its stream's ledger is BOUND (its identity is live in the stream); any other entry
 *               with a non-zero row is a query, numbered in (stream, entry) order; those past max_queries are DEFERRED; a zero
 *               row is NO_DESCRIPTOR;
 *   3. sim      dot = <q, s8> (int32), sim = dot <= 0 ? 0 : min(1000, 1000 dot / max(1, isqrt(|q|^2 |s8|^2))), all exact;
 *   4. match    per stream the exact maximum of sum(sim - min_sim_milli + 1) over the admissible pairs, one-to-one: sim >=
 *               min_sim_milli, equal classes (match_class), the identity not live in the stream, and some stream f with
 *               last_seen[f] > 0 and tmin[f][s] <= c - last_seen[f] <= tmax[f][s] on start-of-call values.  A matched query is
 *               LINKED, an older binding of that identity in the stream is removed.  Past the solver's contested limits (256
 *               rows / 256 columns / 2048 pairs) the stream's queries are UNBOUND this call and the stream's sticky error is 2;
 *   5. births   serially in query order over the rest: JOINED to an identity born earlier in this call by another stream (sim
 *               against its birth feature >= min_sim_milli, equal classes, not live in the stream, tmin[f][s] == 0 <= tmax[f][s]
 *               for a stream f it is live in; best sim, then lowest gid), else BORN, else TABLE_FULL;
 *   6. feature  BoT-SORT's integer EMA once per sighting with a non-zero row, in ascending stream order; last_seen[s] = c.
 * sim of an entry: LINKED against the identity's s8, JOINED against the birth feature, else 0.  An event per LINKED / JOINED
 * entry, in (stream, entry) order; from_stream = the stream of the greatest start-of-call last_seen (lowest on a tie; JOINED:
 * the founder's stream, gap 0). */
typedef struct rtmodt_crosscam rtmodt_crosscam;
#define RTMODT_CROSSCAM_NONE 0
#define RTMODT_CROSSCAM_BOUND 1
#define RTMODT_CROSSCAM_LINKED 2
#define RTMODT_CROSSCAM_JOINED 3
#define RTMODT_CROSSCAM_BORN 4
#define RTMODT_CROSSCAM_NO_DESCRIPTOR 5
#define RTMODT_CROSSCAM_DEFERRED 6
#define RTMODT_CROSSCAM_TABLE_FULL 7
#define RTMODT_CROSSCAM_UNBOUND 8
typedef struct rtmodt_crosscam_cfg {
    int32_t device;
    int32_t n_streams;       /* 1..64                                                                          */
    int32_t dim;             /* 64..512 in multiples of 64                                                     */
    int32_t max_tracks;      /* entries per stream per call, 1..256                                            */
    int32_t max_identities;  /* 1..4096                                                                        */
    int32_t max_queries;     /* per call over all streams, 1..1024 (with max_identities: the int32 product buffer
                              * max_queries x (max_identities + max_queries), 21 MB at the caps; design limits)  */
    int32_t min_sim_milli;   /* 1..1000                                                                        */
    int32_t max_age;         /* calls                                                                          */
    int32_t bind_age;        /* calls; 0 = max_age                                                             */
    int32_t match_class;
} rtmodt_crosscam_cfg;
typedef struct rtmodt_crosscam_event {
    int64_t gid, local_id;
    int32_t stream, from_stream, gap, sim;
} rtmodt_crosscam_event;
typedef struct rtmodt_crosscam_retired {
    int64_t gid, first_seen, last_seen;
    uint64_t stream_mask;    /* bit s: the identity was sighted in stream s                                    */
} rtmodt_crosscam_retired;
/* Any pointer may be null; with all null nothing is copied back.  gid / status / sim [n_streams][max_tracks]; events
 * [n_streams * max_tracks]; retired [max_identities]; counters[8] = {call, identities, next gid, queries, deferred, table-full,
 * events, retired}. */
typedef struct rtmodt_crosscam_out {
    int64_t *gid;
    int32_t *status, *sim;
    rtmodt_crosscam_event *events;
    int32_t *n_events;
    rtmodt_crosscam_retired *retired;
    int32_t *n_retired;
    int64_t *counters;
} rtmodt_crosscam_out;
void rtmodt_crosscam_default_cfg(rtmodt_crosscam_cfg *cfg);
/* A parameter outside its range is RTMODT_E_INVALID with nothing allocated.  The transit table starts at (0, max_age) everywhere. */
int rtmodt_crosscam_create(const rtmodt_crosscam_cfg *cfg, rtmodt_crosscam **out);
/* Waits for the handle's queued work, frees everything; null is allowed. */
void rtmodt_crosscam_destroy(rtmodt_crosscam *h);
/* The camera topology, one ordered pair of streams: min_calls = 0 for overlapping views, > 0 for disjoint ones, max_calls <
 * min_calls for "cannot get there". */
int rtmodt_crosscam_set_transit(rtmodt_crosscam *h, int src, int dst, int min_calls, int max_calls);
/* One call on host lists: track_ids / cls [n_streams][stride], rows [n_streams][stride][dim], n [n_streams].  A local id twice
 * in one stream's list, or more than max_tracks entries, is RTMODT_E_INVALID with nothing launched.  Float embeddings pass through
 * rtmodt_appearance_quantize first.  One memset and nine launches, whatever the tracks do; the outputs in one copy. */
int rtmodt_crosscam_process(rtmodt_crosscam *h, const int64_t *track_ids, const int32_t *cls, const int8_t *rows, const int32_t *n,
                            int stride, const rtmodt_crosscam_out *out);
/* One call on a BoT-SORT handle's device-resident state, queued on the HIP stream its last update ran on: the tracks
 * rtmodt_crossing_process_botsort passes, each with its smoothed int8 feature.  A handle of another dim, stream count or device,
 * one without appearance, or one with more tracks than max_tracks is RTMODT_E_INVALID with nothing launched. */
int rtmodt_crosscam_process_botsort(rtmodt_crosscam *h, rtmodt_botsort *bot, const rtmodt_crosscam_out *out);
/* The same on a DeepSORT handle: confirmed tracks matched this frame, each with the newest row of its gallery ring. */
int rtmodt_crosscam_process_deepsort(rtmodt_crosscam *h, rtmodt_deepsort *ds, const rtmodt_crosscam_out *out);
/* The whole state (the parity surface of tests/crosscam_ref.py, and what a restart carries over); any array but header may be
 * null.  header[3] = {calls so far, next gid, identities n}; gid / cls / first_seen [n], last_seen [n][n_streams], s16 / s8
 * [n][dim] (arrays sized for max_identities); n_bind [n_streams]; bind_lid / bind_gid / bind_last [n_streams][max_identities], a
 * stream's bindings in ascending local id.  Waits for the handle's queued work. */
int rtmodt_crosscam_state(rtmodt_crosscam *h, int64_t *header, int64_t *gid, int32_t *cls, int64_t *first_seen, int64_t *last_seen,
                          int16_t *s16, int8_t *s8, int32_t *n_bind, int64_t *bind_lid, int64_t *bind_gid, int64_t *bind_last);
/* Replaces the state by one rtmodt_crosscam_state gave (same n_streams, dim and max_identities); the sticky errors are cleared.
 * Unordered gids or local ids, a binding to no identity, or counts past the handle are RTMODT_E_INVALID and change nothing. */
int rtmodt_crosscam_load(rtmodt_crosscam *h, const int64_t *header, const int64_t *gid, const int32_t *cls, const int64_t *first_seen,
                         const int64_t *last_seen, const int16_t *s16, const int8_t *s8, const int32_t *n_bind, const int64_t *bind_lid,
                         const int64_t *bind_gid, const int64_t *bind_last);
/* The sticky error per stream (0 none, 2 the matching was too dense), and its reset. */
int rtmodt_crosscam_errors(rtmodt_crosscam *h, int32_t *err);
int rtmodt_crosscam_clear_errors(rtmodt_crosscam *h);
/* Device time (ms, HIP events around the launches) of the last _process* call. */
int rtmodt_crosscam_last_ms(rtmodt_crosscam *h, float *kernel_ms);
/* The GEMM alone, stateless: dots [nq][nt] = q (nq x dim, int8) times t (nt x dim, int8) transposed, exact in int32, and sim
 * [nq][nt] by rule 3; either output may be null.  nq <= 1024, nt <= 4096.  Synchronous. */
int rtmodt_crosscam_similarity(int device, const int8_t *q, int nq, const int8_t *t, int nt, int dim, int32_t *dots, int32_t *sim);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Appearance index (csrc/index.hip; the per-row rules in csrc/index_rule.h): a device-resident, append-only ring of descriptor
 * rows with metadata, searched by similarity: "where else, and when, did this one appear?".  Up to 64 queries per call get the
 * exact, deterministic top-k under filters.  The reference has no counterpart (its Track has no descriptor, its web API answers
 * with the detections of one image).  PARITY UNPINNED: no published vector index is installed where this runs (and none of them
 * ranks in integers); tests/index_ref.py restates the rules below and every output equals it.
 *
 * A ROW holds dim int8 values, rid (from 1, never reused, below 2^40), key (the caller's: a gid, or stream and track id packed),
 * stream (0..63), cls, t (the caller's clock), n2 = sum v^2 (computed on the device at add) and a dead flag.  Row rid lives in
 * slot (rid - 1) % capacity; a newer row overwrites the oldest.  next_rid lives on the device.
 *   similarity   dot = <q, row> exact in int32; ppm = dot <= 0 ? 0 : min(1000000, 1000000 dot / max(1, isqrt(|q|^2 n2))), floor
 *                division; ppm / 1000 is rule 3 of the cross-camera linker;
 *   eligibility  the slot is filled and the row not dead; t0 <= t <= t1; bit `stream` of stream_mask is set; cls < 0 or the row's
 *                class equals it; key != exclude_key (INT64_MIN: none); ppm >= min_ppm (1..1000000).  A zero row never is;
 *   rank         ppm << 40 | rid, descending: the best similarity first, the newest row first on a tie.  Ranks are distinct, so
 *                the top-k is unique.
 * Not here: approximate indexes (IVF / PQ / HNSW), thumbnails of the hits.  Every entry point waits for what it queued. */
typedef struct rtmodt_index rtmodt_index;
#define RTMODT_INDEX_NO_KEY INT64_MIN
typedef struct rtmodt_index_cfg {
    int32_t device;
    int32_t dim;             /* 64..512 in multiples of 64                                                     */
    int32_t capacity;        /* rows of the ring, 1..2^22                                                      */
    int32_t max_queries;     /* per search, 1..64                                                              */
    int32_t max_k;           /* 1..64                                                                          */
    int32_t max_add;         /* rows per add, 1..65536                                                         */
    int32_t chunk_rows;      /* rows one workgroup scans: 0 = chosen by the library, else a multiple of 64 that
                              * cuts capacity into at most 256 chunks                                          */
} rtmodt_index_cfg;
typedef struct rtmodt_index_filter {
    int64_t t0, t1;          /* inclusive                                                                      */
    uint64_t stream_mask;
    int64_t exclude_key;     /* RTMODT_INDEX_NO_KEY: none                                                      */
    int32_t cls;             /* < 0: any                                                                       */
    int32_t min_ppm;         /* 1..1000000                                                                     */
} rtmodt_index_filter;
typedef struct rtmodt_index_hit {
    int64_t rid, key, t;
    int32_t stream, cls, ppm, reserved;
} rtmodt_index_hit;
void rtmodt_index_default_cfg(rtmodt_index_cfg *cfg);
/* A parameter outside its range is RTMODT_E_INVALID with nothing allocated. */
int rtmodt_index_create(const rtmodt_index_cfg *cfg, rtmodt_index **out);
/* Waits for the handle's queued work, frees everything; null is allowed. */
void rtmodt_index_destroy(rtmodt_index *h);
/* Appends n rows [n][dim] from host or device memory (mem_kind: RTMODT_MEM_*) with their host arrays keys / streams / cls / t
 * [n].  The rows get next_rid .. in list order, their norms are computed on the device; *first_rid (may be null) is the first
 * one.  n > max_add, or a stream outside 0..63, is RTMODT_E_INVALID with nothing changed.  Two launches. */
int rtmodt_index_add(rtmodt_index *h, const int8_t *rows, int mem_kind, const int64_t *keys, const int32_t *streams, const int32_t *cls,
                     const int64_t *t, int n, int64_t *first_rid);
/* Appends from a cross-camera linker's device-resident table, queued behind the linker's last _process* on the stream that ran
 * on.  With c the call the linker just made: an identity is appended when max over s of last_seen[s] == c and (c - first_seen)
 * % every == 0, as a row with key = gid, stream = the lowest s with last_seen[s] == c, its class, its s8 and time t; in gid
 * order (a workgroup prefix sum, no atomic).  *n_added (may be null) is the count.  A linker of another dim or device, one with
 * max_identities > max_add, or every < 1 is RTMODT_E_INVALID with nothing changed.  Three launches. */
int rtmodt_index_add_crosscam(rtmodt_index *h, rtmodt_crosscam *linker, int64_t t, int every, int32_t *n_added);
/* nq query rows [nq][dim] (host) with one filter each, k hits at most per query: hits [nq][k] in rank order, unused entries
 * zero, n_hits [nq].  nq > max_queries, k > max_k or a min_ppm outside 1..1000000 is RTMODT_E_INVALID with nothing launched.
 * Two launches whatever the archive holds (the scan reads rows and metadata once for all queries and writes no product; the
 * merge picks the k best of the chunks' lists), the outputs in one copy. */
int rtmodt_index_search(rtmodt_index *h, const int8_t *queries, int nq, const rtmodt_index_filter *filters, int k, rtmodt_index_hit *hits,
                        int32_t *n_hits);
/* Every live row whose key is among keys [n <= 4096] becomes dead (it stays in its slot until overwritten and is never a hit
 * again); *n_marked (may be null) is how many rows that were. */
int rtmodt_index_forget(rtmodt_index *h, const int64_t *keys, int n, int64_t *n_marked);
/* The whole archive in slot order (the parity surface of tests/index_ref.py, and what a restart carries over); any array but
 * header may be null.  header[2] = {next_rid, rows in the ring}; rows [capacity][dim]; rid / key / t (int64), stream / cls / n2 /
 * dead (int32) [capacity]; an empty slot has rid 0 and zeros everywhere. */
int rtmodt_index_state(rtmodt_index *h, int64_t *header, int8_t *rows, int64_t *rid, int64_t *key, int64_t *t, int32_t *stream, int32_t *cls,
                       int32_t *n2, int32_t *dead);
/* Replaces the archive by one rtmodt_index_state gave (same dim and capacity; n2 is computed again).  A rid that is not the one
 * its slot holds at next_rid (so also a rid >= next_rid), a stream outside 0..63 or a dead flag other than 0 / 1 is
 * RTMODT_E_INVALID and changes nothing. */
int rtmodt_index_load(rtmodt_index *h, int64_t next_rid, const int8_t *rows, const int64_t *rid, const int64_t *key, const int64_t *t,
                      const int32_t *stream, const int32_t *cls, const int32_t *dead);
/* Device time (ms, HIP events around the launches) of the last add / add_crosscam and of the last search. */
int rtmodt_index_last_ms(rtmodt_index *h, float *add_ms, float *search_ms);

/* ---- compositor: video-wall mosaics, sub-streams and zoom insets, BGR24 or 4:2:0 out ---- */
/* A static LAYOUT (sources, outputs, cells) is set once and kept on the device; one RUN per frame set reads the sources where they
 * lie and writes every output in ONE launch.  csrc/compose_rule.h states every rule (crop, fit, the three kinds of axis, the
 * one-rounding pixel, painting order, the forward BT.601 conversion), tests/compose_ref.py restates them and every output byte
 * equals that restatement.  No reference counterpart (its web page shows one image and tools/run_pipeline.py writes the full frame);
 * PARITY UNPINNED against cv2.resize (INTER_AREA / INTER_LINEAR), cv2.cvtColor(COLOR_BGR2YUV_I420) and any encoder's reading of
 * the NV12.  Not here: text and borders (the renderer draws on an output), alpha blending, other filters, BT.709 / full range. */
typedef struct rtmodt_compose rtmodt_compose;
#define RTMODT_COMPOSE_STRETCH 0   /* the crop is mapped onto the whole rectangle                                              */
#define RTMODT_COMPOSE_FIT 1       /* aspect kept, picture centred, the bars take the cell's pad colour                         */
#define RTMODT_COMPOSE_FILL 2      /* aspect kept, the crop is cut centrally until it covers the rectangle: no bars             */
#define RTMODT_COMPOSE_SHRINK 0    /* kinds of axis in rtmodt_compose_plan_out: exact area average                              */
#define RTMODT_COMPOSE_COPY 1      /* one tap                                                                                   */
#define RTMODT_COMPOSE_ENLARGE 2   /* two taps with 11-bit weights (cv::resize INTER_LINEAR tables)                             */
typedef struct rtmodt_compose_cfg {
    int32_t device;
    int32_t max_sources;   /* 64: 1..64                                                                                      */
    int32_t max_outputs;   /* 16: 1..16                                                                                      */
    int32_t max_cells;     /* 64: cells per output, 1..64                                                                    */
    int32_t max_dim;       /* 16384: largest height / width of a source or an output, 1..16384                               */
} rtmodt_compose_cfg;
typedef struct rtmodt_compose_src_desc { int32_t h, w; } rtmodt_compose_src_desc;          /* BGR24 */
typedef struct rtmodt_compose_out_desc {
    int32_t h, w;
    int32_t pixel_format;        /* RTMODT_PIX_BGR24 / _NV12 / _I420 (4:2:0: h and w even)                                    */
    uint8_t background_bgr[3];   /* every pixel no cell covers                                                               */
    uint8_t reserved;
} rtmodt_compose_out_desc;
typedef struct rtmodt_compose_cell {
    int32_t output, source;
    int32_t x, y, w, h;                          /* the rectangle inside the output, NOT clipped (4:2:0 outputs: all four even)   */
    int32_t crop_x, crop_y, crop_w, crop_h;      /* the part of the source shown, inside the source; 0, 0, 0, 0 = all of it       */
    int32_t fit;                                 /* RTMODT_COMPOSE_STRETCH / _FIT / _FILL                                         */
    uint8_t pad_bgr[3];                          /* FIT's bars                                                                    */
    uint8_t reserved0;
    uint8_t offline_bgr[3];                      /* the whole rectangle in a run whose source pointer is null (camera down)       */
    uint8_t reserved1;
} rtmodt_compose_cell;
typedef struct rtmodt_compose_plan_out {
    int32_t crop[4];             /* x, y, w, h of the effective crop inside the source (FILL cuts it)                          */
    int32_t inner[4];            /* x, y, w, h of the picture inside the OUTPUT (FIT shrinks it; 4:2:0: even)                   */
    int32_t kind_x, kind_y;      /* RTMODT_COMPOSE_SHRINK / _COPY / _ENLARGE                                                   */
} rtmodt_compose_plan_out;
/* Host only: the limits above, device 0.  No reference counterpart, PARITY UNPINNED. */
void rtmodt_compose_default_cfg(rtmodt_compose_cfg *cfg);
/* Host only (the device is first touched by set_layout): a limit outside its range is RTMODT_E_INVALID.  No reference
 * counterpart, PARITY UNPINNED. */
int rtmodt_compose_create(const rtmodt_compose_cfg *cfg, rtmodt_compose **out);
void rtmodt_compose_destroy(rtmodt_compose *h);
/* Replaces the layout.  cells[] is the painting order: a later cell lies on top.  EVERYTHING is checked before anything is allocated
 * or touched: counts past the handle's limits are RTMODT_E_CAPACITY; a size outside 1..max_dim, an odd 4:2:0 size or rectangle, an
 * unknown format or fit, an index outside its list, a rectangle that leaves its output or a crop that leaves its source are
 * RTMODT_E_INVALID.  A rejected layout leaves the previous one in force.  The tile work list and the enlarging axes' tables are
 * built here and kept on the device.  No reference counterpart, PARITY UNPINNED. */
int rtmodt_compose_set_layout(rtmodt_compose *h, const rtmodt_compose_src_desc *sources, int n_sources, const rtmodt_compose_out_desc *outputs,
                              int n_outputs, const rtmodt_compose_cell *cells, int n_cells);
/* Re-plans ONE cell (follow-zoom): its crop becomes x, y, w, h (0, 0, 0, 0: the whole source); the rest of the layout, the tile
 * work list included, is left alone.  A crop that leaves the source is RTMODT_E_INVALID and changes nothing.  No reference
 * counterpart, PARITY UNPINNED. */
int rtmodt_compose_set_crop(rtmodt_compose *h, int cell, int x, int y, int w, int hgt);
/* One run, one launch.  src[n_sources]: BGR24 frames, src_pitch[i] bytes per row (src_pitch null: 3w), host or device per
 * src_mem_kind; a null src[i] is a camera that is down: its cells show their offline colour.  dst[n_outputs] with dst_fmt[i]
 * placing output i's planes as rtmodt_detector_enqueue_batch_fmt reads them (same zero defaults, same checks; dst_fmt null: all
 * defaults; the pixel format must be the layout's).  Device destinations are written in place; a host destination is composed in
 * the handle's own buffer of that output and its rows are copied back; a null dst[i] (or dst null) leaves output i in the handle's
 * own buffer (rtmodt_compose_output).  Only a row's 3w bytes (w per plane row) are ever written.  Refused with RTMODT_E_INVALID
 * before anything is launched or written: no layout, a bad mem_kind, pitch or format, a destination that overlaps a source or
 * another destination.  No reference counterpart, PARITY UNPINNED. */
int rtmodt_compose_run(rtmodt_compose *h, const uint8_t *const *src, const int32_t *src_pitch, int src_mem_kind, uint8_t *const *dst,
                       const rtmodt_frame_format *dst_fmt, int dst_mem_kind);
/* The handle's own device buffer of output i, as rtmodt_snapshot_atlas hands out the atlas: rtmodt_render_batch and
 * rtmodt_jpeg_encode_batch take a BGR24 output where it lies.  pitch: bytes per row (BGR24) or per Y row; a 4:2:0 output's chroma
 * follows with rtmodt_frame_format's defaults for that pitch.  Valid until the next set_layout.  No reference counterpart, PARITY
 * UNPINNED. */
int rtmodt_compose_output(rtmodt_compose *h, int i, uint8_t **dev_ptr, size_t *pitch);
/* Device time (ms, HIP events around the launch) of the last run.  No reference counterpart. */
int rtmodt_compose_last_ms(rtmodt_compose *h, float *kernel_ms);
/* Host only: set_layout's checks (against the largest limits) and, per cell, what it would plan: plans[n_cells].  Python's point
 * mapping and the tests read it.  No reference counterpart, PARITY UNPINNED. */
int rtmodt_compose_plan(const rtmodt_compose_src_desc *sources, int n_sources, const rtmodt_compose_out_desc *outputs, int n_outputs,
                        const rtmodt_compose_cell *cells, int n_cells, rtmodt_compose_plan_out *plans);

/* ---- stabiliser: frames of a shaking camera are steadied once, ahead of every fixed-camera stage ------------------------------- */
/* The motion detector, the left-object detector, the speed estimator, the heatmap, zones, tripwires and privacy polygons assume a
 * FIXED camera; one on a pole or a gantry shakes by several pixels.  Per stream this module keeps a camera path on the device,
 * moves it by one similarity per call (supplied, or estimated by an rtmodt_gmc from the same frames with nothing crossing the
 * host between the estimate and the pixels) and resamples the frame into the stabilised picture.  The reference has no
 * counterpart: src/ingestion/rtsp_reader.py hands cap.read()'s frame to the detector, and cv2.estimateAffinePartial2D /
 * warpAffine appear nowhere in it.  csrc/stab_rule.h states the rules (leaky path, per-component limits, four Q16 coefficients,
 * 5 fractional bits, lens_model.h's four integer taps); tests/stab_ref.py restates them and every path (as bit patterns), status,
 * coefficient and output byte equals it exactly.  PARITY UNPINNED against vidstab, OpenCV's videostab and
 * warpAffine (installed nowhere this runs) and on real footage.  One similarity per frame: no rolling-shutter or perspective
 * model; causal, no look-ahead. */
#define RTMODT_STAB_OK 0       /* the path followed a valid input                                                             */
#define RTMODT_STAB_HOLD 1     /* the input was invalid and counted as the identity                                           */
#define RTMODT_STAB_CLAMPED 2  /* a valid input moved a component of the path onto its limit                                  */
#define RTMODT_STAB_RESET 3    /* reset_after consecutive HOLD calls: the path is the identity again                          */
typedef struct rtmodt_stab rtmodt_stab;
typedef struct rtmodt_stab_cfg {
    int32_t device;
    int32_t streams;            /* 1..1024 camera paths                                                                        */
    int32_t h, w;               /* the frame size (source and stabilised picture alike), 1..16384 each                         */
    int32_t leak_shift;         /* 0: no decay (an anchor on the first frame); 1..16: the path decays by k = 1 - 2^-leak_shift  */
    int32_t max_shift_px;       /* |tx|, |ty| <= this, 0..16384                                                                */
    int32_t max_rot_milli;      /* |zb| <= this / 1000, 0..500                                                                 */
    int32_t max_zoom_milli;     /* |za - 1| <= this / 1000, 0..500                                                             */
    int32_t crop_zoom_milli;    /* a fixed enlargement about the centre, 1000..8000 (1000: none), hides the correction band    */
    int32_t reset_after;        /* consecutive HOLD calls after which the path is the identity again; 0: never                 */
    uint8_t border_bgr[3];      /* what a tap off the source reads                                                             */
    uint8_t reserved;
} rtmodt_stab_cfg;
typedef struct rtmodt_stab_stream_result {
    int32_t status;             /* RTMODT_STAB_* of the stream's last call (OK before the first)                               */
    int32_t hold;               /* the run of HOLD calls so far                                                                */
    double j[4];                /* za, zb, tx, ty                                                                              */
    int64_t coef[4];            /* A, B, U, V in Q16: what the last frame was sampled with                                     */
} rtmodt_stab_stream_result;
/* Host only: device 0, 1 stream, size 0 (the caller sets it), leak_shift 6, max_shift_px 32, max_rot_milli 35, max_zoom_milli 50,
 * crop_zoom_milli 1000, reset_after 30, a black border; no default is validated on real footage.  No reference counterpart
 * (rtsp_reader.py hands cap.read()'s frame to the detector).  PARITY UNPINNED. */
void rtmodt_stab_default_cfg(rtmodt_stab_cfg *cfg);
/* Allocates 80 bytes of state per stream, every path the identity.  streams outside 1..1024, a size outside 1..16384 or a
 * parameter outside the range above is RTMODT_E_INVALID.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_stab_create(const rtmodt_stab_cfg *cfg, rtmodt_stab **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  No reference counterpart.  PARITY UNPINNED. */
void rtmodt_stab_destroy(rtmodt_stab *s);
/* One stream's path, status and HOLD run back to the fresh state, or every stream's with stream < 0.  No reference counterpart.
 * PARITY UNPINNED. */
int rtmodt_stab_reset(rtmodt_stab *s, int stream);
/* Two launches for all n frames: dst[i] (BGR24 h x w, row pitch dst_stride >= 3 w) is src[i] (same size, row pitch src_stride)
 * stabilised on the path of streams[i] (streams == NULL: stream i; a stream may occur once in a call) after that path took
 * warps[i] = float32 [a, -b, tx; b, a, ty], previous frame -> this frame in full-resolution pixels, with valid[i] != 0 (valid ==
 * NULL: all valid; warps == NULL: the identity for all).  Source and destination memory kinds are independent; bytes beyond 3 w
 * of a destination row are never written.  RTMODT_E_INVALID with nothing launched and every path as it was: a stream outside the
 * handle or named twice, a pitch below 3 w, a null frame, a destination range that overlaps a source range of the call, a valid
 * warp that is not finite or has |det| < 1e-6; more frames than streams is RTMODT_E_CAPACITY.  n == 0 is a no-op.  Synchronous.
 * No reference counterpart (cv2.warpAffine appears nowhere in it).  PARITY UNPINNED. */
int rtmodt_stab_process(rtmodt_stab *s, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                        int dst_mem_kind, const int32_t *streams, int n, const float *warps, const uint8_t *valid);
/* The same with the warps estimated by gmc from src (frame i is the estimator's stream i; valid = its status 0): the estimate is
 * queued on the estimator's stream, the step waits for it by an event, and neither warp nor status crosses the host.  mask_xyxy,
 * mask_conf, mask_n: optional host mask boxes as rtmodt_gmc_estimate_batch takes them, rows of the estimator's max_boxes, n rows.
 * Refused as above, and with RTMODT_E_INVALID / RTMODT_E_CAPACITY by the estimator's own checks: an estimator on another device,
 * one that has seen another frame size, fewer estimator streams than frames, a frame beyond its limits.  rtmodt_gmc_result
 * returns what the step consumed.  No reference counterpart (cv2.estimateAffinePartial2D appears nowhere in it).  PARITY
 * UNPINNED. */
int rtmodt_stab_process_gmc(rtmodt_stab *s, rtmodt_gmc *gmc, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst,
                            int dst_stride, int dst_mem_kind, const int32_t *streams, int n, const float *mask_xyxy, const float *mask_conf,
                            const int32_t *mask_n);
/* Every stream's status, HOLD run, path and coefficients: out[streams].  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_stab_result(rtmodt_stab *s, rtmodt_stab_stream_result *out);
/* One stream's path j[4] and HOLD run to host memory.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_stab_state(rtmodt_stab *s, int stream, double *j, int32_t *hold);
/* Replaces them, so that a path survives a restart; a path outside the handle's limits or a run outside 0..2^30 is
 * RTMODT_E_INVALID.  The stream's status becomes OK.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_stab_load_state(rtmodt_stab *s, int stream, const double *j, int32_t hold);
/* Device time (ms, HIP events around the two launches) of the last process call that launched; the estimator's part of
 * rtmodt_stab_process_gmc is rtmodt_gmc_last_ms.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_stab_last_ms(rtmodt_stab *s, float *kernel_ms);
/* Host only, float64, no device: n points xy[n][2] through the path j[4] under cfg (h, w and crop_zoom_milli are read).
 * to_source != 0: stabilised picture -> raw frame (a stabilised box drawn back on the raw frame, gmc mask boxes in raw
 * coordinates); else raw frame -> stabilised picture, the closed-form inverse.  No reference counterpart.  PARITY UNPINNED. */
int rtmodt_stab_points(const rtmodt_stab_cfg *cfg, const double *j, int to_source, const double *xy, int n, double *out_xy);
/* Host only: csrc/stab_rule.h on one stream's state without a device: j[4] and *hold are moved by warp[6] (NULL: the identity)
 * with `valid`; *status and coef[4] (each may be null) are the call's.  The parity surface of csrc/stab_rule.h.  No reference
 * counterpart.  PARITY UNPINNED. */
int rtmodt_stab_step(const rtmodt_stab_cfg *cfg, double *j, int32_t *hold, const float *warp, int valid, int32_t *status, int64_t *coef);

/* ---- camera health: is the picture still a valid picture of the scene the camera was aimed at? ------------------------------- */
/* A lens that is covered, a camera turned away, a lens out of focus, a stream that repeats its last frame, night without IR and a
 * torch into the lens: every other stage takes such a picture for the scene, and the motion detector answers one SCENE_CHANGE and
 * then learns it as background.  Per stream this module keeps a reference of the scene's coarse structure (R, unsigned 8.8 per cell
 * of the motion detector's luma grid) and of its fine detail (ref_sharp), compares every frame with it and debounces six conditions
 * into latched RAISED / CLEARED events; it gates nothing.  The reference has no counterpart (src/ingestion/rtsp_reader.py hands
 * cap.read()'s frame on; its events come from tracks only): PARITY UNPINNED throughout, against any camera's or NVR's tamper
 * detection too, and no default is validated on real footage.  PINNED, exactly, against tests/health_ref.py: every count, mask,
 * event and the whole state.  csrc/health_rule.h states the rules, csrc/health.hip's header the launches; all of it is integer
 * arithmetic.  DELIBERATE LIMITS: its own pixel pass (not shared with motion / leftobj), no colour-cast or IR-cut detection, no
 * per-region tamper map, one reference per stream (rebase on a PTZ preset change), no gating of other stages. */
#define RTMODT_HEALTH_DARK 0            /* 1000 n_dark >= dark_pm cells                                                          */
#define RTMODT_HEALTH_BRIGHT 1          /* 1000 n_bright >= bright_pm cells                                                      */
#define RTMODT_HEALTH_COVERED 2         /* the reference's structure is gone and the picture has none of its own                 */
#define RTMODT_HEALTH_MOVED 3           /* the reference's structure is gone and the picture has structure elsewhere             */
#define RTMODT_HEALTH_DEFOCUSED 4       /* the structure is in place and the fine detail is gone                                 */
#define RTMODT_HEALTH_FROZEN 5          /* at most freeze_cells cells differ from the frame before                               */
#define RTMODT_HEALTH_CONDITIONS 6      /* masks hold bit 1 << condition                                                         */
#define RTMODT_HEALTH_NO_STRUCTURE 64   /* a bit of `raw` only: fewer than min_ref_edges reference edges, the structure tests rest */
#define RTMODT_HEALTH_RAISED 1
#define RTMODT_HEALTH_CLEARED 2
#define RTMODT_HEALTH_REBASED 3         /* condition -1: the stream starts a new reference                                       */
#define RTMODT_HEALTH_MAX_EVENTS 8      /* per stream and call; csrc/health_rule.h states why the rule cannot exceed it          */
typedef struct rtmodt_health rtmodt_health;
typedef struct rtmodt_health_cfg {
    int32_t streams;            /* 1..1024                                                                                      */
    int32_t height, width;      /* the frame size, 1..32768 each; the grid at most 2^24 cells, all streams 2^28                 */
    int32_t scale;              /* 1, 2, 4 or 8 pixels per cell side                                                            */
    int32_t edge_threshold;     /* 1..255: a cell is an edge with G >= this, a weak edge with 2 G >= this                       */
    int32_t ref_shift;          /* 1..12: R += ((G << 8) - R) >> ref_shift, and the same for ref_sharp                          */
    int32_t warmup;             /* 1..255 frames that only learn                                                                */
    int32_t dark_level, dark_pm;        /* 0..255; 0..1000 per mille of the cells (0: off)                                      */
    int32_t bright_level, bright_pm;    /* likewise                                                                             */
    int32_t retain_pm;          /* 0..1000: lost = 1000 n_kept < retain_pm n_ref_edge (0: COVERED and MOVED off)                */
    int32_t cover_pm;           /* 0..1000: COVERED = lost and 1000 n_edge < cover_pm n_ref_edge (0: off, a loss is MOVED)      */
    int32_t defocus_pm;         /* 0..1000: DEFOCUSED = not lost and 1000 sharp < defocus_pm (ref_sharp >> 8) (0: off)          */
    int32_t min_ref_edges;      /* 0..2^24 reference edges the structure tests need                                             */
    int32_t hold_frames;        /* 1..65535 consecutive raw frames raise a condition                                            */
    int32_t clear_frames;       /* 1..65535 consecutive frames without it clear it                                              */
    int32_t freeze_frames;      /* 0..65535: FROZEN's hold_frames (it clears on the first changed frame); 0: off                */
    int32_t freeze_cells;       /* 0..2^24: a frame with at most this many changed cells is a repeated frame                    */
    int32_t relearn_frames;     /* 0..2^30: a structure condition active this long rebases the stream; 0: never                 */
    int32_t device;
} rtmodt_health_cfg;
typedef struct rtmodt_health_result {
    int32_t stream;
    int32_t frames_seen;        /* after the call: 0 after a relearn                                                            */
    uint32_t raw, active;       /* masks of 1 << RTMODT_HEALTH_*: this frame's raw conditions (and NO_STRUCTURE); the latched ones */
    uint32_t n_dark, n_bright, n_changed, n_edge, n_ref_edge, n_kept;
    int32_t n_events;           /* events[0 .. n_events - 1] of the stream's row are set, the rest are zero                      */
    int32_t learned;            /* 0: the reference stood still; 1: it took an averaging step; 2: it was set from this frame     */
    uint64_t luma_sum;          /* the sum of the cells' luma                                                                   */
    uint64_t sharp;             /* the sum of |y(x + 1) - y(x)| over the frame's pixels                                         */
    uint64_t ref_sharp;         /* after the call, 8 fractional bits                                                            */
} rtmodt_health_result;
typedef struct rtmodt_health_event {
    int64_t frame_id;
    int32_t condition;          /* RTMODT_HEALTH_DARK .. FROZEN; -1 for REBASED                                                 */
    int32_t kind;               /* RTMODT_HEALTH_RAISED / CLEARED / REBASED                                                     */
} rtmodt_health_event;
typedef struct rtmodt_health_state {
    uint64_t ref_sharp;
    int32_t frames_seen;        /* 0..2^30                                                                                      */
    uint32_t active;            /* mask of the latched conditions                                                               */
    uint32_t pending;           /* events an rtmodt_health_rebase owes the next call: CLEARED bits | 256 (REBASED)              */
    int32_t reserved;
    int32_t run[6], off[6];     /* per condition: raw run (inactive) or age (active); frames without the raw condition          */
} rtmodt_health_state;
/* Host only: 1 stream, height and width 0 (the caller sets them), scale 4, edge_threshold 24, ref_shift 6, warmup 25, dark 16 / 950,
 * bright 240 / 950, retain_pm 500, cover_pm 300, defocus_pm 500, min_ref_edges 16, hold_frames 25, clear_frames 25, freeze_frames
 * 50, freeze_cells 0, relearn_frames 0, device 0.  No default has been validated on real footage.  PARITY UNPINNED. */
void rtmodt_health_default_cfg(rtmodt_health_cfg *cfg);
/* Every parameter is checked before anything is allocated: one outside its range is RTMODT_E_INVALID, a grid above 2^24 cells (or
 * 2^28 over all streams) RTMODT_E_CAPACITY.  Every stream starts with frames_seen 0 and nothing active.  PARITY UNPINNED. */
int rtmodt_health_create(const rtmodt_health_cfg *cfg, rtmodt_health **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  PARITY UNPINNED. */
void rtmodt_health_destroy(rtmodt_health *m);
/* One frame for each of n distinct streams: frame i (BGR24, height x width as created, row pitch stride_bytes >= 3w, host or
 * device memory by mem_kind, read only) is judged against the reference of streams[i] (streams == NULL: stream i, and n must be
 * the stream count); frame_ids[i] is the number its events carry (NULL: 0).  results[i] and events[i][RTMODT_HEALTH_MAX_EVENTS]
 * describe it.  A frame size other than the handle's, a stream outside 0..streams - 1 or named twice, a null frame and n above the
 * stream count are RTMODT_E_INVALID with nothing launched.  Four launches, whatever the frames show; all results come back in one
 * copy.  Streams the call does not name keep their state.  Synchronous.  PARITY UNPINNED. */
int rtmodt_health_process(rtmodt_health *m, const uint8_t *const *frames, const int32_t *streams, const int64_t *frame_ids, int n, int height,
                          int width, int stride_bytes, int mem_kind, rtmodt_health_result *results, rtmodt_health_event *events);
/* One stream's state to host memory: R as uint16[gh][gw], the previous luma grid as uint8[gh][gw], and the rest.  PARITY UNPINNED. */
int rtmodt_health_read_state(rtmodt_health *m, int stream, uint16_t *r, uint8_t *prev_y, rtmodt_health_state *state);
/* Replaces one stream's state, so that a monitor survives a restart; a field outside its range (R above 255 << 8, frames_seen
 * outside 0..2^30, an unknown mask bit, a counter outside 0..2^30) is RTMODT_E_INVALID and nothing is replaced.  PARITY UNPINNED. */
int rtmodt_health_load_state(rtmodt_health *m, int stream, const uint16_t *r, const uint8_t *prev_y, const rtmodt_health_state *state);
/* The operator's word that the camera now shows what it should: the stream's active structure conditions are cleared, frames_seen
 * becomes 0 (the next frame starts a new reference), and the CLEARED and REBASED events are reported by the stream's next process
 * call, ahead of that frame's own.  PARITY UNPINNED. */
int rtmodt_health_rebase(rtmodt_health *m, int stream);
/* Forgets one stream's reference, previous grid, counters and active conditions (no event), or every stream's with stream == -1.
 * PARITY UNPINNED. */
int rtmodt_health_reset(rtmodt_health *m, int stream);
/* Device time (ms, HIP events around the memset and the four launches) of the last process call that launched.  PARITY UNPINNED. */
int rtmodt_health_last_ms(rtmodt_health *m, float *kernel_ms);
/* Host only, no device needed: csrc/health_rule.h's decision, debounce and relearn on one row of counts (row's n_*, luma_sum and
 * sharp are read; frames_seen, raw, active, n_events, learned and ref_sharp are written) and one state of a stream with `cells`
 * cells; events[RTMODT_HEALTH_MAX_EVENTS] carry frame_id.  Only the rule fields of cfg are read (edge_threshold .. relearn_frames).
 * A count above cells or a state outside its ranges is RTMODT_E_INVALID.  The parity surface of csrc/health_rule.h.  PARITY
 * UNPINNED. */
int rtmodt_health_decide(const rtmodt_health_cfg *cfg, int64_t cells, int64_t frame_id, rtmodt_health_result *row, rtmodt_health_state *state,
                         rtmodt_health_event *events);

/* ---- frame enhancement: low-light and low-contrast frames lifted before every stage that reads pixels ------------------------- */
/* At night without IR, at dusk, in backlight or in fog the scene occupies twenty or thirty grey levels out of 256; the motion
 * detector's fixed thresholds and the detector see a flat picture.  This module is contrast-limited adaptive histogram equalisation
 * (CLAHE) of the luma: per-tile histograms, clipped, integrated into tone curves, interpolated between tile centres -- with the
 * tone curves held per stream on the device and moved by an integer EMA, because a per-frame CLAHE flickers on video.  The reference
 * has no counterpart (src/ingestion/rtsp_reader.py hands cap.read()'s frame on): PARITY UNPINNED throughout, against
 * cv2.createCLAHE too (its tiles are padded by reflection, its interpolation is float), and no default is validated on real footage.
 * PINNED, exactly, against tests/enhance_ref.py: every output byte, histogram, state value and result field.  csrc/enhance_rule.h
 * states the rules, csrc/enhance.hip's header the launches; all of it is integer arithmetic.  DELIBERATE LIMITS: luma only, no
 * denoising (rtmodt_denoise, run before this), no gamma or white balance, one tile grid per handle, `auto` follows the frame mean without hysteresis. */
#define RTMODT_ENHANCE_SHIFT 0          /* each channel becomes clamp(c + (Y2 - Y)): chroma untouched                           */
#define RTMODT_ENHANCE_GAIN 1           /* each channel becomes min(255, (c * Y2 + Y / 2) / Y): hue and saturation kept         */
#define RTMODT_ENHANCE_MAX_TILES 16
typedef struct rtmodt_enhance rtmodt_enhance;
typedef struct rtmodt_enhance_cfg {
    int32_t streams;            /* 1..1024                                                                                      */
    int32_t height, width;      /* the frame size, 1..16384 each                                                                */
    int32_t tiles_y, tiles_x;   /* 1..16 each and no more than the pixels of their axis                                         */
    int32_t clip_q8;            /* 0..65536: the clip limit in 1 / 256 (OpenCV's clipLimit 2.0 is 512); 0: no clipping          */
    int32_t strength;           /* 0..256: how much of the equalised luma is taken                                              */
    int32_t smooth_shift;       /* 0..7: the tone curves move by 1 / 2^smooth_shift per frame; 0 follows the frame at once      */
    int32_t auto_lo, auto_hi;   /* 0 <= auto_lo <= auto_hi <= 255; auto_hi > auto_lo: full strength at a mean luma of auto_lo
                                   and below, none at auto_hi and above                                                         */
    int32_t colour;             /* RTMODT_ENHANCE_SHIFT or RTMODT_ENHANCE_GAIN                                                  */
    int32_t device;
} rtmodt_enhance_cfg;
typedef struct rtmodt_enhance_result {
    int32_t stream;
    int32_t frames_seen;        /* after the call                                                                               */
    uint32_t eff;               /* the strength this frame was enhanced with, 0..256                                            */
    uint32_t clipped;           /* the pixels above the clip limit, summed over the stream's tiles                              */
    uint64_t luma_sum;          /* the sum of the frame's luma                                                                  */
} rtmodt_enhance_result;
/* Host only: 1 stream, height and width 0 (the caller sets them), 8 x 8 tiles, clip_q8 512, strength 256, smooth_shift 2, auto off
 * (0, 0), SHIFT, device 0.  No default has been validated on real footage.  PARITY UNPINNED. */
void rtmodt_enhance_default_cfg(rtmodt_enhance_cfg *cfg);
/* Every parameter is checked before anything is allocated: one outside its range is RTMODT_E_INVALID and the message names it.
 * Every stream starts with frames_seen 0.  PARITY UNPINNED. */
int rtmodt_enhance_create(const rtmodt_enhance_cfg *cfg, rtmodt_enhance **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  PARITY UNPINNED. */
void rtmodt_enhance_destroy(rtmodt_enhance *e);
/* One frame for each of n distinct streams: src[i] (BGR24, height x width as created, row pitch src_stride >= 3w, host or device
 * memory by src_mem_kind) is enhanced with the tone curves of streams[i] (streams == NULL: stream i, and n must be the stream
 * count) into dst[i] (dst_stride, dst_mem_kind; any mix of host and device).  dst[i] may BE src[i] at the same pitch (in place:
 * the step is pointwise); any other meeting of a destination range with a source range of the call, a frame size other than the
 * handle's, a stream outside 0..streams - 1 or named twice, a null frame and n above the stream count are RTMODT_E_INVALID with
 * nothing launched.  Padding bytes of the rows are not touched.  A memset and three launches, whatever the frames show; results
 * (NULL: none are copied) come back in one copy.  Streams the call does not name keep their state.  Synchronous.  PARITY UNPINNED. */
int rtmodt_enhance_process(rtmodt_enhance *e, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                           int dst_mem_kind, const int32_t *streams, int n, int height, int width, rtmodt_enhance_result *results);
/* One stream's state to host memory: s as uint16[tiles_y][tiles_x][256] (8.8 fixed point) and frames_seen.  PARITY UNPINNED. */
int rtmodt_enhance_read_state(rtmodt_enhance *e, int stream, uint16_t *s, int32_t *frames_seen);
/* Replaces one stream's state (n_values must be tiles_y * tiles_x * 256), so that an enhancer survives a restart; another size, a
 * value above 255 << 8 or frames_seen outside 0..2^30 is RTMODT_E_INVALID and nothing is replaced.  PARITY UNPINNED. */
int rtmodt_enhance_load_state(rtmodt_enhance *e, int stream, const uint16_t *s, int64_t n_values, int32_t frames_seen);
/* Forgets one stream's tone curves (its next frame sets them), or every stream's with stream == -1.  PARITY UNPINNED. */
int rtmodt_enhance_reset(rtmodt_enhance *e, int stream);
/* The histograms the last process call built for `stream`, uint32[tiles_y][tiles_x][256]; RTMODT_E_INVALID when that call did not
 * name the stream.  For tests and tuning.  PARITY UNPINNED. */
int rtmodt_enhance_histograms(rtmodt_enhance *e, int stream, uint32_t *hist);
/* Device time (ms, HIP events around the memset and the three launches) of the last process call that launched.  PARITY UNPINNED. */
int rtmodt_enhance_last_ms(rtmodt_enhance *e, float *kernel_ms);
/* Host only, no device needed: csrc/enhance_rule.h's tone curve of one tile from its histogram hist[256], whose sum must be the
 * area n (1..2^28), under clip_q8 -> curve[256] and the excess.  The parity surface of the curve rule.  PARITY UNPINNED. */
int rtmodt_enhance_curve(const uint32_t *hist, int64_t n, int32_t clip_q8, uint32_t *curve, uint32_t *excess);
/* Host only, no device needed: where each of px pixels (1..16384) sits among `tiles` tiles (1..16, at most px) along one axis
 * -> k[px] and f[px] (0..256, in 1 / 256 of the way from the centre of tile k to that of tile min(k + 1, tiles - 1)), and
 * bounds[tiles + 1], the first pixel of every tile and px.  The parity surface of the axis rule.  PARITY UNPINNED. */
int rtmodt_enhance_axis(int32_t px, int32_t tiles, int32_t *k, int32_t *f, int32_t *bounds);

/* ---- frame noise reduction: motion-adaptive temporal and spatial filtering ("3DNR") before the enhancer ------------------------- */
/* High-gain sensor noise is on every pixel of every night frame; the enhancer multiplies it, the JPEG encoder spends bytes on it.
 * Per stream the module keeps acc, a running mean of every channel of every pixel in 8.8 fixed point.  A pixel whose 3 x 3
 * neighbourhood did not change in the sum of its luma differences (noise cancels in the sum, a real change does not) moves towards
 * the frame by 1 / 2^temporal_shift; a pixel that changed takes the frame at once, smoothed by a sigma filter over the neighbours
 * of similar luma; between motion_lo and motion_hi the two blend.  It belongs directly after stabilisation (a temporal filter
 * needs registered frames) and directly before rtmodt_enhance.  The reference has no counterpart (src/ingestion/rtsp_reader.py
 * hands cap.read()'s frame on): PARITY UNPINNED throughout, against any camera's 3DNR, cv2.fastNlMeansDenoising and ffmpeg's
 * hqdn3d too, and no default is validated on real footage.  PINNED, exactly, against tests/denoise_ref.py: every output byte,
 * state value and result field.  csrc/denoise_rule.h states the rules, csrc/denoise.hip's header the launches; all of it is
 * integer arithmetic.  DELIBERATE LIMITS: no motion compensation (a PTZ move is motion everywhere: the frame passes), thresholds
 * do not adapt to the measured noise (it is reported, the choice is the caller's), BGR24 only, and no in-place form. */
typedef struct rtmodt_denoise rtmodt_denoise;
typedef struct rtmodt_denoise_cfg {
    int32_t streams;            /* 1..1024                                                                                      */
    int32_t height, width;      /* the frame size, 1..16384 each                                                                */
    int32_t motion_lo, motion_hi; /* 0 <= motion_lo < motion_hi <= 2295, in units of the 3 x 3 luma sum: at and below motion_lo
                                   a pixel is static, at and above motion_hi it is moving                                       */
    int32_t temporal_shift;     /* 0..6: a static pixel moves by 1 / 2^temporal_shift per frame; 0: no temporal filtering        */
    int32_t spatial;            /* 0..256: how much of the sigma filter a moving pixel takes; 0: none                           */
    int32_t spatial_thr;        /* 0..255: a neighbour counts in the sigma filter when its luma is at most this far from the pixel's */
    int32_t device;
} rtmodt_denoise_cfg;
typedef struct rtmodt_denoise_result {
    int32_t stream;
    int32_t frames_seen;        /* after the call                                                                               */
    uint32_t n_static;          /* the pixels with a == 0                                                                       */
    uint32_t n_moving;          /* the pixels with a == 256                                                                     */
    uint64_t absdiff_static;    /* the sum of |Y(x) - Y(prev)| over the static pixels: 256 * absdiff_static / n_static is the
                                   noise figure to tune the thresholds with                                                     */
} rtmodt_denoise_result;
/* Host only: 1 stream, height and width 0 (the caller sets them), motion_lo 18, motion_hi 54, temporal_shift 3, spatial 256,
 * spatial_thr 6, device 0.  No default has been validated on real footage.  Replaces nothing (rtsp_reader.py).  PARITY UNPINNED. */
void rtmodt_denoise_default_cfg(rtmodt_denoise_cfg *cfg);
/* Every parameter is checked before anything is allocated: one outside its range (motion_hi <= motion_lo too) is RTMODT_E_INVALID
 * and the message names it; more than 2^30 pixels over all streams is RTMODT_E_CAPACITY.  Every stream starts with frames_seen 0.
 * Replaces nothing (rtsp_reader.py).  PARITY UNPINNED. */
int rtmodt_denoise_create(const rtmodt_denoise_cfg *cfg, rtmodt_denoise **out);
/* Waits for the handle's own stream, frees its buffers; null is allowed.  Replaces nothing (rtsp_reader.py).  PARITY UNPINNED. */
void rtmodt_denoise_destroy(rtmodt_denoise *d);
/* One frame for each of n distinct streams: src[i] (BGR24, height x width as created, row pitch src_stride >= 3w, host or device
 * memory by src_mem_kind) is filtered with the state of streams[i] (streams == NULL: stream i, and n must be the stream count)
 * into dst[i] (dst_stride, dst_mem_kind; any mix of host and device).  An output pixel depends on its neighbours' inputs, so
 * there is NO in-place form: any meeting of a destination range with a source range of the call, dst[i] == src[i] included, a
 * frame size other than the handle's, a stream outside 0..streams - 1 or named twice, a null frame and n above the stream count
 * are RTMODT_E_INVALID with nothing launched.  Padding bytes of the rows are not touched.  A memset and two launches, whatever the
 * frames show; results (NULL: none are copied) come back in one copy.  Streams the call does not name keep their state.
 * Synchronous.  Replaces the hand-over of cap.read()'s frame (rtsp_reader.py).  PARITY UNPINNED. */
int rtmodt_denoise_process(rtmodt_denoise *d, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                           int dst_mem_kind, const int32_t *streams, int n, int height, int width, rtmodt_denoise_result *results);
/* One stream's state to host memory: acc as uint16[height][width][3] (8.8 fixed point) and frames_seen.  Replaces nothing
 * (rtsp_reader.py).  PARITY UNPINNED. */
int rtmodt_denoise_read_state(rtmodt_denoise *d, int stream, uint16_t *acc, int32_t *frames_seen);
/* Replaces one stream's state (n_values must be height * width * 3), so that a denoiser survives a restart; another size, a value
 * above 255 << 8 or frames_seen outside 0..2^30 is RTMODT_E_INVALID and nothing is replaced.  Replaces nothing (rtsp_reader.py).
 * PARITY UNPINNED. */
int rtmodt_denoise_load_state(rtmodt_denoise *d, int stream, const uint16_t *acc, int64_t n_values, int32_t frames_seen);
/* Forgets one stream's state (its next frame passes and sets it), or every stream's with stream == -1.  Replaces nothing
 * (rtsp_reader.py).  PARITY UNPINNED. */
int rtmodt_denoise_reset(rtmodt_denoise *d, int stream);
/* Device time (ms, HIP events around the memset and the two launches) of the last process call that launched.  Replaces nothing
 * (rtsp_reader.py).  PARITY UNPINNED. */
int rtmodt_denoise_last_ms(rtmodt_denoise *d, float *kernel_ms);
/* Host only, no device needed: csrc/denoise_rule.h's rule for one pixel from its two 3 x 3 neighbourhoods, row by row, the
 * caller having clamped the coordinates: cur[9][3] the frame's BGR bytes and acc[9][3] the state (each at most 255 << 8); bit q
 * of `inside` says that neighbour q lies inside the frame (bit 4, the centre, must be set).  Only the rule fields of cfg are read
 * (motion_lo .. spatial_thr).  -> out[3], the centre's new acc_out[3], and (each may be NULL) a and D.  The parity surface of
 * csrc/denoise_rule.h.  Replaces nothing (rtsp_reader.py).  PARITY UNPINNED. */
int rtmodt_denoise_pixel(const rtmodt_denoise_cfg *cfg, const uint8_t *cur, const uint16_t *acc, uint32_t inside, int32_t frames_seen, uint8_t *out,
                         uint16_t *acc_out, int32_t *a, int32_t *d);

/* ---- colour attributes: the colour names of every track, kept on the device ------------------------------------------------------ */
/* What colour a track IS, for attribute search ("red top, dark trousers") and the alert record: the reference's Track and alert
 * carry bbox_xyxy, a class and a frame_id.  Per track and call the module samples the inside of the box on a bounded grid, names
 * every sample with one of 12 colour names by an all-integer rule, adds the counts of the UPPER and the LOWER part to the track's
 * row of a per-stream ledger on the device, and answers the dominant and the second name of each part and of the WHOLE with
 * their shares per mille, for live and for retired tracks.  csrc/colour_rule.h states the per-pixel and per-box rules, the header
 * of csrc/colour.hip the ledger rules; tests/colour_ref.py restates both and the kernels equal it exactly.  No reference
 * counterpart.  PARITY UNPINNED: the names agree with no human colour naming study and with no product's by any measurement; every
 * default is validated on no real footage; there is no white balance, and night or IR frames honestly answer grey everywhere.
 * Two launches per call for all streams whatever the tracks do.  Every call carries a frame_id per stream, strictly increasing
 * per stream (else RTMODT_E_INVALID, nothing changes).  Frames are BGR24, h x w at a row pitch of stride_bytes >= 3 w, in host or
 * device memory, and are only read.  An entry is SAMPLED (takes a row) when its class passes the filter, its coordinates are
 * finite and x1 >= x0, y1 >= y0 after truncation; its sampled rectangle may still be empty (no samples, no error). */
#define RTMODT_COLOUR_NAMES 12
#define RTMODT_COLOUR_UPPER 0
#define RTMODT_COLOUR_LOWER 1
#define RTMODT_COLOUR_WHOLE 2
#define RTMODT_COLOUR_F_NEW 1             /* the row was created by this call */
#define RTMODT_COLOUR_F_MANY_OCCLUDERS 2  /* more than 8 occluders met the sampled rectangle in the row's last call; the extras were ignored */
#define RTMODT_COLOUR_F_THIN 4            /* the row's last call took fewer than min_samples samples: its counts were not added */
typedef struct rtmodt_colour rtmodt_colour;
typedef struct rtmodt_colour_cfg {
    /* the name of a pixel (csrc/colour_rule.h, step 1) */
    int32_t black_max;          /* 0..256: max(b, g, r) below this is black */
    int32_t chroma_min;         /* 0..256: max - min below this is achromatic */
    int32_t sat_split;          /* 0..256: sat_hi_pm applies from this max on, sat_lo_pm below */
    int32_t sat_hi_pm, sat_lo_pm; /* 0..1000: (max - min) * 1000 <= sat * max is achromatic */
    int32_t y_black, y_white;   /* 0 <= y_black <= y_white <= 256: achromatic luma below y_black is black, from y_white on white, else grey */
    int32_t hue[8];             /* ascending, 0..1536: the hue bounds red|orange|yellow|green|cyan|blue|purple|pink|red */
    int32_t pink_mx, red_brown_mx, orange_brown_mx, yellow_brown_mx;   /* 0..256: the max thresholds of the pink and brown cases */
    /* the sampled rectangle, the grid, the occluders (steps 2..4) */
    int32_t inset_x_pm;         /* 0..499: the columns lose this many thousandths of the box width on each side */
    int32_t top_pm, split_pm, bottom_pm;   /* 0 <= top < split < bottom <= 1000: thousandths of the box height */
    int32_t max_side;           /* 1..256: at most this many samples along each axis */
    int32_t skip_occluded;      /* 0 / 1: samples inside a nearer box of the list are skipped */
    /* the ledger (step 5) */
    int32_t min_samples;        /* 0..65536: a frame's counts are added only with at least this many samples over both parts */
    int32_t retire_after;       /* >= 0: a row whose track was last sampled more than this many frame ids ago is retired */
    int32_t device;
    int32_t n_classes;          /* with `classes`: only these class ids are sampled (at most 256); classes == NULL: all */
    const int32_t *classes;
} rtmodt_colour_cfg;
/* The label of one part: name and second are indices into the name order black, grey, white, red, orange, yellow, green, cyan,
 * blue, purple, pink, brown (-1: none); shares in thousandths of `samples`, the part's total count. */
typedef struct rtmodt_colour_label {
    int32_t name, share_pm, second, second_pm, samples;
} rtmodt_colour_label;
/* One row: of `updated` (a member of this call, in list order), of `retired` (ascending track id) or of the ledger (_state, _load).
 * `track`: index into the caller's list, or into the tracker's list; -1 in retired and ledger rows.  frame_samples: the samples
 * this call took (0 in retired and ledger rows).  label[UPPER, LOWER, WHOLE] is read off hist; _load ignores it. */
typedef struct rtmodt_colour_row {
    int64_t track_id;
    int64_t first_frame, last_frame;
    uint32_t hist[2][RTMODT_COLOUR_NAMES];
    int32_t cls, frames_used, flags, track;
    int32_t frame_samples, reserved[2];
    rtmodt_colour_label label[3];
} rtmodt_colour_row;
/* What one call hands back; the struct pointer and every member may be null.  With none given nothing crosses to the host and the
 * call does not wait for the device; otherwise the streams' result blocks come back in one copy.  One-stream calls: updated
 * [max_tracks], retired [2 max_tracks], counts [1]; all-stream calls: [n_streams][...] and counts [n_streams]. */
typedef struct rtmodt_colour_out {
    rtmodt_colour_row *updated;
    int32_t *n_updated;
    rtmodt_colour_row *retired;
    int32_t *n_retired;
} rtmodt_colour_out;
/* The plan of one box (the parity surface of csrc/colour_rule.h): rectangles are inclusive x0, y0, x1, y1. */
typedef struct rtmodt_colour_plan_out {
    int32_t sampled;            /* 0: the box takes no row, nothing else is written */
    int32_t raw[4];             /* truncated corners, not clipped */
    int32_t box[4];             /* raw clipped to the frame (x1 < x0 or y1 < y0: empty) */
    int32_t rect[4];            /* the sampled rectangle, clipped (empty likewise) */
    int32_t split_row;          /* rows below it are UPPER */
    int32_t sx, sy, nx, ny;     /* strides and sample counts (nx = ny = 0: no samples) */
} rtmodt_colour_plan_out;
/* black_max 48, chroma_min 20, sat_split 96, sat 180 / 400, y_black 64, y_white 176, hue 64 192 299 725 853 1109 1344 1472,
 * pink_mx 192, red_brown_mx 96, orange_brown_mx 176, yellow_brown_mx 128, inset_x_pm 200, top / split / bottom 150 / 500 / 900,
 * max_side 48, skip_occluded 1, min_samples 16, retire_after 30, device 0, every class. */
void rtmodt_colour_default_cfg(rtmodt_colour_cfg *cfg);
/* n_streams independent ledgers; max_tracks <= 4096.  A ledger holds 2 x max_tracks rows sorted by track id.  Per call and stream:
 *   retire   a row with frame_id - last_frame > retire_after leaves the ledger and is reported in `retired` with its final label
 *            (a track of the same id sampled in this call starts a new row);
 *   member   a sampled entry keeps or takes its row: last_frame = frame_id, cls = the entry's, flags = this call's; its frame
 *            counts are added (frames_used gains one) when they hold min_samples samples, and a part past 2^24 is halved.
 * Occluders are taken in LIST order: ascending track id for a caller's list, the tracker's own order for a tracker.
 * Capacity, as the snapshot gallery's: the call that needs more than 2 x max_tracks rows returns RTMODT_E_CAPACITY, the idle rows
 * are dropped and the stream stays in error for good (every later call that asks for output, and _state, returns
 * RTMODT_E_CAPACITY) until rtmodt_colour_reset.  A call made without outputs cannot report it. */
int rtmodt_colour_create(const rtmodt_colour_cfg *cfg, int n_streams, int max_tracks, rtmodt_colour **out);
/* Waits for the handle's queued work, frees everything; null is allowed. */
void rtmodt_colour_destroy(rtmodt_colour *h);
/* One stream, a caller-supplied track list (any order, unique ids, at most max_tracks) and its frame. */
int rtmodt_colour_process(rtmodt_colour *h, int stream, const int64_t *track_ids, const float *xyxy, const int32_t *cls, int n,
                          const uint8_t *frame, int fh, int fw, int stride_bytes, int mem_kind, int64_t frame_id, const rtmodt_colour_out *out);
/* Every stream in one call: track_ids / cls [n_streams][stride], xyxy [n_streams][stride][4], n [n_streams], frames [n_streams]
 * of one geometry, frame_id [n_streams]. */
int rtmodt_colour_process_batch(rtmodt_colour *h, const int64_t *track_ids, const float *xyxy, const int32_t *cls, const int32_t *n, int stride,
                                const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind, const int64_t *frame_id,
                                const rtmodt_colour_out *out);
/* Every stream of a ByteTrack handle, straight on its device-resident state and on the HIP stream its last update ran on:
 * exactly the tracks rtmodt_snapshot_process_tracker passes.  frames / frame_id [n_streams of the tracker]. */
int rtmodt_colour_process_tracker(rtmodt_colour *h, rtmodt_tracker *trk, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                  const int64_t *frame_id, int report_tsu, const rtmodt_colour_out *out);
/* The same on a DeepSORT handle. */
int rtmodt_colour_process_deepsort(rtmodt_colour *h, rtmodt_deepsort *ds, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                   const int64_t *frame_id, int report_tsu, const rtmodt_colour_out *out);
/* The same on an OC-SORT handle. */
int rtmodt_colour_process_ocsort(rtmodt_colour *h, rtmodt_ocsort *oc, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                 const int64_t *frame_id, const rtmodt_colour_out *out);
/* The same on a BoT-SORT handle. */
int rtmodt_colour_process_botsort(rtmodt_colour *h, rtmodt_botsort *bot, const uint8_t *const *frames, int fh, int fw, int stride_bytes, int mem_kind,
                                  const int64_t *frame_id, const rtmodt_colour_out *out);
/* The whole ledger of one stream, rows in ascending track id with their labels (the parity surface of tests/colour_ref.py); rows
 * [2 max_tracks] may be null.  A stream in error fills them all the same and returns RTMODT_E_CAPACITY. */
int rtmodt_colour_state(rtmodt_colour *h, int stream, rtmodt_colour_row *rows, int32_t *n);
/* Replaces one stream's ledger by n rows in strictly ascending track id (at most 2 max_tracks, first_frame <= last_frame,
 * frames_used >= 0; labels are ignored), clears its error, and takes the largest last_frame as the stream's last frame_id: a
 * handle continues where _state left another.  Anything else is RTMODT_E_INVALID and nothing is replaced. */
int rtmodt_colour_load(rtmodt_colour *h, int stream, const rtmodt_colour_row *rows, int n);
/* Empties one stream's ledger, forgets its last frame_id and its error. */
int rtmodt_colour_reset(rtmodt_colour *h, int stream);
/* Device time (ms, HIP events around the two launches) of the last _process* call. */
int rtmodt_colour_last_ms(rtmodt_colour *h, float *kernel_ms);
/* Host only, no device needed: the name (0..11) of the pixel (b, g, r), each 0..255, under cfg's thresholds; a negative error
 * code when cfg or a channel is out of range. */
int rtmodt_colour_name(int b, int g, int r, const rtmodt_colour_cfg *cfg);
/* Host only, no device needed: the sampled rectangle, the split row and the grid of one box xyxy[4] of any class in an h x w frame. */
int rtmodt_colour_plan(const rtmodt_colour_cfg *cfg, const float *xyxy, int h, int w, rtmodt_colour_plan_out *out);

#ifdef __cplusplus
}
#endif
#endif /* RTMODT_H */
