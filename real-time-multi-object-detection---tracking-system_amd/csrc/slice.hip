// slice.hip -- sliced inference (the SAHI scheme) around the detector: cut every frame into overlapping tiles at native
// resolution plus one letterboxed overview, run the detector on that image batch, and merge the per-image detections back in
// frame coordinates -- the cut (slice_gather) and the merge (slice_merge) on the GPU, the conv path untouched.
//
// Why: the reference feeds 1920 x 1080 frames to a 640 x 640 detector (its config/default.yaml:24-26, 34), so every
// object shrinks three times before the network sees it; its design document lists "Missed small objects" (B.4's failure table)
// and marks conf 0.40 "Misses small objects" (B.3) with no cure that keeps the model.  PARITY UNPINNED: the `sahi` package is
// installed nowhere this runs; tests/slice_ref.py restates the rules below and the kernels equal it bit for bit.
//
// slice_gather: ONE launch; image f * I + j of the batch is tile j of frame f (a byte copy of the te_w x te_h window at
//   (x_j, y_j)) or, for j == T, the whole frame letterboxed into te_w x te_h by the detector's own letterbox (letterbox.h's
//   geometry and tables, letterbox_dev.h's pixel: cv2.resize INTER_LINEAR fixed point, 114 padding).  Images are BGR24 with pitch 3 * te_w.  A window starts 3 * x_j bytes into a
//   row, so nothing is known about its alignment: a row is copied as a byte head up to the first 16-byte boundary of the
//   DESTINATION, 16-byte stores fed by one 16-byte load, four 4-byte loads or sixteen byte loads -- whichever the source
//   address of that row allows -- and a byte tail.  No byte outside the window is read, none outside the row is written.
// slice_merge: one workgroup per frame on the detector's post-processing stream.  Candidates = the detections of the frame's I
//   images, mapped to frame coordinates (tile: x + float(x_j), clip; overview: subtract pad, divide by gain, clip -- float32),
//   sorted by (conf descending as float32, image ascending, slot ascending) with a bitonic network in LDS, then walked in that
//   order: a live candidate becomes a keeper and takes every later live candidate that matches its ORIGINAL box out -- dropped
//   (NMS) or absorbed into the keeper's min / max union box (NMM, SAHI's greedy non-maximum merging).  Match: float32, every
//   operation rounded on its own (this file is built with FMA contraction off and IEEE division),
//     iw = min(ax2, bx2) - max(ax1, bx1), ih likewise, both clamped at 0; inter = iw * ih; area = (x2 - x1) * (y2 - y1);
//     IoU = inter / ((aa + ab) - inter), IoS = inter / min(aa, ab); denominator > 0, metric > match_thresh (strict), and the
//     classes equal unless agnostic.
//   The first max_out keepers leave as box / conf / cls / n_merged / n, device-resident behind a DetOutputs (kernels.h).
//   Capacities: 64 tiles per frame, I x max_det <= 8192 candidates per frame (the LDS sort), max_frames x I <= 64 (a detector batch).
#include <vector>

#include "frame_stage.h"
#include "handle_host.h"
#include "letterbox_dev.h"
#include "slice_grid.h"

using namespace rtmodt;

namespace rtmodt {

struct SliceGeom { int W, H, te_w, te_h, T, I; int tx[SLICE_MAX_TILES], ty[SLICE_MAX_TILES]; };

// ---------------------------------------------------------------------------------------------------------------- gather
struct SliceGatherArgs {
    FramePtrs frames; int pitch;
    SliceGeom g;
    LetterboxGeom lb; ResizeTables t;        // the overview
    uint8_t *out;                            // [n * I][te_h][3 * te_w]
};

__global__ __launch_bounds__(256) void slice_gather_kernel(SliceGatherArgs a) {
    const SliceGeom &g = a.g;
    const int img = blockIdx.y, f = img / g.I, j = img % g.I;
    const size_t img_bytes = (size_t)3 * g.te_w * g.te_h;
    uint8_t *dimg = a.out + (size_t)img * img_bytes;
    const uint8_t *src = a.frames.p[f];
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (j == g.T) {
        // the overview: the image is one run of te_w * te_h pixels (pitch == 3 * te_w); four pixels = 12 bytes per thread and trip
        const long npx = (long)g.te_w * g.te_h;
        const bool aligned = ((uintptr_t)dimg & 3) == 0;
        for (long q = first; q * 4 < npx; q += stride) {
            const long p0 = q * 4;
            uint8_t b[12];
            const int cnt = (int)min(4L, npx - p0);
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    int c0, c1, c2;
                    letterbox_pixel((int)((p0 + k) % g.te_w), (int)((p0 + k) / g.te_w), a.lb, a.t, Bgr24Source{src, a.pitch}, c0, c1, c2);
                    b[3 * k] = (uint8_t)c0; b[3 * k + 1] = (uint8_t)c1; b[3 * k + 2] = (uint8_t)c2;
                }
            uint8_t *d = dimg + p0 * 3;
            if (aligned && cnt == 4) {
                uint32_t *d4 = (uint32_t *)d;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    d4[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
            } else {
                for (int k = 0; k < 3 * cnt; ++k) d[k] = b[k];
            }
        }
        return;
    }
    // a tile: rows of RB bytes; per row one item for the byte head, one per 16-byte chunk, one for the byte tail
    const int RB = 3 * g.te_w, CP = RB / 16 + 2;
    const long items = (long)g.te_h * CP;
    const uint8_t *win = src + (long)g.ty[j] * a.pitch + (long)3 * g.tx[j];
    for (long it = first; it < items; it += stride) {
        const int r = (int)(it / CP), c = (int)(it % CP);
        uint8_t *d = dimg + (size_t)r * RB;
        const uint8_t *s = win + (long)r * a.pitch;
        const int head = min((int)((16 - ((uintptr_t)d & 15)) & 15), RB);
        const int nb = (RB - head) >> 4;
        if (c == 0) {
            for (int k = 0; k < head; ++k) d[k] = s[k];
        } else if (c == CP - 1) {
            for (int k = head + 16 * nb; k < RB; ++k) d[k] = s[k];
        } else if (c - 1 < nb) {
            const int off = head + 16 * (c - 1);
            const uint8_t *sp = s + off;
            uint4 v;
            if (((uintptr_t)sp & 15) == 0) {
                v = *(const uint4 *)sp;
            } else if (((uintptr_t)sp & 3) == 0) {
                const uint32_t *s4 = (const uint32_t *)sp;
                v = make_uint4(s4[0], s4[1], s4[2], s4[3]);
            } else {
                uint32_t w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    w[q] = (uint32_t)sp[4 * q] | ((uint32_t)sp[4 * q + 1] << 8) | ((uint32_t)sp[4 * q + 2] << 16) | ((uint32_t)sp[4 * q + 3] << 24);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4 *)(d + off) = v;
        }
    }
}

static int launch_slice_gather(const SliceGatherArgs &a, int n, hipStream_t s) {
    const long groups = ((long)a.g.te_w * a.g.te_h + 3) / 4;
    const unsigned gx = (unsigned)std::max(1L, std::min((groups + 255) / 256, 1024L));
    hipLaunchKernelGGL(slice_gather_kernel, dim3(gx, (unsigned)(n * a.g.I)), dim3(256), 0, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- merge
constexpr int SM_THREADS = 1024, SM_WAVES = SM_THREADS / 64;

struct SliceMergeArgs {
    SliceGeom g;
    float gain, pad_x, pad_y;                // the overview's way back (scale_boxes)
    int nms, iou, agnostic, max_out;         // nms: 1 = drop, 0 = absorb (NMM); iou: 1 = IoU, 0 = IoS
    float thresh;
    const float4 *box; const float *conf; const int32_t *cls; const int32_t *n; int stride;      // per image: [frames * I][stride], counts [frames * I]
    float4 *sbox; int32_t *scls; int cap;    // scratch [frames][cap], cap = I * stride <= SLICE_MAX_CAND: the candidates in walk order
    float4 *out_box; float *out_conf; int32_t *out_cls, *out_nm, *out_n;                        // [frames][max_out], out_n [frames]
};

__device__ __forceinline__ bool slice_match(const float4 a, float aa, const float4 b, int iou, float thr) {
    float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x), ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    iw = iw < 0.0f ? 0.0f : iw; ih = ih < 0.0f ? 0.0f : ih;
    const float inter = iw * ih;
    const float ab = (b.z - b.x) * (b.w - b.y);
    const float den = iou ? (aa + ab) - inter : fminf(aa, ab);
    return den > 0.0f && inter / den > thr;
}

__device__ __forceinline__ float clipf(float v, float hi) { return fminf(fmaxf(v, 0.0f), hi); }

constexpr int SM_LDS_BOX = 2048;             // up to this many candidates per frame the walk reads boxes and classes from LDS (40 KiB), beyond it from the scratch

// LDSBOX: the candidates in walk order live in LDS (cap <= SM_LDS_BOX) instead of the global scratch -- the walk's two dependent
// loads per keeper (its own box, then the boxes it is compared with) then cost LDS latency, not L2 latency
template <bool LDSBOX>
__global__ __launch_bounds__(SM_THREADS) void slice_merge_kernel(SliceMergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const int I = a.g.I, T = a.g.T, stride = a.stride;
    int P = 1;
    while (P < a.cap) P <<= 1;
    unsigned long long *keys = (unsigned long long *)smem;           // [P]
    unsigned char *state = smem + (((size_t)P * 8 + 15) & ~(size_t)15);   // [cap]: 0 live, 1 taken
    const size_t cap16 = ((size_t)a.cap + 15) & ~(size_t)15;
    __shared__ int s_off[SLICE_MAX_IMAGES + 1], s_tx[SLICE_MAX_IMAGES], s_ty[SLICE_MAX_IMAGES];
    __shared__ float s_red[2][SM_WAVES][4];
    __shared__ int s_cnt[2][SM_WAVES];

    if (tid == 0) {
        int o = 0;
        for (int j = 0; j < I; ++j) {
            s_off[j] = o;
            o += min(max(a.n[(size_t)f * I + j], 0), stride);
        }
        s_off[I] = o;
    }
    if (tid < T) { s_tx[tid] = a.g.tx[tid]; s_ty[tid] = a.g.ty[tid]; }
    __syncthreads();
    const int N = s_off[I];
    float4 *sbox = LDSBOX ? (float4 *)(state + cap16) : a.sbox + (size_t)f * a.cap;                  // [cap]
    int32_t *scls = LDSBOX ? (int32_t *)(state + cap16 + (size_t)a.cap * 16) : a.scls + (size_t)f * a.cap;   // [cap]
    const float4 *ibox = a.box + (size_t)f * I * stride;
    const float *iconf = a.conf + (size_t)f * I * stride;
    const int32_t *icls = a.cls + (size_t)f * I * stride;

    // ---- 1. keys: (conf descending, image ascending, slot ascending) as one ascending 64-bit key ----
    for (int e = tid; e < I * stride; e += SM_THREADS) {
        const int j = e / stride, slot = e % stride;
        if (slot < s_off[j + 1] - s_off[j]) {
            const float c = iconf[e];
            unsigned u = c == 0.0f ? 0u : __float_as_uint(c);             // -0 and +0 compare equal
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                // ascending in the float order
            keys[s_off[j] + slot] = ((unsigned long long)(~u) << 32) | (unsigned)e;
        }
    }
    for (int i = N + tid; i < P; i += SM_THREADS) keys[i] = ~0ull;
    for (int i = tid; i < a.cap; i += SM_THREADS) state[i] = 0;
    __syncthreads();
    int Pn = 1;                                                            // sort only what holds candidates
    while (Pn < N) Pn <<= 1;
    for (int k = 2; k <= Pn; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (Pn >> 1); t += SM_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const unsigned long long x = keys[i], y = keys[l];
                const bool asc = (i & k) == 0;
                if ((x > y) == asc) { keys[i] = y; keys[l] = x; }
            }
            __syncthreads();
        }

    // ---- 2. the candidates in walk order, in frame coordinates ----
    const float W = (float)a.g.W, H = (float)a.g.H;
    for (int i = tid; i < N; i += SM_THREADS) {
        const int e = (int)(unsigned)(keys[i] & 0xFFFFFFFFull), j = e / stride;
        float4 b = ibox[e];
        if (j < T) {
            const float ox = (float)s_tx[j], oy = (float)s_ty[j];
            b.x = b.x + ox; b.z = b.z + ox; b.y = b.y + oy; b.w = b.w + oy;
        } else {
            b.x = b.x - a.pad_x; b.z = b.z - a.pad_x; b.y = b.y - a.pad_y; b.w = b.w - a.pad_y;
            b.x = b.x / a.gain; b.y = b.y / a.gain; b.z = b.z / a.gain; b.w = b.w / a.gain;
        }
        b.x = clipf(b.x, W); b.z = clipf(b.z, W); b.y = clipf(b.y, H); b.w = clipf(b.w, H);
        sbox[i] = b;
        scls[i] = icls[e];
    }
    __syncthreads();

    // ---- 3. the walk: one barrier per keeper; dead positions are stepped over 64 at a time by every wave for itself ----
    int kept = 0, cursor = 0;
    while (cursor < N && kept < a.max_out) {
        const int p = cursor + lane;
        const unsigned long long live = __ballot(p < N && state[p] == 0);
        if (live == 0ull) { cursor += 64; continue; }                      // uniform over the workgroup: state is settled here
        const int i = cursor + __builtin_ctzll(live);
        const float4 kb = sbox[i];
        const int kc = scls[i];
        const float ka = (kb.z - kb.x) * (kb.w - kb.y);
        float ux1 = kb.x, uy1 = kb.y, ux2 = kb.z, uy2 = kb.w;
        int cnt = 0;
        for (int q = i + 1 + tid; q < N; q += SM_THREADS) {
            if (state[q]) continue;
            if (!a.agnostic && scls[q] != kc) continue;
            const float4 b = sbox[q];
            if (slice_match(kb, ka, b, a.iou, a.thresh)) {
                state[q] = 1;
                ++cnt;
                ux1 = fminf(ux1, b.x); uy1 = fminf(uy1, b.y); ux2 = fmaxf(ux2, b.z); uy2 = fmaxf(uy2, b.w);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            cnt += __shfl_xor(cnt, d);
            ux1 = fminf(ux1, __shfl_xor(ux1, d)); uy1 = fminf(uy1, __shfl_xor(uy1, d));
            ux2 = fmaxf(ux2, __shfl_xor(ux2, d)); uy2 = fmaxf(uy2, __shfl_xor(uy2, d));
        }
        const int par = kept & 1;
        if (lane == 0) { s_cnt[par][wave] = cnt; s_red[par][wave][0] = ux1; s_red[par][wave][1] = uy1; s_red[par][wave][2] = ux2; s_red[par][wave][3] = uy2; }
        __syncthreads();                                                   // removals and partial unions visible
        if (tid == 0) {
            int c = 0;
            float4 u = kb;
            for (int w = 0; w < SM_WAVES; ++w) {
                c += s_cnt[par][w];
                u.x = fminf(u.x, s_red[par][w][0]); u.y = fminf(u.y, s_red[par][w][1]);
                u.z = fmaxf(u.z, s_red[par][w][2]); u.w = fmaxf(u.w, s_red[par][w][3]);
            }
            const int e = (int)(unsigned)(keys[i] & 0xFFFFFFFFull);
            const size_t o = (size_t)f * a.max_out + kept;
            a.out_box[o] = a.nms ? kb : u;
            a.out_conf[o] = iconf[e];
            a.out_cls[o] = kc;
            a.out_nm[o] = c;
        }
        kept += 1;
        cursor = i + 1;
    }
    if (tid == 0) a.out_n[f] = kept;
}

static size_t slice_merge_lds(int cap) {
    int P = 1;
    while (P < cap) P <<= 1;
    return align_up((size_t)P * 8, 16) + align_up((size_t)cap, 16) + (cap <= SM_LDS_BOX ? (size_t)cap * 20 : 0);
}

static int launch_slice_merge(const SliceMergeArgs &a, int frames, hipStream_t s) {
    RT_CHECK(a.cap >= 1 && a.cap <= SLICE_MAX_CAND && a.cap == a.g.I * a.stride, RTMODT_E_CAPACITY, "slice_merge: %d candidates per frame (at most %d)", a.cap,
             SLICE_MAX_CAND);
    const size_t smem = slice_merge_lds(a.cap);
    const bool lds_box = a.cap <= SM_LDS_BOX;
    static DynLdsSeen seen[2];
    RT_TRY(raise_dynamic_lds(lds_box ? (const void *)slice_merge_kernel<true> : (const void *)slice_merge_kernel<false>, smem, seen[lds_box]));
    if (lds_box) hipLaunchKernelGGL(slice_merge_kernel<true>, dim3(frames), dim3(SM_THREADS), smem, s, a);
    else hipLaunchKernelGGL(slice_merge_kernel<false>, dim3(frames), dim3(SM_THREADS), smem, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct SlicePlan {                           // everything a cfg decides, computed before the device is touched
    SliceGrid grid; SliceGeom geom{}; Letterbox lb{};        // lb: the overview (letterbox.h)
    int T = 0, I = 0, cap = 0;
    size_t img_bytes = 0;
};

static int slice_plan(const rtmodt_slice_cfg *c, int max_det, SlicePlan *p) {
    RT_CHECK(c && p, RTMODT_E_INVALID, "null argument");
    RT_CHECK(c->frame_w >= 1 && c->frame_h >= 1 && c->frame_w <= 16384 && c->frame_h <= 16384, RTMODT_E_INVALID, "frame %dx%d", c->frame_w, c->frame_h);
    RT_CHECK(c->tile_w >= 1 && c->tile_h >= 1, RTMODT_E_INVALID, "tile %dx%d", c->tile_w, c->tile_h);
    RT_CHECK(c->overlap_w >= 0 && c->overlap_w < c->tile_w && c->overlap_h >= 0 && c->overlap_h < c->tile_h, RTMODT_E_INVALID,
             "overlap %dx%d outside [0, tile %dx%d)", c->overlap_w, c->overlap_h, c->tile_w, c->tile_h);
    RT_CHECK(c->merge == RTMODT_SLICE_MERGE_NMM || c->merge == RTMODT_SLICE_MERGE_NMS, RTMODT_E_INVALID, "merge %d: 0 (NMM) or 1 (NMS)", c->merge);
    RT_CHECK(c->metric == RTMODT_SLICE_METRIC_IOS || c->metric == RTMODT_SLICE_METRIC_IOU, RTMODT_E_INVALID, "metric %d: 0 (IoS) or 1 (IoU)", c->metric);
    RT_CHECK(c->match_thresh == c->match_thresh, RTMODT_E_INVALID, "match_thresh is NaN");
    RT_CHECK(c->max_out >= 1 && c->max_out <= 4096, RTMODT_E_INVALID, "max_out %d outside [1, 4096]", c->max_out);
    RT_CHECK(max_det >= 1, RTMODT_E_INVALID, "max_det %d", max_det);
    const int rc = slice_grid(c->frame_w, c->frame_h, c->tile_w, c->tile_h, c->overlap_w, c->overlap_h, &p->grid);
    RT_CHECK(rc != 1, RTMODT_E_INVALID, "bad grid arguments");
    RT_CHECK(rc == 0, RTMODT_E_CAPACITY, "more than %d tiles per frame", SLICE_MAX_TILES);
    p->T = p->grid.tiles(); p->I = p->T + (c->overview ? 1 : 0);
    RT_CHECK((long)p->I * max_det <= SLICE_MAX_CAND, RTMODT_E_CAPACITY, "%d images x max_det %d = %ld candidates per frame, the merge takes %d", p->I, max_det,
             (long)p->I * max_det, SLICE_MAX_CAND);
    p->cap = p->I * max_det;
    SliceGeom &g = p->geom;
    g.W = c->frame_w; g.H = c->frame_h; g.te_w = p->grid.te_w; g.te_h = p->grid.te_h; g.T = p->T; g.I = p->I;
    for (int j = 0; j < p->T; ++j) { g.tx[j] = p->grid.x[j]; g.ty[j] = p->grid.y[j]; }
    p->lb = letterbox_geometry(c->frame_h, c->frame_w, g.te_h, g.te_w);
    p->img_bytes = (size_t)3 * g.te_w * g.te_h;
    return RTMODT_OK;
}

static SliceMergeArgs merge_args(const rtmodt_slice_cfg &c, const SlicePlan &p, int max_det) {
    SliceMergeArgs a{};
    a.g = p.geom; a.gain = (float)p.lb.gain; a.pad_x = (float)p.lb.pad_x; a.pad_y = (float)p.lb.pad_y;
    a.nms = c.merge == RTMODT_SLICE_MERGE_NMS; a.iou = c.metric == RTMODT_SLICE_METRIC_IOU; a.agnostic = c.agnostic != 0; a.max_out = c.max_out;
    a.thresh = c.match_thresh; a.stride = max_det; a.cap = p.cap;
    return a;
}

}  // namespace rtmodt

struct rtmodt_slicer : HandleBase {             // stream: staging copies + slice_gather; idle before the detector is handed the tile pointers
    rtmodt_slice_cfg cfg{};
    int max_det = 0;
    SlicePlan plan;
    FrameStage stage;                        // host frames, repacked to pitch 3 * frame_w; sized for max_frames at create
    uint8_t *d_tiles[2] = {nullptr, nullptr};   // the image batch of the two sliced batches that may be in flight
    int32_t *d_tab = nullptr; ResizeTables tabs{};
    float4 *d_sbox = nullptr; int32_t *d_scls = nullptr;      // merge scratch [max_frames][cap]
    struct Out {
        float4 *box = nullptr; float *conf = nullptr; int32_t *cls = nullptr, *nm = nullptr, *n = nullptr;      // device [max_frames][max_out], n [max_frames]
        char *host = nullptr;                // pinned mirror: box | conf | cls | nm | n
        hipEvent_t m0 = nullptr, m1 = nullptr, done = nullptr;
        int frames = 0;
    } out[2];
    hipEvent_t g0 = nullptr, g1 = nullptr;
    int head = 0, pending = 0, newest = -1, last_fetched = -1;
    hipStream_t merge_stream = nullptr;      // the detector's post-processing stream the newest merge was queued on
    float gather_ms = 0.f;
    std::vector<int32_t> tile_n;             // fetch's scratch when the caller does not want the per-image counts
};

namespace rtmodt {

int slicer_outputs(rtmodt_slicer *s, DetOutputs *o) {
    RT_CHECK(s && o, RTMODT_E_INVALID, "null argument");
    RT_CHECK(s->newest >= 0, RTMODT_E_INVALID, "slicer has no enqueued batch");
    const rtmodt_slicer::Out &b = s->out[s->newest];
    o->box = b.box; o->conf = b.conf; o->cls = b.cls; o->n = b.n;
    o->stride = s->cfg.max_out; o->count = b.frames; o->device = s->cfg.device; o->stream = s->merge_stream;
    return RTMODT_OK;
}

}  // namespace rtmodt

static size_t out_host_bytes(const rtmodt_slicer *s) { return (size_t)s->cfg.max_frames * s->cfg.max_out * 28 + (size_t)s->cfg.max_frames * 4; }

// frames -> the image batch d_tiles[buf], on the slicer's stream; returns with the stream idle
static int slicer_run_gather(rtmodt_slicer *s, const uint8_t *const *frames, int n, int pitch, int mem_kind, int buf) {
    const rtmodt_slice_cfg &c = s->cfg;
    SliceGatherArgs a{};
    a.g = s->plan.geom;
    a.lb = s->plan.lb.g;
    a.t = s->tabs;
    a.out = s->d_tiles[buf];
    RT_TRY(s->stage.in(frames, n, c.frame_h, c.frame_w, pitch, mem_kind, s->stream, FRAMES_TIGHT));
    for (int i = 0; i < n; ++i) a.frames.p[i] = s->stage.at(frames, i);
    a.pitch = (int)s->stage.pitch;
    RT_HIP(hipEventRecord(s->g0, s->stream));
    RT_TRY(launch_slice_gather(a, n, s->stream));
    RT_HIP(hipEventRecord(s->g1, s->stream));
    RT_HIP(hipStreamSynchronize(s->stream));
    RT_HIP(hipEventElapsedTime(&s->gather_ms, s->g0, s->g1));
    return RTMODT_OK;
}

static int slicer_check_frames(const rtmodt_slicer *s, const uint8_t *const *frames, int n, int pitch, int mem_kind) {
    RT_CHECK(s && frames, RTMODT_E_INVALID, "null argument");
    RT_CHECK(n >= 1 && n <= s->cfg.max_frames, RTMODT_E_INVALID, "n %d outside [1, max_frames %d]", n, s->cfg.max_frames);
    RT_CHECK(pitch_holds(pitch, s->cfg.frame_w), RTMODT_E_INVALID, "pitch %d < 3 x frame_w %d", pitch, s->cfg.frame_w);      // (h and w are the handle's)
    RT_TRY(check_mem_kind(mem_kind));
    return check_frame_ptrs(frames, n);
}

extern "C" {

int rtmodt_slice_grid(int frame_w, int frame_h, int tile_w, int tile_h, int overlap_w, int overlap_h, int32_t *xs, int32_t *ys, int32_t *n_tiles,
                      int32_t *te_w, int32_t *te_h) {
    SliceGrid g;
    const int rc = slice_grid(frame_w, frame_h, tile_w, tile_h, overlap_w, overlap_h, &g);
    RT_CHECK(rc != 1, RTMODT_E_INVALID, "slice_grid: frame %dx%d, tile %dx%d, overlap %dx%d (need frame >= 1, tile >= 1, 0 <= overlap < tile)", frame_w, frame_h,
             tile_w, tile_h, overlap_w, overlap_h);
    RT_CHECK(rc == 0, RTMODT_E_CAPACITY, "slice_grid: more than %d tiles per frame", SLICE_MAX_TILES);
    for (int j = 0; j < g.tiles(); ++j) {
        if (xs) xs[j] = g.x[j];
        if (ys) ys[j] = g.y[j];
    }
    if (n_tiles) *n_tiles = g.tiles();
    if (te_w) *te_w = g.te_w;
    if (te_h) *te_h = g.te_h;
    return RTMODT_OK;
}

void rtmodt_slicer_destroy(rtmodt_slicer *s) {
    if (!s) return;
    hipSetDevice(s->cfg.device);
    for (auto &o : s->out)
        if (o.done) hipEventSynchronize(o.done);         // a merge may still be queued on a detector's stream
    handle_close(s, [&] {
        for (auto &o : s->out) {
            hipFree(o.box); hipFree(o.conf); hipFree(o.cls); hipFree(o.nm); hipFree(o.n); hipHostFree(o.host);
            if (o.m0) hipEventDestroy(o.m0);
            if (o.m1) hipEventDestroy(o.m1);
            if (o.done) hipEventDestroy(o.done);
        }
        if (s->g0) hipEventDestroy(s->g0);
        if (s->g1) hipEventDestroy(s->g1);
        s->stage.release(); hipFree(s->d_tiles[0]); hipFree(s->d_tiles[1]); hipFree(s->d_tab); hipFree(s->d_sbox); hipFree(s->d_scls);
    });
    delete s;
}

static int slicer_create_impl(rtmodt_slicer *s) {
    const rtmodt_slice_cfg &c = s->cfg;
    const SlicePlan &p = s->plan;
    RT_TRY(handle_open(s));
    RT_HIP(hipEventCreate(&s->g0)); RT_HIP(hipEventCreate(&s->g1));
    RT_TRY(s->stage.reserve((size_t)c.max_frames * c.frame_h * c.frame_w * 3));      // max_frames in the FRAMES_TIGHT layout: every call fits
    const size_t batch_bytes = (size_t)c.max_frames * p.I * p.img_bytes;
    for (int b = 0; b < 2; ++b) RT_HIP(hipMalloc((void **)&s->d_tiles[b], batch_bytes + 256));      // (slack: a reader may take the last row in wide loads)
    if (c.overview && p.lb.g.resize) {
        RT_HIP(hipMalloc((void **)&s->d_tab, (size_t)3 * (p.lb.g.new_w + p.lb.g.new_h) * 4));
        RT_TRY(upload_resize_tables(p.lb.g, s->d_tab, &s->tabs));
    }
    RT_HIP(hipMalloc((void **)&s->d_sbox, (size_t)c.max_frames * p.cap * 16));
    RT_HIP(hipMalloc((void **)&s->d_scls, (size_t)c.max_frames * p.cap * 4));
    const size_t FO = (size_t)c.max_frames * c.max_out;
    for (auto &o : s->out) {
        RT_HIP(hipMalloc((void **)&o.box, FO * 16)); RT_HIP(hipMalloc((void **)&o.conf, FO * 4)); RT_HIP(hipMalloc((void **)&o.cls, FO * 4));
        RT_HIP(hipMalloc((void **)&o.nm, FO * 4)); RT_HIP(hipMalloc((void **)&o.n, (size_t)c.max_frames * 4));
        RT_HIP(handle_zero(o.n, (size_t)c.max_frames * 4, s->stream));
        RT_HIP(hipHostMalloc((void **)&o.host, out_host_bytes(s), hipHostMallocDefault));
        RT_HIP(hipEventCreate(&o.m0)); RT_HIP(hipEventCreate(&o.m1));
        RT_HIP(hipEventCreateWithFlags(&o.done, hipEventDisableTiming));
    }
    s->tile_n.assign((size_t)c.max_frames * p.I, 0);
    return RTMODT_OK;
}

int rtmodt_slicer_create(const rtmodt_slice_cfg *cfg, int max_det, rtmodt_slicer **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    SlicePlan plan;
    RT_TRY(slice_plan(cfg, max_det, &plan));
    RT_CHECK(cfg->max_frames >= 1 && (long)cfg->max_frames * plan.I <= 64, RTMODT_E_CAPACITY,
             "max_frames %d x %d images per frame: a detector batch holds at most 64 images", cfg->max_frames, plan.I);
    rtmodt_slicer *s = new rtmodt_slicer();
    s->device = cfg->device; s->cfg = *cfg; s->max_det = max_det; s->plan = plan;
    return handle_created(slicer_create_impl(s), s, rtmodt_slicer_destroy, out);
}

int rtmodt_slicer_info(rtmodt_slicer *s, int32_t *n_tiles, int32_t *images_per_frame, int32_t *te_w, int32_t *te_h) {
    RT_CHECK(s, RTMODT_E_INVALID, "null argument");
    if (n_tiles) *n_tiles = s->plan.T;
    if (images_per_frame) *images_per_frame = s->plan.I;
    if (te_w) *te_w = s->plan.geom.te_w;
    if (te_h) *te_h = s->plan.geom.te_h;
    return RTMODT_OK;
}

int rtmodt_slicer_gather(rtmodt_slicer *s, const uint8_t *const *frames, int n, int pitch, int mem_kind, uint8_t *tiles_out_host) {
    RT_TRY(slicer_check_frames(s, frames, n, pitch, mem_kind));
    RT_CHECK(tiles_out_host, RTMODT_E_INVALID, "null argument");
    RT_CHECK(s->pending == 0, RTMODT_E_INVALID, "gather with %d sliced batches in flight: fetch them first", s->pending);
    RT_HIP(hipSetDevice(s->cfg.device));
    RT_TRY(slicer_run_gather(s, frames, n, pitch, mem_kind, s->head));
    RT_HIP(hipMemcpy(tiles_out_host, s->d_tiles[s->head], (size_t)n * s->plan.I * s->plan.img_bytes, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_slice_merge(int device, const rtmodt_slice_cfg *cfg, int max_det, int n_frames, const float *det_xyxy, const float *det_conf,
                       const int32_t *det_cls, const int32_t *det_n, float *xyxy, float *conf, int32_t *cls, int32_t *n_merged, int32_t *n_out,
                       float *kernel_ms) {
    RT_CHECK(cfg && det_xyxy && det_conf && det_cls && det_n && xyxy && conf && cls && n_merged && n_out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(n_frames >= 1 && n_frames <= 4096, RTMODT_E_INVALID, "n_frames %d", n_frames);
    SlicePlan p;
    RT_TRY(slice_plan(cfg, max_det, &p));
    const size_t NI = (size_t)n_frames * p.I, FO = (size_t)n_frames * cfg->max_out;
    for (size_t i = 0; i < NI; ++i) RT_CHECK(det_n[i] >= 0 && det_n[i] <= max_det, RTMODT_E_INVALID, "image %zu: %d detections outside [0, max_det %d]", i, det_n[i], max_det);
    RT_HIP(hipSetDevice(device));
    char *pool = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto body = [&]() -> int {
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
        const size_t o_box = take(NI * max_det * 16), o_conf = take(NI * max_det * 4), o_cls = take(NI * max_det * 4), o_n = take(NI * 4);
        const size_t o_sbox = take((size_t)n_frames * p.cap * 16), o_scls = take((size_t)n_frames * p.cap * 4);
        const size_t r_box = take(FO * 16), r_conf = take(FO * 4), r_cls = take(FO * 4), r_nm = take(FO * 4), r_n = take((size_t)n_frames * 4);
        RT_HIP(hipMalloc((void **)&pool, off));
        RT_HIP(hipMemcpy(pool + o_box, det_xyxy, NI * max_det * 16, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(pool + o_conf, det_conf, NI * max_det * 4, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(pool + o_cls, det_cls, NI * max_det * 4, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(pool + o_n, det_n, NI * 4, hipMemcpyHostToDevice));
        SliceMergeArgs a = merge_args(*cfg, p, max_det);
        a.box = (const float4 *)(pool + o_box); a.conf = (const float *)(pool + o_conf); a.cls = (const int32_t *)(pool + o_cls); a.n = (const int32_t *)(pool + o_n);
        a.sbox = (float4 *)(pool + o_sbox); a.scls = (int32_t *)(pool + o_scls);
        a.out_box = (float4 *)(pool + r_box); a.out_conf = (float *)(pool + r_conf); a.out_cls = (int32_t *)(pool + r_cls);
        a.out_nm = (int32_t *)(pool + r_nm); a.out_n = (int32_t *)(pool + r_n);
        RT_HIP(hipEventCreate(&e0)); RT_HIP(hipEventCreate(&e1));
        RT_HIP(hipEventRecord(e0, nullptr));
        RT_TRY(launch_slice_merge(a, n_frames, nullptr));
        RT_HIP(hipEventRecord(e1, nullptr));
        RT_HIP(hipDeviceSynchronize());
        if (kernel_ms) RT_HIP(hipEventElapsedTime(kernel_ms, e0, e1));
        RT_HIP(hipMemcpy(xyxy, pool + r_box, FO * 16, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(conf, pool + r_conf, FO * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(cls, pool + r_cls, FO * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(n_merged, pool + r_nm, FO * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(n_out, pool + r_n, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
        return RTMODT_OK;
    };
    const int rc = body();
    hipFree(pool);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    return rc;
}

int rtmodt_slicer_enqueue(rtmodt_slicer *s, rtmodt_detector *det, const uint8_t *const *frames, int n, int pitch, int mem_kind) {
    RT_CHECK(det, RTMODT_E_INVALID, "null argument");
    RT_TRY(slicer_check_frames(s, frames, n, pitch, mem_kind));
    RT_CHECK(s->pending < 2, RTMODT_E_INVALID, "two sliced batches already in flight: fetch before enqueueing more");
    const SlicePlan &p = s->plan;
    DetLimits lim;
    RT_TRY(detector_limits(det, &lim));
    RT_CHECK(lim.device == s->cfg.device, RTMODT_E_INVALID, "slicer on device %d, detector on device %d", s->cfg.device, lim.device);
    RT_CHECK(lim.max_det == s->max_det, RTMODT_E_INVALID, "detector max_det %d, slicer built for %d", lim.max_det, s->max_det);
    RT_CHECK(lim.batch >= n * p.I, RTMODT_E_CAPACITY, "%d frames x %d images = %d, detector batch %d", n, p.I, n * p.I, lim.batch);
    RT_CHECK(lim.max_src_w >= p.geom.te_w && lim.max_src_h >= p.geom.te_h, RTMODT_E_CAPACITY, "tile %dx%d exceeds the detector's max_src %dx%d", p.geom.te_w,
             p.geom.te_h, lim.max_src_w, lim.max_src_h);
    RT_CHECK(lim.pending == s->pending, RTMODT_E_INVALID, "the detector has %d batches in flight, %d of them this slicer's: fetch the others first", lim.pending,
             s->pending);
    RT_HIP(hipSetDevice(s->cfg.device));
    const int b = s->head;
    rtmodt_slicer::Out &o = s->out[b];
    RT_TRY(slicer_run_gather(s, frames, n, pitch, mem_kind, b));
    const uint8_t *imgs[64];
    for (int i = 0; i < n * p.I; ++i) imgs[i] = s->d_tiles[b] + (size_t)i * p.img_bytes;
    RT_TRY(rtmodt_detector_enqueue_batch(det, imgs, n * p.I, p.geom.te_h, p.geom.te_w, 3 * p.geom.te_w, RTMODT_MEM_DEVICE));
    // from here on the detector has a batch in flight that fetch must drain, whatever happens to the merge
    s->head ^= 1; s->pending += 1; s->newest = b; o.frames = n;
    DetOutputs d;
    RT_TRY(detector_outputs(det, &d));
    s->merge_stream = d.stream;
    SliceMergeArgs a = merge_args(s->cfg, p, s->max_det);
    a.box = d.box; a.conf = d.conf; a.cls = d.cls; a.n = d.n;
    a.sbox = s->d_sbox; a.scls = s->d_scls;
    a.out_box = o.box; a.out_conf = o.conf; a.out_cls = o.cls; a.out_nm = o.nm; a.out_n = o.n;
    RT_HIP(hipEventRecord(o.m0, d.stream));
    RT_TRY(launch_slice_merge(a, n, d.stream));             // behind the detector's NMS on its own stream: ordered, no host round trip
    RT_HIP(hipEventRecord(o.m1, d.stream));
    const size_t FO = (size_t)s->cfg.max_frames * s->cfg.max_out, no = (size_t)n * s->cfg.max_out;
    RT_HIP(hipMemcpyAsync(o.host, o.box, no * 16, hipMemcpyDeviceToHost, d.stream));
    RT_HIP(hipMemcpyAsync(o.host + FO * 16, o.conf, no * 4, hipMemcpyDeviceToHost, d.stream));
    RT_HIP(hipMemcpyAsync(o.host + FO * 20, o.cls, no * 4, hipMemcpyDeviceToHost, d.stream));
    RT_HIP(hipMemcpyAsync(o.host + FO * 24, o.nm, no * 4, hipMemcpyDeviceToHost, d.stream));
    RT_HIP(hipMemcpyAsync(o.host + FO * 28, o.n, (size_t)n * 4, hipMemcpyDeviceToHost, d.stream));
    RT_HIP(hipEventRecord(o.done, d.stream));
    return RTMODT_OK;
}

int rtmodt_slicer_fetch(rtmodt_slicer *s, rtmodt_detector *det, float *xyxy, float *conf, int32_t *cls, int32_t *n_merged, int32_t *n_out,
                        float *tile_xyxy, float *tile_conf, int32_t *tile_cls, int32_t *tile_n) {
    RT_CHECK(s && det && n_out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(s->pending > 0, RTMODT_E_INVALID, "fetch without a pending enqueue");
    RT_HIP(hipSetDevice(s->cfg.device));
    const int b = (s->head + 2 - s->pending) % 2;            // oldest in flight
    rtmodt_slicer::Out &o = s->out[b];
    RT_TRY(rtmodt_detector_fetch(det, tile_xyxy, tile_conf, tile_cls, tile_n ? tile_n : s->tile_n.data()));
    s->pending -= 1;
    s->last_fetched = b;
    RT_HIP(hipEventSynchronize(o.done));
    const size_t FO = (size_t)s->cfg.max_frames * s->cfg.max_out, no = (size_t)o.frames * s->cfg.max_out;
    if (xyxy) memcpy(xyxy, o.host, no * 16);
    if (conf) memcpy(conf, o.host + FO * 16, no * 4);
    if (cls) memcpy(cls, o.host + FO * 20, no * 4);
    if (n_merged) memcpy(n_merged, o.host + FO * 24, no * 4);
    memcpy(n_out, o.host + FO * 28, (size_t)o.frames * 4);
    return RTMODT_OK;
}

int rtmodt_slicer_last_ms(rtmodt_slicer *s, float *gather_ms, float *merge_ms) {
    RT_CHECK(s, RTMODT_E_INVALID, "null argument");
    RT_CHECK(s->last_fetched >= 0, RTMODT_E_INVALID, "no sliced batch has been fetched yet");
    if (gather_ms) *gather_ms = s->gather_ms;
    if (merge_ms) {
        RT_HIP(hipSetDevice(s->cfg.device));
        RT_HIP(hipEventElapsedTime(merge_ms, s->out[s->last_fetched].m0, s->out[s->last_fetched].m1));
    }
    return RTMODT_OK;
}

}  // extern "C"
