// appearance.hip -- the appearance side of the DeepSORT tracker (deepsort.hip): one descriptor per detection box, and the
// gallery-to-detection distance on the int8 matrix cores.  Serves the reference's `deepsort:` block (config/default.yaml:
// `embedder`, `max_dist`, `nn_budget`); the descriptor is the colour histogram its design document proposes (B.4), because the
// embedder file the config names ships nowhere.  Everything here is integer arithmetic: tests/deepsort_ref.py restates it and
// the results agree byte for byte.
//
// Descriptor of a box on a BGR24 frame (h x w, row pitch >= 3w):
//   corners   int(v) (truncation, clamped to +-2^20 first, like render.hip), then clamped to the frame: pixels x0 <= x < x1,
//             y0 <= y < y1; H = y1 - y0, W = x1 - x0.  H <= 0, W <= 0 or a NaN corner: the all-zero descriptor.
//   bins      D = 192 = 4 horizontal stripes x (B, G, R) x 16 bins; stripe s = rows y0 + (s*H)/4 .. y0 + ((s+1)*H)/4 - 1;
//             bin = value >> 4; index = s*48 + c*16 + bin; int32 counts.
//   int8      n2 = sum count^2 (int64), r = floor(sqrt(n2)) exactly, q = min(127, (127*count + r/2) / r); r == 0: zeros.
// Two launches per batch whatever the number of boxes: appearance_hist (grid = box slot x stream x stripe; a workgroup reads
// its stripe's pixels once and owns its 48 bins, so the counts need neither zeroing nor global atomics) and
// appearance_quant (one workgroup per box slot).
//
// Distance: dotmax[t][n] = max over track t's stored samples of <sample, descriptor n>, int8 x int8 -> int32 with
// v_mfma_i32_16x16x64_i8.  A = 16 samples x 64 k, B = 64 k x 16 descriptors; lane l holds the 16 consecutive k of group l >> 4
// for row / column l & 15 -- both operands take the same k from the same lane group, and integer accumulation is exact, so
// the sum does not depend on the order inside a group.  C: column l & 15, rows 4 * (l >> 4) + reg.
#include "kernels.h"
#include "frame_stage.h"

#include <climits>
#include <cmath>

namespace rtmodt {

constexpr int APP_COORD_MAX = 1 << 20;

__device__ __forceinline__ int app_coord(float v) { return (int)truncf(fminf(fmaxf(v, (float)-APP_COORD_MAX), (float)APP_COORD_MAX)); }

constexpr int HIST_THREADS = 256;

__global__ __launch_bounds__(HIST_THREADS) void appearance_hist(DescribeArgs a) {
    const int b = blockIdx.x, s = blockIdx.y, stripe = blockIdx.z;
    if (b >= a.box_n[s]) return;
    __shared__ int hist[4][48];                            // one copy per wave: fewer LDS atomic collisions on flat colours
    for (int i = threadIdx.x; i < 4 * 48; i += HIST_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    const float4 bx = a.box[(size_t)s * a.box_stride + b];
    const bool nan = bx.x != bx.x || bx.y != bx.y || bx.z != bx.z || bx.w != bx.w;
    const int x0 = min(max(app_coord(bx.x), 0), a.w), x1 = min(max(app_coord(bx.z), 0), a.w);
    const int y0 = min(max(app_coord(bx.y), 0), a.h), y1 = min(max(app_coord(bx.w), 0), a.h);
    const int W = x1 - x0, H = y1 - y0;
    if (!nan && W > 0 && H > 0) {
        const int r0 = y0 + (stripe * H) / 4, r1 = y0 + ((stripe + 1) * H) / 4;     // rows r0 <= y < r1, all inside [0, h)
        const int rowbytes = 3 * W;
        const uint8_t *f = a.frames.p[s] + (size_t)3 * x0;
        int *hw = hist[threadIdx.x >> 6];
        const long total = (long)(r1 - r0) * rowbytes;
        for (long i = threadIdx.x; i < total; i += HIST_THREADS) {
            const int row = (int)(i / rowbytes), off = (int)(i - (long)row * rowbytes);
            const int v = f[(size_t)(r0 + row) * a.pitch + off];
            atomicAdd(&hw[(off % 3) * 16 + (v >> 4)], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 48) {
        const int t = threadIdx.x;
        a.counts[((size_t)s * a.max_boxes + b) * APP_DIM + stripe * 48 + t] = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
    }
}

__global__ __launch_bounds__(APP_DIM) void appearance_quant(DescribeArgs a) {
    const int b = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    if (b >= a.box_n[s]) return;
    __shared__ long long part[APP_DIM / 64];
    const long long c = a.counts[((size_t)s * a.max_boxes + b) * APP_DIM + t];
    long long sq = c * c;
    for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d);
    if ((t & 63) == 0) part[t >> 6] = sq;
    __syncthreads();
    const long long r = isqrt64(part[0] + part[1] + part[2]);
    int q = 0;
    if (r > 0) q = (int)min(127ll, (127 * c + r / 2) / r);
    a.desc[((size_t)s * a.desc_stride + b) * APP_DIM + t] = (int8_t)q;
}

int launch_describe(const DescribeArgs &a, int n_streams, hipStream_t s) {
    if (n_streams <= 0 || a.max_boxes <= 0) return RTMODT_OK;
    hipLaunchKernelGGL(appearance_hist, dim3(a.max_boxes, n_streams, 4), dim3(HIST_THREADS), 0, s, a);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(appearance_quant, dim3(a.max_boxes, n_streams), dim3(APP_DIM), 0, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// dotmax: grid (track slot, 64-descriptor tile, stream), 4 waves; wave w owns descriptors [64 * tile + 16 w, + 16)
// ---------------------------------------------------------------------------------------------------------------------
typedef int intx4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void appearance_dotmax(DotmaxArgs a) {
    const int t = blockIdx.x, s = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = a.states || a.meta_rows ? (int)a.meta[(size_t)s * 8 + 1] : a.n_tracks;
    const int N = a.n_dets_dev ? min(a.n_dets_dev[s], a.max_dets) : a.n_dets;
    const int col0 = blockIdx.y * 64 + wave * 16;
    if (t >= T || col0 >= N) return;                       // wave-uniform
    int slot = t, cnt;
    if (a.states) {
        const int cur = (int)a.meta[(size_t)s * 8];
        const DsState &st = a.states[s];
        slot = (cur ? st.slot[1] : st.slot[0])[t];
        cnt = (cur ? st.gcount[1] : st.gcount[0])[t];
    } else if (a.meta_rows) {
        cnt = 1;
    } else {
        cnt = a.counts[t];
    }
    if (slot < 0 || slot >= DS_MAX_TRACKS) return;
    cnt = min(max(cnt, 0), a.budget);
    const int KC = a.dim / 64;                             // 1..8
    const int col = col0 + (lane & 15), kg = 16 * (lane >> 4);
    const int8_t *dp = a.dets + ((size_t)s * a.det_stride + col) * a.dim + kg;
    intx4_t bf[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        bf[k] = intx4_t{0, 0, 0, 0};
        if (k < KC && col < N) bf[k] = *(const intx4_t *)(dp + 64 * k);
    }
    const int8_t *gp = a.gallery + ((size_t)s * a.gallery_stream_stride + (size_t)slot * a.budget * a.dim);
    if (a.meta_rows) gp += (size_t)(a.meta[(size_t)s * 8] & 1) * a.gallery_cur_stride;
    int best = INT_MIN;
    for (int r0 = 0; r0 < cnt; r0 += 16) {
        const int row = r0 + (lane & 15);
        intx4_t acc = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < KC) {
                intx4_t af = {0, 0, 0, 0};
                if (row < cnt) af = *(const intx4_t *)(gp + (size_t)row * a.dim + 64 * k + kg);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[k], acc, 0, 0, 0);
            }
        }
        const int rbase = r0 + 4 * (lane >> 4);            // C: rows rbase + j of column lane & 15
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rbase + j < cnt) best = max(best, acc[j]);
    }
    best = max(best, __shfl_xor(best, 16));
    best = max(best, __shfl_xor(best, 32));
    if (lane < 16 && col < N) a.out[((size_t)s * a.out_stream_stride) + (size_t)t * a.out_row_stride + col] = best;
}

int launch_dotmax(const DotmaxArgs &a, int grid_tracks, int grid_dets, int n_streams, hipStream_t s) {
    if (grid_tracks <= 0 || grid_dets <= 0 || n_streams <= 0) return RTMODT_OK;
    hipLaunchKernelGGL(appearance_dotmax, dim3(grid_tracks, cdiv(grid_dets, 64), n_streams), dim3(256), 0, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

}  // namespace rtmodt

using namespace rtmodt;

extern "C" {

int rtmodt_appearance_quantize(const float *x, int n, int dim, int8_t *out) {
    RT_CHECK(n >= 0 && dim >= 64 && dim <= 512 && dim % 64 == 0, RTMODT_E_INVALID, "n %d, dim %d: rows of 64..512 values in multiples of 64", n, dim);
    RT_CHECK(n == 0 || (x && out), RTMODT_E_INVALID, "null argument");
    for (int i = 0; i < n; ++i) {
        const float *row = x + (size_t)i * dim;
        double n2 = 0.0;
        for (int k = 0; k < dim; ++k) n2 += (double)row[k] * (double)row[k];      // sequential, float64
        const double norm = std::sqrt(n2);
        for (int k = 0; k < dim; ++k) {
            double q = 0.0;
            if (norm > 0.0 && norm == norm && std::isfinite(norm)) q = std::nearbyint(127.0 * (double)row[k] / norm);   // round half to even, like np.rint
            out[(size_t)i * dim + k] = (int8_t)(q != q ? 0.0 : std::min(127.0, std::max(-127.0, q)));
        }
    }
    return RTMODT_OK;
}

int rtmodt_appearance_describe(int device, const uint8_t *const *frames, int n_frames, int h, int w, int stride_bytes, int mem_kind,
                               const float *xyxy, const int32_t *n_boxes, int max_boxes, int8_t *desc, int32_t *counts) {
    RT_CHECK(n_frames >= 0 && n_frames <= 64, RTMODT_E_CAPACITY, "%d frames: at most 64 per call", n_frames);
    if (n_frames == 0) return RTMODT_OK;
    RT_CHECK(frames && xyxy && n_boxes && desc, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_frame_block(n_frames, h, w, stride_bytes, mem_kind, kAppFrames));
    RT_CHECK(max_boxes >= 1 && max_boxes <= 1024, RTMODT_E_CAPACITY, "max_boxes %d: 1..1024", max_boxes);
    for (int i = 0; i < n_frames; ++i) {
        RT_CHECK(frames[i], RTMODT_E_INVALID, "frame %d is null", i);
        RT_CHECK(n_boxes[i] >= 0, RTMODT_E_INVALID, "frame %d: %d boxes", i, n_boxes[i]);
        RT_CHECK(n_boxes[i] <= max_boxes, RTMODT_E_CAPACITY, "frame %d: %d boxes > max_boxes %d", i, n_boxes[i], max_boxes);
    }
    RT_HIP(hipSetDevice(device));
    const size_t nb = (size_t)n_frames * max_boxes;
    FrameStage stage;                                       // of this call alone
    float4 *d_box = nullptr; int32_t *d_n = nullptr, *d_counts = nullptr; int8_t *d_desc = nullptr;
    auto body = [&]() -> int {
        DescribeArgs a{};
        RT_TRY(stage.in(frames, n_frames, h, w, stride_bytes, mem_kind, nullptr, FRAMES_AS_GIVEN));
        for (int i = 0; i < n_frames; ++i) a.frames.p[i] = stage.at(frames, i);
        RT_HIP(hipMalloc((void **)&d_box, nb * 16)); RT_HIP(hipMalloc((void **)&d_n, (size_t)n_frames * 4));
        RT_HIP(hipMalloc((void **)&d_counts, nb * APP_DIM * 4)); RT_HIP(hipMalloc((void **)&d_desc, nb * APP_DIM));
        RT_HIP(hipMemset(d_counts, 0, nb * APP_DIM * 4)); RT_HIP(hipMemset(d_desc, 0, nb * APP_DIM));
        RT_HIP(hipMemcpy(d_box, xyxy, nb * 16, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_n, n_boxes, (size_t)n_frames * 4, hipMemcpyHostToDevice));
        a.h = h; a.w = w; a.pitch = stride_bytes; a.box = d_box; a.box_n = d_n; a.box_stride = max_boxes; a.max_boxes = max_boxes;
        a.counts = d_counts; a.desc = d_desc; a.desc_stride = max_boxes;
        RT_TRY(launch_describe(a, n_frames, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(desc, d_desc, nb * APP_DIM, hipMemcpyDeviceToHost));
        if (counts) RT_HIP(hipMemcpy(counts, d_counts, nb * APP_DIM * 4, hipMemcpyDeviceToHost));
        return RTMODT_OK;
    };
    const int rc = body();
    stage.release(); hipFree(d_box); hipFree(d_n); hipFree(d_counts); hipFree(d_desc);
    return rc;
}

int rtmodt_appearance_dotmax(int device, const int8_t *gallery, const int32_t *counts, int n_tracks, int budget, const int8_t *dets,
                             int n_dets, int dim, int32_t *out) {
    RT_CHECK(n_tracks >= 0 && n_dets >= 0 && budget >= 1, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(dim >= 64 && dim <= 512 && dim % 64 == 0, RTMODT_E_INVALID, "dim %d: 64..512 in multiples of 64", dim);
    RT_CHECK(n_tracks <= 256 && n_dets <= 1024 && budget <= 128, RTMODT_E_CAPACITY, "%d tracks / %d detections / budget %d: at most 256 / 1024 / 128",
             n_tracks, n_dets, budget);
    if (n_tracks == 0 || n_dets == 0) return RTMODT_OK;
    RT_CHECK(gallery && counts && dets && out, RTMODT_E_INVALID, "null argument");
    for (int t = 0; t < n_tracks; ++t) RT_CHECK(counts[t] >= 0 && counts[t] <= budget, RTMODT_E_INVALID, "track %d: %d samples, budget %d", t, counts[t], budget);
    RT_HIP(hipSetDevice(device));
    int8_t *d_g = nullptr, *d_d = nullptr; int32_t *d_c = nullptr, *d_o = nullptr;
    const size_t gb = (size_t)n_tracks * budget * dim, db = (size_t)n_dets * dim, ob = (size_t)n_tracks * n_dets * 4;
    auto body = [&]() -> int {
        RT_HIP(hipMalloc((void **)&d_g, gb)); RT_HIP(hipMalloc((void **)&d_d, db));
        RT_HIP(hipMalloc((void **)&d_c, (size_t)n_tracks * 4)); RT_HIP(hipMalloc((void **)&d_o, ob));
        RT_HIP(hipMemcpy(d_g, gallery, gb, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(d_d, dets, db, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_c, counts, (size_t)n_tracks * 4, hipMemcpyHostToDevice));
        DotmaxArgs a{};
        a.gallery = d_g; a.counts = d_c; a.budget = budget; a.dim = dim; a.dets = d_d; a.det_stride = n_dets; a.n_tracks = n_tracks;
        a.n_dets = n_dets; a.max_dets = n_dets; a.out = d_o; a.out_row_stride = n_dets;
        RT_TRY(launch_dotmax(a, n_tracks, n_dets, 1, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(out, d_o, ob, hipMemcpyDeviceToHost));
        return RTMODT_OK;
    };
    const int rc = body();
    hipFree(d_g); hipFree(d_d); hipFree(d_c); hipFree(d_o);
    return rc;
}

}  // extern "C"
