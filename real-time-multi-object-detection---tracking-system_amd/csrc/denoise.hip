// denoise.hip -- frame noise reduction on the GPU ("3DNR"): a motion-adaptive temporal filter per pixel, with a sigma filter of the
// current frame taken in where the temporal filter lets go, directly after `stabilize` (a temporal filter needs registered frames) and
// directly before `enhance` (which should equalise the clean picture, not the noise): pipeline.run(denoise=...).  The reference hands
// cap.read()'s frame on (rtsp_reader.py) and has no counterpart; PARITY UNPINNED against any camera's 3DNR, cv2.fastNlMeansDenoising
// and ffmpeg's hqdn3d, and against any default tuned on real footage.  tests/denoise_ref.py restates every rule in NumPy and the
// kernel equals it exactly: all of it is integer arithmetic, no float appears anywhere.
//
// Rules: denoise_rule.h (pixel luma: motion_model.h).  A stream holds acc (uint16 8.8 per pixel and channel, rows of 24 bytes per run
// of 4 pixels so that a lane's 24 bytes are 8-byte aligned whatever the width), a double-buffered uint8 plane of Y(prev) (rows of 4
// bytes per run), frames_seen and the index of the plane that is current.  The neighbours' Y(prev) must come from before the call
// while every lane replaces its own: the call reads one plane and writes the other, and dn_finish swaps them.  acc is read and
// written by the same lane and needs one buffer.  20 bytes of traffic per pixel: 3 + 6 + 1 in, 3 + 6 + 1 out.
//
// Kernels (256 threads; a memset of the call's counters and TWO launches per call for all its streams, whatever the frames show; no
// grid-wide barrier, no spin on another workgroup; every sum is an integer sum, so its order cannot change a result):
//   dn_filter  one workgroup per tile of 256 x 16 pixels of a frame.  It stages the tile and a 1-pixel halo (coordinates clamped to
//              the frame) in LDS: the frame's bytes with Y(x) in the fourth byte of a dword, and Y(x) - Y(prev) as int16.  Every frame
//              byte and every byte of the Y(prev) plane is read once apart from the halo; a lane owns a run of 4 pixels (12-byte loads
//              and stores where base and pitch allow, bytes otherwise; the plane and acc always in dwords).  LDS column c lies at
//              [c % 4][c / 4]: the lanes of a wave read neighbouring words, where [c] would put them 4 words apart (4 lanes to a
//              bank).  A lane reads the 3 x 6 words around its run once and runs dn_pixel for its 4 pixels.  The counters go through
//              wave sums, LDS and one integer atomic per workgroup and counter.
//   dn_finish  one thread per frame: the result row, frames_seen, the swap of the planes.
// An output depends on its neighbours' inputs: there is no in-place form, and a destination may meet no source of the call.
#include <algorithm>
#include <cstring>
#include <vector>

#define MO_HD __host__ __device__
#include "grid_host.h"
#include "denoise_rule.h"

namespace rtmodt {

#include "wg_dev.h"

constexpr int DN_THREADS = 256, DN_WAVES = DN_THREADS / 64;
constexpr int DN_TW = 64 * DN_RUN, DN_TH = 16;              // the tile
constexpr int DN_LROWS = DN_TH + 2, DN_PLANE = 65, DN_LROW = DN_RUN * DN_PLANE;     // LDS: rows, words of one c % 4, words of a row
constexpr int DN_MAX_STREAMS = 1024;
constexpr long long DN_MAX_PIXELS = 1LL << 30;              // over all streams: 6 GiB of acc
static_assert(sizeof(rtmodt_denoise_result) == 24, "layout");
static_assert((DN_TW + 2 + DN_RUN - 1) / DN_RUN <= DN_PLANE, "the halo columns fit");

struct DnSlot { uint64_t src, dst; int32_t stream, pad; };
static_assert(sizeof(DnSlot) == 24, "layout");
struct DnCount { unsigned long long absdiff; uint32_t n_static, n_moving; };
static_assert(sizeof(DnCount) == 16, "layout");
struct __attribute__((aligned(8))) DnAccRun { uint32_t v[6]; };            // 4 pixels x 3 channels x uint16

struct DnArgs {
    const DnSlot *slots;
    long long spitch, dpitch;
    int n, h, w, blocks_x;
    DnRule rule;
    uint8_t *acc; long long acc_pitch, acc_stream;          // bytes: a row, a stream
    uint8_t *yprev; long long y_pitch, y_plane;             // bytes: a row, a plane; a stream holds two planes
    int32_t *seen, *cur;                                    // per stream: frames_seen, the plane that holds Y(prev)
    DnCount *cnt;                                           // [n], zeroed before the launches
    rtmodt_denoise_result *res;                             // [n]
};

__device__ __forceinline__ int dn_lds_at(int r, int c) { return r * DN_LROW + (c & 3) * DN_PLANE + (c >> 2); }

template <bool WSRC, bool WDST> __global__ __launch_bounds__(DN_THREADS) void dn_filter(DnArgs a) {
    __shared__ uint32_t s_px[DN_LROWS * DN_LROW];           // b | g << 8 | r << 16 | Y(x) << 24
    __shared__ int16_t s_dy[DN_LROWS * DN_LROW];            // Y(x) - Y(prev)
    __shared__ uint32_t s_cnt[DN_WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bx = (int)blockIdx.x % a.blocks_x, by = (int)blockIdx.x / a.blocks_x;
    const DnSlot sl = a.slots[blockIdx.y];
    const int seen = a.seen[sl.stream], cur = a.cur[sl.stream];
    const int xa = bx * DN_TW, cols = min(DN_TW, a.w - xa), ya = by * DN_TH, rows = min(DN_TH, a.h - ya);
    const int x0 = xa + lane * DN_RUN, npx = min(DN_RUN, a.w - x0);         // npx <= 0: the lane has no run
    const uint8_t *frame = (const uint8_t *)sl.src;
    const uint8_t *yp_in = a.yprev + (2LL * sl.stream + cur) * a.y_plane;
    uint8_t *yp_out = a.yprev + (2LL * sl.stream + (cur ^ 1)) * a.y_plane;

    // ---- the tile and its halo: LDS row r is frame row clamp(ya - 1 + r), LDS column c is frame column clamp(xa - 1 + c)
    for (int r = wave; r < rows + 2; r += DN_WAVES) {
        const int y = min(max(ya - 1 + r, 0), a.h - 1);
        const uint8_t *row = frame + (long long)y * a.spitch;
        const uint8_t *yrow = yp_in + (long long)y * a.y_pitch;
        if (npx > 0) {
            uint32_t px[DN_RUN];
            dn_load_run<WSRC>(row + 3LL * x0, npx, px);
            const uint32_t yp = *(const uint32_t *)(yrow + x0);             // (a row of the plane holds whole runs)
#pragma unroll
            for (int i = 0; i < DN_RUN; ++i)
                if (i < npx) {
                    const uint32_t yv = dn_luma_of(px[i]);
                    const int at = dn_lds_at(r, DN_RUN * lane + i + 1);
                    s_px[at] = px[i] | yv << 24;
                    s_dy[at] = (int16_t)((int)yv - (int)(yp >> (8 * i) & 255u));
                }
        }
        if (lane == 0 || lane == 63) {                      // the halo columns, byte by byte
            const int x = lane == 0 ? max(xa - 1, 0) : min(xa + cols, a.w - 1);
            const uint8_t *p = row + 3LL * x;
            const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16, yv = dn_luma_of(v);
            const int at = dn_lds_at(r, lane == 0 ? 0 : cols + 1);
            s_px[at] = v | yv << 24;
            s_dy[at] = (int16_t)((int)yv - (int)yrow[x]);
        }
    }
    __syncthreads();

    // ---- a lane's runs, row by row
    uint32_t n_static = 0, n_moving = 0, absdiff = 0;
    if (npx > 0) {
        for (int r = 1 + wave; r <= rows; r += DN_WAVES) {
            const int y = ya + r - 1;
            uint32_t px[3][DN_RUN + 2];
            int32_t dy[3][DN_RUN + 2];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < DN_RUN + 2; ++k) {
                    const int at = dn_lds_at(r - 1 + j, DN_RUN * lane + k);
                    px[j][k] = s_px[at]; dy[j][k] = s_dy[at];
                }
            const uint32_t row_bits = (y > 0 ? 0007u : 0u) | 0070u | (y + 1 < a.h ? 0700u : 0u);
            DnAccRun *ap = (DnAccRun *)(a.acc + (long long)sl.stream * a.acc_stream + (long long)y * a.acc_pitch + 6LL * x0);
            DnAccRun av = *ap;                              // (a row of acc holds whole runs)
            uint32_t out[DN_RUN], yout = 0;
#pragma unroll
            for (int i = 0; i < DN_RUN; ++i) {
                out[i] = 0;
                if (i < npx) {
                    const int x = x0 + i;
                    uint32_t nb[9], acc[3];
                    int32_t nd[9];
#pragma unroll
                    for (int q = 0; q < 9; ++q) { nb[q] = px[q / 3][i + q % 3]; nd[q] = dy[q / 3][i + q % 3]; }
                    const uint32_t inside = row_bits & ((x > 0 ? 0111u : 0u) | 0222u | (x + 1 < a.w ? 0444u : 0u));      // bit q = 3 * (dy + 1) + dx + 1
                    // channel k of pixel i is halfword 3 i + k of the run
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[k] = av.v[(3 * i + k) >> 1] >> (16 * ((3 * i + k) & 1)) & 0xffffu;
                    const DnPixel p = dn_pixel(a.rule, nb, nd, inside, seen, acc);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int hw = 3 * i + k;
                        av.v[hw >> 1] = (av.v[hw >> 1] & ~(0xffffu << (16 * (hw & 1)))) | acc[k] << (16 * (hw & 1));
                    }
                    out[i] = p.out & 0xffffffu;
                    yout |= (p.out >> 24) << (8 * i);
                    n_static += p.a == 0; n_moving += p.a == 256;
                    if (p.a == 0) absdiff += (uint32_t)(nd[4] < 0 ? -nd[4] : nd[4]);
                }
            }
            *ap = av;
            *(uint32_t *)(yp_out + (long long)y * a.y_pitch + x0) = yout;
            dn_store_run<WDST>((uint8_t *)sl.dst + (long long)y * a.dpitch + 3LL * x0, npx, out);
        }
    }
    n_static = wave_sum_u32(n_static); n_moving = wave_sum_u32(n_moving); absdiff = wave_sum_u32(absdiff);   // (a wave adds at most 2^20 to absdiff)
    if (lane == 0) { s_cnt[wave][0] = n_static; s_cnt[wave][1] = n_moving; s_cnt[wave][2] = absdiff; }
    __syncthreads();
    if (tid < 3) {
        uint32_t v = 0;
#pragma unroll
        for (int wv = 0; wv < DN_WAVES; ++wv) v += s_cnt[wv][tid];
        DnCount *c = a.cnt + blockIdx.y;
        if (v) {
            if (tid == 0) atomicAdd(&c->n_static, v);
            else if (tid == 1) atomicAdd(&c->n_moving, v);
            else atomicAdd(&c->absdiff, (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(DN_THREADS) void dn_finish(DnArgs a) {
    const int i = (int)(blockIdx.x * DN_THREADS + threadIdx.x);
    if (i >= a.n) return;
    const int stream = a.slots[i].stream, seen = dn_next_seen(a.seen[stream]);
    const DnCount c = a.cnt[i];
    a.seen[stream] = seen;
    a.cur[stream] ^= 1;
    a.res[i] = rtmodt_denoise_result{stream, seen, c.n_static, c.n_moving, c.absdiff};
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_denoise : HandleBase {
    rtmodt_denoise_cfg cfg{};
    DnRule rule{};
    int runs = 0, blocks_x = 0, blocks_y = 0;
    size_t acc_pitch = 0, acc_stream = 0, y_pitch = 0, y_plane = 0;
    EventTimer<2> timer;
    uint8_t *d_acc = nullptr, *d_y = nullptr;
    int32_t *d_seen = nullptr;                              // seen[S] | cur[S]
    char *d_work = nullptr;                                 // counters[S] | results[S]
    rtmodt_denoise_result *h_out = nullptr;
    CmdBuf cmd;                                             // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage sin, sout;                                   // host sources in, host destinations out
};

namespace {

DnRule dn_rule_of(const rtmodt_denoise_cfg &c) { return DnRule{c.motion_lo, c.motion_hi, c.temporal_shift, c.spatial, c.spatial_thr}; }

int dn_check_rule(const rtmodt_denoise_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null denoise config");
    RT_CHECK(c->motion_lo >= 0 && c->motion_lo <= DN_MAX_THRESHOLD, RTMODT_E_INVALID, "motion_lo %d outside 0..%d", c->motion_lo, DN_MAX_THRESHOLD);
    RT_CHECK(c->motion_hi >= 0 && c->motion_hi <= DN_MAX_THRESHOLD, RTMODT_E_INVALID, "motion_hi %d outside 0..%d", c->motion_hi, DN_MAX_THRESHOLD);
    RT_CHECK(c->motion_hi > c->motion_lo, RTMODT_E_INVALID, "motion_hi %d is not above motion_lo %d", c->motion_hi, c->motion_lo);
    RT_CHECK(c->temporal_shift >= 0 && c->temporal_shift <= DN_MAX_SHIFT, RTMODT_E_INVALID, "temporal_shift %d outside 0..%d", c->temporal_shift, DN_MAX_SHIFT);
    RT_CHECK(c->spatial >= 0 && c->spatial <= DN_MAX_SPATIAL, RTMODT_E_INVALID, "spatial %d outside 0..%d", c->spatial, DN_MAX_SPATIAL);
    RT_CHECK(c->spatial_thr >= 0 && c->spatial_thr <= 255, RTMODT_E_INVALID, "spatial_thr %d outside 0..255", c->spatial_thr);
    return RTMODT_OK;
}

int dn_check_cfg(const rtmodt_denoise_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null denoise config");
    RT_CHECK(c->streams >= 1 && c->streams <= DN_MAX_STREAMS, RTMODT_E_INVALID, "streams %d outside 1..%d", c->streams, DN_MAX_STREAMS);
    RT_CHECK(c->height >= 1 && c->height <= DN_MAX_DIM, RTMODT_E_INVALID, "height of %d pixels outside 1..%d", c->height, DN_MAX_DIM);
    RT_CHECK(c->width >= 1 && c->width <= DN_MAX_DIM, RTMODT_E_INVALID, "width of %d pixels outside 1..%d", c->width, DN_MAX_DIM);
    RT_TRY(dn_check_rule(c));
    RT_CHECK((long long)c->streams * c->height * c->width <= DN_MAX_PIXELS, RTMODT_E_CAPACITY, "%lld pixels over all streams (at most %lld)",
             (long long)c->streams * c->height * c->width, DN_MAX_PIXELS);
    return RTMODT_OK;
}

void (*const dn_filter_kernels[2][2])(DnArgs) = {{dn_filter<false, false>, dn_filter<false, true>}, {dn_filter<true, false>, dn_filter<true, true>}};

size_t dn_stream_values(const rtmodt_denoise *p) { return (size_t)p->cfg.height * p->cfg.width * 3; }

}  // namespace

extern "C" {

void rtmodt_denoise_default_cfg(rtmodt_denoise_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_denoise_cfg{};
    cfg->streams = 1; cfg->height = 0; cfg->width = 0;
    cfg->motion_lo = 18; cfg->motion_hi = 54; cfg->temporal_shift = 3; cfg->spatial = 256; cfg->spatial_thr = 6;
    cfg->device = 0;
}

void rtmodt_denoise_destroy(rtmodt_denoise *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_acc); hipFree(p->d_y); hipFree(p->d_seen); hipFree(p->d_work);
        hipHostFree(p->h_out);
        p->cmd.release(); p->sin.release(); p->sout.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_denoise_create(const rtmodt_denoise_cfg *cfg, rtmodt_denoise **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(dn_check_cfg(cfg));
    rtmodt_denoise *p = new rtmodt_denoise();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->rule = dn_rule_of(*cfg);
    const int h = cfg->height, w = cfg->width;
    p->runs = cdiv(w, DN_RUN);
    p->blocks_x = cdiv(w, DN_TW); p->blocks_y = cdiv(h, DN_TH);
    p->acc_pitch = (size_t)p->runs * sizeof(DnAccRun); p->acc_stream = p->acc_pitch * h;
    p->y_pitch = (size_t)p->runs * DN_RUN; p->y_plane = p->y_pitch * h;
    auto body = [&]() -> int {
        const size_t S = (size_t)cfg->streams;
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_acc, S * p->acc_stream));
        RT_HIP(hipMalloc((void **)&p->d_y, S * 2 * p->y_plane));
        RT_HIP(hipMalloc((void **)&p->d_seen, 2 * S * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_work, S * (sizeof(DnCount) + sizeof(rtmodt_denoise_result))));
        RT_HIP(hipHostMalloc((void **)&p->h_out, S * sizeof(rtmodt_denoise_result), hipHostMallocDefault));
        RT_HIP(handle_zero(p->d_acc, S * p->acc_stream, p->stream));
        RT_HIP(handle_zero(p->d_y, S * 2 * p->y_plane, p->stream));
        RT_HIP(handle_zero(p->d_seen, 2 * S * sizeof(int32_t), p->stream));
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_denoise_destroy, out);
}

int rtmodt_denoise_process(rtmodt_denoise *p, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                           int dst_mem_kind, const int32_t *streams, int n, int h, int w, rtmodt_denoise_result *results) {
    RT_CHECK(p && n >= 0 && (n == 0 || (src && dst)), RTMODT_E_INVALID, "null argument");
    p->timer.timed = false;
    const rtmodt_denoise_cfg &c = p->cfg;
    RT_CHECK(h == c.height && w == c.width, RTMODT_E_INVALID, "frames of %dx%d, the denoiser was created for %dx%d", w, h, c.width, c.height);
    RT_TRY(check_stream_list(src, streams, n, c.streams));
    if (n == 0) return RTMODT_OK;
    RT_TRY(check_frames(src, n, h, w, src_stride, src_mem_kind, kLensFrames));
    RT_TRY(check_frames((const uint8_t *const *)dst, n, h, w, dst_stride, dst_mem_kind, kLensFrames));
    RT_TRY(check_not_in_place(src, h, w, src_stride, dst, h, w, dst_stride, n));      // an output reads its neighbours' inputs: no in-place form

    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->sin.place(n, h, w, src_stride, src_mem_kind, FRAMES_TIGHT16));
    RT_TRY(p->sout.place(n, h, w, dst_stride, dst_mem_kind, FRAMES_TIGHT16));
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(DnSlot)));
    DnSlot *sl = (DnSlot *)p->cmd.h;
    bool wsrc = p->sin.pitch % 4 == 0, wdst = p->sout.pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        sl[i] = DnSlot{(uint64_t)(uintptr_t)p->sin.at(src, i), (uint64_t)(uintptr_t)p->sout.at(dst, i), streams ? streams[i] : i, 0};
        wsrc = wsrc && sl[i].src % 4 == 0;
        wdst = wdst && sl[i].dst % 4 == 0;
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(DnSlot), hipMemcpyHostToDevice, q));
    RT_TRY(p->sin.copy_in(src, q));

    DnArgs a{};
    a.slots = (const DnSlot *)p->cmd.d;
    a.spitch = (long long)p->sin.pitch; a.dpitch = (long long)p->sout.pitch;
    a.n = n; a.h = h; a.w = w; a.blocks_x = p->blocks_x;
    a.rule = p->rule;
    a.acc = p->d_acc; a.acc_pitch = (long long)p->acc_pitch; a.acc_stream = (long long)p->acc_stream;
    a.yprev = p->d_y; a.y_pitch = (long long)p->y_pitch; a.y_plane = (long long)p->y_plane;
    a.seen = p->d_seen; a.cur = p->d_seen + c.streams;
    a.cnt = (DnCount *)p->d_work;
    a.res = (rtmodt_denoise_result *)(p->d_work + (size_t)c.streams * sizeof(DnCount));

    RT_TRY(p->timer.record(0, q));
    RT_HIP(hipMemsetAsync(a.cnt, 0, (size_t)n * sizeof(DnCount), q));
    hipLaunchKernelGGL(dn_filter_kernels[wsrc][wdst], dim3((unsigned)(p->blocks_x * p->blocks_y), (unsigned)n), dim3(DN_THREADS), 0, q, a);
    hipLaunchKernelGGL(dn_finish, dim3((unsigned)cdiv(n, DN_THREADS)), dim3(DN_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_TRY(p->sout.copy_out(dst, q));
    if (results) RT_HIP(hipMemcpyAsync(p->h_out, a.res, (size_t)n * sizeof(rtmodt_denoise_result), hipMemcpyDeviceToHost, q));      // every result in one copy
    RT_HIP(hipStreamSynchronize(q));
    if (results) memcpy(results, p->h_out, (size_t)n * sizeof(rtmodt_denoise_result));
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_denoise_read_state(rtmodt_denoise *p, int stream, uint16_t *acc, int32_t *frames_seen) {
    RT_CHECK(p && acc && frames_seen, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    const size_t row = (size_t)p->cfg.width * 6;
    RT_HIP(hipMemcpy2DAsync(acc, row, p->d_acc + (size_t)stream * p->acc_stream, p->acc_pitch, row, (size_t)p->cfg.height, hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(frames_seen, p->d_seen + stream, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_denoise_load_state(rtmodt_denoise *p, int stream, const uint16_t *acc, int64_t n_values, int32_t frames_seen) {
    RT_CHECK(p && acc, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    const int h = p->cfg.height, w = p->cfg.width;
    RT_CHECK(n_values == (int64_t)dn_stream_values(p), RTMODT_E_INVALID, "state of %lld values, this denoiser holds %dx%dx3 per stream", (long long)n_values, h, w);
    RT_CHECK(frames_seen >= 0 && frames_seen <= DN_MAX_SEEN, RTMODT_E_INVALID, "state: frames_seen %d outside 0..2^30", frames_seen);
    for (int64_t i = 0; i < n_values; ++i) RT_CHECK(acc[i] <= DN_MAX_ACC, RTMODT_E_INVALID, "state: value %lld is %u, above 255 << 8", (long long)i, (unsigned)acc[i]);
    // the plane of Y(prev) follows from acc; both planes take it, whichever is current
    std::vector<uint8_t> plane(p->y_plane, 0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint16_t *v = acc + ((size_t)y * w + x) * 3;
            plane[(size_t)y * p->y_pitch + x] = (uint8_t)dn_luma_of(dn_prev_px(v[0], v[1], v[2]));
        }
    RT_HIP(hipSetDevice(p->device));
    const size_t row = (size_t)w * 6;
    RT_HIP(hipMemcpy2DAsync(p->d_acc + (size_t)stream * p->acc_stream, p->acc_pitch, acc, row, row, (size_t)h, hipMemcpyHostToDevice, p->stream));
    for (int k = 0; k < 2; ++k) RT_HIP(hipMemcpyAsync(p->d_y + ((size_t)2 * stream + k) * p->y_plane, plane.data(), p->y_plane, hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_seen + stream, &frames_seen, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));                // (the plane is a local of this function)
    return RTMODT_OK;
}

int rtmodt_denoise_reset(rtmodt_denoise *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    const size_t first = stream < 0 ? 0 : (size_t)stream, count = stream < 0 ? (size_t)p->cfg.streams : 1;
    RT_HIP(handle_zero(p->d_acc + first * p->acc_stream, count * p->acc_stream, p->stream));
    RT_HIP(handle_zero(p->d_seen + first, count * sizeof(int32_t), p->stream));       // (the first frame reads no Y(prev): the planes stay)
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_denoise_last_ms(rtmodt_denoise *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

int rtmodt_denoise_pixel(const rtmodt_denoise_cfg *cfg, const uint8_t *cur, const uint16_t *acc, uint32_t inside, int32_t frames_seen, uint8_t *out,
                         uint16_t *acc_out, int32_t *a, int32_t *d) {
    RT_CHECK(cur && acc && out && acc_out, RTMODT_E_INVALID, "null argument");
    RT_TRY(dn_check_rule(cfg));
    RT_CHECK(frames_seen >= 0 && frames_seen <= DN_MAX_SEEN, RTMODT_E_INVALID, "frames_seen %d outside 0..2^30", frames_seen);
    RT_CHECK(inside < 512u && (inside & 16u), RTMODT_E_INVALID, "inside %u: nine bits, the centre's (16) set", inside);
    uint32_t px[9], mine[3];
    int32_t dy[9];
    for (int q = 0; q < 9; ++q) {
        RT_CHECK(acc[3 * q] <= DN_MAX_ACC && acc[3 * q + 1] <= DN_MAX_ACC && acc[3 * q + 2] <= DN_MAX_ACC, RTMODT_E_INVALID, "acc of neighbour %d above 255 << 8", q);
        const uint32_t v = (uint32_t)cur[3 * q] | (uint32_t)cur[3 * q + 1] << 8 | (uint32_t)cur[3 * q + 2] << 16, yv = dn_luma_of(v);
        px[q] = v | yv << 24;
        dy[q] = (int32_t)yv - (int32_t)dn_luma_of(dn_prev_px(acc[3 * q], acc[3 * q + 1], acc[3 * q + 2]));
    }
    for (int k = 0; k < 3; ++k) mine[k] = acc[12 + k];
    const DnPixel r = dn_pixel(dn_rule_of(*cfg), px, dy, inside, frames_seen, mine);
    for (int k = 0; k < 3; ++k) { out[k] = (uint8_t)(r.out >> (8 * k)); acc_out[k] = (uint16_t)mine[k]; }
    if (a) *a = r.a;
    if (d) *d = r.D;
    return RTMODT_OK;
}

}  // extern "C"
