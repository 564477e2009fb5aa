// stab.hip -- the stabiliser: frames of a camera that shakes on its mount are steadied once, directly after decode / undistort, so that
// every fixed-camera stage (motion gate, left objects, speed, heatmap, zones, tripwires, privacy polygons) sees a steady picture.  The
// reference has no counterpart (src/ingestion/rtsp_reader.py hands cap.read()'s frame to the detector; cv2.estimateAffinePartial2D /
// warpAffine appear nowhere in it); PARITY UNPINNED against vidstab / OpenCV's videostab / warpAffine.  csrc/stab_rule.h states every
// rule and tests/stab_ref.py restates it: path (as bit patterns), status, HOLD run, coefficients and output bytes are equal.
//
// State on the device: 80 bytes per stream (StDev): the path J as four doubles, the four Q16 coefficients of the last call, the HOLD
// run and the status.  Two launches per call for all its frames, whatever the warps are:
//   stab_step   one lane per frame of the call: reads six floats and a status word (0: valid) from the call's command block or from
//               the estimator's device buffers (gmc.hip: gmc_enqueue_frames; ordered behind the estimate by an event, no host wait),
//               runs stab_rule.h rules 1 to 6 in float64 (FMA contraction off) and writes the stream's StDev.
//   stab_warp   256 threads, frame index in gridDim.y; a workgroup makes a tile of 256 output pixels x 4 rows, a thread a run of 4
//               pixels of one row: its stream's coefficients from StDev, X and Y of the first pixel in int64 (the next pixel is X + A,
//               Y + B), per pixel the four taps of three channels as byte loads at the caller's pitch and lens_model.h's integer
//               blend (lens_sample itself: the header is compiled for the device here); a pixel whose four taps are all on the source
//               loads its twelve bytes up front.  No floats, no atomics, no LDS, no table.  WIDE (every destination base and the
//               pitch a multiple of 4): a full run is one 12-byte store; else, and for the partial run at a row's end, byte by byte.
//               Bytes beyond 3 w of a row are never touched.  At the angles this is for, neighbouring lanes read neighbouring bytes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "frame_stage.h"
#include "handle_host.h"
#include "kernels.h"

// the rule headers are plain C++; here their functions are compiled for the host and the device alike
#pragma clang force_cuda_host_device begin
#include "lens_model.h"
#include "stab_rule.h"
#pragma clang force_cuda_host_device end

namespace rtmodt {

constexpr int ST_THREADS = 256, ST_RUN = 4, ST_ROWS = ST_THREADS / 64, ST_MAX_STREAMS = 1024;

struct StDev { double j[4]; int64_t c[4]; int32_t hold, status; int32_t pad[2]; };
struct StSlot { uint64_t src, dst; int32_t stream; int32_t pad[3]; };
static_assert(sizeof(StDev) == 80 && sizeof(StSlot) == 32, "layout");

struct StStepArgs {
    const StSlot *slots; int n;
    const float *warp;            // [n][6]; null: the identity
    const int32_t *invalid;       // [n], 0: valid (gmc's status); null: all valid
    StDev *state;
    StabRule rule;
};

struct StWarpArgs {
    const StSlot *slots; const StDev *state;
    long long spitch, dpitch;
    int h, w, tiles_x;
    uint32_t border;              // b | g << 8 | r << 16
};

struct __attribute__((aligned(4))) StRun { uint32_t a, b, c; };

__global__ __launch_bounds__(64) void stab_step_kernel(StStepArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    StDev *st = a.state + a.slots[i].stream;               // (the host checked the stream against the handle)
    StabPath j{st->j[0], st->j[1], st->j[2], st->j[3]};
    int32_t hold = st->hold;
    float W[6];
    if (a.warp)
        for (int k = 0; k < 6; ++k) W[k] = a.warp[6 * i + k];
    const bool valid = !a.invalid || a.invalid[i] == 0;
    const int status = stab_step(a.rule, j, hold, a.warp ? W : nullptr, valid);
    const StabCoef c = stab_quantise(a.rule, j);
    st->j[0] = j.za; st->j[1] = j.zb; st->j[2] = j.tx; st->j[3] = j.ty;
    st->c[0] = c.A; st->c[1] = c.B; st->c[2] = c.U; st->c[3] = c.V;
    st->hold = hold; st->status = status;
}

// one output pixel as b | g << 8 | r << 16
__device__ __forceinline__ uint32_t st_pixel(const uint8_t *src, long long spitch, int W, int H, int32_t qx, int32_t qy, uint32_t border) {
    const int x0 = qx >> LENS_BITS, y0 = qy >> LENS_BITS;
    uint32_t out = 0;
    if (x0 >= 0 && x0 + 1 < W && y0 >= 0 && y0 + 1 < H) {
        const uint8_t *p = src + (long long)y0 * spitch + 3LL * x0, *q = p + spitch;
        int t[12];                                          // every load is issued before the first is used
#pragma unroll
        for (int k = 0; k < 6; ++k) { t[k] = p[k]; t[6 + k] = q[k]; }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out |= (uint32_t)lens_sample(qx, qy, H, W, 0, [&](int x, int y) { return t[6 * (y - y0) + 3 * (x - x0) + c]; }) << (8 * c);
        return out;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out |= (uint32_t)lens_sample(qx, qy, H, W, (int)((border >> (8 * c)) & 255u), [&](int x, int y) { return (int)src[(long long)y * spitch + 3LL * x + c]; })
               << (8 * c);
    return out;
}

template <bool WIDE> __global__ __launch_bounds__(ST_THREADS) void stab_warp_kernel(StWarpArgs a) {
    const int tid = threadIdx.x;
    const int row = (int)(blockIdx.x / a.tiles_x) * ST_ROWS + (tid >> 6);
    const int u0 = ((int)(blockIdx.x % a.tiles_x) * 64 + (tid & 63)) * ST_RUN;
    if (row >= a.h || u0 >= a.w) return;
    const StSlot sl = a.slots[blockIdx.y];
    const StDev *st = a.state + sl.stream;
    const StabCoef c{st->c[0], st->c[1], st->c[2], st->c[3]};
    const uint8_t *src = (const uint8_t *)sl.src;
    int64_t X, Y;
    stab_xy(c, u0, row, X, Y);
    uint32_t px[ST_RUN];
#pragma unroll
    for (int i = 0; i < ST_RUN; ++i) {
        px[i] = st_pixel(src, a.spitch, a.w, a.h, stab_q5(X), stab_q5(Y), a.border);
        X += c.A; Y += c.B;
    }
    uint8_t *d = (uint8_t *)sl.dst + (long long)row * a.dpitch + 3LL * u0;
    const int npx = min(ST_RUN, a.w - u0);
    if (WIDE && npx == ST_RUN) {
        StRun r;
        r.a = px[0] | px[1] << 24; r.b = px[1] >> 8 | px[2] << 16; r.c = px[2] >> 16 | px[3] << 8;
        *(StRun *)d = r;                                    // base, pitch and 3 * u0 (a multiple of 12) are multiples of 4
        return;
    }
#pragma unroll
    for (int i = 0; i < ST_RUN; ++i)
        if (i < npx) {
            d[3 * i] = (uint8_t)px[i]; d[3 * i + 1] = (uint8_t)(px[i] >> 8); d[3 * i + 2] = (uint8_t)(px[i] >> 16);
        }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_stab : HandleBase {
    rtmodt_stab_cfg cfg{};
    StabRule rule{};
    EventTimer<2> timer;
    StDev *d_state = nullptr;
    std::vector<StDev> h_state;         // staging for reset / result
    std::vector<char> seen;
    CmdBuf cmd;                         // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage sin, sout;               // host sources in, host destinations out
};

namespace {

StabRule st_rule(const rtmodt_stab_cfg &c) {
    return StabRule{c.h, c.w, c.leak_shift, c.max_shift_px, c.max_rot_milli, c.max_zoom_milli, c.crop_zoom_milli, c.reset_after};
}

int st_check_rule(const rtmodt_stab_cfg *cfg, StabRule &r) {
    RT_CHECK(cfg, RTMODT_E_INVALID, "null argument");
    r = st_rule(*cfg);
    RT_CHECK(r.h >= 1 && r.w >= 1 && r.h <= STAB_MAX_DIM && r.w <= STAB_MAX_DIM, RTMODT_E_INVALID, "frame size %dx%d outside 1..%d", r.w, r.h, STAB_MAX_DIM);
    RT_CHECK(stab_rule_ok(r), RTMODT_E_INVALID,
             "bad parameter (leak_shift %d in 0..%d, max_shift_px %d in 0..%d, max_rot_milli %d and max_zoom_milli %d in 0..%d, crop_zoom_milli %d in 1000..%d, "
             "reset_after %d in 0..2^30)", r.leak_shift, STAB_MAX_LEAK, r.max_shift_px, STAB_MAX_SHIFT, r.max_rot_milli, r.max_zoom_milli, STAB_MAX_MILLI,
             r.crop_zoom_milli, STAB_MAX_CROP, r.reset_after);
    return RTMODT_OK;
}

int st_check_stream(const rtmodt_stab *p, int stream) {
    RT_CHECK(stream >= 0 && stream < p->cfg.streams, RTMODT_E_INVALID, "stream %d outside 0..%d", stream, p->cfg.streams - 1);
    return RTMODT_OK;
}

StDev st_fresh(const StabRule &r) {
    StDev d{};
    const StabPath j{1.0, 0.0, 0.0, 0.0};
    const StabCoef c = stab_quantise(r, j);
    d.j[0] = 1.0;
    d.c[0] = c.A; d.c[1] = c.B; d.c[2] = c.U; d.c[3] = c.V;
    d.status = STAB_OK;
    return d;
}

int st_fetch(rtmodt_stab *p, int first, int count) {
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->h_state.data() + first, p->d_state + first, (size_t)count * sizeof(StDev), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int st_store(rtmodt_stab *p, int first, int count) {
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_state + first, p->h_state.data() + first, (size_t)count * sizeof(StDev), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

// everything a call is refused for, then the two launches; gmc == nullptr: the warps are the caller's
int st_process(rtmodt_stab *p, rtmodt_gmc *gmc, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride, int dst_mem_kind,
               const int32_t *streams, int n, const float *warps, const uint8_t *valid, const float *mask_xyxy, const float *mask_conf, const int32_t *mask_n) {
    RT_CHECK(p && n >= 0 && (n == 0 || (src && dst)), RTMODT_E_INVALID, "null argument");
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    const rtmodt_stab_cfg &c = p->cfg;
    RT_CHECK(n <= c.streams, RTMODT_E_CAPACITY, "%d frames in one call for %d streams", n, c.streams);
    RT_TRY(check_frames(src, n, c.h, c.w, src_stride, src_mem_kind, kLensFrames));
    RT_TRY(check_frames((const uint8_t *const *)dst, n, c.h, c.w, dst_stride, dst_mem_kind, kLensFrames));
    p->seen.assign(c.streams, 0);
    for (int i = 0; i < n; ++i) {
        const int s = streams ? streams[i] : i;
        RT_TRY(st_check_stream(p, s));
        RT_CHECK(!p->seen[s], RTMODT_E_INVALID, "stream %d is named twice in one call", s);
        p->seen[s] = 1;
    }
    RT_TRY(check_not_in_place(src, c.h, c.w, src_stride, dst, c.h, c.w, dst_stride, n));
    if (!gmc && warps)
        for (int i = 0; i < n; ++i)
            RT_CHECK((valid && !valid[i]) || stab_input_ok(warps + 6 * i), RTMODT_E_INVALID, "warp %d is not finite or has |det| < 1e-6", i);
    if (gmc)
        RT_TRY(gmc_enqueue_frames(gmc, p->device, src, n, c.h, c.w, src_stride, src_mem_kind, mask_xyxy, mask_conf, mask_n, true, nullptr, nullptr, nullptr));

    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->sin.place(n, c.h, c.w, src_stride, src_mem_kind, FRAMES_TIGHT16));
    RT_TRY(p->sout.place(n, c.h, c.w, dst_stride, dst_mem_kind, FRAMES_TIGHT16));
    // the command block: slots | warps | invalid
    const size_t o_warp = (size_t)n * sizeof(StSlot), o_inv = o_warp + (size_t)n * 24, bytes = o_inv + (size_t)n * 4;
    RT_TRY(p->cmd.reserve(bytes));
    StSlot *sl = (StSlot *)p->cmd.h;
    float *hw = (float *)(p->cmd.h + o_warp);
    int32_t *hi = (int32_t *)(p->cmd.h + o_inv);
    bool wide = p->sout.pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        sl[i] = StSlot{(uint64_t)(uintptr_t)p->sin.at(src, i), (uint64_t)(uintptr_t)p->sout.at(dst, i), streams ? streams[i] : i, {0, 0, 0}};
        wide = wide && sl[i].dst % 4 == 0;
        const float id[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        memcpy(hw + 6 * i, !gmc && warps ? warps + 6 * i : id, 24);
        hi[i] = valid && !valid[i] ? 1 : 0;
    }
    StStepArgs sa{};
    sa.slots = (const StSlot *)p->cmd.d; sa.n = n; sa.state = p->d_state; sa.rule = p->rule;
    sa.warp = (const float *)(p->cmd.d + o_warp); sa.invalid = (const int32_t *)(p->cmd.d + o_inv);
    if (gmc) {
        hipEvent_t done = nullptr;
        RT_TRY(gmc_enqueue_frames(gmc, p->device, src, n, c.h, c.w, src_stride, src_mem_kind, mask_xyxy, mask_conf, mask_n, false, &sa.warp, &sa.invalid, &done));
        RT_HIP(hipStreamWaitEvent(q, done, 0));             // the step is ordered behind the estimate on the device; the host does not wait
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, bytes, hipMemcpyHostToDevice, q));
    RT_TRY(p->sin.copy_in(src, q));

    StWarpArgs wa{};
    wa.slots = sa.slots; wa.state = p->d_state;
    wa.spitch = (long long)p->sin.pitch; wa.dpitch = (long long)p->sout.pitch;
    wa.h = c.h; wa.w = c.w; wa.tiles_x = cdiv(c.w, 64 * ST_RUN);
    wa.border = (uint32_t)c.border_bgr[0] | (uint32_t)c.border_bgr[1] << 8 | (uint32_t)c.border_bgr[2] << 16;
    const dim3 grid((unsigned)(wa.tiles_x * cdiv(c.h, ST_ROWS)), (unsigned)n), block(ST_THREADS);
    RT_TRY(p->timer.record(0, q));
    hipLaunchKernelGGL(stab_step_kernel, dim3(cdiv(n, 64)), dim3(64), 0, q, sa);
    if (wide) hipLaunchKernelGGL(stab_warp_kernel<true>, grid, block, 0, q, wa);
    else hipLaunchKernelGGL(stab_warp_kernel<false>, grid, block, 0, q, wa);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_TRY(p->sout.copy_out(dst, q));
    RT_HIP(hipStreamSynchronize(q));
    p->timer.timed = true;
    return RTMODT_OK;
}

}  // namespace

extern "C" {

void rtmodt_stab_default_cfg(rtmodt_stab_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_stab_cfg{};
    cfg->streams = 1;
    cfg->leak_shift = 6; cfg->max_shift_px = 32; cfg->max_rot_milli = 35; cfg->max_zoom_milli = 50; cfg->crop_zoom_milli = 1000; cfg->reset_after = 30;
}

void rtmodt_stab_destroy(rtmodt_stab *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_state);
        p->cmd.release(); p->sin.release(); p->sout.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_stab_create(const rtmodt_stab_cfg *cfg, rtmodt_stab **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(cfg->streams >= 1 && cfg->streams <= ST_MAX_STREAMS, RTMODT_E_INVALID, "streams %d outside 1..%d", cfg->streams, ST_MAX_STREAMS);
    StabRule r;
    RT_TRY(st_check_rule(cfg, r));
    rtmodt_stab *p = new rtmodt_stab();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->rule = r;
    p->h_state.assign(cfg->streams, st_fresh(r));
    auto body = [&]() -> int {
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_state, (size_t)cfg->streams * sizeof(StDev)));
        return st_store(p, 0, cfg->streams);
    };
    return handle_created(body(), p, rtmodt_stab_destroy, out);
}

int rtmodt_stab_reset(rtmodt_stab *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream >= 0) RT_TRY(st_check_stream(p, stream));
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? p->cfg.streams : 1;
    for (int s = first; s < first + count; ++s) p->h_state[s] = st_fresh(p->rule);
    return st_store(p, first, count);
}

int rtmodt_stab_process(rtmodt_stab *p, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride, int dst_mem_kind,
                        const int32_t *streams, int n, const float *warps, const uint8_t *valid) {
    return st_process(p, nullptr, src, src_stride, src_mem_kind, dst, dst_stride, dst_mem_kind, streams, n, warps, valid, nullptr, nullptr, nullptr);
}

int rtmodt_stab_process_gmc(rtmodt_stab *p, rtmodt_gmc *gmc, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                            int dst_mem_kind, const int32_t *streams, int n, const float *mask_xyxy, const float *mask_conf, const int32_t *mask_n) {
    RT_CHECK(p && gmc, RTMODT_E_INVALID, "null argument");
    return st_process(p, gmc, src, src_stride, src_mem_kind, dst, dst_stride, dst_mem_kind, streams, n, nullptr, nullptr, mask_xyxy, mask_conf, mask_n);
}

int rtmodt_stab_result(rtmodt_stab *p, rtmodt_stab_stream_result *out) {
    RT_CHECK(p && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(st_fetch(p, 0, p->cfg.streams));
    for (int s = 0; s < p->cfg.streams; ++s) {
        const StDev &d = p->h_state[s];
        out[s].status = d.status; out[s].hold = d.hold;
        memcpy(out[s].j, d.j, sizeof(d.j));
        memcpy(out[s].coef, d.c, sizeof(d.c));
    }
    return RTMODT_OK;
}

int rtmodt_stab_state(rtmodt_stab *p, int stream, double *j, int32_t *hold) {
    RT_CHECK(p && j && hold, RTMODT_E_INVALID, "null argument");
    RT_TRY(st_check_stream(p, stream));
    RT_TRY(st_fetch(p, stream, 1));
    memcpy(j, p->h_state[stream].j, 4 * sizeof(double));
    *hold = p->h_state[stream].hold;
    return RTMODT_OK;
}

int rtmodt_stab_load_state(rtmodt_stab *p, int stream, const double *j, int32_t hold) {
    RT_CHECK(p && j, RTMODT_E_INVALID, "null argument");
    RT_TRY(st_check_stream(p, stream));
    const StabPath path{j[0], j[1], j[2], j[3]};
    RT_CHECK(stab_path_ok(p->rule, path), RTMODT_E_INVALID, "path (%g, %g, %g, %g) outside the handle's limits", j[0], j[1], j[2], j[3]);
    RT_CHECK(hold >= 0 && hold <= STAB_MAX_HOLD, RTMODT_E_INVALID, "hold run %d outside 0..2^30", hold);
    StDev d{};
    const StabCoef c = stab_quantise(p->rule, path);
    memcpy(d.j, j, sizeof(d.j));
    d.c[0] = c.A; d.c[1] = c.B; d.c[2] = c.U; d.c[3] = c.V;
    d.hold = hold; d.status = STAB_OK;
    p->h_state[stream] = d;
    return st_store(p, stream, 1);
}

int rtmodt_stab_last_ms(rtmodt_stab *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

int rtmodt_stab_points(const rtmodt_stab_cfg *cfg, const double *j, int to_source, const double *xy, int n, double *out_xy) {
    StabRule r;
    RT_TRY(st_check_rule(cfg, r));
    RT_CHECK(j && n >= 0 && (n == 0 || (xy && out_xy)), RTMODT_E_INVALID, "null argument");
    const StabPath path{j[0], j[1], j[2], j[3]};
    for (int i = 0; i < n; ++i) stab_point(r, path, to_source != 0, xy[2 * i], xy[2 * i + 1], out_xy[2 * i], out_xy[2 * i + 1]);
    return RTMODT_OK;
}

int rtmodt_stab_step(const rtmodt_stab_cfg *cfg, double *j, int32_t *hold, const float *warp, int valid, int32_t *status, int64_t *coef) {
    StabRule r;
    RT_TRY(st_check_rule(cfg, r));
    RT_CHECK(j && hold, RTMODT_E_INVALID, "null argument");
    StabPath path{j[0], j[1], j[2], j[3]};
    const int st = stab_step(r, path, *hold, warp, valid != 0);
    const StabCoef c = stab_quantise(r, path);
    j[0] = path.za; j[1] = path.zb; j[2] = path.tx; j[3] = path.ty;
    if (status) *status = st;
    if (coef) { coef[0] = c.A; coef[1] = c.B; coef[2] = c.U; coef[3] = c.V; }
    return RTMODT_OK;
}

}  // extern "C"
