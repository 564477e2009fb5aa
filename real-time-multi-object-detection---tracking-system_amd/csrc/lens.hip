// lens.hip -- lens correction on the GPU: frames are undistorted once, directly after decode, so that every later stage (detector,
// motion, trackers, zones, speed, privacy, heatmap, render, JPEG) runs in the rectified pixel coordinates it assumes.  The reference
// has no counterpart (src/ingestion/rtsp_reader.py hands cap.read()'s frame straight to the detector; cv2.undistort appears nowhere
// in it); PARITY UNPINNED against cv2.undistort / initUndistortRectifyMap / remap.  csrc/lens_model.h states every rule; the host
// builds one table per lens at set_model / set_map time with it, and tests/lens_ref.py restates it: table and output bytes are equal.
//
// Table on the device: 8 bytes per output pixel, int2 (qx, qy) with 5 fractional bits; an OUTSIDE pixel is (INT32_MIN, 0) (a position
// is inside (-2^20, 2^20), so |qx| <= 2^25 and the sentinel cannot be a position).  A table row holds align_up(out_w, 4) entries, the
// pad entries OUTSIDE, so that every thread reads its four entries as two 16-byte loads.
//
// Kernel lens_remap (256 threads, ONE launch per call for all its frames, frame index in gridDim.y; no atomics, no floats, no LDS):
//   a workgroup makes a tile of 256 output pixels x 4 rows; a thread makes a run of 4 pixels of one row: two 16-byte table loads, per
//   pixel the four taps of three channels as byte loads at the caller's pitch (any base address, any pitch; taps off the source read
//   the border colour; a pixel whose four taps are all on the source takes a path without the per-tap tests), the integer blend of
//   lens_model.h rule 3, and 12 output bytes.  WIDE (every destination base and the pitch a multiple of 4): a full run is one
//   12-byte store; else, and for the partial run at a row's end, byte by byte.  Bytes beyond 3 out_w of a row are never touched.
//   Lanes are adjacent runs: a wave reads 2 KiB of contiguous table and writes 768 contiguous bytes per row.
#include <algorithm>
#include <cstring>
#include <vector>

#include "frame_stage.h"
#include "handle_host.h"
#include "lens_model.h"

namespace rtmodt {

constexpr int LN_THREADS = 256, LN_RUN = 4, LN_ROWS = LN_THREADS / 64, LN_MAX_STREAMS = 1024;
constexpr int32_t LN_OUTSIDE = INT32_MIN;

struct LnSlot { uint64_t src, dst, table, pad; };
static_assert(sizeof(LnSlot) == 32, "layout");
static_assert(sizeof(LensModel) == sizeof(rtmodt_lens_params) && sizeof(LensModel) == 17 * sizeof(double), "layout");

struct LnArgs {
    const LnSlot *slots;
    long long spitch, dpitch;
    int src_h, src_w, out_h, out_w, tpitch, tiles_x;     // tpitch: entries per table row
    uint32_t border;                                     // b | g << 8 | r << 16
};

struct __attribute__((aligned(4))) LnRun { uint32_t a, b, c; };

// one output pixel as b | g << 8 | r << 16
__device__ __forceinline__ uint32_t ln_pixel(const uint8_t *src, long long spitch, int W, int H, int32_t qx, int32_t qy, uint32_t border) {
    if (qx == LN_OUTSIDE) return border;
    const int x0 = qx >> LENS_BITS, y0 = qy >> LENS_BITS, ax = qx & (LENS_ONE - 1), ay = qy & (LENS_ONE - 1);
    const int w00 = (LENS_ONE - ax) * (LENS_ONE - ay), w10 = ax * (LENS_ONE - ay), w01 = (LENS_ONE - ax) * ay, w11 = ax * ay;
    uint32_t out = 0;
    if (x0 >= 0 && x0 + 1 < W && y0 >= 0 && y0 + 1 < H) {
        const uint8_t *p = src + (long long)y0 * spitch + 3LL * x0, *q = p + spitch;
        uint32_t t[12];                                     // every load is issued before the first is used
#pragma unroll
        for (int k = 0; k < 6; ++k) { t[k] = p[k]; t[6 + k] = q[k]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t sum = w00 * t[c] + w10 * t[3 + c] + w01 * t[6 + c] + w11 * t[9 + c];
            out |= ((sum + 512u) >> 10) << (8 * c);
        }
        return out;
    }
    const bool xin0 = x0 >= 0 && x0 < W, xin1 = x0 + 1 >= 0 && x0 + 1 < W, yin0 = y0 >= 0 && y0 < H, yin1 = y0 + 1 >= 0 && y0 + 1 < H;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t bc = (border >> (8 * c)) & 255u;
        const uint32_t t00 = xin0 && yin0 ? src[(long long)y0 * spitch + 3LL * x0 + c] : bc;
        const uint32_t t10 = xin1 && yin0 ? src[(long long)y0 * spitch + 3LL * (x0 + 1) + c] : bc;
        const uint32_t t01 = xin0 && yin1 ? src[(long long)(y0 + 1) * spitch + 3LL * x0 + c] : bc;
        const uint32_t t11 = xin1 && yin1 ? src[(long long)(y0 + 1) * spitch + 3LL * (x0 + 1) + c] : bc;
        const uint32_t sum = w00 * t00 + w10 * t10 + w01 * t01 + w11 * t11;
        out |= ((sum + 512u) >> 10) << (8 * c);
    }
    return out;
}

template <bool WIDE> __global__ __launch_bounds__(LN_THREADS) void lens_remap(LnArgs a) {
    const int tid = threadIdx.x;
    const int row = (int)(blockIdx.x / a.tiles_x) * LN_ROWS + (tid >> 6);
    const int u0 = ((int)(blockIdx.x % a.tiles_x) * 64 + (tid & 63)) * LN_RUN;
    if (row >= a.out_h || u0 >= a.out_w) return;
    const LnSlot sl = a.slots[blockIdx.y];
    const int4 *e = (const int4 *)((const int2 *)sl.table + (size_t)row * a.tpitch + u0);       // u0 and tpitch are multiples of 4: 32-byte aligned
    const int4 e01 = e[0], e23 = e[1];
    const uint8_t *src = (const uint8_t *)sl.src;
    const uint32_t p0 = ln_pixel(src, a.spitch, a.src_w, a.src_h, e01.x, e01.y, a.border);
    const uint32_t p1 = ln_pixel(src, a.spitch, a.src_w, a.src_h, e01.z, e01.w, a.border);
    const uint32_t p2 = ln_pixel(src, a.spitch, a.src_w, a.src_h, e23.x, e23.y, a.border);
    const uint32_t p3 = ln_pixel(src, a.spitch, a.src_w, a.src_h, e23.z, e23.w, a.border);
    uint8_t *d = (uint8_t *)sl.dst + (long long)row * a.dpitch + 3LL * u0;
    const int npx = min(LN_RUN, a.out_w - u0);
    if (WIDE && npx == LN_RUN) {
        LnRun r;
        r.a = p0 | p1 << 24; r.b = p1 >> 8 | p2 << 16; r.c = p2 >> 16 | p3 << 8;
        *(LnRun *)d = r;                                    // base, pitch and 3 * u0 (a multiple of 12) are multiples of 4
        return;
    }
    const uint32_t px[LN_RUN] = {p0, p1, p2, p3};
#pragma unroll
    for (int i = 0; i < LN_RUN; ++i)
        if (i < npx) {
            d[3 * i] = (uint8_t)px[i]; d[3 * i + 1] = (uint8_t)(px[i] >> 8); d[3 * i + 2] = (uint8_t)(px[i] >> 16);
        }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_lens : HandleBase {
    rtmodt_lens_cfg cfg{};
    int tpitch = 0;
    size_t entries = 0;                 // per stream: out_h * tpitch
    EventTimer<2> timer;
    int2 *d_table = nullptr;
    std::vector<char> has;              // a lens was set
    CmdBuf cmd;                         // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage sin, sout;               // host sources in, host destinations out
    std::vector<int32_t> qx, qy;        // the canonical table of the lens being set or read
    std::vector<uint8_t> outside;
    std::vector<int2> packed;
};

namespace {

LensModel ln_model(const rtmodt_lens_params &p) {
    LensModel m;
    memcpy(&m, &p, sizeof(m));
    return m;
}

int ln_check_params(const rtmodt_lens_params *params, LensModel &m) {
    RT_CHECK(params, RTMODT_E_INVALID, "null lens parameters");
    m = lens_resolve(ln_model(*params));
    RT_CHECK(lens_model_ok(m), RTMODT_E_INVALID, "focal lengths fx %g fy %g nfx %g nfy %g: each must be finite and > 0", m.fx, m.fy, m.nfx, m.nfy);
    return RTMODT_OK;
}

int ln_check_size(int src_h, int src_w, int out_h, int out_w) {
    RT_CHECK(src_h >= 1 && src_w >= 1 && src_h <= LENS_MAX_DIM && src_w <= LENS_MAX_DIM, RTMODT_E_INVALID, "source size %dx%d outside 1..%d", src_w, src_h,
             LENS_MAX_DIM);
    RT_CHECK(out_h >= 1 && out_w >= 1 && out_h <= LENS_MAX_DIM && out_w <= LENS_MAX_DIM, RTMODT_E_INVALID, "output size %dx%d outside 1..%d", out_w, out_h,
             LENS_MAX_DIM);
    return RTMODT_OK;
}

int ln_check_stream(const rtmodt_lens *p, int stream) {
    RT_CHECK(stream >= 0 && stream < p->cfg.streams, RTMODT_E_INVALID, "stream %d outside 0..%d", stream, p->cfg.streams - 1);
    return RTMODT_OK;
}

// the canonical table in p->qx / qy / outside -> the device table of `stream`
int ln_upload(rtmodt_lens *p, int stream, long long n_out, int32_t *n_outside) {
    const int oh = p->cfg.out_h, ow = p->cfg.out_w;
    p->packed.assign(p->entries, make_int2(LN_OUTSIDE, 0));
    for (int v = 0; v < oh; ++v)
        for (int u = 0; u < ow; ++u) {
            const size_t i = (size_t)v * ow + u;
            if (!p->outside[i]) p->packed[(size_t)v * p->tpitch + u] = make_int2(p->qx[i], p->qy[i]);
        }
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_table + (size_t)stream * p->entries, p->packed.data(), p->entries * sizeof(int2), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    p->has[stream] = 1;
    if (n_outside) *n_outside = (int32_t)n_out;
    return RTMODT_OK;
}

void ln_size_host(rtmodt_lens *p) {
    const size_t n = (size_t)p->cfg.out_h * p->cfg.out_w;
    p->qx.resize(n); p->qy.resize(n); p->outside.resize(n);
}

}  // namespace

extern "C" {

void rtmodt_lens_default_cfg(rtmodt_lens_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_lens_cfg{};
    cfg->streams = 1;
}

void rtmodt_lens_destroy(rtmodt_lens *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_table);
        p->cmd.release(); p->sin.release(); p->sout.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_lens_create(const rtmodt_lens_cfg *cfg, rtmodt_lens **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(cfg->streams >= 1 && cfg->streams <= LN_MAX_STREAMS, RTMODT_E_INVALID, "streams %d outside 1..%d", cfg->streams, LN_MAX_STREAMS);
    RT_TRY(ln_check_size(cfg->src_h, cfg->src_w, cfg->out_h, cfg->out_w));
    rtmodt_lens *p = new rtmodt_lens();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->tpitch = (int)align_up((size_t)cfg->out_w, LN_RUN);
    p->entries = (size_t)cfg->out_h * p->tpitch;
    p->has.assign(cfg->streams, 0);
    auto body = [&]() -> int {
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_table, (size_t)cfg->streams * p->entries * sizeof(int2)));
        return RTMODT_OK;
    };
    return handle_created(body(), p, rtmodt_lens_destroy, out);
}

int rtmodt_lens_set_model(rtmodt_lens *p, int stream, const rtmodt_lens_params *params, int32_t *n_outside) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    RT_TRY(ln_check_stream(p, stream));
    LensModel m;
    RT_TRY(ln_check_params(params, m));
    ln_size_host(p);
    const long long n_out = lens_build_model(m, p->cfg.src_h, p->cfg.src_w, p->cfg.out_h, p->cfg.out_w, p->qx.data(), p->qy.data(), p->outside.data());
    return ln_upload(p, stream, n_out, n_outside);
}

int rtmodt_lens_set_map(rtmodt_lens *p, int stream, const float *map_x, const float *map_y, int32_t *n_outside) {
    RT_CHECK(p && map_x && map_y, RTMODT_E_INVALID, "null argument");
    RT_TRY(ln_check_stream(p, stream));
    ln_size_host(p);
    const long long n_out = lens_build_from_map(map_x, map_y, p->cfg.src_h, p->cfg.src_w, p->cfg.out_h, p->cfg.out_w, p->qx.data(), p->qy.data(),
                                                p->outside.data());
    return ln_upload(p, stream, n_out, n_outside);
}

int rtmodt_lens_read_map(rtmodt_lens *p, int stream, int32_t *qx, int32_t *qy, uint8_t *outside) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    RT_TRY(ln_check_stream(p, stream));
    RT_CHECK(p->has[stream], RTMODT_E_INVALID, "stream %d has no lens", stream);
    p->packed.resize(p->entries);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->packed.data(), p->d_table + (size_t)stream * p->entries, p->entries * sizeof(int2), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    const int oh = p->cfg.out_h, ow = p->cfg.out_w;
    for (int v = 0; v < oh; ++v)
        for (int u = 0; u < ow; ++u) {
            const int2 e = p->packed[(size_t)v * p->tpitch + u];
            const size_t i = (size_t)v * ow + u;
            const bool out = e.x == LN_OUTSIDE;
            if (qx) qx[i] = out ? 0 : e.x;
            if (qy) qy[i] = out ? 0 : e.y;
            if (outside) outside[i] = out ? 1 : 0;
        }
    return RTMODT_OK;
}

int rtmodt_lens_process(rtmodt_lens *p, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                        int dst_mem_kind, const int32_t *streams, int n) {
    RT_CHECK(p && n >= 0 && (n == 0 || (src && dst)), RTMODT_E_INVALID, "null argument");
    p->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    const rtmodt_lens_cfg &c = p->cfg;
    RT_TRY(check_frames(src, n, c.src_h, c.src_w, src_stride, src_mem_kind, kLensFrames));
    RT_TRY(check_frames((const uint8_t *const *)dst, n, c.out_h, c.out_w, dst_stride, dst_mem_kind, kLensFrames));
    for (int i = 0; i < n; ++i) {
        const int s = streams ? streams[i] : i;
        RT_TRY(ln_check_stream(p, s));
        RT_CHECK(p->has[s], RTMODT_E_INVALID, "stream %d has no lens", s);
    }
    RT_TRY(check_not_in_place(src, c.src_h, c.src_w, src_stride, dst, c.out_h, c.out_w, dst_stride, n));
    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    RT_TRY(p->sin.place(n, c.src_h, c.src_w, src_stride, src_mem_kind, FRAMES_TIGHT16));
    RT_TRY(p->sout.place(n, c.out_h, c.out_w, dst_stride, dst_mem_kind, FRAMES_TIGHT16));
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(LnSlot)));
    LnSlot *sl = (LnSlot *)p->cmd.h;
    bool wide = p->sout.pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        const int s = streams ? streams[i] : i;
        sl[i] = LnSlot{(uint64_t)(uintptr_t)p->sin.at(src, i), (uint64_t)(uintptr_t)p->sout.at(dst, i),
                       (uint64_t)(uintptr_t)(p->d_table + (size_t)s * p->entries), 0};
        wide = wide && sl[i].dst % 4 == 0;
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(LnSlot), hipMemcpyHostToDevice, q));
    RT_TRY(p->sin.copy_in(src, q));

    LnArgs a{};
    a.slots = (const LnSlot *)p->cmd.d;
    a.spitch = (long long)p->sin.pitch; a.dpitch = (long long)p->sout.pitch;
    a.src_h = c.src_h; a.src_w = c.src_w; a.out_h = c.out_h; a.out_w = c.out_w; a.tpitch = p->tpitch;
    a.tiles_x = cdiv(c.out_w, 64 * LN_RUN);
    a.border = (uint32_t)c.border_bgr[0] | (uint32_t)c.border_bgr[1] << 8 | (uint32_t)c.border_bgr[2] << 16;
    const dim3 grid((unsigned)(a.tiles_x * cdiv(c.out_h, LN_ROWS)), (unsigned)n), block(LN_THREADS);
    RT_TRY(p->timer.record(0, q));
    if (wide) hipLaunchKernelGGL(lens_remap<true>, grid, block, 0, q, a);
    else hipLaunchKernelGGL(lens_remap<false>, grid, block, 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_TRY(p->sout.copy_out(dst, q));
    RT_HIP(hipStreamSynchronize(q));
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_lens_last_ms(rtmodt_lens *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

int rtmodt_lens_distort_points(const rtmodt_lens_params *params, const double *xy, int n, double *out_xy, double *residual) {
    LensModel m;
    RT_TRY(ln_check_params(params, m));
    RT_CHECK(n >= 0 && (n == 0 || (xy && out_xy)), RTMODT_E_INVALID, "null argument");
    (void)residual;
    for (int i = 0; i < n; ++i) lens_distort_point(m, xy[2 * i], xy[2 * i + 1], out_xy[2 * i], out_xy[2 * i + 1]);
    return RTMODT_OK;
}

int rtmodt_lens_undistort_points(const rtmodt_lens_params *params, const double *xy, int n, double *out_xy, double *residual) {
    LensModel m;
    RT_TRY(ln_check_params(params, m));
    RT_CHECK(n >= 0 && (n == 0 || (xy && out_xy)), RTMODT_E_INVALID, "null argument");
    for (int i = 0; i < n; ++i) {
        double r;
        lens_undistort_point(m, xy[2 * i], xy[2 * i + 1], out_xy[2 * i], out_xy[2 * i + 1], r);
        if (residual) residual[i] = r;
    }
    return RTMODT_OK;
}

int rtmodt_lens_build_map(const rtmodt_lens_params *params, int src_h, int src_w, int out_h, int out_w, int32_t *qx, int32_t *qy, uint8_t *outside) {
    LensModel m;
    RT_TRY(ln_check_params(params, m));
    RT_TRY(ln_check_size(src_h, src_w, out_h, out_w));
    RT_CHECK(qx && qy && outside, RTMODT_E_INVALID, "null argument");
    lens_build_model(m, src_h, src_w, out_h, out_w, qx, qy, outside);
    return RTMODT_OK;
}

int rtmodt_lens_quantise_map(const float *map_x, const float *map_y, int src_h, int src_w, int out_h, int out_w, int32_t *qx, int32_t *qy,
                             uint8_t *outside) {
    RT_TRY(ln_check_size(src_h, src_w, out_h, out_w));
    RT_CHECK(map_x && map_y && qx && qy && outside, RTMODT_E_INVALID, "null argument");
    lens_build_from_map(map_x, map_y, src_h, src_w, out_h, out_w, qx, qy, outside);
    return RTMODT_OK;
}

}  // extern "C"
