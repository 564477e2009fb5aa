// enhance.hip -- frame enhancement on the GPU: low-light and low-contrast frames are lifted by contrast-limited adaptive histogram
// equalisation of the luma before every stage that reads pixels (pipeline.run(enhance=...), directly before `motion`).  Per stream the
// tone curves of the tiles live on the device and move by an integer EMA, because a per-frame CLAHE flickers on video and flicker is
// motion to the motion detector.  The reference hands cap.read()'s frame on (rtsp_reader.py) and has no counterpart; PARITY UNPINNED
// against cv2.createCLAHE (padded tiles, float interpolation) and against any default tuned on real footage.  tests/enhance_ref.py
// restates every rule in NumPy and the kernels equal it exactly: all of it is integer arithmetic, no float appears anywhere.
//
// Rules: enhance_rule.h (pixel luma: motion_model.h).  A stream holds s (uint16 8.8 per tile and level), lut8 (the curve applied, uint8
// per tile and level) and frames_seen; a call holds one histogram per frame and tile.
//
// Kernels (256 threads; a memset of the call's histograms and THREE launches per call for all its streams, whatever the frames
// show; no grid-wide barrier, no spin on another workgroup; every sum is an integer sum, so its order cannot change a result):
//   en_hist    every pixel is read once, by cell_grid.h's reader at scale 1 (a lane owns a run of 4 pixels, 12 bytes; dwords where
//              every source base and the pitch are multiples of 4).  A workgroup is a slab of up to 16 rows of ONE tile row, walked
//              across the full width, a wave to a row: its tx histograms are built in LDS with integer atomics and merged into the
//              frame's per-tile histograms with one integer atomic per non-zero bin.  PRIVATISATION: per lane group -- lane L adds
//              into copy L & (copies - 1), 4 copies up to 8 tile columns and 2 above (at most 33 KB), the copies 16 words apart so
//              that one level in neighbouring copies lies in different banks; and a lane adds a run of equal neighbours once.
//              A night frame puts a wave's 64 pixels into a handful of bins, and atomics to one address are served one after
//              another: copies per WAVE would not separate them, copies per lane group do.  profiles/enhance has the measurement.
//   en_curve   one workgroup per (frame, tile), one thread per level: the excess by a workgroup sum, the clipped and refilled bin,
//              the prefix sum (wg_dev.h), the level of the curve, the EMA into s, lut8, and the tile's sum(v * count) and excess.
//   en_apply   every pixel is read once and written once.  A workgroup is 256 x 64 pixels; the lut8 of every tile its pixels
//              interpolate between -- however many tile rows and columns that is -- are staged in LDS (a stream's whole lut8 is
//              64 KB at most).  Its head sums the tile sums into the frame's mean luma and derives eff: the device decides, no
//              host round trip; workgroup 0 of a frame writes the result row and frames_seen.  12-byte loads and stores of a
//              4-pixel run where base and pitch allow, bytes otherwise.  The step is pointwise: dst may be src.
#include <algorithm>
#include <cstring>
#include <vector>

#define MO_HD __host__ __device__
#include "grid_host.h"
#include "enhance_rule.h"

namespace rtmodt {

#include "wg_dev.h"

constexpr int EN_THREADS = CG_THREADS, EN_WAVES = EN_THREADS / 64, EN_RUN = CgRun<1>::PX;
constexpr int EN_HIST_ROWS = 16, EN_COPY_PAD = 16;
constexpr int EN_APPLY_COLS = 64 * EN_RUN, EN_APPLY_ROWS = 64;
constexpr int EN_MAX_STREAMS = 1024, EN_MAX_STREAM_TILES = 1 << 16;
static_assert(EN_RUN == 4 && CgRun<1>::RUN == 12, "a run is 4 pixels");
static_assert(sizeof(rtmodt_enhance_result) == 24, "layout");
static_assert(RTMODT_ENHANCE_SHIFT == EN_SHIFT && RTMODT_ENHANCE_GAIN == EN_GAIN && RTMODT_ENHANCE_MAX_TILES == EN_MAX_TILES, "constants");

struct EnSlot { uint64_t src, dst; int32_t stream, pad; };
static_assert(sizeof(EnSlot) == 24, "layout");
struct __attribute__((aligned(4))) EnRun { uint32_t a, b, c; };

struct EnArgs {
    const EnSlot *slots;
    long long spitch, dpitch;
    int n, h, w, ty, tx, tiles;
    int slabs, copies;                              // en_hist: slabs of a tile row, LDS copies of a histogram (a power of two)
    int blocks_x;                                   // en_apply: workgroups to a row of them
    EnRule rule;
    uint32_t *hist;                                 // [n][tiles][256], zeroed before the launches
    uint16_t *s; uint8_t *lut; int32_t *seen;       // per stream: [tiles][256], [tiles][256], one
    unsigned long long *tile_sum; uint32_t *tile_excess;    // [n][tiles]
    const uint16_t *axis_x, *axis_y;                // [w], [h]: k << 9 | f
    rtmodt_enhance_result *res;                     // [n]
};

// ---- histograms -----------------------------------------------------------------------------------------------------------------
template <bool WIDE> __global__ __launch_bounds__(EN_THREADS) void en_hist(EnArgs a) {
    extern __shared__ uint32_t s_hist[];            // [copies][tx * 256 + EN_COPY_PAD]
    __shared__ int s_bx[EN_MAX_TILES + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ky = (int)blockIdx.x / a.slabs, slab = (int)blockIdx.x % a.slabs;
    const int ya = en_bound(ky, a.h, a.ty) + slab * EN_HIST_ROWS, yb = min(ya + EN_HIST_ROWS, en_bound(ky + 1, a.h, a.ty));
    if (ya >= yb) return;                           // (the whole workgroup: tile rows differ in height by one)
    const int stride = a.tx * EN_LEVELS + EN_COPY_PAD;
    for (int i = tid; i < a.copies * stride; i += EN_THREADS) s_hist[i] = 0;
    if (tid <= a.tx) s_bx[tid] = en_bound(tid, a.w, a.tx);
    __syncthreads();
    const uint8_t *frame = (const uint8_t *)a.slots[blockIdx.y].src;
    uint32_t *mine = s_hist + (lane & (a.copies - 1)) * stride;
    const int runs = (a.w + EN_RUN - 1) / EN_RUN;
    int k_first = 0;                                // the tile column of the lane's first run
    while (k_first + 1 < a.tx && EN_RUN * lane >= s_bx[k_first + 1]) ++k_first;
    for (int y = ya + wave; y < yb; y += EN_WAVES) {
        int k = k_first;
        for (int r = lane; r < runs; r += 64) {
            const int x0 = EN_RUN * r, npx = min(EN_RUN, a.w - x0);
            en_hist_run<WIDE>(frame + (long long)y * a.spitch + 3LL * x0, a.spitch, x0, npx, s_bx, k, [&](uint32_t at, uint32_t cnt) { atomicAdd(&mine[at], cnt); });
        }
    }
    __syncthreads();
    uint32_t *out = a.hist + ((size_t)blockIdx.y * a.tiles + (size_t)ky * a.tx) * EN_LEVELS;
    for (int i = tid; i < a.tx * EN_LEVELS; i += EN_THREADS) {
        uint32_t v = 0;
        for (int c = 0; c < a.copies; ++c) v += s_hist[c * stride + i];
        if (v) atomicAdd(&out[i], v);
    }
}

// ---- curves: one workgroup per (frame, tile), one thread per level ------------------------------------------------------------------
__global__ __launch_bounds__(EN_THREADS) void en_curve(EnArgs a) {
    __shared__ int s_scan[EN_WAVES];
    __shared__ uint32_t s_ex[EN_WAVES];
    __shared__ unsigned long long s_sum[EN_WAVES];
    const int t = threadIdx.x, tile = blockIdx.x, ky = tile / a.tx, kx = tile % a.tx;
    const int stream = a.slots[blockIdx.y].stream;
    const uint32_t n = (uint32_t)(en_bound(ky + 1, a.h, a.ty) - en_bound(ky, a.h, a.ty)) * (uint32_t)(en_bound(kx + 1, a.w, a.tx) - en_bound(kx, a.w, a.tx));
    const size_t at = (size_t)blockIdx.y * a.tiles + tile;
    const uint32_t hv = a.hist[at * EN_LEVELS + t], clip = en_clip(a.rule.clip_q8, n);
    const uint32_t ex = wave_sum_u32(en_excess_of(hv, clip));
    const unsigned long long ws = wave_sum_u64((unsigned long long)hv * (unsigned)t);
    if ((t & 63) == 0) { s_ex[t >> 6] = ex; s_sum[t >> 6] = ws; }
    __syncthreads();
    uint32_t excess = 0;
    unsigned long long luma = 0;
#pragma unroll
    for (int wv = 0; wv < EN_WAVES; ++wv) { excess += s_ex[wv]; luma += s_sum[wv]; }
    const uint32_t bin = en_bin(hv, t, clip, excess);
    int total;
    const uint32_t cdf = (uint32_t)block_scan_count<EN_WAVES>((int)bin, s_scan, total) + bin;     // (at most n <= 2^28)
    const uint32_t curve = en_level(cdf, n);
    const size_t st = ((size_t)stream * a.tiles + tile) * EN_LEVELS + t;
    const uint32_t s = en_ema(a.s[st], curve, a.seen[stream], a.rule.smooth_shift);
    a.s[st] = (uint16_t)s;
    a.lut[st] = (uint8_t)en_lut8(s);
    if (t == 0) { a.tile_sum[at] = luma; a.tile_excess[at] = excess; }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
template <bool WSRC, bool WDST> __global__ __launch_bounds__(EN_THREADS) void en_apply(EnArgs a) {
    extern __shared__ uint32_t s_lut32[];           // [nky][nkx][256] bytes: the lut8 of the tiles this workgroup interpolates between
    __shared__ unsigned long long s_sum[EN_WAVES];
    __shared__ uint32_t s_ex[EN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bx = (int)blockIdx.x % a.blocks_x, by = (int)blockIdx.x / a.blocks_x;
    const EnSlot sl = a.slots[blockIdx.y];
    {
        const size_t at = (size_t)blockIdx.y * a.tiles + tid;
        const unsigned long long v = wave_sum_u64(tid < a.tiles ? a.tile_sum[at] : 0ull);
        const uint32_t e = wave_sum_u32(tid < a.tiles ? a.tile_excess[at] : 0u);
        if (lane == 0) { s_sum[wave] = v; s_ex[wave] = e; }
    }
    const int xa = bx * EN_APPLY_COLS, xl = min(xa + EN_APPLY_COLS, a.w) - 1, ya = by * EN_APPLY_ROWS, yl = min(ya + EN_APPLY_ROWS, a.h) - 1;
    const int kx_lo = a.axis_x[xa] >> 9, nkx = en_neighbour(a.axis_x[xl] >> 9, a.tx) - kx_lo + 1;
    const int ky_lo = a.axis_y[ya] >> 9, nky = en_neighbour(a.axis_y[yl] >> 9, a.ty) - ky_lo + 1;
    const uint32_t *g = (const uint32_t *)(a.lut + (size_t)sl.stream * a.tiles * EN_LEVELS);
    for (int i = tid; i < nky * nkx * 64; i += EN_THREADS) {
        const int tl = i >> 6, j = tl / nkx, c = tl - j * nkx;
        s_lut32[i] = g[((ky_lo + j) * a.tx + kx_lo + c) * 64 + (i & 63)];
    }
    __syncthreads();
    unsigned long long luma = 0;
    uint32_t clipped = 0;
#pragma unroll
    for (int wv = 0; wv < EN_WAVES; ++wv) { luma += s_sum[wv]; clipped += s_ex[wv]; }
    const int eff = (int)en_eff(a.rule, luma, (uint64_t)a.h * (uint64_t)a.w);
    if (blockIdx.x == 0 && tid == 0) {              // (en_curve, the reader of frames_seen, has finished)
        const int seen = en_next_seen(a.seen[sl.stream]);
        a.seen[sl.stream] = seen;
        a.res[blockIdx.y] = rtmodt_enhance_result{sl.stream, seen, (uint32_t)eff, clipped, luma};
    }
    const int x0 = xa + lane * EN_RUN;
    if (x0 >= a.w) return;
    const int npx = min(EN_RUN, a.w - x0);
    const uint8_t *s_lut = (const uint8_t *)s_lut32;
    uint32_t o0[EN_RUN], o1[EN_RUN], fx[EN_RUN];    // the run's columns: LDS offsets of tile k and of its neighbour, and f
#pragma unroll
    for (int i = 0; i < EN_RUN; ++i) {
        const uint32_t p = a.axis_x[x0 + (i < npx ? i : 0)];
        const int k = (int)(p >> 9);
        fx[i] = p & 511u;
        o0[i] = (uint32_t)(k - kx_lo) * EN_LEVELS; o1[i] = (uint32_t)(en_neighbour(k, a.tx) - kx_lo) * EN_LEVELS;
    }
    for (int y = ya + wave; y <= yl; y += EN_WAVES) {
        const uint32_t py = a.axis_y[y], fy = py & 511u;
        const int ky = (int)(py >> 9);
        const uint8_t *r0 = s_lut + (ky - ky_lo) * nkx * EN_LEVELS, *r1 = s_lut + (en_neighbour(ky, a.ty) - ky_lo) * nkx * EN_LEVELS;
        const uint8_t *src = (const uint8_t *)sl.src + (long long)y * a.spitch + 3LL * x0;
        uint8_t *dst = (uint8_t *)sl.dst + (long long)y * a.dpitch + 3LL * x0;
        uint32_t px[EN_RUN];                        // b | g << 8 | r << 16
        if (WSRC && npx == EN_RUN) {
            const EnRun v = *(const EnRun *)src;    // base, pitch and 3 * x0 (a multiple of 12) are multiples of 4
            px[0] = v.a & 0xffffffu; px[1] = v.a >> 24 | (v.b & 0xffffu) << 8; px[2] = v.b >> 16 | (v.c & 0xffu) << 16; px[3] = v.c >> 8;
        } else {
#pragma unroll
            for (int i = 0; i < EN_RUN; ++i) px[i] = i < npx ? (uint32_t)src[3 * i] | (uint32_t)src[3 * i + 1] << 8 | (uint32_t)src[3 * i + 2] << 16 : 0u;
        }
#pragma unroll
        for (int i = 0; i < EN_RUN; ++i) {
            const int b = (int)(px[i] & 255u), gr = (int)(px[i] >> 8 & 255u), r = (int)(px[i] >> 16);
            const uint32_t yv = mo_luma((uint32_t)b, (uint32_t)gr, (uint32_t)r);
            const uint32_t y1 = en_interp(r0[o0[i] + yv], r0[o1[i] + yv], r1[o0[i] + yv], r1[o1[i] + yv], fx[i], fy);
            const int y2 = en_y2((int)yv, (int)y1, eff);
            px[i] = en_channel(a.rule.colour, b, (int)yv, y2) | en_channel(a.rule.colour, gr, (int)yv, y2) << 8 | en_channel(a.rule.colour, r, (int)yv, y2) << 16;
        }
        if (WDST && npx == EN_RUN) {
            EnRun v;
            v.a = px[0] | px[1] << 24; v.b = px[1] >> 8 | px[2] << 16; v.c = px[2] >> 16 | px[3] << 8;
            *(EnRun *)dst = v;
        } else {
#pragma unroll
            for (int i = 0; i < EN_RUN; ++i)
                if (i < npx) {
                    dst[3 * i] = (uint8_t)px[i]; dst[3 * i + 1] = (uint8_t)(px[i] >> 8); dst[3 * i + 2] = (uint8_t)(px[i] >> 16);
                }
        }
    }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_enhance : HandleBase {
    rtmodt_enhance_cfg cfg{};
    EnRule rule{};
    int tiles = 0, slabs = 0, copies = 0, blocks_x = 0, blocks_y = 0;
    size_t hist_lds = 0, apply_lds = 0;
    EventTimer<2> timer;
    uint16_t *d_s = nullptr, *d_axis = nullptr;     // d_axis: [w] then [h]
    uint8_t *d_lut = nullptr;
    int32_t *d_seen = nullptr;
    uint32_t *d_hist = nullptr;
    char *d_work = nullptr;                         // tile_sum[S][tiles] | tile_excess[S][tiles] | results[S]
    rtmodt_enhance_result *h_out = nullptr;
    std::vector<int32_t> last_slot;                 // per stream: its frame in the last call, or -1
    CmdBuf cmd;                                     // (every call ends with a synchronize: the pinned half is idle when the next one writes it)
    FrameStage sin, sout;                           // host sources in, host destinations out
};

namespace {

int en_check_axis(int px, int tiles, const char *what) {
    RT_CHECK(px >= 1 && px <= EN_MAX_DIM, RTMODT_E_INVALID, "%s of %d pixels outside 1..%d", what, px, EN_MAX_DIM);
    RT_CHECK(en_tiles_ok(tiles, px), RTMODT_E_INVALID, "tiles: %d along the %s of %d pixels (1..%d and no more than the pixels)", tiles, what, px, EN_MAX_TILES);
    return RTMODT_OK;
}

int en_check_cfg(const rtmodt_enhance_cfg *c) {
    RT_CHECK(c, RTMODT_E_INVALID, "null enhance config");
    RT_CHECK(c->streams >= 1 && c->streams <= EN_MAX_STREAMS, RTMODT_E_INVALID, "streams %d outside 1..%d", c->streams, EN_MAX_STREAMS);
    RT_TRY(en_check_axis(c->height, c->tiles_y, "height"));
    RT_TRY(en_check_axis(c->width, c->tiles_x, "width"));
    RT_CHECK(c->clip_q8 >= 0 && c->clip_q8 <= EN_MAX_CLIP_Q8, RTMODT_E_INVALID, "clip_limit: clip_q8 %d outside 0..%d", c->clip_q8, EN_MAX_CLIP_Q8);
    RT_CHECK(c->strength >= 0 && c->strength <= EN_MAX_STRENGTH, RTMODT_E_INVALID, "strength %d outside 0..%d", c->strength, EN_MAX_STRENGTH);
    RT_CHECK(c->smooth_shift >= 0 && c->smooth_shift <= EN_MAX_SHIFT, RTMODT_E_INVALID, "smooth_shift %d outside 0..%d", c->smooth_shift, EN_MAX_SHIFT);
    RT_CHECK(c->auto_lo >= 0 && c->auto_hi >= c->auto_lo && c->auto_hi <= 255, RTMODT_E_INVALID, "auto (%d, %d): 0 <= auto_lo <= auto_hi <= 255", c->auto_lo, c->auto_hi);
    RT_CHECK(c->colour == EN_SHIFT || c->colour == EN_GAIN, RTMODT_E_INVALID, "colour %d: RTMODT_ENHANCE_SHIFT or RTMODT_ENHANCE_GAIN", c->colour);
    RT_CHECK((long long)c->streams * c->tiles_y * c->tiles_x <= EN_MAX_STREAM_TILES, RTMODT_E_CAPACITY, "%lld tiles over all streams (at most %d)",
             (long long)c->streams * c->tiles_y * c->tiles_x, EN_MAX_STREAM_TILES);
    return RTMODT_OK;
}

void en_axis_table(int px, int tiles, uint16_t *out) {
    for (int x = 0; x < px; ++x) {
        int32_t k, f;
        en_axis(x, px, tiles, k, f);
        out[x] = (uint16_t)en_axis_pack(k, f);
    }
}

// the most tiles a workgroup of en_apply interpolates between along one axis: blocks of `block` pixels
int en_most_tiles(const uint16_t *axis, int px, int tiles, int block) {
    int most = 1;
    for (int a = 0; a < px; a += block) most = std::max(most, en_neighbour(axis[std::min(a + block, px) - 1] >> 9, tiles) - (axis[a] >> 9) + 1);
    return most;
}

void (*const en_hist_kernels[2])(EnArgs) = {en_hist<false>, en_hist<true>};
void (*const en_apply_kernels[2][2])(EnArgs) = {{en_apply<false, false>, en_apply<false, true>}, {en_apply<true, false>, en_apply<true, true>}};

size_t en_stream_values(const rtmodt_enhance *p) { return (size_t)p->tiles * EN_LEVELS; }

}  // namespace

extern "C" {

void rtmodt_enhance_default_cfg(rtmodt_enhance_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_enhance_cfg{};
    cfg->streams = 1; cfg->height = 0; cfg->width = 0;
    cfg->tiles_y = 8; cfg->tiles_x = 8; cfg->clip_q8 = 512; cfg->strength = 256; cfg->smooth_shift = 2;
    cfg->auto_lo = 0; cfg->auto_hi = 0; cfg->colour = EN_SHIFT;
    cfg->device = 0;
}

void rtmodt_enhance_destroy(rtmodt_enhance *p) {
    if (!p) return;
    handle_close(p, [&] {
        hipFree(p->d_s); hipFree(p->d_axis); hipFree(p->d_lut); hipFree(p->d_seen); hipFree(p->d_hist); hipFree(p->d_work);
        hipHostFree(p->h_out);
        p->cmd.release(); p->sin.release(); p->sout.release();
        p->timer.destroy();
    });
    delete p;
}

int rtmodt_enhance_create(const rtmodt_enhance_cfg *cfg, rtmodt_enhance **out) {
    RT_CHECK(out, RTMODT_E_INVALID, "null argument");
    RT_TRY(en_check_cfg(cfg));
    rtmodt_enhance *p = new rtmodt_enhance();
    p->device = cfg->device;
    p->cfg = *cfg;
    p->rule = EnRule{cfg->clip_q8, cfg->strength, cfg->smooth_shift, cfg->auto_lo, cfg->auto_hi, cfg->colour};
    const int h = cfg->height, w = cfg->width, ty = cfg->tiles_y, tx = cfg->tiles_x;
    p->tiles = ty * tx;
    p->slabs = cdiv(cdiv(h, ty), EN_HIST_ROWS);                      // (the tallest tile row has ceil(h / ty) rows)
    p->copies = tx <= 8 ? 4 : 2;
    p->hist_lds = (size_t)p->copies * (tx * EN_LEVELS + EN_COPY_PAD) * sizeof(uint32_t);
    p->blocks_x = cdiv(w, EN_APPLY_COLS); p->blocks_y = cdiv(h, EN_APPLY_ROWS);
    std::vector<uint16_t> axis((size_t)w + h);
    en_axis_table(w, tx, axis.data());
    en_axis_table(h, ty, axis.data() + w);
    p->apply_lds = (size_t)en_most_tiles(axis.data(), w, tx, EN_APPLY_COLS) * en_most_tiles(axis.data() + w, h, ty, EN_APPLY_ROWS) * EN_LEVELS;
    p->last_slot.assign(cfg->streams, -1);
    auto body = [&]() -> int {
        const size_t S = (size_t)cfg->streams, all = S * en_stream_values(p), st = S * p->tiles;
        RT_TRY(handle_open(p));
        RT_TRY(p->timer.create());
        RT_HIP(hipMalloc((void **)&p->d_s, all * sizeof(uint16_t)));
        RT_HIP(hipMalloc((void **)&p->d_lut, all));
        RT_HIP(hipMalloc((void **)&p->d_seen, S * sizeof(int32_t)));
        RT_HIP(hipMalloc((void **)&p->d_hist, all * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&p->d_work, align_up(st * 12, 8) + S * sizeof(rtmodt_enhance_result)));
        RT_HIP(hipMalloc((void **)&p->d_axis, axis.size() * sizeof(uint16_t)));
        RT_HIP(hipHostMalloc((void **)&p->h_out, S * sizeof(rtmodt_enhance_result), hipHostMallocDefault));
        RT_HIP(handle_zero(p->d_s, all * sizeof(uint16_t), p->stream));
        RT_HIP(handle_zero(p->d_lut, all, p->stream));
        RT_HIP(handle_zero(p->d_seen, S * sizeof(int32_t), p->stream));
        RT_HIP(handle_zero(p->d_hist, all * sizeof(uint32_t), p->stream));
        RT_HIP(hipMemcpyAsync(p->d_axis, axis.data(), axis.size() * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
        return handle_wait(p->stream);                      // (the table is a local of this function)
    };
    return handle_created(body(), p, rtmodt_enhance_destroy, out);
}

int rtmodt_enhance_process(rtmodt_enhance *p, const uint8_t *const *src, int src_stride, int src_mem_kind, uint8_t *const *dst, int dst_stride,
                           int dst_mem_kind, const int32_t *streams, int n, int h, int w, rtmodt_enhance_result *results) {
    RT_CHECK(p && n >= 0 && (n == 0 || (src && dst)), RTMODT_E_INVALID, "null argument");
    p->timer.timed = false;
    const rtmodt_enhance_cfg &c = p->cfg;
    RT_CHECK(h == c.height && w == c.width, RTMODT_E_INVALID, "frames of %dx%d, the enhancer was created for %dx%d", w, h, c.width, c.height);
    RT_TRY(check_stream_list(src, streams, n, c.streams));
    if (n == 0) return RTMODT_OK;
    RT_TRY(check_frames(src, n, h, w, src_stride, src_mem_kind, kLensFrames));
    RT_TRY(check_frames((const uint8_t *const *)dst, n, h, w, dst_stride, dst_mem_kind, kLensFrames));
    RT_TRY(check_not_in_place(src, h, w, src_stride, dst, h, w, dst_stride, n, true));

    RT_HIP(hipSetDevice(p->device));
    hipStream_t q = p->stream;
    // host frames enhanced in place are staged once: the kernel writes where it read
    bool alias = src_mem_kind == RTMODT_MEM_HOST && dst_mem_kind == RTMODT_MEM_HOST && src_stride == dst_stride;
    for (int i = 0; i < n; ++i) alias = alias && dst[i] == src[i];
    RT_TRY(p->sin.place(n, h, w, src_stride, src_mem_kind, FRAMES_TIGHT16));
    if (!alias) RT_TRY(p->sout.place(n, h, w, dst_stride, dst_mem_kind, FRAMES_TIGHT16));
    FrameStage &so = alias ? p->sin : p->sout;
    RT_TRY(p->cmd.reserve((size_t)n * sizeof(EnSlot)));
    EnSlot *sl = (EnSlot *)p->cmd.h;
    bool wsrc = p->sin.pitch % 4 == 0, wdst = so.pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        sl[i] = EnSlot{(uint64_t)(uintptr_t)p->sin.at(src, i), (uint64_t)(uintptr_t)so.at(dst, i), streams ? streams[i] : i, 0};
        wsrc = wsrc && sl[i].src % 4 == 0;
        wdst = wdst && sl[i].dst % 4 == 0;
    }
    RT_HIP(hipMemcpyAsync(p->cmd.d, p->cmd.h, (size_t)n * sizeof(EnSlot), hipMemcpyHostToDevice, q));
    RT_TRY(p->sin.copy_in(src, q));

    const size_t st = (size_t)c.streams * p->tiles;
    EnArgs a{};
    a.slots = (const EnSlot *)p->cmd.d;
    a.spitch = (long long)p->sin.pitch; a.dpitch = (long long)so.pitch;
    a.n = n; a.h = h; a.w = w; a.ty = c.tiles_y; a.tx = c.tiles_x; a.tiles = p->tiles;
    a.slabs = p->slabs; a.copies = p->copies; a.blocks_x = p->blocks_x;
    a.rule = p->rule;
    a.hist = p->d_hist; a.s = p->d_s; a.lut = p->d_lut; a.seen = p->d_seen;
    a.tile_sum = (unsigned long long *)p->d_work; a.tile_excess = (uint32_t *)(p->d_work + st * 8);
    a.axis_x = p->d_axis; a.axis_y = p->d_axis + w;
    a.res = (rtmodt_enhance_result *)(p->d_work + align_up(st * 12, 8));

    static DynLdsSeen seen_hist[2], seen_apply[2][2];
    RT_TRY(raise_dynamic_lds((const void *)en_hist_kernels[wsrc], p->hist_lds, seen_hist[wsrc]));
    RT_TRY(raise_dynamic_lds((const void *)en_apply_kernels[wsrc][wdst], p->apply_lds, seen_apply[wsrc][wdst]));
    const dim3 block(EN_THREADS);
    RT_TRY(p->timer.record(0, q));
    RT_HIP(hipMemsetAsync(p->d_hist, 0, (size_t)n * en_stream_values(p) * sizeof(uint32_t), q));
    hipLaunchKernelGGL(en_hist_kernels[wsrc], dim3((unsigned)(c.tiles_y * p->slabs), (unsigned)n), block, p->hist_lds, q, a);
    hipLaunchKernelGGL(en_curve, dim3((unsigned)p->tiles, (unsigned)n), block, 0, q, a);
    hipLaunchKernelGGL(en_apply_kernels[wsrc][wdst], dim3((unsigned)(p->blocks_x * p->blocks_y), (unsigned)n), block, p->apply_lds, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(p->timer.record(1, q));
    RT_TRY(so.copy_out(dst, q));
    if (results) RT_HIP(hipMemcpyAsync(p->h_out, a.res, (size_t)n * sizeof(rtmodt_enhance_result), hipMemcpyDeviceToHost, q));      // every result in one copy
    RT_HIP(hipStreamSynchronize(q));
    if (results) memcpy(results, p->h_out, (size_t)n * sizeof(rtmodt_enhance_result));
    std::fill(p->last_slot.begin(), p->last_slot.end(), -1);
    for (int i = 0; i < n; ++i) p->last_slot[streams ? streams[i] : i] = i;
    p->timer.timed = true;
    return RTMODT_OK;
}

int rtmodt_enhance_read_state(rtmodt_enhance *p, int stream, uint16_t *s, int32_t *frames_seen) {
    RT_CHECK(p && s && frames_seen, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(s, p->d_s + (size_t)stream * en_stream_values(p), en_stream_values(p) * sizeof(uint16_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipMemcpyAsync(frames_seen, p->d_seen + stream, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_enhance_load_state(rtmodt_enhance *p, int stream, const uint16_t *s, int64_t n_values, int32_t frames_seen) {
    RT_CHECK(p && s, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    RT_CHECK(n_values == (int64_t)en_stream_values(p), RTMODT_E_INVALID, "state of %lld values, this enhancer holds %dx%dx%d per stream", (long long)n_values,
             p->cfg.tiles_y, p->cfg.tiles_x, EN_LEVELS);
    RT_CHECK(frames_seen >= 0 && frames_seen <= EN_MAX_SEEN, RTMODT_E_INVALID, "state: frames_seen %d outside 0..2^30", frames_seen);
    for (int64_t i = 0; i < n_values; ++i) RT_CHECK(s[i] <= EN_MAX_S, RTMODT_E_INVALID, "state: value %lld is %u, above 255 << 8", (long long)i, (unsigned)s[i]);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(p->d_s + (size_t)stream * en_stream_values(p), s, en_stream_values(p) * sizeof(uint16_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipMemcpyAsync(p->d_seen + stream, &frames_seen, sizeof(int32_t), hipMemcpyHostToDevice, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_enhance_reset(rtmodt_enhance *p, int stream) {
    RT_CHECK(p, RTMODT_E_INVALID, "null argument");
    if (stream != -1) RT_TRY(check_stream(stream, p->cfg.streams));
    RT_HIP(hipSetDevice(p->device));
    const size_t first = stream < 0 ? 0 : (size_t)stream, count = stream < 0 ? (size_t)p->cfg.streams : 1;
    RT_HIP(handle_zero(p->d_s + first * en_stream_values(p), count * en_stream_values(p) * sizeof(uint16_t), p->stream));
    RT_HIP(handle_zero(p->d_seen + first, count * sizeof(int32_t), p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_enhance_histograms(rtmodt_enhance *p, int stream, uint32_t *hist) {
    RT_CHECK(p && hist, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_stream(stream, p->cfg.streams));
    const int slot = p->last_slot[stream];
    RT_CHECK(slot >= 0, RTMODT_E_INVALID, "stream %d was not in the last process call: it has no histograms", stream);
    RT_HIP(hipSetDevice(p->device));
    RT_HIP(hipMemcpyAsync(hist, p->d_hist + (size_t)slot * en_stream_values(p), en_stream_values(p) * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    RT_HIP(hipStreamSynchronize(p->stream));
    return RTMODT_OK;
}

int rtmodt_enhance_last_ms(rtmodt_enhance *p, float *kernel_ms) {
    RT_CHECK(p && kernel_ms, RTMODT_E_INVALID, "null argument");
    return p->timer.elapsed(p->device, 0, 1, kernel_ms, "no process call has launched yet");
}

int rtmodt_enhance_curve(const uint32_t *hist, int64_t n, int32_t clip_q8, uint32_t *curve, uint32_t *excess) {
    RT_CHECK(hist && curve, RTMODT_E_INVALID, "null argument");
    RT_CHECK(n >= 1 && n <= (int64_t)EN_MAX_AREA, RTMODT_E_INVALID, "n %lld outside 1..2^28", (long long)n);
    RT_CHECK(clip_q8 >= 0 && clip_q8 <= EN_MAX_CLIP_Q8, RTMODT_E_INVALID, "clip_q8 %d outside 0..%d", clip_q8, EN_MAX_CLIP_Q8);
    uint64_t sum = 0;
    for (int i = 0; i < EN_LEVELS; ++i) sum += hist[i];
    RT_CHECK(sum == (uint64_t)n, RTMODT_E_INVALID, "hist sums to %llu, n is %lld", (unsigned long long)sum, (long long)n);
    const uint32_t ex = en_curve_of(hist, (uint32_t)n, clip_q8, curve);
    if (excess) *excess = ex;
    return RTMODT_OK;
}

int rtmodt_enhance_axis(int32_t px, int32_t tiles, int32_t *k, int32_t *f, int32_t *bounds) {
    RT_CHECK(k && f, RTMODT_E_INVALID, "null argument");
    RT_TRY(en_check_axis(px, tiles, "axis"));
    for (int x = 0; x < px; ++x) en_axis(x, px, tiles, k[x], f[x]);
    if (bounds)
        for (int i = 0; i <= tiles; ++i) bounds[i] = en_bound(i, px, tiles);
    return RTMODT_OK;
}

}  // extern "C"
