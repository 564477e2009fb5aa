// jpeg_dec.hip -- the first step of the reference's loop, `cap.read()` of src/ingestion/rtsp_reader.py (cv2.VideoCapture decoding a
// camera's stream) and the image upload of web/server.py (cv2.imdecode), for Motion-JPEG on the GPU: batches of complete baseline JPEG
// files in host memory become BGR24 frames in device or host memory -- the frames rtmodt_detector_enqueue_batch(RTMODT_MEM_DEVICE)
// and rtmodt_render_batch take.  What is accepted, and every rule of the stream side, is in jpeg_dec_core.h; tests/jpeg_dec_ref.py
// restates both sides in NumPy and equals libjpeg-turbo's default decoder byte for byte on accepted streams.
//
// Host: every file is parsed up to and including SOS (jd_parse) into a descriptor -- geometry, sampling, quantisation tables, the (at
// most four) derived Huffman tables, restart interval, the scan's byte range, where its blocks and restart table lie -- the files are
// concatenated in page-locked memory, and bytes and descriptors go up in one copy each.  Frames of one call share h x w, nothing else.
//
// Four launches per call, whatever n is (all on the handle's stream, no workgroup waits for another):
//   jd_scan     (frame): 1024 threads sweep the scan 16 KB at a time for FF D0..D7; a workgroup prefix sum compacts the positions, in
//               stream order, into the frame's restart table (never past its ceil(MCUs / Ri) - 1 slots); another count: CORRUPT.
//   jd_entropy  (L intervals, frame): ONE LANE PER RESTART INTERVAL, the L intervals of a wave consecutive; L = 1 while the call has
//               at most 4096 intervals (lanes in lockstep on unlike streams cost 3 x: profiles/jpegdec), else the power of two up to 64
//               that brings the waves down to 4096 (RTMODT_JPEGDEC_LANES forces it: a test hook) (jd_decode_interval: bit
//               reader with FF 00 unstuffing bounded by the interval's end, 8-bit lookahead + maxcode / valoff walk, tables in LDS).
//               Nonzero coefficients go as int16, natural order, into the zeroed block array: 128 B per block, 768 B per 4:2:0 MCU.
//               RST(m mod 8) is checked; an interval's status reaches the frame's by atomicMax (OK < UNSUPPORTED < CORRUPT < TRUNCATED).
//   jd_idct     (32 blocks, frame): dequantise, jidctint.c "islow" (13-bit constants, columns descaled by 11, rows by 18, 32-bit
//               wrap-around), range limit (the result as a 10-bit two's-complement number, + 128, clamped to 0..255) -> one 8-bit plane
//               per component, whole blocks.  8 lanes per block: a column each, then (through LDS) a row each.
//   jd_pixels   (64 x 4 pixels, frame): jdsample.c fancy upsampling of the chroma planes (h2v1: (3 s + neighbour + 1 | 2) >> 2; h2v2:
//               colsum = 3 this_row + neighbour_row, (3 c + neighbour_c + 8 | 7) >> 4; edges are those of the component's REAL extent
//               ceil(w / 2) x ceil(h / 2), not of the block-padded plane; a component of real width <= 2 is replicated), jdcolor.c's
//               16-bit fixed point YCbCr -> BGR24 into the caller's rows; one component: B = G = R = Y.  Only the 3 w bytes of a row
//               are written.
// Planes in HBM, not halo recomputation: upsampling needs one neighbour row and column of chroma.  A workgroup that kept an MCU tile
// in LDS (160 KB per CU would hold it easily) would have to decode the blocks around its tile a second time, or tiles would have to
// talk; the planes cost 1.5 B per pixel written and read once, through L2, against an entropy stage that dominates by an order of
// magnitude (profiles/jpegdec).  DESIGN.md section 24.
//
// A stream WITHOUT restart markers (many cameras) is one interval: one wave decodes the whole frame.  That is correct and slow --
// measured 30 ms per 1080p frame at quality 95 and 11 ms at 85 (8 frames side by side: 240 / 88 ms), against 0.49 / 0.20 ms per
// frame with a restart interval per MCU row (profiles/jpegdec/README.md); a self-synchronising parallel Huffman decoder is future work.
//
// Frames whose status is not OK are skipped by the later launches: their pixels stay what they were.  Whatever the bytes hold, no
// read leaves the file's own bytes and no write leaves the frame's own blocks, restart slots, planes and output rows.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "frame_stage.h"
#include "handle_host.h"
#include "jpeg_dec_core.h"

namespace rtmodt {

constexpr int JD_SCAN_THREADS = 1024, JD_SCAN_BYTES = 16;
constexpr int JD_WAVES = 4096;                  // 256 CUs x 4 SIMDs x 4 waves
constexpr int JD_IDCT_BLOCKS = 32, JD_IDCT_THREADS = JD_IDCT_BLOCKS * 8, JD_WS_STRIDE = 72;

struct JdFrame {
    JdHeader hd;                // hd.status: the host's verdict (SIZE_MISMATCH included)
    JdLayout lay;
    uint32_t file_off;          // the file's first byte in the concatenation
    uint32_t ivl_base;          // its first slot in the restart table; it owns hd.intervals - 1 slots
    uint32_t blocks, reserved;
    uint64_t blk_off;           // its first block in the coefficient array (x 64 int16) and the plane array (x 64 bytes)
    uint64_t dst;               // BGR24 rows, device memory
    long long dst_pitch;
};

struct JdArgs {
    const JdFrame *frames;
    const uint8_t *bytes;
    uint32_t *marks;
    int32_t *status;
    int16_t *coef;
    uint8_t *planes;
    int h, w;
    int lanes;                  // restart intervals per wave of jd_entropy, 1..64
};

// exclusive prefix sum over a 1024-thread workgroup; two barriers
__device__ __forceinline__ uint32_t jd_block_scan(uint32_t v, uint32_t *s_w, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < JD_SCAN_THREADS / 64; ++w) {
        const uint32_t s = s_w[w];
        if (w < wave) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + incl - v;
}

__global__ __launch_bounds__(JD_SCAN_THREADS) void jd_scan(JdArgs a) {
    __shared__ uint32_t s_w[JD_SCAN_THREADS / 64];
    const int tid = threadIdx.x, f = blockIdx.x;
    const JdFrame &fr = a.frames[f];
    const int st0 = fr.hd.status;
    if (st0 != JD_OK) {
        if (tid == 0) a.status[f] = st0;
        return;
    }
    const uint32_t lo = fr.file_off + fr.hd.scan_off, hi = fr.file_off + fr.hd.scan_end;
    const uint32_t slots = (uint32_t)fr.hd.intervals - 1u;
    uint32_t *marks = a.marks + fr.ivl_base;
    uint32_t found = 0;
    for (uint32_t chunk = lo; chunk < hi; chunk += JD_SCAN_THREADS * JD_SCAN_BYTES) {          // (uniform trip count)
        const uint32_t p0 = chunk + (uint32_t)tid * JD_SCAN_BYTES;
        uint32_t mask = 0;
        if (p0 < hi) {
            const uint32_t p1 = min(p0 + JD_SCAN_BYTES, hi - 1u);                                // a marker needs both bytes below hi
            uint32_t prev = p0 < p1 ? a.bytes[p0] : 0u;
            for (uint32_t p = p0; p < p1; ++p) {
                const uint32_t next = a.bytes[p + 1];
                if (prev == 0xFFu && next >= 0xD0u && next <= 0xD7u) mask |= 1u << (p - p0);
                prev = next;
            }
        }
        uint32_t total;
        uint32_t at = found + jd_block_scan((uint32_t)__popc(mask), s_w, total);
        while (mask) {
            const int k = __ffs((int)mask) - 1;
            mask &= mask - 1u;
            if (at < slots) marks[at] = p0 + (uint32_t)k - fr.file_off;                          // relative to the file
            ++at;
        }
        found += total;
    }
    if (tid == 0) a.status[f] = found == slots ? JD_OK : JD_CORRUPT;
}

// SOLO (a.lanes == 1): all 64 lanes decode the workgroup's one interval in step -- nothing depends on the lane, so the bit reader and
// the decoder's state live in scalar registers and branches are scalar branches (half the time of one busy lane among 63 idle ones);
// lane 0 stores.
template <bool SOLO>
__global__ __launch_bounds__(64) void jd_entropy(JdArgs a) {
    __shared__ JdHuff s_tab[4];
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x, f = blockIdx.y;
    if (a.status[f] != JD_OK) return;                                   // (the host's verdict or jd_scan's: uniform over the workgroup)
    const JdFrame &fr = a.frames[f];
    const long long j = SOLO ? (long long)blockIdx.x : (long long)blockIdx.x * a.lanes + tid;
    if ((long long)blockIdx.x * (SOLO ? 1 : a.lanes) >= fr.hd.intervals) return;
    {
        static_assert(sizeof(JdHuff) % 4 == 0, "tables are copied by words");
        const uint32_t *src = (const uint32_t *)fr.hd.huff;
        uint32_t *dst = (uint32_t *)s_tab;
        for (int i = tid; i < (int)(4 * sizeof(JdHuff) / 4); i += 64) dst[i] = src[i];
        if (tid == 0) jd_zigzag_fill(s_zz);
    }
    __syncthreads();
    if (!SOLO && (tid >= a.lanes || j >= fr.hd.intervals)) return;
    const uint8_t *file = a.bytes + fr.file_off;
    const uint32_t *marks = a.marks + fr.ivl_base;
    const long long mcus = (long long)fr.hd.mcus_x * fr.hd.mcus_y, per = fr.hd.ri ? fr.hd.ri : mcus;
    // jd_scan stored fr.hd.intervals - 1 positions, each inside [scan_off, scan_end - 1)
    const uint32_t start = j == 0 ? fr.hd.scan_off : marks[j - 1] + 2u;
    const uint32_t end = j == fr.hd.intervals - 1 ? fr.hd.scan_end : marks[j];
    const bool writer = !SOLO || tid == 0;
    int st;
    if (j > 0 && (file[marks[j - 1] + 1u] & 7u) != (uint32_t)((j - 1) & 7)) {
        st = JD_CORRUPT;
    } else {
        const long long first = j * per, count = min(per, mcus - first);
        st = jd_decode_interval(file + start, file + max(start, end), fr.hd, s_tab, s_zz, fr.lay, first, count, a.coef + fr.blk_off * 64, writer);
    }
    if (st != JD_OK && writer) atomicMax(&a.status[f], st);
}

// one pass of jidctint.c over d[0..7] in 32-bit wrap-around arithmetic; SHIFT 11: the column pass, 18: the row pass
template <int SHIFT>
__device__ __forceinline__ void jd_idct8(const uint32_t *d, int *o) {
    uint32_t z2 = d[2], z3 = d[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 - z3 * 15137u, tmp3 = z1 + z2 * 6270u;
    z2 = d[0]; z3 = d[4];
    uint32_t tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7]; tmp1 = d[5]; tmp2 = d[3]; tmp3 = d[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5;
    z4 = z4 * (uint32_t)-3196 + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr uint32_t R = 1u << (SHIFT - 1);
    o[0] = (int)(tmp10 + tmp3 + R) >> SHIFT; o[7] = (int)(tmp10 - tmp3 + R) >> SHIFT;
    o[1] = (int)(tmp11 + tmp2 + R) >> SHIFT; o[6] = (int)(tmp11 - tmp2 + R) >> SHIFT;
    o[2] = (int)(tmp12 + tmp1 + R) >> SHIFT; o[5] = (int)(tmp12 - tmp1 + R) >> SHIFT;
    o[3] = (int)(tmp13 + tmp0 + R) >> SHIFT; o[4] = (int)(tmp13 - tmp0 + R) >> SHIFT;
}

__global__ __launch_bounds__(JD_IDCT_THREADS) void jd_idct(JdArgs a) {
    __shared__ int s_ws[JD_IDCT_BLOCKS * JD_WS_STRIDE];                 // a block's 64 ints padded to 72: the row pass meets no bank twice
    const int tid = threadIdx.x, f = blockIdx.y;
    if (a.status[f] != JD_OK) return;
    const JdFrame &fr = a.frames[f];
    const uint32_t b = blockIdx.x * JD_IDCT_BLOCKS + (uint32_t)(tid >> 3);
    const int l8 = tid & 7;
    if (blockIdx.x * JD_IDCT_BLOCKS >= fr.blocks) return;
    const bool valid = b < fr.blocks;
    int c = 0;
    if (fr.hd.ncomp > 1 && b >= fr.lay.comp_blk[1]) c = b >= fr.lay.comp_blk[2] ? 2 : 1;
    int *ws = s_ws + (tid >> 3) * JD_WS_STRIDE;
    if (valid) {
        const int16_t *src = a.coef + (fr.blk_off + b) * 64;
        const uint8_t *qt = fr.hd.qt[fr.hd.tq[c] & 3];
        uint32_t d[8];
        int o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (uint32_t)((int)src[i * 8 + l8] * (int)qt[i * 8 + l8]);
        jd_idct8<11>(d, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[i * 8 + l8] = o[i];
    }
    __syncthreads();
    if (!valid) return;
    uint32_t d[8];
    int o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (uint32_t)ws[l8 * 8 + i];
    jd_idct8<18>(d, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int s = ((o[i] + 512) & 1023) - 512;                      // 10-bit two's complement
        const uint32_t v = (uint32_t)max(0, min(s + 128, 255));
        if (i < 4) lo |= v << (8 * i);
        else hi |= v << (8 * (i - 4));
    }
    const uint32_t bi = b - fr.lay.comp_blk[c], bcols = fr.lay.bcols[c], by = bi / bcols, bx = bi - by * bcols;
    uint8_t *plane = a.planes + (fr.blk_off + fr.lay.comp_blk[c]) * 64;
    *(uint2 *)(plane + ((size_t)by * 8 + l8) * ((size_t)bcols * 8) + (size_t)bx * 8) = make_uint2(lo, hi);
}

// jdsample.c, do_fancy_upsampling: the chroma sample of pixel (x, y) from a plane of real extent ch x cw
__device__ __forceinline__ int jd_chroma(const uint8_t *p, size_t stride, int ch, int cw, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * stride + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + cx];          // replicated in both directions
    if (vs == 1) {                                                                  // h2v1
        const uint8_t *r = p + (size_t)y * stride;
        const int s = r[cx];
        if (x & 1) return cx == cw - 1 ? s : (3 * s + r[cx + 1] + 2) >> 2;
        return cx == 0 ? s : (3 * s + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1, ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);   // h2v2
    const uint8_t *r = p + (size_t)cy * stride, *q = p + (size_t)ny * stride;
    const int c = 3 * r[cx] + q[cx];
    if (x & 1) return cx == cw - 1 ? (4 * c + 7) >> 4 : (3 * c + 3 * r[cx + 1] + q[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * c + 8) >> 4 : (3 * c + 3 * r[cx - 1] + q[cx - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jd_pixels(JdArgs a) {
    const int f = blockIdx.z;
    if (a.status[f] != JD_OK) return;
    const JdFrame &fr = a.frames[f];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const uint8_t *yp = a.planes + fr.blk_off * 64;
    const int Y = yp[(size_t)y * ((size_t)fr.lay.bcols[0] * 8) + x];
    int B = Y, G = Y, R = Y;
    if (fr.hd.ncomp == 3) {
        const int hs = fr.hd.hs, vs = fr.hd.vs, cw = (a.w + hs - 1) / hs, ch = (a.h + vs - 1) / vs;
        const size_t cs = (size_t)fr.lay.bcols[1] * 8;
        const int cb = jd_chroma(a.planes + (fr.blk_off + fr.lay.comp_blk[1]) * 64, cs, ch, cw, hs, vs, x, y) - 128;
        const int cr = jd_chroma(a.planes + (fr.blk_off + fr.lay.comp_blk[2]) * 64, cs, ch, cw, hs, vs, x, y) - 128;
        R = Y + ((91881 * cr + 32768) >> 16);
        G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        B = Y + ((116130 * cb + 32768) >> 16);
    }
    uint8_t *dst = (uint8_t *)fr.dst + (long long)y * fr.dst_pitch + 3 * (long long)x;
    dst[0] = (uint8_t)max(0, min(B, 255));
    dst[1] = (uint8_t)max(0, min(G, 255));
    dst[2] = (uint8_t)max(0, min(R, 255));
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_jpegdec : HandleBase {
    int max_h = 0, max_w = 0, max_batch = 0, force_lanes = 0;
    size_t max_file = 0, slot = 0;                          // slot: max_file rounded up to 16
    EventTimer<2> timer;
    int last_n = 0;
    uint8_t *h_bytes = nullptr, *d_bytes = nullptr;         // h_*: page-locked
    JdFrame *h_frames = nullptr, *d_frames = nullptr;
    int32_t *h_status = nullptr, *d_status = nullptr;
    uint8_t *d_marks = nullptr, *d_coef = nullptr, *d_planes = nullptr;      // grown on demand
    size_t marks_cap = 0, coef_cap = 0, planes_cap = 0;
    FrameStage stage;                                       // host frames are decoded here, rows of 3w bytes
};

extern "C" {

int rtmodt_jpeg_probe(const uint8_t *file, size_t bytes, rtmodt_jpeg_info *info) {
    RT_CHECK(info && (file || bytes == 0), RTMODT_E_INVALID, "null argument");
    JdHeader *hd = new JdHeader();
    memset(hd, 0, sizeof(*hd));
    const char *msg = "";
    const int st = jd_parse(file, bytes, *hd, &msg);
    memset(info, 0, sizeof(*info));
    info->status = st;
    info->h = hd->h; info->w = hd->w; info->components = hd->ncomp;
    info->h_samp = hd->hs; info->v_samp = hd->vs; info->restart_interval = hd->ri;
    snprintf(info->message, sizeof(info->message), "%s", msg);
    delete hd;
    return RTMODT_OK;
}

void rtmodt_jpegdec_destroy(rtmodt_jpegdec *j) {
    if (!j) return;
    handle_close(j, [&] {
        hipFree(j->d_bytes); hipFree(j->d_frames); hipFree(j->d_status); hipFree(j->d_marks); hipFree(j->d_coef); hipFree(j->d_planes);
        j->stage.release();
        hipHostFree(j->h_bytes); hipHostFree(j->h_frames); hipHostFree(j->h_status);
        j->timer.destroy();
    });
    delete j;
}

int rtmodt_jpegdec_create(int device, const rtmodt_jpegdec_cfg *cfg, rtmodt_jpegdec **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(cfg->max_h >= 1 && cfg->max_w >= 1 && cfg->max_h <= JD_MAX_DIM && cfg->max_w <= JD_MAX_DIM, RTMODT_E_INVALID,
             "max frame %dx%d outside 1..%d", cfg->max_w, cfg->max_h, JD_MAX_DIM);
    RT_CHECK(cfg->max_batch >= 1 && cfg->max_batch <= 65535, RTMODT_E_INVALID, "max_batch %d outside 1..65535", cfg->max_batch);
    RT_CHECK(cfg->max_file_bytes >= 0, RTMODT_E_INVALID, "max_file_bytes %lld", (long long)cfg->max_file_bytes);
    rtmodt_jpegdec *j = new rtmodt_jpegdec();
    j->device = device; j->max_h = cfg->max_h; j->max_w = cfg->max_w; j->max_batch = cfg->max_batch;
    j->max_file = cfg->max_file_bytes ? (size_t)cfg->max_file_bytes : (size_t)cfg->max_h * cfg->max_w * 3 / 4 + 65536;
    j->slot = align_up(j->max_file, 16);
    if (const char *e = rt_opt("JPEGDEC_LANES")) j->force_lanes = std::min(std::max(atoi(e), 1), 64);      // test hook: every value decodes the same
    auto body = [&]() -> int {
        const size_t nb = (size_t)j->max_batch;
        RT_CHECK(nb * j->slot < (1ull << 32), RTMODT_E_INVALID, "%d files of %zu bytes pass 4 GiB", j->max_batch, j->max_file);
        RT_TRY(handle_open(j));
        RT_TRY(j->timer.create());
        RT_HIP(hipHostMalloc((void **)&j->h_bytes, nb * j->slot, hipHostMallocDefault));
        RT_HIP(hipMalloc((void **)&j->d_bytes, nb * j->slot));
        RT_HIP(hipHostMalloc((void **)&j->h_frames, nb * sizeof(JdFrame), hipHostMallocDefault));
        RT_HIP(hipMalloc((void **)&j->d_frames, nb * sizeof(JdFrame)));
        RT_HIP(hipHostMalloc((void **)&j->h_status, nb * sizeof(int32_t), hipHostMallocDefault));
        RT_HIP(hipMalloc((void **)&j->d_status, nb * sizeof(int32_t)));
        return RTMODT_OK;
    };
    return handle_created(body(), j, rtmodt_jpegdec_destroy, out);
}

int rtmodt_jpegdec_decode_batch(rtmodt_jpegdec *j, const uint8_t *const *files, const size_t *sizes, int n, uint8_t *const *frames, int h, int w,
                                int stride_bytes, int mem_kind, int32_t *status) {
    RT_CHECK(j && n >= 0 && (n == 0 || (files && sizes && frames && status)), RTMODT_E_INVALID, "bad argument");
    RT_TRY(check_frame_block(n, h, w, stride_bytes, mem_kind, kJpegFrames));
    for (int i = 0; i < n; ++i) RT_CHECK(files[i] && frames[i], RTMODT_E_INVALID, "file or frame %d is null", i);
    RT_CHECK(n <= j->max_batch && h <= j->max_h && w <= j->max_w, RTMODT_E_CAPACITY,
             "%d frames of %dx%d: the handle was made for %d frames of %dx%d", n, w, h, j->max_batch, j->max_w, j->max_h);
    for (int i = 0; i < n; ++i)
        RT_CHECK(sizes[i] <= j->max_file, RTMODT_E_CAPACITY, "file %d has %zu bytes, the handle was made for %zu", i, sizes[i], j->max_file);
    j->timer.timed = false;
    j->last_n = 0;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(j->device));
    RT_HIP(hipStreamSynchronize(j->stream));               // the pinned buffers may still feed the previous call's copies
    RT_TRY(j->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_TIGHT));      // nothing is copied in: the decoder writes every pixel
    size_t total_bytes = 0, total_slots = 0, total_blocks = 0;
    int max_intervals = 0;
    uint32_t max_blocks = 0;
    for (int i = 0; i < n; ++i) {
        JdFrame &fr = j->h_frames[i];
        memset(&fr, 0, sizeof(fr));
        memcpy(j->h_bytes + total_bytes, files[i], sizes[i]);
        int st = jd_parse(j->h_bytes + total_bytes, sizes[i], fr.hd, nullptr);
        if (st == JD_OK && (fr.hd.h != h || fr.hd.w != w)) st = fr.hd.status = JD_SIZE_MISMATCH;
        fr.file_off = (uint32_t)total_bytes;
        if (st == JD_OK) {
            fr.blocks = jd_layout(fr.hd, fr.lay);
            fr.ivl_base = (uint32_t)total_slots;
            fr.blk_off = total_blocks;
            total_slots += (size_t)fr.hd.intervals - 1;
            total_blocks += fr.blocks;
            max_intervals = std::max(max_intervals, fr.hd.intervals);
            max_blocks = std::max(max_blocks, fr.blocks);
        }
        fr.dst = (uint64_t)(uintptr_t)j->stage.at(frames, i);
        fr.dst_pitch = (long long)j->stage.pitch;
        total_bytes += align_up(sizes[i], 16);
    }
    RT_CHECK(total_slots < (1ull << 32), RTMODT_E_CAPACITY, "%zu restart intervals in one call", total_slots);
    RT_TRY(dev_grow(&j->d_marks, &j->marks_cap, std::max<size_t>(total_slots, 1) * sizeof(uint32_t)));
    RT_TRY(dev_grow(&j->d_coef, &j->coef_cap, std::max<size_t>(total_blocks, 1) * 64 * sizeof(int16_t)));
    RT_TRY(dev_grow(&j->d_planes, &j->planes_cap, std::max<size_t>(total_blocks, 1) * 64));
    RT_HIP(hipMemcpyAsync(j->d_bytes, j->h_bytes, std::max<size_t>(total_bytes, 16), hipMemcpyHostToDevice, j->stream));
    RT_HIP(hipMemcpyAsync(j->d_frames, j->h_frames, (size_t)n * sizeof(JdFrame), hipMemcpyHostToDevice, j->stream));
    if (total_blocks) RT_HIP(hipMemsetAsync(j->d_coef, 0, total_blocks * 64 * sizeof(int16_t), j->stream));

    JdArgs a{};
    a.frames = j->d_frames; a.bytes = j->d_bytes; a.marks = (uint32_t *)j->d_marks; a.status = j->d_status;
    a.coef = (int16_t *)j->d_coef; a.planes = j->d_planes; a.h = h; a.w = w;
    RT_TRY(j->timer.record(0, j->stream));
    hipLaunchKernelGGL(jd_scan, dim3(n), dim3(JD_SCAN_THREADS), 0, j->stream, a);
    // the lanes of a wave run in lockstep through unlike streams: few intervals are spread one per wave, and only a call with more
    // intervals than JD_WAVES waves can take at once packs several (consecutive ones) into a wave
    a.lanes = j->force_lanes;
    if (!a.lanes)
        for (a.lanes = 1; a.lanes < 64 && (long long)cdiv(max_intervals, a.lanes) * n > JD_WAVES;) a.lanes *= 2;
    if (a.lanes == 1) hipLaunchKernelGGL(jd_entropy<true>, dim3(std::max(max_intervals, 1), n), dim3(64), 0, j->stream, a);
    else hipLaunchKernelGGL(jd_entropy<false>, dim3(cdiv(max_intervals, a.lanes), n), dim3(64), 0, j->stream, a);
    hipLaunchKernelGGL(jd_idct, dim3(std::max<uint32_t>((max_blocks + JD_IDCT_BLOCKS - 1) / JD_IDCT_BLOCKS, 1), n), dim3(JD_IDCT_THREADS), 0, j->stream, a);
    hipLaunchKernelGGL(jd_pixels, dim3(cdiv(w, 64), cdiv(h, 4), n), dim3(64, 4), 0, j->stream, a);
    RT_HIP(hipGetLastError());
    RT_TRY(j->timer.record(1, j->stream));
    RT_HIP(hipMemcpyAsync(j->h_status, j->d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, j->stream));
    RT_HIP(hipStreamSynchronize(j->stream));
    j->timer.timed = true;
    j->last_n = n;
    for (int i = 0; i < n; ++i) {
        status[i] = j->h_status[i];
        if (j->stage.host && status[i] == JD_OK) RT_TRY(j->stage.copy_out_one(frames[i], i, j->stream));      // a rejected file leaves its frame as it was
    }
    if (j->stage.host) RT_HIP(hipStreamSynchronize(j->stream));
    return RTMODT_OK;
}

int rtmodt_jpegdec_last_ms(rtmodt_jpegdec *j, float *kernel_ms) {
    RT_CHECK(j && kernel_ms, RTMODT_E_INVALID, "null argument");
    return j->timer.elapsed(j->device, 0, 1, kernel_ms, "no decode_batch has run a kernel yet");
}

int rtmodt_jpegdec_coefficients(rtmodt_jpegdec *j, int frame, int component, int16_t *out, size_t out_elems, int *rows, int *cols) {
    RT_CHECK(j && rows && cols, RTMODT_E_INVALID, "null argument");
    RT_CHECK(frame >= 0 && frame < j->last_n, RTMODT_E_INVALID, "frame %d: the last decode_batch had %d", frame, j->last_n);
    const JdFrame &fr = j->h_frames[frame];
    RT_CHECK(fr.hd.status == JD_OK, RTMODT_E_INVALID, "frame %d was rejected on the host (status %d)", frame, fr.hd.status);
    RT_CHECK(component >= 0 && component < fr.hd.ncomp, RTMODT_E_INVALID, "component %d of %d", component, fr.hd.ncomp);
    *cols = (int)fr.lay.bcols[component];
    *rows = fr.hd.mcus_y * jd_comp_v(fr.hd, component);
    const size_t elems = (size_t)*rows * *cols * 64;
    if (!out || out_elems < elems) return RTMODT_OK;
    RT_HIP(hipSetDevice(j->device));
    RT_HIP(hipMemcpy(out, (const int16_t *)j->d_coef + (fr.blk_off + fr.lay.comp_blk[component]) * 64, elems * sizeof(int16_t), hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

}  // extern "C"
