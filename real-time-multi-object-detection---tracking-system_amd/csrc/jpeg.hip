// jpeg.hip -- the step after FrameRenderer.render in the reference's loop (tools/run_pipeline.py:112-117,160-161: every annotated
// frame goes through cv2.VideoWriter, `MJPG` included) on the GPU: batches of BGR24 frames, in device or host memory, become
// complete baseline JPEG files (ITU-T T.81 sequential DCT, Huffman, 8-bit, YCbCr 4:2:0, JFIF) in host memory.
//
// Stream (fixed, so that the work is parallel and any decoder reads it):
//   SOI | APP0 JFIF 1.1, density 1:1 | DQT luminance | DQT chrominance | SOF0 (Y 2x2, Cb 1x1, Cr 1x1) | DHT DC0, AC0, DC1, AC1 (the
//   Annex K "typical" tables, never optimised) | DRI = ceil(w / 16) MCUs = ONE MCU ROW | SOS | scan | EOI.
//   Every restart interval starts byte-aligned with the three DC predictors at 0, is padded with 1-bits to a whole byte and is
//   followed by RST(m mod 8), m = its MCU row, except the last: an interval depends on no other.
//
// Arithmetic: integers only; tests/jpeg_ref.py restates it in NumPy and the two agree bit for bit.  They are libjpeg's rules
// (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jccoefct.c, jchuff.c), so the stream equals libjpeg-turbo's for the same pixels:
//   quantisation tables  Annex K scaled by  s = q < 50 ? 5000 / q : 200 - 2q,  (base * s + 50) / 100  clamped to 1..255;
//   colour               Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//                        Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//                        Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16;
//   edges                a pixel right of or below the frame is the pixel at the clamped coordinate (last column / row replicated);
//   chroma               2 x 2 box sum, (sum + bias) >> 2, bias 1, 2, 1, 2 ... along a row; a chroma row below ceil(h / 2) - 1 is a
//                        copy of that row (libjpeg pads the down-sampled rows, not the pixels: it matters when h is even);
//   forward DCT          Loeffler-Ligtenberg-Moschytz with 13-bit constants ("islow"): rows first, keeping 2 extra bits, then
//                        columns; samples - 128 in, coefficients x 8 out;  DESCALE(x, n) = (x + (1 << (n - 1))) >> n;
//   quantisation         sign(c) * ((|c| + 4 q) / (8 q)), then clamped to -1024..1023 (DC) / -1023..1023 (AC): the clamp never acts
//                        on 8-bit samples, it bounds the code length of a block whatever the scratch holds;
//   dummy blocks         a luminance block wholly outside the ceil(w / 8) x ceil(h / 8) blocks of the frame has zero AC and the DC
//                        of the block before it in its MCU: right edge DC1 = DC0, DC3 = DC2; bottom edge DC2 = DC3 = DC1;
//   entropy coding       DC: category of the difference to the previous block of the component, AC: (run, size) with ZRL and EOB,
//                        negative values as value - 1 in `size` bits; FF -> FF 00 inside an interval.
//
// Kernels (all grids sized from the work, no workgroup waits for another):
//   jpeg_dct      (8-MCU chunk, MCU row, frame): 256 threads convert 128 x 16 pixels into 48 blocks in LDS (one thread per 2 x 2
//                 pixel quad), run the row pass and the column pass (one thread per row / column of a block), quantise, and store
//                 the int16 coefficients in zigzag order, 768 contiguous bytes per MCU, into the handle's scratch.
//   jpeg_code<0>  (MCU row, frame): codes the interval and stores only its stuffed length.
//   jpeg_offsets  (frame): exclusive scan of the interval lengths (+ 2 per marker) -> where each interval starts, the file size,
//                 and whether the file fits the caller's slot.
//   jpeg_code<1>  codes the interval again, now to its final place -- only for frames that fit.
//   jpeg_code walks an interval in chunks of 42 MCUs = 252 blocks, one thread per block: the block's bit length (a walk over its
//   coefficients), an exclusive scan over the workgroup (cross-lane moves inside a wave, one LDS step across the 4 waves), the same
//   walk again depositing the bits at the block's offset into an LDS bit buffer (words shared by neighbouring blocks are OR-ed),
//   then per 1024 bytes a second scan over the count of FF bytes and the byte stores.  The bit position inside the last byte and
//   that byte's value are carried to the next chunk; the DC predictor of a block is its neighbour's DC in the scratch.
//   LDS does not depend on w: 51 KB bit buffer (252 blocks x 1658 bits worst case: 20 for DC, 63 x 26 for AC) + 2 KB of tables.
//   Scratch: 768 bytes per MCU (6.3 MB per 1080p frame) + 8 bytes per MCU row; staging for the scans, at most the caller's slot.
//   No byte is written outside the handle's scratch and staging; the host copies sizes[i] <= slot_bytes bytes into slot i.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "frame_stage.h"
#include "handle_host.h"

namespace rtmodt {

constexpr int JP_THREADS = 256, JP_WAVES = JP_THREADS / 64;
constexpr int JP_DCT_MCUS = 8, JP_BSTRIDE = 72;                 // a block's 64 ints padded to 72: the column pass meets no bank twice
constexpr int JP_CODE_MCUS = 42, JP_CODE_BLOCKS = JP_CODE_MCUS * 6;
constexpr int JP_BLOCK_BITS = 20 + 63 * 26;                    // worst case of one block
constexpr int JP_WORDS = (JP_CODE_BLOCKS * JP_BLOCK_BITS + 14 + 31) / 32 + 2;
constexpr int JP_BLOCK_BYTES = 2 * ((JP_BLOCK_BITS + 7) / 8);  // stuffed
constexpr int JP_MAX_DIM = 8192;
static_assert(JP_CODE_BLOCKS <= JP_THREADS && JP_WORDS * 4 + 2048 + 256 <= 64 * 1024, "LDS budget");

static const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                                    54, 47, 55, 62, 63};
static const uint8_t kLumaQ[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                                   101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: BITS and HUFFVAL of the four typical tables
static const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// what the kernels read besides the frames: divisors 8 q in natural order, the zigzag position of a natural index, and the four
// Huffman tables as symbol -> code | length << 16 (0: DC luminance, 1: AC luminance, 2: DC chrominance, 3: AC chrominance)
struct JpegTables {
    uint32_t huff[4][256];
    uint16_t qdiv[2][64];
    uint8_t zzpos[64];
};

struct DctArgs {
    const uint64_t *frames;
    const JpegTables *tab;
    int16_t *coef;
    long long stride, coef_frame;          // bytes between rows; int16 elements between frames
    int h, w, mcus_x, mcus_y;
};

struct CodeArgs {
    const int16_t *coef;
    const JpegTables *tab;
    uint32_t *ilen;                        // [n][mcus_y] stuffed bytes of an interval
    const uint32_t *ioff;                  // [n][mcus_y] where it starts in the frame's staging
    const uint32_t *fits;                  // [n]
    uint8_t *out;
    long long coef_frame, out_stride;
    int mcus_x, mcus_y;
};

struct OffArgs {
    const uint32_t *ilen;
    uint32_t *ioff, *sizes, *fits;
    int mcus_y;
    uint32_t hdr;
    unsigned long long cap;                // scan + EOI bytes a frame may take
};

#define JP_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

// one pass of jfdctint.c over d[0..7]; FIRST: the row pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int *d) {
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    } else {
        d[0] = JP_DESCALE(t10 + t11, 2);
        d[4] = JP_DESCALE(t10 - t11, 2);
    }
    const int z1 = (t12 + t13) * 4433;
    d[2] = JP_DESCALE(z1 + t13 * 6270, N);
    d[6] = JP_DESCALE(z1 - t12 * 15137, N);
    const int y1 = t4 + t7, y2 = t5 + t6, y3 = t4 + t6, y4 = t5 + t7;
    const int z5 = (y3 + y4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    const int b1 = y1 * -7373, b2 = y2 * -20995, b3 = y3 * -16069 + z5, b4 = y4 * -3196 + z5;
    d[7] = JP_DESCALE(a4 + b1 + b3, N);
    d[5] = JP_DESCALE(a5 + b2 + b4, N);
    d[3] = JP_DESCALE(a6 + b2 + b3, N);
    d[1] = JP_DESCALE(a7 + b1 + b4, N);
}

__device__ __forceinline__ void ycc(const uint8_t *p, int &y, int &cb, int &cr) {
    const int b = p[0], g = p[1], r = p[2];
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_dct(DctArgs a) {
    __shared__ __attribute__((aligned(16))) int s_ws[JP_DCT_MCUS * 6 * JP_BSTRIDE];
    __shared__ __attribute__((aligned(16))) int16_t s_out[JP_DCT_MCUS * 6 * 64];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * JP_DCT_MCUS, mrow = blockIdx.y;
    const int nm = min(JP_DCT_MCUS, a.mcus_x - m0), nblk = nm * 6;
    const uint8_t *src = (const uint8_t *)a.frames[blockIdx.z];
    const int hb = (a.h + 7) >> 3, wb = (a.w + 7) >> 3, ch_last = ((a.h + 1) >> 1) - 1;

    // ---- pixels -> level-shifted samples, block by block ----
    for (int q = tid; q < 8 * 8 * JP_DCT_MCUS; q += JP_THREADS) {
        const int qy = q >> 6, qx = q & 63, mc = qx >> 3;
        if (mc >= nm) continue;
        const int x0 = min(m0 * 16 + 2 * qx, a.w - 1), x1 = min(m0 * 16 + 2 * qx + 1, a.w - 1);
        const int y0 = min(mrow * 16 + 2 * qy, a.h - 1), y1 = min(mrow * 16 + 2 * qy + 1, a.h - 1);
        const uint8_t *r0 = src + (long long)y0 * a.stride, *r1 = src + (long long)y1 * a.stride;
        int yv[4], cb[4], cr[4];
        ycc(r0 + 3 * x0, yv[0], cb[0], cr[0]);
        ycc(r0 + 3 * x1, yv[1], cb[1], cr[1]);
        ycc(r1 + 3 * x0, yv[2], cb[2], cr[2]);
        ycc(r1 + 3 * x1, yv[3], cb[3], cr[3]);
        const int cy = mrow * 8 + qy;
        if (cy > ch_last) {                                   // below the frame: the last chroma row again
            const int c0 = min(2 * ch_last, a.h - 1), c1 = min(2 * ch_last + 1, a.h - 1);
            const uint8_t *q0 = src + (long long)c0 * a.stride, *q1 = src + (long long)c1 * a.stride;
            int t;
            ycc(q0 + 3 * x0, t, cb[0], cr[0]);
            ycc(q0 + 3 * x1, t, cb[1], cr[1]);
            ycc(q1 + 3 * x0, t, cb[2], cr[2]);
            ycc(q1 + 3 * x1, t, cb[3], cr[3]);
        }
        const int bias = 1 + (qx & 1);                        // (a chunk starts at an even chroma column)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ly = 2 * qy + (i >> 1), lx = 2 * qx + (i & 1);
            const int blk = mc * 6 + (ly >> 3) * 2 + ((lx >> 3) & 1);
            s_ws[blk * JP_BSTRIDE + (ly & 7) * 8 + (lx & 7)] = yv[i] - 128;
        }
        const int cpos = qy * 8 + (qx & 7);
        s_ws[(mc * 6 + 4) * JP_BSTRIDE + cpos] = ((cb[0] + cb[1] + cb[2] + cb[3] + bias) >> 2) - 128;
        s_ws[(mc * 6 + 5) * JP_BSTRIDE + cpos] = ((cr[0] + cr[1] + cr[2] + cr[3] + bias) >> 2) - 128;
    }
    __syncthreads();

    // ---- row pass ----
    for (int t = tid; t < nblk * 8; t += JP_THREADS) {
        int *p = s_ws + (t >> 3) * JP_BSTRIDE + (t & 7) * 8;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = p[i];
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = d[i];
    }
    __syncthreads();

    // ---- column pass, quantisation, zigzag ----
    for (int t = tid; t < nblk * 8; t += JP_THREADS) {
        const int blk = t >> 3, c = t & 7, k = blk % 6, m = m0 + blk / 6;
        const int *p = s_ws + blk * JP_BSTRIDE + c;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = p[i * 8];
        fdct8<false>(d);
        const bool dummy = k < 4 && (2 * m + (k & 1) >= wb || 2 * mrow + (k >> 1) >= hb);
        const uint16_t *qd = a.tab->qdiv[k >= 4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int nat = i * 8 + c;
            const unsigned qv = qd[nat], mag = (unsigned)(d[i] < 0 ? -d[i] : d[i]);
            int v = (int)((mag + (qv >> 1)) / qv);
            v = d[i] < 0 ? -v : v;
            v = max(nat == 0 ? -1024 : -1023, min(v, 1023));
            s_out[blk * 64 + a.tab->zzpos[nat]] = (int16_t)(dummy ? 0 : v);
        }
    }
    __syncthreads();

    // ---- dummy luminance blocks take the DC of the block before them in the MCU ----
    if (tid < nm) {
        int16_t *mcu = s_out + tid * 6 * 64;
        const bool col1 = 2 * (m0 + tid) + 1 < wb, row1 = 2 * mrow + 1 < hb;
        if (!col1) mcu[64] = mcu[0];
        if (!row1) {
            mcu[128] = mcu[64];
            mcu[192] = mcu[64];
        } else if (!col1) {
            mcu[192] = mcu[128];
        }
    }
    __syncthreads();

    uint4 *dst = (uint4 *)(a.coef + (long long)blockIdx.z * a.coef_frame + ((long long)mrow * a.mcus_x + m0) * 384);
    const uint4 *so = (const uint4 *)s_out;
    for (int i = tid; i < nblk * 8; i += JP_THREADS) dst[i] = so[i];
}

// exclusive prefix sum of v over the workgroup; two barriers
__device__ __forceinline__ uint32_t jp_scan(uint32_t v, uint32_t *s_w, uint32_t &total) {
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
    for (int w = 0; w < JP_WAVES; ++w) {
        const uint32_t s = s_w[w];
        if (w < wave) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + incl - v;
}

__device__ __forceinline__ int jp_nbits(int v) { return 32 - __clz(v < 0 ? -v : v); }     // 0 for 0

// the symbols of one block, in order, handed to put(code, length)
template <class Put>
__device__ __forceinline__ void walk_block(const int16_t *p, int pred, const uint32_t *dc, const uint32_t *ac, Put &put) {
    const uint32_t zrl = ac[0xF0], eob = ac[0x00];
    int run = 0;
    for (int g = 0; g < 8; ++g) {
        const uint4 q = ((const uint4 *)p)[g];
        const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(int16_t)(wds[j >> 1] >> (16 * (j & 1)));
            if (g == 0 && j == 0) {
                const int diff = c - pred, n = jp_nbits(diff);
                const uint32_t e = dc[n];
                put(e & 0xffffu, (int)(e >> 16));
                if (n) put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
            } else if (c == 0) {
                ++run;
            } else {
                for (; run > 15; run -= 16) put(zrl & 0xffffu, (int)(zrl >> 16));
                const int n = jp_nbits(c);
                const uint32_t e = ac[(run << 4) | n];
                put(e & 0xffffu, (int)(e >> 16));
                put((uint32_t)(c < 0 ? c - 1 : c) & ((1u << n) - 1u), n);
                run = 0;
            }
        }
    }
    if (run > 0) put(eob & 0xffffu, (int)(eob >> 16));
}

struct BitCount {
    uint32_t bits = 0;
    __device__ __forceinline__ void operator()(uint32_t, int len) { bits += (uint32_t)len; }
};

// MSB-first bits into LDS words (bit p of the chunk = bit 31 - (p & 31) of word p >> 5); a word may be shared with the neighbours
struct BitDeposit {
    uint32_t *buf;
    unsigned long long acc = 0;
    int n, wi;
    __device__ __forceinline__ BitDeposit(uint32_t *b, uint32_t start) : buf(b), n((int)(start & 31u)), wi((int)(start >> 5)) {}
    __device__ __forceinline__ void operator()(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            atomicOr(&buf[wi++], (uint32_t)(acc >> (n - 32)));
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0) atomicOr(&buf[wi], (uint32_t)(acc << (32 - n)));
    }
};

template <bool EMIT>
__global__ __launch_bounds__(JP_THREADS) void jpeg_code(CodeArgs a) {
    __shared__ uint32_t s_bits[JP_WORDS];
    __shared__ uint32_t s_ac[2][256];
    __shared__ uint32_t s_dc[2][16];
    __shared__ uint32_t s_w[JP_WAVES];
    const int tid = threadIdx.x, r = blockIdx.x, f = blockIdx.y;
    if (EMIT && !a.fits[f]) return;
    s_ac[0][tid] = a.tab->huff[1][tid];
    s_ac[1][tid] = a.tab->huff[3][tid];
    if (tid < 32) s_dc[tid >> 4][tid & 15] = a.tab->huff[(tid >> 4) * 2][tid & 15];
    __syncthreads();

    const int16_t *base = a.coef + (long long)f * a.coef_frame + (long long)r * a.mcus_x * 384;
    uint8_t *dst = EMIT ? a.out + (long long)f * a.out_stride + a.ioff[(long long)f * a.mcus_y + r] : nullptr;
    uint32_t out_pos = 0, carry_bits = 0, carry_val = 0, ff_mine = 0;

    for (int m0 = 0; m0 < a.mcus_x; m0 += JP_CODE_MCUS) {
        const int nblk = min(JP_CODE_MCUS, a.mcus_x - m0) * 6;
        const bool active = tid < nblk, last = m0 + JP_CODE_MCUS >= a.mcus_x;
        const int b = m0 * 6 + tid, k = tid % 6, chroma = k >= 4;
        const int16_t *p = base + (long long)b * 64;
        int pred = 0;
        if (active) {
            if (k >= 1 && k <= 3) pred = p[-64];
            else if (b >= 6) pred = p[k == 0 ? -3 * 64 : -6 * 64];
        }
        BitCount cnt;
        if (active) walk_block(p, pred, s_dc[chroma], s_ac[chroma], cnt);
        uint32_t total;
        const uint32_t start = carry_bits + jp_scan(cnt.bits, s_w, total);
        uint32_t T = carry_bits + total;
        const int nwords = (int)((T + 31) >> 5) + 1;
        for (int i = tid; i < nwords; i += JP_THREADS) s_bits[i] = (i == 0 && carry_bits) ? carry_val << (32 - carry_bits) : 0u;
        __syncthreads();
        if (active) {
            BitDeposit dep(s_bits, start);
            walk_block(p, pred, s_dc[chroma], s_ac[chroma], dep);
            dep.flush();
        }
        if (last) {                                           // pad the interval with 1-bits
            const uint32_t pad = (8u - (T & 7u)) & 7u;
            if (tid == 0 && pad) atomicOr(&s_bits[T >> 5], ((1u << pad) - 1u) << (32u - (T & 31u) - pad));
            T += pad;
        }
        __syncthreads();
        const uint32_t nbytes = T >> 3;
        for (uint32_t tb = 0; tb < nbytes; tb += 4 * JP_THREADS) {
            const uint32_t i0 = tb + 4 * tid;
            const uint32_t nv = i0 < nbytes ? min(4u, nbytes - i0) : 0u;
            const uint32_t word = nv ? s_bits[i0 >> 2] : 0u;
            uint32_t ff = 0;
            for (uint32_t j = 0; j < nv; ++j) ff += ((word >> (24 - 8 * j)) & 0xffu) == 0xffu;
            if (EMIT) {
                uint32_t tot;
                uint32_t pos = out_pos + 4 * tid + jp_scan(ff, s_w, tot);
                for (uint32_t j = 0; j < nv; ++j) {
                    const uint32_t v = (word >> (24 - 8 * j)) & 0xffu;
                    dst[pos++] = (uint8_t)v;
                    if (v == 0xffu) dst[pos++] = 0;
                }
                out_pos += min((uint32_t)(4 * JP_THREADS), nbytes - tb) + tot;
            } else {
                ff_mine += ff;
            }
        }
        if (!EMIT) out_pos += nbytes;
        carry_bits = T & 7u;
        carry_val = carry_bits ? ((s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3u))) & 0xffu) >> (8 - carry_bits) : 0u;
        __syncthreads();                                      // every thread has read its words and the carry
    }
    if (EMIT) {
        if (tid == 0) {
            dst[out_pos] = 0xff;
            dst[out_pos + 1] = (uint8_t)(r + 1 < a.mcus_y ? 0xd0 + (r & 7) : 0xd9);
        }
    } else {
        uint32_t tot;
        jp_scan(ff_mine, s_w, tot);
        if (tid == 0) a.ilen[(long long)f * a.mcus_y + r] = out_pos + tot;
    }
}

// per frame: interval offsets (each interval is followed by 2 marker bytes, the last by EOI), the file size, fits
__global__ __launch_bounds__(JP_THREADS) void jpeg_offsets(OffArgs a) {
    __shared__ uint32_t s_w[JP_WAVES];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int per = (a.mcus_y + JP_THREADS - 1) / JP_THREADS, i0 = tid * per, i1 = min(i0 + per, a.mcus_y);
    const uint32_t *len = a.ilen + (long long)f * a.mcus_y;
    unsigned long long mine = 0;
    for (int i = i0; i < i1; ++i) mine += (unsigned long long)len[i] + 2ull;
    uint32_t total;
    uint32_t off = jp_scan((uint32_t)mine, s_w, total);       // (<= 8192 x 8192: a scan stays below 2^32 bytes)
    for (int i = i0; i < i1; ++i) {
        a.ioff[(long long)f * a.mcus_y + i] = off;
        off += len[i] + 2u;
    }
    if (tid == 0) {
        a.sizes[f] = a.hdr + total;
        a.fits[f] = (unsigned long long)total <= a.cap ? 1u : 0u;
    }
}

// ======================================================================================
// host side: tables and the header
// ======================================================================================
static void quant_tables(int quality, uint8_t ql[64], uint8_t qc[64]) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        ql[i] = (uint8_t)std::min(std::max((kLumaQ[i] * s + 50) / 100, 1), 255);
        qc[i] = (uint8_t)std::min(std::max((kChromaQ[i] * s + 50) / 100, 1), 255);
    }
}

static void huff_codes(const uint8_t *bits, const uint8_t *vals, uint32_t *out) {      // T.81 Annex C
    memset(out, 0, 256 * sizeof(uint32_t));
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = code++ | (uint32_t)len << 16;
        code <<= 1;
    }
}

static void put_segment(std::vector<uint8_t> &o, int marker, const std::vector<uint8_t> &payload) {
    const size_t len = payload.size() + 2;
    o.push_back(0xff); o.push_back((uint8_t)marker); o.push_back((uint8_t)(len >> 8)); o.push_back((uint8_t)len);
    o.insert(o.end(), payload.begin(), payload.end());
}

static std::vector<uint8_t> make_header(int quality, int h, int w) {
    uint8_t ql[64], qc[64];
    quant_tables(quality, ql, qc);
    std::vector<uint8_t> o = {0xff, 0xd8};
    put_segment(o, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        std::vector<uint8_t> p(1, (uint8_t)t);
        for (int i = 0; i < 64; ++i) p.push_back((t ? qc : ql)[kZigzag[i]]);
        put_segment(o, 0xdb, p);
    }
    put_segment(o, 0xc0, {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    const struct { int tc; const uint8_t *bits, *vals; int n; } T[4] = {{0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162},
                                                                       {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
    for (const auto &t : T) {
        std::vector<uint8_t> p(1, (uint8_t)t.tc);
        p.insert(p.end(), t.bits, t.bits + 16);
        p.insert(p.end(), t.vals, t.vals + t.n);
        put_segment(o, 0xc4, p);
    }
    const int ri = cdiv(w, 16);
    put_segment(o, 0xdd, {(uint8_t)(ri >> 8), (uint8_t)ri});
    put_segment(o, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return o;
}

static void make_tables(int quality, JpegTables &t) {
    memset(&t, 0, sizeof(t));
    uint8_t ql[64], qc[64];
    quant_tables(quality, ql, qc);
    for (int i = 0; i < 64; ++i) {
        t.qdiv[0][i] = (uint16_t)(8 * ql[i]);
        t.qdiv[1][i] = (uint16_t)(8 * qc[i]);
        t.zzpos[kZigzag[i]] = (uint8_t)i;
    }
    huff_codes(kDcLumaBits, kDcVals, t.huff[0]);
    huff_codes(kAcLumaBits, kAcLumaVals, t.huff[1]);
    huff_codes(kDcChromaBits, kDcVals, t.huff[2]);
    huff_codes(kAcChromaBits, kAcChromaVals, t.huff[3]);
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_jpeg : HandleBase {
    int quality = 95, max_h = 0, max_w = 0, max_batch = 0;
    EventTimer<2> timer;
    JpegTables *d_tab = nullptr;
    int16_t *d_coef = nullptr;
    uint32_t *d_ilen = nullptr, *d_ioff = nullptr, *d_sizes = nullptr, *d_fits = nullptr;
    uint64_t *d_ptrs = nullptr, *h_ptrs = nullptr;          // h_*: page-locked
    uint32_t *h_sizes = nullptr;
    FrameStage stage;                                       // host frames staged on the device
    uint8_t *d_out = nullptr;                               // the scans before they go to the host
    size_t out_cap = 0;
};

extern "C" {

int rtmodt_jpeg_header(int quality, int h, int w, uint8_t *out, size_t out_bytes, size_t *needed) {
    RT_CHECK(needed, RTMODT_E_INVALID, "null argument");
    RT_CHECK(quality >= 1 && quality <= 100, RTMODT_E_INVALID, "quality %d outside 1..100", quality);
    RT_CHECK(h >= 1 && w >= 1 && h <= JP_MAX_DIM && w <= JP_MAX_DIM, RTMODT_E_INVALID, "bad frame geometry %dx%d (1..%d)", w, h, JP_MAX_DIM);
    const std::vector<uint8_t> hd = make_header(quality, h, w);
    *needed = hd.size();
    if (out && out_bytes >= hd.size()) memcpy(out, hd.data(), hd.size());
    return RTMODT_OK;
}

void rtmodt_jpeg_destroy(rtmodt_jpeg *j) {
    if (!j) return;
    handle_close(j, [&] {
        hipFree(j->d_tab); hipFree(j->d_coef); hipFree(j->d_ilen); hipFree(j->d_ioff); hipFree(j->d_sizes); hipFree(j->d_fits);
        hipFree(j->d_ptrs); j->stage.release(); hipFree(j->d_out);
        hipHostFree(j->h_ptrs); hipHostFree(j->h_sizes);
        j->timer.destroy();
    });
    delete j;
}

int rtmodt_jpeg_create(int device, const rtmodt_jpeg_cfg *cfg, rtmodt_jpeg **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    const int quality = cfg->quality == 0 ? 95 : cfg->quality;
    RT_CHECK(quality >= 1 && quality <= 100, RTMODT_E_INVALID, "quality %d outside 1..100", cfg->quality);
    RT_CHECK(cfg->subsampling == 0, RTMODT_E_UNSUPPORTED, "subsampling %d: only 0 (4:2:0) is implemented", cfg->subsampling);
    RT_CHECK(cfg->max_h >= 1 && cfg->max_w >= 1 && cfg->max_h <= JP_MAX_DIM && cfg->max_w <= JP_MAX_DIM, RTMODT_E_INVALID,
             "max frame %dx%d outside 1..%d", cfg->max_w, cfg->max_h, JP_MAX_DIM);
    RT_CHECK(cfg->max_batch >= 1 && cfg->max_batch <= 65535, RTMODT_E_INVALID, "max_batch %d outside 1..65535", cfg->max_batch);
    rtmodt_jpeg *j = new rtmodt_jpeg();
    j->device = device; j->quality = quality; j->max_h = cfg->max_h; j->max_w = cfg->max_w; j->max_batch = cfg->max_batch;
    auto body = [&]() -> int {
        RT_TRY(handle_open(j));
        RT_TRY(j->timer.create());
        const size_t rows = (size_t)cdiv(j->max_h, 16), mcus = rows * cdiv(j->max_w, 16), nb = (size_t)j->max_batch;
        RT_HIP(hipMalloc((void **)&j->d_tab, sizeof(JpegTables)));
        RT_HIP(hipMalloc((void **)&j->d_coef, nb * mcus * 384 * sizeof(int16_t)));
        RT_HIP(hipMalloc((void **)&j->d_ilen, nb * rows * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&j->d_ioff, nb * rows * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&j->d_sizes, nb * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&j->d_fits, nb * sizeof(uint32_t)));
        RT_HIP(hipMalloc((void **)&j->d_ptrs, nb * sizeof(uint64_t)));
        RT_HIP(hipHostMalloc((void **)&j->h_ptrs, nb * sizeof(uint64_t), hipHostMallocDefault));
        RT_HIP(hipHostMalloc((void **)&j->h_sizes, nb * sizeof(uint32_t), hipHostMallocDefault));
        JpegTables t;
        make_tables(quality, t);
        RT_HIP(hipMemcpy(j->d_tab, &t, sizeof(t), hipMemcpyHostToDevice));
        return RTMODT_OK;
    };
    return handle_created(body(), j, rtmodt_jpeg_destroy, out);
}

int rtmodt_jpeg_encode_batch(rtmodt_jpeg *j, const uint8_t *const *frames, int n, int h, int w, int stride_bytes, int mem_kind, uint8_t *out,
                             size_t slot_bytes, uint32_t *sizes) {
    RT_CHECK(j && n >= 0 && (n == 0 || (frames && out && sizes)), RTMODT_E_INVALID, "bad argument");
    RT_TRY(check_frames(frames, n, h, w, stride_bytes, mem_kind, kJpegFrames));
    RT_CHECK(n <= j->max_batch && h <= j->max_h && w <= j->max_w, RTMODT_E_CAPACITY,
             "%d frames of %dx%d: the handle was made for %d frames of %dx%d", n, w, h, j->max_batch, j->max_w, j->max_h);
    j->timer.timed = false;
    if (n == 0) return RTMODT_OK;
    RT_HIP(hipSetDevice(j->device));
    const std::vector<uint8_t> hd = make_header(j->quality, h, w);
    const size_t hdr = hd.size();
    const int mcus_x = cdiv(w, 16), mcus_y = cdiv(h, 16);
    // staging of the scans (+ markers, EOI): never more than a frame can need, never more than the caller's slot takes
    const size_t worst = (size_t)mcus_x * mcus_y * 6 * JP_BLOCK_BYTES + 2 * (size_t)mcus_y;
    const size_t cap = slot_bytes > hdr ? std::min(slot_bytes - hdr, worst) : 0;
    const size_t out_stride = align_up(std::max<size_t>(cap, 16), 16);
    RT_TRY(dev_grow(&j->d_out, &j->out_cap, (size_t)n * out_stride));
    RT_TRY(j->stage.place(n, h, w, stride_bytes, mem_kind, FRAMES_TIGHT16));
    RT_HIP(hipStreamSynchronize(j->stream));               // the pinned buffers may still feed the previous call's copies
    for (int i = 0; i < n; ++i) j->h_ptrs[i] = (uint64_t)(uintptr_t)j->stage.at(frames, i);
    RT_HIP(hipMemcpyAsync(j->d_ptrs, j->h_ptrs, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, j->stream));
    RT_TRY(j->stage.copy_in(frames, j->stream));

    DctArgs da{};
    da.frames = j->d_ptrs; da.tab = j->d_tab; da.coef = j->d_coef;
    da.stride = (long long)j->stage.pitch;
    da.coef_frame = (long long)mcus_x * mcus_y * 384;
    da.h = h; da.w = w; da.mcus_x = mcus_x; da.mcus_y = mcus_y;
    CodeArgs ca{};
    ca.coef = j->d_coef; ca.tab = j->d_tab; ca.ilen = j->d_ilen; ca.ioff = j->d_ioff; ca.fits = j->d_fits; ca.out = j->d_out;
    ca.coef_frame = da.coef_frame; ca.out_stride = (long long)out_stride; ca.mcus_x = mcus_x; ca.mcus_y = mcus_y;
    OffArgs oa{};
    oa.ilen = j->d_ilen; oa.ioff = j->d_ioff; oa.sizes = j->d_sizes; oa.fits = j->d_fits; oa.mcus_y = mcus_y; oa.hdr = (uint32_t)hdr;
    oa.cap = cap;
    RT_TRY(j->timer.record(0, j->stream));
    hipLaunchKernelGGL(jpeg_dct, dim3(cdiv(mcus_x, JP_DCT_MCUS), mcus_y, n), dim3(JP_THREADS), 0, j->stream, da);
    hipLaunchKernelGGL(jpeg_code<false>, dim3(mcus_y, n), dim3(JP_THREADS), 0, j->stream, ca);
    hipLaunchKernelGGL(jpeg_offsets, dim3(n), dim3(JP_THREADS), 0, j->stream, oa);
    hipLaunchKernelGGL(jpeg_code<true>, dim3(mcus_y, n), dim3(JP_THREADS), 0, j->stream, ca);
    RT_HIP(hipGetLastError());
    RT_TRY(j->timer.record(1, j->stream));
    RT_HIP(hipMemcpyAsync(j->h_sizes, j->d_sizes, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, j->stream));
    RT_HIP(hipStreamSynchronize(j->stream));
    j->timer.timed = true;
    int first_bad = -1;
    for (int i = 0; i < n; ++i) {
        sizes[i] = j->h_sizes[i];
        if ((size_t)sizes[i] > slot_bytes || (size_t)sizes[i] - hdr > cap) {
            if (first_bad < 0) first_bad = i;
            continue;
        }
        uint8_t *slot = out + (size_t)i * slot_bytes;
        memcpy(slot, hd.data(), hdr);
        RT_HIP(hipMemcpyAsync(slot + hdr, j->d_out + (size_t)i * out_stride, (size_t)sizes[i] - hdr, hipMemcpyDeviceToHost, j->stream));
    }
    RT_HIP(hipStreamSynchronize(j->stream));
    RT_CHECK(first_bad < 0, RTMODT_E_CAPACITY, "frame %d needs %u bytes, the slot holds %zu", first_bad, sizes[first_bad], slot_bytes);
    return RTMODT_OK;
}

int rtmodt_jpeg_last_ms(rtmodt_jpeg *j, float *kernel_ms) {
    RT_CHECK(j && kernel_ms, RTMODT_E_INVALID, "null argument");
    return j->timer.elapsed(j->device, 0, 1, kernel_ms, "no encode_batch has run a kernel yet");
}

}  // extern "C"
