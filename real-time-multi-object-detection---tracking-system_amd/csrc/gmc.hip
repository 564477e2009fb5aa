// gmc.hip -- the camera-motion warp BoT-SORT compensates with (botsort.hip: `warp`), estimated from two consecutive BGR24 frames that
// are already on the device: the 2x3 similarity (rotation, uniform scale, translation) from the previous frame to the current one,
// per stream, in full-resolution pixel coordinates.  The rules are this project's own, restated in tests/gmc_ref.py; the kernels equal
// that restatement bit for bit.  PARITY UNPINNED: OpenCV and BoT-SORT's GMC (sparse optical flow / ORB / ECC, then
// estimateAffinePartial2D) are installed nowhere this runs; DESIGN.md section 23 lists the deliberate differences.
//
// One call = six launches for all streams, whatever the frame, block and box counts:
//   gmc_luma_l0        streams x tiles     luma, L0; clears the coarse table
//   gmc_l1             streams x tiles     L1
//   gmc_coarse_sad     streams x row tiles the coarse SAD table (integer vector atomics: the order of an integer sum is free)
//   gmc_coarse_argmin  one wave a stream   the coarse shift
//   gmc_blocks         one wave a block    previous block and current window in LDS, v_sad_u8 on four pixels an instruction
//   gmc_fit            one workgroup a stream   compaction, hypotheses, integer sums, fit, output
// Which of a stream's two pyramid buffers is the previous one is host state (the calls of a handle are ordered), so there is no
// swap on the device.  Every sum is an integer sum:
//   luma      Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 (jpeg.hip's Y)
//   L0        (sum of Y over a d x d cell + d d / 2) / (d d); W0 = w / d, H0 = h / d, partial right and bottom cells dropped
//   L1        (sum of L0 over 4 x 4 + 8) >> 4; W1 = W0 / 4, H1 = H0 / 4.  Both levels of the previous frame stay on the device
//   first     the first frame after create or reset stores the pyramid: identity, status FIRST (1)
//   coarse    SAD(dx, dy) = sum |L1prev(x, y) - L1cur(x + dx, y + dy)| over cs <= x < W1 - cs, cs <= y < H1 - cs, |dx|, |dy| <= cs =
//             coarse_search (0..16: 8 by default; beyond 8 for cameras that move more than 32 d pixels a frame); argmin, ties to the smallest dx^2 + dy^2, then the smaller dy, then the smaller dx.  The smallest
//             frame accepted has W1 >= 2 cs + 4 and H1 >= 2 cs + 4 (an interior of 4 x 4); below that RTMODT_E_INVALID
//   blocks    L0prev in 16 x 16 blocks, raster order, BX = W0 / 16, BY = H0 / 16 (a partial block row or column is dropped).  Block
//             (bx, by) at (x0, y0) = 16 (bx, by) is searched in L0cur at (x0, y0) + 4 coarse + (dx, dy), |dx|, |dy| <= search, same
//             SAD and tie rule.  reason = the first that holds of: 1 the search window leaves the image (nothing is searched: dx =
//             dy = off = sad = 0); 2 sum |I(x+1) - I(x)| or sum |I(y+1) - I(y)| inside the previous block < min_texture; 3 best SAD
//             > max_sad; 4 the best shift is on the border of the search square; 5 the block's rectangle [16 d bx, 16 d (bx + 1)) x
//             [16 d by, 16 d (by + 1)) meets a mask box (x1 < X1 && x2 > X0 && y1 < Y1 && y2 > Y0 in float32) with conf >=
//             mask_conf; else 0, valid
//   sub-pixel per axis, from S-, S0, S+ around a best shift that is not on the border: den = S- - 2 S0 + S+; off = 0 when den <= 0
//             or S0 == 0 (an exact match has no sub-pixel part), else 8 (S- - S+) / den as an integer division rounded half away
//             from zero, clamped to +-8: 1/16 of an L0 pixel
//   points    per axis P = 16 d x0 + 128 d - 8 (the block's centre), Q = P + d (16 (4 coarse + shift) + off), in 1/16 pixel
//   compact   the valid blocks in block order: N correspondences.  N < min_blocks: identity, status FEW_BLOCKS (2)
//   draw      hypothesis k < n_hyp: x = seed + 0x9E3779B9 k; x = 1664525 x + 1013904223; i = (x >> 16) % N; x = 1664525 x +
//             1013904223; j = (x >> 16) % (N - 1), j += 1 when j >= i (all mod 2^32).  Rejected (score -1) when |Pj - Pi|^2 <
//             (16 min_sep)^2.  No state survives a call
//   model     float64, one rounding per operation (FMA contraction off): with dp = Pj - Pi, dq = Qj - Qi exact integers, a =
//             (dp . dq) / |dp|^2, b = (dp x dq) / |dp|^2; tx = Qix - (a Pix - b Piy); ty = Qiy - (b Pix + a Piy)
//   score     the correspondences with rx = ((a Px - b Py) + tx) - Qx, ry = ((b Px + a Py) + ty) - Qy, rx rx + ry ry <= (16
//             inlier_px)^2.  The best score wins, ties to the lowest k.  Best < min_inliers: identity, FEW_INLIERS (3)
//   refit     over the inliers of the winner, from N, SPx, SPy, SQx, SQy, S(P.Q), S(PxQ), S|P|^2 in int64: A = N S(P.Q) - (SPx SQx
//             + SPy SQy), B = N S(PxQ) - (SPx SQy - SPy SQx), D = N S|P|^2 - (SPx^2 + SPy^2); a = A / D, b = B / D; tx = (SQx - (a
//             SPx - b SPy)) / N, ty = (SQy - (b SPx + a SPy)) / N in float64.  Then the inliers of that model, and the same once
//             more.  Fewer than min_inliers inliers in a round, or D <= 0: identity, FEW_INLIERS.
//             Bound at 3840 x 2160 with 4096 blocks: |P|, |Q| < 2^16 per axis (16 x 3840 = 61440, and a window inside the image
//             keeps Q there), N <= 2^12, so SPx < 2^28, S(P.Q), S|P|^2 < 2^12 x 2 x 2^32 = 2^45, N S(.) < 2^57, SPx SQx + SPy SQy
//             < 2^57: every term and every difference stays below 2^58 < 2^63
//   scale     a a + b b outside [0.25, 4] (scale outside [0.5, 2]): identity, BAD_SCALE (4)
//   result    float32 of [a, 0 - b, tx / 16; b, a, ty / 16] (0 - b: no rotation gives +0, the identity's bits): what rtmodt_botsort_update_* take and rtmodt_botsort_check_warp accepts
// Limits: 64 streams, 4096 blocks a stream, frames up to 3840 x 2160, 1024 mask boxes a stream; beyond them RTMODT_E_CAPACITY before
// anything is launched, never a fault.  Every index a kernel forms from device data is clamped.
#include <vector>

#include "track_host.h"
#include "frame_stage.h"

#include <cmath>

namespace rtmodt {

#include "wg_dev.h"

constexpr int GMC_MAX_STREAMS = 64, GMC_MAX_BLOCKS = 4096, GMC_MAX_W = 3840, GMC_MAX_H = 2160, GMC_MAX_HYP = 256, GMC_MAX_BOXES = 1024;
constexpr int GMC_MAX_CS = 16, GMC_MAX_SR = 8, GMC_TABLE = (2 * GMC_MAX_CS + 1) * (2 * GMC_MAX_CS + 1), GMC_BLK_TABLE = (2 * GMC_MAX_SR + 1) * (2 * GMC_MAX_SR + 1);
constexpr int GMC_ROWS = 4;                                   // interior L1 rows a coarse workgroup takes
constexpr int GMC_MAX_W1 = GMC_MAX_W / 4;                     // d = 1
constexpr int GMC_WIN_DW = 9;                                 // dwords a window row holds in LDS: 16 + 2 x 8 pixels and one dword of slack
constexpr int GMC_FIT_THREADS = 1024, GMC_FIT_WAVES = 16;
enum { GMC_OK = 0, GMC_FIRST = 1, GMC_FEW_BLOCKS = 2, GMC_FEW_INLIERS = 3, GMC_BAD_SCALE = 4 };

struct GmcArgs {
    AppFrames frames; int h, w, pitch, d;
    int W0, H0, W1, H1, BX, BY, nb;
    int cs, sr, min_texture, max_sad; float mask_conf;
    int n_hyp; uint32_t seed; double sep2, thr2; int min_blocks, min_inliers;
    uint8_t *l0, *l1; size_t l0_bytes, l1_bytes;             // [stream][2][l0_bytes], [stream][2][l1_bytes]
    uint8_t state[GMC_MAX_STREAMS];                          // bit 0: the buffer this frame is written to, bit 1: a previous frame exists
    uint32_t *table; int32_t *coarse;                        // [stream][GMC_TABLE], [stream][2]
    int32_t *blk;                                            // [stream][6][nb]: reason, dx, dy, offx, offy, sad
    const float4 *mbox; const float *mconf; const int32_t *mn; int mstride, mmax;
    int32_t *order, *nvalid, *scores, *bestk; uint8_t *inl; int64_t *sums; double *model;     // [stream][nb], [stream], [stream][256], [stream], [stream][2][nb], [stream][16], [stream][12]
    float *warp; int32_t *status;                            // [stream][6], [stream]
};

__device__ __forceinline__ const uint8_t *gmc_level(const uint8_t *base, size_t bytes, int s, int which) { return base + ((size_t)s * 2 + which) * bytes; }

__global__ __launch_bounds__(256) void gmc_luma_l0(GmcArgs a) {
    const int s = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < GMC_TABLE; k += 256) a.table[(size_t)s * GMC_TABLE + k] = 0;
    if (idx >= a.W0 * a.H0) return;
    const int x = idx % a.W0, y = idx / a.W0, d = a.d;
    const uint8_t *f = a.frames.p[s] + (size_t)y * d * a.pitch + (size_t)x * d * 3;
    int sum = 0;
    for (int r = 0; r < d; ++r) {
        const uint8_t *p = f + (size_t)r * a.pitch;
        if (d == 4 && ((uintptr_t)p & 3) == 0) {             // twelve bytes as three dwords
            const uint32_t w0 = ((const uint32_t *)p)[0], w1 = ((const uint32_t *)p)[1], w2 = ((const uint32_t *)p)[2];
            const int px[12] = {(int)(w0 & 255), (int)(w0 >> 8 & 255), (int)(w0 >> 16 & 255), (int)(w0 >> 24), (int)(w1 & 255), (int)(w1 >> 8 & 255),
                                (int)(w1 >> 16 & 255), (int)(w1 >> 24), (int)(w2 & 255), (int)(w2 >> 8 & 255), (int)(w2 >> 16 & 255), (int)(w2 >> 24)};
#pragma unroll
            for (int c = 0; c < 4; ++c) sum += (19595 * px[3 * c + 2] + 38470 * px[3 * c + 1] + 7471 * px[3 * c] + 32768) >> 16;
        } else {
            for (int c = 0; c < d; ++c) sum += (19595 * (int)p[3 * c + 2] + 38470 * (int)p[3 * c + 1] + 7471 * (int)p[3 * c] + 32768) >> 16;
        }
    }
    uint8_t *out = (uint8_t *)gmc_level(a.l0, a.l0_bytes, s, a.state[s] & 1);
    out[idx] = (uint8_t)((sum + d * d / 2) / (d * d));
}

__global__ __launch_bounds__(256) void gmc_l1(GmcArgs a) {
    const int s = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.W1 * a.H1) return;
    const int x = idx % a.W1, y = idx / a.W1;
    const uint8_t *l0 = gmc_level(a.l0, a.l0_bytes, s, a.state[s] & 1) + (size_t)(4 * y) * a.W0 + 4 * x;
    int sum = 8;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) sum += l0[(size_t)r * a.W0 + c];
    ((uint8_t *)gmc_level(a.l1, a.l1_bytes, s, a.state[s] & 1))[idx] = (uint8_t)(sum >> 4);
}

// (sad, dx^2 + dy^2, dy, dx) as one ordered integer: the tie rule is its minimum
__device__ __forceinline__ unsigned long long gmc_key(uint32_t sad, int dx, int dy) {
    return ((unsigned long long)sad << 22) | ((unsigned long long)(dx * dx + dy * dy) << 12) | ((unsigned long long)(dy + 16) << 6) | (unsigned long long)(dx + 16);
}
__device__ __forceinline__ int gmc_key_dx(unsigned long long k) { return (int)(k & 63) - 16; }
__device__ __forceinline__ int gmc_key_dy(unsigned long long k) { return (int)(k >> 6 & 63) - 16; }
__device__ __forceinline__ unsigned long long gmc_wave_min(unsigned long long k) {
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o);
        k = other < k ? other : k;
    }
    return k;
}

__global__ __launch_bounds__(256) void gmc_coarse_sad(GmcArgs a) {
    __shared__ uint8_t cur_s[(GMC_ROWS + 2 * GMC_MAX_CS) * GMC_MAX_W1];
    __shared__ uint8_t prev_s[GMC_ROWS * GMC_MAX_W1];
    const int s = blockIdx.y, tid = threadIdx.x;
    if (!(a.state[s] & 2)) return;
    const int cs = a.cs, W1 = a.W1, H1 = a.H1, Wi = W1 - 2 * cs, n = 2 * cs + 1;
    const int y0 = cs + GMC_ROWS * blockIdx.x, rows = min(GMC_ROWS, H1 - cs - y0);
    if (rows <= 0 || Wi <= 0 || W1 > GMC_MAX_W1) return;
    const int which = a.state[s] & 1;
    const uint8_t *cur = gmc_level(a.l1, a.l1_bytes, s, which), *prev = gmc_level(a.l1, a.l1_bytes, s, which ^ 1);
    for (int i = tid; i < (rows + 2 * cs) * W1; i += 256) cur_s[i] = cur[(size_t)(y0 - cs) * W1 + i];
    for (int i = tid; i < rows * Wi; i += 256) prev_s[i] = prev[(size_t)(y0 + i / Wi) * W1 + cs + i % Wi];
    __syncthreads();
    for (int k = tid; k < n * n; k += 256) {
        const int dy = k / n, dx = k % n;                    // 0-based
        uint32_t sad = 0;
        for (int r = 0; r < rows; ++r) {
            const uint8_t *p = prev_s + r * Wi, *c = cur_s + (r + dy) * W1 + dx;
            for (int x = 0; x < Wi; ++x) sad += (uint32_t)abs((int)p[x] - (int)c[x]);
        }
        atomicAdd(&a.table[(size_t)s * GMC_TABLE + k], sad);
    }
}

__global__ __launch_bounds__(64) void gmc_coarse_argmin(GmcArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x, cs = a.cs, n = 2 * cs + 1;
    unsigned long long best = ~0ull;
    if (a.state[s] & 2)
        for (int k = lane; k < n * n; k += 64) {
            const unsigned long long key = gmc_key(a.table[(size_t)s * GMC_TABLE + k], k % n - cs, k / n - cs);
            best = key < best ? key : best;
        }
    best = gmc_wave_min(best);
    if (lane == 0) {
        const bool have = (a.state[s] & 2) != 0;
        a.coarse[2 * s] = have ? gmc_key_dx(best) : 0;
        a.coarse[2 * s + 1] = have ? gmc_key_dy(best) : 0;
    }
}

__device__ __forceinline__ int gmc_subpixel(int sm, int s0, int sp) {
    const int den = sm - 2 * s0 + sp;
    if (den <= 0 || s0 == 0) return 0;
    const int num = 8 * (sm - sp), an = num < 0 ? -num : num;
    const int q = (2 * an + den) / (2 * den);
    return max(-8, min(8, num < 0 ? -q : q));
}
__device__ __forceinline__ int gmc_absdiff_bytes(uint32_t x, uint32_t y, int n) {      // the first n byte lanes
    int t = 0;
    for (int k = 0; k < n; ++k) t += abs((int)(x >> (8 * k) & 255) - (int)(y >> (8 * k) & 255));
    return t;
}

__global__ __launch_bounds__(256) void gmc_blocks(GmcArgs a) {
    __shared__ uint32_t prev_s[4][64];
    __shared__ uint32_t win_s[4][(16 + 2 * GMC_MAX_SR) * GMC_WIN_DW];
    __shared__ int sad_s[4][GMC_BLK_TABLE];
    const int s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (!(a.state[s] & 2)) return;                            // the whole workgroup: one stream
    const int nb = a.nb, W0 = a.W0, H0 = a.H0, sr = a.sr, n = 2 * sr + 1, d = a.d;
    const int b = blockIdx.x * 4 + wave, bc = min(b, nb - 1);
    const bool active = b < nb;
    const int bx = bc % a.BX, by = bc / a.BX, x0 = 16 * bx, y0 = 16 * by;
    const int cx = 4 * max(-GMC_MAX_CS, min(GMC_MAX_CS, a.coarse[2 * s])), cy = 4 * max(-GMC_MAX_CS, min(GMC_MAX_CS, a.coarse[2 * s + 1]));
    const int wx0 = x0 + cx - sr, wy0 = y0 + cy - sr;
    const bool inwin = wx0 >= 0 && wy0 >= 0 && wx0 + 2 * sr + 16 <= W0 && wy0 + 2 * sr + 16 <= H0;
    const int which = a.state[s] & 1;
    const uint8_t *cur = gmc_level(a.l0, a.l0_bytes, s, which), *prev = gmc_level(a.l0, a.l0_bytes, s, which ^ 1);
    {   // the previous block: lane = row * 4 + dword
        const uint8_t *p = prev + (size_t)(y0 + (lane >> 2)) * W0 + x0 + 4 * (lane & 3);
        prev_s[wave][lane] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    const int wrows = 16 + 2 * sr;
    for (int i = lane; i < wrows * GMC_WIN_DW; i += 64) {     // the window, coordinates clamped into the image (the slack is never compared)
        const int r = i / GMC_WIN_DW, dw = i - r * GMC_WIN_DW;
        const uint8_t *row = cur + (size_t)min(max(wy0 + r, 0), H0 - 1) * W0;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= (uint32_t)row[min(max(wx0 + 4 * dw + k, 0), W0 - 1)] << (8 * k);
        win_s[wave][i] = v;
    }
    __syncthreads();
    // ---- texture of the previous block ----
    int gx, gy = 0;
    {
        const uint32_t v = prev_s[wave][lane];
        gx = gmc_absdiff_bytes(v >> 8, v, 3);
        if ((lane & 3) != 3) gx += abs((int)(prev_s[wave][lane + 1] & 255) - (int)(v >> 24));
        if (lane < 60) gy = gmc_absdiff_bytes(prev_s[wave][lane + 4], v, 4);
    }
    for (int o = 32; o >= 1; o >>= 1) { gx += __shfl_xor(gx, o); gy += __shfl_xor(gy, o); }
    // ---- the SAD of every shift: a lane per shift ----
    unsigned long long best = ~0ull;
    for (int k = lane; k < n * n; k += 64) {
        const int dy = k / n, dx = k - dy * n, base = dx >> 2, sh = dx & 3;
        uint32_t acc = 0;
        for (int r = 0; r < 16; ++r) {
            const uint32_t *w = &win_s[wave][(r + dy) * GMC_WIN_DW + base];
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            const uint32_t *p = &prev_s[wave][4 * r];
            acc = __builtin_amdgcn_sad_u8(p[0], __builtin_amdgcn_alignbyte(w1, w0, sh), acc);
            acc = __builtin_amdgcn_sad_u8(p[1], __builtin_amdgcn_alignbyte(w2, w1, sh), acc);
            acc = __builtin_amdgcn_sad_u8(p[2], __builtin_amdgcn_alignbyte(w3, w2, sh), acc);
            acc = __builtin_amdgcn_sad_u8(p[3], __builtin_amdgcn_alignbyte(w4, w3, sh), acc);
        }
        sad_s[wave][k] = (int)acc;
        const unsigned long long key = gmc_key(acc, dx - sr, dy - sr);
        best = key < best ? key : best;
    }
    best = gmc_wave_min(best);
    __syncthreads();
    // ---- the mask: a lane per box ----
    const float X0 = (float)(16 * d * bx), Y0 = (float)(16 * d * by), X1 = (float)(16 * d * (bx + 1)), Y1 = (float)(16 * d * (by + 1));
    const int mn = a.mn ? min(max(a.mn[s], 0), min(a.mstride, a.mmax)) : 0;
    int hit = 0;
    for (int j = lane; j < mn; j += 64) {
        const float4 m = a.mbox[(size_t)s * a.mstride + j];
        if (a.mconf[(size_t)s * a.mstride + j] >= a.mask_conf && m.x < X1 && m.z > X0 && m.y < Y1 && m.w > Y0) hit = 1;
    }
    hit = __any(hit);
    if (lane == 0 && active) {
        int reason = 1, dx = 0, dy = 0, ox = 0, oy = 0, sad = 0;
        if (inwin) {
            dx = gmc_key_dx(best); dy = gmc_key_dy(best);
            dx = max(-sr, min(sr, dx)); dy = max(-sr, min(sr, dy));
            const int *t = sad_s[wave], at = (dy + sr) * n + dx + sr;
            sad = t[at];
            const bool border = dx == -sr || dx == sr || dy == -sr || dy == sr;
            if (!border) { ox = gmc_subpixel(t[at - 1], sad, t[at + 1]); oy = gmc_subpixel(t[at - n], sad, t[at + n]); }
            reason = gx < a.min_texture || gy < a.min_texture ? 2 : sad > a.max_sad ? 3 : border ? 4 : hit ? 5 : 0;
        }
        int32_t *o = a.blk + (size_t)s * 6 * nb + b;
        o[0] = reason; o[nb] = dx; o[2 * nb] = dy; o[3 * nb] = ox; o[4 * nb] = oy; o[5 * nb] = sad;
    }
}

struct GmcModel { double a, b, tx, ty; };
__device__ __forceinline__ bool gmc_inlier(const GmcModel &m, double px, double py, double qx, double qy, double thr2) {
    const double rx = ((m.a * px - m.b * py) + m.tx) - qx, ry = ((m.b * px + m.a * py) + m.ty) - qy;
    return rx * rx + ry * ry <= thr2;
}
__device__ __forceinline__ void gmc_pair(uint32_t seed, int k, int N, int &i, int &j) {
    uint32_t x = seed + 0x9E3779B9u * (uint32_t)k;
    x = 1664525u * x + 1013904223u;
    i = (int)((x >> 16) % (uint32_t)N);
    x = 1664525u * x + 1013904223u;
    j = (int)((x >> 16) % (uint32_t)(N - 1));
    if (j >= i) j += 1;
}
__device__ __forceinline__ GmcModel gmc_two_point(long long pix, long long piy, long long pjx, long long pjy, long long qix, long long qiy, long long qjx,
                                                  long long qjy) {
    const long long dpx = pjx - pix, dpy = pjy - piy, dqx = qjx - qix, dqy = qjy - qiy;
    const double den = (double)(dpx * dpx + dpy * dpy);
    GmcModel m;
    m.a = (double)(dpx * dqx + dpy * dqy) / den;
    m.b = (double)(dpx * dqy - dpy * dqx) / den;
    const double px = (double)pix, py = (double)piy;
    m.tx = (double)qix - (m.a * px - m.b * py);
    m.ty = (double)qiy - (m.b * px + m.a * py);
    return m;
}

__global__ __launch_bounds__(GMC_FIT_THREADS) void gmc_fit(GmcArgs a) {
    __shared__ uint16_t ord_s[GMC_MAX_BLOCKS];
    __shared__ int qx_s[GMC_MAX_BLOCKS], qy_s[GMC_MAX_BLOCKS];
    __shared__ int score_s[GMC_MAX_HYP];
    __shared__ int wsum[GMC_FIT_WAVES];
    __shared__ int pick_s[2];
    __shared__ unsigned long long psum[8];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = min(a.nb, GMC_MAX_BLOCKS), BX = a.BX, d = a.d;
    float *warp = a.warp + 6 * s;
    int32_t *scores = a.scores + (size_t)s * GMC_MAX_HYP;
    uint8_t *inl = a.inl + (size_t)s * 2 * a.nb;
    int64_t *sums = a.sums + (size_t)s * 16;
    double *model = a.model + (size_t)s * 12;
    auto finish = [&](int status, const GmcModel *m) {       // thread 0
        float w[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        if (m) { w[0] = (float)m->a; w[1] = (float)(0.0 - m->b); w[2] = (float)(m->tx / 16.0); w[3] = (float)m->b; w[4] = (float)m->a; w[5] = (float)(m->ty / 16.0); }
        for (int k = 0; k < 6; ++k) warp[k] = w[k];
        a.status[s] = status;
    };
    // ---- defaults of everything a later stage may not reach ----
    for (int k = tid; k < GMC_MAX_HYP; k += GMC_FIT_THREADS) { scores[k] = -1; score_s[k] = -1; }
    for (int k = tid; k < 2 * a.nb; k += GMC_FIT_THREADS) inl[k] = 0;
    if (tid < 16) sums[tid] = 0;
    if (tid < 12) model[tid] = 0.0;
    if (tid == 0) { a.bestk[s] = -1; a.nvalid[s] = 0; }
    if (!(a.state[s] & 2)) {
        if (tid == 0) finish(GMC_FIRST, nullptr);
        return;
    }
    // ---- compaction in block order: four consecutive blocks a thread ----
    const int32_t *blk = a.blk + (size_t)s * 6 * a.nb;
    const int cx = max(-GMC_MAX_CS, min(GMC_MAX_CS, a.coarse[2 * s])), cy = max(-GMC_MAX_CS, min(GMC_MAX_CS, a.coarse[2 * s + 1]));
    int cnt = 0, ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * tid + q;
        ok[q] = i < nb && blk[i] == 0;
        cnt += ok[q];
    }
    int N = 0;
    int pos = block_scan_count<GMC_FIT_WAVES>(cnt, wsum, N);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (ok[q]) {
            const int i = 4 * tid + q;
            const int bx = i % BX, by = i / BX;
            ord_s[pos] = (uint16_t)i;
            qx_s[pos] = 256 * d * bx + 128 * d - 8 + d * (16 * (4 * cx + blk[a.nb + i]) + blk[3 * a.nb + i]);
            qy_s[pos] = 256 * d * by + 128 * d - 8 + d * (16 * (4 * cy + blk[2 * a.nb + i]) + blk[4 * a.nb + i]);
            a.order[(size_t)s * a.nb + pos] = i;
            ++pos;
        }
    if (tid == 0) a.nvalid[s] = N;
    __syncthreads();
    if (N < a.min_blocks || N < 2) {
        if (tid == 0) finish(GMC_FEW_BLOCKS, nullptr);
        return;
    }
    auto Px = [&](int m) { return (long long)(256 * d * ((int)ord_s[m] % BX) + 128 * d - 8); };
    auto Py = [&](int m) { return (long long)(256 * d * ((int)ord_s[m] / BX) + 128 * d - 8); };
    auto hypothesis = [&](int k, GmcModel &m) -> bool {
        int i, j;
        gmc_pair(a.seed, k, N, i, j);
        const long long dx = Px(j) - Px(i), dy = Py(j) - Py(i);
        if ((double)(dx * dx + dy * dy) < a.sep2) return false;
        m = gmc_two_point(Px(i), Py(i), Px(j), Py(j), qx_s[i], qy_s[i], qx_s[j], qy_s[j]);
        return true;
    };
    // ---- hypotheses: a wave each ----
    const int n_hyp = min(a.n_hyp, GMC_MAX_HYP);
    for (int k = wave; k < n_hyp; k += GMC_FIT_WAVES) {
        GmcModel m;
        if (!hypothesis(k, m)) continue;                     // uniform over the wave
        int c = 0;
        for (int q = lane; q < N; q += 64) c += gmc_inlier(m, (double)Px(q), (double)Py(q), (double)qx_s[q], (double)qy_s[q], a.thr2) ? 1 : 0;
        for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) score_s[k] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int best = -1, bk = -1;
        for (int k = 0; k < n_hyp; ++k)
            if (score_s[k] > best) { best = score_s[k]; bk = k; }
        pick_s[0] = best; pick_s[1] = bk;
        a.bestk[s] = bk;
    }
    for (int k = tid; k < GMC_MAX_HYP; k += GMC_FIT_THREADS) scores[k] = score_s[k];
    __syncthreads();
    if (pick_s[0] < a.min_inliers || pick_s[1] < 0) {
        if (tid == 0) finish(GMC_FEW_INLIERS, nullptr);
        return;
    }
    GmcModel m;
    hypothesis(pick_s[1], m);
    if (tid == 0) { model[0] = m.a; model[1] = m.b; model[2] = m.tx; model[3] = m.ty; }
    // ---- two rounds: inliers of the model, integer sums, closed-form refit ----
    for (int rnd = 0; rnd < 2; ++rnd) {
        if (tid < 8) psum[tid] = 0;
        __syncthreads();
        long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = tid; q < N; q += GMC_FIT_THREADS) {
            const long long px = Px(q), py = Py(q), qx = qx_s[q], qy = qy_s[q];
            const bool in = gmc_inlier(m, (double)px, (double)py, (double)qx, (double)qy, a.thr2);
            inl[(size_t)rnd * a.nb + q] = in ? 1 : 0;
            if (in) {
                t[0] += 1; t[1] += px; t[2] += py; t[3] += qx; t[4] += qy; t[5] += px * qx + py * qy; t[6] += px * qy - py * qx; t[7] += px * px + py * py;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            for (int o = 32; o >= 1; o >>= 1) t[k] += __shfl_xor(t[k], o);
            if (lane == 0) atomicAdd(&psum[k], (unsigned long long)t[k]);
        }
        __syncthreads();
        const long long n = (long long)psum[0], spx = (long long)psum[1], spy = (long long)psum[2], sqx = (long long)psum[3], sqy = (long long)psum[4],
                        dot = (long long)psum[5], cross = (long long)psum[6], pp = (long long)psum[7];
        if (tid < 8) sums[8 * rnd + tid] = (long long)psum[tid];
        const long long A = n * dot - (spx * sqx + spy * sqy), B = n * cross - (spx * sqy - spy * sqx), D = n * pp - (spx * spx + spy * spy);
        if (n < a.min_inliers || D <= 0) {
            if (tid == 0) finish(GMC_FEW_INLIERS, nullptr);
            return;
        }
        m.a = (double)A / (double)D;
        m.b = (double)B / (double)D;
        const double fx = (double)spx, fy = (double)spy, nn = (double)n;
        m.tx = ((double)sqx - (m.a * fx - m.b * fy)) / nn;
        m.ty = ((double)sqy - (m.b * fx + m.a * fy)) / nn;
        if (tid == 0) { double *o = model + 4 * (1 + rnd); o[0] = m.a; o[1] = m.b; o[2] = m.tx; o[3] = m.ty; }
        __syncthreads();
    }
    if (tid == 0) {
        const double s2 = m.a * m.a + m.b * m.b;
        if (!(s2 >= 0.25 && s2 <= 4.0)) finish(GMC_BAD_SCALE, nullptr);
        else finish(GMC_OK, &m);
    }
}

}  // namespace rtmodt

using namespace rtmodt;

struct rtmodt_gmc : HandleBase {
    int S = 1;
    rtmodt_gmc_cfg cfg = {};
    hipEvent_t foreign_done = nullptr, own_done = nullptr;
    EventTimer<2> timer;
    bool foreign_pending = false;
    int gh = 0, gw = 0;                                      // the geometry the buffers are carved for (0: none yet)
    int W0 = 0, H0 = 0, W1 = 0, H1 = 0, BX = 0, BY = 0, nb = 0;
    size_t l0_bytes = 0, l1_bytes = 0;
    uint8_t which[GMC_MAX_STREAMS] = {}, have[GMC_MAX_STREAMS] = {};     // the buffer the last frame went to; a previous frame exists
    uint8_t *d_l0 = nullptr, *d_l1 = nullptr, *d_inl = nullptr;
    uint32_t *d_table = nullptr; int32_t *d_coarse = nullptr, *d_blk = nullptr, *d_order = nullptr, *d_nvalid = nullptr, *d_scores = nullptr, *d_bestk = nullptr;
    int64_t *d_sums = nullptr; double *d_model = nullptr;
    float *d_warp = nullptr, *h_warp = nullptr; int32_t *d_status = nullptr, *h_status = nullptr;        // h_*: pinned
    float4 *d_mbox = nullptr; float *d_mconf = nullptr; int32_t *d_mn = nullptr, *h_mn = nullptr;
    FrameStage stage;                                        // host frames
};

static void gmc_free_geometry(rtmodt_gmc *g) {
    hipFree(g->d_l0); hipFree(g->d_l1); hipFree(g->d_blk); hipFree(g->d_order); hipFree(g->d_inl);
    g->d_l0 = g->d_l1 = g->d_inl = nullptr; g->d_blk = g->d_order = nullptr;
    g->gh = g->gw = 0;
}

static int gmc_join(rtmodt_gmc *g) {
    if (g->foreign_pending) {
        RT_HIP(hipStreamWaitEvent(g->stream, g->foreign_done, 0));
        g->foreign_pending = false;
    }
    return RTMODT_OK;
}

// everything a call is refused for, before anything is launched or allocated
static int gmc_check_geometry(const rtmodt_gmc *g, int h, int w, int pitch, int mem_kind) {
    RT_TRY(check_frame_block(g->S, h, w, pitch, mem_kind, kGmcFrames));      // (the size limits are the estimator's own, below)
    RT_CHECK(w <= GMC_MAX_W && h <= GMC_MAX_H, RTMODT_E_CAPACITY, "frame %dx%d: at most %dx%d", w, h, GMC_MAX_W, GMC_MAX_H);
    const int d = g->cfg.downscale, W0 = w / d, H0 = h / d;
    RT_CHECK((W0 / 16) * (H0 / 16) <= GMC_MAX_BLOCKS, RTMODT_E_CAPACITY, "frame %dx%d at downscale %d has %d blocks: at most %d", w, h, d, (W0 / 16) * (H0 / 16),
             GMC_MAX_BLOCKS);
    const int need = 2 * g->cfg.coarse_search + 4;
    RT_CHECK(W0 / 4 >= need && H0 / 4 >= need, RTMODT_E_INVALID, "frame %dx%d at downscale %d: level 1 is %dx%d, the smallest accepted is %dx%d", w, h, d,
             W0 / 4, H0 / 4, need, need);
    bool any = false;
    for (int s = 0; s < g->S; ++s) any |= g->have[s] != 0;
    RT_CHECK(!any || (h == g->gh && w == g->gw), RTMODT_E_INVALID, "frame size changed from %dx%d to %dx%d without a reset", g->gw, g->gh, w, h);
    return RTMODT_OK;
}

static int gmc_set_geometry(rtmodt_gmc *g, int h, int w) {
    if (h == g->gh && w == g->gw) return RTMODT_OK;
    RT_HIP(hipDeviceSynchronize());
    gmc_free_geometry(g);
    const int d = g->cfg.downscale;
    g->W0 = w / d; g->H0 = h / d; g->W1 = g->W0 / 4; g->H1 = g->H0 / 4; g->BX = g->W0 / 16; g->BY = g->H0 / 16; g->nb = g->BX * g->BY;
    g->l0_bytes = align_up((size_t)g->W0 * g->H0, 16); g->l1_bytes = align_up((size_t)g->W1 * g->H1, 16);
    const size_t S = (size_t)g->S, nb = (size_t)g->nb;
    RT_HIP(hipMalloc((void **)&g->d_l0, S * 2 * g->l0_bytes));
    RT_HIP(hipMalloc((void **)&g->d_l1, S * 2 * g->l1_bytes));
    RT_HIP(hipMalloc((void **)&g->d_blk, S * 6 * nb * 4)); RT_HIP(handle_zero(g->d_blk, S * 6 * nb * 4, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_order, S * nb * 4)); RT_HIP(handle_zero(g->d_order, S * nb * 4, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_inl, S * 2 * nb)); RT_HIP(handle_zero(g->d_inl, S * 2 * nb, g->stream));
    RT_TRY(handle_wait(g->stream));                        // (the estimate that follows may run on a detector's stream)
    g->gh = h; g->gw = w;
    return RTMODT_OK;
}

// frames of a call -> device pointers (host frames are staged on stream q)
static int gmc_stage(rtmodt_gmc *g, const uint8_t *const *frames, int count, int h, int w, int pitch, int mem_kind, hipStream_t q, AppFrames *out) {
    RT_TRY(g->stage.in(frames, count, h, w, pitch, mem_kind, q, FRAMES_AS_GIVEN));
    for (int i = 0; i < count; ++i) out->p[i] = g->stage.at(frames, i);
    return RTMODT_OK;
}

// the six launches of one call on stream q for streams [0, count); the masks are device arrays
static int gmc_run(rtmodt_gmc *g, const AppFrames &fp, int count, int h, int w, int pitch, const float4 *mbox, const float *mconf, const int32_t *mn,
                   int mstride, hipStream_t q) {
    GmcArgs a{};
    a.frames = fp; a.h = h; a.w = w; a.pitch = pitch; a.d = g->cfg.downscale;
    a.W0 = g->W0; a.H0 = g->H0; a.W1 = g->W1; a.H1 = g->H1; a.BX = g->BX; a.BY = g->BY; a.nb = g->nb;
    a.cs = g->cfg.coarse_search; a.sr = g->cfg.search; a.min_texture = g->cfg.min_texture; a.max_sad = g->cfg.max_sad; a.mask_conf = g->cfg.mask_conf;
    a.n_hyp = g->cfg.n_hyp; a.seed = g->cfg.seed;
    const double sep = 16.0 * (double)g->cfg.min_sep, thr = 16.0 * (double)g->cfg.inlier_px;
    a.sep2 = sep * sep; a.thr2 = thr * thr; a.min_blocks = g->cfg.min_blocks; a.min_inliers = g->cfg.min_inliers;
    a.l0 = g->d_l0; a.l1 = g->d_l1; a.l0_bytes = g->l0_bytes; a.l1_bytes = g->l1_bytes;
    for (int s = 0; s < count; ++s) {
        g->which[s] ^= 1;
        a.state[s] = (uint8_t)(g->which[s] | (g->have[s] ? 2 : 0));
        g->have[s] = 1;
    }
    a.table = g->d_table; a.coarse = g->d_coarse; a.blk = g->d_blk;
    a.mbox = mbox; a.mconf = mconf; a.mn = mn; a.mstride = mstride; a.mmax = GMC_MAX_BOXES;
    a.order = g->d_order; a.nvalid = g->d_nvalid; a.scores = g->d_scores; a.bestk = g->d_bestk; a.inl = g->d_inl; a.sums = g->d_sums; a.model = g->d_model;
    a.warp = g->d_warp; a.status = g->d_status;
    RT_TRY(g->timer.record(0, q));
    hipLaunchKernelGGL(gmc_luma_l0, dim3(cdiv(a.W0 * a.H0, 256), count), dim3(256), 0, q, a);
    hipLaunchKernelGGL(gmc_l1, dim3(cdiv(a.W1 * a.H1, 256), count), dim3(256), 0, q, a);
    hipLaunchKernelGGL(gmc_coarse_sad, dim3(cdiv(a.H1 - 2 * a.cs, GMC_ROWS), count), dim3(256), 0, q, a);
    hipLaunchKernelGGL(gmc_coarse_argmin, dim3(count), dim3(64), 0, q, a);
    hipLaunchKernelGGL(gmc_blocks, dim3(cdiv(a.nb, 4), count), dim3(256), 0, q, a);
    hipLaunchKernelGGL(gmc_fit, dim3(count), dim3(GMC_FIT_THREADS), 0, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(g->timer.record(1, q));
    g->timer.timed = true;
    return RTMODT_OK;
}

namespace rtmodt {
// botsort.hip: the estimate of det's batch queued on det's stream; *warp_dev = the [stream][6] device buffer gmc_fit writes
int gmc_enqueue_detector(rtmodt_gmc *g, const DetOutputs &o, const uint8_t *const *frames, int n_frames, int h, int w, int pitch, int mem_kind,
                         const float **warp_dev) {
    RT_CHECK(g && frames, RTMODT_E_INVALID, "null argument");
    RT_CHECK(o.device == g->device, RTMODT_E_INVALID, "estimator on device %d, detector on device %d", g->device, o.device);
    RT_CHECK(n_frames == o.count, RTMODT_E_INVALID, "%d frames for the detector's batch of %d", n_frames, o.count);
    RT_CHECK(o.count >= 1 && o.count <= g->S, RTMODT_E_INVALID, "%d frames > estimator streams %d", o.count, g->S);
    RT_CHECK(o.stride <= GMC_MAX_BOXES, RTMODT_E_CAPACITY, "detector max_det %d > %d mask boxes", o.stride, GMC_MAX_BOXES);
    RT_TRY(check_frame_ptrs(frames, n_frames));
    RT_TRY(gmc_check_geometry(g, h, w, pitch, mem_kind));
    RT_HIP(hipSetDevice(g->device));
    RT_TRY(gmc_set_geometry(g, h, w));
    AppFrames fp{};
    RT_TRY(gmc_stage(g, frames, o.count, h, w, pitch, mem_kind, o.stream, &fp));
    RT_TRY(gmc_run(g, fp, o.count, h, w, pitch, o.box, o.conf, o.n, o.stride, o.stream));
    RT_HIP(hipEventRecord(g->foreign_done, o.stream));
    g->foreign_pending = true;
    if (warp_dev) *warp_dev = g->d_warp;
    return RTMODT_OK;
}

// stab.hip: the estimate of caller frames queued on the estimator's own stream, as rtmodt_gmc_estimate_batch queues it, for streams
// [0, n_frames); nothing is fetched and the host does not wait: *done is recorded behind the estimate
int gmc_enqueue_frames(rtmodt_gmc *g, int device, const uint8_t *const *frames, int n_frames, int h, int w, int pitch, int mem_kind, const float *mask_xyxy,
                       const float *mask_conf, const int32_t *mask_n, bool check_only, const float **warp_dev, const int32_t **status_dev,
                       hipEvent_t *done) {
    RT_CHECK(g && frames, RTMODT_E_INVALID, "null argument");
    RT_CHECK(device == g->device, RTMODT_E_INVALID, "estimator on device %d, caller on device %d", g->device, device);
    RT_CHECK(n_frames >= 1 && n_frames <= g->S, RTMODT_E_INVALID, "%d frames > estimator streams %d", n_frames, g->S);
    RT_TRY(check_frame_ptrs(frames, n_frames));
    RT_TRY(gmc_check_geometry(g, h, w, pitch, mem_kind));
    bool any = false;
    if (mask_n)
        for (int s = 0; s < n_frames; ++s) {
            RT_CHECK(mask_n[s] >= 0, RTMODT_E_INVALID, "stream %d: %d mask boxes", s, mask_n[s]);
            RT_CHECK(mask_n[s] <= g->cfg.max_boxes, RTMODT_E_CAPACITY, "stream %d: %d mask boxes > max_boxes %d", s, mask_n[s], g->cfg.max_boxes);
            any |= mask_n[s] > 0;
        }
    RT_CHECK(!any || (mask_xyxy && mask_conf), RTMODT_E_INVALID, "null mask boxes");
    if (check_only) return RTMODT_OK;
    RT_HIP(hipSetDevice(g->device));
    RT_TRY(gmc_join(g));
    RT_TRY(gmc_set_geometry(g, h, w));
    hipStream_t q = g->stream;
    AppFrames fp{};
    RT_TRY(gmc_stage(g, frames, n_frames, h, w, pitch, mem_kind, q, &fp));
    const size_t SM = (size_t)n_frames * g->cfg.max_boxes;
    for (int s = 0; s < g->S; ++s) g->h_mn[s] = mask_n && s < n_frames ? mask_n[s] : 0;
    if (any) {
        RT_HIP(hipMemcpyAsync(g->d_mbox, mask_xyxy, SM * 16, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(g->d_mconf, mask_conf, SM * 4, hipMemcpyHostToDevice, q));
    }
    RT_HIP(hipMemcpyAsync(g->d_mn, g->h_mn, (size_t)g->S * 4, hipMemcpyHostToDevice, q));
    RT_TRY(gmc_run(g, fp, n_frames, h, w, pitch, g->d_mbox, g->d_mconf, g->d_mn, g->cfg.max_boxes, q));
    RT_HIP(hipEventRecord(g->own_done, q));
    if (warp_dev) *warp_dev = g->d_warp;
    if (status_dev) *status_dev = g->d_status;
    if (done) *done = g->own_done;
    return RTMODT_OK;
}
}  // namespace rtmodt

extern "C" {

void rtmodt_gmc_default_cfg(rtmodt_gmc_cfg *cfg) {
    if (!cfg) return;
    *cfg = rtmodt_gmc_cfg{};
    cfg->downscale = 4; cfg->coarse_search = 8; cfg->search = 4; cfg->min_texture = 256; cfg->max_sad = 4096; cfg->mask_conf = 0.1f;
    cfg->n_hyp = 128; cfg->seed = 1; cfg->min_sep = 32.0f; cfg->inlier_px = 1.5f; cfg->min_blocks = 16; cfg->min_inliers = 12;
    cfg->max_boxes = GMC_MAX_BOXES; cfg->n_streams = 1; cfg->device = 0;
}

void rtmodt_gmc_destroy(rtmodt_gmc *g) {
    if (!g) return;
    hipSetDevice(g->device);
    if (g->foreign_done) hipEventSynchronize(g->foreign_done);
    handle_close(g, [&] {
        if (g->foreign_done) hipEventDestroy(g->foreign_done);
        if (g->own_done) hipEventDestroy(g->own_done);
        g->timer.destroy();
        gmc_free_geometry(g);
        hipFree(g->d_table); hipFree(g->d_coarse); hipFree(g->d_nvalid); hipFree(g->d_scores); hipFree(g->d_bestk); hipFree(g->d_sums); hipFree(g->d_model);
        hipFree(g->d_warp); hipFree(g->d_status); hipFree(g->d_mbox); hipFree(g->d_mconf); hipFree(g->d_mn); g->stage.release();
        hipHostFree(g->h_warp); hipHostFree(g->h_status); hipHostFree(g->h_mn);
    });
    delete g;
}

static int gmc_create_impl(rtmodt_gmc *g) {
    RT_TRY(handle_open(g));
    RT_HIP(hipEventCreateWithFlags(&g->foreign_done, hipEventDisableTiming));
    RT_HIP(hipEventCreateWithFlags(&g->own_done, hipEventDisableTiming));
    RT_TRY(g->timer.create());
    const size_t S = (size_t)g->S, MB = (size_t)std::max(g->cfg.max_boxes, 1);
    RT_HIP(hipMalloc((void **)&g->d_table, S * GMC_TABLE * 4)); RT_HIP(handle_zero(g->d_table, S * GMC_TABLE * 4, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_coarse, S * 8)); RT_HIP(handle_zero(g->d_coarse, S * 8, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_nvalid, S * 4)); RT_HIP(handle_zero(g->d_nvalid, S * 4, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_scores, S * GMC_MAX_HYP * 4)); RT_HIP(handle_fill(g->d_scores, 0xff, S * GMC_MAX_HYP * 4, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_bestk, S * 4)); RT_HIP(handle_fill(g->d_bestk, 0xff, S * 4, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_sums, S * 16 * 8)); RT_HIP(handle_zero(g->d_sums, S * 16 * 8, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_model, S * 12 * 8)); RT_HIP(handle_zero(g->d_model, S * 12 * 8, g->stream));
    RT_HIP(hipMalloc((void **)&g->d_warp, S * 6 * 4)); RT_HIP(hipMalloc((void **)&g->d_status, S * 4));
    RT_HIP(hipHostMalloc((void **)&g->h_warp, S * 6 * 4, hipHostMallocDefault)); RT_HIP(hipHostMalloc((void **)&g->h_status, S * 4, hipHostMallocDefault));
    RT_HIP(hipHostMalloc((void **)&g->h_mn, S * 4, hipHostMallocDefault));
    for (size_t s = 0; s < S; ++s) {
        const float id[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        memcpy(g->h_warp + 6 * s, id, sizeof(id));
        g->h_status[s] = GMC_FIRST;
    }
    RT_HIP(hipMemcpy(g->d_warp, g->h_warp, S * 6 * 4, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(g->d_status, g->h_status, S * 4, hipMemcpyHostToDevice));
    RT_HIP(hipMalloc((void **)&g->d_mbox, S * MB * 16)); RT_HIP(hipMalloc((void **)&g->d_mconf, S * MB * 4));
    RT_HIP(hipMalloc((void **)&g->d_mn, S * 4)); RT_HIP(handle_zero(g->d_mn, S * 4, g->stream));
    return RTMODT_OK;
}

int rtmodt_gmc_create(const rtmodt_gmc_cfg *cfg, rtmodt_gmc **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    const int d = cfg->downscale;
    const auto fin = [](float v) { return v == v && v - v == 0.0f; };
    RT_CHECK((d == 1 || d == 2 || d == 4 || d == 8) && cfg->coarse_search >= 0 && cfg->coarse_search <= GMC_MAX_CS && cfg->search >= 1 && cfg->search <= GMC_MAX_SR &&
                 cfg->min_texture >= 0 && cfg->max_sad >= 0 && fin(cfg->mask_conf) && cfg->n_hyp >= 1 && cfg->n_hyp <= GMC_MAX_HYP && fin(cfg->min_sep) &&
                 cfg->min_sep >= 0.f && cfg->min_sep <= 8192.f && fin(cfg->inlier_px) && cfg->inlier_px >= 0.f && cfg->inlier_px <= 4096.f && cfg->min_blocks >= 2 &&
                 cfg->min_inliers >= 2,
             RTMODT_E_INVALID, "bad parameter (downscale %d in {1, 2, 4, 8}, coarse_search %d in 0..16, search %d in 1..8, min_texture %d, max_sad %d, n_hyp %d in "
             "1..256, min_sep %g, inlier_px %g, min_blocks %d >= 2, min_inliers %d >= 2)", d, cfg->coarse_search, cfg->search, cfg->min_texture, cfg->max_sad,
             cfg->n_hyp, (double)cfg->min_sep, (double)cfg->inlier_px, cfg->min_blocks, cfg->min_inliers);
    RT_CHECK(cfg->n_streams >= 1 && cfg->max_boxes >= 0, RTMODT_E_INVALID, "n_streams %d / max_boxes %d", cfg->n_streams, cfg->max_boxes);
    RT_CHECK(cfg->n_streams <= GMC_MAX_STREAMS && cfg->max_boxes <= GMC_MAX_BOXES, RTMODT_E_CAPACITY, "n_streams %d / max_boxes %d: at most %d / %d", cfg->n_streams,
             cfg->max_boxes, GMC_MAX_STREAMS, GMC_MAX_BOXES);
    rtmodt_gmc *g = new rtmodt_gmc();
    g->cfg = *cfg; g->device = cfg->device; g->S = cfg->n_streams;
    return handle_created(gmc_create_impl(g), g, rtmodt_gmc_destroy, out);
}

int rtmodt_gmc_reset(rtmodt_gmc *g, int stream) {
    RT_CHECK(g && stream < g->S, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(g->device));
    RT_HIP(hipDeviceSynchronize());
    g->foreign_pending = false;
    for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? g->S : stream + 1); ++s) g->have[s] = 0;
    return RTMODT_OK;
}

int rtmodt_gmc_estimate_batch(rtmodt_gmc *g, const uint8_t *const *frames, int h, int w, int stride_bytes, int mem_kind, const float *mask_xyxy,
                              const float *mask_conf, const int32_t *mask_n, float *warp_out, int32_t *status_out) {
    RT_CHECK(g && frames, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_frame_ptrs(frames, g->S));
    RT_TRY(gmc_check_geometry(g, h, w, stride_bytes, mem_kind));
    bool any = false;
    if (mask_n)
        for (int s = 0; s < g->S; ++s) {
            RT_CHECK(mask_n[s] >= 0, RTMODT_E_INVALID, "stream %d: %d mask boxes", s, mask_n[s]);
            RT_CHECK(mask_n[s] <= g->cfg.max_boxes, RTMODT_E_CAPACITY, "stream %d: %d mask boxes > max_boxes %d", s, mask_n[s], g->cfg.max_boxes);
            any |= mask_n[s] > 0;
        }
    RT_CHECK(!any || (mask_xyxy && mask_conf), RTMODT_E_INVALID, "null mask boxes");
    RT_HIP(hipSetDevice(g->device));
    RT_TRY(gmc_join(g));
    RT_TRY(gmc_set_geometry(g, h, w));
    hipStream_t q = g->stream;
    AppFrames fp{};
    RT_TRY(gmc_stage(g, frames, g->S, h, w, stride_bytes, mem_kind, q, &fp));
    const size_t SM = (size_t)g->S * g->cfg.max_boxes;
    for (int s = 0; s < g->S; ++s) g->h_mn[s] = mask_n ? mask_n[s] : 0;
    if (any) {
        RT_HIP(hipMemcpyAsync(g->d_mbox, mask_xyxy, SM * 16, hipMemcpyHostToDevice, q));
        RT_HIP(hipMemcpyAsync(g->d_mconf, mask_conf, SM * 4, hipMemcpyHostToDevice, q));
    }
    RT_HIP(hipMemcpyAsync(g->d_mn, g->h_mn, (size_t)g->S * 4, hipMemcpyHostToDevice, q));
    RT_TRY(gmc_run(g, fp, g->S, h, w, stride_bytes, g->d_mbox, g->d_mconf, g->d_mn, g->cfg.max_boxes, q));
    return rtmodt_gmc_result(g, warp_out, status_out);
}

int rtmodt_gmc_estimate_from_detector(rtmodt_gmc *g, rtmodt_detector *det, const uint8_t *const *frames, int n_frames, int h, int w, int stride_bytes,
                                      int mem_kind) {
    RT_CHECK(g && det, RTMODT_E_INVALID, "null argument");
    DetOutputs o;
    RT_TRY(detector_outputs(det, &o));
    return gmc_enqueue_detector(g, o, frames, n_frames, h, w, stride_bytes, mem_kind, nullptr);
}

int rtmodt_gmc_result(rtmodt_gmc *g, float *warp_out, int32_t *status_out) {
    RT_CHECK(g, RTMODT_E_INVALID, "null argument");
    RT_HIP(hipSetDevice(g->device));
    RT_TRY(gmc_join(g));
    RT_HIP(hipMemcpyAsync(g->h_warp, g->d_warp, (size_t)g->S * 24, hipMemcpyDeviceToHost, g->stream));
    RT_HIP(hipMemcpyAsync(g->h_status, g->d_status, (size_t)g->S * 4, hipMemcpyDeviceToHost, g->stream));
    RT_HIP(hipStreamSynchronize(g->stream));
    if (warp_out) memcpy(warp_out, g->h_warp, (size_t)g->S * 24);
    if (status_out) memcpy(status_out, g->h_status, (size_t)g->S * 4);
    return RTMODT_OK;
}

int rtmodt_gmc_debug(rtmodt_gmc *g, int stream, uint8_t *l0, uint8_t *l1, int32_t *coarse_table, int32_t *coarse_shift, int32_t *blk, int32_t *order,
                     int32_t *n_valid, int32_t *hyp_score, int32_t *best_k, uint8_t *inliers, int64_t *sums, double *model) {
    RT_CHECK(g && stream >= 0 && stream < g->S, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(g->gh, RTMODT_E_INVALID, "no frame has been estimated yet");
    RT_HIP(hipSetDevice(g->device));
    RT_TRY(gmc_join(g));
    RT_HIP(hipStreamSynchronize(g->stream));
    const size_t s = (size_t)stream, nb = (size_t)g->nb;
    const auto get = [](void *dst, const void *src, size_t bytes) { return !dst || !bytes ? hipSuccess : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    RT_HIP(get(l0, g->d_l0 + (s * 2 + g->which[stream]) * g->l0_bytes, (size_t)g->W0 * g->H0));
    RT_HIP(get(l1, g->d_l1 + (s * 2 + g->which[stream]) * g->l1_bytes, (size_t)g->W1 * g->H1));
    RT_HIP(get(coarse_table, g->d_table + s * GMC_TABLE, GMC_TABLE * 4));
    RT_HIP(get(coarse_shift, g->d_coarse + 2 * s, 8));
    RT_HIP(get(blk, g->d_blk + s * 6 * nb, 6 * nb * 4));
    RT_HIP(get(order, g->d_order + s * nb, nb * 4));
    RT_HIP(get(n_valid, g->d_nvalid + s, 4));
    RT_HIP(get(hyp_score, g->d_scores + s * GMC_MAX_HYP, GMC_MAX_HYP * 4));
    RT_HIP(get(best_k, g->d_bestk + s, 4));
    RT_HIP(get(inliers, g->d_inl + s * 2 * nb, 2 * nb));
    RT_HIP(get(sums, g->d_sums + s * 16, 16 * 8));
    RT_HIP(get(model, g->d_model + s * 12, 12 * 8));
    return RTMODT_OK;
}

int rtmodt_gmc_last_ms(rtmodt_gmc *g, float *estimate_ms) {
    RT_CHECK(g && estimate_ms, RTMODT_E_INVALID, "null argument");
    return g->timer.elapsed(g->device, 0, 1, estimate_ms, "no estimate has run yet");
}

}  // extern "C"
