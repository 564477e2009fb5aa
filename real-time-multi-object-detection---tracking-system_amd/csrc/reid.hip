// reid.hip -- the DeepSORT re-identification network on the GPU: OSNet x0.25 (Zhou et al.; torchreid's osnet_x0_25 in eval mode,
// output = the 512-value feature after fc), the model config/default.yaml:60 (`tracking.deepsort.embedder`) names.  For every
// detection box of every stream: BGR frame in HBM -> 256 x 128 RGB crop -> network -> L2-normalised int8[512] descriptor, in a
// number of launches that does not depend on the number of boxes (80), with no host hop.  Weights: the project's
// .rtreid file (reid_weights.py).  PARITY UNPINNED: neither torchreid nor cv2 nor deep_sort_realtime is installed anywhere this
// runs; tests/reid_ref.py restates the crop and the quantiser exactly and the network in float64.
//
// CROP (integers; tests/reid_ref.py agrees bit for bit)
//   rectangle  app_coord of appearance.hip: int(v) by truncation after clamping to +-2^20, then clamped to the frame; pixels
//              x0 <= x < x1, y0 <= y < y1, W = x1 - x0, H = y1 - y0.  W <= 0, H <= 0 or a NaN corner: the box is EMPTY -- its
//              descriptor and feature rows are zero and no network work is done for it (its other taps keep stale bytes).
//   resize     bilinear to 256 (h) x 128 (w), half-pixel centres, 11 fractional bits: fx = (2 ox + 1) * W * 8 - 1024
//              (= ((ox + 1/2) W / 128 - 1/2) * 2048 exactly), fy = (2 oy + 1) * H * 4 - 1024; f < 0 -> 0; lo = f >> 11,
//              w1 = f & 2047, w0 = 2048 - w1; lo >= n - 1 -> lo = n - 1, w1 = 0; hi = min(lo + 1, n - 1) (edge replicated);
//              acc = wy0 (wx0 p00 + wx1 p01) + wy1 (wx0 p10 + wx1 p11) in int32; value = (acc + (1 << 21)) >> 22.  BGR -> RGB.
//   input      x = table[value][c], table = RNE16((v / 255 - mean_c) / std_c) evaluated in float32 on the host (ImageNet mean / std);
//              rtmodt_reid_norm_table returns the host's table, and a CPU test compares it bit for bit with the restatement's.
//   This file is compiled with -ffp-contract=off and IEEE float32 division (the Makefile's EXACT): an fma is one only where written.
//
// ROUNDING CONTRACT of the network (fp16 weights with BN folded, fp32 bias, fp32 accumulation; RNE16 = round to nearest even fp16)
//   stored     every activation tensor in HBM is fp16 and is rounded exactly once, when it is stored.
//   conv1      7x7 stride 2 pad 3 on the vector ALU: acc = 0, fma over (ky, kx, c) ascending (taps in the padding skipped), + bias,
//              ReLU, RNE16.  maxpool 3x3 stride 2 pad 1 is exact.
//   1x1 / fc   v_mfma_f32_16x16x16_f16, k blocks ascending from acc = 0; + bias (+ the fp32 value of the stored residual),
//              ReLU where the layer has one, RNE16.  Channel counts 24 are zero-padded to 32 (weights, bias and maps).
//   LightConv  1x1 (linear, no bias) stored RNE16; depthwise 3x3 pad 1: acc = 0, fma over (ky, kx) ascending (taps in the padding
//              skipped), + bias, ReLU, RNE16.
//   gate       float32 throughout, weights float32: mean = (fixed-order sum of the stream's stored map) * (1 / P);
//              h = ReLU(b1 + sum_c w1 mean_c), g = 1 / (1 + expf(-(b2 + sum_j w2 h_j))) -- sums by fma in index order, expf = __expf
//              (v_exp_f32), the division IEEE; x2 = RNE16(g_a a + g_b b + g_c c + g_d d), one fma chain in that order.
//   block      out = RNE16(ReLU(conv3(x2) + bias + idn)), idn = the block's stored input or the stored RNE16(downsample(x) + bias).
//   transition RNE16(ReLU(1x1 + bias)) stored, then RNE16(((p00 + p01) + p10 + p11) * 0.25) of the stored values.
//   feature    v = RNE16(sum over the 128 positions in order * (1 / 128)) of conv5's stored map; feat = ReLU(fc(v) + bias), float32.
//
// DESCRIPTOR  rtmodt_appearance_quantize's rule on the device: n2 = sum_k (double)feat_k^2 for k = 0..511 IN THAT ORDER (one
//   thread), norm = sqrt(n2), q_k = rint(127 * (double)feat_k / norm) clamped to +-127; norm == 0 (or not finite): zeros.
//
// LAUNCHES    crop, conv1, maxpool; per block 11 or 12 (conv1, 4 x (1x1 + depthwise) over the streams still running -- a launch
//   covers every stream of a level through blockIdx.z --, gate, [downsample], conv3); per transition 2; conv5, pool, fc, quantise.
//   Every kernel's grid covers (slot, position tile); a workgroup whose slot holds no box, or an empty one, returns at once.
//   The gate kernel is the one place a workgroup owns a crop's whole map (LDS: 4 x 256 partial sums + means + gates = 5 KB).
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "frame_stage.h"
#include "handle_host.h"

namespace rtmodt {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int REID_H = 256, REID_W = 128, REID_DIM = 512;
constexpr int REID_COORD_MAX = 1 << 20;
constexpr int REID_MAX_SLOTS = 8192;
__device__ __forceinline__ int reid_coord(float v) { return (int)truncf(fminf(fmaxf(v, (float)-REID_COORD_MAX), (float)REID_COORD_MAX)); }

// ------------------------------------------------------------------------------------------------------------------- crop
struct CropArgs {
    AppFrames frames; int h, w, pitch;
    const float4 *box; const int32_t *box_n; int box_stride;
    int launch_mb, slot_mb;                  // boxes launched per stream; slot = stream * slot_mb + box
    uint8_t *crop; int32_t *valid;
};

__global__ __launch_bounds__(256) void reid_crop(CropArgs a) {
    const int b = blockIdx.x, s = blockIdx.y, slot = s * a.slot_mb + b;
    bool ok = b < a.box_n[s] && b < a.box_stride;
    int x0 = 0, y0 = 0, W = 0, H = 0;
    if (ok) {
        const float4 bx = a.box[(size_t)s * a.box_stride + b];
        const bool nan = bx.x != bx.x || bx.y != bx.y || bx.z != bx.z || bx.w != bx.w;
        x0 = min(max(reid_coord(bx.x), 0), a.w); y0 = min(max(reid_coord(bx.y), 0), a.h);
        W = min(max(reid_coord(bx.z), 0), a.w) - x0; H = min(max(reid_coord(bx.w), 0), a.h) - y0;
        ok = !nan && W > 0 && H > 0;
    }
    if (blockIdx.z == 0 && threadIdx.x == 0) a.valid[slot] = ok ? 1 : 0;
    if (!ok) return;
    const uint8_t *f = a.frames.p[s] + (size_t)y0 * a.pitch + (size_t)3 * x0;
    uint8_t *out = a.crop + (size_t)slot * (REID_H * REID_W * 3);
    for (int i = threadIdx.x; i < 32 * REID_W; i += 256) {
        const int oy = blockIdx.z * 32 + i / REID_W, ox = i % REID_W;
        int fx = (2 * ox + 1) * W * 8 - 1024, fy = (2 * oy + 1) * H * 4 - 1024;
        fx = max(fx, 0); fy = max(fy, 0);
        int xl = fx >> 11, wx1 = fx & 2047, yl = fy >> 11, wy1 = fy & 2047;
        if (xl >= W - 1) { xl = W - 1; wx1 = 0; }
        if (yl >= H - 1) { yl = H - 1; wy1 = 0; }
        const int xh = min(xl + 1, W - 1), yh = min(yl + 1, H - 1), wx0 = 2048 - wx1, wy0 = 2048 - wy1;
        const uint8_t *r0 = f + (size_t)yl * a.pitch, *r1 = f + (size_t)yh * a.pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int top = wx0 * r0[3 * xl + c] + wx1 * r0[3 * xh + c], bot = wx0 * r1[3 * xl + c] + wx1 * r1[3 * xh + c];
            out[((size_t)oy * REID_W + ox) * 3 + (2 - c)] = (uint8_t)((wy0 * top + wy1 * bot + (1 << 21)) >> 22);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ conv1 + pools
struct StemArgs {
    const uint8_t *crop; const int32_t *valid; const float *table;       // table[256][3] float32 values of the fp16 input
    const float *w; const float *bias;                                   // w[147][16], k = (ky * 7 + kx) * 3 + c
    f16 *out;                                                            // [slot][128][64][16]
    int launch_mb, slot_mb;
};
__device__ __forceinline__ int reid_slot(int i, int launch_mb, int slot_mb) { return (i / launch_mb) * slot_mb + i % launch_mb; }

__global__ __launch_bounds__(256) void reid_conv1(StemArgs a) {
    const int slot = reid_slot(blockIdx.y, a.launch_mb, a.slot_mb);
    if (!a.valid[slot]) return;
    __shared__ float w[147 * 16];
    __shared__ float tab[256 * 3];
    for (int i = threadIdx.x; i < 147 * 16; i += 256) w[i] = a.w[i];
    for (int i = threadIdx.x; i < 256 * 3; i += 256) tab[i] = a.table[i];
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x, oy = idx >> 6, ox = idx & 63;
    const uint8_t *in = a.crop + (size_t)slot * (REID_H * REID_W * 3);
    float acc[16];
#pragma unroll
    for (int co = 0; co < 16; ++co) acc[co] = 0.f;
    for (int ky = 0; ky < 7; ++ky) {
        const int iy = 2 * oy - 3 + ky;
        if (iy < 0 || iy >= REID_H) continue;
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = 2 * ox - 3 + kx;
            if (ix < 0 || ix >= REID_W) continue;
            const uint8_t *p = in + ((size_t)iy * REID_W + ix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = tab[p[c] * 3 + c];
                const float *wk = w + ((ky * 7 + kx) * 3 + c) * 16;
#pragma unroll
                for (int co = 0; co < 16; ++co) acc[co] = fmaf(x, wk[co], acc[co]);
            }
        }
    }
    f16 *o = a.out + ((size_t)slot * 8192 + idx) * 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        half4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (f16)fmaxf(acc[4 * q + j] + a.bias[4 * q + j], 0.f);
        *(half4 *)(o + 4 * q) = v;
    }
}

// pooling over NHWC fp16 maps, 4 channels per thread.  mode 0: max 3x3 stride 2 pad 1; mode 1: average 2x2 stride 2
struct PoolArgs { const f16 *in; f16 *out; const int32_t *valid; int H, W, C, mode, launch_mb, slot_mb; long in_slot, out_slot; };

__global__ __launch_bounds__(256) void reid_pool(PoolArgs a) {
    const int slot = reid_slot(blockIdx.y, a.launch_mb, a.slot_mb);
    if (!a.valid[slot]) return;
    const int Ho = a.H / 2, Wo = a.W / 2, C4 = a.C / 4;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ho * Wo * C4) return;
    const int c4 = idx % C4, p = idx / C4, oy = p / Wo, ox = p % Wo;
    const f16 *in = a.in + (size_t)slot * a.in_slot + 4 * c4;
    float v[4];
    if (a.mode == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = -INFINITY;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if (iy < 0 || iy >= a.H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (ix < 0 || ix >= a.W) continue;
                const half4 x = *(const half4 *)(in + ((size_t)iy * a.W + ix) * a.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], (float)x[j]);
            }
        }
    } else {
        const half4 p00 = *(const half4 *)(in + ((size_t)(2 * oy) * a.W + 2 * ox) * a.C), p01 = *(const half4 *)(in + ((size_t)(2 * oy) * a.W + 2 * ox + 1) * a.C);
        const half4 p10 = *(const half4 *)(in + ((size_t)(2 * oy + 1) * a.W + 2 * ox) * a.C), p11 = *(const half4 *)(in + ((size_t)(2 * oy + 1) * a.W + 2 * ox + 1) * a.C);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((((float)p00[j] + (float)p01[j]) + (float)p10[j]) + (float)p11[j]) * 0.25f;
    }
    half4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (f16)v[j];
    *(half4 *)(a.out + (size_t)slot * a.out_slot + (size_t)p * a.C + 4 * c4) = o;
}

// ------------------------------------------------------------------------------------------------------ 1x1 conv / fc (MFMA)
// D[cout][position] = W[cout][cin] x X[cin][position]: A = 16 output channels x 16 k (lane l: row l & 15, k = 4 (l >> 4) + j),
// B = 16 k x 16 positions (lane l: column l & 15, the same k); C: column l & 15, rows 4 (l >> 4) + reg -- a lane ends up with 4
// consecutive output channels of one position, one 8-byte NHWC store.  A wave owns 16 positions and walks the output-channel
// tiles with its positions' fragments in registers (cin <= 128: 8 fragments); grid = (position tiles of 64, slot, stream).
constexpr int PW_MAX_G = 4;
struct PwArgs {
    const f16 *in[PW_MAX_G]; f16 *out[PW_MAX_G]; const f16 *w[PW_MAX_G]; const float *bias[PW_MAX_G];    // per stream of the level
    const f16 *res; float *out32; const int32_t *valid;
    int P, Cin, Cout, relu, fc, launch_mb, slot_mb;     // fc: positions ARE slots (one launch for all), valid is read per position
    long in_slot, out_slot, res_slot;
};

__global__ __launch_bounds__(256) void reid_pw(PwArgs a) {
    const int g = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot = 0;
    if (!a.fc) {
        slot = reid_slot(blockIdx.y, a.launch_mb, a.slot_mb);
        if (!a.valid[slot]) return;
    }
    const int p0 = blockIdx.x * 64 + wave * 16;
    if (p0 >= a.P) return;                                 // wave-uniform
    const int p = p0 + (lane & 15), kq = 4 * (lane >> 4);
    const bool live = p < a.P;
    const long prow = a.fc ? (long)reid_slot(live ? p : 0, a.launch_mb, a.slot_mb) : (long)p;      // fc: row of position p
    const f16 *in = a.in[g] + (size_t)slot * a.in_slot + (size_t)prow * a.Cin + kq;
    const int KT = a.Cin / 16;
    half4 bf[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        bf[k] = half4{0, 0, 0, 0};
        if (k < KT && live) bf[k] = *(const half4 *)(in + 16 * k);
    }
    const bool keep = live && (!a.fc || a.valid[prow]);
    const f16 *w = a.w[g] + (size_t)(lane & 15) * a.Cin + kq;
    for (int ct = 0; ct < a.Cout / 16; ++ct) {
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < KT) acc = __builtin_amdgcn_mfma_f32_16x16x16f16(*(const half4 *)(w + (size_t)ct * 16 * a.Cin + 16 * k), bf[k], acc, 0, 0, 0);
        const int c = ct * 16 + kq;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[j] + a.bias[g][c + j];
        if (a.res && live) {
            const half4 r = *(const half4 *)(a.res + (size_t)slot * a.res_slot + (size_t)p * a.Cout + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += (float)r[j];
        }
        if (a.relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        if (!live) continue;
        if (a.out32) {
            float *o = a.out32 + (size_t)prow * a.Cout + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = keep ? v[j] : 0.f;
        } else {
            half4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (f16)v[j];
            *(half4 *)(a.out[g] + (size_t)slot * a.out_slot + (size_t)p * a.Cout + c) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- depthwise 3x3
struct DwArgs {
    const f16 *in[PW_MAX_G]; f16 *out[PW_MAX_G]; const f16 *w[PW_MAX_G]; const float *bias[PW_MAX_G];    // w[9][C]
    const int32_t *valid; int H, W, C, launch_mb, slot_mb; long slot_stride;
};

__global__ __launch_bounds__(256) void reid_dw(DwArgs a) {
    const int slot = reid_slot(blockIdx.y, a.launch_mb, a.slot_mb), g = blockIdx.z;
    if (!a.valid[slot]) return;
    const int C4 = a.C / 4, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.H * a.W * C4) return;
    const int c4 = idx % C4, p = idx / C4, y = p / a.W, x = p % a.W;
    const f16 *in = a.in[g] + (size_t)slot * a.slot_stride + 4 * c4;
    const f16 *w = a.w[g] + 4 * c4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y - 1 + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x - 1 + kx;
            if (ix < 0 || ix >= a.W) continue;
            const half4 v = *(const half4 *)(in + ((size_t)iy * a.W + ix) * a.C), wk = *(const half4 *)(w + (ky * 3 + kx) * a.C);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf((float)v[j], (float)wk[j], acc[j]);
        }
    }
    half4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (f16)fmaxf(acc[j] + a.bias[g][4 * c4 + j], 0.f);
    *(half4 *)(a.out[g] + (size_t)slot * a.slot_stride + (size_t)p * a.C + 4 * c4) = o;
}

// --------------------------------------------------------------------------------------------------------------- gate
// one workgroup per crop: pools the four streams' maps, evaluates the shared gate on each, writes the gated sum
struct GateArgs {
    const f16 *s[4]; f16 *out; const float *w1, *b1, *w2, *b2;          // w1[hid][C], w2[C][hid]
    const int32_t *valid; int P, C, hid, launch_mb, slot_mb; long slot_stride;
};

__global__ __launch_bounds__(256) void reid_gate(GateArgs a) {
    const int slot = reid_slot(blockIdx.x, a.launch_mb, a.slot_mb), t = threadIdx.x;
    if (!a.valid[slot]) return;
    __shared__ float part[4][256];
    __shared__ float mean[4][32], hid[4][2], gate[4][32];
    const int C = a.C, c = t % C, q = t / C, Q = 256 / C;
    const size_t base = (size_t)slot * a.slot_stride;
    for (int s = 0; s < 4; ++s) {
        const f16 *m = a.s[s] + base;
        float sum = 0.f;
        for (int p = q; p < a.P; p += Q) sum += (float)m[(size_t)p * C + c];
        part[s][t] = sum;
    }
    __syncthreads();
    if (t < 4 * C) {
        const int s = t / C, cc = t % C;
        float sum = 0.f;
        for (int k = 0; k < Q; ++k) sum += part[s][k * C + cc];
        mean[s][cc] = sum * (1.0f / (float)a.P);
    }
    __syncthreads();
    if (t < 4 * a.hid) {
        const int s = t / a.hid, j = t % a.hid;
        float h = a.b1[j];
        for (int k = 0; k < C; ++k) h = fmaf(a.w1[j * C + k], mean[s][k], h);
        hid[s][j] = fmaxf(h, 0.f);
    }
    __syncthreads();
    if (t < 4 * C) {
        const int s = t / C, cc = t % C;
        float z = a.b2[cc];
        for (int j = 0; j < a.hid; ++j) z = fmaf(a.w2[cc * a.hid + j], hid[s][j], z);
        gate[s][cc] = 1.0f / (1.0f + __expf(-z));
    }
    __syncthreads();
    const int C4 = C / 4;
    for (int i = t; i < a.P * C4; i += 256) {
        const int c0 = 4 * (i % C4);
        const size_t off = base + (size_t)(i / C4) * C + c0;
        const half4 va = *(const half4 *)(a.s[0] + off), vb = *(const half4 *)(a.s[1] + off), vc = *(const half4 *)(a.s[2] + off),
                    vd = *(const half4 *)(a.s[3] + off);
        half4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = gate[0][c0 + j] * (float)va[j];
            v = fmaf(gate[1][c0 + j], (float)vb[j], v);
            v = fmaf(gate[2][c0 + j], (float)vc[j], v);
            v = fmaf(gate[3][c0 + j], (float)vd[j], v);
            o[j] = (f16)v;
        }
        *(half4 *)(a.out + off) = o;
    }
}

// ----------------------------------------------------------------------------------------- global pool, quantiser
struct TailArgs { const f16 *conv5; f16 *pooled; const float *feat; int8_t *desc; int desc_stride; const int32_t *valid; int launch_mb, slot_mb; };

__global__ __launch_bounds__(128) void reid_gap(TailArgs a) {
    const int slot = reid_slot(blockIdx.x, a.launch_mb, a.slot_mb), c = threadIdx.x;
    float sum = 0.f;
    if (a.valid[slot]) {
        const f16 *m = a.conv5 + (size_t)slot * (128 * 128);
        for (int p = 0; p < 128; ++p) sum += (float)m[p * 128 + c];
    }
    a.pooled[(size_t)slot * 128 + c] = (f16)(sum * (1.0f / 128.0f));
}

__global__ __launch_bounds__(REID_DIM) void reid_quant(TailArgs a) {
    const int i = blockIdx.x, slot = reid_slot(i, a.launch_mb, a.slot_mb), t = threadIdx.x;
    __shared__ float f[REID_DIM];
    __shared__ double norm;
    const float x = a.valid[slot] ? a.feat[(size_t)slot * REID_DIM + t] : 0.f;
    f[t] = x;
    __syncthreads();
    if (t == 0) {
        double n2 = 0.0;
        for (int k = 0; k < REID_DIM; ++k) n2 += (double)f[k] * (double)f[k];
        norm = sqrt(n2);
    }
    __syncthreads();
    double q = 0.0;
    if (norm > 0.0 && isfinite(norm)) q = rint(127.0 * (double)x / norm);
    q = q != q ? 0.0 : fmin(127.0, fmax(-127.0, q));
    a.desc[((size_t)(i / a.launch_mb) * a.desc_stride + i % a.launch_mb) * REID_DIM + t] = (int8_t)q;
}

// ======================================================================================================================
// host side
// ======================================================================================================================
struct ReidRec { int f32 = 0, nd = 0; uint32_t shape[4] = {1, 1, 1, 1}; const uint8_t *w = nullptr; const float *b = nullptr; };
struct ReidFile { std::vector<uint8_t> raw; std::map<std::string, ReidRec> recs; uint32_t crc = 0; };

struct Crc32Table {
    uint32_t v[256];
    Crc32Table() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            v[i] = c;
        }
    }
};

static uint32_t crc32_ieee(const uint8_t *p, size_t n) {
    static const Crc32Table table;                         // a function-local static: built once, also when two handles are created at once
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table.v[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// host-only: the network's input values, table[v][c] = RNE16((v / 255 - mean_c) / std_c) evaluated in float32 (c in R, G, B), as
// float32.  reid_weights.norm_table builds the same one; rtmodt_reid_norm_table exposes this one so that a test compares them bit for bit.
static void reid_norm_table(float *out) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    for (int v = 0; v < 256; ++v)
        for (int c = 0; c < 3; ++c) {
            const volatile float n = (float)v / 255.0f;    // volatile: each step rounded to float32, whatever the host compiler would keep wider
            const volatile float d = n - mean[c];
            out[v * 3 + c] = (float)(f16)(d / sd[c]);
        }
}

static float h2f(uint16_t h) { f16 v; memcpy(&v, &h, 2); return (float)v; }

struct BlockSpec { const char *prefix; int P, H, W, cin, mid, midp, cout, first; };
static const BlockSpec kBlocks[6] = {{"conv2.0", 2048, 64, 32, 16, 16, 16, 64, 1}, {"conv2.1", 2048, 64, 32, 64, 16, 16, 64, 0},
                                     {"conv3.0", 512, 32, 16, 64, 24, 32, 96, 1},  {"conv3.1", 512, 32, 16, 96, 24, 32, 96, 0},
                                     {"conv4.0", 128, 16, 8, 96, 32, 32, 128, 1},  {"conv4.1", 128, 16, 8, 128, 32, 32, 128, 0}};
static const int kStreamLen[4] = {1, 2, 3, 4};

// host-only: read and verify the file; every record the network needs must be there with the right shape
static int reid_parse(const char *path, ReidFile *f) {
    RT_CHECK(path && *path, RTMODT_E_INVALID, "no weight file given");
    FILE *fp = fopen(path, "rb");
    RT_CHECK(fp, RTMODT_E_INVALID, "Re-ID weights not found: %s", path);
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (size < 24 || size > (64l << 20)) { fclose(fp); return fail(RTMODT_E_INVALID, "%s: not an RTREID01 weight file", path); }
    f->raw.resize((size_t)size);
    const size_t got = fread(f->raw.data(), 1, (size_t)size, fp);
    fclose(fp);
    RT_CHECK(got == (size_t)size, RTMODT_E_INVALID, "%s: short read", path);
    const uint8_t *raw = f->raw.data();
    uint32_t hdr[4];
    memcpy(hdr, raw + 8, 16);
    RT_CHECK(memcmp(raw, "RTREID01", 8) == 0 && hdr[0] == 1, RTMODT_E_INVALID, "%s: not an RTREID01 weight file", path);
    f->crc = hdr[2];
    RT_CHECK(crc32_ieee(raw + 24, (size_t)size - 24) == f->crc, RTMODT_E_INVALID, "%s: digest mismatch (the file is damaged)", path);
    const uint32_t n = hdr[1];
    RT_CHECK(n <= 4096 && 24 + (size_t)n * 96 <= (size_t)size, RTMODT_E_INVALID, "%s: bad record table", path);
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *r = raw + 24 + (size_t)i * 96;
        char name[49] = {};
        memcpy(name, r, 48);
        uint32_t v[6]; uint64_t off[2];
        memcpy(v, r + 48, 24); memcpy(off, r + 72, 16);
        ReidRec rec;
        rec.f32 = (int)v[0]; rec.nd = (int)v[1];
        RT_CHECK(rec.nd >= 1 && rec.nd <= 4 && v[0] <= 1, RTMODT_E_INVALID, "%s: bad record %s", path, name);
        size_t count = 1;
        for (int k = 0; k < 4; ++k) { rec.shape[k] = v[2 + k]; RT_CHECK(v[2 + k] >= 1 && v[2 + k] <= 4096, RTMODT_E_INVALID, "%s: bad shape in %s", path, name); count *= v[2 + k]; }
        // count <= 4096^4 = 2^48: the byte counts cannot wrap; an offset is compared with what is left of the file, never added to
        const uint64_t fsize = (uint64_t)size, wbytes = (uint64_t)count * (rec.f32 ? 4 : 2), bbytes = (uint64_t)rec.shape[0] * 4;
        RT_CHECK(off[0] % 4 == 0 && off[1] % 4 == 0 && wbytes <= fsize && off[0] <= fsize - wbytes && bbytes <= fsize && off[1] <= fsize - bbytes,
                 RTMODT_E_INVALID, "%s: record %s lies outside the file", path, name);
        rec.w = raw + off[0]; rec.b = (const float *)(raw + off[1]);
        f->recs[name] = rec;
    }
    auto need = [&](const std::string &name, int f32, std::initializer_list<uint32_t> shape) -> int {
        auto it = f->recs.find(name);
        RT_CHECK(it != f->recs.end(), RTMODT_E_INVALID, "%s: no record %s (not an osnet_x0_25 file)", path, name.c_str());
        int k = 0;
        bool ok = it->second.f32 == f32 && it->second.nd == (int)shape.size();
        for (uint32_t s : shape) ok = ok && it->second.shape[k++] == s;
        RT_CHECK(ok, RTMODT_E_INVALID, "%s: record %s has the wrong type or shape", path, name.c_str());
        return RTMODT_OK;
    };
    RT_TRY(need("conv1", 0, {16, 7, 7, 3}));
    for (const BlockSpec &b : kBlocks) {
        const std::string p = b.prefix;
        const uint32_t mid = (uint32_t)b.mid;
        RT_TRY(need(p + ".conv1", 0, {mid, (uint32_t)b.cin}));
        for (int s = 0; s < 4; ++s)
            for (int i = 0; i < kStreamLen[s]; ++i) {
                const std::string q = p + ".conv2" + (char)('a' + s) + "." + std::to_string(i);
                RT_TRY(need(q + ".pw", 0, {mid, mid}));
                RT_TRY(need(q + ".dw", 0, {mid, 3, 3}));
            }
        RT_TRY(need(p + ".gate.fc1", 1, {mid / 16, mid}));
        RT_TRY(need(p + ".gate.fc2", 1, {mid, mid / 16}));
        RT_TRY(need(p + ".conv3", 0, {(uint32_t)b.cout, mid}));
        if (b.first) RT_TRY(need(p + ".downsample", 0, {(uint32_t)b.cout, (uint32_t)b.cin}));
    }
    RT_TRY(need("conv2.2", 0, {64, 64}));
    RT_TRY(need("conv3.2", 0, {96, 96}));
    RT_TRY(need("conv5", 0, {128, 128}));
    RT_TRY(need("fc", 0, {512, 128}));
    return RTMODT_OK;
}

struct PwW { const f16 *w; const float *b; };             // device
struct BlockW { PwW conv1, pw[4][4], dw[4][4], conv3, down; const float *g_w1, *g_b1, *g_w2, *g_b2; int hid; };

}  // namespace rtmodt

using namespace rtmodt;

struct rtmodt_reid : HandleBase {        // stream: null when a tracker embeds the network and runs it on its own streams
    int max_frames = 0, max_boxes = 0, n_slots = 0;
    EventTimer<3> timer;
    uint32_t crc = 0;
    // weights (one arena)
    uint8_t *arena = nullptr;
    const float *table = nullptr, *c1_w = nullptr, *c1_b = nullptr;
    BlockW blocks[6];
    PwW trans[2], conv5, fc;
    // per-slot buffers
    int32_t *valid = nullptr;
    uint8_t *crop = nullptr;
    f16 *t_conv1 = nullptr, *t_maxpool = nullptr, *t_block[6] = {}, *t_trans[2] = {}, *t_conv5 = nullptr, *pooled = nullptr;
    float *feat = nullptr;
    f16 *x1 = nullptr, *tmp[4] = {}, *lvl[4][4] = {}, *x2 = nullptr, *big[2] = {};       // scratch: lvl[level][stream]; big: downsample / pre-pool
    int8_t *desc = nullptr;                                 // standalone embed
    float4 *d_box = nullptr; int32_t *d_n = nullptr;
    FrameStage stage;                        // host frames of rtmodt_reid_embed
    int last_count = 0, last_mb = 0;
};

namespace rtmodt {

static constexpr long SCR = 2048 * 16;                      // elements of the largest mid-channel map (stage 2; 512 * 32 and 128 * 32 are smaller)
static constexpr long BIG = 2048 * 64;

static int reid_upload(rtmodt_reid *e, const ReidFile &f) {
    std::vector<uint8_t> host;
    auto place = [&](size_t bytes) { const size_t at = align_up(host.size(), 256); host.resize(at + bytes, 0); return at; };
    struct Fix { const void **dst; size_t at; };
    std::vector<Fix> fix;
    auto rec = [&](const std::string &n) -> const ReidRec & { return f.recs.at(n); };
    // 1x1 / fc: fp16 [coutp][cinp], bias [coutp]
    auto put_pw = [&](const std::string &n, PwW *dst) {
        const ReidRec &r = rec(n);
        const int cout = (int)r.shape[0], cin = (int)r.shape[1], coutp = (int)align_up(cout, 16), cinp = (int)align_up(cin, 16);
        const size_t wa = place((size_t)coutp * cinp * 2);
        for (int o = 0; o < cout; ++o) memcpy(host.data() + wa + ((size_t)o * cinp) * 2, r.w + (size_t)o * cin * 2, (size_t)cin * 2);
        const size_t ba = place((size_t)coutp * 4);
        memcpy(host.data() + ba, r.b, (size_t)cout * 4);
        fix.push_back({(const void **)&dst->w, wa}); fix.push_back({(const void **)&dst->b, ba});
    };
    // depthwise: fp16 [9][cp], bias [cp]
    auto put_dw = [&](const std::string &n, PwW *dst) {
        const ReidRec &r = rec(n);
        const int c = (int)r.shape[0], cp = (int)align_up(c, 16);
        const size_t wa = place((size_t)9 * cp * 2);
        for (int ch = 0; ch < c; ++ch)
            for (int k = 0; k < 9; ++k) memcpy(host.data() + wa + ((size_t)k * cp + ch) * 2, r.w + ((size_t)ch * 9 + k) * 2, 2);
        const size_t ba = place((size_t)cp * 4);
        memcpy(host.data() + ba, r.b, (size_t)c * 4);
        fix.push_back({(const void **)&dst->w, wa}); fix.push_back({(const void **)&dst->b, ba});
    };
    {   // input table and conv1 as float32 [147][16]
        const size_t ta = place(256 * 3 * 4);
        float table[256 * 3];
        reid_norm_table(table);
        memcpy(host.data() + ta, table, sizeof(table));
        fix.push_back({(const void **)&e->table, ta});
        const ReidRec &r = rec("conv1");
        const size_t wa = place(147 * 16 * 4), ba = place(16 * 4);
        for (int co = 0; co < 16; ++co)
            for (int k = 0; k < 147; ++k) {
                uint16_t h; memcpy(&h, r.w + ((size_t)co * 147 + k) * 2, 2);
                const float x = h2f(h);
                memcpy(host.data() + wa + ((size_t)k * 16 + co) * 4, &x, 4);
            }
        memcpy(host.data() + ba, r.b, 64);
        fix.push_back({(const void **)&e->c1_w, wa}); fix.push_back({(const void **)&e->c1_b, ba});
    }
    for (int bi = 0; bi < 6; ++bi) {
        const BlockSpec &b = kBlocks[bi];
        BlockW &w = e->blocks[bi];
        const std::string p = b.prefix;
        put_pw(p + ".conv1", &w.conv1);
        for (int s = 0; s < 4; ++s)
            for (int i = 0; i < kStreamLen[s]; ++i) {
                const std::string q = p + ".conv2" + (char)('a' + s) + "." + std::to_string(i);
                put_pw(q + ".pw", &w.pw[s][i]);
                put_dw(q + ".dw", &w.dw[s][i]);
            }
        put_pw(p + ".conv3", &w.conv3);
        if (b.first) put_pw(p + ".downsample", &w.down);
        w.hid = b.mid / 16;
        const ReidRec &f1 = rec(p + ".gate.fc1"), &f2 = rec(p + ".gate.fc2");
        const size_t a1 = place((size_t)w.hid * b.midp * 4), a2 = place((size_t)w.hid * 4), a3 = place((size_t)b.midp * w.hid * 4), a4 = place((size_t)b.midp * 4);
        for (int j = 0; j < w.hid; ++j) memcpy(host.data() + a1 + (size_t)j * b.midp * 4, f1.w + (size_t)j * b.mid * 4, (size_t)b.mid * 4);
        memcpy(host.data() + a2, f1.b, (size_t)w.hid * 4);
        memcpy(host.data() + a3, f2.w, (size_t)b.mid * w.hid * 4);
        memcpy(host.data() + a4, f2.b, (size_t)b.mid * 4);
        fix.push_back({(const void **)&w.g_w1, a1}); fix.push_back({(const void **)&w.g_b1, a2});
        fix.push_back({(const void **)&w.g_w2, a3}); fix.push_back({(const void **)&w.g_b2, a4});
    }
    put_pw("conv2.2", &e->trans[0]); put_pw("conv3.2", &e->trans[1]); put_pw("conv5", &e->conv5); put_pw("fc", &e->fc);
    RT_HIP(hipMalloc((void **)&e->arena, host.size()));
    RT_HIP(hipMemcpy(e->arena, host.data(), host.size(), hipMemcpyHostToDevice));
    for (const Fix &x : fix) *x.dst = e->arena + x.at;
    return RTMODT_OK;
}

static int reid_alloc(rtmodt_reid *e) {
    const size_t n = (size_t)e->n_slots;
    auto h = [&](f16 **p, size_t elems) -> int { RT_HIP(hipMalloc((void **)p, n * elems * 2)); return RTMODT_OK; };
    RT_HIP(hipMalloc((void **)&e->valid, n * 4)); RT_HIP(handle_zero(e->valid, n * 4, e->stream));
    RT_HIP(hipMalloc((void **)&e->crop, n * REID_H * REID_W * 3));
    RT_TRY(h(&e->t_conv1, 8192 * 16)); RT_TRY(h(&e->t_maxpool, 2048 * 16));
    for (int b = 0; b < 6; ++b) RT_TRY(h(&e->t_block[b], (size_t)kBlocks[b].P * kBlocks[b].cout));
    RT_TRY(h(&e->t_trans[0], 512 * 64)); RT_TRY(h(&e->t_trans[1], 128 * 96)); RT_TRY(h(&e->t_conv5, 128 * 128)); RT_TRY(h(&e->pooled, 128));
    RT_HIP(hipMalloc((void **)&e->feat, n * REID_DIM * 4)); RT_HIP(handle_zero(e->feat, n * REID_DIM * 4, e->stream));
    RT_TRY(h(&e->x1, SCR)); RT_TRY(h(&e->x2, SCR));
    for (int s = 0; s < 4; ++s) RT_TRY(h(&e->tmp[s], SCR));
    for (int l = 0; l < 4; ++l)
        for (int s = l; s < 4; ++s) RT_TRY(h(&e->lvl[l][s], SCR));
    RT_TRY(h(&e->big[0], BIG)); RT_TRY(h(&e->big[1], BIG));
    RT_HIP(hipMalloc((void **)&e->desc, n * REID_DIM)); RT_HIP(handle_zero(e->desc, n * REID_DIM, e->stream));
    RT_HIP(hipMalloc((void **)&e->d_box, n * 16)); RT_HIP(hipMalloc((void **)&e->d_n, (size_t)e->max_frames * 4));
    RT_TRY(e->timer.create());
    return RTMODT_OK;
}

void reid_close(rtmodt_reid *e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (!e->stream) hipDeviceSynchronize();
    handle_close(e, [&] {
        e->timer.destroy();
        hipFree(e->arena); hipFree(e->valid); hipFree(e->crop); hipFree(e->t_conv1); hipFree(e->t_maxpool);
        for (auto p : e->t_block) hipFree(p);
        hipFree(e->t_trans[0]); hipFree(e->t_trans[1]); hipFree(e->t_conv5); hipFree(e->pooled); hipFree(e->feat); hipFree(e->x1); hipFree(e->x2);
        for (auto p : e->tmp) hipFree(p);
        for (auto &l : e->lvl) for (auto p : l) hipFree(p);
        hipFree(e->big[0]); hipFree(e->big[1]); hipFree(e->desc); hipFree(e->d_box); hipFree(e->d_n); e->stage.release();
    });
    delete e;
}

int reid_open(const char *path, int device, int max_frames, int max_boxes, bool own_stream, rtmodt_reid **out) {
    RT_CHECK(max_frames >= 1 && max_boxes >= 1, RTMODT_E_INVALID, "max_frames %d / max_boxes %d must be positive", max_frames, max_boxes);
    RT_CHECK(max_frames <= DS_MAX_STREAMS && max_boxes <= DS_MAX_DETS && (long)max_frames * max_boxes <= REID_MAX_SLOTS, RTMODT_E_CAPACITY,
             "max_frames %d / max_boxes %d = %ld crops of 2.9 MB of device memory each (%.1f GB): at most %d / %d and %d crops in all", max_frames,
             max_boxes, (long)max_frames * max_boxes, (double)max_frames * max_boxes * 2.9e-3, DS_MAX_STREAMS, DS_MAX_DETS, REID_MAX_SLOTS);
    ReidFile f;
    RT_TRY(reid_parse(path, &f));                          // everything above and in here: before the device is touched
    rtmodt_reid *e = new rtmodt_reid();
    e->device = device; e->max_frames = max_frames; e->max_boxes = max_boxes; e->n_slots = max_frames * max_boxes; e->crc = f.crc;
    auto body = [&]() -> int {
        if (own_stream) RT_TRY(handle_open(e));
        else RT_HIP(hipSetDevice(device));
        RT_TRY(reid_upload(e, f));
        RT_TRY(reid_alloc(e));
        return own_stream ? RTMODT_OK : handle_wait(nullptr);        // (embedded: the zeroing went to the null stream)
    };
    return handle_created(body(), e, reid_close, out);
}

#define REID_LAUNCH(kernel, grid, block, q, args)              \
    do {                                                       \
        hipLaunchKernelGGL(kernel, grid, block, 0, q, args);   \
        RT_HIP(hipGetLastError());                             \
    } while (0)

// All launches of one batch on stream q: boxes [count][box_stride] and their counts on the device, frames as device pointers.
// launch_mb box slots are launched per stream (<= max_boxes); desc[stream][desc_stride][512] receives the int8 rows.
int reid_run(rtmodt_reid *e, const AppFrames &frames, int count, int h, int w, int pitch, const float4 *box, const int32_t *box_n, int box_stride,
             int launch_mb, int8_t *desc, int desc_stride, hipStream_t q) {
    RT_CHECK(count >= 1 && count <= e->max_frames, RTMODT_E_CAPACITY, "%d frames > max_frames %d", count, e->max_frames);
    launch_mb = std::min(std::min(launch_mb, box_stride), e->max_boxes);
    if (launch_mb <= 0) return RTMODT_OK;
    const int mb = launch_mb, smb = e->max_boxes, NS = count * mb;
    e->last_count = count; e->last_mb = mb;
    RT_TRY(e->timer.record(0, q));
    CropArgs c{};
    c.frames = frames; c.h = h; c.w = w; c.pitch = pitch; c.box = box; c.box_n = box_n; c.box_stride = box_stride; c.launch_mb = mb; c.slot_mb = smb;
    c.crop = e->crop; c.valid = e->valid;
    REID_LAUNCH(reid_crop, dim3(mb, count, REID_H / 32), dim3(256), q, c);
    RT_TRY(e->timer.record(1, q));
    StemArgs st{e->crop, e->valid, e->table, e->c1_w, e->c1_b, e->t_conv1, mb, smb};
    REID_LAUNCH(reid_conv1, dim3(8192 / 256, NS), dim3(256), q, st);
    auto pool = [&](const f16 *in, f16 *out, int H, int W, int C, int mode) -> int {
        PoolArgs p{in, out, e->valid, H, W, C, mode, mb, smb, (long)H * W * C, (long)(H / 2) * (W / 2) * C};
        REID_LAUNCH(reid_pool, dim3(cdiv((H / 2) * (W / 2) * (C / 4), 256), NS), dim3(256), q, p);
        return RTMODT_OK;
    };
    auto pw1 = [&](const f16 *in, long in_slot, int cin, const PwW &wt, f16 *out, long out_slot, int cout, int P, int relu, const f16 *res) -> int {
        PwArgs a{};
        a.in[0] = in; a.out[0] = out; a.w[0] = wt.w; a.bias[0] = wt.b; a.res = res; a.valid = e->valid; a.P = P; a.Cin = cin; a.Cout = cout; a.relu = relu;
        a.launch_mb = mb; a.slot_mb = smb; a.in_slot = in_slot; a.out_slot = out_slot; a.res_slot = out_slot;
        REID_LAUNCH(reid_pw, dim3(cdiv(P, 64), NS, 1), dim3(256), q, a);
        return RTMODT_OK;
    };
    RT_TRY(pool(e->t_conv1, e->t_maxpool, 128, 64, 16, 0));
    const f16 *x = e->t_maxpool;
    for (int bi = 0; bi < 6; ++bi) {
        const BlockSpec &b = kBlocks[bi];
        const BlockW &bw = e->blocks[bi];
        const long xs = (long)b.P * b.cin, ms = (long)b.P * b.midp, os = (long)b.P * b.cout;
        RT_TRY(pw1(x, xs, b.cin, bw.conv1, e->x1, ms, b.midp, b.P, 1, nullptr));
        for (int l = 0; l < 4; ++l) {                      // level l: the l-th LightConv of the streams l..3
            PwArgs a{}; DwArgs d{};
            const int G = 4 - l;
            for (int g = 0; g < G; ++g) {
                const int s = l + g;
                a.in[g] = l == 0 ? e->x1 : e->lvl[l - 1][s]; a.out[g] = e->tmp[g]; a.w[g] = bw.pw[s][l].w; a.bias[g] = bw.pw[s][l].b;
                d.in[g] = e->tmp[g]; d.out[g] = e->lvl[l][s]; d.w[g] = bw.dw[s][l].w; d.bias[g] = bw.dw[s][l].b;
            }
            a.valid = d.valid = e->valid; a.P = b.P; a.Cin = a.Cout = b.midp; a.launch_mb = d.launch_mb = mb; a.slot_mb = d.slot_mb = smb;
            a.in_slot = a.out_slot = ms; d.H = b.H; d.W = b.W; d.C = b.midp; d.slot_stride = ms;
            REID_LAUNCH(reid_pw, dim3(cdiv(b.P, 64), NS, G), dim3(256), q, a);
            REID_LAUNCH(reid_dw, dim3(cdiv(b.P * b.midp / 4, 256), NS, G), dim3(256), q, d);
        }
        GateArgs g{};
        for (int s = 0; s < 4; ++s) g.s[s] = e->lvl[s][s];
        g.out = e->x2; g.w1 = bw.g_w1; g.b1 = bw.g_b1; g.w2 = bw.g_w2; g.b2 = bw.g_b2; g.valid = e->valid; g.P = b.P; g.C = b.midp; g.hid = bw.hid;
        g.launch_mb = mb; g.slot_mb = smb; g.slot_stride = ms;
        REID_LAUNCH(reid_gate, dim3(NS), dim3(256), q, g);
        const f16 *idn = x;
        if (b.first) {
            RT_TRY(pw1(x, xs, b.cin, bw.down, e->big[0], os, b.cout, b.P, 0, nullptr));
            idn = e->big[0];
        }
        RT_TRY(pw1(e->x2, ms, b.midp, bw.conv3, e->t_block[bi], os, b.cout, b.P, 1, idn));
        x = e->t_block[bi];
        if (bi == 1 || bi == 3) {
            const int t = bi / 2;
            RT_TRY(pw1(x, os, b.cout, e->trans[t], e->big[1], os, b.cout, b.P, 1, nullptr));
            RT_TRY(pool(e->big[1], e->t_trans[t], b.H, b.W, b.cout, 1));
            x = e->t_trans[t];
        }
    }
    RT_TRY(pw1(x, 128 * 128, 128, e->conv5, e->t_conv5, 128 * 128, 128, 128, 1, nullptr));
    TailArgs t{e->t_conv5, e->pooled, e->feat, desc, desc_stride, e->valid, mb, smb};
    REID_LAUNCH(reid_gap, dim3(NS), dim3(128), q, t);
    {
        PwArgs a{};
        a.in[0] = e->pooled; a.w[0] = e->fc.w; a.bias[0] = e->fc.b; a.out32 = e->feat; a.valid = e->valid; a.P = NS; a.Cin = 128; a.Cout = REID_DIM; a.relu = 1;
        a.fc = 1; a.launch_mb = mb; a.slot_mb = smb;
        REID_LAUNCH(reid_pw, dim3(cdiv(NS, 64), 1, 1), dim3(256), q, a);
    }
    REID_LAUNCH(reid_quant, dim3(NS), dim3(REID_DIM), q, t);
    RT_TRY(e->timer.record(2, q));
    e->timer.timed = true;
    return RTMODT_OK;
}

}  // namespace rtmodt

extern "C" {

int rtmodt_reid_create(const rtmodt_reid_cfg *cfg, rtmodt_reid **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_CHECK(cfg->device >= 0, RTMODT_E_INVALID, "device %d", cfg->device);
    return reid_open(cfg->weight_path, cfg->device, cfg->max_frames, cfg->max_boxes, true, out);
}

void rtmodt_reid_destroy(rtmodt_reid *e) { reid_close(e); }

int rtmodt_reid_norm_table(float *out, size_t out_bytes) {
    RT_CHECK(out && out_bytes >= 256 * 3 * sizeof(float), RTMODT_E_INVALID, "the table is float32[256][3]: %zu bytes", (size_t)256 * 3 * sizeof(float));
    reid_norm_table(out);
    return RTMODT_OK;
}

int rtmodt_reid_embed(rtmodt_reid *e, const uint8_t *const *frames, int n_frames, int h, int w, int stride_bytes, int mem_kind, const float *xyxy,
                      const int32_t *n_boxes, int max_boxes, float *feat, int8_t *desc) {
    RT_CHECK(e, RTMODT_E_INVALID, "null argument");
    RT_CHECK(n_frames >= 0 && n_frames <= e->max_frames, RTMODT_E_CAPACITY, "%d frames > max_frames %d", n_frames, e->max_frames);
    if (n_frames == 0) return RTMODT_OK;
    RT_CHECK(frames && xyxy && n_boxes && desc, RTMODT_E_INVALID, "null argument");
    RT_TRY(check_frame_block(n_frames, h, w, stride_bytes, mem_kind, kAppFrames));
    RT_CHECK(max_boxes >= 1 && max_boxes <= e->max_boxes, RTMODT_E_CAPACITY, "max_boxes %d: 1..%d", max_boxes, e->max_boxes);
    for (int i = 0; i < n_frames; ++i) {
        RT_CHECK(frames[i], RTMODT_E_INVALID, "frame %d is null", i);
        RT_CHECK(n_boxes[i] >= 0, RTMODT_E_INVALID, "frame %d: %d boxes", i, n_boxes[i]);
        RT_CHECK(n_boxes[i] <= max_boxes, RTMODT_E_CAPACITY, "frame %d: %d boxes > max_boxes %d", i, n_boxes[i], max_boxes);
    }
    RT_HIP(hipSetDevice(e->device));
    hipStream_t q = e->stream;
    AppFrames fp{};
    RT_TRY(e->stage.in(frames, n_frames, h, w, stride_bytes, mem_kind, q, FRAMES_AS_GIVEN));
    for (int i = 0; i < n_frames; ++i) fp.p[i] = e->stage.at(frames, i);
    const size_t nb = (size_t)n_frames * max_boxes;
    RT_HIP(hipMemcpyAsync(e->d_box, xyxy, nb * 16, hipMemcpyHostToDevice, q));
    RT_HIP(hipMemcpyAsync(e->d_n, n_boxes, (size_t)n_frames * 4, hipMemcpyHostToDevice, q));
    RT_TRY(reid_run(e, fp, n_frames, h, w, stride_bytes, e->d_box, e->d_n, max_boxes, max_boxes, e->desc, max_boxes, q));
    RT_HIP(hipMemcpyAsync(desc, e->desc, nb * REID_DIM, hipMemcpyDeviceToHost, q));
    if (feat)
        for (int i = 0; i < n_frames; ++i)
            RT_HIP(hipMemcpyAsync(feat + (size_t)i * max_boxes * REID_DIM, e->feat + (size_t)i * e->max_boxes * REID_DIM, (size_t)max_boxes * REID_DIM * 4,
                                  hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    return RTMODT_OK;
}

int rtmodt_reid_tap(rtmodt_reid *e, const char *name, void *out, size_t out_bytes, size_t *needed) {
    RT_CHECK(e && name, RTMODT_E_INVALID, "null argument");
    const void *src = nullptr;
    size_t per = 0;
    const std::string n = name;
    if (n == "crop") { src = e->crop; per = REID_H * REID_W * 3; }
    else if (n == "conv1") { src = e->t_conv1; per = 8192 * 16 * 2; }
    else if (n == "maxpool") { src = e->t_maxpool; per = 2048 * 16 * 2; }
    else if (n == "conv2.2") { src = e->t_trans[0]; per = 512 * 64 * 2; }
    else if (n == "conv3.2") { src = e->t_trans[1]; per = 128 * 96 * 2; }
    else if (n == "conv5") { src = e->t_conv5; per = 128 * 128 * 2; }
    else if (n == "feat") { src = e->feat; per = REID_DIM * 4; }
    else
        for (int b = 0; b < 6; ++b)
            if (n == kBlocks[b].prefix) { src = e->t_block[b]; per = (size_t)kBlocks[b].P * kBlocks[b].cout * 2; }
    RT_CHECK(src, RTMODT_E_INVALID, "no tap named '%s'", name);
    const size_t total = per * e->n_slots;
    if (needed) *needed = total;
    if (!out) return RTMODT_OK;
    RT_CHECK(out_bytes >= total, RTMODT_E_CAPACITY, "tap %s needs %zu bytes, the buffer has %zu", name, total, out_bytes);
    RT_HIP(hipSetDevice(e->device));
    RT_HIP(e->stream ? hipStreamSynchronize(e->stream) : hipDeviceSynchronize());
    RT_HIP(hipMemcpy(out, src, total, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_reid_last_ms(rtmodt_reid *e, float *crop_ms, float *net_ms) {
    RT_CHECK(e, RTMODT_E_INVALID, "null argument");
    float a = 0, b = 0;
    RT_TRY(e->timer.elapsed(e->device, 1, 2, &b, "no embed has run yet"));       // (the last event first: it waits for the call)
    RT_TRY(e->timer.elapsed(e->device, 0, 1, &a, "no embed has run yet"));
    if (crop_ms) *crop_ms = a;
    if (net_ms) *net_ms = b;
    return RTMODT_OK;
}

}  // extern "C"
