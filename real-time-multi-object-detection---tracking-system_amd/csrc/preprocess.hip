// preprocess.hip -- frame -> network input: packed BGR24 (letterbox_kernel) or 4:2:0 YUV (letterbox_yuv420_kernel).
//
// Replaces what ultralytics' predictor does before the model for the call at
// /root/reference/src/detection/detector.py:100-111: LetterBox
// (cv2.resize INTER_LINEAR + copyMakeBorder(114)), BGR->RGB, HWC uint8 -> float, /255,
// .half().  Output goes straight into the engine's input tensor: fp16 NHWC with 4 channels
// (R, G, B, 0) and the 1-pixel zero border the stem conv reads as its padding.
//
// The resize is OpenCV's 8-bit fixed-point bilinear, restated bit for bit (11-bit
// coefficients; horizontal pass x2048 in int32; vertical pass
// (((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2); the coefficient tables are built on the
// host (engine.hip: build_resize_tables) exactly as oracle/yolo_oracle.py:_resize_coeffs does.
#include "kernels.h"

namespace rtmodt {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void letterbox_kernel(FramePtrs frames, int pitch, LetterboxGeom g,
                                                        ResizeTables t, f16 *__restrict__ out, int in_h, int in_w, long total) {
    long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    int x = (int)(gid % in_w);
    long r = gid / in_w;
    int y = (int)(r % in_h);
    int b = (int)(r / in_h);
    int sy = y - g.top, sx = x - g.left;
    int c0 = 114, c1 = 114, c2 = 114;                       // B, G, R
    if (sy >= 0 && sy < g.new_h && sx >= 0 && sx < g.new_w) {
        const uint8_t *f = frames.p[b];
        if (!g.resize) {
            const uint8_t *p = f + (long)sy * pitch + sx * 3;
            c0 = p[0]; c1 = p[1]; c2 = p[2];
        } else {
            int xi = t.xofs[sx], a0 = t.xa0[sx], a1 = t.xa1[sx];
            int yi = t.yofs[sy], b0 = t.yb0[sy], b1 = t.yb1[sy];
            int xj = min(xi + 1, g.src_w - 1), yj = min(yi + 1, g.src_h - 1);
            const uint8_t *p00 = f + (long)yi * pitch + xi * 3, *p01 = f + (long)yi * pitch + xj * 3;
            const uint8_t *p10 = f + (long)yj * pitch + xi * 3, *p11 = f + (long)yj * pitch + xj * 3;
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int h0 = p00[c] * a0 + p01[c] * a1;
                int h1 = p10[c] * a0 + p11[c] * a1;
                int o = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                v[c] = min(max(o, 0), 255);
            }
            c0 = v[0]; c1 = v[1]; c2 = v[2];
        }
    }
    half4 o = {(f16)((float)c2 / 255.0f), (f16)((float)c1 / 255.0f), (f16)((float)c0 / 255.0f), (f16)0.0f};
    *(half4 *)(out + (((long)b * (in_h + 2) + y + 1) * (in_w + 2) + x + 1) * 4) = o;
}

int launch_letterbox(const FramePtrs &frames, int pitch, const LetterboxGeom &g, const ResizeTables &t,
                     const TensorView &img4, int B, hipStream_t s) {
    RT_CHECK(img4.C == 4 && img4.pad == 1, RTMODT_E_INVALID, "letterbox: image tensor must be 4-channel with border");
    RT_CHECK(B >= 1 && B <= 64, RTMODT_E_INVALID, "letterbox: batch %d", B);
    long total = (long)B * img4.H * img4.W;
    hipLaunchKernelGGL(letterbox_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, pitch, g, t, img4.base,
                       img4.H, img4.W, total);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}


// ---------------------------------------------------------------------------------------
// 4:2:0 input (NV12 / I420): OpenCV's integer BT.601 limited-range conversion (cv::cvtColor COLOR_YUV2BGR_NV12 / _I420),
// restated bit for bit -- the pixel at (x, y) takes the chroma sample (x/2, y/2), nearest, no chroma interpolation:
//   yv = max(0, Y - 16) * CY;  R = sat8((yv + 2^19 + CVR*vv) >> 20), G = sat8((yv + 2^19 + CVG*vv + CUG*uu) >> 20),
//   B = sat8((yv + 2^19 + CUB*uu) >> 20)   with uu = U - 128, vv = V - 128 (largest |sum| < 2^30: int32 is exact)
// The conversion is per-pixel integer arithmetic, so converting the four bilinear taps and interpolating them equals
// "convert the whole frame, then letterbox it" -- the same resize, fill and c / 255 as letterbox_kernel above.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// BGR of source pixel (x, y) of one 4:2:0 frame
__device__ __forceinline__ void yuv420_bgr(const uint8_t *__restrict__ f, const YuvLayout &l, int x, int y, int &b, int &g, int &r) {
    const int Y = f[(long)y * l.pitch + x];
    const long crow = (long)(y >> 1) * l.chroma_pitch;
    int U, V;
    if (l.nv12) {
        const uint8_t *uv = f + l.u_off + crow + (x & ~1);
        U = uv[0]; V = uv[1];
    } else {
        U = f[l.u_off + crow + (x >> 1)];
        V = f[l.v_off + crow + (x >> 1)];
    }
    const int uu = U - 128, vv = V - 128, yv = max(0, Y - 16) * 1220542 + (1 << 19);
    r = sat8((yv + 1673527 * vv) >> 20);
    g = sat8((yv - 852492 * vv - 409993 * uu) >> 20);
    b = sat8((yv + 2116026 * uu) >> 20);
}

__global__ __launch_bounds__(256) void letterbox_yuv420_kernel(FramePtrs frames, YuvLayout l, LetterboxGeom g, ResizeTables t,
                                                               f16 *__restrict__ out, int in_h, int in_w, long total) {
    long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    int x = (int)(gid % in_w);
    long r = gid / in_w;
    int y = (int)(r % in_h);
    int b = (int)(r / in_h);
    int sy = y - g.top, sx = x - g.left;
    int c0 = 114, c1 = 114, c2 = 114;                       // B, G, R
    if (sy >= 0 && sy < g.new_h && sx >= 0 && sx < g.new_w) {
        const uint8_t *f = frames.p[b];
        if (!g.resize) {
            yuv420_bgr(f, l, sx, sy, c0, c1, c2);
        } else {
            int xi = t.xofs[sx], a0 = t.xa0[sx], a1 = t.xa1[sx];
            int yi = t.yofs[sy], b0 = t.yb0[sy], b1 = t.yb1[sy];
            int xj = min(xi + 1, g.src_w - 1), yj = min(yi + 1, g.src_h - 1);
            int p00[3], p01[3], p10[3], p11[3];
            yuv420_bgr(f, l, xi, yi, p00[0], p00[1], p00[2]);
            yuv420_bgr(f, l, xj, yi, p01[0], p01[1], p01[2]);
            yuv420_bgr(f, l, xi, yj, p10[0], p10[1], p10[2]);
            yuv420_bgr(f, l, xj, yj, p11[0], p11[1], p11[2]);
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int h0 = p00[c] * a0 + p01[c] * a1;
                int h1 = p10[c] * a0 + p11[c] * a1;
                int o = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                v[c] = min(max(o, 0), 255);
            }
            c0 = v[0]; c1 = v[1]; c2 = v[2];
        }
    }
    half4 o = {(f16)((float)c2 / 255.0f), (f16)((float)c1 / 255.0f), (f16)((float)c0 / 255.0f), (f16)0.0f};
    *(half4 *)(out + (((long)b * (in_h + 2) + y + 1) * (in_w + 2) + x + 1) * 4) = o;
}

int launch_letterbox_yuv420(const FramePtrs &frames, const YuvLayout &l, const LetterboxGeom &g, const ResizeTables &t,
                            const TensorView &img4, int B, hipStream_t s) {
    RT_CHECK(img4.C == 4 && img4.pad == 1, RTMODT_E_INVALID, "letterbox_yuv420: image tensor must be 4-channel with border");
    RT_CHECK(B >= 1 && B <= 64, RTMODT_E_INVALID, "letterbox_yuv420: batch %d", B);
    RT_CHECK(g.src_h % 2 == 0 && g.src_w % 2 == 0, RTMODT_E_INVALID, "letterbox_yuv420: odd frame %dx%d", g.src_w, g.src_h);
    long total = (long)B * img4.H * img4.W;
    hipLaunchKernelGGL(letterbox_yuv420_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, l, g, t, img4.base,
                       img4.H, img4.W, total);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

}  // namespace rtmodt
