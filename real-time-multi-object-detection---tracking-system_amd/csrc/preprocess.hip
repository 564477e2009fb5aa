// preprocess.hip -- frame -> network input: packed BGR24 (letterbox_kernel) or 4:2:0 YUV (letterbox_yuv420_kernel).
//
// Replaces what ultralytics' predictor does before the model for the call at
// /root/reference/src/detection/detector.py:100-111: LetterBox
// (cv2.resize INTER_LINEAR + copyMakeBorder(114)), BGR->RGB, HWC uint8 -> float, /255,
// .half().  Output goes straight into the engine's input tensor: fp16 NHWC with 4 channels
// (R, G, B, 0) and the 1-pixel zero border the stem conv reads as its padding.
//
// The resize is OpenCV's 8-bit fixed-point bilinear, restated bit for bit: the pixel is
// letterbox_dev.h's letterbox_pixel, and the coefficient tables are built on the host
// (letterbox.h: resize_table) exactly as oracle/yolo_oracle.py:_resize_coeffs does.
#include "letterbox_dev.h"

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
    int c0, c1, c2;                                         // B, G, R
    letterbox_pixel(x, y, g, t, Bgr24Source{frames.p[b], pitch}, c0, c1, c2);
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
    int c0, c1, c2;                                         // B, G, R
    const uint8_t *f = frames.p[b];
    letterbox_pixel(x, y, g, t, [&](int sx, int sy, int &cb, int &cg, int &cr) { yuv420_bgr(f, l, sx, sy, cb, cg, cr); }, c0, c1, c2);
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
