// frame_stage.h -- the host plumbing every module that takes a batch of BGR frames as (frames[], n, h, w, stride_bytes, mem_kind) shares:
// the one validator of that argument block, the one grower of a device buffer, the pinned + device command buffer pair, the stager of
// host frames (in, and back out for the modules that work in place), and the host builder of a polygon table.  Host code only.
#pragma once

#include <climits>

#include "common.h"

namespace rtmodt {

// ---------------------------------------------------------------------------------------------------------------- buffers
// THE grower of a device buffer that lives in a handle: at least `need_bytes`, contents not kept.  A buffer that is replaced is freed
// only after the whole DEVICE is idle, not one stream: deepsort, botsort, swapguard and gmc queue on their own stream in one entry point
// and on a detector's stream in another, so no single stream knows who still reads the old buffer.  A regrow happens only when a call is
// larger than every call before it; steady-state calls return on the first line.  A failed allocation leaves *buf == nullptr, *cap == 0.
template <typename T> int dev_grow(T **buf, size_t *cap, size_t need_bytes) {
    if (need_bytes <= *cap) return RTMODT_OK;
    if (*buf) {
        RT_HIP(hipDeviceSynchronize());
        hipFree(*buf);
        *buf = nullptr;
    }
    *cap = 0;
    RT_HIP(hipMalloc((void **)buf, need_bytes));
    *cap = need_bytes;
    return RTMODT_OK;
}

// the pinned + device pair a call writes its command block into and sends in one copy; grows by doubling, under dev_grow's rule
struct CmdBuf {
    char *h = nullptr, *d = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return RTMODT_OK;
        const size_t want = std::max(bytes, 2 * cap);
        if (cap) RT_HIP(hipDeviceSynchronize());
        release();
        RT_HIP(hipHostMalloc((void **)&h, want, hipHostMallocDefault));
        RT_HIP(hipMalloc((void **)&d, want));
        cap = want;
        return RTMODT_OK;
    }
    void release() {
        hipHostFree(h); hipFree(d);
        h = d = nullptr; cap = 0;
    }
};

// ---------------------------------------------------------------------------------------------------------------- checks
// What differs between the modules is API and stays; it is data: the largest h / w (0: the module has a capacity check of its own), the
// largest n (n becomes gridDim.y in the in-place modules; 0: bounded by the handle), whether mem_kind is looked at before the geometry, and
// the word the geometry message uses for stride_bytes.  DESIGN.md has the table.
struct FrameLimits { int max_dim; int max_n; bool kind_first; const char *pitch_word; };
static const FrameLimits kAppFrames = {16384, 0, false, "pitch"};        // the descriptor readers: deepsort, botsort, swapguard, reid, appearance
static const FrameLimits kPaintFrames = {32768, 65535, true, "stride"};  // render, privacy
static const FrameLimits kJpegFrames = {0, 0, true, "stride"};           // jpeg, jpeg_dec: the handle's max_h / max_w / max_batch bound them
static const FrameLimits kGmcFrames = {0, 0, false, "pitch"};            // gmc: GMC_MAX_W x GMC_MAX_H and its streams, checked by the estimator itself
static const FrameLimits kSnapFrames = {16384, 0, false, "pitch"};       // snapshot: read-only, one frame per stream of the handle (or of the crop call)
static const FrameLimits kLensFrames = {16384, 65535, true, "pitch"};    // lens: sources and destinations alike (n becomes gridDim.y)

inline int check_mem_kind(int mem_kind) {
    RT_CHECK(mem_kind == RTMODT_MEM_HOST || mem_kind == RTMODT_MEM_DEVICE, RTMODT_E_INVALID, "mem_kind %d", mem_kind);
    return RTMODT_OK;
}
inline bool pitch_holds(int stride_bytes, int w) { return (long long)stride_bytes >= 3LL * w; }

// geometry, mem_kind and the frame count of the block, without the pointers (for the entry points that check those among other lists)
inline int check_frame_block(int n, int h, int w, int stride_bytes, int mem_kind, const FrameLimits &lim) {
    if (lim.kind_first) RT_TRY(check_mem_kind(mem_kind));
    RT_CHECK(h >= 1 && w >= 1 && (!lim.max_dim || (h <= lim.max_dim && w <= lim.max_dim)) && pitch_holds(stride_bytes, w), RTMODT_E_INVALID,
             "bad frame geometry %dx%d, %s %d", w, h, lim.pitch_word, stride_bytes);
    if (!lim.kind_first) RT_TRY(check_mem_kind(mem_kind));
    RT_CHECK(!lim.max_n || n <= lim.max_n, RTMODT_E_CAPACITY, "%d frames in one call (at most %d)", n, lim.max_n);
    return RTMODT_OK;
}
inline int check_frame_ptrs(const uint8_t *const *frames, int n) {
    for (int i = 0; i < n; ++i) RT_CHECK(frames[i], RTMODT_E_INVALID, "frame %d is null", i);
    return RTMODT_OK;
}
// THE validator of the block; `frames` itself and n >= 0 are the entry point's own "null argument" / "bad argument" check
inline int check_frames(const uint8_t *const *frames, int n, int h, int w, int stride_bytes, int mem_kind, const FrameLimits &lim) {
    RT_TRY(check_frame_block(n, h, w, stride_bytes, mem_kind, lim));
    return check_frame_ptrs(frames, n);
}

// A gather cannot work in place (lens, stab): no destination range of a call may meet a source range of it.  Sources of sh x sw at
// src_stride, destinations of dh x dw at dst_stride.
//   exact_ok (enhance: a pointwise step): destination i may BE source i -- the same base, size and pitch -- and must then meet no
//   other source of the call; every other meeting is refused as before.
inline int check_not_in_place(const uint8_t *const *src, int sh, int sw, int src_stride, uint8_t *const *dst, int dh, int dw, int dst_stride, int n,
                              bool exact_ok = false) {
    const size_t sspan = (size_t)(sh - 1) * (size_t)src_stride + (size_t)3 * sw, dspan = (size_t)(dh - 1) * (size_t)dst_stride + (size_t)3 * dw;
    const bool same_shape = sh == dh && sw == dw && src_stride == dst_stride;
    std::vector<uintptr_t> starts(n);
    for (int i = 0; i < n; ++i) starts[i] = (uintptr_t)src[i];
    std::sort(starts.begin(), starts.end());
    for (int i = 0; i < n; ++i) {
        const uintptr_t a = (uintptr_t)dst[i], b = a + dspan;
        // the source with the largest start below b; all spans are equal, so it is the one that reaches furthest
        auto it = std::lower_bound(starts.begin(), starts.end(), b);
        if (exact_ok && same_shape && (uintptr_t)src[i] == a) {
            // its own source is the one start inside [a, b); what must end before a is the source below it
            const auto own = std::lower_bound(starts.begin(), starts.end(), a);
            RT_CHECK(it - own == 1, RTMODT_E_INVALID, "destination frame %d overlaps a source frame of the call other than its own", i);
            it = own;
        }
        RT_CHECK(it == starts.begin() || *(it - 1) + sspan <= a, RTMODT_E_INVALID, "destination frame %d overlaps a source frame of the call", i);
    }
    return RTMODT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- staging
// Where host frames stand on the device.  Device frames are never staged: the kernels get the caller's pointers and pitch.
enum FrameLayout {
    FRAMES_AS_GIVEN,     // rows at the caller's pitch, one copy of (h - 1) * pitch + 3w bytes per frame into a slot of h * pitch (the read-only descriptor modules)
    FRAMES_TIGHT16,      // rows of align_up(3w, 16) bytes, copied row by row (the in-place modules; jpeg)
    FRAMES_TIGHT         // rows of 3w bytes (jpeg_dec, slice)
};

inline size_t tight16_pitch(int w) { return align_up((size_t)3 * w, 16); }

// rows of 3w bytes between two pitches (also privacy's device src -> dst copy)
inline int copy_bgr_rows(void *dst, size_t dpitch, const void *src, size_t spitch, int h, int w, hipMemcpyKind kind, hipStream_t q) {
    RT_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, (size_t)3 * w, (size_t)h, kind, q));
    return RTMODT_OK;
}

// A handle owns one of these in place of a buffer / capacity pair.  place() decides where the frames of a call stand (and grows the
// buffer), at() and pitch are what the kernels get, copy_in() / copy_out() queue the copies of host frames; in() = place() + copy_in().
struct FrameStage {
    uint8_t *d = nullptr;
    size_t cap = 0;
    // the call place() last saw
    bool host = false;
    FrameLayout layout = FRAMES_AS_GIVEN;
    int n = 0, h = 0, w = 0;
    size_t src_pitch = 0, pitch = 0, fbytes = 0;      // pitch: the one the kernels use

    int place(int n_, int h_, int w_, int stride_bytes, int mem_kind, FrameLayout layout_) {
        host = mem_kind == RTMODT_MEM_HOST; layout = layout_; n = n_; h = h_; w = w_;
        src_pitch = (size_t)stride_bytes;
        pitch = !host || layout == FRAMES_AS_GIVEN ? src_pitch : layout == FRAMES_TIGHT16 ? tight16_pitch(w) : (size_t)3 * w;
        fbytes = (size_t)h * pitch;
        return host ? dev_grow(&d, &cap, (size_t)n * fbytes) : RTMODT_OK;
    }
    // room for every call the handle will take, made once (the slicer, at create): place() then never regrows
    int reserve(size_t bytes) { return dev_grow(&d, &cap, bytes); }
    // the device address of frame i (B: uint8_t or const uint8_t)
    template <typename B> B *at(B *const *frames, int i) const { return host ? (B *)(d + (size_t)i * fbytes) : frames[i]; }

    int copy_in(const uint8_t *const *frames, hipStream_t q) {
        if (!host) return RTMODT_OK;
        for (int i = 0; i < n; ++i) {
            // a frame owns (h - 1) pitch + 3w bytes: a crop that touches its parent's last byte has nothing behind its last row
            if (layout == FRAMES_AS_GIVEN) RT_HIP(hipMemcpyAsync(d + (size_t)i * fbytes, frames[i], fbytes - pitch + (size_t)3 * w, hipMemcpyHostToDevice, q));
            else RT_TRY(copy_bgr_rows(d + (size_t)i * fbytes, pitch, frames[i], src_pitch, h, w, hipMemcpyHostToDevice, q));
        }
        return RTMODT_OK;
    }
    int in(const uint8_t *const *frames, int n_, int h_, int w_, int stride_bytes, int mem_kind, hipStream_t q, FrameLayout layout_) {
        RT_TRY(place(n_, h_, w_, stride_bytes, mem_kind, layout_));
        return copy_in(frames, q);
    }
    // staged frame i back to a host frame: rows of 3w bytes only, the caller's padding is not touched
    int copy_out_one(uint8_t *frame, int i, hipStream_t q) {
        return copy_bgr_rows(frame, src_pitch, d + (size_t)i * fbytes, pitch, h, w, hipMemcpyDeviceToHost, q);
    }
    int copy_out(uint8_t *const *frames, hipStream_t q) {
        if (!host) return RTMODT_OK;
        for (int i = 0; i < n; ++i) RT_TRY(copy_out_one(frames[i], i, q));
        return RTMODT_OK;
    }
    void release() {
        hipFree(d);
        d = nullptr; cap = 0;
    }
};

// ---------------------------------------------------------------------------------------------------------------- polygons
// Host builder of the table the polygon kernels read (polygon.h): pts | off | bbox, each part on a 16-byte boundary, plus the box that
// encloses every non-empty polygon.  `noun` names a polygon in the messages ("zone", "polygon").
struct PolyTable {
    std::vector<int2> pts;
    std::vector<int32_t> off = std::vector<int32_t>(1, 0);
    std::vector<int4> bbox;
    int4 stage = make_int4(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN);
    size_t o_off = 0, o_box = 0;                             // after layout(); pts are at 0

    int add(const int32_t *xy, int np, int z, int max_points, const char *noun) {
        RT_CHECK(np >= 0 && (np == 0 || xy), RTMODT_E_INVALID, "%s %d: bad polygon", noun, z);
        RT_CHECK(pts.size() + np <= (size_t)max_points, RTMODT_E_CAPACITY, "%zu polygon points (at most %d)", pts.size() + np, max_points);
        int4 b = make_int4(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN);
        for (int k = 0; k < np; ++k) {
            const int x = xy[2 * k], y = xy[2 * k + 1];
            pts.push_back(make_int2(x, y));
            b.x = std::min(b.x, x); b.y = std::min(b.y, y); b.z = std::max(b.z, x); b.w = std::max(b.w, y);
        }
        off.push_back((int32_t)pts.size());
        bbox.push_back(b);
        enclose(b);
        return RTMODT_OK;
    }
    int build(const int32_t *const *polygons_xy, const int32_t *n_points, int n, int max_points, const char *noun) {
        for (int z = 0; z < n; ++z) RT_TRY(add(polygons_xy[z], n_points[z], z, max_points, noun));
        return RTMODT_OK;
    }
    void enclose(int4 b) {                                   // (an empty box has x > z)
        if (b.x > b.z || b.y > b.w) return;
        stage.x = std::min(stage.x, b.x); stage.y = std::min(stage.y, b.y); stage.z = std::max(stage.z, b.z); stage.w = std::max(stage.w, b.w);
    }
    // carves pts | off | bbox from offset 0 and returns the end offset, a multiple of 16: the caller may append its own arrays there
    size_t layout() {
        o_off = align_up(std::max<size_t>(pts.size(), 1) * sizeof(int2), 16);
        o_box = align_up(o_off + off.size() * 4, 16);
        return align_up(o_box + bbox.size() * sizeof(int4), 16);
    }
    void write(char *dst) const {
        if (!pts.empty()) memcpy(dst, pts.data(), pts.size() * sizeof(int2));
        memcpy(dst + o_off, off.data(), off.size() * 4);
        if (!bbox.empty()) memcpy(dst + o_box, bbox.data(), bbox.size() * sizeof(int4));
    }
    // the three arrays inside a device pool that write()'s bytes were copied to
    template <typename V> void view(const char *pool, V *v) const {
        v->pts = (const int2 *)pool; v->off = (const int32_t *)(pool + o_off); v->bbox = (const int4 *)(pool + o_box);
    }
};

}  // namespace rtmodt
