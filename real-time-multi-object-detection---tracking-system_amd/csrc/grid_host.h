// grid_host.h -- the host plumbing of the modules that read frames into the luma grid of cell_grid.h (motion.hip, leftobj.hip,
// health.hip): the grid of a handle and the launch grids over it, the checks of a config's grid and of a call's stream list with
// their messages, the test for the reader's dword path, and the one launcher of a <SCALE, WIDE> kernel.  Host code only.  What a
// handle holds on the device differs between the modules and stays with them; its frame (open, zeroing, create tail, close) is
// handle_host.h's, like every other handle's.  enhance.hip, which reads frames through the same reader into histograms and has no
// grid, takes the checks of a stream and of a call's stream list from here.
#pragma once

#include <vector>

#include "frame_stage.h"
#include "handle_host.h"
#include "cell_grid.h"

namespace rtmodt {

constexpr int GRID_TW = 64, GRID_TH = 16;                   // the tile of the filter / edge kernels, in cells

// the grid of a handle (per stream) and the launch grids over it for n frames
struct GridGeom {
    int scale = 1, gw = 0, gh = 0, n_chunks = 0;            // n_chunks: of 4096 cells (ccl_dev.h)
    long long cells = 0;
    void set(int h, int w, int scale_) {
        scale = scale_; gw = mo_grid(w, scale); gh = mo_grid(h, scale);
        cells = (long long)gw * gh;
        n_chunks = (int)((cells + 4095) / 4096);
    }
    int model_tiles_x() const { return cg_tiles_x(gw, scale); }
    int filter_tiles_x() const { return cdiv(gw, GRID_TW); }
    dim3 model_grid(int n) const { return dim3((unsigned)(model_tiles_x() * cg_tiles_y(gh)), n); }
    dim3 filter_grid(int n) const { return dim3((unsigned)(filter_tiles_x() * cdiv(gh, GRID_TH)), n); }
    dim3 per_cell(int n) const { return dim3((unsigned)((cells + CG_THREADS - 1) / CG_THREADS), n); }
    dim3 per_chunk(int n) const { return dim3((unsigned)n_chunks, n); }
};

// the part of a config that makes the grid: first what is INVALID, then (after the module's own parameters) what is beyond CAPACITY
inline int check_grid_cfg(int streams, int height, int width, int scale, int max_streams) {
    RT_CHECK(streams >= 1 && streams <= max_streams, RTMODT_E_INVALID, "streams %d outside 1..%d", streams, max_streams);
    RT_CHECK(height >= 1 && width >= 1 && height <= MO_MAX_DIM && width <= MO_MAX_DIM, RTMODT_E_INVALID, "bad frame geometry %dx%d", width, height);
    RT_CHECK(mo_scale_ok(scale), RTMODT_E_INVALID, "scale %d: one of 1, 2, 4, 8", scale);
    return RTMODT_OK;
}
inline int check_grid_cells(int streams, int height, int width, int scale, long long max_total_cells) {
    const long long cells = (long long)mo_grid(height, scale) * mo_grid(width, scale);
    RT_CHECK(cells <= MO_MAX_CELLS, RTMODT_E_CAPACITY, "a grid of %lld cells (at most %lld)", cells, MO_MAX_CELLS);
    RT_CHECK(cells * streams <= max_total_cells, RTMODT_E_CAPACITY, "%lld cells in all (at most %lld)", cells * streams, max_total_cells);
    return RTMODT_OK;
}

inline int check_stream(int stream, int S) {
    RT_CHECK(stream >= 0 && stream < S, RTMODT_E_INVALID, "stream %d outside 0..%d", stream, S - 1);
    return RTMODT_OK;
}
// n frames of a call for a handle of S streams: frame i is stream streams[i], or stream i without a list
inline int check_stream_list(const uint8_t *const *frames, const int32_t *streams, int n, int S) {
    RT_CHECK(n <= S, RTMODT_E_INVALID, "%d frames in one call for %d streams", n, S);
    RT_CHECK(streams || n == S || n == 0, RTMODT_E_INVALID, "%d frames for %d streams and no stream list", n, S);
    std::vector<char> named(S, 0);
    for (int i = 0; i < n; ++i) {
        RT_CHECK(frames[i], RTMODT_E_INVALID, "frame %d is null", i);
        const int s = streams ? streams[i] : i;
        RT_TRY(check_stream(s, S));
        RT_CHECK(!named[s], RTMODT_E_INVALID, "stream %d is named twice in one call", s);
        named[s] = 1;
    }
    return RTMODT_OK;
}

// every frame base (slot.frame) and the pitch a multiple of 4: the reader's WIDE path
template <typename Slot> bool frames_wide(const FrameStage &stage, const Slot *slots, int n) {
    bool wide = stage.pitch % 4 == 0;
    for (int i = 0; i < n; ++i) wide = wide && slots[i].frame % 4 == 0;
    return wide;
}

// the eight instantiations of a kernel template <int SCALE, bool WIDE>, as launch_by_scale takes them
#define RTMODT_SCALE_KERNELS(K) {{K<1, false>, K<2, false>, K<4, false>, K<8, false>}, {K<1, true>, K<2, true>, K<4, true>, K<8, true>}}
template <typename A> void launch_by_scale(void (*const k[2][4])(A), int scale, bool wide, dim3 grid, hipStream_t q, const A &a) {
    int i;
    switch (scale) {
    case 1: i = 0; break;
    case 2: i = 1; break;
    case 4: i = 2; break;
    default: i = 3; break;
    }
    hipLaunchKernelGGL(k[wide][i], grid, dim3(CG_THREADS), 0, q, a);
}

}  // namespace rtmodt
