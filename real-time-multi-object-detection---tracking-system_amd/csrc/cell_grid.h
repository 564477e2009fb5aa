// cell_grid.h -- the one reader of BGR pixels into the luma grid of motion_model.h: how the 256 threads of a workgroup map onto runs
// of cells, how a thread reads its run, and how a run's sums become cell lumas.  motion_model, leftobj_model and health_pixels are
// this reader plus what each does with a cell; it is the only code of those modules that dereferences a caller's frame memory.  Plain
// C++, no HIP, like motion_model.h: tests/native/motion_model_check.cpp walks it over frames whose last byte is the buffer's last
// byte, under the address and UB sanitizers (a frame owns (h - 1) * pitch + 3w bytes and not one more: frame_stage.h).
//   Mapping.  A workgroup is a tile of CG_ROWS cell rows x 64 lanes; a lane owns a run of CPT = 4 / scale cells (at least one) of one
//             cell row, 12 bytes of each pixel row (24 at scale 8); lanes are adjacent runs, so a wave reads 768 contiguous bytes per
//             pixel row.  Tiles go row-major over the grid, tiles_x = ceil(gw / (64 * CPT)) to a row.
//   WIDE.     Every frame base and the pitch a multiple of 4 (3 * px0 is a multiple of 12): the full runs of full cell rows are read
//             as dwords, all of them issued before the first is used; partial runs and every run of a frame that is not WIDE are
//             read byte by byte.
#pragma once

#include <type_traits>

#include "motion_model.h"

namespace rtmodt {

constexpr int CG_ROWS = 4, CG_THREADS = 64 * CG_ROWS;

MO_HD constexpr int cg_cpt(int scale) { return scale >= 4 ? 1 : 4 / scale; }
MO_HD inline int cg_tiles_x(int gw, int scale) { return (gw + 64 * cg_cpt(scale) - 1) / (64 * cg_cpt(scale)); }
MO_HD inline int cg_tiles_y(int gh) { return (gh + CG_ROWS - 1) / CG_ROWS; }

// cells, pixels and bytes of a thread's run
template <int SCALE> struct CgRun { static constexpr int CPT = cg_cpt(SCALE), PX = SCALE * CPT, RUN = 3 * PX; };

// the run of thread `tid` of tile `tile`: cell row cy, first cell cxb, its first pixel (px0, y0) at p and the npx x nrows pixels of
// it inside the frame.  A lane outside the grid is not live: it reads nothing, and its npx, nrows and p mean nothing
struct CgLane { int cy, cxb, px0, y0, npx, nrows; bool live; const uint8_t *p; };

template <int SCALE> MO_HD inline CgLane cg_lane(unsigned tile, int tiles_x, int tid, const uint8_t *frame, long long pitch, int h, int w, int gw, int gh) {
    constexpr int CPT = CgRun<SCALE>::CPT, PX = CgRun<SCALE>::PX;
    CgLane l;
    l.cy = (int)(tile / tiles_x) * CG_ROWS + (tid >> 6);
    l.cxb = ((int)(tile % tiles_x) * 64 + (tid & 63)) * CPT;
    l.live = l.cy < gh && l.cxb < gw;
    l.px0 = l.cxb * SCALE; l.y0 = l.cy * SCALE;
    l.npx = w - l.px0 < PX ? w - l.px0 : PX;
    l.nrows = h - l.y0 < SCALE ? h - l.y0 : SCALE;
    l.p = frame + (long long)l.y0 * pitch + 3LL * l.px0;
    return l;
}

struct CgNoVisit { MO_HD void operator()(int, int, uint32_t) const {} };

// Reads the npx x nrows pixels of a run at p into sum[CPT], the luma sums of its cells; visit(row, i, luma) sees every pixel read,
// row by row and left to right.  A visitor keeps per-row state in registers, so its rows are unrolled; without one the byte path
// stays a loop over the rows.
template <int SCALE, bool WIDE, typename V = CgNoVisit>
MO_HD inline void cg_read_run(const uint8_t *p, long long pitch, int npx, int nrows, uint32_t (&sum)[CgRun<SCALE>::CPT], V &&visit = V()) {
    constexpr int CPT = CgRun<SCALE>::CPT, PX = CgRun<SCALE>::PX, RUN = CgRun<SCALE>::RUN;
#pragma unroll
    for (int j = 0; j < CPT; ++j) sum[j] = 0;
    if (WIDE && npx == PX && nrows == SCALE) {
        uint32_t v[SCALE][RUN / 4];                                 // every load of the run is issued before the first is used
#pragma unroll
        for (int r = 0; r < SCALE; ++r) {
            const uint32_t *q = (const uint32_t *)(p + r * pitch);
#pragma unroll
            for (int k = 0; k < RUN / 4; ++k) v[r][k] = q[k];
        }
#pragma unroll
        for (int r = 0; r < SCALE; ++r)
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                uint32_t c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = (v[r][(3 * i + k) >> 2] >> (8 * ((3 * i + k) & 3))) & 255u;
                const uint32_t y = mo_luma(c[0], c[1], c[2]);
                sum[i / SCALE] += y;
                visit(r, i, y);
            }
    } else {
        constexpr int ROWS_UNROLLED = std::is_same<typename std::decay<V>::type, CgNoVisit>::value ? 1 : SCALE;
#pragma unroll ROWS_UNROLLED
        for (int r = 0; r < SCALE; ++r) {
            if (r >= nrows) break;
            const uint8_t *q = p + r * pitch;
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                if (i >= npx) continue;
                const uint32_t y = mo_luma(q[3 * i], q[3 * i + 1], q[3 * i + 2]);
                sum[i / SCALE] += y;
                visit(r, i, y);
            }
        }
    }
}

// Yc of cell cx from its sum over nrows pixel rows; false for a cell outside the grid
template <int SCALE> MO_HD inline bool cg_cell_luma(uint32_t sum, int cx, int nrows, int w, uint32_t &yc) {
    const int cols = mo_cell_span(cx, SCALE, w);
    if (cols == 0) return false;
    const uint32_t cnt = (uint32_t)(cols * nrows);
    yc = cnt == SCALE * SCALE ? (sum + SCALE * SCALE / 2) / (SCALE * SCALE) : mo_cell_mean(sum, cnt);
    return true;
}

}  // namespace rtmodt
