// stitch.hip -- offline track stitching: the fragments a tracker leaves behind an occlusion are merged back into one
// identity, and the frames between them can be filled in.  TECHNICAL_DESIGN_DOCUMENT.md prescribes the step three times and
// never builds it: B.4 "IDF1 Optimization" item 4 ("post-process merging -- merge tracks with overlapping time windows and
// similar positions (< 20 px centroid distance)"), G.1 row 1 ("post-process merge tracks within 20 px and 30-frame gap") and
// G.2's correct_id_switches(tracks_history, max_gap=30, max_dist=20), whose body is `...`.  PARITY UNPINNED: the reference has
// no implementation and no third-party stitcher is installed anywhere this runs; the rules below are the definition
// (DESIGN.md section 18), tests/stitch_ref.py restates them in plain Python and the GPU tests require equality with it.
//
// THE RULES.  A sequence is a set of rows frame, id, x, y, w, h ((frame, id) unique, boxes float64, 0-based).  A tracklet is
// all the rows of one id in frame order; s / e are its first / last frame; a row's centre is c = (x + 0.5 w, y + 0.5 h).
//   exit point   where tracklet A is expected g frames after its end: p = c_e + v g.  v = (0, 0) when velocity_window == 0
//                or A has one row; else with r the row min(velocity_window, n_A - 1) rows before A's last,
//                v = (c_e - c_r) / (f_e - f_r) per component.  float64: one division, one multiply, one add, no contraction.
//   link A -> B  admissible when 1 <= g = s_B - e_A <= max_gap and d2 = (p.x - c_sB.x)^2 + (p.y - c_sB.y)^2 < max_dist *
//                max_dist (strict).  Its cost is d2 -- no square root, exact for boxes on an integer grid.
//   choice       one-to-one (a tracklet has at most one successor and one predecessor): the maximum number of links and,
//                among those, the minimum sum of d2 -- lap.h's lexicographic LexCost{-1, d2}, the optimum and not the greedy
//                nearest-first choice.  Isolated pairs (a row of degree 1 whose column has degree 1) are linked directly; the
//                contested remainder is split into connected components, each solved by lap_solve<LexCost>, all of them
//                concurrently.  A component beyond LAP_ROWS / LAP_COLS / LAP_EDGES is RTMODT_E_CAPACITY, no output valid.
//   chains       links go forward in time, so chains cannot cycle; every row's new id is the id of its chain's head (root).
//   gap filling  (interpolate) for a link A -> B with A's last box a and B's first box b: for k = 1 .. g - 1 a row at frame
//                e_A + k with the root's id and the box a + (b - a) * (k / g), t = k / g by one division.  Rows are ordered
//                by sequence, then tracklet A, then k.
//
// THE LAUNCHES, the same number whatever the number of sequences or tracklets:
//   stitch_summary       one thread per tracklet: s, e, the start centre, the end centre and v; the union-find forest and the
//                        ancestor array start as the identity
//   stitch_links<false>  one thread per tracklet A: the tracklets of its sequence ordered by start frame (a host std::sort of
//                        the tracklet indices inside the call) are searched by two binary searches for the window
//                        (e_A, e_A + max_gap]; the admissible ones are counted.  Work follows tracklets x window population.
//   (host scan)          the counts become the CSR of the links, as rtmodt_mot_eval's pairs do: memory follows the links
//   stitch_links<true>   the same decisions again, written into A's CSR slice in (start frame, tracklet) order; column
//                        degrees by integer atomics
//   stitch_isolate       the degree rule: an isolated pair is linked at once; a contested row joins its columns in a
//                        lock-free union-find forest (ccl_dev.h; the larger root goes under the smaller: the label of a component
//                        is its smallest row, whatever the arrival order)
//   stitch_label         key (label << 32 | row) per contested row, all ones otherwise; rocPRIM radix_sort_keys puts every
//                        component's rows side by side in ascending row order -- a deterministic problem for the solver
//   stitch_assign        one wave per sorted position, the one at a component's head compacts its rows, columns and links
//                        into LDS and runs lap_solve<LexCost>; components of all sequences run concurrently
//   stitch_roots         pointer jumping on the predecessor links (anc[t] <- anc[anc[t]] until it stops at a head; the
//                        jumps of all threads shorten each other's paths); root and the fill rows of every link
//   (host scan)          fill offsets per tracklet; the fill rows' need against fill_cap
//   stitch_fill          one thread per fill row: a binary search for its link, then the interpolated box
//
// Built with -ffp-contract=off and IEEE division, like eval.o.
#include "common.h"
#include "lap.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace rtmodt {

#include "wg_dev.h"
#include "ccl_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_NO_ERR = INT_MAX;
constexpr unsigned long long ST_NO_KEY = ~0ull;

struct StitchArgs {
    int n_trk, max_gap, vwin, interpolate;
    double max_d2;                          // max_dist * max_dist
    const int32_t *trk_seq;                 // [n_trk]
    const int32_t *seq_trk_start;           // [n_seq + 1]
    const int32_t *trk_row_start;           // [n_trk + 1]
    const int64_t *row_frame;               // [n_rows]
    const double *row_box;                  // [n_rows][4]
    const int32_t *order;                   // [n_trk] tracklets by (sequence, start frame, index)
    const int64_t *order_start;             // [n_trk] their start frames
    int64_t *ts, *te;                       // [n_trk] first / last frame
    double *cs, *ce, *vel;                  // [n_trk][2] start centre, end centre, exit velocity
    int32_t *link_n;                        // [n_trk] admissible links of the row (count pass)
    const int64_t *link_start;              // [n_trk + 1] CSR of the links (exclusive scan of link_n)
    int32_t *link_col;                      // [n_links] successor candidate B
    double *link_d2, *link_p;               // [n_links], [n_links][2] (link_p only when the caller asks for it)
    int32_t *cdeg;                          // [n_trk] links into the tracklet
    int32_t *parent;                        // [2 n_trk] union-find forest: node t = row t, node n_trk + t = column t
    unsigned long long *key, *key_sorted;   // [n_trk]
    int32_t *colmap;                        // [n_trk] column -> local column of its component (-1 none)
    int32_t *succ, *anc, *root;             // [n_trk] successor (-1 none); predecessor chain -> root
    double *succ_d2;                        // [n_trk]
    int32_t *fill_n;                        // [n_trk] fill rows of the tracklet's link
    int32_t *err;                           // the smallest head row of a component over capacity, ST_NO_ERR none
    const int64_t *fill_start;              // [n_trk + 1]
    int64_t n_fill_write;                   // min(need, fill_cap)
    int32_t *fill_trk;
    int64_t *fill_frame;
    double *fill_box;
};

__global__ __launch_bounds__(ST_THREADS) void stitch_summary(StitchArgs a) {
    const int t = blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= a.n_trk) return;
    const int r0 = a.trk_row_start[t], r1 = a.trk_row_start[t + 1] - 1, n = r1 - r0 + 1;
    const double *b0 = a.row_box + (size_t)r0 * 4, *b1 = a.row_box + (size_t)r1 * 4;
    const double cex = b1[0] + 0.5 * b1[2], cey = b1[1] + 0.5 * b1[3];
    double vx = 0.0, vy = 0.0;
    if (a.vwin > 0 && n > 1) {
        const int rr = r1 - min(a.vwin, n - 1);
        const double *br = a.row_box + (size_t)rr * 4;
        const double df = (double)(a.row_frame[r1] - a.row_frame[rr]);
        vx = (cex - (br[0] + 0.5 * br[2])) / df;
        vy = (cey - (br[1] + 0.5 * br[3])) / df;
    }
    a.ts[t] = a.row_frame[r0];
    a.te[t] = a.row_frame[r1];
    a.cs[2 * (size_t)t] = b0[0] + 0.5 * b0[2];
    a.cs[2 * (size_t)t + 1] = b0[1] + 0.5 * b0[3];
    a.ce[2 * (size_t)t] = cex;
    a.ce[2 * (size_t)t + 1] = cey;
    a.vel[2 * (size_t)t] = vx;
    a.vel[2 * (size_t)t + 1] = vy;
    a.parent[t] = t;
    a.parent[a.n_trk + t] = a.n_trk + t;
    a.anc[t] = t;
    a.succ[t] = -1;
    a.succ_d2[t] = 0.0;
    a.cdeg[t] = 0;
    a.colmap[t] = -1;
}

// first position in [lo, hi) of the ascending `v` whose value is > x
__device__ __forceinline__ int upper_bound_i64(const int64_t *v, int lo, int hi, int64_t x) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (v[mid] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// WRITE = false: the count pass (link_n only); WRITE = true: the same decisions again, written into the row's CSR slice
template <bool WRITE>
__global__ __launch_bounds__(ST_THREADS) void stitch_links(StitchArgs a) {
    const int t = blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= a.n_trk) return;
    const int s = a.trk_seq[t];
    const int o0 = a.seq_trk_start[s], o1 = a.seq_trk_start[s + 1];
    const int64_t e = a.te[t];
    const int lo = upper_bound_i64(a.order_start, o0, o1, e);
    const int hi = upper_bound_i64(a.order_start, lo, o1, e + a.max_gap);
    const double cx = a.ce[2 * (size_t)t], cy = a.ce[2 * (size_t)t + 1], vx = a.vel[2 * (size_t)t], vy = a.vel[2 * (size_t)t + 1];
    int64_t w = WRITE ? a.link_start[t] : 0;
    int cnt = 0;
    for (int j = lo; j < hi; ++j) {
        const int b = a.order[j];
        const double g = (double)(a.order_start[j] - e);   // 1 .. max_gap
        const double px = cx + vx * g, py = cy + vy * g;
        const double dx = px - a.cs[2 * (size_t)b], dy = py - a.cs[2 * (size_t)b + 1];
        const double d2 = dx * dx + dy * dy;
        if (!(d2 < a.max_d2)) continue;
        if (WRITE) {
            a.link_col[w] = b;
            a.link_d2[w] = d2;
            if (a.link_p) { a.link_p[2 * w] = px; a.link_p[2 * w + 1] = py; }
            atomicAdd(&a.cdeg[b], 1);
            ++w;
        }
        ++cnt;
    }
    if (!WRITE) a.link_n[t] = cnt;
}

__global__ __launch_bounds__(ST_THREADS) void stitch_isolate(StitchArgs a) {
    const int t = blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= a.n_trk) return;
    const int64_t l0 = a.link_start[t], l1 = a.link_start[t + 1];
    unsigned long long key = ST_NO_KEY;
    if (l1 > l0) {
        const int b = a.link_col[l0];
        if (l1 - l0 == 1 && a.cdeg[b] == 1) {
            a.succ[t] = b;
            a.succ_d2[t] = a.link_d2[l0];
            a.anc[b] = t;
        } else {
            for (int64_t e = l0; e < l1; ++e) ccl_unite(a.parent, t, a.n_trk + a.link_col[e]);
            key = 0;                                       // contested: stitch_label writes the key
        }
    }
    a.key[t] = key;
}

__global__ __launch_bounds__(ST_THREADS) void stitch_label(StitchArgs a) {
    const int t = blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= a.n_trk) return;
    if (a.key[t] != ST_NO_KEY) a.key[t] = ((unsigned long long)ccl_find(a.parent, t) << 32) | (unsigned)t;
}

// one wave per sorted position; the wave at the head of a component solves it (one lane, as mot_accumulate's contested rest)
__global__ __launch_bounds__(64) void stitch_assign(StitchArgs a) {
    __shared__ LexCost s_ecost[LAP_EDGES], s_u[LAP_ROWS], s_v[LAP_COLS], s_minv[LAP_COLS];     // 60.3 KB in all
    __shared__ int s_hrow[LAP_ROWS], s_hcol[LAP_COLS], s_estart[LAP_ROWS + 1], s_ecol[LAP_EDGES], s_p[LAP_COLS], s_rm[LAP_ROWS],
        s_wayrow[LAP_COLS], s_touched[LAP_COLS], s_usedl[LAP_COLS];
    __shared__ unsigned char s_used[LAP_COLS];
    const int i = blockIdx.x;
    const unsigned long long k0 = a.key_sorted[i];
    if (k0 == ST_NO_KEY) return;
    const unsigned label = (unsigned)(k0 >> 32);
    if (i > 0 && (unsigned)(a.key_sorted[i - 1] >> 32) == label) return;
    if (threadIdx.x != 0) return;
    LapSmemT<LexCost> L;
    L.colmap = a.colmap;                                   // components share no column: each touches its own cells
    L.ecost = s_ecost; L.u = s_u; L.v = s_v; L.minv = s_minv; L.hrow = s_hrow; L.hcol = s_hcol; L.estart = s_estart; L.ecol = s_ecol;
    L.p = s_p; L.rm = s_rm; L.wayrow = s_wayrow; L.touched = s_touched; L.usedl = s_usedl; L.used = s_used;
    int nhr = 0;
    while (i + nhr < a.n_trk && nhr <= LAP_ROWS && (unsigned)(a.key_sorted[i + nhr] >> 32) == label) ++nhr;
    bool over = nhr > LAP_ROWS;
    int ne = 0, nhc = 0;
    for (int h = 0; h < nhr && !over; ++h) {
        const int r = (int)(unsigned)a.key_sorted[i + h];
        L.hrow[h] = r;
        L.estart[h] = ne;
        L.u[h] = LapCost<LexCost>::zero();
        L.rm[h] = -1;
        for (int64_t e = a.link_start[r]; e < a.link_start[r + 1]; ++e) {
            const int c = a.link_col[e];
            if (L.colmap[c] < 0) {
                if (nhc == LAP_COLS) { over = true; break; }
                L.colmap[c] = nhc; L.hcol[nhc] = c;
                L.v[nhc] = LapCost<LexCost>::zero(); L.minv[nhc] = LapCost<LexCost>::inf(); L.p[nhc] = -1; L.used[nhc] = 0;
                ++nhc;
            }
            if (ne == LAP_EDGES) { over = true; break; }
            L.ecol[ne] = L.colmap[c];
            L.ecost[ne] = LexCost{-1, a.link_d2[e]};
            ++ne;
        }
    }
    if (over) {
        atomicMin(a.err, (int)label);
        return;
    }
    L.estart[nhr] = ne;
    lap_solve(L, nhr);
    for (int h = 0; h < nhr; ++h)
        if (L.rm[h] >= 0) {
            const int r = L.hrow[h], c = L.hcol[L.rm[h]];
            a.succ[r] = c;
            a.anc[c] = r;
            for (int e = L.estart[h]; e < L.estart[h + 1]; ++e)
                if (L.ecol[e] == L.rm[h]) { a.succ_d2[r] = L.ecost[e].d; break; }
        }
}

__global__ __launch_bounds__(ST_THREADS) void stitch_roots(StitchArgs a) {
    const int t = blockIdx.x * ST_THREADS + threadIdx.x;
    if (t >= a.n_trk) return;
    int x = ccl_ld(&a.anc[t]);
    while (true) {                                         // anc[] always holds an ancestor: jumps of other threads only help
        const int g = ccl_ld(&a.anc[x]);
        if (g == x) break;
        ccl_st(&a.anc[t], g);
        x = g;
    }
    a.root[t] = x;
    const int b = a.succ[t];
    a.fill_n[t] = (a.interpolate && b >= 0) ? (int)(a.ts[b] - a.te[t] - 1) : 0;
}

__global__ __launch_bounds__(ST_THREADS) void stitch_fill(StitchArgs a) {
    const int64_t f = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (f >= a.n_fill_write) return;
    int lo = 0, hi = a.n_trk;                              // the last tracklet whose fill_start <= f
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.fill_start[mid] <= f) lo = mid; else hi = mid;
    }
    const int t = lo, b = a.succ[t];
    const int k = (int)(f - a.fill_start[t]) + 1;
    const int64_t e = a.te[t];
    const double tt = (double)k / (double)(a.ts[b] - e);
    const double *pa = a.row_box + (size_t)(a.trk_row_start[t + 1] - 1) * 4, *pb = a.row_box + (size_t)a.trk_row_start[b] * 4;
    a.fill_trk[f] = t;
    a.fill_frame[f] = e + k;
    for (int q = 0; q < 4; ++q) a.fill_box[4 * f + q] = pa[q] + (pb[q] - pa[q]) * tt;
}

constexpr int64_t ST_MAX_FRAME = (int64_t)1 << 53;         // frames come from float64 files: exact, and e + max_gap cannot overflow

}  // namespace

}  // namespace rtmodt

using namespace rtmodt;

extern "C" {

int rtmodt_stitch_tracks(int device, const rtmodt_stitch_params *params, int n_seq, const int32_t *seq_trk_start,
                         const int32_t *trk_row_start, const int64_t *row_frame, const double *row_box, int32_t *trk_succ,
                         int32_t *trk_root, double *trk_link_d2, int64_t *seq_links, double *seq_cost, int64_t fill_cap,
                         int32_t *fill_trk, int64_t *fill_frame, double *fill_box, int64_t *n_fill, int64_t cand_cap, int32_t *cand_a,
                         int32_t *cand_b, double *cand_d2, double *cand_p, int64_t *n_cand) {
    // ---- every check before the first HIP call ----
    RT_CHECK(params && n_fill, RTMODT_E_INVALID, "stitch_tracks: null params or n_fill");
    RT_CHECK(params->max_gap >= 1 && params->max_gap <= (1 << 20), RTMODT_E_INVALID, "stitch_tracks: max_gap %d outside 1..%d", params->max_gap,
             1 << 20);
    RT_CHECK(std::isfinite(params->max_dist) && params->max_dist > 0, RTMODT_E_INVALID, "stitch_tracks: max_dist %g must be finite and > 0",
             params->max_dist);
    RT_CHECK(params->velocity_window >= 0, RTMODT_E_INVALID, "stitch_tracks: velocity_window %d < 0", params->velocity_window);
    RT_CHECK(params->interpolate == 0 || params->interpolate == 1, RTMODT_E_INVALID, "stitch_tracks: interpolate %d is not 0 or 1",
             params->interpolate);
    RT_CHECK(n_seq >= 0 && fill_cap >= 0 && cand_cap >= 0, RTMODT_E_INVALID, "stitch_tracks: n_seq %d, fill_cap %lld, cand_cap %lld", n_seq,
             (long long)fill_cap, (long long)cand_cap);
    RT_CHECK(fill_cap == 0 || (fill_trk && fill_frame && fill_box), RTMODT_E_INVALID, "stitch_tracks: null fill arrays with fill_cap %lld",
             (long long)fill_cap);
    RT_CHECK(!n_cand || cand_cap == 0 || (cand_a && cand_b && cand_d2), RTMODT_E_INVALID, "stitch_tracks: null candidate arrays with cand_cap %lld",
             (long long)cand_cap);
    *n_fill = 0;
    if (n_cand) *n_cand = 0;
    if (n_seq == 0) return RTMODT_OK;
    RT_CHECK(seq_trk_start && seq_links && seq_cost, RTMODT_E_INVALID, "stitch_tracks: null sequence arrays");
    RT_CHECK(seq_trk_start[0] == 0, RTMODT_E_INVALID, "stitch_tracks: the tracklet CSR must start at 0");
    for (int s = 0; s < n_seq; ++s)
        RT_CHECK(seq_trk_start[s + 1] >= seq_trk_start[s], RTMODT_E_INVALID, "stitch_tracks: sequence %d: the tracklet CSR is not monotone", s);
    const int n_trk = seq_trk_start[n_seq];
    RT_CHECK(n_trk <= (1 << 30), RTMODT_E_CAPACITY, "stitch_tracks: %d tracklets in one call (at most 2^30)", n_trk);
    for (int s = 0; s < n_seq; ++s) { seq_links[s] = 0; seq_cost[s] = 0.0; }
    if (n_trk == 0) return RTMODT_OK;
    RT_CHECK(trk_row_start && row_frame && row_box && trk_succ && trk_root && trk_link_d2, RTMODT_E_INVALID, "stitch_tracks: null tracklet or row arrays");
    RT_CHECK(trk_row_start[0] == 0, RTMODT_E_INVALID, "stitch_tracks: the row CSR must start at 0");
    std::vector<int32_t> trk_seq(n_trk), order(n_trk);
    std::vector<int64_t> order_start(n_trk);
    for (int s = 0; s < n_seq; ++s)
        for (int t = seq_trk_start[s]; t < seq_trk_start[s + 1]; ++t) {
            trk_seq[t] = s;
            RT_CHECK(trk_row_start[t + 1] > trk_row_start[t], RTMODT_E_INVALID,
                     "stitch_tracks: sequence %d tracklet %d (row %d): the row CSR is not monotone (every tracklet holds a row)", s,
                     t - seq_trk_start[s], trk_row_start[t]);
            for (int r = trk_row_start[t]; r < trk_row_start[t + 1]; ++r) {
                RT_CHECK(row_frame[r] >= -ST_MAX_FRAME && row_frame[r] <= ST_MAX_FRAME, RTMODT_E_INVALID,
                         "stitch_tracks: sequence %d row %d: frame %lld outside +-2^53", s, r, (long long)row_frame[r]);
                RT_CHECK(r == trk_row_start[t] || row_frame[r] > row_frame[r - 1], RTMODT_E_INVALID,
                         "stitch_tracks: sequence %d row %d: frames must ascend strictly inside a tracklet (%lld after %lld)", s, r,
                         (long long)row_frame[r], (long long)row_frame[r == 0 ? 0 : r - 1]);
                for (int q = 0; q < 4; ++q)
                    RT_CHECK(std::isfinite(row_box[4 * (size_t)r + q]), RTMODT_E_INVALID, "stitch_tracks: sequence %d row %d has a NaN or infinite box", s, r);
            }
        }
    const int n_rows = trk_row_start[n_trk];
    // the tracklets of every sequence by (start frame, index)
    std::iota(order.begin(), order.end(), 0);
    for (int s = 0; s < n_seq; ++s)
        std::sort(order.begin() + seq_trk_start[s], order.begin() + seq_trk_start[s + 1], [&](int32_t x, int32_t y) {
            const int64_t fx = row_frame[trk_row_start[x]], fy = row_frame[trk_row_start[y]];
            return fx < fy || (fx == fy && x < y);
        });
    for (int t = 0; t < n_trk; ++t) order_start[t] = row_frame[trk_row_start[order[t]]];

    RT_HIP(hipSetDevice(device));
    DevBufs B;
    StitchArgs a{};
    a.n_trk = n_trk; a.max_gap = params->max_gap; a.vwin = params->velocity_window; a.interpolate = params->interpolate;
    a.max_d2 = params->max_dist * params->max_dist;
    int32_t *d_seq, *d_sts, *d_trs, *d_order;
    int64_t *d_rf, *d_os, *d_ls;
    double *d_rb;
    RT_TRY(B.up(&d_seq, trk_seq.data(), n_trk)); RT_TRY(B.up(&d_sts, seq_trk_start, n_seq + 1)); RT_TRY(B.up(&d_trs, trk_row_start, n_trk + 1));
    RT_TRY(B.up(&d_rf, row_frame, n_rows)); RT_TRY(B.up(&d_rb, row_box, (size_t)n_rows * 4));
    RT_TRY(B.up(&d_order, order.data(), n_trk)); RT_TRY(B.up(&d_os, order_start.data(), n_trk));
    a.trk_seq = d_seq; a.seq_trk_start = d_sts; a.trk_row_start = d_trs; a.row_frame = d_rf; a.row_box = d_rb; a.order = d_order; a.order_start = d_os;
    RT_TRY(B.alloc(&a.ts, n_trk)); RT_TRY(B.alloc(&a.te, n_trk));
    RT_TRY(B.alloc(&a.cs, (size_t)n_trk * 2)); RT_TRY(B.alloc(&a.ce, (size_t)n_trk * 2)); RT_TRY(B.alloc(&a.vel, (size_t)n_trk * 2));
    RT_TRY(B.alloc(&a.link_n, n_trk)); RT_TRY(B.alloc(&a.cdeg, n_trk)); RT_TRY(B.alloc(&a.parent, (size_t)n_trk * 2));
    RT_TRY(B.alloc(&a.key, n_trk)); RT_TRY(B.alloc(&a.key_sorted, n_trk)); RT_TRY(B.alloc(&a.colmap, n_trk));
    RT_TRY(B.alloc(&a.succ, n_trk)); RT_TRY(B.alloc(&a.anc, n_trk)); RT_TRY(B.alloc(&a.root, n_trk)); RT_TRY(B.alloc(&a.succ_d2, n_trk));
    RT_TRY(B.alloc(&a.fill_n, n_trk)); RT_TRY(B.alloc(&a.err, 1));
    const int no_err = ST_NO_ERR;
    RT_HIP(hipMemcpy(a.err, &no_err, 4, hipMemcpyHostToDevice));
    const dim3 grid(cdiv(n_trk, ST_THREADS)), block(ST_THREADS);
    hipLaunchKernelGGL(stitch_summary, grid, block, 0, 0, a);
    RT_HIP(hipGetLastError());
    // ---- count pass, then the CSR of the admissible links ----
    hipLaunchKernelGGL(stitch_links<false>, grid, block, 0, 0, a);
    RT_HIP(hipGetLastError());
    std::vector<int32_t> link_n(n_trk);
    std::vector<int64_t> link_start(n_trk + 1, 0);
    RT_HIP(hipMemcpy(link_n.data(), a.link_n, (size_t)n_trk * 4, hipMemcpyDeviceToHost));
    for (int t = 0; t < n_trk; ++t) link_start[t + 1] = link_start[t] + link_n[t];
    const size_t n_links = (size_t)link_start[n_trk];
    RT_CHECK(n_links <= (size_t(1) << 28), RTMODT_E_CAPACITY, "stitch_tracks: %zu admissible links in one call (at most 2^28)", n_links);
    if (n_cand) {
        *n_cand = (int64_t)n_links;
        RT_CHECK((int64_t)n_links <= cand_cap, RTMODT_E_CAPACITY, "stitch_tracks: %zu candidate links do not fit cand_cap %lld", n_links,
                 (long long)cand_cap);
    }
    RT_TRY(B.up(&d_ls, link_start.data(), n_trk + 1));
    a.link_start = d_ls;
    RT_TRY(B.alloc(&a.link_col, n_links)); RT_TRY(B.alloc(&a.link_d2, n_links));
    if (n_cand && cand_p) RT_TRY(B.alloc(&a.link_p, n_links * 2));
    if (n_links) {
        hipLaunchKernelGGL(stitch_links<true>, grid, block, 0, 0, a);
        RT_HIP(hipGetLastError());
        hipLaunchKernelGGL(stitch_isolate, grid, block, 0, 0, a);
        RT_HIP(hipGetLastError());
        hipLaunchKernelGGL(stitch_label, grid, block, 0, 0, a);
        RT_HIP(hipGetLastError());
        size_t tb = 0;
        RT_HIP(rocprim::radix_sort_keys(nullptr, tb, a.key, a.key_sorted, (unsigned)n_trk));
        unsigned char *tmp;
        RT_TRY(B.alloc(&tmp, tb));
        RT_HIP(rocprim::radix_sort_keys((void *)tmp, tb, a.key, a.key_sorted, (unsigned)n_trk));
        hipLaunchKernelGGL(stitch_assign, dim3(n_trk), dim3(64), 0, 0, a);
        RT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(stitch_roots, grid, block, 0, 0, a);
    RT_HIP(hipGetLastError());
    int err = ST_NO_ERR;
    RT_HIP(hipMemcpy(&err, a.err, 4, hipMemcpyDeviceToHost));
    RT_CHECK(err == ST_NO_ERR, RTMODT_E_CAPACITY,
             "stitch_tracks: sequence %d: the contested component of tracklet %d exceeds %d rows / %d columns / %d links", trk_seq[err < n_trk ? err : 0],
             err < n_trk ? err - seq_trk_start[trk_seq[err]] : -1, LAP_ROWS, LAP_COLS, LAP_EDGES);
    std::vector<int32_t> fill_n(n_trk);
    RT_HIP(hipMemcpy(trk_succ, a.succ, (size_t)n_trk * 4, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(trk_root, a.root, (size_t)n_trk * 4, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(trk_link_d2, a.succ_d2, (size_t)n_trk * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(fill_n.data(), a.fill_n, (size_t)n_trk * 4, hipMemcpyDeviceToHost));
    if (n_cand && n_links) {
        std::vector<int32_t> rows(n_links);
        for (int t = 0; t < n_trk; ++t) std::fill(rows.begin() + link_start[t], rows.begin() + link_start[t + 1], t);
        memcpy(cand_a, rows.data(), n_links * 4);
        RT_HIP(hipMemcpy(cand_b, a.link_col, n_links * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(cand_d2, a.link_d2, n_links * 8, hipMemcpyDeviceToHost));
        if (cand_p) RT_HIP(hipMemcpy(cand_p, a.link_p, n_links * 16, hipMemcpyDeviceToHost));
    }
    for (int t = 0; t < n_trk; ++t)
        if (trk_succ[t] >= 0) { seq_links[trk_seq[t]] += 1; seq_cost[trk_seq[t]] += trk_link_d2[t]; }   // tracklet order
    // ---- the fill rows ----
    std::vector<int64_t> fill_start(n_trk + 1, 0);
    for (int t = 0; t < n_trk; ++t) fill_start[t + 1] = fill_start[t] + fill_n[t];
    const int64_t need = fill_start[n_trk];
    *n_fill = need;
    a.n_fill_write = std::min(need, fill_cap);
    if (a.n_fill_write > 0) {
        int64_t *d_fs;
        RT_TRY(B.up(&d_fs, fill_start.data(), n_trk + 1));
        a.fill_start = d_fs;
        RT_TRY(B.alloc(&a.fill_trk, (size_t)a.n_fill_write)); RT_TRY(B.alloc(&a.fill_frame, (size_t)a.n_fill_write));
        RT_TRY(B.alloc(&a.fill_box, (size_t)a.n_fill_write * 4));
        hipLaunchKernelGGL(stitch_fill, dim3((unsigned)((a.n_fill_write + ST_THREADS - 1) / ST_THREADS)), block, 0, 0, a);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpy(fill_trk, a.fill_trk, (size_t)a.n_fill_write * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(fill_frame, a.fill_frame, (size_t)a.n_fill_write * 8, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(fill_box, a.fill_box, (size_t)a.n_fill_write * 32, hipMemcpyDeviceToHost));
    }
    RT_HIP(hipDeviceSynchronize());
    RT_CHECK(need <= fill_cap, RTMODT_E_CAPACITY, "stitch_tracks: %lld fill rows do not fit fill_cap %lld", (long long)need, (long long)fill_cap);
    return RTMODT_OK;
}

}  // extern "C"
