// lap.h -- the sparse shortest-augmenting-path assignment solver shared by the tracker's lapjv branch (tracker.hip:
// assoc_lap) and the evaluator (eval.hip: the per-frame CLEAR MOT assignment on the device, the IDF1 identity pairing on
// the host; hota.hip: the per-frame HOTA matching on the device).
//
// The problem: rows 0..nhr-1, each with a private dummy column of cost 0 (= stay unmatched) and real edges (CSR:
// estart / ecol / ecost) of cost < 0.  lap_solve finds the minimum-cost assignment, row by row, with Jonker-Volgenant style
// Dijkstra scans over the touched columns only.  The cost type C is any totally ordered additive group:
//   double    the tracker (edge cost c_ij - cost_limit), unchanged from when this code lived in tracker.hip; HOTA (edge
//             cost -score: a maximum-weight matching)
//   LexCost   (count, distance) compared lexicographically: edge cost (-1, d) makes the optimum "maximum cardinality, then
//             minimum sum of d" exactly -- the count part is an integer, so no large constant is folded into d
//   long long exact integer weights (edge cost -n): a maximum-weight matching
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

namespace rtmodt {

// Capacities of the arrays below, inclusive: a problem of <= 256 rows, <= 256 columns and <= 2048 edges is solved; the callers
// that compact into them (assoc_sparse in track_dev.h, mot_accumulate in eval.hip, hota_match in hota.hip) refuse one more of any with a capacity error.
constexpr int LAP_ROWS = 256, LAP_COLS = 256, LAP_EDGES = 2048;

struct LexCost {
    int n;
    double d;
};
__host__ __device__ __forceinline__ LexCost operator+(LexCost a, LexCost b) { return LexCost{a.n + b.n, a.d + b.d}; }
__host__ __device__ __forceinline__ LexCost operator-(LexCost a, LexCost b) { return LexCost{a.n - b.n, a.d - b.d}; }
__host__ __device__ __forceinline__ LexCost &operator+=(LexCost &a, LexCost b) { a = a + b; return a; }
__host__ __device__ __forceinline__ LexCost &operator-=(LexCost &a, LexCost b) { a = a - b; return a; }
__host__ __device__ __forceinline__ bool operator<(LexCost a, LexCost b) { return a.n < b.n || (a.n == b.n && a.d < b.d); }
__host__ __device__ __forceinline__ bool operator==(LexCost a, LexCost b) { return a.n == b.n && a.d == b.d; }

template <typename C> struct LapCost;
template <> struct LapCost<double> {
    __host__ __device__ static double zero() { return 0.0; }
    __host__ __device__ static double inf() { return __builtin_huge_val(); }
};
template <> struct LapCost<LexCost> {
    __host__ __device__ static LexCost zero() { return LexCost{0, 0.0}; }
    __host__ __device__ static LexCost inf() { return LexCost{INT_MAX, __builtin_huge_val()}; }
};
template <> struct LapCost<long long> {
    __host__ __device__ static long long zero() { return 0; }
    __host__ __device__ static long long inf() { return LLONG_MAX; }
};

template <typename C> struct LapSmemT {
    int *colmap;                   // [n_cols capacity] column -> local index among contested columns (-1 none, -2 marked)
    C *ecost, *u, *v, *minv;       // [edges], [rows], [cols], [cols]
    int *hrow, *hcol, *estart, *ecol;         // [rows], [cols], [rows + 1], [edges]
    int *p, *rm, *wayrow, *touched, *usedl;   // col -> row, row -> col, col -> row it was reached from, lists
    unsigned char *used;           // [cols]
};
using LapSmem = LapSmemT<double>;

static inline size_t lap_smem_bytes(int Nc) {
    return (size_t)LAP_EDGES * 12 + (size_t)LAP_ROWS * (8 + 4 + 4 + 4) + (size_t)LAP_COLS * (8 + 8 + 4 + 4 + 4 + 4 + 4 + 1) + (size_t)Nc * 4 + 64;
}
template <typename C> __device__ __forceinline__ LapSmemT<C> lap_carve_t(unsigned char *base, int Nc) {     // base 8-byte aligned; any 8-byte cost type
    static_assert(sizeof(C) == 8, "lap_smem_bytes counts 8 bytes per cost");
    LapSmemT<C> L;
    L.ecost = (C *)base;
    L.u = L.ecost + LAP_EDGES;
    L.v = L.u + LAP_ROWS;
    L.minv = L.v + LAP_COLS;
    L.colmap = (int *)(L.minv + LAP_COLS);
    L.hrow = L.colmap + Nc;
    L.hcol = L.hrow + LAP_ROWS;
    L.estart = L.hcol + LAP_COLS;
    L.ecol = L.estart + LAP_ROWS + 1;
    L.p = L.ecol + LAP_EDGES;
    L.rm = L.p + LAP_COLS;
    L.wayrow = L.rm + LAP_ROWS;
    L.touched = L.wayrow + LAP_COLS;
    L.usedl = L.touched + LAP_COLS;
    L.used = (unsigned char *)(L.usedl + LAP_COLS);
    return L;
}

__device__ __forceinline__ LapSmem lap_carve(unsigned char *base, int Nc) { return lap_carve_t<double>(base, Nc); }

// Exact sparse assignment, run by ONE lane (or the host).  On entry: u[0..nhr) = 0, rm = -1; for every column v = 0,
// minv = inf, p = -1, used = 0.  On exit rm[row] is the row's column or -1 (its dummy).  Only the source row's edges can
// have a negative reduced cost, so the Dijkstra scan is valid; only touched columns are ever visited or reset.
template <typename C>
__host__ __device__ void lap_solve(const LapSmemT<C> &L, int nhr) {
    const C INF = LapCost<C>::inf();
    for (int h0 = 0; h0 < nhr; ++h0) {
        int nt = 0, nu = 0, i0 = h0, jend = -1, drow = -1;
        C dmin = INF;
        bool to_dummy = false;
        while (true) {
            const C ui = L.u[i0];
            for (int e = L.estart[i0]; e < L.estart[i0 + 1]; ++e) {          // relax the real edges of row i0
                const int j = L.ecol[e];
                if (L.used[j]) continue;
                const C cur = L.ecost[e] - ui - L.v[j];
                if (L.minv[j] == INF) L.touched[nt++] = j;
                if (cur < L.minv[j]) { L.minv[j] = cur; L.wayrow[j] = i0; }
            }
            if (LapCost<C>::zero() - ui < dmin) { dmin = LapCost<C>::zero() - ui; drow = i0; }   // ... and its dummy edge
            C delta = dmin;
            int j1 = -1;
            for (int t = 0; t < nt; ++t) {
                const int j = L.touched[t];
                if (!L.used[j] && L.minv[j] < delta) { delta = L.minv[j]; j1 = j; }
            }
            L.u[h0] += delta;
            for (int t = 0; t < nu; ++t) { const int j = L.usedl[t]; L.u[L.p[j]] += delta; L.v[j] -= delta; }
            for (int t = 0; t < nt; ++t) { const int j = L.touched[t]; if (!L.used[j]) L.minv[j] -= delta; }
            dmin -= delta;
            if (j1 < 0) { to_dummy = true; break; }
            if (L.p[j1] < 0) { jend = j1; break; }
            L.used[j1] = 1;
            L.usedl[nu++] = j1;
            i0 = L.p[j1];
        }
        if (to_dummy) {                                   // row drow gives up its column; shift the path back to h0
            int i = drow, jfree = L.rm[i];
            L.rm[i] = -1;
            while (i != h0) {
                const int j = jfree, ip = L.wayrow[j];
                jfree = L.rm[ip];
                L.p[j] = ip;
                L.rm[ip] = j;
                i = ip;
            }
        } else {
            int j = jend;
            while (true) {
                const int ip = L.wayrow[j], jn = L.rm[ip];
                L.p[j] = ip;
                L.rm[ip] = j;
                if (ip == h0) break;
                j = jn;
            }
        }
        for (int t = 0; t < nt; ++t) { const int j = L.touched[t]; L.minv[j] = INF; L.used[j] = 0; }
    }
}

}  // namespace rtmodt
