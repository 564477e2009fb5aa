// hota.hip -- HOTA (Luiten et al., "HOTA: A Higher Order Metric for Evaluating Multi-Object Tracking", IJCV 2021) on the GPU,
// beside eval.hip's CLEAR MOT and IDF1: rtmodt_hota_eval restates TrackEval's trackeval/metrics/hota.py without the library.
// PARITY UNPINNED: TrackEval is installed nowhere this runs.  The rules below are the normative restatement (INTEGRATION.md
// section 17); tests/hota_ref.py states them in plain Python / NumPy and the GPU tests require bit identity with it.  The
// restatement's per-frame matching is pinned to scipy.optimize.linear_sum_assignment, the solver TrackEval calls.
//
// Rules (all float64, every operation rounded separately; eps = 2^-52 = np.finfo(float).eps):
//   input       rtmodt_mot_eval's: many sequences per call, a sequence's frames ascending, GT / hypothesis rows per frame
//               as CSR, boxes x, y, w, h, dense ids per sequence.  Rows are evaluated as given (no benchmark preprocessing).
//   similarity  S[o, h] = the evaluator's IoU (eval_dev.h: mot_iou; mot_eval's d is 1 - S).  Only pairs with S > 0 are
//               stored; every other pair contributes exactly 0 everywhere.
//   thresholds  alphas[n_alpha], ascending, used as given, n_alpha <= 32.
//   pass 1      per frame: r[o] = sum_h S[o, h] in ascending hypothesis row, c[h] = sum_o S[o, h] in ascending GT row;
//               per stored pair q = S / ((r[o] + c[h]) - S) if that denominator > eps, else 0.  Per sequence:
//               pmc(o, h) = sum of q over the frames in ascending frame order; gtc(o), trc(h) = the frames in which the id
//               appears; gas(o, h) = pmc / ((gtc(o) + trc(h)) - pmc).
//   pass 2      per frame, frames independent: one maximum-weight one-to-one matching of the edges with
//               score = gas(o, h) * S[o, h] > 0.  Isolated edges (the only edge of their row and of their column) are taken
//               directly; the contested remainder goes to lap_solve<double> with edge cost -score, rows in ascending GT row,
//               a row's edges in ascending hypothesis row, contested columns numbered in first-touch order.  A matched pair
//               counts at alpha when S >= alpha - eps: the alphas ascend, so a match passes a prefix of them and one
//               integer per match (the prefix length) builds every mc_alpha.  Per sequence and alpha, k counting matches
//               in the frame: TP += k, FN += nO - k, FP += nH - k, loc_sum += S of the counting matches in ascending frame,
//               then ascending GT row; mc_alpha(o, h) += 1.
//   finish      per sequence and alpha over the (o, h) with mc > 0 in ascending (o, h):
//               ass_a_sum += mc * (mc / ((gtc + trc) - mc)), ass_re_sum += mc * (mc / max(1, gtc)),
//               ass_pr_sum += mc * (mc / max(1, trc)).  On the host, from the sparse integer table.
//   limits      mot_eval's: 1024 rows per frame and side, 2^28 stored pairs per call; a contested remainder above 256 rows /
//               256 columns / 2048 edges fails with RTMODT_E_CAPACITY naming the sequence and frame, before anything is counted.
//
// Kernels (a fixed number of launches per call, whatever the number of sequences):
//   hota_pairs<false>  one wave per frame: the count of S > 0 pairs, the row / column sums r, c and the id counts gtc, trc
//   hota_pairs<true>   (after a host scan of the counts) the pairs compacted in (GT row, hyp row) order into the frame's CSR
//                      slice with S, q and the (sequence, o, h) key
//   (rocPRIM)          radix_sort_pairs (stable: equal keys stay in frame order) of (key, pair index), run_length_encode,
//                      exclusive_scan of the run lengths: the sparse (sequence, o, h) table
//   hota_gas           one thread per (o, h) run: pmc summed in frame order, gas, then score = gas * S of each of its pairs
//   hota_match         one workgroup per frame: degrees, isolated edges, the contested rest by ONE lane with the solver's
//                      state in LDS; per GT row the matched S and the number of alphas it passes
//   hota_mc            one thread per run: mc_alpha from the prefix lengths of its pairs
//   hota_loc           one wave per sequence, lane = alpha: TP and loc_sum walking the GT rows in order
//
// Built with -ffp-contract=off: every float64 operation rounds separately, as NumPy's do.
#include "common.h"
#include "eval_dev.h"
#include "lap.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <climits>
#include <vector>

namespace rtmodt {

#pragma clang fp contract(off)

constexpr int HOTA_MAX_ALPHA = 32;
constexpr double HOTA_EPS = 2.220446049250313e-16;

struct HotaArgs {
    int n_frames, n_seq, n_alpha;
    const int32_t *frame_seq;               // [n_frames]
    const int32_t *seq_frame_start;         // [n_seq + 1]
    const int32_t *gt_start, *hyp_start;    // [n_frames + 1] into the GT / hypothesis rows
    const int32_t *gt_oid, *hyp_hid;        // [n_gt], [n_hyp]: dense ids within the sequence
    const double *gt_box, *hyp_box;         // [n][4] x, y, w, h
    const double *alphas;                   // [n_alpha]
    const uint64_t *key_base;               // [n_seq]: key = key_base[seq] + oid * n_hid + hid
    const int32_t *seq_n_hid;               // [n_seq]
    const int32_t *oid_start, *hid_start;   // [n_seq]: the sequence's slice of gtc / trc
    int32_t *gtc, *trc;                     // frames in which the id appears
    double *rsum, *csum;                    // [n_gt], [n_hyp]: the frame's row / column sums of S
    int32_t *pair_n;                        // [n_frames] stored pairs of the frame (count pass)
    const int64_t *pair_start;              // [n_frames + 1]
    int32_t *pair_o, *pair_h;               // local row indices, (GT row, hyp row) order inside a frame
    int32_t *pair_go, *pair_gh;             // the pair's ids as indices into gtc / trc
    double *pair_s, *pair_q, *pair_score;
    uint64_t *pair_key;
    uint32_t *pair_idx;                     // iota: the sort's values
    uint8_t *pair_na;                       // alphas the pair's match passes (0: not matched in its frame)
    const uint32_t *sorted_idx, *run_cnt, *run_start;   // pairs ordered by (key, frame); [n_runs] lengths and offsets
    uint32_t n_runs;
    int32_t *mc;                            // [n_runs][n_alpha]
    double *row_s;                          // [n_gt] S of the GT row's match
    int32_t *row_na;                        // [n_gt] alphas it passes
    int32_t *err_frame;                     // the first frame whose contested remainder exceeds the solver's limits
    int64_t *tp;                            // [n_seq][n_alpha]
    double *loc;                            // [n_seq][n_alpha]
    int max_rows, lap_bytes;                // LDS sizing of hota_match
};

// WRITE = false: the count pass, the row / column sums and the id counts; WRITE = true: the same S > 0 decisions again,
// compacted into the frame's CSR slice
template <bool WRITE>
__global__ __launch_bounds__(EV_THREADS) void hota_pairs(HotaArgs a) {
    const int f = blockIdx.x * EV_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= a.n_frames) return;
    const int go = a.gt_start[f], nO = a.gt_start[f + 1] - go;
    const int gh = a.hyp_start[f], nH = a.hyp_start[f + 1] - gh;
    const int s = a.frame_seq[f];
    if (!WRITE) {
        for (int o = lane; o < nO; o += 64) {              // r[o]: ascending hypothesis row (a zero adds exactly nothing)
            double r = 0.0;
            for (int h = 0; h < nH; ++h) r += mot_iou(a.gt_box + (size_t)(go + o) * 4, a.hyp_box + (size_t)(gh + h) * 4);
            a.rsum[go + o] = r;
            atomicAdd(&a.gtc[a.oid_start[s] + a.gt_oid[go + o]], 1);
        }
        for (int h = lane; h < nH; h += 64) {              // c[h]: ascending GT row
            double c = 0.0;
            for (int o = 0; o < nO; ++o) c += mot_iou(a.gt_box + (size_t)(go + o) * 4, a.hyp_box + (size_t)(gh + h) * 4);
            a.csum[gh + h] = c;
            atomicAdd(&a.trc[a.hid_start[s] + a.hyp_hid[gh + h]], 1);
        }
    }
    const uint64_t nh_ids = (uint64_t)a.seq_n_hid[s];
    const int64_t p0 = WRITE ? a.pair_start[f] : 0;
    const int total = nO * nH;
    int cnt = 0;
    for (int base = 0; base < total; base += 64) {
        const int p = base + lane;
        bool valid = false;
        int o = 0, h = 0;
        double S = 0.0;
        if (p < total) {
            o = p / nH; h = p - o * nH;
            S = mot_iou(a.gt_box + (size_t)(go + o) * 4, a.hyp_box + (size_t)(gh + h) * 4);
            valid = S > 0.0;
        }
        const unsigned long long mk = __ballot(valid);
        if (WRITE && valid) {
            const int64_t e = p0 + cnt + __popcll(mk & ((1ull << lane) - 1ull));
            const int oid = a.gt_oid[go + o], hid = a.hyp_hid[gh + h];
            const double den = (a.rsum[go + o] + a.csum[gh + h]) - S;
            a.pair_o[e] = o; a.pair_h[e] = h; a.pair_s[e] = S;
            a.pair_q[e] = den > HOTA_EPS ? S / den : 0.0;
            a.pair_go[e] = a.oid_start[s] + oid; a.pair_gh[e] = a.hid_start[s] + hid;
            a.pair_key[e] = a.key_base[s] + (uint64_t)oid * nh_ids + (uint64_t)hid;
            a.pair_idx[e] = (uint32_t)e;
        }
        cnt += __popcll(mk);
    }
    if (!WRITE && lane == 0) a.pair_n[f] = cnt;
}

// one thread per (sequence, o, h) run of the sorted pairs: the run is in frame order (the sort is stable)
__global__ __launch_bounds__(EV_THREADS) void hota_gas(HotaArgs a) {
    const uint32_t i = blockIdx.x * EV_THREADS + threadIdx.x;
    if (i >= a.n_runs) return;
    const uint32_t beg = a.run_start[i], n = a.run_cnt[i];
    double pmc = 0.0;
    for (uint32_t j = 0; j < n; ++j) pmc += a.pair_q[a.sorted_idx[beg + j]];
    const uint32_t e0 = a.sorted_idx[beg];
    const double gtc = (double)a.gtc[a.pair_go[e0]], trc = (double)a.trc[a.pair_gh[e0]];
    const double gas = pmc / ((gtc + trc) - pmc);          // q <= 1 per frame: pmc <= min(gtc, trc), the denominator >= 1
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t e = a.sorted_idx[beg + j];
        a.pair_score[e] = gas * a.pair_s[e];
    }
}

// LDS of hota_match beyond lap.h's carve (R = the most rows of a frame), all in the dynamic region
struct HotaSmem {
    int *odeg, *hdeg, *oedge;              // [R] degrees over the edges with score > 0, a row's last such edge
    int *rbeg, *rend;                      // [R] each GT row's range in the frame's pairs (they are in row order)
    int *omatch;                           // [R] the matched pair of the GT row (-1 none)
    int *wtoti;                            // [EV_WAVES]
    int *over;                             // [1]
};
__device__ __forceinline__ HotaSmem hota_carve(unsigned char *base, int R) {
    HotaSmem S;
    S.odeg = (int *)base;
    S.hdeg = S.odeg + R;
    S.oedge = S.hdeg + R;
    S.rbeg = S.oedge + R;
    S.rend = S.rbeg + R;
    S.omatch = S.rend + R;
    S.wtoti = S.omatch + R;
    S.over = S.wtoti + EV_WAVES;
    return S;
}
static size_t hota_match_smem(int R, int *lap_bytes) {
    *lap_bytes = (int)align_up(lap_smem_bytes(R), 16);
    return (size_t)*lap_bytes + (size_t)R * 6 * 4 + (EV_WAVES + 1) * 4 + 16;
}

__global__ __launch_bounds__(EV_THREADS) void hota_match(HotaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int f = blockIdx.x, tid = threadIdx.x;
    const LapSmemT<double> L = lap_carve_t<double>(smem, a.max_rows);
    const HotaSmem S = hota_carve(smem + a.lap_bytes, a.max_rows);
    int *odeg = S.odeg, *hdeg = S.hdeg, *oedge = S.oedge, *rbeg = S.rbeg, *rend = S.rend, *omatch = S.omatch;

    const int go = a.gt_start[f], nO = a.gt_start[f + 1] - go;
    const int nH = a.hyp_start[f + 1] - a.hyp_start[f];
    const int np = a.pair_n[f];
    const int64_t p0 = a.pair_start[f];
    for (int r = tid; r < nO; r += EV_THREADS) { odeg[r] = 0; rbeg[r] = 0; rend[r] = 0; omatch[r] = -1; }
    for (int c = tid; c < nH; c += EV_THREADS) { hdeg[c] = 0; L.colmap[c] = -1; }
    if (tid == 0) *S.over = 0;
    __syncthreads();
    for (int e = tid; e < np; e += EV_THREADS) {           // row ranges; degrees over the edges with score > 0
        const int r = a.pair_o[p0 + e];
        if (e == 0 || a.pair_o[p0 + e - 1] != r) rbeg[r] = e;
        if (e == np - 1 || a.pair_o[p0 + e + 1] != r) rend[r] = e + 1;
        if (a.pair_score[p0 + e] > 0.0) { atomicAdd(&odeg[r], 1); atomicAdd(&hdeg[a.pair_h[p0 + e]], 1); oedge[r] = e; }
    }
    __syncthreads();
    // isolated edges resolve directly; a row is contested when it or its one column has another edge
    int nhr = 0;
    for (int base = 0; base < nO; base += EV_THREADS) {
        const int r = base + tid;
        bool hard = false;
        if (r < nO && odeg[r] > 0) {
            const int e = oedge[r];
            if (odeg[r] == 1 && hdeg[a.pair_h[p0 + e]] == 1) omatch[r] = e;
            else hard = true;
        }
        int tot;
        const int pos = block_scan((int)hard, [](int x, int y) { return x + y; }, S.wtoti, tot) - (int)hard;
        if (hard && nhr + pos < LAP_ROWS) L.hrow[nhr + pos] = r;
        nhr += tot;
    }
    __syncthreads();
    if (nhr > 0 && tid == 0) {                             // the contested remainder: one lane, cost -score
        bool over = nhr > LAP_ROWS;
        int ne = 0, nhc = 0;
        for (int h = 0; h < nhr && !over; ++h) {
            const int r = L.hrow[h];
            L.estart[h] = ne;
            L.u[h] = 0.0;
            L.rm[h] = -1;
            for (int e = rbeg[r]; e < rend[r]; ++e) {
                const double sc = a.pair_score[p0 + e];
                if (!(sc > 0.0)) continue;
                const int c = a.pair_h[p0 + e];
                if (L.colmap[c] < 0) {
                    if (nhc == LAP_COLS) { over = true; break; }
                    L.colmap[c] = nhc; L.hcol[nhc] = c;
                    L.v[nhc] = 0.0; L.minv[nhc] = LapCost<double>::inf(); L.p[nhc] = -1; L.used[nhc] = 0;
                    ++nhc;
                }
                if (ne == LAP_EDGES) { over = true; break; }
                L.ecol[ne] = L.colmap[c];
                L.ecost[ne] = -sc;
                ++ne;
            }
        }
        if (over) {
            *S.over = 1;
            atomicMin(a.err_frame, f);
        } else {
            L.estart[nhr] = ne;
            lap_solve(L, nhr);
            for (int h = 0; h < nhr; ++h)
                if (L.rm[h] >= 0) {
                    const int r = L.hrow[h], c = L.hcol[L.rm[h]];
                    for (int e = rbeg[r]; e < rend[r]; ++e)
                        if (a.pair_h[p0 + e] == c) { omatch[r] = e; break; }
                }
        }
    }
    __syncthreads();
    const bool over = *S.over != 0;
    for (int r = tid; r < nO; r += EV_THREADS) {
        const int e = over ? -1 : omatch[r];
        double s = 0.0;
        int na = 0;
        if (e >= 0) {
            s = a.pair_s[p0 + e];
            for (int k = 0; k < a.n_alpha; ++k) na += s >= a.alphas[k] - HOTA_EPS;   // ascending alphas: a prefix
            a.pair_na[p0 + e] = (uint8_t)na;
        }
        a.row_s[go + r] = s;
        a.row_na[go + r] = na;
    }
}

// one thread per run: mc_alpha(o, h) = its pairs whose match passes more than `alpha index` thresholds (mc zeroed by the host)
__global__ __launch_bounds__(EV_THREADS) void hota_mc(HotaArgs a) {
    const uint32_t i = blockIdx.x * EV_THREADS + threadIdx.x;
    if (i >= a.n_runs) return;
    const uint32_t beg = a.run_start[i], n = a.run_cnt[i];
    int32_t *m = a.mc + (size_t)i * a.n_alpha;
    for (uint32_t j = 0; j < n; ++j) {
        const int na = a.pair_na[a.sorted_idx[beg + j]];
        if (na) m[na - 1] += 1;
    }
    for (int k = a.n_alpha - 2; k >= 0; --k) m[k] += m[k + 1];
}

// one wave per sequence, lane = alpha index: TP and loc_sum over the GT rows in ascending (frame, GT row) order
__global__ __launch_bounds__(64) void hota_loc(HotaArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int g0 = a.gt_start[a.seq_frame_start[s]], g1 = a.gt_start[a.seq_frame_start[s + 1]];
    double loc = 0.0;
    long long tp = 0;
    for (int base = g0; base < g1; base += 64) {
        const int g = base + lane;
        const double sv = g < g1 ? a.row_s[g] : 0.0;
        const int nv = g < g1 ? a.row_na[g] : 0;
        if (__ballot(nv > 0) == 0ull) continue;
        const int cnt = min(64, g1 - base);
        for (int j = 0; j < cnt; ++j) {
            const double sj = __shfl(sv, j);
            const int nj = __shfl(nv, j);
            if (nj > lane) { loc += sj; ++tp; }
        }
    }
    if (lane < a.n_alpha) {
        a.tp[(size_t)s * a.n_alpha + lane] = tp;
        a.loc[(size_t)s * a.n_alpha + lane] = loc;
    }
}

}  // namespace rtmodt

using namespace rtmodt;

extern "C" {

int rtmodt_hota_eval(int device, int n_seq, const int32_t *seq_frame_start, const int64_t *frame_id, const int32_t *gt_start,
                     const int32_t *hyp_start, const int32_t *gt_oid, const double *gt_box, const int32_t *hyp_hid, const double *hyp_box,
                     const int32_t *seq_n_oid, const int32_t *seq_n_hid, const double *alphas, int n_alpha, rtmodt_hota_counts *out) {
    RT_CHECK(n_seq >= 0 && alphas && n_alpha >= 1, RTMODT_E_INVALID, "hota_eval: bad argument");
    RT_CHECK(n_alpha <= HOTA_MAX_ALPHA, RTMODT_E_CAPACITY, "hota_eval: %d alphas (at most %d)", n_alpha, HOTA_MAX_ALPHA);
    for (int k = 0; k < n_alpha; ++k)
        RT_CHECK(alphas[k] == alphas[k] && (k == 0 || alphas[k] >= alphas[k - 1]), RTMODT_E_INVALID, "hota_eval: the alphas must ascend (index %d)", k);
    if (n_seq == 0) return RTMODT_OK;
    RT_CHECK(seq_frame_start && frame_id && gt_start && hyp_start && seq_n_oid && seq_n_hid && out, RTMODT_E_INVALID, "hota_eval: bad argument");
    RT_CHECK(seq_frame_start[0] == 0, RTMODT_E_INVALID, "hota_eval: frame CSR must start at 0");
    const int n_frames = seq_frame_start[n_seq];
    RT_CHECK(n_frames >= 0 && gt_start[0] == 0 && hyp_start[0] == 0, RTMODT_E_INVALID, "hota_eval: row CSR must start at 0");
    std::vector<int32_t> frame_seq(n_frames), oid_start(n_seq + 1, 0), hid_start(n_seq + 1, 0);
    std::vector<uint64_t> key_base(n_seq + 1, 0);
    int max_rows = 1;
    for (int s = 0; s < n_seq; ++s) {
        RT_CHECK(seq_frame_start[s + 1] >= seq_frame_start[s] && seq_n_oid[s] >= 0 && seq_n_hid[s] >= 0, RTMODT_E_INVALID,
                 "hota_eval: sequence %d is malformed", s);
        for (int f = seq_frame_start[s]; f < seq_frame_start[s + 1]; ++f) {
            frame_seq[f] = s;
            const int nO = gt_start[f + 1] - gt_start[f], nH = hyp_start[f + 1] - hyp_start[f];
            RT_CHECK(nO >= 0 && nH >= 0, RTMODT_E_INVALID, "hota_eval: sequence %d frame %lld: malformed rows", s, (long long)frame_id[f]);
            RT_CHECK(nO <= MOT_MAX_ROWS && nH <= MOT_MAX_ROWS, RTMODT_E_CAPACITY,
                     "hota_eval: sequence %d frame %lld holds %d GT / %d hypothesis rows (at most %d each)", s, (long long)frame_id[f], nO, nH,
                     MOT_MAX_ROWS);
            for (int r = gt_start[f]; r < gt_start[f + 1]; ++r)
                RT_CHECK(gt_oid && gt_oid[r] >= 0 && gt_oid[r] < seq_n_oid[s], RTMODT_E_INVALID, "hota_eval: GT row %d: object index out of range", r);
            for (int r = hyp_start[f]; r < hyp_start[f + 1]; ++r)
                RT_CHECK(hyp_hid && hyp_hid[r] >= 0 && hyp_hid[r] < seq_n_hid[s], RTMODT_E_INVALID, "hota_eval: hypothesis row %d: index out of range", r);
            max_rows = std::max(max_rows, std::max(nO, nH));
        }
        key_base[s + 1] = key_base[s] + (uint64_t)seq_n_oid[s] * (uint64_t)seq_n_hid[s];   // < 2^62 per sequence
        RT_CHECK(key_base[s + 1] >= key_base[s], RTMODT_E_CAPACITY, "hota_eval: the id key space of one call overflows 64 bits");
        RT_CHECK((int64_t)oid_start[s] + seq_n_oid[s] <= INT_MAX && (int64_t)hid_start[s] + seq_n_hid[s] <= INT_MAX, RTMODT_E_CAPACITY,
                 "hota_eval: more than 2^31 - 1 ids in one call");
        oid_start[s + 1] = oid_start[s] + seq_n_oid[s];
        hid_start[s + 1] = hid_start[s] + seq_n_hid[s];
    }
    const int n_gt = gt_start[n_frames], n_hyp = hyp_start[n_frames];
    RT_CHECK((n_gt == 0 || (gt_oid && gt_box)) && (n_hyp == 0 || (hyp_hid && hyp_box)), RTMODT_E_INVALID, "hota_eval: null row arrays");
    const size_t n_oid = (size_t)oid_start[n_seq], n_hid = (size_t)hid_start[n_seq];
    int lap_bytes = 0;
    const size_t smem = hota_match_smem(max_rows, &lap_bytes);
    RT_CHECK(smem <= 160 * 1024, RTMODT_E_CAPACITY, "hota_eval: %d rows per frame need %zu B of LDS", max_rows, smem);

    RT_HIP(hipSetDevice(device));
    DevBufs B;
    HotaArgs ha{};
    ha.n_frames = n_frames; ha.n_seq = n_seq; ha.n_alpha = n_alpha; ha.max_rows = max_rows; ha.lap_bytes = lap_bytes;
    int32_t *d_fs, *d_sfs, *d_gs, *d_hs, *d_oid, *d_hid, *d_nh, *d_os, *d_his;
    double *d_gb, *d_hb, *d_al;
    int64_t *d_ps;
    uint64_t *d_kb;
    RT_TRY(B.up(&d_fs, frame_seq.data(), n_frames)); RT_TRY(B.up(&d_sfs, seq_frame_start, n_seq + 1));
    RT_TRY(B.up(&d_gs, gt_start, n_frames + 1)); RT_TRY(B.up(&d_hs, hyp_start, n_frames + 1));
    RT_TRY(B.up(&d_oid, gt_oid, n_gt)); RT_TRY(B.up(&d_hid, hyp_hid, n_hyp));
    RT_TRY(B.up(&d_gb, gt_box, (size_t)n_gt * 4)); RT_TRY(B.up(&d_hb, hyp_box, (size_t)n_hyp * 4));
    RT_TRY(B.up(&d_kb, key_base.data(), n_seq + 1)); RT_TRY(B.up(&d_nh, seq_n_hid, n_seq));
    RT_TRY(B.up(&d_os, oid_start.data(), n_seq + 1)); RT_TRY(B.up(&d_his, hid_start.data(), n_seq + 1));
    RT_TRY(B.up(&d_al, alphas, n_alpha));
    ha.frame_seq = d_fs; ha.seq_frame_start = d_sfs; ha.gt_start = d_gs; ha.hyp_start = d_hs; ha.gt_oid = d_oid; ha.hyp_hid = d_hid;
    ha.gt_box = d_gb; ha.hyp_box = d_hb; ha.key_base = d_kb; ha.seq_n_hid = d_nh; ha.oid_start = d_os; ha.hid_start = d_his; ha.alphas = d_al;
    RT_TRY(B.alloc(&ha.pair_n, n_frames));
    RT_TRY(B.alloc(&ha.gtc, n_oid)); RT_TRY(B.alloc(&ha.trc, n_hid));
    RT_TRY(B.alloc(&ha.rsum, n_gt)); RT_TRY(B.alloc(&ha.csum, n_hyp));
    RT_TRY(B.alloc(&ha.row_s, n_gt)); RT_TRY(B.alloc(&ha.row_na, n_gt));
    RT_TRY(B.alloc(&ha.err_frame, 1));
    RT_TRY(B.alloc(&ha.tp, (size_t)n_seq * n_alpha)); RT_TRY(B.alloc(&ha.loc, (size_t)n_seq * n_alpha));
    RT_HIP(hipMemset(ha.gtc, 0, std::max<size_t>(n_oid, 1) * 4));
    RT_HIP(hipMemset(ha.trc, 0, std::max<size_t>(n_hid, 1) * 4));
    const int32_t no_err = INT_MAX;
    RT_HIP(hipMemcpy(ha.err_frame, &no_err, 4, hipMemcpyHostToDevice));
    // ---- count pass (with the row / column sums and the id counts), then the per-frame CSR of the S > 0 pairs ----
    std::vector<int32_t> pair_n(n_frames);
    std::vector<int64_t> pair_start(n_frames + 1, 0);
    if (n_frames) {
        hipLaunchKernelGGL(hota_pairs<false>, dim3(cdiv(n_frames, EV_WAVES)), dim3(EV_THREADS), 0, 0, ha);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpy(pair_n.data(), ha.pair_n, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
    }
    for (int f = 0; f < n_frames; ++f) pair_start[f + 1] = pair_start[f] + pair_n[f];
    const size_t npairs = (size_t)pair_start[n_frames];
    RT_CHECK(npairs <= (size_t(1) << 28), RTMODT_E_CAPACITY, "hota_eval: %zu overlapping (IoU > 0) pairs in one call (at most 2^28)", npairs);
    RT_TRY(B.up(&d_ps, pair_start.data(), n_frames + 1));
    ha.pair_start = d_ps;
    RT_TRY(B.alloc(&ha.pair_o, npairs)); RT_TRY(B.alloc(&ha.pair_h, npairs)); RT_TRY(B.alloc(&ha.pair_go, npairs)); RT_TRY(B.alloc(&ha.pair_gh, npairs));
    RT_TRY(B.alloc(&ha.pair_s, npairs)); RT_TRY(B.alloc(&ha.pair_q, npairs)); RT_TRY(B.alloc(&ha.pair_score, npairs));
    RT_TRY(B.alloc(&ha.pair_key, npairs)); RT_TRY(B.alloc(&ha.pair_idx, npairs)); RT_TRY(B.alloc(&ha.pair_na, npairs));
    RT_HIP(hipMemset(ha.pair_na, 0, std::max<size_t>(npairs, 1)));
    if (n_frames) {
        hipLaunchKernelGGL(hota_pairs<true>, dim3(cdiv(n_frames, EV_WAVES)), dim3(EV_THREADS), 0, 0, ha);
        RT_HIP(hipGetLastError());
    }
    // ---- the sparse (sequence, o, h) table: a stable sort of (key, pair), run lengths and their offsets ----
    uint64_t *d_skey, *d_unique;
    uint32_t *d_sidx, *d_cnt, *d_off, *d_nruns;
    RT_TRY(B.alloc(&d_skey, npairs)); RT_TRY(B.alloc(&d_sidx, npairs)); RT_TRY(B.alloc(&d_unique, npairs));
    RT_TRY(B.alloc(&d_cnt, npairs)); RT_TRY(B.alloc(&d_off, npairs)); RT_TRY(B.alloc(&d_nruns, 1));
    uint32_t nruns = 0;
    if (npairs) {
        size_t tb = 0, tb2 = 0, tb3 = 0;
        RT_HIP(rocprim::radix_sort_pairs(nullptr, tb, ha.pair_key, d_skey, ha.pair_idx, d_sidx, (unsigned)npairs));
        RT_HIP(rocprim::run_length_encode(nullptr, tb2, d_skey, (unsigned)npairs, d_unique, d_cnt, d_nruns));
        RT_HIP(rocprim::exclusive_scan(nullptr, tb3, d_cnt, d_off, 0u, npairs, rocprim::plus<uint32_t>()));
        unsigned char *tmp;
        RT_TRY(B.alloc(&tmp, std::max(tb, std::max(tb2, tb3))));
        RT_HIP(rocprim::radix_sort_pairs((void *)tmp, tb, ha.pair_key, d_skey, ha.pair_idx, d_sidx, (unsigned)npairs));
        RT_HIP(rocprim::run_length_encode((void *)tmp, tb2, d_skey, (unsigned)npairs, d_unique, d_cnt, d_nruns));
        RT_HIP(hipMemcpy(&nruns, d_nruns, 4, hipMemcpyDeviceToHost));
        RT_HIP(rocprim::exclusive_scan((void *)tmp, tb3, d_cnt, d_off, 0u, (size_t)nruns, rocprim::plus<uint32_t>()));
    }
    ha.sorted_idx = d_sidx; ha.run_cnt = d_cnt; ha.run_start = d_off; ha.n_runs = nruns;
    RT_TRY(B.alloc(&ha.mc, (size_t)nruns * n_alpha));
    RT_HIP(hipMemset(ha.mc, 0, std::max<size_t>((size_t)nruns * n_alpha, 1) * 4));
    if (nruns) {
        hipLaunchKernelGGL(hota_gas, dim3(cdiv((int)nruns, EV_THREADS)), dim3(EV_THREADS), 0, 0, ha);
        RT_HIP(hipGetLastError());
    }
    // ---- the per-frame matching; a frame past the solver's limits is refused before anything is counted ----
    if (n_frames) {
        static DynLdsSeen seen;
        RT_TRY(raise_dynamic_lds((const void *)hota_match, smem, seen));
        hipLaunchKernelGGL(hota_match, dim3(n_frames), dim3(EV_THREADS), smem, 0, ha);
        RT_HIP(hipGetLastError());
    }
    int32_t err_frame = INT_MAX;
    RT_HIP(hipMemcpy(&err_frame, ha.err_frame, 4, hipMemcpyDeviceToHost));
    if (err_frame != INT_MAX) {
        RT_CHECK(err_frame >= 0 && err_frame < n_frames, RTMODT_E_HIP, "hota_eval: bad error frame %d", err_frame);
        return fail(RTMODT_E_CAPACITY, "hota_eval: sequence %d frame %lld: the contested assignment exceeds %d rows / %d columns / %d pairs",
                    frame_seq[err_frame], (long long)frame_id[err_frame], LAP_ROWS, LAP_COLS, LAP_EDGES);
    }
    if (nruns) {
        hipLaunchKernelGGL(hota_mc, dim3(cdiv((int)nruns, EV_THREADS)), dim3(EV_THREADS), 0, 0, ha);
        RT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(hota_loc, dim3(n_seq), dim3(64), 0, 0, ha);
    RT_HIP(hipGetLastError());
    RT_HIP(hipDeviceSynchronize());
    // ---- the finish on the host, from the sparse integer table (keys ascend: sequences, then objects, then hypotheses) ----
    std::vector<int64_t> tp((size_t)n_seq * n_alpha);
    std::vector<double> loc((size_t)n_seq * n_alpha);
    std::vector<int32_t> gtc(n_oid), trc(n_hid), mc((size_t)nruns * n_alpha);
    std::vector<uint64_t> ukey(nruns);
    RT_HIP(hipMemcpy(tp.data(), ha.tp, tp.size() * 8, hipMemcpyDeviceToHost));
    RT_HIP(hipMemcpy(loc.data(), ha.loc, loc.size() * 8, hipMemcpyDeviceToHost));
    if (n_oid) RT_HIP(hipMemcpy(gtc.data(), ha.gtc, n_oid * 4, hipMemcpyDeviceToHost));
    if (n_hid) RT_HIP(hipMemcpy(trc.data(), ha.trc, n_hid * 4, hipMemcpyDeviceToHost));
    if (nruns) {
        RT_HIP(hipMemcpy(mc.data(), ha.mc, mc.size() * 4, hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(ukey.data(), d_unique, (size_t)nruns * 8, hipMemcpyDeviceToHost));
    }
    for (int s = 0; s < n_seq; ++s) {
        const int64_t rows_o = gt_start[seq_frame_start[s + 1]] - gt_start[seq_frame_start[s]];
        const int64_t rows_h = hyp_start[seq_frame_start[s + 1]] - hyp_start[seq_frame_start[s]];
        for (int k = 0; k < n_alpha; ++k) {
            rtmodt_hota_counts &o = out[(size_t)s * n_alpha + k];
            o.tp = tp[(size_t)s * n_alpha + k]; o.fn = rows_o - o.tp; o.fp = rows_h - o.tp;
            o.loc_sum = loc[(size_t)s * n_alpha + k];
            o.ass_a_sum = 0.0; o.ass_re_sum = 0.0; o.ass_pr_sum = 0.0;
        }
    }
    for (size_t i = 0, s = 0; i < nruns; ++i) {
        while (ukey[i] >= key_base[s + 1]) ++s;
        const uint64_t key = ukey[i] - key_base[s];
        const double g = (double)gtc[oid_start[s] + (size_t)(key / (uint64_t)seq_n_hid[s])];
        const double t = (double)trc[hid_start[s] + (size_t)(key % (uint64_t)seq_n_hid[s])];
        for (int k = 0; k < n_alpha; ++k) {
            const int32_t n = mc[i * n_alpha + k];
            if (n <= 0) break;                                 // mc descends with alpha
            const double m = (double)n;
            rtmodt_hota_counts &o = out[s * n_alpha + k];
            o.ass_a_sum += m * (m / ((g + t) - m));
            o.ass_re_sum += m * (m / std::max(1.0, g));
            o.ass_pr_sum += m * (m / std::max(1.0, t));
        }
    }
    return RTMODT_OK;
}

}  // extern "C"
