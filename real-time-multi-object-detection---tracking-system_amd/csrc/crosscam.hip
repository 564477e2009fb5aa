// crosscam.hip -- links the tracks of several cameras to site-wide identities.  A device-resident TABLE of identities (gid from 1,
// never reused; class; the smoothed feature as int16 and int8; first_seen; last_seen per stream) in gid order, and per stream a
// LEDGER of bindings (local track id -> gid, call of the last sighting) in local-id order; both double-buffered and rebuilt by rank
// every call, as speed.hip builds its ledger.  The reference has no counterpart: its Track has no global id and its tracker sees one
// source.  crosscam_rule.h states the per-pair and per-row arithmetic, include/rtmodt.h the per-call rules, tests/crosscam_ref.py
// restates both and the kernels equal it exactly.  PARITY UNPINNED (no published multi-camera tracker is installed where this runs).
//
// One call = one memset and NINE launches for all streams whatever the tracks do, no host hop between them (a device source adds
// one in front, on the tracker's stream):
//   cc_retire    one workgroup: identities past max_age leave, the survivors' small fields move to their rank in the new buffer
//   cc_compact   one wave per surviving row: its int16 / int8 feature moves with it
//   cc_bound     one workgroup per stream: bindings of retired identities or past bind_age are marked dropped; every entry finds its
//                binding by binary search (BOUND), the others with a non-zero row are counted as queries by a workgroup prefix sum
//   cc_gather    one workgroup per stream: queries get their number in (stream, entry) order (those past max_queries: DEFERRED), their
//                row goes into the query matrix, and their birth feature and both squared norms are computed, one wave per query
//   cc_gemm      ONE int8 GEMM on v_mfma_i32_16x16x64_i8, K = dim: all queries x (all table rows | all birth features) -> int32
//   cc_match     one 1024-thread workgroup per stream: the exact maximum of sum(sim - min_sim + 1) over the admissible pairs by
//                assoc_sparse<long long> (track_dev.h over lap.h); matched queries are LINKED.  In front of it, one wave per query:
//                has the query anyone it could JOIN (an earlier query of another stream, its class, a similar birth feature)?
//   cc_births    one wave, serially in query order over what is left: JOIN an identity born earlier in this call (for a query that
//                could, the wave scans them in parallel: best sim, then lowest gid), found one (BORN), or TABLE_FULL
//   cc_update    one wave per identity: the integer EMA once per sighting in ascending stream order, last_seen
//   cc_ledger    one workgroup per stream: the new ledger = surviving bindings (minus the one a LINK displaced) merged by rank with
//                this call's new bindings; the hand-off events in entry order
// No atomic decides an index or an order; there is no atomic here at all.  The outputs of a call lie in one block and come back
// in one copy, or in none when the caller asks for nothing.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "handle_host.h"
#include "track_layout.h"
#include "lap.h"

#define CC_HD __host__ __device__
#include "crosscam_rule.h"

namespace rtmodt {

#include "wg_dev.h"
#include "track_dev.h"
#include "track_select_dev.h"

constexpr int CC_THREADS = 256, CC_WAVES = CC_THREADS / 64;

struct CcTab { int64_t *gid, *first, *last; int32_t *cls, *n8; int16_t *s16; int8_t *s8; };     // one buffer: [I], last [I][S], s16 / s8 [I][D]
struct CcLed { int64_t *lid, *gid, *last; int32_t *n; };                                      // one buffer: [S][I], n [S]

struct CcArgs {
    int S, D, Mc, I, Q, min_sim, max_age, bind_age, match_class;
    long long c;                                // this call's number
    CcTab to, tn;                               // the table as the call found it, and as it leaves it
    CcLed lo, ln;
    int64_t *state;                             // [2]: identities in the table, next gid
    int64_t *call;                              // [8]: kept, queries, deferred, table-full, born, retired
    const int32_t *tmin, *tmax;                 // [S][S], [from][to]
    int32_t *err;                               // [S] sticky
    int64_t *e_id; int32_t *e_cls; int8_t *e_row; int32_t *e_n;          // the entries [S][Mc], rows [S][Mc][D], counts [S]
    int32_t *newpos, *oldrow;                   // [I]: old row -> new row (-1 retired), new row -> old row
    int32_t *lk_row, *lk_seen, *lk_pre;         // [S][I], [S][I], [S][I + 1]: a binding's new table row (-1 dropped), sighted, rank
    int32_t *sq_cnt;                            // [S] queries per stream, before the cap
    int32_t *e_q, *e_trow, *e_nz, *e_from, *e_gap;                        // [S][Mc]
    int32_t *q_entry, *q_match, *q_cand, *b_n8; int64_t *q_n;             // [Q]; q_cand: the query has someone it could JOIN
    int8_t *Qm, *B8; int16_t *B16;              // [Q][D]: query rows, birth features
    int32_t *dots; int ldc;                     // [Q][I + Q]
    int32_t *sight;                             // [I][S]: entry + 1 of the new row's sighting in the stream, 0 none
    int64_t *o_counters, *o_gid; int32_t *o_status, *o_sim, *o_nev; rtmodt_crosscam_event *o_ev; rtmodt_crosscam_retired *o_ret;
    // a device source (cc_stage): the tracker's state, its meta rows, its int8 rows
    TrackSrc trk; const int8_t *t_rows; int t_mc, t_budget;
};

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- a tracker's device-resident state -> the entry list, in the tracker's list order ----
__global__ __launch_bounds__(CC_THREADS) void cc_stage(CcArgs a) {
    __shared__ int wsum[CC_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x, D = a.D;
    const int cur = (int)a.trk.meta[(size_t)s * 8] & 1;
    const TrackSel src = select_tracks(a.trk, s);
    const int n = src.n < 0 ? 0 : (src.n > a.t_mc ? a.t_mc : src.n);
    int cnt = 0;
    for (int base = 0; base < n; base += CC_THREADS) {
        const int i = base + tid;
        const bool f = i < n && selected(src, i);
        int tot;
        const int pos = cnt + block_scan_count<CC_WAVES>(f ? 1 : 0, wsum, tot);
        if (f && pos < a.Mc) {
            const size_t o = (size_t)s * a.Mc + pos;
            a.e_id[o] = src.ids[i]; a.e_cls[o] = src.cls[i];
            const int8_t *row = nullptr;
            if (a.trk.botsort) row = a.t_rows + (((size_t)s * 2 + cur) * a.t_mc + i) * D;
            else {
                const DsState &st = a.trk.deepsort[s];
                const int slot = st.slot[cur][i], gc = st.gcount[cur][i];
                if (gc > 0 && slot >= 0 && slot < a.t_mc) row = a.t_rows + (((size_t)s * a.t_mc + slot) * a.t_budget + (gc - 1) % a.t_budget) * D;
            }
            int4 *dst = (int4 *)(a.e_row + o * D);
            for (int k = 0; k < D / 16; ++k) dst[k] = row ? ((const int4 *)row)[k] : make_int4(0, 0, 0, 0);
        }
        cnt += tot;
    }
    if (tid == 0) a.e_n[s] = cnt < a.Mc ? cnt : a.Mc;
}

// ---- 1. retire ----
__global__ __launch_bounds__(TRK_THREADS) void cc_retire(CcArgs a) {
    __shared__ int wsum[TRK_WAVES + 1];
    const int tid = threadIdx.x, S = a.S;
    int n = (int)a.state[0];
    n = n < 0 ? 0 : (n > a.I ? a.I : n);
    int kept = 0, nret = 0;
    for (int base = 0; base < n; base += TRK_THREADS) {
        const int i = base + tid;
        const bool valid = i < n;
        bool keep = false;
        long long mx = 0;
        unsigned long long mask = 0;
        if (valid) {
            for (int s = 0; s < S; ++s) {
                const long long l = a.to.last[(size_t)i * S + s];
                mx = l > mx ? l : mx;
                if (l > 0) mask |= 1ull << s;
            }
            keep = a.c - mx <= a.max_age;
        }
        int tot, tot2;
        const int pos = block_scan_flag(valid && keep, wsum, tot);
        const int pos2 = block_scan_flag(valid && !keep, wsum, tot2);
        if (valid && keep) {
            const int np = kept + pos;
            a.newpos[i] = np; a.oldrow[np] = i;
            a.tn.gid[np] = a.to.gid[i]; a.tn.cls[np] = a.to.cls[i]; a.tn.first[np] = a.to.first[i]; a.tn.n8[np] = a.to.n8[i];
            for (int s = 0; s < S; ++s) a.tn.last[(size_t)np * S + s] = a.to.last[(size_t)i * S + s];
        } else if (valid) {
            a.newpos[i] = -1;
            rtmodt_crosscam_retired r;
            r.gid = a.to.gid[i]; r.first_seen = a.to.first[i]; r.last_seen = mx; r.stream_mask = mask;
            a.o_ret[nret + pos2] = r;
        }
        kept += tot; nret += tot2;
    }
    if (tid < 8) a.call[tid] = tid == 0 ? kept : (tid == 5 ? nret : 0);
}

__global__ __launch_bounds__(CC_THREADS) void cc_compact(CcArgs a) {
    const int i = blockIdx.x * CC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63, D = a.D;
    int n = (int)a.state[0];
    n = n > a.I ? a.I : n;
    if (i >= n) return;
    const int np = a.newpos[i];
    if (np < 0) return;
    if (lane < D / 8) ((int4 *)(a.tn.s16 + (size_t)np * D))[lane] = ((const int4 *)(a.to.s16 + (size_t)i * D))[lane];
    if (lane < D / 16) ((int4 *)(a.tn.s8 + (size_t)np * D))[lane] = ((const int4 *)(a.to.s8 + (size_t)i * D))[lane];
}

// ---- 2. the bound pass ----
__global__ __launch_bounds__(CC_THREADS) void cc_bound(CcArgs a) {
    __shared__ int wsum[CC_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x, S = a.S, I = a.I, Mc = a.Mc, D = a.D;
    int n_l = a.lo.n[s];
    n_l = n_l < 0 ? 0 : (n_l > I ? I : n_l);
    int n_old = (int)a.state[0];
    n_old = n_old < 0 ? 0 : (n_old > I ? I : n_old);
    const int64_t *lid = a.lo.lid + (size_t)s * I, *lgid = a.lo.gid + (size_t)s * I, *llast = a.lo.last + (size_t)s * I;
    int32_t *lk_row = a.lk_row + (size_t)s * I, *lk_seen = a.lk_seen + (size_t)s * I;
    for (int j = tid; j < n_l; j += CC_THREADS) {
        const int64_t g = lgid[j];
        const int r = lower_bound_i64(a.to.gid, n_old, g);
        int row = r < n_old && a.to.gid[r] == g ? a.newpos[r] : -1;
        if (a.c - llast[j] > a.bind_age) row = -1;
        lk_row[j] = row; lk_seen[j] = 0;
    }
    __syncthreads();
    int n = a.e_n[s];
    n = n < 0 ? 0 : (n > Mc ? Mc : n);
    int nq = 0;
    for (int base = 0; base < Mc; base += CC_THREADS) {
        const int e = base + tid;
        const size_t o = (size_t)s * Mc + e;
        bool isq = false;
        if (e < Mc) {
            a.o_gid[o] = 0; a.o_sim[o] = 0; a.o_status[o] = CC_NONE;
            a.e_q[o] = -1; a.e_trow[o] = -1; a.e_from[o] = -1; a.e_gap[o] = 0; a.e_nz[o] = 0;
        }
        if (e < n) {
            const int64_t id = a.e_id[o];
            const int j = lower_bound_i64(lid, n_l, id);
            const bool hit = j < n_l && lid[j] == id && lk_row[j] >= 0;
            const int4 *row = (const int4 *)(a.e_row + o * D);
            int nz = 0;
            for (int k = 0; k < D / 16; ++k) { const int4 v = row[k]; nz |= v.x | v.y | v.z | v.w; }
            a.e_nz[o] = nz != 0;
            if (hit) {
                const int r = lk_row[j];
                a.o_status[o] = CC_BOUND; a.o_gid[o] = lgid[j]; a.e_trow[o] = r;
                lk_seen[j] = 1;
                a.sight[(size_t)r * S + s] = e + 1;
            } else if (!nz) a.o_status[o] = CC_NO_DESCRIPTOR;
            else isq = true;
        }
        int tot;
        const int pos = nq + block_scan_count<CC_WAVES>(isq ? 1 : 0, wsum, tot);
        if (isq) a.e_q[o] = pos;                           // its rank in the stream; cc_gather adds the streams before
        nq += tot;
    }
    if (tid == 0) a.sq_cnt[s] = nq;
}

// ---- 3a. query numbers, query rows, birth features, norms ----
__global__ __launch_bounds__(CC_THREADS) void cc_gather(CcArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Mc = a.Mc, D = a.D;
    int off = 0, total = 0;
    for (int t = 0; t < a.S; ++t) { const int v = a.sq_cnt[t]; if (t < s) off += v; total += v; }
    if (s == 0 && threadIdx.x == 0) { a.call[1] = total < a.Q ? total : a.Q; a.call[2] = total < a.Q ? 0 : total - a.Q; }
    int n = a.e_n[s];
    n = n < 0 ? 0 : (n > Mc ? Mc : n);
    for (int e = wave; e < n; e += CC_WAVES) {
        const size_t o = (size_t)s * Mc + e;
        const int r = a.e_q[o];
        if (r < 0) continue;                               // (wave-uniform)
        const int q = off + r;
        if (q >= a.Q) {
            if (lane == 0) { a.o_status[o] = CC_DEFERRED; a.e_q[o] = -1; }
            continue;
        }
        const int8_t *row = a.e_row + o * D;
        int32_t v[CC_MAX_DIM / 64];
        long long n2 = 0, nq = 0;
        for (int k = 0; k < D / 64; ++k) {
            const int f = row[lane + 64 * k];
            a.Qm[(size_t)q * D + lane + 64 * k] = (int8_t)f;
            v[k] = cc_feat_mix(true, 0, f);
            n2 += (long long)v[k] * v[k]; nq += f * f;
        }
        n2 = wave_sum_ll(n2); nq = wave_sum_ll(nq);
        const long long rr = cc_isqrt(n2);
        long long nb = 0;
        for (int k = 0; k < D / 64; ++k) {
            const int16_t h = rr ? cc_feat_s16(v[k], rr) : (int16_t)0;
            const int8_t b = rr ? cc_feat_s8(v[k], rr) : (int8_t)0;
            a.B16[(size_t)q * D + lane + 64 * k] = h; a.B8[(size_t)q * D + lane + 64 * k] = b;
            nb += (int)b * (int)b;
        }
        nb = wave_sum_ll(nb);
        if (lane == 0) { a.e_q[o] = q; a.q_entry[q] = (int)o; a.q_match[q] = -1; a.q_n[q] = nq; a.b_n8[q] = (int32_t)nb; }
    }
}

// ---- 3b. the GEMM: dots[q][col] = <Q[q], T[col]> for col < nT, dots[q][I + p] = <Q[q], B[p]> for p < nQ ----
// grid (64-query tile, 64-column tile); the column tiles of the table come first, then those of the birth features.  4 waves; wave w
// owns queries [64 tile + 16 w, + 16) and walks the tile's four 16-column fragments.  Fragment layout as appearance_dotmax: A = 16
// queries x 64 k, B = 64 k x 16 columns, lane l holds the 16 consecutive k of group l >> 4 for row / column l & 15; C: column
// l & 15, rows 4 (l >> 4) + reg.
typedef int cc_intx4 __attribute__((ext_vector_type(4)));
struct CcGemm {
    const int8_t *Qm, *T, *B; const int64_t *nq_dev, *nt_dev; int nq, nt, D, I, ldc; int32_t *dots;
};

__global__ __launch_bounds__(CC_THREADS) void cc_gemm(CcGemm g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nQ = g.nq_dev ? (int)*g.nq_dev : g.nq, nT = g.nt_dev ? (int)*g.nt_dev : g.nt;
    const int t_tiles = (g.I + 63) / 64;
    const bool birth = (int)blockIdx.y >= t_tiles;
    const int cbase = 64 * (birth ? blockIdx.y - t_tiles : blockIdx.y);
    const int ncols = birth ? nQ : (nT > g.I ? g.I : nT);
    const int q0 = blockIdx.x * 64 + wave * 16;
    if (q0 >= nQ || cbase >= ncols) return;                // wave-uniform
    const int8_t *Bp = birth ? g.B : g.T;
    const int ocol0 = birth ? g.I + cbase : cbase;
    const int KC = g.D / 64, kg = 16 * (lane >> 4), qrow = q0 + (lane & 15);
    cc_intx4 af[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        af[k] = cc_intx4{0, 0, 0, 0};
        if (k < KC && qrow < nQ) af[k] = *(const cc_intx4 *)(g.Qm + (size_t)qrow * g.D + 64 * k + kg);
    }
    for (int ct = 0; ct < 4; ++ct) {
        const int c0 = cbase + 16 * ct;
        if (c0 >= ncols) break;
        const int col = c0 + (lane & 15);
        cc_intx4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < KC) {
                cc_intx4 bf = {0, 0, 0, 0};
                if (col < ncols) bf = *(const cc_intx4 *)(Bp + (size_t)col * g.D + 64 * k + kg);
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[k], bf, acc, 0, 0, 0);
            }
        }
        const int rbase = q0 + 4 * (lane >> 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rbase + j < nQ && col < ncols) g.dots[(size_t)(rbase + j) * g.ldc + ocol0 + 16 * ct + (lane & 15)] = acc[j];
    }
}

// sim of a dots matrix [nq][nt] (the stand-alone entry)
__global__ void cc_sim_kernel(const int32_t *dots, const int64_t *nq2, const int64_t *nt2, int nq, int nt, int32_t *sim) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nq * nt) return;
    sim[i] = cc_sim(dots[i], nq2[i / nt], nt2[i % nt]);
}

// ---- 4. the matching of one stream ----
static size_t cc_match_smem(int I) { return (size_t)LAP_ROWS * (4 * 3 + 8) + (size_t)I * 4 + (TRK_WAVES + 1) * 4 + 64 * 8 + 64 + lap_smem_bytes(I); }

__global__ __launch_bounds__(TRK_THREADS) void cc_match(CcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = blockIdx.x, tid = threadIdx.x, S = a.S, Mc = a.Mc;
    long long *r_nq = (long long *)smem;                   // [LAP_ROWS]
    int *r_cls = (int *)(r_nq + LAP_ROWS);                 // [LAP_ROWS]
    int *row_best = r_cls + LAP_ROWS, *rowcand = row_best + LAP_ROWS;
    int *t_lo = rowcand + LAP_ROWS, *t_hi = t_lo + 64;     // the transit windows into this stream
    int *col_winner = t_hi + 64;                           // [I]
    int *wsum = col_winner + a.I;
    unsigned char *lap_base = (unsigned char *)(((uintptr_t)(wsum + TRK_WAVES + 1) + 7) & ~(uintptr_t)7);
    const LapSmemT<long long> L = lap_carve_t<long long>(lap_base, a.I);
    __shared__ int lap_err;
    int off = 0;
    for (int t = 0; t < s; ++t) off += a.sq_cnt[t];
    int nr = (off + a.sq_cnt[s] < a.Q ? off + a.sq_cnt[s] : a.Q) - off;
    nr = nr < 0 ? 0 : (nr > LAP_ROWS ? LAP_ROWS : nr);     // (max_tracks <= 256 = LAP_ROWS)
    const int nT = (int)a.call[0];
    // Which of this stream's queries could JOIN at all: one with an earlier query of another stream (the queries before `off`) of its
    // class whose birth feature is similar enough.  cc_births scans the identities born in this call for these queries alone.
    for (int r = (tid >> 6); r < nr; r += TRK_WAVES) {
        const int q = off + r, lane = tid & 63, k = a.e_cls[a.q_entry[q]];
        const long long nq = a.q_n[q];
        bool any = false;
        for (int p = lane; p < off && !any; p += 64)
            any = a.e_cls[a.q_entry[p]] == k && cc_sim(a.dots[(size_t)q * a.ldc + a.I + p], nq, a.b_n8[p]) >= a.min_sim;
        const unsigned long long m = __ballot(any);
        if (lane == 0) a.q_cand[q] = m != 0;
    }
    if (nr == 0 || nT == 0) return;                        // (workgroup-uniform) every query goes on to the births
    if (tid == 0) lap_err = 0;
    if (tid < S) { t_lo[tid] = a.tmin[tid * S + s]; t_hi[tid] = a.tmax[tid * S + s]; }
    for (int r = tid; r < nr; r += TRK_THREADS) { r_nq[r] = a.q_n[off + r]; r_cls[r] = a.e_cls[a.q_entry[off + r]]; }
    __syncthreads();
    auto sim_of = [&](int r, int c) { return cc_sim(a.dots[(size_t)(off + r) * a.ldc + c], r_nq[r], a.tn.n8[c]); };
    auto edge = [&](int r, int c, long long &cost) -> bool {
        if (a.dots[(size_t)(off + r) * a.ldc + c] <= 0) return false;
        if (a.match_class && a.tn.cls[c] != r_cls[r]) return false;
        if (a.sight[(size_t)c * S + s] != 0) return false;                // live in this stream
        const int sim = sim_of(r, c);
        if (sim < a.min_sim) return false;
        const int64_t *last = a.to.last + (size_t)a.oldrow[c] * S;         // start-of-call values
        bool ok = false;
        for (int f = 0; f < S && !ok; ++f) ok = cc_transit_ok(a.c, last[f], t_lo[f], t_hi[f]);
        if (!ok) return false;
        cost = -(long long)(sim - a.min_sim + 1);
        return true;
    };
    assoc_sparse<long long>(edge, nr, nT, row_best, col_winner, rowcand, L, wsum, &lap_err);
    if (lap_err) {                                         // past the contested limits: the stream's queries stay unbound this call
        if (tid == 0) a.err[s] = 2;
        for (int r = tid; r < nr; r += TRK_THREADS) { a.q_match[off + r] = -2; a.o_status[a.q_entry[off + r]] = CC_UNBOUND; }
        return;
    }
    for (int r = tid; r < nr; r += TRK_THREADS) {
        const int c = row_best[r];
        if (!(c >= 0 && col_winner[c] == r)) continue;
        const int o = a.q_entry[off + r], e = o - s * Mc;
        const int64_t *last = a.to.last + (size_t)a.oldrow[c] * S;
        int from = 0;
        for (int f = 1; f < S; ++f) from = last[f] > last[from] ? f : from;
        a.q_match[off + r] = c;
        a.o_status[o] = CC_LINKED; a.o_gid[o] = a.tn.gid[c]; a.o_sim[o] = sim_of(r, c);
        a.e_trow[o] = c; a.e_from[o] = from; a.e_gap[o] = (int32_t)(a.c - last[from]);
        a.sight[(size_t)c * S + s] = e + 1;
    }
}

// ---- 5. births: one wave, serially in query order ----
__global__ __launch_bounds__(64) void cc_births(CcArgs a) {
    __shared__ int b_q[CC_MAX_QUERIES], b_cls[CC_MAX_QUERIES], b_fs[CC_MAX_QUERIES];
    __shared__ unsigned long long b_live[CC_MAX_QUERIES], okmask[64];
    const int lane = threadIdx.x, S = a.S, Mc = a.Mc;
    const int nQ = (int)a.call[1], nK = (int)a.call[0];
    const long long next = a.state[1];
    if (lane < S) {                                        // the streams an identity may be live in to be joined from this one
        unsigned long long m = 0;
        for (int f = 0; f < S; ++f)
            if (a.tmin[f * S + lane] == 0 && a.tmax[f * S + lane] >= 0) m |= 1ull << f;
        okmask[lane] = m;
    }
    __syncthreads();
    int nb = 0, nfull = 0;
    for (int q = 0; q < nQ; ++q) {
        if (a.q_match[q] != -1) continue;                  // (uniform)
        const int o = a.q_entry[q], s = o / Mc, e = o - s * Mc, k = a.e_cls[o];
        const long long nq = a.q_n[q];
        int key = -1;
        for (int p = lane; p < (a.q_cand[q] ? nb : 0); p += 64) {
            if (b_cls[p] != k || (b_live[p] >> s & 1) || !(b_live[p] & okmask[s])) continue;
            const int fq = b_q[p];
            const int sim = cc_sim(a.dots[(size_t)q * a.ldc + a.I + fq], nq, a.b_n8[fq]);
            if (sim >= a.min_sim) key = max(key, (sim << 10) | (CC_MAX_QUERIES - 1 - p));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = max(key, __shfl_xor(key, d));
        if (key >= 0) {
            const int p = CC_MAX_QUERIES - 1 - (key & (CC_MAX_QUERIES - 1));
            if (lane == 0) {
                b_live[p] |= 1ull << s;
                a.o_status[o] = CC_JOINED; a.o_gid[o] = next + p; a.o_sim[o] = key >> 10;
                a.e_trow[o] = nK + p; a.e_from[o] = b_fs[p]; a.e_gap[o] = 0;
                a.sight[(size_t)(nK + p) * S + s] = e + 1;
            }
        } else if (nK + nb < a.I) {
            if (lane == 0) {
                b_q[nb] = q; b_cls[nb] = k; b_fs[nb] = s; b_live[nb] = 1ull << s;
                a.o_status[o] = CC_BORN; a.o_gid[o] = next + nb;
                a.e_trow[o] = nK + nb;
                a.sight[(size_t)(nK + nb) * S + s] = e + 1;
            }
            ++nb;
        } else {
            if (lane == 0) a.o_status[o] = CC_TABLE_FULL;
            ++nfull;
        }
        __syncthreads();
    }
    for (int p = lane; p < nb; p += 64) {
        const int r = nK + p;
        a.tn.gid[r] = next + p; a.tn.cls[r] = b_cls[p]; a.tn.first[r] = a.c; a.tn.n8[r] = 0;
        for (int s = 0; s < S; ++s) a.tn.last[(size_t)r * S + s] = 0;
    }
    if (lane == 0) { a.state[0] = nK + nb; a.state[1] = next + nb; a.call[3] = nfull; a.call[4] = nb; }
}

// ---- 6. the feature update: one wave per identity ----
__global__ __launch_bounds__(CC_THREADS) void cc_update(CcArgs a) {
    const int r = blockIdx.x * CC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63, S = a.S, D = a.D, KC = a.D / 64;
    int n = (int)a.state[0];
    n = n > a.I ? a.I : n;
    if (r >= n) return;
    bool started = r < (int)a.call[0], any = false;
    int32_t h[CC_MAX_DIM / 64], b[CC_MAX_DIM / 64];
    for (int k = 0; k < KC; ++k) { h[k] = started ? a.tn.s16[(size_t)r * D + lane + 64 * k] : 0; b[k] = 0; }
    for (int s = 0; s < S; ++s) {
        const int e1 = a.sight[(size_t)r * S + s];
        if (!e1) continue;                                 // (wave-uniform)
        const size_t o = (size_t)s * a.Mc + e1 - 1;
        if (lane == 0) a.tn.last[(size_t)r * S + s] = a.c;
        if (!a.e_nz[o]) continue;
        const int8_t *f = a.e_row + o * D;
        int32_t v[CC_MAX_DIM / 64];
        long long n2 = 0;
        for (int k = 0; k < KC; ++k) {
            v[k] = cc_feat_mix(!started, h[k], f[lane + 64 * k]);
            n2 += (long long)v[k] * v[k];
        }
        const long long rr = cc_isqrt(wave_sum_ll(n2));
        for (int k = 0; k < KC; ++k) { h[k] = rr ? cc_feat_s16(v[k], rr) : 0; b[k] = rr ? cc_feat_s8(v[k], rr) : 0; }
        started = true; any = true;
    }
    if (!any) return;
    long long nb = 0;
    for (int k = 0; k < KC; ++k) {
        a.tn.s16[(size_t)r * D + lane + 64 * k] = (int16_t)h[k]; a.tn.s8[(size_t)r * D + lane + 64 * k] = (int8_t)b[k];
        nb += b[k] * b[k];
    }
    nb = wave_sum_ll(nb);
    if (lane == 0) a.tn.n8[r] = (int32_t)nb;
}

// ---- 7. the new ledger of one stream, and its events ----
static size_t cc_ledger_smem(int Mc) { return (size_t)Mc * (8 + 4 + 4) + CC_WAVES * 4 + 16; }

__global__ __launch_bounds__(CC_THREADS) void cc_ledger(CcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int s = blockIdx.x, tid = threadIdx.x, S = a.S, I = a.I, Mc = a.Mc;
    int64_t *s_lid = (int64_t *)smem;                      // [Mc] the new bindings' local ids, ascending
    int *s_ent = (int *)(s_lid + Mc), *cand = s_ent + Mc;  // [Mc] their entries; [Mc] the same, in entry order
    int *wsum = cand + Mc;
    int n_l = a.lo.n[s];
    n_l = n_l < 0 ? 0 : (n_l > I ? I : n_l);
    const int64_t *lid = a.lo.lid + (size_t)s * I, *lgid = a.lo.gid + (size_t)s * I, *llast = a.lo.last + (size_t)s * I;
    const int32_t *lk_row = a.lk_row + (size_t)s * I, *lk_seen = a.lk_seen + (size_t)s * I;
    int32_t *lk_pre = a.lk_pre + (size_t)s * (I + 1);
    int64_t *n_lid = a.ln.lid + (size_t)s * I, *n_gid = a.ln.gid + (size_t)s * I, *n_last = a.ln.last + (size_t)s * I;
    // surviving bindings: kept by cc_bound, and not displaced by a LINK of their identity in this stream
    int run = 0;
    for (int base = 0; base < n_l; base += CC_THREADS) {
        const int j = base + tid;
        const int f = j < n_l && lk_row[j] >= 0 && (lk_seen[j] || a.sight[(size_t)lk_row[j] * S + s] == 0) ? 1 : 0;
        int tot;
        const int pos = run + block_scan_count<CC_WAVES>(f, wsum, tot);
        if (j < n_l) lk_pre[j] = f ? pos : -pos - 1;       // kept: rank; dropped: -(rank of the next kept) - 1
        run += tot;
    }
    if (tid == 0) lk_pre[n_l] = -run - 1;
    int n = a.e_n[s];
    n = n < 0 ? 0 : (n > Mc ? Mc : n);
    int nn = 0, nev = 0;
    for (int base = 0; base < n; base += CC_THREADS) {
        const int e = base + tid;
        const size_t o = (size_t)s * Mc + e;
        const int st = e < n ? a.o_status[o] : CC_NONE;
        const int f = st == CC_LINKED || st == CC_JOINED || st == CC_BORN ? 1 : 0, fe = st == CC_LINKED || st == CC_JOINED ? 1 : 0;
        int tot, tot2;
        const int pos = nn + block_scan_count<CC_WAVES>(f, wsum, tot);
        const int pe = nev + block_scan_count<CC_WAVES>(fe, wsum, tot2);
        if (f) cand[pos] = e;
        if (fe) {
            rtmodt_crosscam_event ev;
            ev.gid = a.o_gid[o]; ev.local_id = a.e_id[o]; ev.stream = s; ev.from_stream = a.e_from[o]; ev.gap = a.e_gap[o]; ev.sim = a.o_sim[o];
            a.o_ev[(size_t)s * Mc + pe] = ev;
        }
        nn += tot; nev += tot2;
    }
    __syncthreads();
    for (int t = tid; t < nn; t += CC_THREADS) {           // rank by counting: nn <= 256
        const int64_t x = a.e_id[(size_t)s * Mc + cand[t]];
        int rank = 0;
        for (int u = 0; u < nn; ++u) rank += a.e_id[(size_t)s * Mc + cand[u]] < x ? 1 : 0;
        s_lid[rank] = x; s_ent[rank] = cand[t];
    }
    __syncthreads();
    for (int j = tid; j < n_l; j += CC_THREADS) {
        const int v = lk_pre[j];
        if (v < 0) continue;
        const int np = v + lower_bound_i64(s_lid, nn, lid[j]);
        if (np < I) { n_lid[np] = lid[j]; n_gid[np] = lgid[j]; n_last[np] = lk_seen[j] ? a.c : llast[j]; }
    }
    for (int t = tid; t < nn; t += CC_THREADS) {
        const int pv = lk_pre[lower_bound_i64(lid, n_l, s_lid[t])];
        const int np = (pv >= 0 ? pv : -pv - 1) + t;
        if (np < I) { n_lid[np] = s_lid[t]; n_gid[np] = a.o_gid[(size_t)s * Mc + s_ent[t]]; n_last[np] = a.c; }
    }
    if (tid == 0) {
        a.ln.n[s] = run + nn < I ? run + nn : I;
        a.o_nev[s] = nev;
        if (s == 0) {
            a.o_counters[0] = a.c; a.o_counters[1] = a.state[0]; a.o_counters[2] = a.state[1]; a.o_counters[3] = a.call[1];
            a.o_counters[4] = a.call[2]; a.o_counters[5] = a.call[3]; a.o_counters[6] = 0; a.o_counters[7] = a.call[5];
        }
    }
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_crosscam : HandleBase {
    rtmodt_crosscam_cfg cfg{};
    int cur = 0;
    long long calls = 0;
    hipStream_t last_stream = nullptr;            // the stream of the most recent call (a tracker's, or the own one)
    EventTimer<2> timer;
    char *pool = nullptr;
    CcArgs a{};                                   // every device pointer; to / tn and lo / ln are set per call from tab / led
    CcTab tab[2]; CcLed led[2];
    int32_t *d_tmin = nullptr, *d_tmax = nullptr;
    char *o_block = nullptr; size_t o_bytes = 0, off_gid = 0, off_status = 0, off_sim = 0, off_nev = 0, off_ev = 0, off_ret = 0;
    char *h_pin = nullptr;
    std::vector<int32_t> tmin, tmax;
};

namespace {

size_t cc_carve(rtmodt_crosscam *z, char *base) {
    Carver c{base};
    const size_t S = z->cfg.n_streams, D = z->cfg.dim, Mc = z->cfg.max_tracks, I = z->cfg.max_identities, Q = z->cfg.max_queries;
    CcArgs &a = z->a;
    for (int b = 0; b < 2; ++b) {
        CcTab &t = z->tab[b];
        t.gid = c.take<int64_t>(I); t.first = c.take<int64_t>(I); t.last = c.take<int64_t>(I * S); t.cls = c.take<int32_t>(I); t.n8 = c.take<int32_t>(I);
        t.s16 = c.take<int16_t>(I * D); t.s8 = c.take<int8_t>(I * D);
        CcLed &l = z->led[b];
        l.lid = c.take<int64_t>(S * I); l.gid = c.take<int64_t>(S * I); l.last = c.take<int64_t>(S * I); l.n = c.take<int32_t>(S);
    }
    a.state = c.take<int64_t>(2); a.call = c.take<int64_t>(8);
    z->d_tmin = c.take<int32_t>(S * S); z->d_tmax = c.take<int32_t>(S * S);
    a.err = c.take<int32_t>(S);
    a.e_id = c.take<int64_t>(S * Mc); a.e_cls = c.take<int32_t>(S * Mc); a.e_row = c.take<int8_t>(S * Mc * D); a.e_n = c.take<int32_t>(S);
    a.newpos = c.take<int32_t>(I); a.oldrow = c.take<int32_t>(I);
    a.lk_row = c.take<int32_t>(S * I); a.lk_seen = c.take<int32_t>(S * I); a.lk_pre = c.take<int32_t>(S * (I + 1));
    a.sq_cnt = c.take<int32_t>(S);
    a.e_q = c.take<int32_t>(S * Mc); a.e_trow = c.take<int32_t>(S * Mc); a.e_nz = c.take<int32_t>(S * Mc); a.e_from = c.take<int32_t>(S * Mc);
    a.e_gap = c.take<int32_t>(S * Mc);
    a.q_entry = c.take<int32_t>(Q); a.q_match = c.take<int32_t>(Q); a.q_cand = c.take<int32_t>(Q); a.b_n8 = c.take<int32_t>(Q); a.q_n = c.take<int64_t>(Q);
    a.Qm = c.take<int8_t>(Q * D); a.B8 = c.take<int8_t>(Q * D); a.B16 = c.take<int16_t>(Q * D);
    a.dots = c.take<int32_t>(Q * (I + Q)); a.ldc = (int)(I + Q);
    a.sight = c.take<int32_t>(I * S);
    // the output block: counters | gid | status | sim | n_events | events | retired
    z->off_gid = 64;
    z->off_status = align_up(z->off_gid + S * Mc * 8, 16);
    z->off_sim = align_up(z->off_status + S * Mc * 4, 16);
    z->off_nev = align_up(z->off_sim + S * Mc * 4, 16);
    z->off_ev = align_up(z->off_nev + S * 4, 16);
    z->off_ret = align_up(z->off_ev + S * Mc * sizeof(rtmodt_crosscam_event), 16);
    z->o_bytes = align_up(z->off_ret + I * sizeof(rtmodt_crosscam_retired), 16);
    z->o_block = c.take<char>(z->o_bytes);
    a.o_counters = (int64_t *)z->o_block; a.o_gid = (int64_t *)(z->o_block + z->off_gid); a.o_status = (int32_t *)(z->o_block + z->off_status);
    a.o_sim = (int32_t *)(z->o_block + z->off_sim); a.o_nev = (int32_t *)(z->o_block + z->off_nev);
    a.o_ev = (rtmodt_crosscam_event *)(z->o_block + z->off_ev); a.o_ret = (rtmodt_crosscam_retired *)(z->o_block + z->off_ret);
    return c.size();
}

int cc_sync(rtmodt_crosscam *z) {
    RT_HIP(hipSetDevice(z->device));
    RT_HIP(hipStreamSynchronize(z->stream));
    if (z->last_stream && z->last_stream != z->stream) RT_HIP(hipStreamSynchronize(z->last_stream));
    return RTMODT_OK;
}

// the launches of one call on q (the entries are staged, or `stage` fills them from a tracker), then the one copy
int cc_run(rtmodt_crosscam *z, hipStream_t q, bool stage, const rtmodt_crosscam_out *out) {
    const rtmodt_crosscam_cfg &c = z->cfg;
    if (z->last_stream && z->last_stream != q) RT_HIP(hipStreamSynchronize(z->last_stream));   // the table is read where the last call left it
    CcArgs &a = z->a;
    a.c = z->calls + 1;
    a.to = z->tab[z->cur]; a.tn = z->tab[z->cur ^ 1]; a.lo = z->led[z->cur]; a.ln = z->led[z->cur ^ 1];
    const int S = c.n_streams, I = c.max_identities, Q = c.max_queries;
    const size_t sm_match = cc_match_smem(I), sm_led = cc_ledger_smem(c.max_tracks);
    static DynLdsSeen seen_m, seen_l;
    RT_TRY(raise_dynamic_lds((const void *)cc_match, sm_match, seen_m));
    RT_TRY(raise_dynamic_lds((const void *)cc_ledger, sm_led, seen_l));
    RT_TRY(z->timer.record(0, q));
    RT_HIP(hipMemsetAsync(a.sight, 0, (size_t)I * S * 4, q));
    if (stage) hipLaunchKernelGGL(cc_stage, dim3(S), dim3(CC_THREADS), 0, q, a);
    hipLaunchKernelGGL(cc_retire, dim3(1), dim3(TRK_THREADS), 0, q, a);
    hipLaunchKernelGGL(cc_compact, dim3(cdiv(I, CC_WAVES)), dim3(CC_THREADS), 0, q, a);
    hipLaunchKernelGGL(cc_bound, dim3(S), dim3(CC_THREADS), 0, q, a);
    hipLaunchKernelGGL(cc_gather, dim3(S), dim3(CC_THREADS), 0, q, a);
    CcGemm g{a.Qm, a.tn.s8, a.B8, a.call + 1, a.call, 0, 0, c.dim, I, a.ldc, a.dots};
    hipLaunchKernelGGL(cc_gemm, dim3(cdiv(Q, 64), cdiv(I, 64) + cdiv(Q, 64)), dim3(CC_THREADS), 0, q, g);
    hipLaunchKernelGGL(cc_match, dim3(S), dim3(TRK_THREADS), sm_match, q, a);
    hipLaunchKernelGGL(cc_births, dim3(1), dim3(64), 0, q, a);
    hipLaunchKernelGGL(cc_update, dim3(cdiv(I, CC_WAVES)), dim3(CC_THREADS), 0, q, a);
    hipLaunchKernelGGL(cc_ledger, dim3(S), dim3(CC_THREADS), sm_led, q, a);
    RT_HIP(hipGetLastError());
    RT_TRY(z->timer.record(1, q));
    z->timer.timed = true;
    z->last_stream = q;
    z->calls += 1;
    z->cur ^= 1;
    const bool any = out && (out->gid || out->status || out->sim || out->events || out->n_events || out->retired || out->n_retired || out->counters);
    if (!any) return RTMODT_OK;
    RT_HIP(hipMemcpyAsync(z->h_pin, z->o_block, z->o_bytes, hipMemcpyDeviceToHost, q));
    RT_HIP(hipStreamSynchronize(q));
    const size_t SM = (size_t)S * c.max_tracks;
    int64_t counters[8];
    memcpy(counters, z->h_pin, sizeof(counters));
    const int32_t *nev = (const int32_t *)(z->h_pin + z->off_nev);
    int total = 0;
    for (int s = 0; s < S; ++s) {                          // the streams' events, concatenated: (stream, entry) order
        const int k = std::min(std::max(nev[s], 0), c.max_tracks);
        if (out->events && k) memcpy(out->events + total, z->h_pin + z->off_ev + (size_t)s * c.max_tracks * sizeof(rtmodt_crosscam_event), k * sizeof(rtmodt_crosscam_event));
        total += k;
    }
    counters[6] = total;
    const int nret = (int)std::min<int64_t>(std::max<int64_t>(counters[7], 0), I);
    if (out->gid) memcpy(out->gid, z->h_pin + z->off_gid, SM * 8);
    if (out->status) memcpy(out->status, z->h_pin + z->off_status, SM * 4);
    if (out->sim) memcpy(out->sim, z->h_pin + z->off_sim, SM * 4);
    if (out->n_events) *out->n_events = total;
    if (out->retired && nret) memcpy(out->retired, z->h_pin + z->off_ret, nret * sizeof(rtmodt_crosscam_retired));
    if (out->n_retired) *out->n_retired = nret;
    if (out->counters) memcpy(out->counters, counters, sizeof(counters));
    return RTMODT_OK;
}

int cc_check_cfg(const rtmodt_crosscam_cfg &c) {
    RT_CHECK(c.n_streams >= 1 && c.n_streams <= CC_MAX_STREAMS, RTMODT_E_INVALID, "crosscam: n_streams %d (1..%d)", c.n_streams, CC_MAX_STREAMS);
    RT_CHECK(c.dim >= 64 && c.dim <= CC_MAX_DIM && c.dim % 64 == 0, RTMODT_E_INVALID, "crosscam: dim %d: 64..%d in multiples of 64", c.dim, CC_MAX_DIM);
    RT_CHECK(c.max_tracks >= 1 && c.max_tracks <= CC_MAX_TRACKS, RTMODT_E_INVALID, "crosscam: max_tracks %d (1..%d)", c.max_tracks, CC_MAX_TRACKS);
    RT_CHECK(c.max_identities >= 1 && c.max_identities <= CC_MAX_IDENTITIES, RTMODT_E_INVALID, "crosscam: max_identities %d (1..%d)", c.max_identities,
             CC_MAX_IDENTITIES);
    RT_CHECK(c.max_queries >= 1 && c.max_queries <= CC_MAX_QUERIES, RTMODT_E_INVALID, "crosscam: max_queries %d (1..%d)", c.max_queries, CC_MAX_QUERIES);
    RT_CHECK(c.min_sim_milli >= 1 && c.min_sim_milli <= 1000, RTMODT_E_INVALID, "crosscam: min_sim_milli %d (1..1000)", c.min_sim_milli);
    RT_CHECK(c.max_age >= 1 && c.max_age <= (1 << 30) && c.bind_age >= 0 && c.bind_age <= (1 << 30), RTMODT_E_INVALID, "crosscam: max_age %d / bind_age %d",
             c.max_age, c.bind_age);
    return RTMODT_OK;
}

}  // namespace

// the table for the appearance index (kernels.h)
int rtmodt::crosscam_table_view(rtmodt_crosscam *z, CcTableView *out) {
    RT_CHECK(z && out, RTMODT_E_INVALID, "bad argument");
    const CcTab &t = z->tab[z->cur];
    *out = CcTableView{z->a.state, t.gid, t.first, t.last, t.cls, t.s8, z->cfg.n_streams, z->cfg.dim, z->cfg.max_identities, z->device, z->calls,
                       z->last_stream ? z->last_stream : z->stream};
    return RTMODT_OK;
}

extern "C" {

void rtmodt_crosscam_default_cfg(rtmodt_crosscam_cfg *c) {
    if (!c) return;
    *c = rtmodt_crosscam_cfg{};
    c->n_streams = 1; c->dim = 512; c->max_tracks = 256; c->max_identities = 4096; c->max_queries = 1024;
    c->min_sim_milli = 700; c->max_age = 9000; c->bind_age = 0; c->match_class = 1;
}

void rtmodt_crosscam_destroy(rtmodt_crosscam *z) {
    if (!z) return;
    handle_close(z, [&] {
        z->timer.destroy();
        hipFree(z->pool);
        hipHostFree(z->h_pin);
    }, z->last_stream);
    delete z;
}

int rtmodt_crosscam_create(const rtmodt_crosscam_cfg *cfg, rtmodt_crosscam **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    rtmodt_crosscam_cfg c = *cfg;
    if (c.bind_age == 0) c.bind_age = c.max_age;           // the default
    RT_TRY(cc_check_cfg(c));
    rtmodt_crosscam *z = new rtmodt_crosscam();
    z->cfg = c; z->device = c.device;
    const int S = c.n_streams;
    z->tmin.assign((size_t)S * S, 0); z->tmax.assign((size_t)S * S, c.max_age);
    const int64_t st[2] = {0, 1};
    auto body = [&]() -> int {
        RT_CHECK(cc_match_smem(c.max_identities) <= 150 * 1024, RTMODT_E_INVALID, "crosscam: max_identities %d needs %zu B of LDS", c.max_identities,
                 cc_match_smem(c.max_identities));
        RT_TRY(handle_open(z));
        RT_TRY(z->timer.create());
        const size_t total = cc_carve(z, nullptr);
        RT_HIP(hipMalloc((void **)&z->pool, total));
        RT_HIP(handle_zero(z->pool, total, z->stream));
        cc_carve(z, z->pool);
        RT_HIP(hipHostMalloc((void **)&z->h_pin, z->o_bytes, hipHostMallocDefault));
        RT_HIP(hipMemcpyAsync(z->a.state, st, sizeof(st), hipMemcpyHostToDevice, z->stream));              // (these three behind the zeroing of the pool)
        RT_HIP(hipMemcpyAsync(z->d_tmin, z->tmin.data(), z->tmin.size() * 4, hipMemcpyHostToDevice, z->stream));
        RT_HIP(hipMemcpyAsync(z->d_tmax, z->tmax.data(), z->tmax.size() * 4, hipMemcpyHostToDevice, z->stream));
        CcArgs &a = z->a;
        a.S = S; a.D = c.dim; a.Mc = c.max_tracks; a.I = c.max_identities; a.Q = c.max_queries; a.min_sim = c.min_sim_milli; a.max_age = c.max_age;
        a.bind_age = c.bind_age; a.match_class = c.match_class != 0; a.tmin = z->d_tmin; a.tmax = z->d_tmax;
        return RTMODT_OK;
    };
    return handle_created(body(), z, rtmodt_crosscam_destroy, out);
}

int rtmodt_crosscam_set_transit(rtmodt_crosscam *z, int src, int dst, int min_calls, int max_calls) {
    RT_CHECK(z && src >= 0 && src < z->cfg.n_streams && dst >= 0 && dst < z->cfg.n_streams, RTMODT_E_INVALID, "crosscam: transit %d -> %d of %d streams", src, dst,
             z ? z->cfg.n_streams : 0);
    RT_CHECK(min_calls >= 0 && std::abs((long long)max_calls) <= (1 << 30) && min_calls <= (1 << 30), RTMODT_E_INVALID, "crosscam: transit window %d..%d", min_calls,
             max_calls);
    RT_TRY(cc_sync(z));
    const size_t o = (size_t)src * z->cfg.n_streams + dst;
    z->tmin[o] = min_calls; z->tmax[o] = max_calls;
    RT_HIP(hipMemcpy(z->d_tmin + o, &z->tmin[o], 4, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(z->d_tmax + o, &z->tmax[o], 4, hipMemcpyHostToDevice));
    return RTMODT_OK;
}

int rtmodt_crosscam_process(rtmodt_crosscam *z, const int64_t *track_ids, const int32_t *cls, const int8_t *rows, const int32_t *n, int stride,
                            const rtmodt_crosscam_out *out) {
    RT_CHECK(z && n && stride >= 0, RTMODT_E_INVALID, "bad argument");
    const int S = z->cfg.n_streams, Mc = z->cfg.max_tracks, D = z->cfg.dim;
    bool any = false;
    for (int s = 0; s < S; ++s) {
        RT_CHECK(n[s] >= 0 && n[s] <= stride, RTMODT_E_INVALID, "crosscam stream %d: %d entries in rows of %d", s, n[s], stride);
        RT_CHECK(n[s] <= Mc, RTMODT_E_INVALID, "crosscam stream %d: %d entries > max_tracks %d", s, n[s], Mc);
        any |= n[s] > 0;
    }
    RT_CHECK(!any || (track_ids && cls && rows), RTMODT_E_INVALID, "null entries");
    std::vector<int64_t> ids((size_t)S * Mc, 0), tmp;
    std::vector<int32_t> kc((size_t)S * Mc, 0);
    std::vector<int8_t> rw((size_t)S * Mc * D, 0);
    for (int s = 0; s < S; ++s) {
        tmp.assign(track_ids + (size_t)s * stride * (n[s] ? 1 : 0), track_ids + (size_t)s * stride * (n[s] ? 1 : 0) + n[s]);
        std::sort(tmp.begin(), tmp.end());
        for (int i = 1; i < n[s]; ++i) RT_CHECK(tmp[i] != tmp[i - 1], RTMODT_E_INVALID, "crosscam stream %d: track id %lld appears twice", s, (long long)tmp[i]);
        if (!n[s]) continue;
        memcpy(ids.data() + (size_t)s * Mc, track_ids + (size_t)s * stride, (size_t)n[s] * 8);
        memcpy(kc.data() + (size_t)s * Mc, cls + (size_t)s * stride, (size_t)n[s] * 4);
        memcpy(rw.data() + (size_t)s * Mc * D, rows + (size_t)s * stride * D, (size_t)n[s] * D);
    }
    RT_HIP(hipSetDevice(z->device));
    CcArgs &a = z->a;
    if (z->last_stream && z->last_stream != z->stream) RT_HIP(hipStreamSynchronize(z->last_stream));   // a call on a tracker's stream still reads the entries
    RT_HIP(hipMemcpyAsync(a.e_id, ids.data(), ids.size() * 8, hipMemcpyHostToDevice, z->stream));
    RT_HIP(hipMemcpyAsync(a.e_cls, kc.data(), kc.size() * 4, hipMemcpyHostToDevice, z->stream));
    RT_HIP(hipMemcpyAsync(a.e_row, rw.data(), rw.size(), hipMemcpyHostToDevice, z->stream));
    RT_HIP(hipMemcpyAsync(a.e_n, n, (size_t)S * 4, hipMemcpyHostToDevice, z->stream));
    RT_HIP(hipStreamSynchronize(z->stream));               // the vectors above are pageable and about to go away
    a.trk = TrackSrc{};
    return cc_run(z, z->stream, false, out);
}

int rtmodt_crosscam_process_botsort(rtmodt_crosscam *z, rtmodt_botsort *bot, const rtmodt_crosscam_out *out) {
    RT_CHECK(z && bot, RTMODT_E_INVALID, "bad argument");
    TrackSrc src;
    TrackViewBase v;
    RT_TRY(track_src(bot, 0, &src, &v));
    const int8_t *rows = nullptr; int dim = 0;
    RT_TRY(botsort_feature_view(bot, &rows, &dim));
    RT_CHECK(v.device == z->device, RTMODT_E_INVALID, "crosscam on device %d, tracker on device %d", z->device, v.device);
    RT_CHECK(v.n_streams == z->cfg.n_streams && dim == z->cfg.dim && rows, RTMODT_E_INVALID, "crosscam (%d streams, dim %d) given a BoT-SORT tracker of %d streams, dim %d",
             z->cfg.n_streams, z->cfg.dim, v.n_streams, dim);
    RT_CHECK(v.max_tracks <= z->cfg.max_tracks, RTMODT_E_INVALID, "tracker max_tracks %d > crosscam max_tracks %d", v.max_tracks, z->cfg.max_tracks);
    RT_HIP(hipSetDevice(z->device));
    CcArgs &a = z->a;
    a.trk = src; a.t_rows = rows; a.t_mc = v.max_tracks; a.t_budget = 1;
    return cc_run(z, v.stream, true, out);                 // the stream the tracker's last update ran on: ordered after it
}

int rtmodt_crosscam_process_deepsort(rtmodt_crosscam *z, rtmodt_deepsort *ds, const rtmodt_crosscam_out *out) {
    RT_CHECK(z && ds, RTMODT_E_INVALID, "bad argument");
    TrackSrc src;
    TrackViewBase v;
    RT_TRY(track_src(ds, 0, &src, &v));
    const int8_t *rows = nullptr; int dim = 0, budget = 0;
    RT_TRY(deepsort_gallery_view(ds, &rows, &dim, &budget));
    RT_CHECK(v.device == z->device, RTMODT_E_INVALID, "crosscam on device %d, tracker on device %d", z->device, v.device);
    RT_CHECK(v.n_streams == z->cfg.n_streams && dim == z->cfg.dim && rows, RTMODT_E_INVALID, "crosscam (%d streams, dim %d) given a DeepSORT tracker of %d streams, dim %d",
             z->cfg.n_streams, z->cfg.dim, v.n_streams, dim);
    RT_CHECK(v.max_tracks <= z->cfg.max_tracks, RTMODT_E_INVALID, "tracker max_tracks %d > crosscam max_tracks %d", v.max_tracks, z->cfg.max_tracks);
    RT_HIP(hipSetDevice(z->device));
    CcArgs &a = z->a;
    a.trk = src; a.t_rows = rows; a.t_mc = v.max_tracks; a.t_budget = budget;
    return cc_run(z, v.stream, true, out);
}

int rtmodt_crosscam_state(rtmodt_crosscam *z, int64_t *header, int64_t *gid, int32_t *cls, int64_t *first_seen, int64_t *last_seen, int16_t *s16, int8_t *s8,
                          int32_t *n_bind, int64_t *bind_lid, int64_t *bind_gid, int64_t *bind_last) {
    RT_CHECK(z && header, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cc_sync(z));
    int64_t st[2];
    RT_HIP(hipMemcpy(st, z->a.state, sizeof(st), hipMemcpyDeviceToHost));
    const size_t S = z->cfg.n_streams, D = z->cfg.dim, I = z->cfg.max_identities;
    RT_CHECK(st[0] >= 0 && st[0] <= (int64_t)I, RTMODT_E_INVALID, "crosscam: corrupt identity count");
    header[0] = z->calls; header[1] = st[1]; header[2] = st[0];
    const size_t n = (size_t)st[0];
    const CcTab &t = z->tab[z->cur]; const CcLed &l = z->led[z->cur];
    if (n) {
        if (gid) RT_HIP(hipMemcpy(gid, t.gid, n * 8, hipMemcpyDeviceToHost));
        if (cls) RT_HIP(hipMemcpy(cls, t.cls, n * 4, hipMemcpyDeviceToHost));
        if (first_seen) RT_HIP(hipMemcpy(first_seen, t.first, n * 8, hipMemcpyDeviceToHost));
        if (last_seen) RT_HIP(hipMemcpy(last_seen, t.last, n * S * 8, hipMemcpyDeviceToHost));
        if (s16) RT_HIP(hipMemcpy(s16, t.s16, n * D * 2, hipMemcpyDeviceToHost));
        if (s8) RT_HIP(hipMemcpy(s8, t.s8, n * D, hipMemcpyDeviceToHost));
    }
    if (n_bind) RT_HIP(hipMemcpy(n_bind, l.n, S * 4, hipMemcpyDeviceToHost));
    if (bind_lid) RT_HIP(hipMemcpy(bind_lid, l.lid, S * I * 8, hipMemcpyDeviceToHost));
    if (bind_gid) RT_HIP(hipMemcpy(bind_gid, l.gid, S * I * 8, hipMemcpyDeviceToHost));
    if (bind_last) RT_HIP(hipMemcpy(bind_last, l.last, S * I * 8, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_crosscam_load(rtmodt_crosscam *z, const int64_t *header, const int64_t *gid, const int32_t *cls, const int64_t *first_seen, const int64_t *last_seen,
                         const int16_t *s16, const int8_t *s8, const int32_t *n_bind, const int64_t *bind_lid, const int64_t *bind_gid, const int64_t *bind_last) {
    RT_CHECK(z && header && n_bind, RTMODT_E_INVALID, "bad argument");
    const size_t S = z->cfg.n_streams, D = z->cfg.dim, I = z->cfg.max_identities;
    const int64_t calls = header[0], next = header[1], n64 = header[2];
    RT_CHECK(calls >= 0 && n64 >= 0 && n64 <= (int64_t)I && next >= 1, RTMODT_E_INVALID, "crosscam load: call %lld, next gid %lld, %lld identities (table of %zu)",
             (long long)calls, (long long)next, (long long)n64, I);
    const size_t n = (size_t)n64;
    RT_CHECK(n == 0 || (gid && cls && first_seen && last_seen && s16 && s8), RTMODT_E_INVALID, "crosscam load: null table");
    for (size_t i = 0; i < n; ++i) {
        RT_CHECK(gid[i] >= 1 && gid[i] < next && (i == 0 || gid[i] > gid[i - 1]), RTMODT_E_INVALID, "crosscam load: gids not ascending in 1..next gid at row %zu", i);
        for (size_t s = 0; s < S; ++s) RT_CHECK(last_seen[i * S + s] >= 0 && last_seen[i * S + s] <= calls, RTMODT_E_INVALID, "crosscam load: last_seen of row %zu", i);
    }
    std::vector<int32_t> n8(n);
    for (size_t i = 0; i < n; ++i) {
        long long v = 0;
        for (size_t k = 0; k < D; ++k) v += (int)s8[i * D + k] * (int)s8[i * D + k];
        n8[i] = (int32_t)v;
    }
    for (size_t s = 0; s < S; ++s) {
        RT_CHECK(n_bind[s] >= 0 && n_bind[s] <= (int)I, RTMODT_E_INVALID, "crosscam load: stream %zu has %d bindings", s, n_bind[s]);
        RT_CHECK(n_bind[s] == 0 || (bind_lid && bind_gid && bind_last), RTMODT_E_INVALID, "crosscam load: null ledger");
        for (int j = 0; j < n_bind[s]; ++j) {
            const size_t o = s * I + j;
            RT_CHECK(j == 0 || bind_lid[o] > bind_lid[o - 1], RTMODT_E_INVALID, "crosscam load: stream %zu: local ids not ascending", s);
            RT_CHECK(std::binary_search(gid, gid + n, bind_gid[o]) && bind_last[o] >= 1 && bind_last[o] <= calls, RTMODT_E_INVALID,
                     "crosscam load: stream %zu: binding %d names no identity of the table", s, j);
        }
    }
    RT_TRY(cc_sync(z));
    const CcTab &t = z->tab[z->cur]; const CcLed &l = z->led[z->cur];
    if (n) {
        RT_HIP(hipMemcpy(t.gid, gid, n * 8, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(t.cls, cls, n * 4, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(t.first, first_seen, n * 8, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(t.last, last_seen, n * S * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(t.s16, s16, n * D * 2, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(t.s8, s8, n * D, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(t.n8, n8.data(), n * 4, hipMemcpyHostToDevice));
    }
    RT_HIP(hipMemcpy(l.n, n_bind, S * 4, hipMemcpyHostToDevice));
    for (size_t s = 0; s < S; ++s) {
        const size_t o = s * I, k = (size_t)n_bind[s];
        if (!k) continue;
        RT_HIP(hipMemcpy(l.lid + o, bind_lid + o, k * 8, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(l.gid + o, bind_gid + o, k * 8, hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(l.last + o, bind_last + o, k * 8, hipMemcpyHostToDevice));
    }
    const int64_t st[2] = {n64, next};
    RT_HIP(hipMemcpy(z->a.state, st, sizeof(st), hipMemcpyHostToDevice));
    RT_HIP(handle_zero(z->a.err, S * 4, z->stream));
    RT_TRY(handle_wait(z->stream));
    z->calls = calls;
    return RTMODT_OK;
}

int rtmodt_crosscam_errors(rtmodt_crosscam *z, int32_t *err) {
    RT_CHECK(z && err, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cc_sync(z));
    RT_HIP(hipMemcpy(err, z->a.err, (size_t)z->cfg.n_streams * 4, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_crosscam_clear_errors(rtmodt_crosscam *z) {
    RT_CHECK(z, RTMODT_E_INVALID, "bad argument");
    RT_TRY(cc_sync(z));
    RT_HIP(handle_zero(z->a.err, (size_t)z->cfg.n_streams * 4, z->stream));
    return handle_wait(z->stream);
}

int rtmodt_crosscam_last_ms(rtmodt_crosscam *z, float *ms) {
    RT_CHECK(z && ms, RTMODT_E_INVALID, "bad argument");
    return z->timer.elapsed(z->device, 0, 1, ms, "crosscam: no call yet");
}

int rtmodt_crosscam_similarity(int device, const int8_t *q, int nq, const int8_t *t, int nt, int dim, int32_t *dots, int32_t *sim) {
    RT_CHECK(dim >= 64 && dim <= CC_MAX_DIM && dim % 64 == 0, RTMODT_E_INVALID, "crosscam: dim %d: 64..%d in multiples of 64", dim, CC_MAX_DIM);
    RT_CHECK(nq >= 0 && nq <= CC_MAX_QUERIES && nt >= 0 && nt <= CC_MAX_IDENTITIES, RTMODT_E_INVALID, "crosscam: %d queries / %d rows: at most %d / %d", nq, nt,
             CC_MAX_QUERIES, CC_MAX_IDENTITIES);
    if (nq == 0 || nt == 0) return RTMODT_OK;
    RT_CHECK(q && t && (dots || sim), RTMODT_E_INVALID, "null argument");
    std::vector<int64_t> n2q(nq), n2t(nt);
    for (int i = 0; i < nq; ++i) { long long v = 0; for (int k = 0; k < dim; ++k) v += (int)q[(size_t)i * dim + k] * (int)q[(size_t)i * dim + k]; n2q[i] = v; }
    for (int i = 0; i < nt; ++i) { long long v = 0; for (int k = 0; k < dim; ++k) v += (int)t[(size_t)i * dim + k] * (int)t[(size_t)i * dim + k]; n2t[i] = v; }
    RT_HIP(hipSetDevice(device));
    DevBufs bufs;
    int8_t *d_q, *d_t; int64_t *d_nq, *d_nt; int32_t *d_dots, *d_sim;
    RT_TRY(bufs.up(&d_q, q, (size_t)nq * dim)); RT_TRY(bufs.up(&d_t, t, (size_t)nt * dim));
    RT_TRY(bufs.up(&d_nq, (const int64_t *)n2q.data(), (size_t)nq)); RT_TRY(bufs.up(&d_nt, (const int64_t *)n2t.data(), (size_t)nt));
    RT_TRY(bufs.alloc(&d_dots, (size_t)nq * nt)); RT_TRY(bufs.alloc(&d_sim, (size_t)nq * nt));
    CcGemm g{d_q, d_t, nullptr, nullptr, nullptr, nq, nt, dim, nt, nt, d_dots};
    hipLaunchKernelGGL(cc_gemm, dim3(cdiv(nq, 64), cdiv(nt, 64)), dim3(CC_THREADS), 0, nullptr, g);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_sim_kernel, dim3(cdiv(nq * nt, 256)), dim3(256), 0, nullptr, d_dots, d_nq, d_nt, nq, nt, d_sim);
    RT_HIP(hipGetLastError());
    RT_HIP(hipDeviceSynchronize());
    if (dots) RT_HIP(hipMemcpy(dots, d_dots, (size_t)nq * nt * 4, hipMemcpyDeviceToHost));
    if (sim) RT_HIP(hipMemcpy(sim, d_sim, (size_t)nq * nt * 4, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

}  // extern "C"
