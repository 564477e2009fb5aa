// tracker.hip -- the reference's _ByteTrackCore (src/tracking/tracker.py:43-194) as ONE
// kernel launch per frame: one 1024-thread workgroup (16 wave64s) per video stream, the
// whole update -- hi/lo split, IoU, row arg-max, assignment, commit, second pass, spawn,
// ageing, expiry -- in LDS.  Integer results (ids, ages, time_since_update, list order)
// and float32 bit patterns are identical to the reference's NumPy evaluation.
//
//   iou_ref            <- _batch_iou          tracker.py:150-161  (never materialised as a
//                                              matrix here: fused into the row arg-max)
//   assoc_pass         <- _linear_assignment  tracker.py:182-194  greedy branch, in its
//                         order-free form: row i is matched iff it is the SMALLEST row among
//                         those whose first-arg-max column is j and whose value >= thresh
//                         (oracle/tracker_oracle.py:assign_greedy_parallel proves the equivalence)
//   assoc_lap          <- _linear_assignment  tracker.py:168-181  lap.lapjv branch (PARITY UNPINNED:
//                         `lap` is not installed anywhere this runs; restated from its published
//                         algorithm, see the comment at assoc_lap)
//   tracker_update     <- _ByteTrackCore.update tracker.py:58-141, _age_tracks :144-148
//
// Build with -ffp-contract=off: every float op below must round separately, exactly like
// NumPy's float32 ufuncs (no FMA contraction of `a + b - w*h`).
#include "kernels.h"
#include "lap.h"

#include <climits>

namespace rtmodt {

#include "track_dev.h"

struct AssocSmem {
    float4 *tbox;      // [max_tracks] track boxes (state before this frame's commits)
    float4 *dbox;      // [max_dets]
    int *row_best;     // [max_tracks] first-arg-max column (position in the column list) or -1
    int *col_winner;   // [max_dets]   smallest passing row per column, INT_MAX = free
};

// One association pass.  rows: n_rows track indices (rows == nullptr -> identity);
// cols: n_cols detection indices.  Afterwards row r is matched iff
// row_best[r] >= 0 && col_winner[row_best[r]] == r.
// R = 2^k lanes cooperate on a row (R chosen so that all rows are in flight at once when
// they fit): with hundreds of live tracks R is 1 -- one lane per row, no cross-lane traffic,
// detection boxes read as LDS broadcasts; with a handful of tracks a whole wave shares a
// row and finishes with a wave64 butterfly (max value, then lowest column).
__device__ __forceinline__ void assoc_pass(const AssocSmem &s, const int *rows, int n_rows, const int *cols, int n_cols,
                                           float thresh) {
    for (int c = threadIdx.x; c < n_cols; c += TRK_THREADS) s.col_winner[c] = INT_MAX;
    __syncthreads();
    int R = 64;
    while (R > 1 && (n_rows * R > TRK_THREADS || (R >> 1) >= n_cols)) R >>= 1;
    const int groups = TRK_THREADS / R;
    const int gid = threadIdx.x / R, sub = threadIdx.x & (R - 1);
    for (int r = gid; r < n_rows; r += groups) {
        const float4 tb = s.tbox[rows ? rows[r] : r];
        float bv = -INFINITY;
        int bc = INT_MAX;
        for (int c = sub; c < n_cols; c += R) {
            float v = iou_ref(tb, s.dbox[cols[c]]);
            if (bc == INT_MAX || v > bv) { bv = v; bc = c; }        // increasing c: first maximum wins
        }
        for (int d = R >> 1; d >= 1; d >>= 1) {                      // butterfly inside the R-lane group
            float ov = __shfl_xor(bv, d);
            int oc = __shfl_xor(bc, d);
            bool take = (oc != INT_MAX) && (bc == INT_MAX || ov > bv || (ov == bv && oc < bc));
            if (take) { bv = ov; bc = oc; }
        }
        if (sub == 0) {
            bool ok = (bc != INT_MAX) && (bv >= thresh);
            s.row_best[r] = ok ? bc : -1;
            if (ok) atomicMin(&s.col_winner[bc], r);
        }
    }
    __syncthreads();
}


// ---------------------------------------------------------------------------------------
// assoc_lap: the `lap.lapjv(1 - iou, extend_cost=True, cost_limit=1 - thresh)` branch
// (tracker.py:168-181).  lap embeds the M x N cost in an (M+N)^2 matrix whose off-diagonal
// blocks are cost_limit/2 and whose lower-right block is 0, so matching (i, j) costs c_ij while
// leaving both unmatched costs cost_limit: the optimum is the MAXIMUM-GAIN matching of the
// bipartite graph of pairs with gain cost_limit - c_ij > 0 (c_ij = double(float32(1 - iou))).
// At match_thresh 0.8 that graph is almost a perfect set of isolated edges, so:
//   1. every lane group scans a row, counts its candidate columns (row degree) and bumps the
//      column degrees (LDS atomics);
//   2. an edge whose row AND column have degree 1 is a connected component by itself and is
//      matched outright (its gain is positive);
//   3. the remaining "contested" rows/columns (<= LAP_ROWS / LAP_COLS, <= LAP_EDGES edges) are
//      compacted into LDS and solved EXACTLY by one lane with the shortest-augmenting-path
//      (Hungarian / Jonker-Volgenant) method on the sparse graph: every row has a private dummy
//      column of cost 0 (= stay unmatched), real edges cost c_ij - cost_limit < 0, potentials in
//      double.  Only the source row's edges can have negative reduced cost, so the Dijkstra
//      scan is valid; only touched columns are ever visited or reset.
// A scene denser than the LDS budget raises the sticky error 2 (host: RTMODT_E_CAPACITY).
// Output convention = assoc_pass: row r matched iff row_best[r] >= 0 && col_winner[row_best[r]] == r.
// ---------------------------------------------------------------------------------------
// (the exact solver of step 3 -- LapSmem, lap_carve, lap_solve -- is shared with the evaluator: lap.h; steps 1-4 themselves are
//  assoc_sparse in track_dev.h, shared with the DeepSORT tracker)
// ---------------------------------------------------------------------------------------

// val(r, c): IoU (float32) of row r and column c of this pass
template <typename F>
__device__ __forceinline__ void assoc_lap(F val, int n_rows, int n_cols, double limit, int *row_best, int *col_winner, int *rowcand,
                                          const LapSmem &L, int *wsum, int *err) {
    assoc_sparse<double>([&](int r, int c, double &cost) -> bool {
        const double cd = (double)(1.0f - val(r, c));
        cost = cd - limit;
        return cd < limit;
    }, n_rows, n_cols, row_best, col_winner, rowcand, L, wsum, err);
}

// one frame of one stream (tracker.py:58-141); `didx` = which detection slot feeds it.  Every thread of the workgroup
// returns together (all exits are on workgroup-uniform conditions).
__device__ __forceinline__ void tracker_step(const TrackerArgs &a, const int sidx, const int didx, unsigned char *smem) {
    const int Mc = a.max_tracks, Nc = a.max_dets;
    // LDS carve
    float4 *tbox = (float4 *)smem;
    float4 *dbox = tbox + Mc;
    float *dconf = (float *)(dbox + Nc);
    int *dcls = (int *)(dconf + Nc);
    int *hi_idx = dcls + Nc;
    int *lo_idx = hi_idx + Nc;
    int *sp_idx = lo_idx + Nc;
    int *col_winner = sp_idx + Nc;
    int *row_best = col_winner + Nc;
    int *um_t = row_best + Mc;
    int *t_matched = um_t + Mc;
    int *wsum = t_matched + Mc;
    const bool lapjv = a.assign_mode == RTMODT_ASSIGN_LAPJV;
    LapSmem lap{};
    if (lapjv) lap = lap_carve((unsigned char *)(((uintptr_t)(wsum + TRK_WAVES + 1) + 7) & ~(uintptr_t)7), Nc);
    __shared__ int lap_err;
    if (threadIdx.x == 0) lap_err = 0;

    TrackerState st = a.states[sidx];
    long long *meta = (long long *)a.meta + (size_t)sidx * 8;
    __shared__ int act_cnt;
    if (threadIdx.x == 0) act_cnt = 0;
    const int cur = (int)meta[0];
    const int M = (int)meta[1];
    const long long next_id = meta[4];
    // explicit selects (a runtime-indexed pointer array would live in scratch)
    int64_t *c_ids = cur ? st.ids[1] : st.ids[0];   int64_t *n_ids = cur ? st.ids[0] : st.ids[1];
    float4 *c_box = cur ? st.box[1] : st.box[0];    float4 *n_box = cur ? st.box[0] : st.box[1];
    float *c_conf = cur ? st.conf[1] : st.conf[0];  float *n_conf = cur ? st.conf[0] : st.conf[1];
    int32_t *c_cls = cur ? st.cls[1] : st.cls[0];   int32_t *n_cls = cur ? st.cls[0] : st.cls[1];
    int32_t *c_age = cur ? st.age[1] : st.age[0];   int32_t *n_age = cur ? st.age[0] : st.age[1];
    int32_t *c_tsu = cur ? st.tsu[1] : st.tsu[0];   int32_t *n_tsu = cur ? st.tsu[0] : st.tsu[1];
    float4 *c_kf = cur ? st.kf[1] : st.kf[0];       float4 *n_kf = cur ? st.kf[0] : st.kf[1];
    const bool kalman = a.kalman && c_kf != nullptr;
    int n = a.det_n[didx];                                // detections are indexed by absolute stream too (+ the frame's slot offset)
    if (n > Nc) n = Nc;                                   // host rejects this; belt and braces
    const int tid = threadIdx.x;

    if (kalman)                                            // every track moves on by one frame; a track that was not matched in
        for (int i = tid; i < M; i += TRK_THREADS) {       // the previous frame (tsu >= 2) coasts with its height velocity zeroed
            Kf k = kf_load(c_kf, Mc, i);
            if (c_tsu[i] >= 2) k.vel.w = 0.f;
            kf_predict(k);
            kf_store(c_kf, Mc, i, k);
            tbox[i] = xyah_to_xyxy(k.pos);                 // association sees the PREDICTED boxes
        }
    if (n == 0) {                                         // tracker.py:70-73: age only, nothing expires
        for (int i = tid; i < M; i += TRK_THREADS) c_tsu[i] += 1;
        if (tid == 0) meta[3] = 0;
        return;
    }

    const float4 *gb = a.det_box + (size_t)didx * a.det_stride;
    const float *gc = a.det_conf + (size_t)didx * a.det_stride;
    const int32_t *gk = a.det_cls + (size_t)didx * a.det_stride;
    for (int i = tid; i < n; i += TRK_THREADS) { dbox[i] = gb[i]; dconf[i] = gc[i]; dcls[i] = gk[i]; }
    if (!kalman) for (int i = tid; i < M; i += TRK_THREADS) tbox[i] = c_box[i];
    __syncthreads();

    // ---- 1. hi / lo split (tracker.py:76-85), input order preserved ----
    int nh = 0;
    for (int base = 0; base < n; base += TRK_THREADS) {
        int i = base + tid;
        bool hi = i < n && dconf[i] >= a.track_thresh;
        int tot;
        int pos = block_scan_flag(hi, wsum, tot);
        if (i < n) {
            if (hi) hi_idx[nh + pos] = i;
            else lo_idx[(i - (nh + pos))] = i;            // lows before i = i - highs before i
        }
        nh += tot;
    }
    const int nl = n - nh;
    __syncthreads();

    AssocSmem as{tbox, dbox, row_best, col_winner};

    // ---- 2. first association: ALL tracks x high detections (tracker.py:91-106) ----
    const bool pass1 = M > 0 && nh > 0;
    if (pass1) {
        if (lapjv) assoc_lap([&](int r, int c) { return iou_ref(tbox[r], dbox[hi_idx[c]]); }, M, nh, a.cost_limit, row_best, col_winner, t_matched, lap, wsum, &lap_err);
        else assoc_pass(as, nullptr, M, hi_idx, nh, a.match_thresh);
        for (int i = tid; i < M; i += TRK_THREADS) {
            int c = row_best[i];
            bool matched = c >= 0 && col_winner[c] == i;
            t_matched[i] = matched;
            if (matched) {                                 // tracker.py:99-104
                int d = hi_idx[c];
                c_box[i] = dbox[d];
                c_conf[i] = dconf[d];
                c_cls[i] = dcls[d];
                c_age[i] += 1;
                c_tsu[i] = 0;
                if (kalman) { Kf k = kf_load(c_kf, Mc, i); kf_update(k, xyxy_to_xyah(dbox[d])); kf_store(c_kf, Mc, i, k); }
            }
        }
    } else {
        for (int i = tid; i < M; i += TRK_THREADS) t_matched[i] = 0;
        for (int c = tid; c < nh; c += TRK_THREADS) col_winner[c] = INT_MAX;
    }
    __syncthreads();

    // spawn list = unmatched high detections, ascending (tracker.py:89,126): taken now,
    // before pass 2 reuses col_winner
    int nsp = 0;
    for (int base = 0; base < nh; base += TRK_THREADS) {
        int c = base + tid;
        bool f = c < nh && col_winner[c] == INT_MAX;
        int tot;
        int pos = block_scan_flag(f, wsum, tot);
        if (f) sp_idx[nsp + pos] = hi_idx[c];
        nsp += tot;
    }
    // unmatched tracks, ascending (tracker.py:109)
    int num = 0;
    for (int base = 0; base < M; base += TRK_THREADS) {
        int i = base + tid;
        bool f = i < M && !t_matched[i];
        int tot;
        int pos = block_scan_flag(f, wsum, tot);
        if (f) um_t[num + pos] = i;
        num += tot;
    }
    __syncthreads();

    // ---- 3. second association: unmatched tracks x low detections, SAME threshold (tracker.py:110-123) ----
    if (num > 0 && nl > 0) {
        if (lapjv) assoc_lap([&](int r, int c) { return iou_ref(tbox[um_t[r]], dbox[lo_idx[c]]); }, num, nl, a.cost_limit, row_best, col_winner, t_matched, lap, wsum, &lap_err);
        else assoc_pass(as, um_t, num, lo_idx, nl, a.match_thresh);
        for (int r = tid; r < num; r += TRK_THREADS) {
            int c = row_best[r];
            if (c >= 0 && col_winner[c] == r) {
                int i = um_t[r], d = lo_idx[c];
                c_box[i] = dbox[d];
                c_conf[i] = dconf[d];
                c_cls[i] = dcls[d];
                c_age[i] += 1;
                c_tsu[i] = 0;
                if (kalman) { Kf k = kf_load(c_kf, Mc, i); kf_update(k, xyxy_to_xyah(dbox[d])); kf_store(c_kf, Mc, i, k); }
            }
        }
    }

    // ---- 4. spawn (tracker.py:126-135) ----
    int err = 0;
    if (M + nsp > Mc) { err = 1; nsp = Mc - M; }
    for (int k = tid; k < nsp; k += TRK_THREADS) {
        int d = sp_idx[k], i = M + k;
        c_ids[i] = next_id + k;
        c_box[i] = dbox[d];
        c_conf[i] = dconf[d];
        c_cls[i] = dcls[d];
        c_age[i] = 1;
        c_tsu[i] = 0;
        if (kalman) kf_store(c_kf, Mc, i, kf_initiate(xyxy_to_xyah(dbox[d])));
    }
    const int M2 = M + nsp;
    __syncthreads();                                      // state writes visible to the whole workgroup

    // ---- 5. age every track, drop tsu > track_buffer, stable (tracker.py:138-139, :144-148) ----
    const int nxt = cur ^ 1;
    int kept = 0, active = 0;
    for (int base = 0; base < M2; base += TRK_THREADS) {
        int i = base + tid;
        int tsu = 0;
        bool keep = false;
        if (i < M2) { tsu = c_tsu[i] + 1; keep = tsu <= a.track_buffer; }
        int tot;
        int pos = block_scan_flag(keep, wsum, tot);
        if (keep) {
            int o = kept + pos;
            n_ids[o] = c_ids[i];
            n_box[o] = c_box[i];
            n_conf[o] = c_conf[i];
            n_cls[o] = c_cls[i];
            n_age[o] = c_age[i];
            n_tsu[o] = tsu;
            if (kalman) kf_store(n_kf, Mc, o, kf_load(c_kf, Mc, i));
        }
        if (keep && tsu == 0) atomicAdd(&act_cnt, 1);      // tracker.py:141 -- never true (SURVEY finding 4)
        kept += tot;
    }
    __syncthreads();
    active = act_cnt;
    if (tid == 0) {
        meta[0] = nxt;
        meta[1] = kept;
        if (err) meta[2] = 1;
        else if (lap_err) meta[2] = lap_err;
        meta[3] = active;
        meta[4] = next_id + nsp;
    }
}

// One workgroup per stream.  A detector batch that holds n_frames CONSECUTIVE frames of every stream (slot f * frame_step + s)
// is consumed in ONE launch: the workgroup walks its stream's frames in order -- tracker.py:58-141 still sees them one at a
// time -- with a workgroup barrier (and its workgroup-scope fence) between frames: the state and meta words frame f wrote
// are what frame f + 1 reads.  n_frames == 1 is the ordinary per-frame update.
__global__ __launch_bounds__(TRK_THREADS) void tracker_update(TrackerArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int sidx = a.stream_base + blockIdx.x;
    for (int f = 0; f < a.n_frames; ++f) {
        tracker_step(a, sidx, sidx + f * a.frame_step, smem);
        __syncthreads();
    }
}

static size_t tracker_smem_bytes(int Mc, int Nc) {
    return (size_t)Mc * 16 + (size_t)Nc * 16 + (size_t)Nc * 4 * 6 + (size_t)Mc * 4 * 3 + (TRK_WAVES + 1) * 4 + 64;
}

int launch_tracker_update(const TrackerArgs &a, hipStream_t s) {
    size_t smem = tracker_smem_bytes(a.max_tracks, a.max_dets) + (a.assign_mode == RTMODT_ASSIGN_LAPJV ? lap_smem_bytes(a.max_dets) + 8 : 0);
    RT_CHECK(smem <= 150 * 1024, RTMODT_E_INVALID, "tracker: max_tracks %d / max_dets %d need %zu B of LDS (> 150 KiB)", a.max_tracks,
             a.max_dets, smem);
    static DynLdsSeen seen;                                // the attribute is per device
    RT_TRY(raise_dynamic_lds((const void *)tracker_update, smem, seen));
    hipLaunchKernelGGL(tracker_update, dim3(a.n_streams), dim3(TRK_THREADS), smem, s, a);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

// ---- standalone pieces for the fixture-level parity tests (G1, G2) ----
__global__ void iou_matrix_kernel(const float4 *__restrict__ a, int m, const float4 *__restrict__ b, int n, float *__restrict__ out) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)m * n) return;
    int i = (int)(idx / n), j = (int)(idx - (long)i * n);
    out[idx] = iou_ref(a[i], b[j]);
}

int launch_iou_matrix(const float4 *a, int m, const float4 *b, int n, float *out, hipStream_t s) {
    long total = (long)m * n;
    if (total == 0) return RTMODT_OK;
    hipLaunchKernelGGL(iou_matrix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, m, b, n, out);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

// greedy assignment on a caller-supplied matrix: one workgroup, wave per row, same
// arg-max / atomicMin scheme as assoc_pass (col_winner lives in global memory here).
__global__ __launch_bounds__(TRK_THREADS) void assign_greedy_kernel(const float *__restrict__ iou, int m, int n, float thresh,
                                                                    int32_t *__restrict__ row_to_col, int32_t *__restrict__ col_winner) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < n; c += TRK_THREADS) col_winner[c] = INT_MAX;
    __syncthreads();
    for (int r = wave; r < m; r += TRK_WAVES) {
        float bv = -INFINITY;
        int bc = INT_MAX;
        for (int c = lane; c < n; c += 64) {
            float v = iou[(long)r * n + c];
            if (bc == INT_MAX || v > bv) { bv = v; bc = c; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            float ov = __shfl_xor(bv, d);
            int oc = __shfl_xor(bc, d);
            bool take = (oc != INT_MAX) && (bc == INT_MAX || ov > bv || (ov == bv && oc < bc));
            if (take) { bv = ov; bc = oc; }
        }
        if (lane == 0) {
            bool ok = (bc != INT_MAX) && (bv >= thresh);
            row_to_col[r] = ok ? bc : -1;
            if (ok) atomicMin(&col_winner[bc], r);
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < m; r += TRK_THREADS) {
        int c = row_to_col[r];
        if (c >= 0 && col_winner[c] != r) row_to_col[r] = -1;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += TRK_THREADS) col_winner[c] = col_winner[c] != INT_MAX;   // -> col_used
}

int launch_assign_greedy(const float *iou, int m, int n, float thresh, int32_t *row_to_col, int32_t *col_used, hipStream_t s) {
    hipLaunchKernelGGL(assign_greedy_kernel, dim3(1), dim3(TRK_THREADS), 0, s, iou, m, n, thresh, row_to_col, col_used);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}


// lapjv branch on a caller-supplied matrix: one workgroup; LDS = row_best[m] rowcand[m] col_winner[n] + LapSmem
__global__ __launch_bounds__(TRK_THREADS) void assign_lapjv_kernel(const float *__restrict__ iou, int m, int n, double limit,
                                                                   int32_t *__restrict__ row_to_col, int32_t *__restrict__ col_used,
                                                                   int32_t *__restrict__ err_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *row_best = (int *)smem, *rowcand = row_best + m, *col_winner = rowcand + m, *wsum = col_winner + n;
    LapSmem L = lap_carve((unsigned char *)(((uintptr_t)(wsum + TRK_WAVES + 1) + 7) & ~(uintptr_t)7), n);
    __shared__ int err;
    if (threadIdx.x == 0) err = 0;
    __syncthreads();
    assoc_lap([&](int r, int c) { return iou[(long)r * n + c]; }, m, n, limit, row_best, col_winner, rowcand, L, wsum, &err);
    for (int r = threadIdx.x; r < m; r += TRK_THREADS) {
        const int c = row_best[r];
        row_to_col[r] = (c >= 0 && col_winner[c] == r) ? c : -1;
    }
    for (int c = threadIdx.x; c < n; c += TRK_THREADS) col_used[c] = col_winner[c] != INT_MAX;
    if (threadIdx.x == 0) *err_out = err;
}

int launch_assign_lapjv(const float *iou, int m, int n, double cost_limit, int32_t *row_to_col, int32_t *col_used, int32_t *err,
                        hipStream_t s) {
    size_t smem = (size_t)(2 * m + n + TRK_WAVES + 1) * 4 + 8 + lap_smem_bytes(n);
    RT_CHECK(smem <= 150 * 1024, RTMODT_E_INVALID, "assign_lapjv: %d x %d needs %zu B of LDS", m, n, smem);
    static DynLdsSeen seen;
    RT_TRY(raise_dynamic_lds((const void *)assign_lapjv_kernel, smem, seen));
    hipLaunchKernelGGL(assign_lapjv_kernel, dim3(1), dim3(TRK_THREADS), smem, s, iou, m, n, cost_limit, row_to_col, col_used, err);
    RT_HIP(hipGetLastError());
    return RTMODT_OK;
}

}  // namespace rtmodt
