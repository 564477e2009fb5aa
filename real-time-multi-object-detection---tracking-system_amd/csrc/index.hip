// index.hip -- an archive of appearance descriptors searched by similarity.  A device-resident, append-only RING of int8 rows with
// their metadata (rid from 1, never reused; the caller's key; stream; class; time; squared norm; a dead flag), row rid in slot
// (rid - 1) % capacity; up to 64 queries per call get the exact top-k under filters.  The reference has no counterpart: its Track
// has no descriptor and its web API answers with the detections of one image.  index_rule.h states the per-row arithmetic,
// include/rtmodt.h the per-call rules, tests/index_ref.py restates both and the kernels equal it exactly.  PARITY UNPINNED (no
// published vector index is installed where this runs, and none ranks in integers).
//
// A search = TWO launches whatever the archive holds, the outputs in one copy:
//   ix_scan    one workgroup per chunk of chunk_rows slots (at most 256 chunks), one wave per 16 queries.  The wave keeps its
//              queries as the A operand of v_mfma_i32_16x16x64_i8 in registers for the whole chunk (fragment layout as cc_gemm and
//              appearance_dotmax: A = 16 queries x 64 k, B = 16 archive rows, lane l holds the 16 consecutive k of group l >> 4 for
//              row / column l & 15; C: column l & 15, rows 4 (l >> 4) + reg) and walks the chunk 64 rows at a time: rows and
//              metadata are read from HBM once for all queries, the nq x N product lives in accumulator registers only.  The
//              epilogue runs on them: eligibility, ppm, rank = ppm << 40 | rid.  Per query a candidate buffer of max(2k, k + 16) <= 128
//              ranks in LDS and a threshold (the k-th best so far, 0 until there are k): ranks above the threshold are appended at
//              positions counted off a ballot; when fewer than 16 places remain the wave sorts the buffer (a wave-wide bitonic sort
//              of 128 keys, two per lane) and keeps k.  A query's buffer belongs to one wave: no workgroup barrier in the scan.  At the
//              end each (chunk, query) writes its k best, sorted.
//   ix_merge   one workgroup per query: the chunks' lists (at most 256 x 64 ranks = 128 KB) are sorted in LDS (bitonic, as
//              nms_kernel does), the k best look up their metadata by slot and are written out.
// Ranks are distinct, so the order in which lanes append cannot show in the result; no atomic decides an index or an order, there
// is no atomic here at all.  An exact ppm costs a 64-bit root and a division, so the epilogue first bounds it from above in
// float32 (ppm <= 10^6 dot / max(1, sqrt(nq n2) - 1), widened by 10^-5 against the rounding) and drops what cannot reach
// max(min_ppm, the threshold's ppm); what passes is computed exactly, the bound never decides a hit.
// An add = two launches (ix_add: one wave per row, its norm by a wave sum; ix_advance: next_rid), from a linker three (ix_cc_select
// in front: one workgroup compacts the identities sighted in the call just made through a prefix sum, in gid order).
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "handle_host.h"
#include "track_layout.h"

#define CC_HD __host__ __device__
#include "index_rule.h"

namespace rtmodt {

#include "wg_dev.h"

constexpr int IX_THREADS = 256, IX_WAVES = IX_THREADS / 64, IX_BUF = 128, IX_MERGE_THREADS = 1024, IX_FORGET_BLOCKS = 256;
typedef unsigned long long ix_u64;

struct IxTab { int8_t *rows; int64_t *rid, *key, *t; int32_t *stream, *cls, *n2, *dead; };     // rows [capacity][dim], the rest [capacity]
struct IxQuery { int64_t t0, t1; uint64_t mask; int64_t excl, nq; int32_t cls, min_ppm; };     // a filter and the query's squared norm

// ---- add ----
struct IxAdd {
    IxTab tab; int64_t *state;                  // state[2]: next_rid, the rows ix_cc_select chose
    const int8_t *src; const int32_t *src_idx;  // row i of the list = src[src_idx ? src_idx[i] : i]
    const int64_t *key, *t; const int32_t *stream, *cls;
    int n, D, cap;                              // n < 0: state[1]
};

__global__ __launch_bounds__(IX_THREADS) void ix_add(IxAdd a) {
    const int i = blockIdx.x * IX_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    int n = a.n >= 0 ? a.n : (int)a.state[1];
    if (i >= n || i < n - a.cap) return;                   // (wave-uniform) a list longer than the ring: only its last `cap` rows stay
    const int64_t rid = a.state[0] + i, slot = ix_slot(rid, a.cap);
    const int8_t *src = a.src + (size_t)(a.src_idx ? a.src_idx[i] : i) * a.D;
    uint32_t sum = 0;
    if (lane < a.D / 16) {
        const int4 v = ((const int4 *)src)[lane];
        ((int4 *)(a.tab.rows + (size_t)slot * a.D))[lane] = v;
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) { const int e = (int8_t)(w[j] >> (8 * b)); sum += (uint32_t)(e * e); }
    }
    sum = wave_sum_u32(sum);
    if (lane == 0) {
        a.tab.rid[slot] = rid; a.tab.key[slot] = a.key[i]; a.tab.t[slot] = a.t[i]; a.tab.stream[slot] = a.stream[i]; a.tab.cls[slot] = a.cls[i];
        a.tab.n2[slot] = (int32_t)sum; a.tab.dead[slot] = 0;
    }
}

__global__ void ix_advance(int64_t *state, int n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] += n >= 0 ? n : state[1];
}

// the identities of a linker's table sighted in call c, every `every`-th call of their life: their metadata and table row, compacted
// in gid (= table) order
struct IxCc {
    CcTableView v; long long c; int every; int64_t t;
    int64_t *state, *key, *tt; int32_t *stream, *cls, *idx;
};

__global__ __launch_bounds__(IX_THREADS) void ix_cc_select(IxCc a) {
    __shared__ int wsum[IX_WAVES];
    const int tid = threadIdx.x, S = a.v.n_streams;
    int n = (int)a.v.n_dev[0];
    n = n < 0 ? 0 : (n > a.v.max_identities ? a.v.max_identities : n);
    int cnt = 0;
    for (int base = 0; base < n; base += IX_THREADS) {
        const int i = base + tid;
        bool f = false;
        int sm = 0;
        if (i < n) {
            for (int s = S - 1; s >= 0; --s)
                if (a.v.last_seen[(size_t)i * S + s] == a.c) { f = true; sm = s; }
            f = f && (a.c - a.v.first_seen[i]) % a.every == 0;
        }
        int tot;
        const int pos = cnt + block_scan_count<IX_WAVES>(f ? 1 : 0, wsum, tot);
        if (f) { a.key[pos] = a.v.gid[i]; a.tt[pos] = a.t; a.stream[pos] = sm; a.cls[pos] = a.v.cls[i]; a.idx[pos] = i; }
        cnt += tot;
    }
    if (tid == 0) a.state[1] = cnt;
}

// ---- forget: keys ascending; a workgroup's count of the rows it marked ----
__global__ __launch_bounds__(IX_THREADS) void ix_forget(IxTab tab, int cap, const int64_t *keys, int n, int32_t *counts) {
    __shared__ int wsum[IX_WAVES];
    int mine = 0;
    for (int base = blockIdx.x * IX_THREADS; base < cap; base += gridDim.x * IX_THREADS) {
        const int i = base + threadIdx.x;
        if (i < cap && tab.rid[i] > 0 && !tab.dead[i]) {
            const int64_t k = tab.key[i];
            const int j = lower_bound_i64(keys, n, k);
            if (j < n && keys[j] == k) { tab.dead[i] = 1; ++mine; }
        }
    }
    int tot;
    block_scan_count<IX_WAVES>(mine, wsum, tot);
    if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

// ---- search ----
typedef int ix_intx4 __attribute__((ext_vector_type(4)));
struct IxSearch {
    IxTab tab; const int64_t *state; const int8_t *Qm; const IxQuery *qf;
    int nq, k, D, cap, chunk_rows, nchunks;
    ix_u64 *part;                               // [nchunks][nq][k]
    int32_t *o_n; rtmodt_index_hit *o_hits;     // [IX_MAX_QUERIES], [nq][k]
};

static size_t ix_scan_smem() { return (size_t)IX_MAX_QUERIES * (IX_BUF * 8 + 8 + 4); }

// LDS traffic between the lanes of ONE wave: the hardware keeps a wave's LDS operations in order, the fence keeps the compiler to it
__device__ __forceinline__ void ix_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ ix_u64 ix_shfl_xor(ix_u64 v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return (ix_u64)hi << 32 | lo;
}
__device__ __forceinline__ ix_u64 ix_shfl(ix_u64 v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return (ix_u64)hi << 32 | lo;
}

// 128 keys, element i in x0 of lane i (i < 64) or x1 of lane i - 64, sorted descending by a bitonic network over the wave
__device__ __forceinline__ void ix_sort128(ix_u64 &x0, ix_u64 &x1, int lane) {
#pragma unroll
    for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride == 64) {                            // (size 128: the whole range descends) the partner is the lane's other key
                const ix_u64 hi = x0 > x1 ? x0 : x1, lo = x0 > x1 ? x1 : x0;
                x0 = hi; x1 = lo;
            } else {
                const bool lower = (lane & stride) == 0;
                const ix_u64 y0 = ix_shfl_xor(x0, stride), y1 = ix_shfl_xor(x1, stride);
                const bool max0 = lower == ((lane & size) == 0), max1 = lower == (((lane + 64) & size) == 0);
                x0 = max0 ? (x0 > y0 ? x0 : y0) : (x0 < y0 ? x0 : y0);
                x1 = max1 ? (x1 > y1 ? x1 : y1) : (x1 < y1 ? x1 : y1);
            }
        }
    }
}

// a query's buffer sorted, its k best kept in front, its threshold renewed; the whole wave calls it
__device__ __forceinline__ void ix_compact(ix_u64 *buf, int *cnt, ix_u64 *thr, int k, int lane) {
    const int c = *cnt;
    ix_u64 x0 = lane < c ? buf[lane] : 0, x1 = lane + 64 < c ? buf[lane + 64] : 0;
    ix_sort128(x0, x1, lane);
    const ix_u64 kth = ix_shfl(x0, k - 1);
    ix_wave_sync();
    if (lane < k) buf[lane] = x0;
    if (lane == 0) { *cnt = c < k ? c : k; *thr = c >= k ? kth : 0; }
    ix_wave_sync();
}

struct IxMeta { int64_t rid, key, t; int32_t stream, cls, n2, dead; };

__global__ __launch_bounds__(IX_THREADS) void ix_scan(IxSearch a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ix_u64 *buf = (ix_u64 *)smem;                          // [64][IX_BUF]
    ix_u64 *sthr = buf + IX_MAX_QUERIES * IX_BUF;          // [64]
    int *scnt = (int *)(sthr + IX_MAX_QUERIES);            // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D, KC = D / 64;
    const int q0 = wave * 16;
    if (q0 >= a.nq) return;                                // (wave-uniform)
    if (lane < 16) { scnt[q0 + lane] = 0; sthr[q0 + lane] = 0; }      // the wave's own queries: no other wave touches them
    ix_wave_sync();
    const int lim = max(2 * a.k, a.k + 16);                // the places of a buffer in use: 2k, and room for 16 arrivals behind k kept
    const int64_t next = a.state[0];
    const int filled = (int)(next - 1 < (int64_t)a.cap ? (next - 1 < 0 ? 0 : next - 1) : (int64_t)a.cap);
    const int r_begin = blockIdx.x * a.chunk_rows;
    const int r_end = min(filled, r_begin + a.chunk_rows);
    const int kg = 16 * (lane >> 4), col = lane & 15, qrow = q0 + col, qb = q0 + 4 * (lane >> 4);
    ix_intx4 af[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        af[k] = ix_intx4{0, 0, 0, 0};
        if (k < KC && qrow < a.nq) af[k] = *(const ix_intx4 *)(a.Qm + (size_t)qrow * D + 64 * k + kg);
    }
    IxQuery F[4];                                          // the filters of the four queries whose dots this lane's accumulators hold
#pragma unroll
    for (int j = 0; j < 4; ++j) F[j] = a.qf[min(qb + j, a.nq - 1)];
    // 64 rows per step, software-pipelined: the rows and metadata of the next step are in flight while this step's epilogue runs
    ix_intx4 bf[4][8];
    IxMeta mt[4];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int row = r0 + 16 * f + col;
            const bool rv = row < r_end;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                bf[f][k] = ix_intx4{0, 0, 0, 0};
                if (k < KC && rv) bf[f][k] = *(const ix_intx4 *)(a.tab.rows + (size_t)row * D + 64 * k + kg);
            }
            mt[f] = IxMeta{0, 0, 0, 0, 0, 0, 1};
            if (rv) mt[f] = IxMeta{a.tab.rid[row], a.tab.key[row], a.tab.t[row], a.tab.stream[row], a.tab.cls[row], a.tab.n2[row], a.tab.dead[row]};
        }
    };
    fetch(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += 64) {
        ix_intx4 acc[4];
        IxMeta cur[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            acc[f] = ix_intx4{0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < KC) acc[f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[k], bf[f][k], acc[f], 0, 0, 0);
            cur[f] = mt[f];
        }
        fetch(r0 + 64);                                    // (past r_end: zeros, nothing is read)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const IxMeta M = cur[f];
            // a row past r_end is dead here and its dots are 0; a query past nq has a zero A row, so its dots are 0 too
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = qb + j, dot = acc[f][j];
                bool ok = dot > 0 && ix_row_ok(M.rid, M.dead, M.t, M.stream, M.cls, M.key, F[j].t0, F[j].t1, F[j].mask, F[j].cls, F[j].excl);
                if (!__ballot(ok)) continue;               // (wave-uniform)
                ix_u64 rank = 0;
                if (ok) {
                    const ix_u64 thr = sthr[q];
                    const int floor_ppm = max(F[j].min_ppm, ix_rank_ppm(thr));
                    const float den = fmaxf(1.0f, sqrtf((float)F[j].nq * (float)M.n2) * 0.99999f - 1.0f);
                    const float ub = 1.0e6f * (float)dot / den * 1.00001f + 1.0f;
                    ok = ub >= (float)floor_ppm;
                    if (ok) {
                        const int32_t ppm = ix_ppm(dot, F[j].nq, M.n2);
                        rank = ix_rank(ppm, M.rid);
                        ok = ppm >= F[j].min_ppm && rank > thr;
                    }
                }
                const ix_u64 m = __ballot(ok);
                if (!m) continue;                          // (wave-uniform)
                any = true;
                const uint32_t g = (uint32_t)(m >> (lane & 48)) & 0xffffu;    // the candidates of this lane's query: its group of 16 rows
                if (g) {
                    const int base = scnt[q];
                    if (ok) buf[q * IX_BUF + base + __popc(g & ((1u << col) - 1u))] = rank;
                    if (col == 0) scnt[q] = base + __popc(g);
                }
            }
            if (!any) continue;                            // (wave-uniform) nothing arrived: no buffer grew
            ix_wave_sync();
            const int cv = lane < 16 ? scnt[q0 + lane] : 0;
            ix_u64 need = __ballot(cv > lim - 16);          // at most 16 more arrive per fragment
            while (need) {
                const int i = __ffsll((long long)need) - 1;
                need &= need - 1;
                ix_compact(buf + (q0 + i) * IX_BUF, scnt + q0 + i, sthr + q0 + i, a.k, lane);
            }
        }
    }
    for (int i = 0; i < 16 && q0 + i < a.nq; ++i) {
        const int q = q0 + i;
        ix_compact(buf + q * IX_BUF, scnt + q, sthr + q, a.k, lane);
        if (lane < a.k) a.part[((size_t)blockIdx.x * a.nq + q) * a.k + lane] = lane < scnt[q] ? buf[q * IX_BUF + lane] : 0;
    }
}

// one workgroup per query; P = the power of two >= nchunks k
__global__ __launch_bounds__(IX_MERGE_THREADS) void ix_merge(IxSearch a, int P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ix_u64 *s = (ix_u64 *)smem;
    const int q = blockIdx.x, tid = threadIdx.x, n = a.nchunks * a.k;
    for (int i = tid; i < P; i += IX_MERGE_THREADS) s[i] = i < n ? a.part[((size_t)(i / a.k) * a.nq + q) * a.k + i % a.k] : 0;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P; i += IX_MERGE_THREADS) {
                const int j = i ^ stride;
                if (j > i) {
                    const ix_u64 x = s[i], y = s[j];
                    if (((i & size) == 0) ? x < y : x > y) { s[i] = y; s[j] = x; }
                }
            }
            __syncthreads();
        }
    bool hit = false;
    if (tid < a.k) {
        const ix_u64 r = tid < P ? s[tid] : 0;
        rtmodt_index_hit h{};
        if (r) {
            const int64_t rid = ix_rank_rid(r), slot = ix_slot(rid, a.cap);
            h.rid = rid; h.key = a.tab.key[slot]; h.t = a.tab.t[slot]; h.stream = a.tab.stream[slot]; h.cls = a.tab.cls[slot]; h.ppm = ix_rank_ppm(r);
            hit = true;
        }
        a.o_hits[(size_t)q * a.k + tid] = h;
    }
    const int nh = __syncthreads_count(hit);
    if (tid == 0) a.o_n[q] = nh;
}

}  // namespace rtmodt

// ======================================================================================
// C ABI
// ======================================================================================
using namespace rtmodt;

struct rtmodt_index : HandleBase {
    rtmodt_index_cfg cfg{};
    int chunk_rows = 0, nchunks = 0;
    int64_t next = 1;                             // next_rid as the device holds it (every entry point waits for what it queued)
    EventTimer<2> t_add, t_search;
    char *pool = nullptr;
    IxTab tab{};
    int64_t *state = nullptr;                     // [2]
    int8_t *st_rows = nullptr; int64_t *st_key = nullptr, *st_t = nullptr; int32_t *st_stream = nullptr, *st_cls = nullptr, *st_idx = nullptr;   // one add's list
    int64_t *f_keys = nullptr; int32_t *f_cnt = nullptr;
    int8_t *Qm = nullptr; IxQuery *qf = nullptr; ix_u64 *part = nullptr;
    char *o_block = nullptr; size_t o_hits_off = 0, o_bytes = 0;
    char *h_pin = nullptr;
};

namespace {

size_t ix_carve(rtmodt_index *z, char *base) {
    Carver c{base};
    const size_t D = z->cfg.dim, N = z->cfg.capacity, A = z->cfg.max_add, Q = z->cfg.max_queries, K = z->cfg.max_k;
    IxTab &t = z->tab;
    t.rows = c.take<int8_t>(N * D); t.rid = c.take<int64_t>(N); t.key = c.take<int64_t>(N); t.t = c.take<int64_t>(N);
    t.stream = c.take<int32_t>(N); t.cls = c.take<int32_t>(N); t.n2 = c.take<int32_t>(N); t.dead = c.take<int32_t>(N);
    z->state = c.take<int64_t>(2);
    z->st_rows = c.take<int8_t>(A * D); z->st_key = c.take<int64_t>(A); z->st_t = c.take<int64_t>(A);
    z->st_stream = c.take<int32_t>(A); z->st_cls = c.take<int32_t>(A); z->st_idx = c.take<int32_t>(A);
    z->f_keys = c.take<int64_t>(IX_MAX_FORGET); z->f_cnt = c.take<int32_t>(IX_FORGET_BLOCKS);
    z->Qm = c.take<int8_t>(Q * D); z->qf = c.take<IxQuery>(Q);
    z->part = c.take<ix_u64>((size_t)z->nchunks * Q * K);
    z->o_hits_off = align_up(IX_MAX_QUERIES * 4, 16);
    z->o_bytes = align_up(z->o_hits_off + Q * K * sizeof(rtmodt_index_hit), 16);
    z->o_block = c.take<char>(z->o_bytes);
    return c.size();
}

int ix_check_cfg(const rtmodt_index_cfg &c) {
    RT_CHECK(c.dim >= 64 && c.dim <= CC_MAX_DIM && c.dim % 64 == 0, RTMODT_E_INVALID, "index: dim %d: 64..%d in multiples of 64", c.dim, CC_MAX_DIM);
    RT_CHECK(c.capacity >= 1 && c.capacity <= IX_MAX_CAPACITY, RTMODT_E_INVALID, "index: capacity %d (1..%d)", c.capacity, IX_MAX_CAPACITY);
    RT_CHECK(c.max_queries >= 1 && c.max_queries <= IX_MAX_QUERIES, RTMODT_E_INVALID, "index: max_queries %d (1..%d)", c.max_queries, IX_MAX_QUERIES);
    RT_CHECK(c.max_k >= 1 && c.max_k <= IX_MAX_K, RTMODT_E_INVALID, "index: max_k %d (1..%d)", c.max_k, IX_MAX_K);
    RT_CHECK(c.max_add >= 1 && c.max_add <= IX_MAX_ADD, RTMODT_E_INVALID, "index: max_add %d (1..%d)", c.max_add, IX_MAX_ADD);
    RT_CHECK(ix_chunk_rows(c.capacity, c.chunk_rows) > 0, RTMODT_E_INVALID, "index: chunk_rows %d: 0, or a multiple of 64 that cuts %d rows into at most %d chunks",
             c.chunk_rows, c.capacity, IX_MAX_CHUNKS);
    return RTMODT_OK;
}

// ix_add + ix_advance on q for the list the staging buffers hold (n >= 0), or the one ix_cc_select left there (n < 0, at most `most`)
void ix_launch_add(rtmodt_index *z, hipStream_t q, const int8_t *src, const int32_t *src_idx, int n, int most) {
    IxAdd a{z->tab, z->state, src, src_idx, z->st_key, z->st_t, z->st_stream, z->st_cls, n, z->cfg.dim, z->cfg.capacity};
    hipLaunchKernelGGL(ix_add, dim3(cdiv(most, IX_WAVES)), dim3(IX_THREADS), 0, q, a);
    hipLaunchKernelGGL(ix_advance, dim3(1), dim3(64), 0, q, z->state, n);
}

}  // namespace

extern "C" {

void rtmodt_index_default_cfg(rtmodt_index_cfg *c) {
    if (!c) return;
    *c = rtmodt_index_cfg{};
    c->dim = 512; c->capacity = 1 << 20; c->max_queries = IX_MAX_QUERIES; c->max_k = IX_MAX_K; c->max_add = CC_MAX_IDENTITIES; c->chunk_rows = 0;
}

void rtmodt_index_destroy(rtmodt_index *z) {
    if (!z) return;
    handle_close(z, [&] {
        z->t_add.destroy(); z->t_search.destroy();
        hipFree(z->pool);
        hipHostFree(z->h_pin);
    });
    delete z;
}

int rtmodt_index_create(const rtmodt_index_cfg *cfg, rtmodt_index **out) {
    RT_CHECK(cfg && out, RTMODT_E_INVALID, "null argument");
    RT_TRY(ix_check_cfg(*cfg));
    rtmodt_index *z = new rtmodt_index();
    z->cfg = *cfg; z->device = cfg->device;
    z->chunk_rows = ix_chunk_rows(cfg->capacity, cfg->chunk_rows);
    z->nchunks = cdiv(cfg->capacity, z->chunk_rows);
    const int64_t st[2] = {1, 0};
    auto body = [&]() -> int {
        RT_TRY(handle_open(z));
        RT_TRY(z->t_add.create()); RT_TRY(z->t_search.create());
        const size_t total = ix_carve(z, nullptr);
        RT_HIP(hipMalloc((void **)&z->pool, total));
        ix_carve(z, z->pool);
        // the rows need no zeroing: an empty slot (rid 0) is never read by a search and state() hands out zeros for it
        const size_t rows_bytes = (size_t)z->cfg.capacity * z->cfg.dim;
        RT_HIP(handle_zero(z->pool + rows_bytes, total - rows_bytes, z->stream));
        RT_HIP(hipHostMalloc((void **)&z->h_pin, z->o_bytes, hipHostMallocDefault));
        RT_HIP(hipMemcpyAsync(z->state, st, sizeof(st), hipMemcpyHostToDevice, z->stream));              // (behind the zeroing of the pool)
        return RTMODT_OK;
    };
    return handle_created(body(), z, rtmodt_index_destroy, out);
}

int rtmodt_index_add(rtmodt_index *z, const int8_t *rows, int mem_kind, const int64_t *keys, const int32_t *streams, const int32_t *cls, const int64_t *t,
                     int n, int64_t *first_rid) {
    RT_CHECK(z && n >= 0, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n <= z->cfg.max_add, RTMODT_E_INVALID, "index: %d rows > max_add %d", n, z->cfg.max_add);
    RT_CHECK(mem_kind == RTMODT_MEM_HOST || mem_kind == RTMODT_MEM_DEVICE, RTMODT_E_INVALID, "index: mem_kind %d", mem_kind);
    if (first_rid) *first_rid = z->next;
    if (n == 0) return RTMODT_OK;
    RT_CHECK(rows && keys && streams && cls && t, RTMODT_E_INVALID, "null argument");
    for (int i = 0; i < n; ++i) RT_CHECK(streams[i] >= 0 && streams[i] < IX_MAX_STREAMS, RTMODT_E_INVALID, "index: row %d: stream %d (0..63)", i, streams[i]);
    RT_CHECK(z->next + n < IX_MAX_RID, RTMODT_E_CAPACITY, "index: rids are used up");
    RT_HIP(hipSetDevice(z->device));
    const hipStream_t q = z->stream;
    RT_HIP(hipMemcpyAsync(z->st_rows, rows, (size_t)n * z->cfg.dim, mem_kind == RTMODT_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, q));
    RT_HIP(hipMemcpyAsync(z->st_key, keys, (size_t)n * 8, hipMemcpyHostToDevice, q));
    RT_HIP(hipMemcpyAsync(z->st_t, t, (size_t)n * 8, hipMemcpyHostToDevice, q));
    RT_HIP(hipMemcpyAsync(z->st_stream, streams, (size_t)n * 4, hipMemcpyHostToDevice, q));
    RT_HIP(hipMemcpyAsync(z->st_cls, cls, (size_t)n * 4, hipMemcpyHostToDevice, q));
    RT_TRY(z->t_add.record(0, q));
    ix_launch_add(z, q, z->st_rows, nullptr, n, n);
    RT_HIP(hipGetLastError());
    RT_TRY(z->t_add.record(1, q));
    z->t_add.timed = true;
    RT_TRY(handle_wait(q));                                // the caller's arrays are pageable and theirs again
    z->next += n;
    return RTMODT_OK;
}

int rtmodt_index_add_crosscam(rtmodt_index *z, rtmodt_crosscam *linker, int64_t t, int every, int32_t *n_added) {
    RT_CHECK(z && linker, RTMODT_E_INVALID, "bad argument");
    CcTableView v;
    RT_TRY(crosscam_table_view(linker, &v));
    RT_CHECK(v.device == z->device, RTMODT_E_INVALID, "index on device %d, linker on device %d", z->device, v.device);
    RT_CHECK(v.dim == z->cfg.dim, RTMODT_E_INVALID, "index of dim %d given a linker of dim %d", z->cfg.dim, v.dim);
    RT_CHECK(v.max_identities <= z->cfg.max_add, RTMODT_E_INVALID, "linker max_identities %d > index max_add %d", v.max_identities, z->cfg.max_add);
    RT_CHECK(every >= 1, RTMODT_E_INVALID, "index: every %d (>= 1)", every);
    RT_CHECK(z->next + v.max_identities < IX_MAX_RID, RTMODT_E_CAPACITY, "index: rids are used up");
    RT_HIP(hipSetDevice(z->device));
    const hipStream_t q = v.stream;                        // the stream the linker's last call ran on: ordered after it
    RT_TRY(z->t_add.record(0, q));
    IxCc c{v, v.calls, every, t, z->state, z->st_key, z->st_t, z->st_stream, z->st_cls, z->st_idx};
    hipLaunchKernelGGL(ix_cc_select, dim3(1), dim3(IX_THREADS), 0, q, c);
    ix_launch_add(z, q, v.s8, z->st_idx, -1, v.max_identities);
    RT_HIP(hipGetLastError());
    RT_TRY(z->t_add.record(1, q));
    z->t_add.timed = true;
    int64_t st[2];
    RT_HIP(hipMemcpyAsync(st, z->state, sizeof(st), hipMemcpyDeviceToHost, q));
    RT_TRY(handle_wait(q));
    z->next = st[0];
    if (n_added) *n_added = (int32_t)st[1];
    return RTMODT_OK;
}

int rtmodt_index_search(rtmodt_index *z, const int8_t *queries, int nq, const rtmodt_index_filter *filters, int k, rtmodt_index_hit *hits, int32_t *n_hits) {
    RT_CHECK(z && nq >= 0, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(nq <= z->cfg.max_queries, RTMODT_E_INVALID, "index: %d queries > max_queries %d", nq, z->cfg.max_queries);
    RT_CHECK(k >= 1 && k <= z->cfg.max_k, RTMODT_E_INVALID, "index: k %d (1..max_k %d)", k, z->cfg.max_k);
    if (nq == 0) return RTMODT_OK;
    RT_CHECK(queries && filters && hits && n_hits, RTMODT_E_INVALID, "null argument");
    const int D = z->cfg.dim;
    std::vector<IxQuery> qf(nq);
    for (int i = 0; i < nq; ++i) {
        const rtmodt_index_filter &f = filters[i];
        RT_CHECK(f.min_ppm >= 1 && f.min_ppm <= IX_PPM, RTMODT_E_INVALID, "index: query %d: min_ppm %d (1..%d)", i, f.min_ppm, IX_PPM);
        long long n2 = 0;
        for (int d = 0; d < D; ++d) n2 += (int)queries[(size_t)i * D + d] * (int)queries[(size_t)i * D + d];
        qf[i] = IxQuery{f.t0, f.t1, f.stream_mask, f.exclude_key, n2, f.cls, f.min_ppm};
    }
    RT_HIP(hipSetDevice(z->device));
    const hipStream_t q = z->stream;
    int P = 2;
    while (P < z->nchunks * k) P <<= 1;
    const size_t sm_scan = ix_scan_smem(), sm_merge = (size_t)P * 8;
    static DynLdsSeen seen_s, seen_m;
    RT_TRY(raise_dynamic_lds((const void *)ix_scan, sm_scan, seen_s));
    RT_TRY(raise_dynamic_lds((const void *)ix_merge, sm_merge, seen_m));
    RT_HIP(hipMemcpyAsync(z->Qm, queries, (size_t)nq * D, hipMemcpyHostToDevice, q));
    RT_HIP(hipMemcpyAsync(z->qf, qf.data(), (size_t)nq * sizeof(IxQuery), hipMemcpyHostToDevice, q));
    IxSearch a{z->tab, z->state, z->Qm, z->qf, nq, k, D, z->cfg.capacity, z->chunk_rows, z->nchunks, z->part, (int32_t *)z->o_block,
               (rtmodt_index_hit *)(z->o_block + z->o_hits_off)};
    RT_TRY(z->t_search.record(0, q));
    hipLaunchKernelGGL(ix_scan, dim3(z->nchunks), dim3(IX_THREADS), sm_scan, q, a);
    hipLaunchKernelGGL(ix_merge, dim3(nq), dim3(IX_MERGE_THREADS), sm_merge, q, a, P);
    RT_HIP(hipGetLastError());
    RT_TRY(z->t_search.record(1, q));
    z->t_search.timed = true;
    const size_t bytes = z->o_hits_off + (size_t)nq * k * sizeof(rtmodt_index_hit);
    RT_HIP(hipMemcpyAsync(z->h_pin, z->o_block, bytes, hipMemcpyDeviceToHost, q));
    RT_TRY(handle_wait(q));
    memcpy(n_hits, z->h_pin, (size_t)nq * 4);
    memcpy(hits, z->h_pin + z->o_hits_off, (size_t)nq * k * sizeof(rtmodt_index_hit));
    return RTMODT_OK;
}

int rtmodt_index_forget(rtmodt_index *z, const int64_t *keys, int n, int64_t *n_marked) {
    RT_CHECK(z && n >= 0, RTMODT_E_INVALID, "bad argument");
    RT_CHECK(n <= IX_MAX_FORGET, RTMODT_E_INVALID, "index: %d keys to forget (at most %d per call)", n, IX_MAX_FORGET);
    if (n_marked) *n_marked = 0;
    if (n == 0) return RTMODT_OK;
    RT_CHECK(keys, RTMODT_E_INVALID, "null argument");
    std::vector<int64_t> ks(keys, keys + n);
    std::sort(ks.begin(), ks.end());
    ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
    RT_HIP(hipSetDevice(z->device));
    const hipStream_t q = z->stream;
    const int blocks = std::min(IX_FORGET_BLOCKS, cdiv(z->cfg.capacity, IX_THREADS));
    int32_t counts[IX_FORGET_BLOCKS];
    RT_HIP(hipMemcpyAsync(z->f_keys, ks.data(), ks.size() * 8, hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(ix_forget, dim3(blocks), dim3(IX_THREADS), 0, q, z->tab, z->cfg.capacity, z->f_keys, (int)ks.size(), z->f_cnt);
    RT_HIP(hipGetLastError());
    RT_HIP(hipMemcpyAsync(counts, z->f_cnt, (size_t)blocks * 4, hipMemcpyDeviceToHost, q));
    RT_TRY(handle_wait(q));
    int64_t total = 0;
    for (int b = 0; b < blocks; ++b) total += counts[b];
    if (n_marked) *n_marked = total;
    return RTMODT_OK;
}

int rtmodt_index_state(rtmodt_index *z, int64_t *header, int8_t *rows, int64_t *rid, int64_t *key, int64_t *t, int32_t *stream, int32_t *cls, int32_t *n2,
                       int32_t *dead) {
    RT_CHECK(z && header, RTMODT_E_INVALID, "bad argument");
    RT_HIP(hipSetDevice(z->device));
    RT_TRY(handle_wait(z->stream));
    int64_t st[2];
    RT_HIP(hipMemcpy(st, z->state, sizeof(st), hipMemcpyDeviceToHost));
    const size_t N = z->cfg.capacity, D = z->cfg.dim;
    RT_CHECK(st[0] >= 1 && st[0] < IX_MAX_RID, RTMODT_E_INVALID, "index: corrupt next_rid");
    const size_t filled = (size_t)std::min<int64_t>(st[0] - 1, (int64_t)N);
    header[0] = st[0]; header[1] = (int64_t)filled;
    if (rows) {                                            // slots 0 .. filled - 1 are the filled ones (the ring fills from slot 0)
        if (filled) RT_HIP(hipMemcpy(rows, z->tab.rows, filled * D, hipMemcpyDeviceToHost));
        memset(rows + filled * D, 0, (N - filled) * D);
    }
    if (rid) RT_HIP(hipMemcpy(rid, z->tab.rid, N * 8, hipMemcpyDeviceToHost));
    if (key) RT_HIP(hipMemcpy(key, z->tab.key, N * 8, hipMemcpyDeviceToHost));
    if (t) RT_HIP(hipMemcpy(t, z->tab.t, N * 8, hipMemcpyDeviceToHost));
    if (stream) RT_HIP(hipMemcpy(stream, z->tab.stream, N * 4, hipMemcpyDeviceToHost));
    if (cls) RT_HIP(hipMemcpy(cls, z->tab.cls, N * 4, hipMemcpyDeviceToHost));
    if (n2) RT_HIP(hipMemcpy(n2, z->tab.n2, N * 4, hipMemcpyDeviceToHost));
    if (dead) RT_HIP(hipMemcpy(dead, z->tab.dead, N * 4, hipMemcpyDeviceToHost));
    return RTMODT_OK;
}

int rtmodt_index_load(rtmodt_index *z, int64_t next_rid, const int8_t *rows, const int64_t *rid, const int64_t *key, const int64_t *t, const int32_t *stream,
                      const int32_t *cls, const int32_t *dead) {
    RT_CHECK(z && rows && rid && key && t && stream && cls && dead, RTMODT_E_INVALID, "null argument");
    RT_CHECK(next_rid >= 1 && next_rid < IX_MAX_RID, RTMODT_E_INVALID, "index load: next_rid %lld", (long long)next_rid);
    const size_t N = z->cfg.capacity, D = z->cfg.dim;
    std::vector<int32_t> n2(N, 0);
    for (size_t s = 0; s < N; ++s) {
        const int64_t want = ix_slot_rid((int64_t)s, (int64_t)N, next_rid);
        RT_CHECK(rid[s] == want, RTMODT_E_INVALID, "index load: slot %zu holds rid %lld, at next_rid %lld it is %lld", s, (long long)rid[s], (long long)next_rid,
                 (long long)want);
        if (!want) continue;
        RT_CHECK(stream[s] >= 0 && stream[s] < IX_MAX_STREAMS && (dead[s] == 0 || dead[s] == 1), RTMODT_E_INVALID, "index load: slot %zu: stream %d, dead %d", s,
                 stream[s], dead[s]);
        long long v = 0;
        for (size_t d = 0; d < D; ++d) v += (int)rows[s * D + d] * (int)rows[s * D + d];
        n2[s] = (int32_t)v;
    }
    RT_HIP(hipSetDevice(z->device));
    RT_TRY(handle_wait(z->stream));
    const int64_t st[2] = {next_rid, 0};
    RT_HIP(hipMemcpy(z->tab.rows, rows, N * D, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(z->tab.rid, rid, N * 8, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(z->tab.key, key, N * 8, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(z->tab.t, t, N * 8, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(z->tab.stream, stream, N * 4, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(z->tab.cls, cls, N * 4, hipMemcpyHostToDevice)); RT_HIP(hipMemcpy(z->tab.dead, dead, N * 4, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(z->tab.n2, n2.data(), N * 4, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(z->state, st, sizeof(st), hipMemcpyHostToDevice));
    RT_HIP(hipDeviceSynchronize());
    z->next = next_rid;
    return RTMODT_OK;
}

int rtmodt_index_last_ms(rtmodt_index *z, float *add_ms, float *search_ms) {
    RT_CHECK(z && (add_ms || search_ms), RTMODT_E_INVALID, "bad argument");
    RT_CHECK(z->t_add.timed || z->t_search.timed, RTMODT_E_INVALID, "index: no add or search yet");
    if (add_ms) *add_ms = 0.0f;
    if (search_ms) *search_ms = 0.0f;
    if (add_ms && z->t_add.timed) RT_TRY(z->t_add.elapsed(z->device, 0, 1, add_ms, "index: no add yet"));
    if (search_ms && z->t_search.timed) RT_TRY(z->t_search.elapsed(z->device, 0, 1, search_ms, "index: no search yet"));
    return RTMODT_OK;
}

}  // extern "C"
