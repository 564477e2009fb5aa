// track_ledger_dev.h -- the workgroup steps of a ledger's merge, built on track_ledger.h and on block_scan_count (wg_dev.h).  Include
// inside namespace rtmodt, after wg_dev.h; track_ledger.h is included at file scope with TL_HD = __host__ __device__.  A module's kernel
// carves its own LDS (old_id[cap], ret_pre[cap + 1], ppre[n_max + 1], wsum[WAVES], an int for the order test) and calls, in order:
//   ledger_stage_old     old ids -> LDS, and a flag per old row: non-zero = retained unless a member matches it     (no barrier)
//   ledger_compact       the members of the list, by the module's predicate, in list order: ppre, p_idx             (2 per pass)
//   ledger_list_ascends  the list's order                                                                           (3, the first on entry)
//   ledger_match         every member's old row; a matched row is no idle row                                       (no barrier)
//   ledger_rank          flags -> the rank encoding, in place; the number of retained rows                          (1 + 2 per pass + 1)
//   ledger_decide        overflow, and the sticky error it raises                                                    (no barrier)
// and then holds a TlMerge: tl_member_pos / tl_idle_pos give a row's new position.  zones.hip has no compaction (every entry is a
// member, p_idx and ppre null); snapshot.hip ranks its rows itself (two scans per pass, three row classes) and shares the rest.
#pragma once

template <int THREADS, typename F>
__device__ __forceinline__ void ledger_stage_old(const int64_t *o_id, int n_old, int64_t *old_id, int *ret_pre, F flag) {
    for (int j = threadIdx.x; j < n_old; j += THREADS) { old_id[j] = o_id[j]; ret_pre[j] = flag(j); }
}

// member(i) is asked of every list entry once; returns the number of members
template <int THREADS, typename F>
__device__ __forceinline__ int ledger_compact(int n, int *ppre, int32_t *p_idx, int *wsum, F member) {
    int n_members = 0;
    for (int base = 0; base < n; base += THREADS) {
        const int i = base + threadIdx.x;
        const bool f = i < n && member(i);
        int tot;
        const int pos = n_members + block_scan_count<THREADS / 64>(f ? 1 : 0, wsum, tot);
        if (i < n) ppre[i] = pos;
        if (f) p_idx[pos] = i;
        n_members += tot;
    }
    if (threadIdx.x == 0) ppre[n] = n_members;
    return n_members;
}

// *flag is 0 on entry and on return (thread 0 wrote it before an earlier barrier, or before this one)
template <int THREADS> __device__ __forceinline__ bool ledger_list_ascends(const int64_t *ids, int n, int *flag) {
    __syncthreads();
    for (int i = threadIdx.x + 1; i < n; i += THREADS)
        if (!(ids[i - 1] < ids[i])) *flag = -1;              // (every writer stores the same value)
    __syncthreads();
    const bool ascending = *flag != -1;
    __syncthreads();
    if (threadIdx.x == 0 && !ascending) *flag = 0;
    return ascending;
}

// oldpos[t] = the old row of member t or -1.  EXPIRED_IS_MISS: a matched row whose flag is already 0 is not this track's row either
// (crossing, speed); otherwise it still is, and the module applies the expiry to what it carries over (zones).  p_idx null: member t is
// list entry t
template <int THREADS, bool EXPIRED_IS_MISS>
__device__ __forceinline__ void ledger_match(const int64_t *ids, const int32_t *p_idx, int n_members, const int64_t *old_id, int n_old, int *ret_pre,
                                             int32_t *oldpos) {
    for (int t = threadIdx.x; t < n_members; t += THREADS) {
        const int j = tl_match(old_id, n_old, ids[p_idx ? p_idx[t] : t]);      // (ids are unique: no other thread touches ret_pre[j])
        oldpos[t] = j >= 0 && (!EXPIRED_IS_MISS || ret_pre[j]) ? j : -1;
        if (j >= 0) ret_pre[j] = 0;
    }
}

template <int THREADS> __device__ __forceinline__ int ledger_rank(int n_old, int *ret_pre, int *wsum) {
    __syncthreads();
    int n_ret = 0;
    for (int base = 0; base < n_old; base += THREADS) {
        const int j = base + threadIdx.x;
        const int f = j < n_old && ret_pre[j] ? 1 : 0;
        int tot;
        const int pos = block_scan_count<THREADS / 64>(f, wsum, tot);
        if (j < n_old) ret_pre[j] = tl_rank_encode(f, n_ret + pos);
        n_ret += tot;
    }
    if (threadIdx.x == 0) ret_pre[n_old] = tl_rank_encode(false, n_ret);
    __syncthreads();
    return n_ret;
}

// the merge's outcome; an overflow raises the sticky error 1 in *err
__device__ __forceinline__ TlMerge ledger_decide(const int64_t *ids, const int *ppre, int n, const int64_t *old_id, const int *ret_pre, int n_old, int n_members,
                                                 int n_ret, bool ascending, int cap, int *err) {
    const TlMerge m{ids, ppre, n, old_id, ret_pre, n_old, n_members, n_ret, ascending, tl_overflow(n_members, n_ret, cap)};
    if (m.overflow && threadIdx.x == 0) *err = 1;
    return m;
}
