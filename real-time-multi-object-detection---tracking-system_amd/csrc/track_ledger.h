// track_ledger.h -- the arithmetic of the per-stream ledgers keyed by track id (zones.hip, crossing.hip, speed.hip, snapshot.hip):
// rows sorted by id, double-buffered, merged by rank once per frame.  Plain C++, no HIP header, like cell_grid.h and motion_model.h:
// the kernels run these functions through the workgroup steps of track_ledger_dev.h, tests/native/track_ledger_check.cpp runs them
// serially against a sort.  DESIGN.md, "The track ledger and the track source".
//   A frame's new ledger = the MEMBERS of this frame's list (the entries the module takes a row for) + the old rows it RETAINS (no
//   member claimed them and the module keeps them), in id order.  Nothing is sorted: a member's position is its place among the
//   members plus the retained rows with a smaller id, a retained row's is its rank plus the members with a smaller id.
//   ret_pre[0 .. n_old]  a flag per old row (non-zero: retained unless a member matches it) until the rows are ranked, then the rank
//                        encoding: a retained row holds its rank, any other row -(rank of the next retained row) - 1; so
//                        tl_ranks_below(ret_pre, j) = retained rows among old[0 .. j) for every j <= n_old.
//   ppre[0 .. n]         exclusive prefix of the list's member flags (null: every entry is a member).
//   The list ascends in id unless the swap guard (swapguard.hip) has exchanged two ids in a tracker's state: then a member's place
//   among the members is counted, not read off its list position.
//   Overflow (members + retained > cap): this frame's rows are kept, the idle ones dropped, sticky error 1.
#pragma once

#include <algorithm>
#include <cstdint>

#ifndef TL_HD
#define TL_HD
#endif

namespace rtmodt {

TL_HD inline int tl_lower_bound(const int64_t *a, int n, int64_t x) {     // first index with a[i] >= x
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the rank encoding and its decode
TL_HD inline int tl_rank_encode(bool retained, int rank) { return retained ? rank : -rank - 1; }
TL_HD inline int tl_ranks_below(const int *ret_pre, int j) { const int v = ret_pre[j]; return v >= 0 ? v : -v - 1; }

// members of the list with an id < x: a binary search when the list ascends, a count when it does not
TL_HD inline int tl_members_below(const int64_t *ids, const int *ppre, int n, bool ascending, int64_t x) {
    if (ascending) { const int k = tl_lower_bound(ids, n, x); return ppre ? ppre[k] : k; }
    int c = 0;
    for (int k = 0; k < n; ++k) c += (!ppre || ppre[k + 1] != ppre[k]) && ids[k] < x ? 1 : 0;
    return c;
}

// the old row of `id`, or -1
TL_HD inline int tl_match(const int64_t *old_id, int n_old, int64_t id) {
    const int j = tl_lower_bound(old_id, n_old, id);
    return j < n_old && old_id[j] == id ? j : -1;
}

TL_HD inline bool tl_overflow(int n_members, int n_ret, int cap) { return n_members + n_ret > cap; }

// one frame's merge, once its steps have run: what a row's new position is computed from
struct TlMerge {
    const int64_t *ids; const int *ppre; int n;               // the list; ppre null: every entry is a member
    const int64_t *old_id; const int *ret_pre; int n_old;     // the old rows, rank-encoded
    int n_members, n_ret;
    bool ascending, overflow;
};

// the new row of member t (its index among the members in list order), whose id is `id`
TL_HD inline int tl_member_pos(const TlMerge &m, int t, int64_t id) {
    const int place = m.ascending ? t : tl_members_below(m.ids, m.ppre, m.n, false, id);
    return m.overflow ? place : place + tl_ranks_below(m.ret_pre, tl_lower_bound(m.old_id, m.n_old, id));
}
// the new row of old row j, or -1: the row is not retained, or the ledger overflows
TL_HD inline int tl_idle_pos(const TlMerge &m, int j) {
    const int v = m.ret_pre[j];
    return m.overflow || v < 0 ? -1 : v + tl_members_below(m.ids, m.ppre, m.n, m.ascending, m.old_id[j]);
}
TL_HD inline int tl_rows(const TlMerge &m) { return m.n_members + (m.overflow ? 0 : m.n_ret); }

// a stream's meta row: {cur, rows, sticky error, 0}
TL_HD inline int tl_meta_cur(const int64_t *meta) { return (int)meta[0] & 1; }
TL_HD inline int tl_meta_rows(const int64_t *meta, int cap) { const int n = (int)meta[1]; return n < 0 ? 0 : (n > cap ? cap : n); }
TL_HD inline void tl_meta_write(int64_t *meta, int cur, int rows, int err) {
    meta[0] = cur ^ 1;
    meta[1] = rows;
    if (err) meta[2] = err;
}

// host: one list in id order.  perm[i] = the caller's index of sorted entry i, inv (may be null) its inverse; the sort is stable.
// Returns -1, or the sorted position of an id that appears twice (the ledger holds one row per id: the caller refuses the list)
inline int tl_sort_list(const int64_t *ids, int n, int32_t *perm, int32_t *inv) {
    for (int i = 0; i < n; ++i) perm[i] = i;
    std::stable_sort(perm, perm + n, [&](int a, int b) { return ids[a] < ids[b]; });
    int dup = -1;
    for (int i = 0; i < n; ++i) {
        if (inv) inv[perm[i]] = i;
        if (dup < 0 && i > 0 && ids[perm[i]] == ids[perm[i - 1]]) dup = i;
    }
    return dup;
}

}  // namespace rtmodt
