// track_ledger_check.cpp -- csrc/track_ledger.h on the host, by itself (tests/test_track_ledger_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers).  It runs a ledger's whole merge serially, step for step as track_ledger_dev.h runs it on
// a workgroup, and compares every new position, every old-row match, the row count and the overflow flag with an oracle that knows
// nothing of ranks: it concatenates the member ids and the retained idle ids, sorts them and looks each one up.
//   sizes       old rows and list lengths each of {0, 1, 63, 64, 65, 255, 256, 257, 600}: around one and two passes of a 256-thread
//               workgroup and past them -- the swap guard's GPU tests stop at 32 tracks
//   membership  every entry a member (zones: no prefix array), then a random half
//   keep        every old row kept, none, a random half
//   expiry      "a matched row that is not kept is a miss" on (crossing, speed) and off (zones)
//   order       the list ascending, then with 1, 2 and every other adjacent id pair exchanged (the counting path)
//   cap         exactly members + retained, one below (overflow), one above
// and the staging sort: perm and inv inverses, the sort stable, a duplicate id reported.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "track_ledger.h"

using namespace rtmodt;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int failures = 0;
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            if (++failures <= 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } \
        }                                                        \
    } while (0)

struct Case { int n_old, n, members, keep, miss, swaps, cap_delta; };

static void run_case(const Case &c) {
    // ids: a shuffled pool; the old rows and the list share about half of the shorter one
    std::vector<int64_t> pool(2 * (c.n_old + c.n) + 2);
    for (size_t i = 0; i < pool.size(); ++i) pool[i] = (int64_t)(7 * i) - 1000;
    for (size_t i = pool.size(); i > 1; --i) std::swap(pool[i - 1], pool[rnd() % i]);
    std::vector<int64_t> old_id(pool.begin(), pool.begin() + c.n_old);
    const int shared = std::min(c.n_old, c.n) / 2;
    std::vector<int64_t> ids(pool.begin(), pool.begin() + shared);
    ids.insert(ids.end(), pool.begin() + c.n_old, pool.begin() + c.n_old + (c.n - shared));
    std::sort(old_id.begin(), old_id.end());
    std::sort(ids.begin(), ids.end());
    const int n = c.n, n_old = c.n_old;
    const int n_swaps = c.swaps == 3 ? n / 2 : c.swaps;
    for (int k = 0; k < n_swaps && 2 * k + 1 < n; ++k) {
        const int at = c.swaps == 3 ? 2 * k : (int)(rnd() % (n - 1));
        std::swap(ids[at], ids[at + 1]);      // (two random exchanges may undo each other: the order test decides)
    }
    std::vector<char> member(n), keep(n_old);
    for (int i = 0; i < n; ++i) member[i] = c.members == 0 ? 1 : (rnd() & 1);
    for (int j = 0; j < n_old; ++j) keep[j] = c.keep == 0 ? 1 : c.keep == 1 ? 0 : (rnd() & 1);

    // ---- the merge, serially, through track_ledger.h ----
    std::vector<int> ret_pre(n_old + 1), ppre_v(n + 1), p_idx, oldpos;
    for (int j = 0; j < n_old; ++j) ret_pre[j] = keep[j];
    for (int i = 0; i < n; ++i) { ppre_v[i] = (int)p_idx.size(); if (member[i]) p_idx.push_back(i); }
    ppre_v[n] = (int)p_idx.size();
    const int *ppre = c.members == 0 ? nullptr : ppre_v.data();
    const int n_members = (int)p_idx.size();
    bool ascending = true;
    for (int i = 1; i < n; ++i) ascending = ascending && ids[i - 1] < ids[i];
    oldpos.resize(n_members);
    for (int t = 0; t < n_members; ++t) {
        const int j = tl_match(old_id.data(), n_old, ids[p_idx[t]]);
        oldpos[t] = j >= 0 && (!c.miss || ret_pre[j]) ? j : -1;
        if (j >= 0) ret_pre[j] = 0;
    }
    int n_ret = 0;
    for (int j = 0; j < n_old; ++j) { const bool f = ret_pre[j] != 0; ret_pre[j] = tl_rank_encode(f, n_ret); n_ret += f ? 1 : 0; }
    ret_pre[n_old] = tl_rank_encode(false, n_ret);
    const int cap = n_members + n_ret + c.cap_delta;
    const TlMerge m{ids.data(), ppre, n, old_id.data(), ret_pre.data(), n_old, n_members, n_ret, ascending, tl_overflow(n_members, n_ret, cap)};

    // ---- the oracle ----
    std::vector<int64_t> mem_ids, idle_ids;
    for (int i = 0; i < n; ++i) if (member[i]) mem_ids.push_back(ids[i]);
    std::vector<int64_t> mem_sorted(mem_ids);
    std::sort(mem_sorted.begin(), mem_sorted.end());
    std::vector<char> idle(n_old);
    for (int j = 0; j < n_old; ++j) {
        idle[j] = keep[j] && !std::binary_search(mem_sorted.begin(), mem_sorted.end(), old_id[j]);
        if (idle[j]) idle_ids.push_back(old_id[j]);
    }
    const bool overflow = (int)(mem_ids.size() + idle_ids.size()) > cap;
    std::vector<int64_t> all(mem_ids);
    if (!overflow) all.insert(all.end(), idle_ids.begin(), idle_ids.end());
    std::sort(all.begin(), all.end());
    auto where = [&](int64_t id) { return (int)(std::lower_bound(all.begin(), all.end(), id) - all.begin()); };      // (ids are unique)

#define WHERE "n_old %d n %d members %d keep %d miss %d swaps %d cap%+d"
#define TAG c.n_old, c.n, c.members, c.keep, c.miss, c.swaps, c.cap_delta
    EXPECT(m.overflow == overflow, "overflow %d, oracle %d: " WHERE, (int)m.overflow, (int)overflow, TAG);
    EXPECT(tl_rows(m) == (int)all.size(), "rows %d, oracle %zu: " WHERE, tl_rows(m), all.size(), TAG);
    EXPECT(n_ret == (int)idle_ids.size(), "n_ret %d, oracle %zu: " WHERE, n_ret, idle_ids.size(), TAG);
    for (int j = 0, below = 0; j <= n_old; below += j < n_old ? idle[j] : 0, ++j) {
        if (tl_ranks_below(ret_pre.data(), j) != below) { EXPECT(false, "ranks_below(%d) = %d, oracle %d: " WHERE, j, tl_ranks_below(ret_pre.data(), j), below, TAG); break; }
    }
    for (int t = 0; t < n_members; ++t) {
        const int64_t id = ids[p_idx[t]];
        const int np = tl_member_pos(m, t, id), want = where(id);
        int j = (int)(std::find(old_id.begin(), old_id.end(), id) - old_id.begin());
        if (j == n_old || (c.miss && !keep[j])) j = -1;
        EXPECT(np == want, "member %d (id %lld) -> %d, oracle %d: " WHERE, t, (long long)id, np, want, TAG);
        EXPECT(oldpos[t] == j, "member %d (id %lld) oldpos %d, oracle %d: " WHERE, t, (long long)id, oldpos[t], j, TAG);
        if (np != want || oldpos[t] != j) break;
    }
    for (int j = 0; j < n_old; ++j) {
        const int np = tl_idle_pos(m, j), want = idle[j] && !overflow ? where(old_id[j]) : -1;
        EXPECT(np == want, "old row %d (id %lld) -> %d, oracle %d: " WHERE, j, (long long)old_id[j], np, want, TAG);
        if (np != want) break;
    }
#undef TAG
#undef WHERE
}

static void check_meta() {
    int64_t meta[4] = {3, 700, 0, 0};
    EXPECT(tl_meta_cur(meta) == 1 && tl_meta_rows(meta, 600) == 600, "meta read: cur %d rows %d", tl_meta_cur(meta), tl_meta_rows(meta, 600));
    meta[1] = -5;
    EXPECT(tl_meta_rows(meta, 600) == 0, "meta read: negative rows -> %d", tl_meta_rows(meta, 600));
    meta[1] = 7;
    EXPECT(tl_meta_rows(meta, 600) == 7, "meta read: rows %d", tl_meta_rows(meta, 600));
    tl_meta_write(meta, 1, 9, 0);
    EXPECT(meta[0] == 0 && meta[1] == 9 && meta[2] == 0, "meta write without an error");
    tl_meta_write(meta, 0, 4, 1);
    EXPECT(meta[0] == 1 && meta[1] == 4 && meta[2] == 1, "meta write with an error");
    tl_meta_write(meta, 1, 4, 0);
    EXPECT(meta[2] == 1, "the error is sticky");
    printf("ok meta\n");
}

static void check_staging() {
    for (int n : {0, 1, 2, 63, 257, 600}) {
        std::vector<int64_t> ids(n);
        for (int i = 0; i < n; ++i) ids[i] = 5 * (int64_t)i - 300;
        for (int i = n; i > 1; --i) std::swap(ids[i - 1], ids[rnd() % i]);
        std::vector<int32_t> perm(n), inv(n);
        EXPECT(tl_sort_list(ids.data(), n, perm.data(), inv.data()) == -1, "staging n %d: a duplicate reported where there is none", n);
        for (int i = 0; i < n; ++i) {
            EXPECT(perm[inv[i]] == i && inv[perm[i]] == i, "staging n %d: perm and inv are no inverses at %d", n, i);
            EXPECT(i == 0 || ids[perm[i - 1]] < ids[perm[i]], "staging n %d: not ascending at %d", n, i);
        }
        std::vector<int32_t> perm2(n);
        EXPECT(tl_sort_list(ids.data(), n, perm2.data(), nullptr) == -1 && perm2 == perm, "staging n %d: without inv", n);
        if (n < 2) continue;
        // one id twice, at two random places: refused, and the two keep the caller's order (stable)
        const int a = (int)(rnd() % n);
        int b = (int)(rnd() % (n - 1));
        b += b >= a ? 1 : 0;
        ids[b] = ids[a];
        const int dup = tl_sort_list(ids.data(), n, perm.data(), inv.data());
        EXPECT(dup >= 1 && dup < n, "staging n %d: the duplicate is not reported (%d)", n, dup);
        if (dup >= 1 && dup < n) {
            EXPECT(ids[perm[dup]] == ids[a] && ids[perm[dup - 1]] == ids[a], "staging n %d: position %d is not the duplicate", n, dup);
            EXPECT(perm[dup - 1] == std::min(a, b) && perm[dup] == std::max(a, b), "staging n %d: the sort is not stable", n);
        }
        for (int i = 0; i < n; ++i) EXPECT(perm[inv[i]] == i, "staging n %d with a duplicate: perm and inv are no inverses at %d", n, i);
    }
    printf("ok staging\n");
}

int main() {
    const int sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 600};
    for (int n_old : sizes)
        for (int n : sizes) {
            const int before = failures;
            int cases = 0;
            for (int members = 0; members < 2; ++members)
                for (int keep = 0; keep < 3; ++keep)
                    for (int miss = 0; miss < 2; ++miss)
                        for (int swaps = 0; swaps < 4; ++swaps)
                            for (int cap_delta = -1; cap_delta <= 1; ++cap_delta) { run_case(Case{n_old, n, members, keep, miss, swaps, cap_delta}); ++cases; }
            printf("%s merge %d %d (%d cases)\n", failures == before ? "ok" : "FAIL", n_old, n, cases);
        }
    check_meta();
    check_staging();
    if (failures) { printf("FAIL %d checks\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
