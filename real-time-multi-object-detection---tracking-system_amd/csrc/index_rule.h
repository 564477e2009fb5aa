// index_rule.h -- the one statement of the appearance index's arithmetic: where a row lives in the ring, the similarity of a query
// and a row in parts per million, when a row is eligible for a query, the rank that orders the hits, and how an archive is cut
// into chunks (csrc/index.hip keeps the ring and runs the scan and the merge; include/rtmodt.h states the per-call rules).  Plain
// C++, no HIP: the kernels of index.hip, its host entry points and tests/native/index_rule_check.cpp (built under the address
// and UB sanitizers) all take it from here, and tests/index_ref.py restates it.  Integer arithmetic throughout.
//   slot           row rid (from 1, never reused, below 2^40) lives in slot (rid - 1) % capacity; a newer row overwrites the oldest.
//   similarity     dot = <q, row> (int32), nq / n2 the squared norms; ppm = dot <= 0 ? 0 :
//                  min(1000000, 1000000 dot / max(1, isqrt(nq n2))), floor division, the root by cc_isqrt of crosscam_rule.h:
//                  ppm / 1000 == cc_sim(dot, nq, n2).  nq n2 <= (512 128^2)^2 = 2^46 and 10^6 dot <= 10^6 2^23 < 2^63.
//   eligibility    the slot is filled and the row not dead; t0 <= t <= t1; bit `stream` of stream_mask; cls_q < 0 or cls == cls_q;
//                  key != exclude_key (INT64_MIN: none); ppm >= min_ppm >= 1 (so a zero row, ppm 0, never is).
//   rank           ppm << 40 | rid, descending: the best similarity first, the newest row first on a tie; ranks are distinct.
//   chunks         at most 256 of chunk_rows rows, chunk_rows a multiple of 64 (0: the smallest that keeps to 256 chunks).
#pragma once

#include <cstdint>

#include "crosscam_rule.h"

namespace rtmodt {

constexpr int IX_MAX_CAPACITY = 1 << 22, IX_MAX_QUERIES = 64, IX_MAX_K = 64, IX_MAX_ADD = 65536, IX_MAX_FORGET = 4096, IX_MAX_CHUNKS = 256;
constexpr int IX_MAX_STREAMS = 64, IX_PPM = 1000000, IX_RID_BITS = 40;
constexpr int64_t IX_NO_KEY = INT64_MIN, IX_MAX_RID = (int64_t)1 << IX_RID_BITS;

CC_HD inline int64_t ix_slot(int64_t rid, int64_t capacity) { return (rid - 1) % capacity; }

// the rid a slot holds when the next row will get next_rid; 0: the slot is empty
CC_HD inline int64_t ix_slot_rid(int64_t slot, int64_t capacity, int64_t next_rid) {
    const int64_t newest = next_rid - 1;                   // rids newest - capacity + 1 .. newest are in the ring
    if (newest < 1) return 0;
    const int64_t r = newest - (ix_slot(newest, capacity) - slot + capacity) % capacity;
    return r >= 1 ? r : 0;
}

CC_HD inline int32_t ix_ppm(int32_t dot, long long nq, long long n2) {
    if (dot <= 0) return 0;
    long long den = cc_isqrt(nq * n2);
    if (den < 1) den = 1;
    const long long v = (long long)IX_PPM * dot / den;
    return (int32_t)(v > IX_PPM ? IX_PPM : v);
}

// everything of the eligibility that needs no similarity
CC_HD inline bool ix_row_ok(int64_t rid, int32_t dead, int64_t t, int32_t stream, int32_t cls, int64_t key, int64_t t0, int64_t t1,
                            uint64_t stream_mask, int32_t cls_q, int64_t exclude_key) {
    if (rid <= 0 || dead) return false;
    if (t < t0 || t > t1) return false;
    if (stream < 0 || stream >= IX_MAX_STREAMS || !(stream_mask >> stream & 1)) return false;
    if (cls_q >= 0 && cls != cls_q) return false;
    return exclude_key == IX_NO_KEY || key != exclude_key;
}

CC_HD inline uint64_t ix_rank(int32_t ppm, int64_t rid) { return (uint64_t)ppm << IX_RID_BITS | (uint64_t)rid; }
CC_HD inline int32_t ix_rank_ppm(uint64_t rank) { return (int32_t)(rank >> IX_RID_BITS); }
CC_HD inline int64_t ix_rank_rid(uint64_t rank) { return (int64_t)(rank & (((uint64_t)1 << IX_RID_BITS) - 1)); }

// the rows of a chunk for an archive of `capacity` slots; requested 0: chosen here.  0: the request is not allowed
inline int ix_chunk_rows(int capacity, int requested) {
    if (capacity < 1 || capacity > IX_MAX_CAPACITY || requested < 0) return 0;
    if (requested == 0) {
        const int per = (capacity + IX_MAX_CHUNKS - 1) / IX_MAX_CHUNKS;
        return (per + 63) / 64 * 64;
    }
    if (requested % 64 != 0 || (capacity + requested - 1) / requested > IX_MAX_CHUNKS) return 0;
    return requested;
}

// `rank` into best[0 .. n), kept descending and at most k long (the host's and the native check's selection; the kernels sort)
inline void ix_topk_insert(uint64_t *best, int &n, int k, uint64_t rank) {
    if (n == k && rank <= best[k - 1]) return;
    int i = n < k ? n++ : k - 1;
    for (; i > 0 && best[i - 1] < rank; --i) best[i] = best[i - 1];
    best[i] = rank;
}

}  // namespace rtmodt
