// crosscam_rule.h -- the one statement of the cross-camera linker's per-pair and per-row arithmetic: the similarity of a query row
// and an identity's feature, when a (query, identity) pair may be linked, and the smoothed feature of an identity
// (csrc/crosscam.hip keeps the table and the ledgers and runs the matching; its header states the per-call rules).  Plain C++, no
// HIP: the kernels of crosscam.hip, its host entry points and tests/native/crosscam_rule_check.cpp (built under the address and
// UB sanitizers) all take it from here, and tests/crosscam_ref.py restates it.  Integer arithmetic throughout.
//   similarity     dot = <q, s8> (int32), nq / ng the squared norms (int64); sim = dot <= 0 ? 0 :
//                  min(1000, 1000 dot / max(1, isqrt(nq ng))), floor division.  nq ng <= (512 128^2)^2 < 2^63.
//   transit        a sighting of the identity in stream f at call l admits stream s at call c iff l > 0 and
//                  tmin[f][s] <= c - l <= tmax[f][s].
//   feature        BoT-SORT's integer EMA: v = 9 s16 + 128 f (128 f at birth), r = isqrt(sum v^2),
//                  s16 = sign(v) ((16256 |v| + r / 2) / r), s8 = sign(v) min(127, (127 |v| + r / 2) / r); r == 0: zeros.
#pragma once

#include <cstdint>

#ifndef CC_HD
#define CC_HD
#endif

namespace rtmodt {

constexpr int CC_MAX_STREAMS = 64, CC_MAX_DIM = 512, CC_MAX_TRACKS = 256, CC_MAX_IDENTITIES = 4096, CC_MAX_QUERIES = 1024;
constexpr int CC_FEAT_NORM = 16256;                        // 127 * 128: the int16 feature's norm
// the status of an entry after a call
constexpr int CC_NONE = 0, CC_BOUND = 1, CC_LINKED = 2, CC_JOINED = 3, CC_BORN = 4, CC_NO_DESCRIPTOR = 5, CC_DEFERRED = 6, CC_TABLE_FULL = 7,
              CC_UNBOUND = 8;

// exact floor(sqrt(n)), n >= 0 (kernels.h: isqrt64, restated so that this header stands alone)
CC_HD inline long long cc_isqrt(long long n) {
    unsigned long long x = (unsigned long long)n, r = 0, bit = 1ull << 62;
    while (bit > x) bit >>= 2;
    while (bit) {
        if (x >= r + bit) { x -= r + bit; r = (r >> 1) + bit; }
        else r >>= 1;
        bit >>= 2;
    }
    return (long long)r;
}

CC_HD inline int32_t cc_sim(int32_t dot, long long nq, long long ng) {
    if (dot <= 0) return 0;
    long long den = cc_isqrt(nq * ng);
    if (den < 1) den = 1;
    const long long v = 1000ll * dot / den;
    return (int32_t)(v > 1000 ? 1000 : v);
}

CC_HD inline bool cc_transit_ok(long long c, long long last, int32_t tmin, int32_t tmax) {
    return last > 0 && c - last >= tmin && c - last <= tmax;
}

// one element of the feature step: v = 9 s16 + 128 f, or 128 f at birth
CC_HD inline int32_t cc_feat_mix(bool birth, int32_t s16, int32_t f) { return birth ? 128 * f : 9 * s16 + 128 * f; }
// ... and its two roundings, given r = isqrt(sum v^2) > 0
CC_HD inline int16_t cc_feat_s16(int32_t v, long long r) {
    const long long a = v < 0 ? -(long long)v : v;
    const long long q = (CC_FEAT_NORM * a + r / 2) / r;
    return (int16_t)(v < 0 ? -q : q);
}
CC_HD inline int8_t cc_feat_s8(int32_t v, long long r) {
    const long long a = v < 0 ? -(long long)v : v;
    long long q = (127 * a + r / 2) / r;
    if (q > 127) q = 127;
    return (int8_t)(v < 0 ? -q : q);
}

// the whole step on one row, for the host and the native check (the kernel spreads the same elements over a wave)
inline void cc_feat_step(bool birth, int16_t *s16, int8_t *s8, const int8_t *f, int dim) {
    int32_t v[CC_MAX_DIM];
    long long n2 = 0;
    for (int k = 0; k < dim; ++k) {
        v[k] = cc_feat_mix(birth, s16[k], f[k]);
        n2 += (long long)v[k] * v[k];
    }
    const long long r = cc_isqrt(n2);
    for (int k = 0; k < dim; ++k) {
        s16[k] = r ? cc_feat_s16(v[k], r) : (int16_t)0;
        s8[k] = r ? cc_feat_s8(v[k], r) : (int8_t)0;
    }
}

}  // namespace rtmodt
