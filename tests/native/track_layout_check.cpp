// track_layout_check.cpp -- csrc/track_layout.h on the host, by itself (tests/test_track_layout_cpu.py builds it plain and with the
// address / undefined-behaviour sanitizers).  For the three trackers' state pools, max_tracks in {1, 5, 7, 255, 256, 2047} and
// n_streams in {1, 3}: the measuring pass returns exactly the offset at which the assigning pass ends, every array starts on a
// 16-byte boundary, no two arrays overlap (each array is also written over its whole extent in a buffer of exactly the measured
// size, so the sanitizer sees an overrun); the DeepSORT and OC-SORT sizes equal the formulas the library carried before the layout
// functions replaced them; and the Kalman read-back equals values worked out by hand.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "track_layout.h"

using namespace rtmodt;

// the state structs of csrc/kernels.h, field for field (float4 / float2 are HIP's 16- and 8-byte vectors)
struct float4 { float x, y, z, w; };
struct float2 { float x, y; };
static_assert(sizeof(float4) == 16 && sizeof(float2) == 8, "vector sizes");
constexpr int OC_RING = 8;
struct TrackerState {
    int64_t *ids[2]; float4 *box[2]; float *conf[2]; int32_t *cls[2]; int32_t *age[2]; int32_t *tsu[2];
    float4 *kf[2];
};
struct DsState {
    int64_t *ids[2]; float4 *dbox[2]; float *conf[2]; int32_t *cls[2];
    int32_t *flag[2], *hits[2], *age[2], *tsu[2];
    int32_t *slot[2], *gcount[2];
    float4 *kf[2];
    int32_t *slot_used;
};
struct OcState {
    int64_t *ids[2]; float4 *obox[2]; float *conf[2]; int32_t *cls[2];
    int32_t *hits[2], *streak[2], *age[2], *tsu[2];
    float2 *dir[2];
    float4 *kf[2], *saved[2];
    float4 *ring[2]; int32_t *ring_age[2];
};

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) { ++failures; printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

struct Span { const char *start; size_t bytes; };
struct Spans {
    std::vector<Span> v;
    template <typename T> void add(T *p, size_t count) { v.push_back(Span{(const char *)p, count * sizeof(T)}); }
};

static void spans_of(const TrackerState &st, size_t M, Spans &out) {
    for (int b = 0; b < 2; ++b) { out.add(st.ids[b], M); out.add(st.box[b], M); out.add(st.conf[b], M); out.add(st.cls[b], M); out.add(st.age[b], M); out.add(st.tsu[b], M); }
}
static void kf_spans_of(const TrackerState &st, size_t M, Spans &out) {
    for (int b = 0; b < 2; ++b) out.add(st.kf[b], 5 * M);
}
static void spans_of(const DsState &st, size_t M, Spans &out) {
    for (int b = 0; b < 2; ++b) {
        out.add(st.ids[b], M); out.add(st.dbox[b], M); out.add(st.conf[b], M); out.add(st.cls[b], M); out.add(st.flag[b], M); out.add(st.hits[b], M);
        out.add(st.age[b], M); out.add(st.tsu[b], M); out.add(st.slot[b], M); out.add(st.gcount[b], M); out.add(st.kf[b], 5 * M);
    }
    out.add(st.slot_used, M);
}
static void spans_of(const OcState &st, size_t M, Spans &out) {
    for (int b = 0; b < 2; ++b) {
        out.add(st.ids[b], M); out.add(st.obox[b], M); out.add(st.conf[b], M); out.add(st.cls[b], M); out.add(st.hits[b], M); out.add(st.streak[b], M);
        out.add(st.age[b], M); out.add(st.tsu[b], M); out.add(st.dir[b], M); out.add(st.kf[b], 5 * M); out.add(st.saved[b], 5 * M);
        out.add(st.ring[b], OC_RING * M); out.add(st.ring_age[b], OC_RING * M);
    }
}

// carve(states, base) -> size; spans(state, out) lists one stream's arrays.  Returns the measured size.
template <typename St, typename Carve, typename ListSpans>
static size_t check_layout(const char *name, size_t S, size_t M, size_t n_arrays, Carve carve, ListSpans spans) {
    std::vector<St> states(S);
    memset(states.data(), 0xff, sizeof(St) * S);
    const size_t measured = carve(states.data(), (char *)nullptr);
    EXPECT(measured > 0 && measured % 16 == 0, "%s S=%zu M=%zu: measured %zu", name, S, M, measured);
    char *base = nullptr;
    if (posix_memalign((void **)&base, 16, measured) != 0) { EXPECT(false, "allocation"); return measured; }
    const size_t end = carve(states.data(), base);
    EXPECT(end == measured, "%s S=%zu M=%zu: measuring pass %zu, assigning pass ends at %zu", name, S, M, measured, end);
    Spans sp;
    for (size_t s = 0; s < S; ++s) spans(states[s], sp);
    EXPECT(sp.v.size() == n_arrays * S, "%s: %zu arrays listed, %zu expected", name, sp.v.size(), n_arrays * S);
    for (const Span &a : sp.v) {
        EXPECT(a.start >= base && (size_t)(a.start - base) % 16 == 0, "%s S=%zu M=%zu: array at offset %td is not 16-byte aligned", name, S, M, a.start - base);
        memset((char *)a.start, 0x5a, a.bytes);                // an array past the pool's end is the sanitizer's to report
    }
    std::sort(sp.v.begin(), sp.v.end(), [](const Span &a, const Span &b) { return a.start < b.start; });
    for (size_t i = 0; i + 1 < sp.v.size(); ++i)
        EXPECT(sp.v[i].start + sp.v[i].bytes <= sp.v[i + 1].start, "%s S=%zu M=%zu: arrays at offsets %td and %td overlap", name, S, M, sp.v[i].start - base,
               sp.v[i + 1].start - base);
    EXPECT(sp.v.back().start + sp.v.back().bytes <= base + measured, "%s S=%zu M=%zu: the last array passes the pool's end", name, S, M);
    free(base);
    return measured;
}

static size_t a16(size_t v) { return (v + 15) / 16 * 16; }

static void check_kalman_unpack() {
    // Mc = 3, cnt = 2: block[row][track][lane] = 100 * row + 10 * track + lane; rows = mean, velocity, a, b, c
    const size_t Mc = 3;
    float block[5 * 3 * 4];
    for (int r = 0; r < 5; ++r)
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 4; ++k) block[(r * 3 + i) * 4 + k] = (float)(100 * r + 10 * i + k);
    const float want_mean[2][8] = {{0, 1, 2, 3, 100, 101, 102, 103}, {10, 11, 12, 13, 110, 111, 112, 113}};
    const float want_cov[2][12] = {{200, 300, 400, 201, 301, 401, 202, 302, 402, 203, 303, 403},
                                   {210, 310, 410, 211, 311, 411, 212, 312, 412, 213, 313, 413}};
    float mean[3 * 8], cov[3 * 12];
    for (float &v : mean) v = -1.f;
    for (float &v : cov) v = -1.f;
    kalman_unpack(block, Mc, 2, mean, cov);
    EXPECT(memcmp(mean, want_mean, sizeof(want_mean)) == 0, "kalman_unpack: mean");
    EXPECT(memcmp(cov, want_cov, sizeof(want_cov)) == 0, "kalman_unpack: cov");
    for (int k = 0; k < 8; ++k) EXPECT(mean[16 + k] == -1.f, "kalman_unpack wrote mean of track 2");
    for (int k = 0; k < 12; ++k) EXPECT(cov[24 + k] == -1.f, "kalman_unpack wrote cov of track 2");
    float mean2[2 * 8], cov2[2 * 12];
    kalman_unpack(block, Mc, 2, mean2, nullptr);
    kalman_unpack(block, Mc, 2, nullptr, cov2);
    EXPECT(memcmp(mean2, want_mean, sizeof(want_mean)) == 0 && memcmp(cov2, want_cov, sizeof(want_cov)) == 0, "kalman_unpack: one output at a time");
    kalman_unpack(block, Mc, 0, nullptr, nullptr);
}

int main() {
    const size_t Ms[] = {1, 5, 7, 255, 256, 2047}, Ss[] = {1, 3};
    for (size_t S : Ss)
        for (size_t M : Ms) {
            check_layout<TrackerState>("bytetrack", S, M, 12, [&](TrackerState *st, char *b) { return carve_bytetrack(st, S, M, b); },
                                       [&](const TrackerState &st, Spans &o) { spans_of(st, M, o); });
            check_layout<TrackerState>("bytetrack_kf", S, M, 2, [&](TrackerState *st, char *b) { return carve_bytetrack_kf(st, S, M, b); },
                                       [&](const TrackerState &st, Spans &o) { kf_spans_of(st, M, o); });
            const size_t ds = check_layout<DsState>("deepsort", S, M, 23, [&](DsState *st, char *b) { return carve_deepsort(st, S, M, b); },
                                                    [&](const DsState &st, Spans &o) { spans_of(st, M, o); });
            const size_t oc = check_layout<OcState>("ocsort", S, M, 26, [&](OcState *st, char *b) { return carve_ocsort(st, S, M, OC_RING, b); },
                                                    [&](const OcState &st, Spans &o) { spans_of(st, M, o); });
            // the size formulas ds_create_impl / oc_create_impl carried until the layout functions replaced them
            const size_t ds_per_buf = a16(M * 80) + a16(M * 16) + a16(M * 8) + 8 * a16(M * 4), ds_per_stream = ds_per_buf * 2 + a16(M * 4);
            EXPECT(ds == ds_per_stream * S, "deepsort S=%zu M=%zu: carved %zu, formula %zu", S, M, ds, ds_per_stream * S);
            const size_t oc_per_buf = 2 * a16(M * 80) + a16(M * 16 * OC_RING) + a16(M * 4 * OC_RING) + a16(M * 16) + 2 * a16(M * 8) + 6 * a16(M * 4);
            EXPECT(oc == oc_per_buf * 2 * S, "ocsort S=%zu M=%zu: carved %zu, formula %zu", S, M, oc, oc_per_buf * 2 * S);
            printf("ok layouts S=%zu M=%zu\n", S, M);
        }
    check_kalman_unpack();
    printf("ok kalman_unpack\n");
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
