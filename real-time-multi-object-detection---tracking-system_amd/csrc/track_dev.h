// track_dev.h -- device functions shared by the trackers (tracker.hip: ByteTrack, deepsort.hip: DeepSORT, ocsort.hip: OC-SORT, botsort.hip: BoT-SORT): the
// bit-exact IoU, the block-diagonal 8-state Kalman filter, the workgroup scan and the compaction built on it, the sparse
// exact assignment all use (assoc_sparse; include lap.h first), and OC-SORT's fixed-sequence acos.
// Include from a translation unit built with -ffp-contract=off and correctly rounded division (Makefile: EXACT), inside
// namespace rtmodt.
#pragma once

#pragma clang fp contract(off)

__device__ __forceinline__ float iou_ref(const float4 a, const float4 b) {
    float x1 = fmaxf(a.x, b.x), y1 = fmaxf(a.y, b.y);
    float x2 = fminf(a.z, b.z), y2 = fminf(a.w, b.w);
    float w = fmaxf(0.0f, x2 - x1), h = fmaxf(0.0f, y2 - y1);
    float inter = w * h;
    float area_a = (a.z - a.x) * (a.w - a.y);
    float area_b = (b.z - b.x) * (b.w - b.y);
    float uni = (area_a + area_b) - inter;
    return inter / (uni + 1e-6f);
}

// ---------------------------------------------------------------------------------------
// Opt-in Kalman motion model (TrackerArgs::kalman; oracle/kalman_oracle.py states the algorithm and its provenance:
// ByteTrack's published 8-state constant-velocity filter -- the reference itself has none, tracker.py:99-104).
// F, H, Q, R and the initial P keep P block-diagonal, so the filter is four independent (position, velocity) pairs
// with covariance [[a, b], [b, c]] whose only coupling is the noise scale h.  float32, one rounding per operation in
// exactly the oracle's order (this file is built with FMA contraction off and correctly rounded division).
// ---------------------------------------------------------------------------------------
struct Kf { float4 pos, vel, pa, pb, pc; };
constexpr float KF_WP = 0.05f, KF_WV = 0.00625f;
__device__ __forceinline__ Kf kf_load(const float4 *kf, int Mc, int i) { return Kf{kf[i], kf[Mc + i], kf[2 * Mc + i], kf[3 * Mc + i], kf[4 * Mc + i]}; }
__device__ __forceinline__ void kf_store(float4 *kf, int Mc, int i, const Kf &k) {
    kf[i] = k.pos; kf[Mc + i] = k.vel; kf[2 * Mc + i] = k.pa; kf[3 * Mc + i] = k.pb; kf[4 * Mc + i] = k.pc;
}
__device__ __forceinline__ float4 xyxy_to_xyah(const float4 b) {
    const float w = b.z - b.x, h = b.w - b.y;
    return float4{b.x + w * 0.5f, b.y + h * 0.5f, w / fmaxf(h, 1e-6f), h};
}
__device__ __forceinline__ float4 xyah_to_xyxy(const float4 m) {
    const float w = m.z * m.w;
    const float x1 = m.x - w * 0.5f, y1 = m.y - m.w * 0.5f;
    return float4{x1, y1, x1 + w, y1 + m.w};
}
__device__ __forceinline__ Kf kf_initiate(const float4 z) {
    const float sp = (2.0f * KF_WP) * z.w, sv = (10.0f * KF_WV) * z.w;
    const float p2 = sp * sp, v2 = sv * sv;
    Kf k;
    k.pos = z; k.vel = float4{0.f, 0.f, 0.f, 0.f};
    k.pa = float4{p2, p2, 1e-2f * 1e-2f, p2};
    k.pb = float4{0.f, 0.f, 0.f, 0.f};
    k.pc = float4{v2, v2, 1e-5f * 1e-5f, v2};
    return k;
}
__device__ __forceinline__ void kf_predict1(float &p, const float v, float &a, float &b, float &c, const float qp, const float qv) {
    const float a0 = a, b0 = b, c0 = c;
    p = p + v;
    a = ((a0 + (b0 + b0)) + c0) + qp;
    b = b0 + c0;
    c = c0 + qv;
}
__device__ __forceinline__ void kf_predict(Kf &k) {
    const float h = k.pos.w;
    const float sp = KF_WP * h, sv = KF_WV * h;
    const float qp = sp * sp, qv = sv * sv;
    kf_predict1(k.pos.x, k.vel.x, k.pa.x, k.pb.x, k.pc.x, qp, qv);
    kf_predict1(k.pos.y, k.vel.y, k.pa.y, k.pb.y, k.pc.y, qp, qv);
    kf_predict1(k.pos.z, k.vel.z, k.pa.z, k.pb.z, k.pc.z, 1e-2f * 1e-2f, 1e-5f * 1e-5f);
    kf_predict1(k.pos.w, k.vel.w, k.pa.w, k.pb.w, k.pc.w, qp, qv);
}
__device__ __forceinline__ void kf_update1(float &p, float &v, float &a, float &b, float &c, const float z, const float r) {
    const float a0 = a, b0 = b, c0 = c;
    const float s = a0 + r;
    const float k0 = a0 / s, k1 = b0 / s;
    const float y = z - p;
    p = p + k0 * y;
    v = v + k1 * y;
    a = a0 - k0 * a0;
    b = b0 - k0 * b0;
    c = c0 - k1 * b0;
}
__device__ __forceinline__ void kf_update(Kf &k, const float4 z) {
    const float sp = KF_WP * k.pos.w;
    const float r = sp * sp;
    kf_update1(k.pos.x, k.vel.x, k.pa.x, k.pb.x, k.pc.x, z.x, r);
    kf_update1(k.pos.y, k.vel.y, k.pa.y, k.pb.y, k.pc.y, z.y, r);
    kf_update1(k.pos.z, k.vel.z, k.pa.z, k.pb.z, k.pc.z, z.z, 1e-1f * 1e-1f);
    kf_update1(k.pos.w, k.vel.w, k.pa.w, k.pb.w, k.pc.w, z.w, r);
}

constexpr int TRK_THREADS = 1024;
constexpr int TRK_WAVES = TRK_THREADS / 64;

// exclusive prefix of a per-thread flag over the workgroup (thread order); returns position,
// writes the total.  Two barriers.  wsum: LDS int[TRK_WAVES + 1].
__device__ __forceinline__ int block_scan_flag(bool flag, int *wsum, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long m = __ballot(flag);
    int within = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TRK_WAVES; ++w) {
        int v = wsum[w];
        if (w < wave) off += v;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return off + within;
}

// compacts the indices i < n with flag(i) into list (ascending); returns their number.  Ends with a barrier.
template <typename F> __device__ __forceinline__ int block_compact(F flag, int n, int *list, int *wsum) {
    int cnt = 0;
    for (int base = 0; base < n; base += TRK_THREADS) {
        const int i = base + threadIdx.x;
        const bool f = i < n && flag(i);
        int tot;
        const int pos = block_scan_flag(f, wsum, tot);
        if (f) list[cnt + pos] = i;
        cnt += tot;
    }
    __syncthreads();
    return cnt;
}

// The exact maximum-gain matching of a sparse bipartite graph, for any cost type of lap.h (the comment at tracker.hip's assoc_lap
// states the method): edge(r, c, cost) tells whether the pair is admissible and gives its cost (< 0, minus the gain).  Pairs whose row
// and column both have degree 1 are matched outright; the contested remainder (<= LAP_ROWS / LAP_COLS / LAP_EDGES, else *err = 2) goes to
// lap_solve on one lane.  Afterwards row r is matched iff row_best[r] >= 0 && col_winner[row_best[r]] == r.  Needs lap.h.
template <typename C, typename F>
__device__ __forceinline__ void assoc_sparse(F edge, int n_rows, int n_cols, int *row_best, int *col_winner, int *rowcand, const LapSmemT<C> &L,
                                             int *wsum, int *err) {
    const int tid = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = tid; c < n_cols; c += TRK_THREADS) { col_winner[c] = 0; L.colmap[c] = -1; }
    __syncthreads();
    int R = 64;
    while (R > 1 && (n_rows * R > TRK_THREADS || (R >> 1) >= n_cols)) R >>= 1;
    const int groups = TRK_THREADS / R;
    const int gid = threadIdx.x / R, sub = threadIdx.x & (R - 1);
    for (int r = gid; r < n_rows; r += groups) {
        int deg = 0, last = -1;
        for (int c = sub; c < n_cols; c += R) {
            C cost;
            if (edge(r, c, cost)) { ++deg; last = c; atomicAdd(&col_winner[c], 1); }
        }
        for (int d = R >> 1; d >= 1; d >>= 1) {
            deg += __shfl_xor(deg, d);
            last = max(last, __shfl_xor(last, d));
        }
        if (sub == 0) { row_best[r] = deg; rowcand[r] = last; }
    }
    __syncthreads();
    int nhr = 0;
    for (int base = 0; base < n_rows; base += TRK_THREADS) {
        const int r = base + tid;
        bool hard = false;
        if (r < n_rows) {
            const int deg = row_best[r];
            hard = deg >= 2 || (deg == 1 && col_winner[rowcand[r]] != 1);
            if (deg != 1 || hard) rowcand[r] = -1;
        }
        int tot;
        const int pos = block_scan_flag(hard, wsum, tot);
        if (hard && nhr + pos < LAP_ROWS) L.hrow[nhr + pos] = r;
        nhr += tot;
    }
    bool dense = nhr > LAP_ROWS;
    if (dense) nhr = 0;
    __syncthreads();
    if (tid == 0) {
        int e = 0;
        for (int h = 0; h < nhr; ++h) { L.estart[h] = e; e += row_best[L.hrow[h]]; }
        L.estart[nhr] = e;
    }
    __syncthreads();
    int ne = L.estart[nhr];
    if (ne > LAP_EDGES) { dense = true; nhr = 0; ne = 0; }
    for (int h = wave; h < nhr; h += TRK_WAVES) {
        const int r = L.hrow[h];
        int e0 = L.estart[h];
        for (int cb = 0; cb < n_cols; cb += 64) {
            const int c = cb + lane;
            bool f = false;
            C cost = LapCost<C>::zero();
            if (c < n_cols) f = edge(r, c, cost);
            const unsigned long long m = __ballot(f);
            if (f) {
                const int e = e0 + __popcll(m & ((1ull << lane) - 1ull));
                L.ecol[e] = c;
                L.ecost[e] = cost;
                L.colmap[c] = -2;
            }
            e0 += __popcll(m);
        }
    }
    __syncthreads();
    int nhc = 0;
    for (int base = 0; base < n_cols; base += TRK_THREADS) {
        const int c = base + tid;
        const bool f = c < n_cols && L.colmap[c] == -2;
        int tot;
        const int pos = block_scan_flag(f, wsum, tot);
        if (f && nhc + pos < LAP_COLS) { L.colmap[c] = nhc + pos; L.hcol[nhc + pos] = c; }
        nhc += tot;
    }
    if (nhc > LAP_COLS) { dense = true; nhr = 0; ne = 0; nhc = 0; }
    __syncthreads();
    for (int e = tid; e < ne; e += TRK_THREADS) L.ecol[e] = L.colmap[L.ecol[e]];
    for (int h = tid; h < nhr; h += TRK_THREADS) { L.u[h] = LapCost<C>::zero(); L.rm[h] = -1; }
    for (int j = tid; j < nhc; j += TRK_THREADS) { L.v[j] = LapCost<C>::zero(); L.minv[j] = LapCost<C>::inf(); L.p[j] = -1; L.used[j] = 0; }
    for (int c = tid; c < n_cols; c += TRK_THREADS) col_winner[c] = INT_MAX;
    __syncthreads();
    for (int r = tid; r < n_rows; r += TRK_THREADS) {
        const int c = rowcand[r];
        row_best[r] = c;
        if (c >= 0) col_winner[c] = r;
    }
    __syncthreads();
    if (tid == 0) {
        if (dense) *err = 2;
        lap_solve(L, nhr);
        for (int h = 0; h < nhr; ++h)
            if (L.rm[h] >= 0) {
                const int r = L.hrow[h], c = L.hcol[L.rm[h]];
                row_best[r] = c;
                col_winner[c] = r;
            }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------
// acos of a float32 in [-1, 1] as a fixed sequence of float64 additions, multiplications and divisions -- each correctly rounded,
// none contracted (fp contract off) -- so that the value is the same wherever it is built: no libm call, no float64 square root.
// tests/ocsort_ref.py (acos_fixed) restates it operation for operation; its largest error against libm's acos is recorded in
// DESIGN.md section 21.  asin(x) = x + x * z * P(z), z = x * x, P = the Taylor coefficients (2k)! / (4^k k!^2 (2k + 1)), k = 1..22.
//   |x| <= 0.5   pi/2 - asin(x)
//   |x| >  0.5   t = (1 - |x|) * 0.5 (exact), s = sqrt(t) by two Newton steps y = 0.5 * (y + t / y) from the correctly rounded
//                float32 square root of float32(t); 2 * asin(s), reflected to pi - that for x < 0
// ---------------------------------------------------------------------------------------
constexpr double ACOS_PI = 0x1.921fb54442d18p+1, ACOS_HALF_PI = 0x1.921fb54442d18p+0;
__device__ __forceinline__ double asin_poly(const double z) {
    constexpr double C[22] = {0x1.5555555555555p-3, 0x1.3333333333333p-4, 0x1.6db6db6db6db7p-5, 0x1.f1c71c71c71c7p-6, 0x1.6e8ba2e8ba2e9p-6,
                              0x1.1c4ec4ec4ec4fp-6, 0x1.c99999999999ap-7, 0x1.7a87878787878p-7, 0x1.3fde50d79435ep-7, 0x1.12ef3cf3cf3cfp-7,
                              0x1.df3bd37a6f4dfp-8, 0x1.a6863d70a3d71p-8, 0x1.782dda12f684cp-8, 0x1.51ba308d3dcb1p-8, 0x1.31683bdef7bdfp-8,
                              0x1.15ee9d45d1746p-8, 0x1.fcaf8fb6db6dbp-9, 0x1.d3d2a8e0dd67dp-9, 0x1.b026f57b13b14p-9, 0x1.90cb77f60c7cep-9,
                              0x1.750de64d7d05fp-9, 0x1.5c5f56efaaaabp-9};
    double p = C[21];
#pragma unroll
    for (int k = 20; k >= 0; --k) p = C[k] + z * p;
    return p;
}
__device__ __forceinline__ double acos_fixed(const float c) {
    const double x = (double)c;
    const double a = x < 0.0 ? -x : x;
    if (a <= 0.5) {
        const double z = x * x;
        return ACOS_HALF_PI - (x + x * (z * asin_poly(z)));
    }
    const double t = (1.0 - a) * 0.5;
    double s = 0.0;
    if (t != 0.0) {
        double y = (double)__builtin_sqrtf((float)t);
        y = 0.5 * (y + t / y);
        y = 0.5 * (y + t / y);
        s = y;
    }
    const double r = s + s * (t * asin_poly(t));
    const double ac = 2.0 * r;
    return x < 0.0 ? ACOS_PI - ac : ac;
}
