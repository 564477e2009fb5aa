// wg_dev.h -- small device helpers of a wave or a workgroup, shared by zones.hip, crossing.hip, swapguard.hip, ocsort.hip, gmc.hip,
// crosscam.hip, speed.hip, snapshot.hip, privacy.hip, heatmap.hip, motion.hip, leftobj.hip, health.hip, enhance.hip, ccl_dev.h and track_ledger_dev.h.  Include inside
// namespace rtmodt.
#pragma once

// neither infinite nor NaN, read off the bits
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int lower_bound_i64(const int64_t *a, int n, int64_t x) {     // first index with a[i] >= x
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sum and maximum of a uint32 over the 64 lanes of a wave, in every lane
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// exclusive prefix of a per-thread count over a workgroup of WAVES waves (thread order); returns the position, writes the total.
// Two barriers.  wsum: LDS int[WAVES].  (A per-thread FLAG over the trackers' 1024 threads: block_scan_flag of track_dev.h.)
template <int WAVES> __device__ __forceinline__ int block_scan_count(int v, int *wsum, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int s = wsum[w];
        if (w < wave) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + incl - v;
}
