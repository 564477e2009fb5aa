// wg_dev.h -- small device helpers shared by the trackers and the ledger kernels (zones.hip, crossing.hip, swapguard.hip,
// ocsort.hip).  Include inside namespace rtmodt.
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
