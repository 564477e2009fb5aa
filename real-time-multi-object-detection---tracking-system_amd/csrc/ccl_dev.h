// ccl_dev.h -- lock-free union-find for connected-component labelling on a grid of cells (leftobj.hip; motion.hip and stitch.hip
// still carry their own copies).  A parent array holds, for every cell that takes part, the index of a cell of the same component
// that is not larger than itself; a root is its own parent, so a component's root ends up as its smallest index: its first cell in
// raster order.  No lock and no spin on another workgroup: a lost compare-and-swap only means another hook landed first, and the
// loop continues from the new roots.  Loads and stores are relaxed agent-scope atomics; the labelling is complete at the end of the
// launch that links, and is read by later launches only.  Include inside namespace rtmodt.
#pragma once

__device__ __forceinline__ int ccl_ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ccl_st(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way
__device__ inline int ccl_find(int32_t *p, int x) {
    int c = ccl_ld(&p[x]);
    while (c != x) {                                        // parents only ever point at smaller cells: no cycle
        const int g = ccl_ld(&p[c]);
        if (g == c) return c;
        ccl_st(&p[x], g);                                   // any ancestor is a valid parent
        x = c;
        c = g;
    }
    return x;
}

// joins the components of x and y: the larger root is hooked under the smaller
__device__ inline void ccl_unite(int32_t *p, int x, int y) {
    while (true) {
        x = ccl_find(p, x);
        y = ccl_find(p, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }
        if (atomicCAS(&p[x], x, y) == x) return;
    }
}
