// ccl_dev.h -- connected-component labelling by a lock-free union-find, and the steps that turn its roots into an ordered region list
// (motion.hip and leftobj.hip: all of it over a grid of cells; stitch.hip: the union-find over its rows and columns).  A parent array
// holds, for every cell that takes part, the index of a cell of the same component that is not larger than itself; a root is its own
// parent, so a component's root ends up as its smallest index: its first cell in raster order.  No lock and no spin on another
// workgroup: a lost compare-and-swap only means another hook landed first, and the loop continues from the new roots.  Loads and
// stores are relaxed agent-scope atomics; the labelling is complete at the end of the launch that links, and is read by later
// launches only.  Include inside namespace rtmodt, after wg_dev.h.
#pragma once

constexpr int CCL_CHUNK = 4096;                             // the cells one workgroup counts and ranks

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

// the link step of cell idx of a mask gw cells wide (8-connected): it looks at W, NW, N, NE and skips the links its neighbours make
__device__ __forceinline__ void ccl_link_cell(const uint8_t *mk, int32_t *par, int gw, long long idx) {
    if (!mk[idx]) return;
    const int cx = (int)(idx % gw), cy = (int)(idx / gw);
    const bool up = cy > 0;
    const bool W = cx > 0 && mk[idx - 1];
    const bool N = up && mk[idx - gw];
    const bool NW = up && cx > 0 && mk[idx - gw - 1];
    const bool NE = up && cx + 1 < gw && mk[idx - gw + 1];
    // N joins W, NW and NE already (N's own W link, NE's W link, W's link upwards); without N, W joins NW
    if (N) { ccl_unite(par, (int)idx, (int)(idx - gw)); return; }
    if (W) ccl_unite(par, (int)idx, (int)idx - 1);
    else if (NW) ccl_unite(par, (int)idx, (int)(idx - gw - 1));
    if (NE) ccl_unite(par, (int)idx, (int)(idx - gw + 1));
}

// What a wave of mask cells (m) with their roots adds at the roots: when all of them share one root, lane `lead` adds once for the n
// of them (the caller reduces its terms over the wave), else every cell adds for itself.  False for a wave without a mask cell.
// (wave-uniform)
struct CclWave { int lead; bool same; uint32_t n; };
__device__ __forceinline__ bool ccl_wave_roots(bool m, int root, CclWave &w) {
    const unsigned long long act = __ballot(m);
    if (!act) return false;
    w.lead = __ffsll((long long)act) - 1;
    const int root0 = __shfl(root, w.lead);
    w.same = __ballot(m && root != root0) == 0;
    w.n = (uint32_t)__popcll(act);
    return true;
}

// the regions (is_region(idx): a qualifying root) among the CCL_CHUNK cells of chunk blockIdx.x
template <int WAVES, typename P> __device__ __forceinline__ void ccl_count_chunk(uint32_t *ch, int *s_wcnt, P is_region) {
    const long long base = (long long)blockIdx.x * CCL_CHUNK;
    int mine = 0;
    for (int r = 0; r < CCL_CHUNK / (64 * WAVES); ++r) mine += is_region(base + r * (64 * WAVES) + threadIdx.x) ? 1 : 0;
    int total;
    block_scan_count<WAVES>(mine, s_wcnt, total);
    if (threadIdx.x == 0) ch[blockIdx.x] = (uint32_t)total;
}

// one workgroup: the exclusive scan of the n_chunks counts in place, their sum at ch[n_chunks]; returns the sum
template <int WAVES> __device__ __forceinline__ uint32_t ccl_scan_chunks(uint32_t *ch, int n_chunks, int *s_wcnt) {
    const int tid = threadIdx.x;
    uint32_t run = 0;
    for (int b = 0; b < n_chunks; b += 64 * WAVES) {
        const int i = b + tid;
        const int v = i < n_chunks ? (int)ch[i] : 0;
        int tot;
        const int pos = block_scan_count<WAVES>(v, s_wcnt, tot);
        if (i < n_chunks) ch[i] = run + (uint32_t)pos;
        run += (uint32_t)tot;
    }
    if (tid == 0) ch[n_chunks] = run;
    return run;
}

// a chunk that holds one of the first max_regions regions ranks its regions in raster order and calls write(idx, pos) for those with
// pos < max_regions
template <int WAVES, typename P, typename W>
__device__ __forceinline__ void ccl_emit_chunk(const uint32_t *ch, int max_regions, int *s_wcnt, P is_region, W write) {
    const uint32_t first = ch[blockIdx.x], n_here = ch[blockIdx.x + 1] - first;
    if (n_here == 0 || first >= (uint32_t)max_regions) return;         // (uniform)
    const long long base = (long long)blockIdx.x * CCL_CHUNK;
    uint32_t run = first;
    for (int r = 0; r < CCL_CHUNK / (64 * WAVES); ++r) {
        const long long idx = base + r * (64 * WAVES) + threadIdx.x;
        const bool f = is_region(idx);
        int tot;
        const uint32_t pos = run + (uint32_t)block_scan_count<WAVES>(f ? 1 : 0, s_wcnt, tot);
        if (f && pos < (uint32_t)max_regions) write(idx, pos);
        run += (uint32_t)tot;
    }
}
