// The union-find of svr_components (include/svr.h; kernels: components_kernels.hip) over one array `parent` of u32, an
// entry per voxel of the box, indexed densely in (z, y, x) order.  The same text runs in the merge kernel and, with the
// atomics mapped to the host's __atomic builtins, in a test that compiles it without HIP (tests/test_components.py).
//
// The rules, which keep a launch from hanging whatever the other workgroups do:
//   * parent[i] <= i always; parent[i] == i marks a root; kUfOutside marks a voxel that is outside and never changes.
//   * After the init pass the only writes are atomic minima (relaxed, agent scope): an entry never grows.
//   * Every read in the merge pass is a relaxed agent-scope atomic load: the L1 of a CU is not refreshed by the atomics
//     of other CUs, and such a load is served by L2, where the atomics execute.
//   * A stale value is still an ancestor of the voxel in the same set, so uf_find walks strictly downward and ends
//     after at most i steps.
//   * uf_union retries only when the atomic minimum returned something other than the root it assumed, and goes on from
//     that returned value: the larger of its two indices shrinks with every retry, so it ends too.
// No thread ever waits for another one.
// svr_split keeps its summits in such an array too (split_kernels.hip); the flatten kernel at the end is the pass that
// follows the unions in both chains.
#pragma once

#include <stdint.h>

#include "components_plan.h"

constexpr uint32_t kUfOutside = 0xFFFFFFFFu;

#ifdef __HIPCC__
#define UF_FN __host__ __device__ __forceinline__
#else
#define UF_FN inline
#endif

UF_FN uint32_t uf_load(const uint32_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
// the atomic minimum; returns what the entry held before
UF_FN uint32_t uf_min(uint32_t* p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
#endif
}

// the root of i's set as far as this thread can see it: some ancestor r with parent[r] == r at the time it was read
UF_FN uint32_t uf_find(const uint32_t* parent, uint32_t i) {
    for (;;) {
        const uint32_t p = uf_load(parent + i);
        if (p == i) return i;
        i = p;                                              // p < i
    }
}

// joins the sets of a and b (both inside)
UF_FN void uf_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = uf_min(parent + hi, lo);
        if (old == hi) return;                              // hi was the root it looked like: linked
        // hi had been linked below already (old < hi), and now hangs under min(old, lo): what is left is to join those two
        a = old; b = lo;
    }
}

// i and j connect if j is inside and, where labels split components (KEYED: aux holds the label of every inside voxel),
// carries i's label
template <bool KEYED>
UF_FN bool uf_connects(const uint32_t* parent, const uint32_t* aux, uint32_t key, uint32_t j) {
    if (uf_load(parent + j) == kUfOutside) return false;
    return !KEYED || aux[j] == key;
}

// What the merge pass does for voxel i = (rz n[1] + ry) n[0] + rx of the box: joins it with the neighbours that come
// before it in (z, y, x) order, 3 under 6-connectivity and 13 under 26 (CONN26), so that every connecting pair is
// joined by its later voxel.  Unions that others make are left out: that with rx - 1 where the init pass linked the two
// (comp_x_implied), and under 26-connectivity those with the two x neighbours of a voxel this one is joined with, which
// connect with that voxel wherever they connect with this one.
template <bool CONN26, bool KEYED>
UF_FN void uf_merge_voxel(uint32_t* parent, const uint32_t* aux, uint32_t i, const uint32_t n[3], uint32_t head) {
    if (uf_load(parent + i) == kUfOutside) return;
    const uint32_t rx = i % n[0], row = i / n[0], ry = row % n[1], rz = row / n[1];
    const uint32_t key = KEYED ? aux[i] : 0u;
    if (rx > 0u && !comp_x_implied(rx, head) && uf_connects<KEYED>(parent, aux, key, i - 1u)) uf_union(parent, i, i - 1u);
    // the rows of neighbours before this voxel's own: (dy, dz) = (-1, 0), then dz = -1 with dy = -1, 0, 1
    for (int r = 0; r < (CONN26 ? 4 : 2); ++r) {
        const int dy = CONN26 ? (r == 0 ? -1 : r - 2) : (r == 0 ? -1 : 0), dz = r == 0 ? 0 : -1;
        const uint32_t qy = ry + (uint32_t)dy, qz = rz + (uint32_t)dz;      // before the box: wraps to a huge value
        if (qy >= n[1] || qz >= n[2]) continue;
        const uint32_t j = (qz * n[1] + qy) * n[0] + rx;
        if (uf_connects<KEYED>(parent, aux, key, j)) { uf_union(parent, i, j); continue; }
        if (!CONN26) continue;
        if (rx > 0u && uf_connects<KEYED>(parent, aux, key, j - 1u)) uf_union(parent, i, j - 1u);
        if (rx + 1u < n[0] && uf_connects<KEYED>(parent, aux, key, j + 1u)) uf_union(parent, i, j + 1u);
    }
}

#ifdef __HIPCC__
// The flatten pass, a thread per entry: parent[i] = root(i), and into cnt[workgroup] the number of roots among the
// workgroup's kBoxScanBlock entries: level 0 of the scan (box_scan.h).  static: no template, and in two units.
static __global__ __launch_bounds__(kBoxScanBlock) void uf_flatten_kernel(uint32_t* parent, uint32_t voxels, uint32_t* cnt) {
    __shared__ uint32_t part[kBoxScanWaves];
    const uint32_t i = blockIdx.x * kBoxScanBlock + threadIdx.x;
    uint32_t is_root = 0u;
    if (i < voxels) {
        const uint32_t p = uf_load(parent + i);
        if (p != kUfOutside) {
            const uint32_t r = uf_find(parent, p);
            if (r != p) (void)uf_min(parent + i, r);
            is_root = r == i;
        }
    }
    const uint32_t total = box_block_sum(is_root, part);
    if (threadIdx.x == 0u) cnt[blockIdx.x] = total;
}
#endif
