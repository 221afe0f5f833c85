// The back end that the chains of svr_mesh, svr_components and svr_split share (mesh_kernels.hip, components_kernels.hip,
// split_kernels.hip): number what a pass has counted, then gather each wave's shares of a record.
//
// The scan.  An exclusive prefix, in place, over count[0] entries of the scratch, kBoxScanBlock of them to a workgroup:
// level k + 1 holds the sums of level k's blocks, until one block holds a whole level.  box_scan_run launches the sums
// level by level going up, one workgroup over the top level, which also hands the total to the pass's functor (it writes
// the header), then each level adds its block's prefix on the way down.  Workgroups never wait for one another inside a
// launch.  An entry is a u32 (components, split) or two of them (the mesh: active cells, crossing edges).
//
// The record reduction.  box_wave_groups: the lanes of a wave that carry the same id reduce their shares of that id's
// record with shuffles, and the body runs once per id, on one lane: an id that fills the wave costs one set of atomics
// per wave, not 64.
//
// The host half is plain C++ on plain integers, which the plan headers include and the tests compile without HIP; the
// device half (under __HIPCC__) holds the kernels, as templates that each unit instantiates with its entry type and functor.
#pragma once

#include <stdint.h>

constexpr uint32_t kBoxScanBlock = 256;           // entries one workgroup scans: one per thread
constexpr int      kBoxScanMaxLevels = 4;         // 2^28 entries -> 2^20 -> 2^12 -> 2^4; 2^22 (2^30 voxels) need three

struct BoxScanPlan {
    int32_t  levels;                              // arrays of the scan, 1 .. kBoxScanMaxLevels
    uint32_t count[kBoxScanMaxLevels];            // entries of level k; count[levels - 1] <= kBoxScanBlock; 0 from `levels` on
    uint64_t off[kBoxScanMaxLevels];              // byte offsets into the scratch; a level that is not used takes no bytes
};

// The levels of a prefix scan over count0 entries, `block` of them to a workgroup -> their number: count[0] = count0,
// count[k + 1] the blocks of level k, until one block holds a level (within max_levels by the caller's limit on count0)
inline int box_scan_levels(uint32_t count0, uint32_t block, int max_levels, uint32_t count[]) {
    int levels = 1;
    count[0] = count0;
    for (int k = 1; k < max_levels; ++k) count[k] = 0;
    for (; count[levels - 1] > block; ++levels) count[levels] = (count[levels - 1] + block - 1u) / block;
    return levels;
}

// The scan over count0 (<= 2^28) entries of entry_bytes each, its levels one behind the other from byte `at` of the
// scratch -> the first byte behind them
inline uint64_t box_scan_plan(uint32_t count0, uint32_t entry_bytes, uint64_t at, BoxScanPlan& s) {
    s.levels = box_scan_levels(count0, kBoxScanBlock, kBoxScanMaxLevels, s.count);
    for (int k = 0; k < kBoxScanMaxLevels; ++k) {
        s.off[k] = at;
        at += (uint64_t)s.count[k] * entry_bytes;
    }
    return at;
}

#ifdef __HIPCC__

constexpr int kBoxScanWaves = (int)kBoxScanBlock / 64;

__device__ __forceinline__ uint32_t box_shfl_xor(uint32_t v, int d) { return (uint32_t)__shfl_xor((int)v, d); }
__device__ __forceinline__ uint2 box_shfl_xor(uint2 v, int d) { return make_uint2(box_shfl_xor(v.x, d), box_shfl_xor(v.y, d)); }
__device__ __forceinline__ uint32_t box_shfl_up(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d); }
__device__ __forceinline__ uint2 box_shfl_up(uint2 v, int d) { return make_uint2(box_shfl_up(v.x, d), box_shfl_up(v.y, d)); }

// the sum of v over the workgroup (kBoxScanBlock threads), in every thread; part: kBoxScanWaves entries of LDS
template <typename V>
__device__ __forceinline__ V box_block_sum(V v, V* part) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += box_shfl_xor(v, d);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
    __syncthreads();
    V s = part[0];
#pragma unroll
    for (int k = 1; k < kBoxScanWaves; ++k) s += part[k];
    return s;
}

// the sum of v over the threads of the workgroup before this one
template <typename V>
__device__ __forceinline__ V box_block_exclusive(V v, V* part) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    V inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V p = box_shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += p;
    }
    if (lane == 63u) part[wave] = inc;
    __syncthreads();
    V before = inc - v;
    for (uint32_t k = 0; k < wave; ++k) before += part[k];
    return before;
}

// out[b] = the sum of block b's kBoxScanBlock entries of in[0 .. n)
template <typename V>
__global__ __launch_bounds__(kBoxScanBlock) void box_scan_sums_kernel(const V* in, uint32_t n, V* out) {
    __shared__ V part[kBoxScanWaves];
    const uint32_t i = blockIdx.x * kBoxScanBlock + threadIdx.x;
    const V total = box_block_sum(i < n ? in[i] : V(), part);
    if (threadIdx.x == 0u) out[blockIdx.x] = total;
}

// data[0 .. n): every block's entries become their exclusive prefix inside the block plus base[block] (null: 0).  On the
// top level (`is_top`: one block holds it all; n may be 0) the last thread calls top(total).
template <typename V, class Top>
__global__ __launch_bounds__(kBoxScanBlock) void box_scan_apply_kernel(V* data, uint32_t n, const V* base, int is_top, const Top top) {
    __shared__ V part[kBoxScanWaves];
    const uint32_t i = blockIdx.x * kBoxScanBlock + threadIdx.x;
    const V v = i < n ? data[i] : V();
    V before = box_block_exclusive(v, part);
    if (base) before += base[blockIdx.x];
    if (i < n) data[i] = before;
    if (is_top && threadIdx.x == kBoxScanBlock - 1u) top(before + v);
}

// The whole chain on a stream.  s: the plan of the scan, its levels at scratch + s->off[]; null: no entry at all, the top
// level alone runs, over nothing, for its call of top(0).
template <typename V, class Top>
hipError_t box_scan_run(const BoxScanPlan* s, void* scratch, const Top& top, hipStream_t stream) {
    const dim3 block(kBoxScanBlock);
    hipError_t e;
    if (!s) {
        hipLaunchKernelGGL((box_scan_apply_kernel<V, Top>), dim3(1), block, 0, stream, (V*)nullptr, 0u, (const V*)nullptr, 1, top);
        return hipGetLastError();
    }
    V* lev[kBoxScanMaxLevels];
    for (int k = 0; k < s->levels; ++k) lev[k] = reinterpret_cast<V*>(static_cast<char*>(scratch) + s->off[k]);
    for (int k = 0; k + 1 < s->levels; ++k) {
        hipLaunchKernelGGL((box_scan_sums_kernel<V>), dim3(s->count[k + 1]), block, 0, stream, (const V*)lev[k], s->count[k], lev[k + 1]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int t = s->levels - 1;
    hipLaunchKernelGGL((box_scan_apply_kernel<V, Top>), dim3(1), block, 0, stream, lev[t], s->count[t], (const V*)nullptr, 1, top);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (int k = t - 1; k >= 0; --k) {
        hipLaunchKernelGGL((box_scan_apply_kernel<V, Top>), dim3(s->count[k + 1]), block, 0, stream, lev[k], s->count[k], (const V*)lev[k + 1], 0, top);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// What the lanes of a wave that share an id add up to, per axis of their coordinates
struct BoxShare {
    uint32_t count;                               // the lanes
    uint32_t cmin[3], cmax[3];
    unsigned long long sum[3];
    unsigned long long best, tops;                // KEYED: the largest key, and the ballot of the lanes whose key is not 0
};

// Every lane of the wave calls this: id 0, no record; else c, its coordinates, and with KEYED a key (0: none).  A round
// per id that has lanes left: body(id, share) runs on the first of them.  Wave-uniform control flow throughout.
template <bool KEYED, class Body>
__device__ __forceinline__ void box_wave_groups(uint32_t id, const uint32_t c[3], unsigned long long key, Body&& body) {
    unsigned long long todo = __ballot(id != 0u);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lid = (uint32_t)__shfl((int)id, leader);
        const bool mine = id == lid;
        const unsigned long long peers = __ballot(mine);
        BoxShare s;
        s.tops = 0ull; s.best = 0ull;
        if constexpr (KEYED) { s.tops = __ballot(mine && key != 0ull); s.best = mine ? key : 0ull; }
        todo &= ~peers;
        s.count = (uint32_t)__popcll(peers);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            s.cmin[ax] = mine ? c[ax] : 0xFFFFFFFFu; s.cmax[ax] = mine ? c[ax] : 0u;
            s.sum[ax] = mine ? (unsigned long long)c[ax] : 0ull;
        }
        if (s.count > 1u) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    s.cmin[ax] = min(s.cmin[ax], (uint32_t)__shfl_xor((int)s.cmin[ax], d));
                    s.cmax[ax] = max(s.cmax[ax], (uint32_t)__shfl_xor((int)s.cmax[ax], d));
                    s.sum[ax] += __shfl_xor(s.sum[ax], d);
                }
                if constexpr (KEYED) {
                    const unsigned long long other = __shfl_xor(s.best, d);
                    s.best = other > s.best ? other : s.best;
                }
            }
        }
        if ((int)__lane_id() == leader) body(lid, s);
    }
}

#endif  // __HIPCC__
