// The watershed of a height field (svr_split, include/svr.h): every positive voxel climbs to its summit, neighbouring
// basins link where the lower peak stands less than sqrt(merge_squared) above their pass, and the classes of the links
// are the regions, numbered by their smallest summits.  A dense volume of numbers and one record per region.  gfx950.
//
// The chain (layout of the scratch: split_plan.h; the order and the link test: split_link.h), every kernel a plain
// launch on the caller's stream, a thread per voxel with consecutive lanes on consecutive x; no workgroup waits for
// another inside a launch and nothing spins on a flag:
//   up       up[i] = the voxel that beats all others among i and its 6 or 26 neighbours in the box (a 64-bit maximum
//            over split_key), kSplitOutside where height[i] <= 0.  A voxel that is its own up is a summit and starts
//            as its own root in uf; every other entry of uf is kSplitOutside for good.  Counts the inside voxels and
//            the summits, one atomic each per wave.
//   summit   up[i] = summit(i).  WHY THE WALK ENDS: up(j) beats j unless j is a summit, and the order is strict and
//            total, so a chain never returns to a voxel and ends after fewer steps than there are voxels.  The walk
//            runs in place, beside the stores of other threads: what it reads at up[j] is up(j) or already summit(j).
//            Both lie on j's chain, both beat j unless j is the summit, and the chain of either ends in summit(j): the
//            end point does not depend on what the other threads have stored so far.  Those loads and stores are
//            relaxed agent-scope atomics (whole words, and served by L2).
//   link     a thread per voxel tests the neighbours before it in (z, y, x) order, 3 or 13, as uf_merge_voxel does, so
//            every neighbouring pair is seen once, by its later voxel; where the summits differ and split_links holds
//            it joins the two summits with uf_union (components_uf.h, unchanged).  That file's rule parent[i] <= i
//            holds among summits because a union hangs the larger index under the smaller; its rule on relaxed
//            agent-scope atomic loads holds because this kernel reads uf through uf_union alone.  The test reads
//            height and up only, which no thread writes here: which pair of two basins comes first does not matter.
//   flatten  uf[S] = root(S), the smallest summit of S's region: its seed; and the number of seeds among each
//            workgroup's voxels: level 0 of the scan (components_uf.h: uf_flatten_kernel, on uf).
//   scan     an exclusive prefix of those counts in place: the scan of box_scan.h on u32, whose top level writes the
//            header (SplitHeader).
//   rank     the number of seeds before a seed is its region's number minus one: into aux[seed]; and, when the records
//            fit, the seed starts its record.
//   emit     ids[i] = aux[uf[up[i]]] + 1, and the voxel's share of its record.  The lanes of a wave that belong to one
//            region reduce their shares with shuffles first (box_scan.h: box_wave_groups).  A summit adds 1 to basins and
//            offers split_key(height, index) to a 64-bit atomic maximum kept in the record's top[0..1].
//   finish   a thread per record unpacks that maximum into top[3] and peak.
// The count-only call ends behind the scan.  uf is written by the up pass and by atomic minima alone; every other store
// is an ordinary vector store or, in the summit pass, a relaxed atomic store.
#include <limits.h>
#include <stddef.h>

#include "svr_host.h"
#include "split_plan.h"
#include "split_link.h"
#include "components_uf.h"
#include "box_scan.h"

namespace {

constexpr int kSplitThreads = 256;
static_assert(kBoxScanBlock == (uint32_t)kSplitThreads, "one entry, and one voxel, per thread");
static_assert(kSplitOutside == kUfOutside, "uf is an array of components_uf.h");
static_assert(sizeof(svr_split_record) == 80 && offsetof(svr_split_record, top) % 8 == 0, "top[0..1] holds a 64-bit maximum");

struct SplitArgs {
    const int32_t* height;
    uint32_t n[3];
    uint32_t voxels;
    uint32_t H;                // merge_squared
    uint32_t* up;
    uint32_t* uf;
    uint32_t* aux;
    uint32_t* cnt;             // level 0 of the scan
    unsigned long long* header;
    uint32_t* ids;             // null: not written (none given, or too small)
    svr_split_record* records;
    unsigned long long rcap;
};

// ---- up -----------------------------------------------------------------------------------------------------------------
template <bool CONN26>
__global__ __launch_bounds__(kSplitThreads) void split_up_kernel(const SplitArgs a) {
    const uint32_t i = blockIdx.x * kSplitThreads + threadIdx.x;
    uint32_t inside = 0u, summits = 0u;
    if (i < a.voxels) {
        const int32_t h = a.height[i];
        uint32_t up = kSplitOutside, root = kSplitOutside;
        if (h > 0) {
            const uint32_t x = i % a.n[0], row = i / a.n[0], y = row % a.n[1], z = row / a.n[1];
            uint64_t best = split_key(h, i);
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int axes = (dx != 0) + (dy != 0) + (dz != 0);
                        if (axes == 0 || (!CONN26 && axes != 1)) continue;
                        const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;   // before the box: wraps to a huge value
                        if (qx >= a.n[0] || qy >= a.n[1] || qz >= a.n[2]) continue;
                        const uint32_t j = (qz * a.n[1] + qy) * a.n[0] + qx;
                        const int32_t hj = a.height[j];
                        if (hj > 0) { const uint64_t k = split_key(hj, j); best = k > best ? k : best; }
                    }
                }
            }
            up = split_key_index(best);
            inside = 1u;
            if (up == i) { root = i; summits = 1u; }
        }
        a.up[i] = up;
        a.uf[i] = root;
    }
    BOX_WAVE_ADD2(&a.header[1], inside, &a.header[4], summits);
}

// ---- summit -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSplitThreads) void split_summit_kernel(const SplitArgs a) {
    const uint32_t i = blockIdx.x * kSplitThreads + threadIdx.x;
    if (i >= a.voxels) return;
    uint32_t j = uf_load(a.up + i);
    if (j == kSplitOutside || j == i) return;
    for (;;) {
        const uint32_t k = uf_load(a.up + j);               // up(j) or summit(j): never kSplitOutside, j is inside
        if (k == j) break;
        j = k;
    }
    __hip_atomic_store(a.up + i, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- link ---------------------------------------------------------------------------------------------------------------
template <bool CONN26>
__global__ __launch_bounds__(kSplitThreads) void split_link_kernel(const SplitArgs a) {
    const uint32_t i = blockIdx.x * kSplitThreads + threadIdx.x;
    if (i >= a.voxels) return;
    const uint32_t si = a.up[i];
    if (si == kSplitOutside) return;
    const int32_t hi = a.height[i], pi = a.height[si];
    const uint32_t x = i % a.n[0], row = i / a.n[0], y = row % a.n[1], z = row / a.n[1];
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                // the neighbours before i: dz < 0; or dz == 0 and dy < 0; or both 0 and dx < 0
                if (!(dz < 0 || dy < 0 || (dy == 0 && dx < 0))) continue;
                const int axes = (dx != 0) + (dy != 0) + (dz != 0);
                if (!CONN26 && axes != 1) continue;
                const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
                if (qx >= a.n[0] || qy >= a.n[1] || qz >= a.n[2]) continue;
                const uint32_t j = (qz * a.n[1] + qy) * a.n[0] + qx;
                const uint32_t sj = a.up[j];
                if (sj == kSplitOutside || sj == si) continue;
                const int32_t hj = a.height[j], pj = a.height[sj];
                if (split_links(pi < pj ? pi : pj, hi < hj ? hi : hj, a.H)) uf_union(a.uf, si, sj);
            }
        }
    }
}

// ---- scan ---------------------------------------------------------------------------------------------------------------
// What the top level of the scan does with N, the number of seeds: the header's words [0], [2], [3] and [10..12]; the up
// pass counted [1] and [4], and the launcher zeroed the rest.
struct SplitHeader {
    unsigned long long* header;
    unsigned long long ids_written, rcap;
    uint32_t n[3];
    __device__ void operator()(uint32_t total) const {
        const unsigned long long N = total;
        header[0] = N;
        header[2] = ids_written;
        header[3] = N <= rcap ? N : 0ull;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) header[10 + ax] = n[ax];
    }
};

// ---- rank ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSplitThreads) void split_rank_kernel(const SplitArgs a) {
    __shared__ uint32_t part[kBoxScanWaves];
    const uint32_t i = blockIdx.x * kSplitThreads + threadIdx.x;
    const uint32_t is_seed = i < a.voxels && a.uf[i] == i;
    const uint32_t rank = box_block_exclusive(is_seed, part) + a.cnt[blockIdx.x];
    if (!is_seed) return;
    a.aux[i] = rank;
    if (!a.records || a.header[0] > a.rcap) return;
    svr_split_record& r = a.records[rank];
    r.id = rank + 1u; r.basins = 0u;
    r.voxels = 0u;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { r.sum[ax] = 0u; r.top[ax] = 0; r.lo[ax] = INT_MAX; r.hi[ax] = INT_MIN; }
    r.peak = 0;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSplitThreads) void split_emit_kernel(const SplitArgs a) {
    const uint32_t i = blockIdx.x * kSplitThreads + threadIdx.x;
    uint32_t id = 0u;
    unsigned long long key = 0ull;                          // of a summit: what it offers as its region's top
    if (i < a.voxels) {
        const uint32_t s = a.up[i];
        if (s != kSplitOutside) {
            id = a.aux[a.uf[s]] + 1u;
            if (s == i) key = split_key(a.height[i], i);
        }
        if (a.ids) a.ids[i] = id;
    }
    if (!a.records || a.header[0] > a.rcap) return;         // the same for every thread of the launch
    const uint32_t rx = i % a.n[0], row = i / a.n[0], ry = row % a.n[1], rz = row / a.n[1];
    const uint32_t c[3] = {rx, ry, rz};
    box_wave_groups<true>(id, c, key, [&](uint32_t lid, const BoxShare& s) {
        svr_split_record& r = a.records[lid - 1u];
        atomicAdd(reinterpret_cast<unsigned long long*>(&r.voxels), (unsigned long long)s.count);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&r.sum[ax]), s.sum[ax]);
            atomicMin(&r.lo[ax], (int32_t)s.cmin[ax]);
            atomicMax(&r.hi[ax], (int32_t)s.cmax[ax]);
        }
        if (s.tops) {
            atomicAdd(&r.basins, (uint32_t)__popcll(s.tops));
            atomicMax(reinterpret_cast<unsigned long long*>(&r.top[0]), s.best);
        }
    });
}

// ---- finish -------------------------------------------------------------------------------------------------------------
// Launched behind an emit pass that wrote records: record k < N holds in top[0..1] the split_key of its best summit.
__global__ __launch_bounds__(kSplitThreads) void split_finish_kernel(const SplitArgs a) {
    const unsigned long long k = (unsigned long long)blockIdx.x * kSplitThreads + threadIdx.x;
    const unsigned long long N = a.header[0];
    if (N > a.rcap || k >= N) return;
    svr_split_record& r = a.records[k];
    const unsigned long long key = *reinterpret_cast<const unsigned long long*>(&r.top[0]);
    const uint32_t i = split_key_index(key), row = i / a.n[0];
    r.top[0] = (int32_t)(i % a.n[0]); r.top[1] = (int32_t)(row % a.n[1]); r.top[2] = (int32_t)(row / a.n[1]);
    r.peak = split_key_height(key);
}

}  // namespace

// plan: split_plan of sp.n; scratch: plan.bytes of device memory no other call is using.  Everything was validated by
// svr_split.
hipError_t svr_launch_split(const SplitPlan& p, const svr_split_params& sp, void* scratch, const svr_split_outputs& out, hipStream_t stream) {
    char* const base = static_cast<char*>(scratch);
    const bool ids_fit = out.ids_capacity >= (uint64_t)p.voxels;
    SplitHeader h;
    h.header = reinterpret_cast<unsigned long long*>(out.header);
    h.ids_written = ids_fit ? (unsigned long long)p.voxels : 0ull;
    h.rcap = out.record_capacity;
    SplitArgs a;
    a.height = sp.height;
    for (int ax = 0; ax < 3; ++ax) { a.n[ax] = p.n[ax]; h.n[ax] = p.n[ax]; }
    a.voxels = p.voxels;
    a.H = sp.merge_squared;
    a.up = reinterpret_cast<uint32_t*>(base + p.up_off);
    a.uf = reinterpret_cast<uint32_t*>(base + p.uf_off);
    a.aux = reinterpret_cast<uint32_t*>(base + p.aux_off);
    a.cnt = reinterpret_cast<uint32_t*>(base + p.scan.off[0]);
    a.header = h.header;
    a.ids = ids_fit ? out.ids : nullptr;
    a.records = out.record_capacity > 0 ? out.records : nullptr;
    a.rcap = out.record_capacity;

    hipError_t e = hipMemsetAsync(h.header, 0, 16 * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(p.scan.count[0]), block(kSplitThreads);
    const bool conn26 = sp.connectivity == 26;
    if (conn26) hipLaunchKernelGGL(split_up_kernel<true>, grid, block, 0, stream, a);
    else        hipLaunchKernelGGL(split_up_kernel<false>, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(split_summit_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (conn26) hipLaunchKernelGGL(split_link_kernel<true>, grid, block, 0, stream, a);
    else        hipLaunchKernelGGL(split_link_kernel<false>, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(uf_flatten_kernel, grid, block, 0, stream, a.uf, a.voxels, a.cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    if ((e = box_scan_run<uint32_t>(&p.scan, scratch, h, stream)) != hipSuccess) return e;
    // the count-only call ends here; a call whose records cannot fit finds that out on the device
    if (!a.ids && !a.records) return hipSuccess;
    hipLaunchKernelGGL(split_rank_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(split_emit_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!a.records) return hipSuccess;
    // N <= rcap records at the most, and N <= voxels: a thread per record that can exist
    const uint64_t most = a.rcap < (uint64_t)p.voxels ? a.rcap : (uint64_t)p.voxels;
    hipLaunchKernelGGL(split_finish_kernel, dim3((uint32_t)((most + kSplitThreads - 1) / kSplitThreads)), block, 0, stream, a);
    return hipGetLastError();
}
