// Connected components of the resident rings (svr_components, include/svr.h): union-find over a box of one LOD's window,
// components numbered by their first voxels, a dense volume of numbers and one record per component.  gfx950.
//
// The chain (layout of the scratch: components_plan.h), every kernel a plain launch on the caller's stream; no
// workgroup waits for another inside a launch and nothing spins on a flag:
//   init     the one pass over the rings.  A lane owns 4 consecutive ring slots at a multiple of 4 (components_plan.h:
//            head): a unit of box_units.h, which states how it is loaded, at a row's ends and at the ring's wrap seam
//            too, and what inside() is.  Writes parent[i]: kUfOutside for a voxel that is outside, else the first voxel
//            of the run of connecting voxels it belongs to among the lane's 4, so x neighbours inside a lane are linked
//            for free; and, where labels split components, the label into aux[i], so that no later pass reads a wrapped
//            ring row.  Counts the inside voxels and the dropped zeros, one atomic each per wave.
//   merge    a thread per voxel joins it with the neighbours before it (components_uf.h: uf_merge_voxel, the rules of
//            the union-find are stated there); 6- and 26-connectivity, with and without labels, are compile-time variants.
//   flatten  parent[i] = root(i), and the number of roots among each workgroup's voxels: level 0 of the scan
//            (components_uf.h: uf_flatten_kernel).
//   scan     an exclusive prefix of those counts in place: the scan of box_scan.h on u32, whose top level writes the
//            header (CompHeader).
//   rank     a root in (z, y, x) order is the first voxel of its component, so the number of roots before it is its
//            component's number minus one: into aux[root]; and, when the records fit, the root starts its record (id,
//            label, first; empty sums and an empty box).
//   emit     a thread per voxel: ids[i] = aux[parent[i]] + 1, and the voxel's share of its record.  The lanes of a
//            wave that belong to one component add up and reduce their shares with shuffles first (box_scan.h:
//            box_wave_groups).  Skipped by the count-only call.
// parent is only ever written by the init pass and by atomic minima; every other store is an ordinary vector store.
#include <limits.h>

#include "svr_host.h"
#include "components_plan.h"
#include "components_uf.h"
#include "box_scan.h"
#include "box_units.h"

namespace {

constexpr int kCompThreads = 256;
static_assert(kBoxScanBlock == (uint32_t)kCompThreads, "one entry, and one voxel, per thread");

struct CompArgs {
    const void* density;
    const uint32_t* labels;    // null: every label reads as 0
    uint32_t ring[3];
    uint32_t n[3];             // extent of the box B
    uint32_t s0[3];            // ring slot of B's first voxel
    int32_t lo[3];             // B's first voxel
    int32_t rel[3];            // B's first voxel minus the window offset
    uint32_t voxels, head, upr, units;
    float level;
    const uint32_t* sel;
    uint32_t nsel;
    int32_t ignore_zero, label_mode;
    uint32_t* parent;
    uint32_t* aux;
    uint32_t* cnt;             // level 0 of the scan
    unsigned long long* header;
    uint32_t* ids;             // null: not written (none given, or too small)
    svr_component_record* records;
    unsigned long long rcap;
};

// ---- init ---------------------------------------------------------------------------------------------------------------
// LEVEL: the value reaches the level; else the label passes `selected` and ignore_zero.  KEYED: labels split components.
template <typename T, bool LEVEL, bool KEYED>
__global__ __launch_bounds__(kCompThreads) void comp_init_kernel(const CompArgs a) {
    const T* const ring = static_cast<const T*>(a.density);
    const uint32_t n0 = a.n[0];
    uint32_t count = 0u, zeros = 0u;                        // this lane's: fewer than 2^32 in a box
    BoxInside cache = {};
    for (uint32_t unit = blockIdx.x * kCompThreads + threadIdx.x; unit < a.units; unit += gridDim.x * kCompThreads) {
        const uint32_t row = unit / a.upr, w = unit - row * a.upr;
        const uint32_t ry = row % a.n[1], rz = row / a.n[1];
        const int32_t r0 = (int32_t)(4u * w) - (int32_t)a.head;                 // the lane's voxels: r0 .. r0 + 3 of the row
        const size_t rowoff = box_row_offset(a, ry, rz);
        uint32_t lab[4] = {0u, 0u, 0u, 0u};
        float val[4] = {0.0f, 0.0f, 0.0f, 0.0f}; uint32_t have = 0u;
        BOX_GATHER(T, LEVEL, a, ring, n0, rowoff, r0, val, lab, have);
        const uint32_t i0 = row * n0 + (uint32_t)r0;                             // dense index of voxel r0 (wraps where r0 < 0: only r0 + j >= 0 is used)
        uint32_t start = 0u; bool prev_in = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(have & (1u << j))) { prev_in = false; continue; }
            bool in;
            BOX_INSIDE(in, LEVEL, cache, val[j], lab[j], a.level, a.nsel == 0u || ring_in_set(a.sel, a.nsel, lab[j]),
                       BOX_DROP_ZERO(in, lab[j], a.ignore_zero, zeros));
            const uint32_t i = i0 + (uint32_t)j;
            if (in) {
                const bool joins = prev_in && (!KEYED || lab[j] == lab[j - (j > 0)]);
                if (!joins) start = i;
                a.parent[i] = start;
                if (KEYED) a.aux[i] = lab[j];
                ++count;
            } else a.parent[i] = kUfOutside;
            prev_in = in;
        }
    }
    BOX_WAVE_ADD2(&a.header[1], count, &a.header[13], zeros);
}

// ---- merge --------------------------------------------------------------------------------------------------------------
template <bool CONN26, bool KEYED>
__global__ __launch_bounds__(kCompThreads) void comp_merge_kernel(const CompArgs a) {
    const uint32_t i = blockIdx.x * kCompThreads + threadIdx.x;
    if (i < a.voxels) uf_merge_voxel<CONN26, KEYED>(a.parent, a.aux, i, a.n, a.head);
}

// ---- scan ---------------------------------------------------------------------------------------------------------------
// What the top level of the scan does with N, the number of roots: the header but for [1] and [13], which the init pass
// counted.
struct CompHeader {
    unsigned long long* header;
    unsigned long long ids_written, rcap;
    int32_t off[3], lo[3];
    uint32_t n[3];
    __device__ void operator()(uint32_t total) const {
        const unsigned long long N = total;
        header[0] = N;
        header[2] = ids_written;
        header[3] = N <= rcap ? N : 0ull;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            header[4 + ax] = (unsigned long long)(long long)off[ax];
            header[7 + ax] = (unsigned long long)(long long)lo[ax];
            header[10 + ax] = n[ax];
        }
        header[14] = 0ull; header[15] = 0ull;
    }
};

// ---- rank ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void comp_rank_kernel(const CompArgs a) {
    __shared__ uint32_t part[kBoxScanWaves];
    const uint32_t i = blockIdx.x * kCompThreads + threadIdx.x;
    const uint32_t is_root = i < a.voxels && a.parent[i] == i;
    const uint32_t rank = box_block_exclusive(is_root, part) + a.cnt[blockIdx.x];
    if (!is_root) return;
    a.aux[i] = rank;
    if (!a.records || a.header[0] > a.rcap) return;
    const uint32_t rx = i % a.n[0], row = i / a.n[0], ry = row % a.n[1], rz = row / a.n[1];
    uint32_t label = 0u;
    if (a.label_mode && a.labels) label = a.labels[box_row_offset(a, ry, rz) + box_slot(a.s0[0], rx, a.ring[0])];
    svr_component_record& r = a.records[rank];
    r.id = rank + 1u; r.label = label;
    r.voxels = 0u;
    r.first[0] = a.lo[0] + (int32_t)rx; r.first[1] = a.lo[1] + (int32_t)ry; r.first[2] = a.lo[2] + (int32_t)rz;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { r.sum[ax] = 0u; r.lo[ax] = INT_MAX; r.hi[ax] = INT_MIN; }
    r.reserved = 0u;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void comp_emit_kernel(const CompArgs a) {
    const uint32_t i = blockIdx.x * kCompThreads + threadIdx.x;
    uint32_t id = 0u;
    if (i < a.voxels) {
        const uint32_t p = a.parent[i];
        if (p != kUfOutside) id = a.aux[p] + 1u;
        if (a.ids) a.ids[i] = id;
    }
    if (!a.records || a.header[0] > a.rcap) return;         // the same for every thread of the launch
    const uint32_t rx = i % a.n[0], row = i / a.n[0], ry = row % a.n[1], rz = row / a.n[1];
    const uint32_t c[3] = {rx, ry, rz};
    box_wave_groups<false>(id, c, 0ull, [&](uint32_t lid, const BoxShare& s) {
        svr_component_record& r = a.records[lid - 1u];
        atomicAdd(reinterpret_cast<unsigned long long*>(&r.voxels), (unsigned long long)s.count);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // every lane's share is its coordinate in the window, rel + c
            atomicAdd(reinterpret_cast<unsigned long long*>(&r.sum[ax]), s.sum[ax] + (unsigned long long)s.count * (uint32_t)a.rel[ax]);
            atomicMin(&r.lo[ax], a.lo[ax] + (int32_t)s.cmin[ax]);
            atomicMax(&r.hi[ax], a.lo[ax] + (int32_t)s.cmax[ax]);
        }
    });
}

template <typename T, bool LEVEL>
void comp_launch_init(const CompArgs& a, bool keyed, uint32_t blocks, hipStream_t stream) {
    if constexpr (!LEVEL) {
        if (keyed) { hipLaunchKernelGGL((comp_init_kernel<T, false, true>), dim3(blocks), dim3(kCompThreads), 0, stream, a); return; }
    }
    hipLaunchKernelGGL((comp_init_kernel<T, LEVEL, false>), dim3(blocks), dim3(kCompThreads), 0, stream, a);
}

}  // namespace

// lo: the first voxel of the box (box and window intersected) in logical voxels of the LOD; plan: comp_plan of its
// extent, or null for an empty box; scratch: plan->bytes of device memory no other call is using.  Everything was
// validated by svr_components.
hipError_t svr_launch_components(const svr_ctx* c, int lod, const int64_t lo[3], const CompPlan* plan, const svr_components_params& cp,
                                 void* scratch, const svr_components_outputs& out, hipStream_t stream) {
    const LodStorage& L = c->lod[lod];
    const svr_lod_state& st = L.state;
    CompHeader h;
    h.header = reinterpret_cast<unsigned long long*>(out.header);
    h.ids_written = 0ull; h.rcap = out.record_capacity;
    for (int ax = 0; ax < 3; ++ax) { h.off[ax] = st.offset[ax]; h.lo[ax] = 0; h.n[ax] = 0u; }
    hipError_t e = hipMemsetAsync(h.header, 0, 16 * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    if (!plan) return box_scan_run<uint32_t>(nullptr, nullptr, h, stream);     // no voxel: the header alone
    const CompPlan& p = *plan;
    char* const base = static_cast<char*>(scratch);
    const bool is_level = cp.mode == SVR_COMPONENTS_LEVEL;
    const bool keyed = !is_level && cp.join_labels == 0;
    const bool ids_fit = out.ids_capacity >= (uint64_t)p.voxels;
    CompArgs a;
    a.density = L.density; a.labels = L.labels;
    for (int ax = 0; ax < 3; ++ax) {
        a.ring[ax] = (uint32_t)L.ring[ax];
        a.n[ax] = p.n[ax];
        a.s0[ax] = (uint32_t)(lo[ax] % (int64_t)L.ring[ax]);
        a.lo[ax] = (int32_t)lo[ax];
        a.rel[ax] = (int32_t)(lo[ax] - (int64_t)st.offset[ax]);
        h.lo[ax] = a.lo[ax]; h.n[ax] = p.n[ax];
    }
    a.voxels = p.voxels; a.head = p.head; a.upr = p.upr; a.units = p.units;
    a.level = cp.level;
    a.sel = is_level ? nullptr : cp.selected; a.nsel = is_level ? 0u : cp.selected_count;
    a.ignore_zero = cp.ignore_zero; a.label_mode = is_level ? 0 : 1;
    a.parent = reinterpret_cast<uint32_t*>(base + p.parent_off);
    a.aux = reinterpret_cast<uint32_t*>(base + p.aux_off);
    a.cnt = reinterpret_cast<uint32_t*>(base + p.scan.off[0]);
    a.header = h.header;
    a.ids = ids_fit ? out.ids : nullptr;
    a.records = out.record_capacity > 0 ? out.records : nullptr;
    a.rcap = out.record_capacity;
    h.ids_written = ids_fit ? (unsigned long long)p.voxels : 0ull;

    // init: 256 units of 4 voxels per workgroup and round, 8 workgroups per CU at the most
    const uint64_t want = ((uint64_t)p.units + kCompThreads - 1) / kCompThreads;
    const uint64_t most = ring_workgroups(c->device, 8);
    const uint32_t init_blocks = (uint32_t)(want < most ? want : most);
    if (!is_level)                             comp_launch_init<uint8_t, false>(a, keyed, init_blocks, stream);   // the density ring is not read
    else if (c->density_storage == SVR_U8)     comp_launch_init<uint8_t, true>(a, false, init_blocks, stream);
    else if (c->density_storage == SVR_U16)    comp_launch_init<uint16_t, true>(a, false, init_blocks, stream);
    else                                       comp_launch_init<float, true>(a, false, init_blocks, stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    const dim3 grid(p.scan.count[0]), block(kCompThreads);
    const bool conn26 = cp.connectivity == 26;
    if (conn26 && keyed)  hipLaunchKernelGGL((comp_merge_kernel<true, true>), grid, block, 0, stream, a);
    else if (conn26)      hipLaunchKernelGGL((comp_merge_kernel<true, false>), grid, block, 0, stream, a);
    else if (keyed)       hipLaunchKernelGGL((comp_merge_kernel<false, true>), grid, block, 0, stream, a);
    else                  hipLaunchKernelGGL((comp_merge_kernel<false, false>), grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(uf_flatten_kernel, grid, block, 0, stream, a.parent, a.voxels, a.cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    if ((e = box_scan_run<uint32_t>(&p.scan, scratch, h, stream)) != hipSuccess) return e;
    // the count-only call skips the last two kernels; a call whose records cannot fit finds that out on the device
    if (!a.ids && !a.records) return hipSuccess;
    hipLaunchKernelGGL(comp_rank_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(comp_emit_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}
