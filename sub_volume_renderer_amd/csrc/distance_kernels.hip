// Exact Euclidean distance transform of the resident rings (svr_distance, include/svr.h): squared distances, in voxels,
// of the targets of a box of one LOD's window to the nearest source, axis by axis.  gfx950.
//
// The chain (layout of the scratch: distance_plan.h), every kernel a plain launch on the caller's stream; no workgroup
// waits for another inside a launch and nothing spins on a flag:
//   init     the one pass over the rings.  A lane owns 4 consecutive ring slots at a multiple of 4: a unit of
//            box_units.h, which states how it is loaded, at a row's ends and at the ring's wrap seam too, and what
//            inside() is.  Its 4 source bits are a nibble; 8 adjacent lanes OR theirs together with three shuffles and
//            one of them stores the word.  Counts the inside voxels and the dropped zeros, one atomic each per wave.
//   header   one thread: the words of the header that need no distance.  The count-only call ends here.
//   x        a thread per voxel: the squared distance to the nearest source bit of its row, from count-leading and
//            count-trailing-zero operations on the row's words (distance_plan.h: dist_row_nearest), into d2.
//   y, z     a thread per column, a wave's lanes adjacent in x, so that every load and store of one position of the
//            column is one contiguous run per wave: the lower envelope of parabolas (distance_scan.h), in place in d2,
//            its stack in the scratch, the last 16 entries pushed also in LDS, where most pops find what they need.
//            Linear in the column's length whatever the data.
//            The z pass ends the chain: it takes the minimum with the squared distance to the nearest lattice point
//            beyond the box (border: the smallest of the six face distances plus one, squared: that point lies straight
//            across the nearest face), and reduces header [3], [14], [15]: shuffles first, then one 64-bit atomic maximum
//            per wave on (d2 << 32) | (0xFFFFFFFF - index), and one add.
//   finish   one thread: unpacks that maximum into header [3] and [14].
// Every store is an ordinary vector store; the only atomics are the counters of the header.
//
// svr_nearest (the nearest source of every voxel) runs the same chain without a border, in the OWN instantiations of the
// x, y and z kernels, which also store who owns each voxel along the axis (u16 planes in the scratch: distance_plan.h),
// and ends with
//   compose  a thread per voxel: z' = own_z[z][y][x], y' = own_y[z'][y][x], x' = own_x[z'][y'][x], the dense index of
//            (x', y', z') into index, and one gather from the label ring at that voxel's ring slot into label.
// Everything else is one text for both calls.
#include "svr_host.h"
#include "distance_plan.h"
#include "distance_scan.h"
#include "box_units.h"

namespace {

constexpr int kDistThreads = 256;      // init and x pass
constexpr int kDistColumnThreads = 64; // y and z pass: one wave, so that few columns still spread over the CUs
constexpr uint32_t kDistRingEntries = 16;  // of a column's stack kept in LDS (distance_scan.h: DistRing): 8 KiB per workgroup

struct DistArgs {
    const void* density;
    const uint32_t* labels;    // null: every label reads as 0
    uint32_t ring[3];
    uint32_t n[3];             // extent of the box B
    uint32_t s0[3];            // ring slot of B's first voxel
    uint32_t voxels, head, upr, wpr, units;
    float level;
    const uint32_t* sel;
    uint32_t nsel;
    int32_t ignore_zero, invert, border;
    uint32_t* bits;
    DistEntry* stack;
    int32_t* d2;
    unsigned long long* header;
};

// ---- init ---------------------------------------------------------------------------------------------------------------
// LEVEL: the value reaches the level; else the label passes `selected` and ignore_zero.  a.units is a multiple of 8 and so
// is every stride of the loop, so the 8 lanes that share a word of bits enter and leave the loop together.
template <typename T, bool LEVEL>
__global__ __launch_bounds__(kDistThreads) void dist_init_kernel(const DistArgs a) {
    const T* const ring = static_cast<const T*>(a.density);
    const uint32_t n0 = a.n[0];
    uint32_t count = 0u, zeros = 0u;                        // this lane's: fewer than 2^32 in a box
    BoxInside cache = {};
    for (uint32_t unit = blockIdx.x * kDistThreads + threadIdx.x; unit < a.units; unit += gridDim.x * kDistThreads) {
        const uint32_t row = unit / a.upr, w = unit - row * a.upr;
        const uint32_t ry = row % a.n[1], rz = row / a.n[1];
        const int32_t r0 = (int32_t)(4u * w) - (int32_t)a.head;                 // the lane's voxels: r0 .. r0 + 3 of the row
        const size_t rowoff = box_row_offset(a, ry, rz);
        uint32_t lab[4] = {0u, 0u, 0u, 0u};
        float val[4] = {0.0f, 0.0f, 0.0f, 0.0f}; uint32_t have = 0u;
        BOX_GATHER(T, LEVEL, a, ring, n0, rowoff, r0, val, lab, have);
        uint32_t nibble = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(have & (1u << j))) continue;
            bool in;
            BOX_INSIDE(in, LEVEL, cache, val[j], lab[j], a.level, a.nsel == 0u || ring_in_set(a.sel, a.nsel, lab[j]),
                       BOX_DROP_ZERO(in, lab[j], a.ignore_zero, zeros));
            if (in) ++count;
            if (in == (a.invert != 0)) nibble |= 1u << j;                        // a source
        }
        uint32_t word = nibble << (4u * (w & 7u));
        word |= (uint32_t)__shfl_xor((int)word, 1);
        word |= (uint32_t)__shfl_xor((int)word, 2);
        word |= (uint32_t)__shfl_xor((int)word, 4);
        if ((w & 7u) == 0u) a.bits[(size_t)row * a.wpr + (w >> 3)] = word;
    }
    BOX_WAVE_ADD2(&a.header[1], count, &a.header[13], zeros);
}

// ---- header and finish ----------------------------------------------------------------------------------------------------
struct DistHeader {
    unsigned long long* header;
    unsigned long long voxels, written;
    int32_t invert;
    int32_t off[3], lo[3];
    uint32_t n[3];
};

// the header but for [1] and [13], which the init pass counted, and [3], [14], [15], which the z pass reduces
__global__ void dist_header_kernel(const DistHeader h) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const unsigned long long inside = h.header[1];
    h.header[0] = h.invert ? h.voxels - inside : inside;
    h.header[2] = h.written;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        h.header[4 + ax] = (unsigned long long)(long long)h.off[ax];
        h.header[7 + ax] = (unsigned long long)(long long)h.lo[ax];
        h.header[10 + ax] = h.n[ax];
    }
}

// header[3] holds the maximum of (d2 << 32) | (0xFFFFFFFF - index) over the targets that are not FAR, or 0
__global__ void dist_finish_kernel(unsigned long long* header) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const unsigned long long key = header[3];
    header[3] = key >> 32;
    header[14] = key ? 0xFFFFFFFFull - (key & 0xFFFFFFFFull) : 0ull;
}

// ---- x ------------------------------------------------------------------------------------------------------------------
// OWN (svr_nearest): and the row voxel of that source into own[i]; else own is not used
template <bool OWN>
__global__ __launch_bounds__(kDistThreads) void dist_x_kernel(const DistArgs a, uint16_t* const own) {
    const uint32_t i = blockIdx.x * kDistThreads + threadIdx.x;
    if (i >= a.voxels) return;
    const uint32_t row = i / a.n[0], rx = i - row * a.n[0];
    if constexpr (OWN) {
        uint32_t at = kDistNoOwner + a.head;
        a.d2[i] = dist_row_nearest_at(a.bits + (size_t)row * a.wpr, a.wpr, rx + a.head, &at);
        own[i] = (uint16_t)(at - a.head);                    // an element of the row -> a voxel of it
    } else {
        a.d2[i] = dist_row_nearest(a.bits + (size_t)row * a.wpr, a.wpr, rx + a.head);
    }
}

// ---- y and z ------------------------------------------------------------------------------------------------------------
// FINAL: the z pass, else the y pass.  columns = voxels / length.  OWN (svr_nearest): the owner of every position into
// the plane `own`, and no border; else own is not used.
template <bool FINAL, bool OWN>
__global__ __launch_bounds__(kDistColumnThreads) void dist_column_kernel(const DistArgs a, uint16_t* const own, uint32_t columns) {
    __shared__ DistEntry slots[kDistRingEntries * kDistColumnThreads];     // slot j of lane l at [j * 64 + l]: no bank conflicts
    const DistRing<kDistRingEntries> ring(slots + threadIdx.x, kDistColumnThreads);
    const uint32_t c = blockIdx.x * kDistColumnThreads + threadIdx.x;
    const uint32_t n0 = a.n[0], n1 = a.n[1], n2 = a.n[2];
    uint32_t far = 0u;
    unsigned long long key = 0ull;
    if (c < columns) {
        const uint32_t x = c % n0, other = c / n0;           // FINAL: other is y; else z
        const uint32_t base = FINAL ? c : other * n1 * n0 + x;
        const uint32_t stride = FINAL ? n0 * n1 : n0, length = FINAL ? n2 : n1;
        int32_t* const col = a.d2 + base;
        // the squared distance to the nearest lattice point beyond the box is ((face distance) + 1)^2; without a
        // border nothing lies there
        const bool border = FINAL && !OWN && a.border != 0 && a.invert == 0;
        const uint32_t fxy = min(min(x + 1u, n0 - x), min(other + 1u, n1 - other));
        const auto sink = [&](uint32_t u, int32_t v, uint32_t s) {
            if (border && v != 0) {
                const uint32_t f = min(fxy, min(u + 1u, n2 - u));
                v = min(v, (int32_t)(f * f));
            }
            col[(size_t)u * stride] = v;
            if (OWN) own[base + (size_t)u * stride] = (uint16_t)s;
            if (FINAL) {
                if (v == kDistFar) ++far;
                else if (v != 0) {
                    // u runs downward: an equal value at a smaller index replaces the key, as its low half is larger
                    const unsigned long long k = ((unsigned long long)(uint32_t)v << 32) | (0xFFFFFFFFu - (base + u * stride));
                    if (k > key) key = k;
                }
            }
        };
        if constexpr (OWN) dist_scan_column_owner(col, stride, length, a.stack + c, columns, ring, sink);
        else dist_scan_column(col, stride, length, a.stack + c, columns, ring, [&](uint32_t u, int32_t v) { sink(u, v, 0u); });
    }
    if (FINAL) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            far += (uint32_t)__shfl_xor((int)far, d);
            const unsigned long long o = __shfl_xor(key, d);
            if (o > key) key = o;
        }
        if (__lane_id() == 0u) {
            if (key) atomicMax(&a.header[3], key);
            if (far) atomicAdd(&a.header[15], (unsigned long long)far);
        }
    }
}

// ---- svr_nearest: compose -----------------------------------------------------------------------------------------------
struct NearOut {
    uint16_t* own[3];          // the owner planes of the x, y and z pass (distance_plan.h)
    int32_t* index;
    uint32_t* label;           // null: not written
};

// Every owner is compared with its extent before it is used: kDistNoOwner, of a column without a source, fails it, and no
// gather leaves its plane or the ring.  An owner that the z pass names has a finite value, so the two below it exist.
__global__ __launch_bounds__(kDistThreads) void near_compose_kernel(const DistArgs a, const NearOut o) {
    const uint32_t i = blockIdx.x * kDistThreads + threadIdx.x;
    if (i >= a.voxels) return;
    const uint32_t n0 = a.n[0], n1 = a.n[1];
    const uint32_t row = i / n0, x = i - row * n0, y = row % n1;
    int32_t index = -1;
    uint32_t label = 0u;
    const uint32_t oz = o.own[2][i];
    if (oz < a.n[2]) {
        const uint32_t oy = o.own[1][(oz * n1 + y) * n0 + x];
        if (oy < n1) {
            const uint32_t r = oz * n1 + oy;
            const uint32_t ox = o.own[0][r * n0 + x];
            if (ox < n0) {
                index = (int32_t)(r * n0 + ox);
                if (a.labels) label = a.labels[box_row_offset(a, oy, oz) + box_slot(a.s0[0], ox, a.ring[0])];
            }
        }
    }
    o.index[i] = index;
    if (o.label) o.label[i] = label;
}

// What both calls want of a box: P is svr_distance_params or svr_nearest_params, whose fields of the same names mean the same.
// The header zeroed, then for a box that is not empty (plan) a and h filled, the init pass and the header kernel.  *go: d2
// is to be written, dist_axes follows.
template <class P>
hipError_t dist_begin(const svr_ctx* c, int lod, const int64_t lo[3], const DistPlan* plan, const P& dp, int border, void* scratch,
                      int32_t* d2, uint64_t capacity, uint64_t* header, hipStream_t stream, DistArgs& a, bool* go) {
    *go = false;
    const LodStorage& L = c->lod[lod];
    const svr_lod_state& st = L.state;
    DistHeader h;
    h.header = reinterpret_cast<unsigned long long*>(header);
    h.voxels = 0ull; h.written = 0ull; h.invert = dp.invert != 0;
    for (int ax = 0; ax < 3; ++ax) { h.off[ax] = st.offset[ax]; h.lo[ax] = 0; h.n[ax] = 0u; }
    hipError_t e = hipMemsetAsync(h.header, 0, 16 * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    if (!plan) {                                            // no voxel: the header alone
        hipLaunchKernelGGL(dist_header_kernel, dim3(1), dim3(1), 0, stream, h);
        return hipGetLastError();
    }
    const DistPlan& p = *plan;
    char* const base = static_cast<char*>(scratch);
    const bool is_level = dp.mode == SVR_COMPONENTS_LEVEL;
    const bool fits = capacity >= (uint64_t)p.voxels;
    a.density = L.density; a.labels = L.labels;
    for (int ax = 0; ax < 3; ++ax) {
        a.ring[ax] = (uint32_t)L.ring[ax];
        a.n[ax] = p.n[ax];
        a.s0[ax] = (uint32_t)(lo[ax] % (int64_t)L.ring[ax]);
        h.lo[ax] = (int32_t)lo[ax]; h.n[ax] = p.n[ax];
    }
    a.voxels = p.voxels; a.head = p.head; a.upr = p.upr; a.wpr = p.wpr; a.units = p.units;
    a.level = dp.level;
    a.sel = is_level ? nullptr : dp.selected; a.nsel = is_level ? 0u : dp.selected_count;
    a.ignore_zero = is_level ? 0 : dp.ignore_zero; a.invert = dp.invert != 0; a.border = border != 0;
    a.bits = reinterpret_cast<uint32_t*>(base + p.bits_off);
    a.stack = reinterpret_cast<DistEntry*>(base + p.stack_off);
    a.d2 = fits ? d2 : nullptr;
    a.header = h.header;
    h.voxels = p.voxels; h.written = fits ? (unsigned long long)p.voxels : 0ull;

    // init: 256 units of 4 voxels per workgroup and round, 8 workgroups per CU at the most
    const uint64_t want = ((uint64_t)p.units + kDistThreads - 1) / kDistThreads;
    const uint64_t most = ring_workgroups(c->device, 8);
    const dim3 init_grid((uint32_t)(want < most ? want : most)), block(kDistThreads);
    if (!is_level)                             hipLaunchKernelGGL((dist_init_kernel<uint8_t, false>), init_grid, block, 0, stream, a);   // the density ring is not read
    else if (c->density_storage == SVR_U8)     hipLaunchKernelGGL((dist_init_kernel<uint8_t, true>), init_grid, block, 0, stream, a);
    else if (c->density_storage == SVR_U16)    hipLaunchKernelGGL((dist_init_kernel<uint16_t, true>), init_grid, block, 0, stream, a);
    else                                       hipLaunchKernelGGL((dist_init_kernel<float, true>), init_grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dist_header_kernel, dim3(1), dim3(1), 0, stream, h);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    *go = a.d2 != nullptr;                                  // else the count-only call, and a capacity that is too small
    return hipSuccess;
}

// x, y, z and finish.  OWN: own[3], the owner planes of the three passes; else own is null.
template <bool OWN>
hipError_t dist_axes(const DistPlan& p, const DistArgs& a, uint16_t* const* own, hipStream_t stream) {
    const dim3 block(kDistThreads), column_block(kDistColumnThreads);
    hipError_t e;
    hipLaunchKernelGGL(dist_x_kernel<OWN>, dim3((p.voxels + kDistThreads - 1u) / kDistThreads), block, 0, stream, a, OWN ? own[0] : nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((dist_column_kernel<false, OWN>), dim3((p.columns[0] + kDistColumnThreads - 1u) / kDistColumnThreads), column_block, 0,
                       stream, a, OWN ? own[1] : nullptr, p.columns[0]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((dist_column_kernel<true, OWN>), dim3((p.columns[1] + kDistColumnThreads - 1u) / kDistColumnThreads), column_block, 0,
                       stream, a, OWN ? own[2] : nullptr, p.columns[1]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dist_finish_kernel, dim3(1), dim3(1), 0, stream, a.header);
    return hipGetLastError();
}

}  // namespace

// lo: the first voxel of the box (box and window intersected) in logical voxels of the LOD; plan: dist_plan of its
// extent, or null for an empty box; scratch: plan->bytes of device memory no other call is using.  Everything was
// validated by svr_distance.
hipError_t svr_launch_distance(const svr_ctx* c, int lod, const int64_t lo[3], const DistPlan* plan, const svr_distance_params& dp,
                               void* scratch, const svr_distance_outputs& out, hipStream_t stream) {
    DistArgs a;
    bool go;
    const hipError_t e = dist_begin(c, lod, lo, plan, dp, dp.border, scratch, out.d2, out.d2_capacity, out.header, stream, a, &go);
    if (e != hipSuccess || !go) return e;
    return dist_axes<false>(*plan, a, nullptr, stream);
}

// As svr_launch_distance without a border; plan: near_plan of the box's extent.  Everything was validated by svr_nearest.
hipError_t svr_launch_nearest(const svr_ctx* c, int lod, const int64_t lo[3], const NearPlan* plan, const svr_nearest_params& np,
                              void* scratch, const svr_nearest_outputs& out, hipStream_t stream) {
    DistArgs a;
    bool go;
    hipError_t e = dist_begin(c, lod, lo, plan ? &plan->d : nullptr, np, 0, scratch, out.d2, out.capacity, out.header, stream, a, &go);
    if (e != hipSuccess || !go) return e;
    const DistPlan& p = plan->d;
    NearOut o;
    for (int ax = 0; ax < 3; ++ax) o.own[ax] = reinterpret_cast<uint16_t*>(static_cast<char*>(scratch) + plan->own_off[ax]);
    o.index = out.index; o.label = out.label;
    if ((e = dist_axes<true>(p, a, o.own, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(near_compose_kernel, dim3((p.voxels + kDistThreads - 1u) / kDistThreads), dim3(kDistThreads), 0, stream, a, o);
    return hipGetLastError();
}
