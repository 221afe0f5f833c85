// Surface meshes of the resident rings (svr_mesh, include/svr.h): naive surface nets over a box of one LOD's window, one
// vertex per mixed cell and one quad per crossing lattice edge, in the order the header defines.  gfx950.
//
// The chain (layout of the scratch: mesh_plan.h), every kernel a plain launch on the caller's stream:
//   inside     the one pass over the rings.  A lane owns 4 consecutive bits of a row of the bit map, which are 4
//              consecutive ring slots at a multiple of 4 (mesh_plan.h: head): a unit of box_units.h, which states how
//              it is loaded, at a row's ends and at the ring's wrap seam too, and what inside() is.  8 lanes join
//              their bits into one u32.  Rows wrap in y and z by their ring slot.  Counts the inside voxels (header[7]).
//   classify   bit operations only: a thread makes one word of 16 cells from 17 bits of each of the 4 voxel rows
//              (y, y + 1) x (z, z + 1); the x neighbour is the same bits shifted by one.  Rows outside the box read as
//              zero without touching memory.  Writes the word and its two counts (active cells, crossing edges).
//   scan       an exclusive prefix of the two counts in place: the scan of box_scan.h on uint2, whose top level writes
//              header[0 .. 6] (MeshTop).
//   emit       a thread per cell.  The index of a cell's vertex is prefix[word] + popcount(active bits below it), that
//              of its quads likewise; the corners' inside bits come from the bit map, and only SVR_MESH_LEVEL reads
//              the rings again, for the values at an active cell's corners.  Does nothing when a capacity is too small.
// All stores are ordinary vector stores; the one atomic is the u64 add of the inside-voxel count, once per wave.
#include "svr_host.h"
#include "mesh_plan.h"
#include "box_scan.h"
#include "box_units.h"

namespace {

constexpr int kMeshThreads = 256;
constexpr unsigned long long kActiveBits = 0x8888888888888888ull;   // bit 3 of every cell of a word
constexpr unsigned long long kEdgeBits = 0x7777777777777777ull;     // bits 0 .. 2

struct MeshArgs {
    const void* density;
    const uint32_t* labels;    // null: every label reads as 0
    uint32_t ring[3];
    uint32_t n[3];             // extent of the box B
    uint32_t s0[3];            // ring slot of B's first voxel
    int32_t rel[3];            // B's first voxel minus the window offset
    uint32_t cells[3], wpr, words;
    uint32_t head, bpr, bit_words;
    float level;
    const uint32_t* sel;
    uint32_t nsel;
    uint32_t* bits;
    unsigned long long* nib;
    uint2* cnt;                // level 0 of the scan: (active cells, crossing edges) per word, then their exclusive prefix
    unsigned long long* header;
    float* vertices;
    int32_t* triangles;
    unsigned long long vcap, tcap;
};

// ---- inside: the bit map ----------------------------------------------------------------------------------------------
// LEVEL false: the label is one of sel; true: the value reaches the level
template <typename T, bool LEVEL>
__global__ __launch_bounds__(kMeshThreads) void mesh_inside_kernel(const MeshArgs a) {
    const uint32_t tid = threadIdx.x, sub = tid & 7u;
    const T* const ring = static_cast<const T*>(a.density);
    const uint32_t n0 = a.n[0];
    uint32_t count = 0u;                                    // this lane's inside voxels: fewer than 2^32 in a box
    BoxInside cache = {};
    // 8 lanes make one u32 of the bit map; the trip count is the same for the whole workgroup
    for (uint32_t u0 = blockIdx.x * (kMeshThreads / 8u); u0 < a.bit_words; u0 += gridDim.x * (kMeshThreads / 8u)) {
        const uint32_t unit = u0 + (tid >> 3);
        const bool ok = unit < a.bit_words;
        const uint32_t row = ok ? unit / a.bpr : 0u, w = ok ? unit - row * a.bpr : 0u;
        const uint32_t ry = row % a.n[1], rz = row / a.n[1];
        const int32_t r0 = (int32_t)(32u * w + 4u * sub) - (int32_t)a.head;      // the lane's voxels: r0 .. r0 + 3 of the row
        uint32_t nibble = 0u;
        if (ok && r0 + 4 > 0 && r0 < (int32_t)n0) {
            const size_t rowoff = box_row_offset(a, ry, rz);
            uint32_t lab[4] = {0u, 0u, 0u, 0u};
            float val[4] = {0.0f, 0.0f, 0.0f, 0.0f}; uint32_t have = 0u;
            BOX_GATHER(T, LEVEL, a, ring, n0, rowoff, r0, val, lab, have);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (have & (1u << j)) {
                    bool in;
                    BOX_INSIDE(in, LEVEL, cache, val[j], lab[j], a.level, ring_in_set(a.sel, a.nsel, lab[j]));
                    if (in) nibble |= 1u << j;
                }
            }
        }
        count += (uint32_t)__popc(nibble);
        uint32_t word = nibble << (4u * sub);
        word |= (uint32_t)__shfl_xor((int)word, 1);
        word |= (uint32_t)__shfl_xor((int)word, 2);
        word |= (uint32_t)__shfl_xor((int)word, 4);
        if (ok && sub == 0u) a.bits[unit] = word;
    }
    BOX_WAVE_ADD(&a.header[7], count);
}

// ---- classify: the words of cells ---------------------------------------------------------------------------------------
// bits o .. o + 16 of a row of the bit map (o >= -1; bit -1 and the bits beyond the row are zero)
__device__ __forceinline__ uint32_t mesh_window(const uint32_t* row, int32_t o, uint32_t bpr) {
    const uint32_t at = o < 0 ? 0u : (uint32_t)o, idx = at >> 5, sh = at & 31u;
    unsigned long long v = idx < bpr ? row[idx] : 0u;
    if (idx + 1u < bpr) v |= (unsigned long long)row[idx + 1u] << 32;
    uint32_t w = (uint32_t)(v >> sh);
    if (o < 0) w <<= 1;
    return w & 0x1FFFFu;
}

// bit i of b (16 bits) to bit 4 i
__device__ __forceinline__ unsigned long long mesh_spread(uint32_t b) {
    unsigned long long x = b & 0xFFFFu;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

__global__ __launch_bounds__(kMeshThreads) void mesh_classify_kernel(const MeshArgs a) {
    const uint32_t word = blockIdx.x * kMeshThreads + threadIdx.x;
    if (word >= a.words) return;
    const uint32_t row = word / a.wpr, xw = word - row * a.wpr;
    const uint32_t cy = row % a.cells[1], cz = row / a.cells[1];
    // cell ci of the row has its corners at voxels ci - 1 and ci of the box's row: bits ci - 1 + head and ci + head
    const int32_t o = (int32_t)(16u * xw + a.head) - 1;
    uint32_t c0[4], c1[4];                                  // by dy + 2 dz: the corners at dx = 0 and dx = 1 of the word's 16 cells
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t ry = cy + (uint32_t)(j & 1) - 1u, rz = cz + (uint32_t)(j >> 1) - 1u;    // 0xFFFFFFFF: before the box
        uint32_t w = 0u;
        if (ry < a.n[1] && rz < a.n[2]) w = mesh_window(a.bits + ((size_t)rz * a.n[1] + ry) * a.bpr, o, a.bpr);
        c0[j] = w & 0xFFFFu; c1[j] = w >> 1;
    }
    const uint32_t any = c0[0] | c0[1] | c0[2] | c0[3] | c1[0] | c1[1] | c1[2] | c1[3];
    const uint32_t all = c0[0] & c0[1] & c0[2] & c0[3] & c1[0] & c1[1] & c1[2] & c1[3];
    const uint32_t active = any & ~all;
    const uint32_t ex = c0[0] ^ c1[0], ey = c0[0] ^ c0[1], ez = c0[0] ^ c0[2];
    a.nib[word] = mesh_spread(ex) | (mesh_spread(ey) << 1) | (mesh_spread(ez) << 2) | (mesh_spread(active) << 3);
    a.cnt[word] = make_uint2((uint32_t)__popc(active), (uint32_t)(__popc(ex) + __popc(ey) + __popc(ez)));
}

// ---- scan ---------------------------------------------------------------------------------------------------------------
// What the top level of the scan (box_scan.h) does with the totals: V, T = 2 x quads, what a call with these capacities
// writes, and the window offset, into header[0 .. 6].
struct MeshTop {
    unsigned long long* header;
    unsigned long long vcap, tcap;
    int32_t off[3];
    __device__ void operator()(uint2 total) const {
        const unsigned long long V = total.x, T = 2ull * total.y;
        const bool fits = V <= vcap && T <= tcap;
        header[0] = V; header[1] = T;
        header[2] = fits ? V : 0ull; header[3] = fits ? T : 0ull;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) header[4 + ax] = (unsigned long long)(long long)off[ax];
    }
};

// ---- emit ---------------------------------------------------------------------------------------------------------------
// inside(voxel (rx, ry, rz) of the box), from the bit map; coordinates outside the box (negative ones wrapped) are outside
__device__ __forceinline__ uint32_t mesh_bit(const MeshArgs& a, uint32_t rx, uint32_t ry, uint32_t rz) {
    if (rx >= a.n[0] || ry >= a.n[1] || rz >= a.n[2]) return 0u;
    const uint32_t b = rx + a.head;
    return (a.bits[((size_t)rz * a.n[1] + ry) * a.bpr + (b >> 5)] >> (b & 31u)) & 1u;
}

// the vertex index of cell (kx, ky, kz), which is active
__device__ __forceinline__ uint32_t mesh_vertex_index(const MeshArgs& a, uint32_t kx, uint32_t ky, uint32_t kz) {
    const size_t wd = ((size_t)kz * a.cells[1] + ky) * a.wpr + (kx >> 4);
    const unsigned long long below = (1ull << (4u * (kx & 15u))) - 1ull;
    return a.cnt[wd].x + (uint32_t)__popcll(a.nib[wd] & kActiveBits & below);
}

__device__ __forceinline__ bool mesh_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

template <typename T, bool LEVEL>
__global__ __launch_bounds__(kMeshThreads) void mesh_emit_kernel(const MeshArgs a) {
    const uint32_t gid = blockIdx.x * kMeshThreads + threadIdx.x;       // a thread per cell of the padded rows
    const uint32_t word = gid >> 4, j = gid & 15u;
    if (word >= a.words) return;
    if (a.header[0] > a.vcap || a.header[1] > a.tcap) return;
    const unsigned long long w = a.nib[word];
    const uint32_t nb = (uint32_t)(w >> (4u * j)) & 15u;
    if (nb == 0u) return;
    const uint32_t row = word / a.wpr, xw = word - row * a.wpr;
    const uint32_t c[3] = {16u * xw + j, row % a.cells[1], row / a.cells[1]};     // the cell; its first corner is voxel c - 1 of the box
    const unsigned long long below = (1ull << (4u * j)) - 1ull;
    const uint2 base = a.cnt[word];
    const uint32_t vi = base.x + (uint32_t)__popcll(w & kActiveBits & below);

    // corner d = dx + 2 dy + 4 dz
    uint32_t in8 = 0u;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        in8 |= mesh_bit(a, c[0] + (uint32_t)(d & 1) - 1u, c[1] + (uint32_t)((d >> 1) & 1) - 1u, c[2] + (uint32_t)(d >> 2) - 1u) << d;

    if (nb & 8u) {
        float val[8];
        uint32_t usable = 0u;                               // LEVEL: the corners in the box whose value is finite
        if (LEVEL) {
            const T* const ring = static_cast<const T*>(a.density);
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const uint32_t rx = c[0] + (uint32_t)(d & 1) - 1u, ry = c[1] + (uint32_t)((d >> 1) & 1) - 1u, rz = c[2] + (uint32_t)(d >> 2) - 1u;
                val[d] = 0.0f;
                if (rx < a.n[0] && ry < a.n[1] && rz < a.n[2]) {
                    val[d] = (float)ring[box_row_offset(a, ry, rz) + box_slot(a.s0[0], rx, a.ring[0])];
                    if (mesh_finite(val[d])) usable |= 1u << d;
                }
            }
        }
        // the crossing points, summed in the header's order: axis x, y, z; within an axis by the offsets on the two
        // other axes, the higher axis the major key
        float sum[3] = {0.0f, 0.0f, 0.0f};
        uint32_t k = 0u;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const int lowax = ax == 0 ? 1 : 0, highax = ax == 2 ? 1 : 2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d0 = ((e & 1) << lowax) | ((e >> 1) << highax), d1 = d0 | (1 << ax);
                if (((in8 >> d0) ^ (in8 >> d1)) & 1u) {
                    float t = 0.5f;
                    if (LEVEL && ((usable >> d0) & (usable >> d1) & 1u)) {
                        const float r = (a.level - val[d0]) / (val[d1] - val[d0]);
                        if (mesh_finite(r)) t = fminf(fmaxf(r, 0.0f), 1.0f);
                    }
                    float pt[3];
                    pt[ax] = t; pt[lowax] = (float)(e & 1); pt[highax] = (float)(e >> 1);
                    sum[0] = sum[0] + pt[0]; sum[1] = sum[1] + pt[1]; sum[2] = sum[2] + pt[2];
                    ++k;
                }
            }
        }
        const float fk = (float)k;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
            a.vertices[3ull * vi + ax] = (float)(a.rel[ax] + (int32_t)c[ax] - 1) + sum[ax] / fk;
    }

    const uint32_t edges = nb & 7u;
    if (edges) {
        const uint32_t q0 = base.y + (uint32_t)__popcll(w & kEdgeBits & below);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!(edges & (1u << ax))) continue;
            const int b = (ax + 1) % 3, cc = (ax + 2) % 3;
            // no edge crosses on the low border of the cell range (include/svr.h); a cell that did would be left out
            if (c[b] == 0u || c[cc] == 0u) continue;
            const uint32_t qi = q0 + (uint32_t)__popc(edges & ((1u << ax) - 1u));
            uint32_t kk[3] = {c[0], c[1], c[2]};
            kk[b] -= 1u;
            const uint32_t k3 = mesh_vertex_index(a, kk[0], kk[1], kk[2]);
            kk[cc] -= 1u;
            const uint32_t k0 = mesh_vertex_index(a, kk[0], kk[1], kk[2]);
            kk[b] += 1u;
            const uint32_t k1 = mesh_vertex_index(a, kk[0], kk[1], kk[2]);
            const bool out_pos = (in8 & 1u) != 0u;              // inside(p): the normal +a points out of the object
            const int32_t v0 = (int32_t)k0, v1 = (int32_t)(out_pos ? k1 : k3), v2 = (int32_t)vi, v3 = (int32_t)(out_pos ? k3 : k1);
            int2* const t = reinterpret_cast<int2*>(a.triangles + 6ull * qi);       // 24 qi bytes: 8-byte aligned
            t[0] = make_int2(v0, v1); t[1] = make_int2(v2, v0); t[2] = make_int2(v2, v3);
        }
    }
}

template <typename T, bool LEVEL>
void mesh_launch_typed(const MeshArgs& a, uint32_t inside_blocks, bool emit, hipStream_t stream, int step) {
    if (step == 0) hipLaunchKernelGGL((mesh_inside_kernel<T, LEVEL>), dim3(inside_blocks), dim3(kMeshThreads), 0, stream, a);
    else if (emit) {
        const uint64_t threads = (uint64_t)a.words * kMeshCellsPerWord;
        hipLaunchKernelGGL((mesh_emit_kernel<T, LEVEL>), dim3((unsigned)((threads + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0,
                           stream, a);
    }
}

void mesh_launch_step(const MeshArgs& a, int storage, bool level, uint32_t inside_blocks, bool emit, hipStream_t stream, int step) {
    if (!level)                    mesh_launch_typed<uint8_t, false>(a, inside_blocks, emit, stream, step);   // the density ring is not read
    else if (storage == SVR_U8)    mesh_launch_typed<uint8_t, true>(a, inside_blocks, emit, stream, step);
    else if (storage == SVR_U16)   mesh_launch_typed<uint16_t, true>(a, inside_blocks, emit, stream, step);
    else                           mesh_launch_typed<float, true>(a, inside_blocks, emit, stream, step);
}

}  // namespace

// lo: the first voxel of the box (box and window intersected) in logical voxels of the LOD; plan: mesh_plan of its
// extent, or null for an empty box; scratch: plan->bytes of device memory no other call is using.  Everything was
// validated by svr_mesh.
hipError_t svr_launch_mesh(const svr_ctx* c, int lod, const int64_t lo[3], const MeshPlan* plan, int mode, float level,
                           const uint32_t* sel, uint32_t nsel, void* scratch, const svr_mesh_outputs& out, hipStream_t stream) {
    const LodStorage& L = c->lod[lod];
    const svr_lod_state& st = L.state;
    unsigned long long* const header = reinterpret_cast<unsigned long long*>(out.header);
    const MeshTop top = {header, out.vertex_capacity, out.triangle_capacity, {st.offset[0], st.offset[1], st.offset[2]}};
    hipError_t e = hipMemsetAsync(header, 0, 8 * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    if (!plan) return box_scan_run<uint2>(nullptr, nullptr, top, stream);      // the empty mesh: the header alone
    const MeshPlan& p = *plan;
    char* const base = static_cast<char*>(scratch);
    MeshArgs a;
    a.density = L.density; a.labels = L.labels;
    for (int ax = 0; ax < 3; ++ax) {
        a.ring[ax] = (uint32_t)L.ring[ax];
        a.n[ax] = p.n[ax]; a.cells[ax] = p.cells[ax];
        a.s0[ax] = (uint32_t)(lo[ax] % (int64_t)L.ring[ax]);
        a.rel[ax] = (int32_t)(lo[ax] - (int64_t)st.offset[ax]);
    }
    a.wpr = p.wpr; a.words = p.words; a.head = p.head; a.bpr = p.bpr; a.bit_words = p.bit_words;
    a.level = level; a.sel = sel; a.nsel = nsel;
    a.bits = reinterpret_cast<uint32_t*>(base + p.bit_off);
    a.nib = reinterpret_cast<unsigned long long*>(base + p.nib_off);
    a.cnt = reinterpret_cast<uint2*>(base + p.scan.off[0]);
    a.header = header;
    a.vertices = out.vertices; a.triangles = out.triangles;
    a.vcap = out.vertex_capacity; a.tcap = out.triangle_capacity;
    const bool is_level = mode == SVR_MESH_LEVEL;

    // inside: 32 words of bits per workgroup and round, 8 workgroups per CU at the most
    const uint64_t want = ((uint64_t)p.bit_words + kMeshThreads / 8 - 1) / (kMeshThreads / 8);
    const uint64_t most = ring_workgroups(c->device, 8);
    mesh_launch_step(a, c->density_storage, is_level, (uint32_t)(want < most ? want : most), false, stream, 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mesh_classify_kernel, dim3((p.words + kMeshThreads - 1) / kMeshThreads), dim3(kMeshThreads), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    if ((e = box_scan_run<uint2>(&p.scan, scratch, top, stream)) != hipSuccess) return e;
    // the count-only call, and one that cannot fit, skip the last kernel
    const bool emit = out.vertex_capacity > 0 && out.triangle_capacity > 0;
    mesh_launch_step(a, c->density_storage, is_level, 0u, emit, stream, 1);
    return hipGetLastError();
}
