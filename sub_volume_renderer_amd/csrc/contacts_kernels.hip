// Contacts between resident objects (svr_contacts, include/svr.h): one streaming pass over the label ring of a box of
// one LOD's window that fills an open-addressed table of records, one per unordered pair of touching labels.  gfx950.
//
// Decomposition.  The row units of box_units.h: a lane owns 4 consecutive ring slots at a multiple of 4 of one row of
// the box, BOX_GATHER reads them (a row's head and tail and the slot the wrap seam cuts element by element), and the two
// neighbour rows (ry + 1, rz) and (ry, rz + 1) come through box_row_offset, which follows the ring's wrap.  Units are
// numbered row by row; a workgroup of kConThreads threads takes one contiguous share of them, kConThreads at a time, so
// consecutive lanes hold consecutive units: the voxel after a unit in x is the next lane's first (one __shfl_down) and
// one element load where the next lane is in another wave.
//
// Faces.  con_unit_updates (contacts_faces.h) turns a unit into merged updates: per axis, the faces of one label pair
// are one update whose count, coordinate sums and extremes are arithmetic on its mask.  Most units own no face: a wave
// in which no lane owns one goes on after the three label gathers, and the density ring is read only by lanes that do.
//
// Tables.  object_kernels.hip's, keyed by the pair: a workgroup table in LDS (kConLdsSlots slots, structure of arrays,
// the 64-bit key claimed by CAS, at most kConLdsProbes probes) that is flushed once at the end into the caller's
// records; a pair that finds no LDS slot goes to the records at once.  The first 8 bytes of a record are its key,
// claimed by a CAS of 0 -> key with linear probing over the WHOLE table.  Every field only grows from 0: minima travel
// complemented under atomicMax, so an unclaimed record stays all-zero.  con_finish_kernel decodes the extremes, counts
// the occupied records and writes the rest of the header.  The only float atomic is the f64 value_sum of float32 rings.
#include "svr_host.h"
#include "box_units.h"
#include "contacts_faces.h"

static_assert(sizeof(svr_contact_record) == 112, "svr_contact_record is 112 bytes");

namespace {

constexpr int kConThreads = 256;             // units of one step of a workgroup's loop
constexpr uint32_t kConLdsSlots = 512;       // 44 KB of LDS per workgroup: three workgroups per CU
constexpr uint32_t kConLdsProbes = 8;
constexpr uint64_t kConWgPerCu = 3;
constexpr uint32_t kConMinSteps = 16;        // steps per workgroup at least: the flush costs ~20 global atomics per pair

struct ConArgs {
    const void* density;
    const uint32_t* labels;    // never null: without label rings there is no face and no launch
    uint32_t ring[3];
    uint32_t n[3];             // extent of the box B
    uint32_t s0[3];            // ring slot of B's first voxel
    int32_t lo[3];             // B's first voxel
    int32_t rel[3];            // B's first voxel minus the window offset
    uint32_t head, upr;
    unsigned long long units, share;
    const uint32_t* sel;
    uint32_t nsel;
    int32_t ignore_zero;
    svr_contact_record* records;
    uint32_t capacity;
    unsigned long long* header;
};

// what a record holds during the pass.  Same layout as svr_contact_record; lo / hi / vmin / vmax are keys that only grow
struct ConRaw {
    unsigned long long key;            // label_lo | label_hi << 32
    unsigned long long faces[3];
    unsigned long long sum2[3];
    uint32_t lok[3], hik[3];
    unsigned long long finite;
    unsigned long long value_sum;
    uint32_t vmink, vmaxk;
    unsigned long long reserved;
};
static_assert(sizeof(ConRaw) == 112, "ConRaw mirrors svr_contact_record");

// keys with identity 0 under max: a minimum travels complemented
__device__ __forceinline__ uint32_t con_lo_key(int32_t v) { return ~((uint32_t)v ^ 0x80000000u); }
__device__ __forceinline__ uint32_t con_hi_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int32_t con_lo_of_key(uint32_t k) { return (int32_t)(~k ^ 0x80000000u); }
__device__ __forceinline__ int32_t con_hi_of_key(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

// one update, or one LDS slot at the flush: what is added to a record
struct ConRun {
    unsigned long long key;
    uint32_t faces[3];                 // a workgroup sees fewer than 2^32 faces
    unsigned long long s[3];
    uint32_t lok[3], hik[3];
    uint32_t fin;
    unsigned long long vsum;           // u64 sum, or the bits of an f64 sum
    uint32_t vmink, vmaxk;             // complemented min key, max key; 0: none
};

// ---- the global table ------------------------------------------------------------------------------------------
// the record of `key`, claimed if need be; null when every record belongs to another pair
__device__ __forceinline__ ConRaw* con_global_slot(ConRaw* records, uint32_t capacity, unsigned long long key) {
    uint32_t i = (uint32_t)(((unsigned long long)con_hash(key) * capacity) >> 32);       // < capacity
    for (uint32_t probe = 0; probe < capacity; ++probe) {
        unsigned long long* const kp = &records[i].key;
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(kp, 0ull, key);
        if (cur == 0ull || cur == key) return &records[i];
        i = i + 1u < capacity ? i + 1u : 0u;
    }
    return nullptr;
}

__device__ __forceinline__ void con_global_max(uint32_t* p, uint32_t k) {
    if (k != 0u && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k) atomicMax(p, k);
}

template <bool F32>
__device__ __forceinline__ void con_global_add(const ConArgs& a, const ConRun& r) {
    ConRaw* const rec = con_global_slot(reinterpret_cast<ConRaw*>(a.records), a.capacity, r.key);
    if (!rec) { atomicAdd(&a.header[2], (unsigned long long)r.faces[0] + r.faces[1] + r.faces[2]); return; }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (r.faces[ax]) atomicAdd(&rec->faces[ax], (unsigned long long)r.faces[ax]);
        if (r.s[ax]) atomicAdd(&rec->sum2[ax], r.s[ax]);
        con_global_max(&rec->lok[ax], r.lok[ax]);
        con_global_max(&rec->hik[ax], r.hik[ax]);
    }
    if (r.fin) {
        atomicAdd(&rec->finite, (unsigned long long)r.fin);
        if (F32) unsafeAtomicAdd(reinterpret_cast<double*>(&rec->value_sum), __longlong_as_double((long long)r.vsum));
        else if (r.vsum) atomicAdd(&rec->value_sum, r.vsum);
        con_global_max(&rec->vmink, r.vmink);
        con_global_max(&rec->vmaxk, r.vmaxk);
    }
}

// ---- the workgroup's table --------------------------------------------------------------------------------------
struct ConLds {
    unsigned long long key[kConLdsSlots];
    unsigned long long sum2[3][kConLdsSlots];
    unsigned long long vsum[kConLdsSlots];
    uint32_t faces[3][kConLdsSlots], fin[kConLdsSlots];
    uint32_t lok[3][kConLdsSlots], hik[3][kConLdsSlots];
    uint32_t vmink[kConLdsSlots], vmaxk[kConLdsSlots];
};

__device__ __forceinline__ void con_lds_max(uint32_t* p, uint32_t k) {
    if (k != 0u && *reinterpret_cast<volatile uint32_t*>(p) < k) atomicMax(p, k);
}

// false: no slot within kConLdsProbes
template <bool F32>
__device__ __forceinline__ bool con_lds_add(ConLds& t, const ConRun& r) {
    uint32_t i = con_hash(r.key) & (kConLdsSlots - 1u);
    bool found = false;
    for (uint32_t probe = 0; probe < kConLdsProbes; ++probe) {
        unsigned long long cur = *reinterpret_cast<volatile unsigned long long*>(&t.key[i]);
        if (cur == 0ull) cur = atomicCAS(&t.key[i], 0ull, r.key);
        if (cur == 0ull || cur == r.key) { found = true; break; }
        i = (i + 1u) & (kConLdsSlots - 1u);
    }
    if (!found) return false;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (r.faces[ax]) atomicAdd(&t.faces[ax][i], r.faces[ax]);
        if (r.s[ax]) atomicAdd(&t.sum2[ax][i], r.s[ax]);
        con_lds_max(&t.lok[ax][i], r.lok[ax]);
        con_lds_max(&t.hik[ax][i], r.hik[ax]);
    }
    if (r.fin) {
        if (F32) {
            atomicAdd(&t.fin[i], r.fin);
            atomicAdd(reinterpret_cast<double*>(&t.vsum[i]), __longlong_as_double((long long)r.vsum));
        } else if (r.vsum) {
            atomicAdd(&t.vsum[i], r.vsum);              // integer rings: finite == 2 * faces, set at the flush
        }
        con_lds_max(&t.vmink[i], r.vmink);
        con_lds_max(&t.vmaxk[i], r.vmaxk);
    }
    return true;
}

// the values a face offers, gathered into an update
template <bool F32> struct ConValues {
    uint32_t fin = 0u, isum = 0u, vmink = 0u, vmaxk = 0u;
    double dsum = 0.0;
    __device__ __forceinline__ void offer(float v) {
        if (F32) {
            if ((__float_as_uint(v) & 0x7F800000u) == 0x7F800000u) return;         // NaN, +-inf
            dsum += (double)v;
        } else {
            isum += (uint32_t)v;                                                   // 8 x 65535 fits
        }
        ++fin;
        const uint32_t k = ring_key_of_float(v);
        vmink = max(vmink, ~k); vmaxk = max(vmaxk, k);
    }
};

template <typename T>
__global__ __launch_bounds__(kConThreads) void con_kernel(const ConArgs a) {
    constexpr bool F32 = sizeof(T) == 4;
    __shared__ ConLds t;
    const uint32_t tid = threadIdx.x;
    {
        uint32_t* const w = reinterpret_cast<uint32_t*>(&t);
        for (uint32_t k = tid; k < sizeof(ConLds) / 4u; k += kConThreads) w[k] = 0u;
    }
    __syncthreads();

    const T* const ring = static_cast<const T*>(a.density);
    const uint32_t n0 = a.n[0];
    const uint32_t lane = __lane_id();
    const bool filter = a.nsel > 0u, drop_zero = a.ignore_zero != 0;
    uint32_t considered = 0u, zeros = 0u;                  // this lane's: a workgroup sees fewer than 2^32 faces
    uint32_t last_label = 0u; bool last_in = false, have_last = false;

    const unsigned long long u0 = (unsigned long long)blockIdx.x * a.share;
    const unsigned long long u1 = min(a.units, u0 + a.share);
    const bool narrow = a.units <= 0xFFFFFFFFull;          // then the row of a unit is a 32-bit division
    for (unsigned long long base = u0; base < u1; base += kConThreads) {          // wave-uniform trip counts
        const unsigned long long unit = base + tid;
        const bool active = unit < u1;
        uint32_t row = 0u, w = 0u;
        if (active) {
            if (narrow) { row = (uint32_t)unit / a.upr; w = (uint32_t)unit - row * a.upr; }
            else        { row = (uint32_t)(unit / a.upr); w = (uint32_t)(unit - (unsigned long long)row * a.upr); }
        }
        const uint32_t ry = row % a.n[1], rz = row / a.n[1];
        const int32_t r0 = (int32_t)(4u * w) - (int32_t)a.head;                 // the lane's voxels: r0 .. r0 + 3 of the row
        const size_t rowoff = box_row_offset(a, ry, rz);
        const bool has_y = active && ry + 1u < a.n[1], has_z = active && rz + 1u < a.n[2];
        const size_t rowoff_y = has_y ? box_row_offset(a, ry + 1u, rz) : rowoff;
        const size_t rowoff_z = has_z ? box_row_offset(a, ry, rz + 1u) : rowoff;

        ConUnit u = {};
        float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (active) BOX_GATHER(T, false, a, ring, n0, rowoff, r0, none, u.lab, u.have);
        if (has_y) BOX_GATHER(T, false, a, ring, n0, rowoff_y, r0, none, u.ylab, u.yhave);
        if (has_z) BOX_GATHER(T, false, a, ring, n0, rowoff_z, r0, none, u.zlab, u.zhave);
        // the voxel after the unit in x: in the row it is the next unit's first, which the next lane holds
        const uint32_t next_first = (uint32_t)__shfl_down((int)u.lab[0], 1);
        const bool xhave = active && r0 + 4 < (int32_t)n0;
        size_t xe = 0;
        if (xhave) {
            xe = rowoff + box_slot(a.s0[0], (uint32_t)(r0 + 4), a.ring[0]);
            u.xhave = 1u;
            u.xlab = (lane != 63u && unit + 1ull < u1) ? next_first : a.labels[xe];
        }

        const bool any = con_unit_any(u);
        if (!__ballot(any)) continue;                                           // wave-uniform: most waves own no face
        if (!any) continue;

        // the values of the unit; those across its faces are read face by face
        float pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        {
            uint32_t lab_none[4], have_again = 0u;
            BOX_GATHER(T, true, a, ring, n0, rowoff, r0, pv, lab_none, have_again);
        }
        const int32_t xr = a.rel[0] + r0, yr = a.rel[1] + (int32_t)ry, zr = a.rel[2] + (int32_t)rz;    // relative to the window offset
        con_unit_updates(u,
            [&](uint64_t key) {
                if (filter) {
                    bool in = false;
                    const uint32_t pair[2] = {con_key_lo(key), con_key_hi(key)};
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        if (!have_last || pair[e] != last_label) {
                            last_in = ring_in_set(a.sel, a.nsel, pair[e]); last_label = pair[e]; have_last = true;
                        }
                        in = in || last_in;
                    }
                    if (!in) return false;
                }
                if (drop_zero && con_key_lo(key) == 0u) { ++zeros; return false; }
                ++considered;
                return true;
            },
            [&](int axis, uint64_t key, uint32_t m) {
                ConRun r;
                r.key = key;
                const uint32_t n = con_mask_count(m);
                r.faces[0] = axis == 0 ? n : 0u; r.faces[1] = axis == 1 ? n : 0u; r.faces[2] = axis == 2 ? n : 0u;
                // twice the face centres: 2 * (p - off) + e_axis, p.x = xr + j over the mask
                const long long sx = 2ll * ((long long)n * xr + (long long)con_mask_sum(m)) + (axis == 0 ? (long long)n : 0ll);
                r.s[0] = (unsigned long long)sx;
                r.s[1] = (unsigned long long)n * (unsigned long long)(2 * yr + (axis == 1 ? 1 : 0));
                r.s[2] = (unsigned long long)n * (unsigned long long)(2 * zr + (axis == 2 ? 1 : 0));
                r.lok[0] = con_lo_key(a.lo[0] + r0 + (int32_t)con_mask_first(m)); r.hik[0] = con_hi_key(a.lo[0] + r0 + (int32_t)con_mask_last(m));
                r.lok[1] = con_lo_key(a.lo[1] + (int32_t)ry); r.hik[1] = con_hi_key(a.lo[1] + (int32_t)ry);
                r.lok[2] = con_lo_key(a.lo[2] + (int32_t)rz); r.hik[2] = con_hi_key(a.lo[2] + (int32_t)rz);
                ConValues<F32> v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!(m >> j & 1u)) continue;
                    v.offer(pv[j]);
                    if (axis == 0) v.offer(j < 3 ? pv[j < 3 ? j + 1 : 3] : (float)ring[xe]);
                    else v.offer((float)ring[(axis == 1 ? rowoff_y : rowoff_z) + box_slot(a.s0[0], (uint32_t)(r0 + j), a.ring[0])]);
                }
                r.fin = v.fin; r.vmink = v.vmink; r.vmaxk = v.vmaxk;
                r.vsum = F32 ? (unsigned long long)__double_as_longlong(v.dsum) : (unsigned long long)v.isum;
                if (!con_lds_add<F32>(t, r)) con_global_add<F32>(a, r);
            });
    }

    BOX_WAVE_ADD2(&a.header[1], considered, &a.header[3], zeros);
    __syncthreads();
    for (uint32_t i = tid; i < kConLdsSlots; i += kConThreads) {
        const unsigned long long key = t.key[i];
        if (key == 0ull) continue;
        ConRun r;
        r.key = key;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { r.faces[ax] = t.faces[ax][i]; r.s[ax] = t.sum2[ax][i]; r.lok[ax] = t.lok[ax][i]; r.hik[ax] = t.hik[ax][i]; }
        r.fin = F32 ? t.fin[i] : 2u * (r.faces[0] + r.faces[1] + r.faces[2]);
        r.vsum = t.vsum[i];
        r.vmink = t.vmink[i]; r.vmaxk = t.vmaxk[i];
        con_global_add<F32>(a, r);
    }
}

// the last step: extremes decoded in place, occupied records counted, the header's offsets and voxel count written
__global__ __launch_bounds__(256) void con_finish_kernel(svr_contact_record* records, uint32_t capacity, unsigned long long* header,
                                                         int32_t ox, int32_t oy, int32_t oz, unsigned long long voxels) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool used = false;
    if (i < capacity) {
        ConRaw* const r = reinterpret_cast<ConRaw*>(records) + i;
        used = r->key != 0ull;
        if (used) {
            svr_contact_record* const o = records + i;
            int32_t lo[3], hi[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { lo[ax] = con_lo_of_key(r->lok[ax]); hi[ax] = con_hi_of_key(r->hik[ax]); }
            const uint32_t kmin = ~r->vmink, kmax = r->vmaxk;
            const bool any = r->finite != 0ull;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { o->lo[ax] = lo[ax]; o->hi[ax] = hi[ax]; }
            o->vmin = any ? ring_float_of_key(kmin) : __builtin_inff();
            o->vmax = any ? ring_float_of_key(kmax) : -__builtin_inff();
        }
    }
    const unsigned long long m = __ballot(used);
    if (__lane_id() == 0u && m) atomicAdd(&header[0], (unsigned long long)__popcll(m));
    if (i == 0) {
        header[4] = (unsigned long long)(long long)ox;
        header[5] = (unsigned long long)(long long)oy;
        header[6] = (unsigned long long)(long long)oz;
        header[7] = voxels;
    }
}

}  // namespace

// lo[a] .. lo[a] + n[a]: the intersection of box and window in logical voxels of the LOD (n may hold a value <= 0: there is
// no voxel and no face).  Everything was validated by svr_contacts.
hipError_t svr_launch_contacts(const svr_ctx* c, int lod, const int64_t lo[3], const int64_t n[3], const uint32_t* sel, uint32_t nsel,
                               int ignore_zero, uint32_t capacity, const svr_contacts_outputs& out, hipStream_t stream) {
    const LodStorage& L = c->lod[lod];
    const svr_lod_state& st = L.state;
    unsigned long long* header = reinterpret_cast<unsigned long long*>(out.header);
    hipError_t e = hipMemsetAsync(out.records, 0, (size_t)capacity * sizeof(svr_contact_record), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(header, 0, 8 * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;

    const bool any = n[0] > 0 && n[1] > 0 && n[2] > 0;
    const unsigned long long voxels = any ? (unsigned long long)n[0] * (unsigned long long)n[1] * (unsigned long long)n[2] : 0ull;
    if (any && L.labels) {                                  // without label rings every label reads 0: no face
        ConArgs a;
        a.density = L.density; a.labels = L.labels;
        for (int ax = 0; ax < 3; ++ax) {
            a.ring[ax] = (uint32_t)L.ring[ax];
            a.n[ax] = (uint32_t)n[ax];
            a.s0[ax] = (uint32_t)(lo[ax] % (int64_t)L.ring[ax]);
            a.lo[ax] = (int32_t)lo[ax];
            a.rel[ax] = (int32_t)(lo[ax] - (int64_t)st.offset[ax]);
        }
        const ConPlan plan = con_plan(n, box_head(lo[0], a.ring[0]), (uint32_t)kConThreads, kConMinSteps, ring_workgroups(c->device, kConWgPerCu));
        a.head = plan.head; a.upr = plan.upr; a.units = plan.units; a.share = plan.share;
        a.sel = sel; a.nsel = nsel; a.ignore_zero = ignore_zero;
        a.records = out.records; a.capacity = capacity; a.header = header;
        const dim3 grid(plan.blocks), block(kConThreads);
        if (c->density_storage == SVR_U8)       hipLaunchKernelGGL(con_kernel<uint8_t>, grid, block, 0, stream, a);
        else if (c->density_storage == SVR_U16) hipLaunchKernelGGL(con_kernel<uint16_t>, grid, block, 0, stream, a);
        else                                    hipLaunchKernelGGL(con_kernel<float>, grid, block, 0, stream, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(con_finish_kernel, dim3((unsigned)(((size_t)capacity + 255) / 256)), dim3(256), 0, stream, out.records, capacity,
                       header, st.offset[0], st.offset[1], st.offset[2], voxels);
    return hipGetLastError();
}
