// Per-object measurements of the resident rings (svr_objects, include/svr.h): one streaming pass over a box of one
// LOD's window that fills an open-addressed table of records, one per label.  gfx950.
//
// Decomposition.  The histogram's, stated once in ring_pieces.h: the host cuts box and window at the ring's wrap seams
// into at most 2 x 2 x 2 dense pieces; a workgroup of 256 threads takes a run of whole rows of one piece; element
// offsets are 64-bit.  A lane owns one slot of 4 consecutive voxels, aligned to 16 bytes of the LABEL ring: a slot
// wholly inside the row is one 16-byte label load and one 4 / 8 / 16-byte density load, the slots at the row's head
// and tail read their own elements one by one.  2^k lanes share a row, as in the histogram.
//
// Merging before any atomic.  A lane's 4 voxels collapse into runs of equal labels (geometry of a run is arithmetic:
// its x span gives count, sum, min and max; y and z are the row's).  A lane whose slot is one label ("solid") joins
// its solid neighbours of the same row and label: a segmented reduction over the lanes of the wave (segment ends from
// one ballot; only the value fields travel, the merged x span is arithmetic again), and only the segment's first lane
// goes further.  Waves without two such neighbours skip the reduction.
//
// Tables.  A run goes to the workgroup's LDS table (512 slots, a 64-bit "occupied | label" key claimed by CAS, then
// adds and maxima; at most kLdsProbes probes), which is flushed to the global table once at the end; a label that finds
// no LDS slot goes to the global table at once.  The global table is the caller's records: the first 8 bytes of a
// record (label, used) are the key, claimed by a 64-bit CAS of 0 -> (1 << 32 | label), with linear probing over the
// WHOLE table, so a label fails only when every record is taken.  Every field is zero-initialised and only grows:
// minima travel as complemented keys under atomicMax, so an untouched record stays all-zero and needs no clean-up.
// obj_finish_kernel decodes the keys of the occupied records, counts them and writes the header's offsets.
// No float atomics except the f64 value_sum of float32 rings; vmin / vmax are u32 keys (ring_pieces.h).
#include <string.h>

#include "svr_host.h"
#include "ring_pieces.h"

static_assert(sizeof(svr_object_record) == 96, "svr_object_record is 96 bytes");

namespace {

constexpr int kObjThreads = 256;
constexpr uint32_t kLdsSlots = 512;          // 40 KB of LDS per workgroup: three workgroups per CU
constexpr uint32_t kLdsProbes = 8;
constexpr uint64_t kObjWgPerCu = 3;
constexpr uint64_t kObjMinShare = 65536;      // bytes read per workgroup at least: the flush costs ~15 global atomics per label
constexpr unsigned long long kUsed = 1ull << 32;

// a piece with the logical coordinate of its first voxel, relative to the window offset, where the kernels' arguments
// have always had it: between extent and rows
struct ObjRel { uint32_t rel[3]; };
struct ObjPiece : RingBox, ObjRel, RingShare {};

struct ObjArgs {
    const void* density;
    const uint32_t* labels;    // null: every label reads as 0
    uint32_t ring[3];
    int32_t off[3];            // the window offset: lo / hi are absolute, the sums relative to it
    const uint32_t* sel;
    uint32_t nsel;
    int32_t ignore_zero;
    svr_object_record* records;
    uint32_t capacity;
    unsigned long long* header;
    int32_t npieces;
    ObjPiece piece[kRingMaxPieces];    // slots of 4 voxels
};

// what a record holds during the pass.  Same layout as svr_object_record; lo / hi / vmin / vmax are keys that only grow
struct ObjRaw {
    unsigned long long key;            // label | used << 32
    unsigned long long voxels;
    unsigned long long sum[3];
    uint32_t lok[3], hik[3];
    unsigned long long finite;
    unsigned long long value_sum;
    uint32_t vmink, vmaxk;
    unsigned long long reserved;
};
static_assert(sizeof(ObjRaw) == 96, "ObjRaw mirrors svr_object_record");

// keys with identity 0 under max: a minimum travels complemented
__device__ __forceinline__ uint32_t lo_key(int32_t v) { return ~((uint32_t)v ^ 0x80000000u); }
__device__ __forceinline__ uint32_t hi_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int32_t lo_of_key(uint32_t k) { return (int32_t)(~k ^ 0x80000000u); }
__device__ __forceinline__ int32_t hi_of_key(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

__device__ __forceinline__ uint32_t obj_hash(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// one run, or one LDS slot at the flush: what is added to a record
template <bool F32> struct ObjRun {
    uint32_t label;
    unsigned long long n;
    unsigned long long s[3];
    uint32_t lok[3], hik[3];
    unsigned long long fin;
    unsigned long long vsum;           // u64 sum, or the bits of an f64 sum
    uint32_t vmink, vmaxk;             // complemented min key, max key; 0: none
};

template <typename T> struct ObjElem;
template <> struct ObjElem<uint8_t> {
    static constexpr bool kF32 = false;
    static __device__ __forceinline__ void load4(const uint8_t* p, uint32_t v[4]) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
        v[0] = q & 0xFFu; v[1] = (q >> 8) & 0xFFu; v[2] = (q >> 16) & 0xFFu; v[3] = q >> 24;
    }
    static __device__ __forceinline__ uint32_t raw1(const uint8_t* p) { return *p; }
};
template <> struct ObjElem<uint16_t> {
    static constexpr bool kF32 = false;
    static __device__ __forceinline__ void load4(const uint16_t* p, uint32_t v[4]) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = q.x & 0xFFFFu; v[1] = q.x >> 16; v[2] = q.y & 0xFFFFu; v[3] = q.y >> 16;
    }
    static __device__ __forceinline__ uint32_t raw1(const uint16_t* p) { return *p; }
};
template <> struct ObjElem<float> {
    static constexpr bool kF32 = true;
    static __device__ __forceinline__ void load4(const float* p, uint32_t v[4]) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ __forceinline__ uint32_t raw1(const float* p) { return __float_as_uint(*p); }
};

__device__ __forceinline__ bool bits_finite(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }

// ---- the global table ------------------------------------------------------------------------------------------
// the record of `label`, claimed if need be; null when every record belongs to another label
__device__ __forceinline__ ObjRaw* obj_global_slot(ObjRaw* records, uint32_t capacity, uint32_t label) {
    const unsigned long long key = kUsed | label;
    uint32_t i = (uint32_t)(((unsigned long long)obj_hash(label) * capacity) >> 32);       // < capacity
    for (uint32_t probe = 0; probe < capacity; ++probe) {
        unsigned long long* const kp = &records[i].key;
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(kp, 0ull, key);
        if (cur == 0ull || cur == key) return &records[i];
        i = i + 1u < capacity ? i + 1u : 0u;
    }
    return nullptr;
}

__device__ __forceinline__ void obj_global_max(uint32_t* p, uint32_t k) {
    if (k != 0u && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k) atomicMax(p, k);
}

template <bool F32>
__device__ __forceinline__ void obj_global_add(const ObjArgs& a, const ObjRun<F32>& r) {
    ObjRaw* const rec = obj_global_slot(reinterpret_cast<ObjRaw*>(a.records), a.capacity, r.label);
    if (!rec) { atomicAdd(&a.header[2], r.n); return; }
    atomicAdd(&rec->voxels, r.n);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (r.s[ax]) atomicAdd(&rec->sum[ax], r.s[ax]);
        obj_global_max(&rec->lok[ax], r.lok[ax]);
        obj_global_max(&rec->hik[ax], r.hik[ax]);
    }
    if (r.fin) {
        atomicAdd(&rec->finite, r.fin);
        if (F32) unsafeAtomicAdd(reinterpret_cast<double*>(&rec->value_sum), __longlong_as_double((long long)r.vsum));
        else if (r.vsum) atomicAdd(&rec->value_sum, r.vsum);
        obj_global_max(&rec->vmink, r.vmink);
        obj_global_max(&rec->vmaxk, r.vmaxk);
    }
}

// ---- the workgroup's table --------------------------------------------------------------------------------------
struct ObjLds {
    unsigned long long key[kLdsSlots];
    unsigned long long sum[3][kLdsSlots];
    unsigned long long vsum[kLdsSlots];
    uint32_t n[kLdsSlots], fin[kLdsSlots];
    uint32_t lok[3][kLdsSlots], hik[3][kLdsSlots];
    uint32_t vmink[kLdsSlots], vmaxk[kLdsSlots];
};

__device__ __forceinline__ void obj_lds_max(uint32_t* p, uint32_t k) {
    if (k != 0u && *reinterpret_cast<volatile uint32_t*>(p) < k) atomicMax(p, k);
}

// false: no slot within kLdsProbes
template <bool F32>
__device__ __forceinline__ bool obj_lds_add(ObjLds& t, const ObjRun<F32>& r) {
    const unsigned long long key = kUsed | r.label;
    uint32_t i = obj_hash(r.label) & (kLdsSlots - 1u);
    bool found = false;
    for (uint32_t probe = 0; probe < kLdsProbes; ++probe) {
        unsigned long long cur = *reinterpret_cast<volatile unsigned long long*>(&t.key[i]);
        if (cur == 0ull) cur = atomicCAS(&t.key[i], 0ull, key);
        if (cur == 0ull || cur == key) { found = true; break; }
        i = (i + 1u) & (kLdsSlots - 1u);
    }
    if (!found) return false;
    atomicAdd(&t.n[i], (uint32_t)r.n);                  // a workgroup sees fewer than 2^32 voxels
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (r.s[ax]) atomicAdd(&t.sum[ax][i], r.s[ax]);
        obj_lds_max(&t.lok[ax][i], r.lok[ax]);
        obj_lds_max(&t.hik[ax][i], r.hik[ax]);
    }
    if (r.fin) {
        if (F32) {
            atomicAdd(&t.fin[i], (uint32_t)r.fin);
            atomicAdd(reinterpret_cast<double*>(&t.vsum[i]), __longlong_as_double((long long)r.vsum));
        } else if (r.vsum) {
            atomicAdd(&t.vsum[i], r.vsum);              // integer rings: finite == voxels, set at the flush
        }
        obj_lds_max(&t.vmink[i], r.vmink);
        obj_lds_max(&t.vmaxk[i], r.vmaxk);
    }
    return true;
}

template <typename T, bool FILT>
__global__ __launch_bounds__(kObjThreads) void obj_kernel(const ObjArgs a) {
    using E = ObjElem<T>;
    constexpr bool F32 = E::kF32;
    __shared__ ObjLds t;
    const uint32_t tid = threadIdx.x;
    {
        uint32_t* const w = reinterpret_cast<uint32_t*>(&t);
        for (uint32_t k = tid; k < sizeof(ObjLds) / 4u; k += kObjThreads) w[k] = 0u;
    }
    __syncthreads();

    RING_WALK(kObjThreads, a, blockIdx.x, tid);
    const uint32_t* const rel = P.rel;
    const uint32_t lane = __lane_id();
    const uint32_t nx = P.n[0];
    const T* const ring = static_cast<const T*>(a.density);

    // without label rings every label is 0: the filter passes everything or nothing
    bool filter = FILT, nothing = false;
    if (FILT && !a.labels) { filter = false; nothing = !ring_in_set(a.sel, a.nsel, 0u); }
    const bool drop_zero = a.ignore_zero != 0;

    uint32_t considered = 0u, zeros = 0u;              // this lane's; a workgroup sees fewer than 2^32 voxels
    uint32_t last_label = 0u; bool last_pass = false, have_last = false;

    if (!nothing)
    for (uint64_t rb = r0; rb < r1; rb += rows_per_iter) {          // wave-uniform trip counts; `row_ok` masks lanes
        const bool row_ok = rb + lane_row < r1;
        const uint32_t row = (uint32_t)(rb + lane_row);
        const uint32_t ry = row_ok ? row % P.n[1] : 0u, rz = row_ok ? row / P.n[1] : 0u;
        const size_t e0 = RING_ROW_OFFSET(P, a.ring, ry, rz);
        const T* const rowp = ring + e0;
        const uint32_t* const lrow = a.labels ? a.labels + e0 : nullptr;
        // elements before the row in its first slot: slots are aligned to 16 bytes of the label ring
        const uint32_t head = a.labels ? (uint32_t)((reinterpret_cast<uintptr_t>(lrow) & 15u) / 4u) : (uint32_t)(e0 & 3u);
        const uint32_t yrel = rel[1] + ry, zrel = rel[2] + rz;
        for (uint32_t sb = 0; sb < P.spr; sb += lpr) {
            const uint32_t slot = sb + lane_slot;
            // the slot holds row elements [first, first + 4), of which [0, nx) exist
            const int64_t first = (int64_t)slot * 4 - (int64_t)head;
            const bool live = row_ok && first < (int64_t)nx && first + 4 > 0;
            const bool full = live && first >= 0 && first + 4 <= (int64_t)nx;
            uint32_t lab[4] = {0u, 0u, 0u, 0u}, val[4] = {0u, 0u, 0u, 0u};
            uint32_t vm = 0u;                                          // which of the slot's 4 voxels are considered
            if (full) {
                vm = 0xFu;
                if (lrow) {
                    const uint4 q = *reinterpret_cast<const uint4*>(lrow + first);
                    lab[0] = q.x; lab[1] = q.y; lab[2] = q.z; lab[3] = q.w;
                }
                const T* const dp = rowp + first;
                if ((reinterpret_cast<uintptr_t>(dp) & (4u * sizeof(T) - 1u)) == 0u) E::load4(dp, val);
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) val[j] = E::raw1(dp + j);
                }
            } else if (live) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t e = first + j;
                    if (e >= 0 && e < (int64_t)nx) {
                        vm |= 1u << j;
                        lab[j] = lrow ? lrow[e] : 0u;
                        val[j] = E::raw1(rowp + e);
                    }
                }
            }
            // the selected filter, then label 0
            if ((filter || drop_zero) && vm) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (vm & (1u << j)) {
                        if (filter) {
                            if (!have_last || lab[j] != last_label) {
                                last_pass = ring_in_set(a.sel, a.nsel, lab[j]); last_label = lab[j]; have_last = true;
                            }
                            if (!last_pass) { vm &= ~(1u << j); continue; }
                        }
                        if (drop_zero && lab[j] == 0u) { vm &= ~(1u << j); ++zeros; }
                    }
                }
            }
            considered += (uint32_t)__popc(vm);

            // where runs start: a considered voxel whose left neighbour is not considered or has another label
            uint32_t starts = vm & 1u;
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if ((vm & (1u << j)) && (!(vm & (1u << (j - 1))) || lab[j] != lab[j - 1])) starts |= 1u << j;

            // solid lanes of one row and label merge inside the wave
            const bool solid = vm == 0xFu && starts == 1u;
            const uint32_t prev_label = (uint32_t)__shfl_up((int)lab[0], 1);
            const unsigned long long solid_m = __ballot(solid);
            const bool joins = solid && lane != 0u && lane_slot != 0u && ((solid_m >> (lane - 1u)) & 1ull) && prev_label == lab[0];
            const unsigned long long join_m = __ballot(joins);
            uint32_t seg_lanes = 1u;                                   // of a segment's first lane: the lanes it stands for
            uint32_t m_fin = 0u, m_vmink = 0u, m_vmaxk = 0u;
            unsigned long long m_vsum = 0ull;
            if (join_m) {                                              // wave-uniform
                // the lane's own value fields
                double dsum = 0.0; uint32_t isum = 0u;
                if (solid) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (F32) {
                            if (bits_finite(val[j])) {
                                const float v = __uint_as_float(val[j]);
                                const uint32_t k = ring_key_of_float(v);
                                ++m_fin; dsum += (double)v; m_vmink = max(m_vmink, ~k); m_vmaxk = max(m_vmaxk, k);
                            }
                        } else {
                            isum += val[j];                            // 256 x 65535 fits
                            const uint32_t k = ring_key_of_float((float)val[j]);
                            m_vmink = max(m_vmink, ~k); m_vmaxk = max(m_vmaxk, k);
                        }
                    }
                    if (!F32) m_fin = 4u;
                }
                // the segment [lane, seg_end): up to the next lane that does not join its left neighbour
                const unsigned long long above = lane == 63u ? 0ull : (~join_m >> (lane + 1u));
                const uint32_t seg_end = above ? lane + (uint32_t)__ffsll((long long)above) : 64u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o_fin = (uint32_t)__shfl_down((int)m_fin, d);
                    const uint32_t o_min = (uint32_t)__shfl_down((int)m_vmink, d);
                    const uint32_t o_max = (uint32_t)__shfl_down((int)m_vmaxk, d);
                    double o_d = 0.0; uint32_t o_i = 0u;
                    if (F32) o_d = __shfl_down(dsum, d); else o_i = (uint32_t)__shfl_down((int)isum, d);
                    if (lane + (uint32_t)d < seg_end) {
                        m_fin += o_fin; m_vmink = max(m_vmink, o_min); m_vmaxk = max(m_vmaxk, o_max);
                        if (F32) dsum += o_d; else isum += o_i;
                    }
                }
                seg_lanes = seg_end - lane;
                m_vsum = F32 ? (unsigned long long)__double_as_longlong(dsum) : (unsigned long long)isum;
            }
            const bool merged = join_m != 0ull && solid;               // this lane's fields are a segment's (from it on)
            if (joins) starts = 0u;                                    // its voxels went to the segment's first lane

            // the runs, one per round: every lane takes its lowest pending start
            while (__ballot(starts != 0u)) {
                if (starts) {
                    const uint32_t s = (uint32_t)__ffs((int)starts) - 1u;
                    starts &= starts - 1u;
                    const uint32_t stop = ((starts | ~vm) >> s) >> 1;                    // a later start or a voxel not considered ends it
                    const uint32_t e = stop ? s + (uint32_t)__ffs((int)stop) : 4u;       // [s, e); ~vm has bits above 3: e <= 4
                    ObjRun<F32> r;
                    r.label = s == 0u ? lab[0] : s == 1u ? lab[1] : s == 2u ? lab[2] : lab[3];
                    uint32_t n = e - s;
                    r.fin = 0ull; r.vsum = 0ull; r.vmink = 0u; r.vmaxk = 0u;
                    if (merged) {
                        n = 4u * seg_lanes;
                        r.fin = m_fin; r.vsum = m_vsum; r.vmink = m_vmink; r.vmaxk = m_vmaxk;
                    } else {
                        double dsum = 0.0; uint32_t isum = 0u, fin = 0u;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if ((uint32_t)j >= s && (uint32_t)j < e) {
                                if (F32) {
                                    if (bits_finite(val[j])) {
                                        const float v = __uint_as_float(val[j]);
                                        const uint32_t k = ring_key_of_float(v);
                                        ++fin; dsum += (double)v; r.vmink = max(r.vmink, ~k); r.vmaxk = max(r.vmaxk, k);
                                    }
                                } else {
                                    isum += val[j]; ++fin;
                                    const uint32_t k = ring_key_of_float((float)val[j]);
                                    r.vmink = max(r.vmink, ~k); r.vmaxk = max(r.vmaxk, k);
                                }
                            }
                        }
                        r.fin = fin;
                        r.vsum = F32 ? (unsigned long long)__double_as_longlong(dsum) : (unsigned long long)isum;
                    }
                    // geometry: x from first + s over n voxels, relative to the window offset
                    const uint32_t xrel = rel[0] + (uint32_t)(first + (int64_t)s);
                    r.n = n;
                    r.s[0] = (unsigned long long)n * xrel + ((unsigned long long)n * (n - 1u)) / 2ull;
                    r.s[1] = (unsigned long long)n * yrel;
                    r.s[2] = (unsigned long long)n * zrel;
                    r.lok[0] = lo_key(a.off[0] + (int32_t)xrel); r.hik[0] = hi_key(a.off[0] + (int32_t)(xrel + n - 1u));
                    r.lok[1] = lo_key(a.off[1] + (int32_t)yrel); r.hik[1] = hi_key(a.off[1] + (int32_t)yrel);
                    r.lok[2] = lo_key(a.off[2] + (int32_t)zrel); r.hik[2] = hi_key(a.off[2] + (int32_t)zrel);
                    if (!obj_lds_add<F32>(t, r)) obj_global_add<F32>(a, r);
                }
            }
        }
    }

    // header[1] and [3]: one add per wave
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        considered += (uint32_t)__shfl_xor((int)considered, d);
        zeros += (uint32_t)__shfl_xor((int)zeros, d);
    }
    if (lane == 0u) {
        if (considered) atomicAdd(&a.header[1], (unsigned long long)considered);
        if (zeros) atomicAdd(&a.header[3], (unsigned long long)zeros);
    }
    __syncthreads();
    for (uint32_t i = tid; i < kLdsSlots; i += kObjThreads) {
        const unsigned long long key = t.key[i];
        if (key == 0ull) continue;
        ObjRun<F32> r;
        r.label = (uint32_t)key;
        r.n = t.n[i];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { r.s[ax] = t.sum[ax][i]; r.lok[ax] = t.lok[ax][i]; r.hik[ax] = t.hik[ax][i]; }
        r.fin = F32 ? t.fin[i] : t.n[i];
        r.vsum = t.vsum[i];
        r.vmink = t.vmink[i]; r.vmaxk = t.vmaxk[i];
        obj_global_add<F32>(a, r);
    }
}

// the last step: keys decoded in place, occupied records counted, the header's offsets written
__global__ __launch_bounds__(256) void obj_finish_kernel(svr_object_record* records, uint32_t capacity, unsigned long long* header,
                                                         int32_t ox, int32_t oy, int32_t oz) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool used = false;
    if (i < capacity) {
        ObjRaw* const r = reinterpret_cast<ObjRaw*>(records) + i;
        used = r->key != 0ull;
        if (used) {
            svr_object_record* const o = records + i;
            int32_t lo[3], hi[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) { lo[ax] = lo_of_key(r->lok[ax]); hi[ax] = hi_of_key(r->hik[ax]); }
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
    }
}

template <typename T>
void obj_launch_typed(const ObjArgs& a, bool filt, uint32_t blocks, hipStream_t stream) {
    if (filt) hipLaunchKernelGGL((obj_kernel<T, true>), dim3(blocks), dim3(kObjThreads), 0, stream, a);
    else      hipLaunchKernelGGL((obj_kernel<T, false>), dim3(blocks), dim3(kObjThreads), 0, stream, a);
}

}  // namespace

// lo[a] .. lo[a] + n[a]: the intersection of box and window in logical voxels of the LOD (n may hold a value <= 0: nothing
// is considered).  Everything was validated by svr_objects.
hipError_t svr_launch_objects(const svr_ctx* c, int lod, const int64_t lo[3], const int64_t n[3], const uint32_t* sel, uint32_t nsel,
                              int ignore_zero, uint32_t capacity, const svr_objects_outputs& out, hipStream_t stream) {
    const LodStorage& L = c->lod[lod];
    unsigned long long* header = reinterpret_cast<unsigned long long*>(out.header);
    hipError_t e = hipMemsetAsync(out.records, 0, (size_t)capacity * sizeof(svr_object_record), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(header, 0, 8 * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;

    if (n[0] > 0 && n[1] > 0 && n[2] > 0) {
        ObjArgs a;
        a.density = L.density; a.labels = L.labels;
        a.sel = sel; a.nsel = nsel; a.ignore_zero = ignore_zero;
        a.records = out.records; a.capacity = capacity; a.header = header;
        for (int ax = 0; ax < 3; ++ax) { a.ring[ax] = (uint32_t)L.ring[ax]; a.off[ax] = L.state.offset[ax]; }
        // a workgroup's share of the bytes read (density + 4 of label per voxel); slots are 16 bytes of the label ring
        const uint32_t es = (uint32_t)svr_dtype_size(c->density_storage);
        const RingPass pass = {es + 4u, 4u, reinterpret_cast<uintptr_t>(L.labels), ring_workgroups(c->device, kObjWgPerCu), kObjMinShare};
        RingPlan plan;
        if (!ring_plan(a.ring, a.off, lo, n, pass, plan)) return hipErrorInvalidValue;
        a.npieces = plan.pieces.npieces;
        for (int p = 0; p < a.npieces; ++p) {
            static_cast<RingBox&>(a.piece[p]) = plan.pieces.piece[p];
            static_cast<RingShare&>(a.piece[p]) = plan.pieces.piece[p];
            memcpy(a.piece[p].rel, plan.rel[p], sizeof(plan.rel[p]));
        }
        const uint32_t blocks = plan.blocks;
        const bool filt = nsel > 0;
        if (c->density_storage == SVR_U8)       obj_launch_typed<uint8_t>(a, filt, blocks, stream);
        else if (c->density_storage == SVR_U16) obj_launch_typed<uint16_t>(a, filt, blocks, stream);
        else                                    obj_launch_typed<float>(a, filt, blocks, stream);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const svr_lod_state& st = L.state;
    hipLaunchKernelGGL(obj_finish_kernel, dim3((unsigned)(((size_t)capacity + 255) / 256)), dim3(256), 0, stream, out.records, capacity,
                       header, st.offset[0], st.offset[1], st.offset[2]);
    return hipGetLastError();
}
