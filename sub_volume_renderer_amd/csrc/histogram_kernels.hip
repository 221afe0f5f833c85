// Intensity histograms of the resident rings (svr_histogram, include/svr.h): one streaming pass over a box of one
// LOD's window.  gfx950.
//
// Decomposition (ring_pieces.h, shared with object_kernels.hip).  The host cuts the intersection of box and window at
// the ring's wrap seams into at most 2 x 2 x 2 pieces; each piece is a dense sub-block of the row-major ring (the
// micro-block copy is never read), so the kernel sees straight rows.  A workgroup of 256 threads takes a run of whole
// rows of one piece, sized so that it sees fewer than 2^32 voxels (its LDS counters are u32).  A row is read in
// 16-byte slots aligned in MEMORY: slot k of a row covers the 16 bytes at (row start rounded down to 16) + 16 k.  A
// slot that lies wholly inside the row is one 16-byte load; the slots that hold the row's head and tail read only
// their own elements, one by one.  2^k lanes share a row (the smallest power of two that covers its slots; for rows of
// more than 8 slots the one from 8 to 256 that wastes the fewest lanes), so short rows still fill the wave.
//
// Counting.  Per-workgroup LDS sub-histogram of K + 3 u32 words (the three tails are bins K .. K + 2), flushed with
// one 64-bit global atomic per non-zero word.  Contention: a ring that is mostly one value sends nearly every lane
// to one bin, and same-address LDS atomics serialise.  So equal bins are merged before they reach the LDS:
//   1. inside a lane: a slot whose 16 bytes are all one value (compared as raw dwords) is ONE (bin, weight) pair;
//   2. inside a wave: the first pending lane's bin is broadcast, the lanes that hold the same bin are counted with a
//      ballot, and their first lane adds weight * popcount once.  Two such rounds (the modal bin may not sit in the
//      first lane); what is still pending adds for itself.  A wave whose lanes do not agree (fewer than one in
//      eight on the first lane's bin, tested on one element per slot) skips the merging: on noise it only costs.
// A constant ring thus costs one LDS atomic per wave and 1 KiB read.  Counts are integers: the result does not
// depend on arrival order.  No float atomics anywhere: min / max travel as u32 keys that order like the floats.
#include "svr_host.h"
#include "ring_pieces.h"

namespace {

constexpr int kHistThreads = 256;
// Every workgroup holds the counters of the largest K (16.4 KB of static LDS, whatever K the call has): that, not
// registers, bounds a CU at nine workgroups of the 160 KB; the grid is sized for eight.
constexpr uint64_t kHistWgPerCu = 8;
constexpr uint64_t kHistMinShare = 16384;    // bytes of voxels

struct HistArgs {
    const void* density;
    const uint32_t* labels;    // null: every label reads as 0
    uint32_t ring[3];
    float lo, hi, inv;
    int32_t K;
    const uint32_t* sel;
    uint32_t nsel;
    unsigned long long* counts;
    unsigned long long* tail;  // may be null
    uint32_t* range_keys;      // the caller's range[2], holding (min key, max key) until hist_finish_kernel; may be null
    RingPieces pieces;
};

template <typename T> struct HistElem;
template <> struct HistElem<uint8_t> {
    static constexpr int kPerSlot = 16;
    static __device__ __forceinline__ uint32_t raw(const uint4& q, int j) { return ((&q.x)[j >> 2] >> ((j & 3) * 8)) & 0xFFu; }
    static __device__ __forceinline__ uint32_t raw1(const uint8_t* p) { return *p; }
    static __device__ __forceinline__ float value(uint32_t r) { return (float)r; }
    static __device__ __forceinline__ bool one_value(const uint4& q) {
        const uint32_t b = (q.x & 0xFFu) * 0x01010101u;
        return ((q.x ^ b) | (q.y ^ b) | (q.z ^ b) | (q.w ^ b)) == 0u;
    }
};
template <> struct HistElem<uint16_t> {
    static constexpr int kPerSlot = 8;
    static __device__ __forceinline__ uint32_t raw(const uint4& q, int j) { return ((&q.x)[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu; }
    static __device__ __forceinline__ uint32_t raw1(const uint16_t* p) { return *p; }
    static __device__ __forceinline__ float value(uint32_t r) { return (float)r; }
    static __device__ __forceinline__ bool one_value(const uint4& q) {
        const uint32_t b = (q.x & 0xFFFFu) * 0x00010001u;
        return ((q.x ^ b) | (q.y ^ b) | (q.z ^ b) | (q.w ^ b)) == 0u;
    }
};
template <> struct HistElem<float> {
    static constexpr int kPerSlot = 4;
    static __device__ __forceinline__ uint32_t raw(const uint4& q, int j) { return (&q.x)[j]; }
    static __device__ __forceinline__ uint32_t raw1(const float* p) { return __float_as_uint(*p); }
    static __device__ __forceinline__ float value(uint32_t r) { return __uint_as_float(r); }
    static __device__ __forceinline__ bool one_value(const uint4& q) {      // bit patterns: the same float either way
        return ((q.x ^ q.y) | (q.x ^ q.z) | (q.x ^ q.w)) == 0u;
    }
};

// the binning chain of include/svr.h; the tails are bins K (under), K + 1 (over) and K + 2 (NaN).  j = min((int)x, K - 1)
// is written as compares around a cast that is always in range: (int) of a float beyond int's range, or of NaN, is
// undefined in C++ (v_cvt_i32_f32 saturates and gives 0, but the compiler need not keep it).  x is never negative;
// it is NaN only as inf * 0, when hi - lo overflowed f32 (inv == 0) and v - lo did too: bin 0, as the header states.
__device__ __forceinline__ uint32_t hist_bin(float v, float lo, float hi, float inv, int K) {
    if (v != v) return (uint32_t)K + 2u;
    if (v < lo) return (uint32_t)K;
    if (v > hi) return (uint32_t)K + 1u;
    const float x = (v - lo) * inv;
    if (x >= (float)K) return (uint32_t)K - 1u;
    return x > 0.0f ? (uint32_t)(int)x : 0u;
}

// `pending` lanes add `weight` (the same in every pending lane) to bins[bin]; equal bins merge inside the wave.
// Called from wave-uniform control flow.
__device__ __forceinline__ void hist_wave_add(uint32_t* bins, uint32_t bin, bool pending, uint32_t weight) {
    const uint32_t lane = __lane_id();
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (pending) {
            const uint32_t cand = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
            const bool mine = bin == cand;
            const unsigned long long m = __ballot(mine);        // over the lanes still pending
            if (mine) {
                if (lane == (uint32_t)(__ffsll(m) - 1)) atomicAdd(&bins[cand], weight * (uint32_t)__popcll(m));
                pending = false;
            }
        }
    }
    if (pending) atomicAdd(&bins[bin], weight);
}

template <typename T, bool FILT>
__global__ __launch_bounds__(kHistThreads) void hist_kernel(const HistArgs a) {
    using E = HistElem<T>;
    constexpr int V = E::kPerSlot;
    constexpr uint32_t kAll = (1u << V) - 1u;
    __shared__ uint32_t bins[SVR_HIST_MAX_BINS + 3];
    __shared__ uint32_t wg_min, wg_max;
    const uint32_t tid = threadIdx.x;
    const int K = a.K;
    for (uint32_t k = tid; k < (uint32_t)K + 3u; k += kHistThreads) bins[k] = 0u;
    if (tid == 0) { wg_min = 0xFFFFFFFFu; wg_max = 0u; }
    __syncthreads();

    RING_WALK(kHistThreads, a.pieces, blockIdx.x, tid);
    const uint32_t nx = P.n[0];
    const T* const ring = static_cast<const T*>(a.density);

    // without label rings every label is 0: the filter passes everything or nothing
    bool filter = FILT, nothing = false;
    if (FILT && !a.labels) { filter = false; nothing = !ring_in_set(a.sel, a.nsel, 0u); }

    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;             // keys of the lane's min / max (integer rings: the raw values)
    bool any = false;
    uint32_t last_label = 0u; bool last_pass = false, have_last = false;

    if (!nothing)
    for (uint64_t rb = r0; rb < r1; rb += rows_per_iter) {          // wave-uniform trip counts; `row_ok` masks lanes
        const bool row_ok = rb + lane_row < r1;
        const uint32_t row = (uint32_t)(rb + lane_row);
        const uint32_t ry = row_ok ? row % P.n[1] : 0u, rz = row_ok ? row / P.n[1] : 0u;
        const size_t e0 = RING_ROW_OFFSET(P, a.ring, ry, rz);
        const T* const rowp = ring + e0;
        const uint32_t head = (uint32_t)((reinterpret_cast<uintptr_t>(rowp) & 15u) / sizeof(T));   // elements before the row in its first slot
        for (uint32_t sb = 0; sb < P.spr; sb += lpr) {
            const uint32_t slot = sb + lane_slot;
            // the slot holds row elements [first, first + V), of which [0, nx) exist
            const int64_t first = (int64_t)slot * V - (int64_t)head;
            const bool live = row_ok && first < (int64_t)nx && first + V > 0;
            const bool full = live && first >= 0 && first + V <= (int64_t)nx;
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            uint32_t vm = 0u;                                          // which of the slot's V elements are considered
            uint32_t rawv[V];
            if (full) {
                q = *reinterpret_cast<const uint4*>(rowp + first);
                vm = kAll;
#pragma unroll
                for (int j = 0; j < V; ++j) rawv[j] = E::raw(q, j);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int64_t e = first + j;
                    const bool ok = live && e >= 0 && e < (int64_t)nx;
                    rawv[j] = ok ? E::raw1(rowp + e) : 0u;
                    vm |= ok ? (1u << j) : 0u;
                }
            }
            if (filter && vm) {
                const uint32_t* const lrow = a.labels + e0;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (vm & (1u << j)) {
                        const uint32_t lab = lrow[first + j];
                        if (!have_last || lab != last_label) {
                            last_pass = ring_in_set(a.sel, a.nsel, lab); last_label = lab; have_last = true;
                        }
                        if (!last_pass) vm &= ~(1u << j);
                    }
                }
            }
            // 1. a slot of one value is one pair
            const bool solid = full && vm == kAll && E::one_value(q);
            const uint32_t b0 = hist_bin(E::value(rawv[0]), a.lo, a.hi, a.inv, K);
            if (solid && b0 != (uint32_t)K + 2u) {
                const uint32_t key = sizeof(T) == 4 ? ring_key_of_float(E::value(rawv[0])) : rawv[0];
                kmin = min(kmin, key); kmax = max(kmax, key); any = true;
            }
            hist_wave_add(bins, b0, solid, (uint32_t)V);
            // 2. the others, element by element (skipped by waves that hold none).  Merging costs two ballots per
            //    element and pays only where lanes agree: the wave looks at element 0 of its lanes first, and where
            //    fewer than one lane in eight holds the first lane's bin (noise, texture) every lane adds for itself.
            const bool mixed = vm != 0u && !solid;
            if (__ballot(mixed)) {
                const bool probe = mixed && (vm & 1u);
                const unsigned long long pm = __ballot(probe);
                bool merge = true;
                if (pm) {
                    const uint32_t cand = (uint32_t)__builtin_amdgcn_readlane((int)b0, __ffsll(pm) - 1);
                    merge = (uint32_t)__popcll(__ballot(probe && b0 == cand)) * 8u >= (uint32_t)__popcll(pm);
                }
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const bool ok = mixed && (vm & (1u << j));
                    const float v = E::value(rawv[j]);
                    const uint32_t b = hist_bin(v, a.lo, a.hi, a.inv, K);
                    if (ok && b != (uint32_t)K + 2u) {
                        const uint32_t key = sizeof(T) == 4 ? ring_key_of_float(v) : rawv[j];
                        kmin = min(kmin, key); kmax = max(kmax, key); any = true;
                    }
                    if (merge) hist_wave_add(bins, b, ok, 1u);
                    else if (ok) atomicAdd(&bins[b], 1u);
                }
            }
        }
    }

    // min / max: per wave, then per workgroup through LDS, then one pair of global u32 atomics
    if (a.range_keys) {
        if (sizeof(T) != 4 && any) {                                   // integer rings tracked raw values: exact in f32
            kmin = ring_key_of_float((float)kmin); kmax = ring_key_of_float((float)kmax);
        }
        if (!any) { kmin = 0xFFFFFFFFu; kmax = 0u; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, d));
            kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, d));
        }
        if ((tid & 63u) == 0u && kmin <= kmax) { atomicMin(&wg_min, kmin); atomicMax(&wg_max, kmax); }
    }
    __syncthreads();
    if (a.range_keys && tid == 0 && wg_min <= wg_max) { atomicMin(&a.range_keys[0], wg_min); atomicMax(&a.range_keys[1], wg_max); }
    for (uint32_t k = tid; k < (uint32_t)K + 3u; k += kHistThreads) {
        const uint32_t c = bins[k];
        if (c == 0u) continue;
        if (k < (uint32_t)K) atomicAdd(&a.counts[k], (unsigned long long)c);
        else if (a.tail) atomicAdd(&a.tail[k - (uint32_t)K], (unsigned long long)c);
    }
}

// the overwrite: zero counts and tail, and put the empty (min, max) keys where the range will be
__global__ __launch_bounds__(256) void hist_init_kernel(unsigned long long* counts, int K, unsigned long long* tail, uint32_t* range_keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < (uint32_t)K) counts[i] = 0ull;
    if (tail && i < 4u) tail[i] = 0ull;
    if (range_keys && i < 2u) range_keys[i] = i == 0u ? 0xFFFFFFFFu : 0u;
}

// the last step: tail[3] = everything counted, and the keys decoded in place into the floats of `range`
__global__ __launch_bounds__(256) void hist_finish_kernel(const unsigned long long* counts, int K, unsigned long long* tail, uint32_t* range_keys) {
    __shared__ unsigned long long part[256];
    const uint32_t tid = threadIdx.x;
    if (tail) {
        unsigned long long s = 0ull;
        for (uint32_t k = tid; k < (uint32_t)K; k += 256u) s += counts[k];
        part[tid] = s;
        __syncthreads();
        for (uint32_t d = 128u; d >= 1u; d >>= 1) {
            if (tid < d) part[tid] += part[tid + d];
            __syncthreads();
        }
        if (tid == 0) tail[3] = part[0] + tail[0] + tail[1] + tail[2];
    }
    if (range_keys && tid == 0) {
        const uint32_t kmin = range_keys[0], kmax = range_keys[1];
        float* const r = reinterpret_cast<float*>(range_keys);
        if (kmin > kmax) { r[0] = __builtin_inff(); r[1] = -__builtin_inff(); }     // nothing considered, or only NaN
        else { r[0] = ring_float_of_key(kmin); r[1] = ring_float_of_key(kmax); }
    }
}

template <typename T>
void hist_launch_typed(const HistArgs& a, bool filt, uint32_t blocks, hipStream_t stream) {
    if (filt) hipLaunchKernelGGL((hist_kernel<T, true>), dim3(blocks), dim3(kHistThreads), 0, stream, a);
    else      hipLaunchKernelGGL((hist_kernel<T, false>), dim3(blocks), dim3(kHistThreads), 0, stream, a);
}

}  // namespace

// lo[a] .. lo[a] + n[a]: the intersection of box and window in logical voxels of the LOD (n may hold a value <= 0: nothing to count).
// Everything was validated by svr_histogram; inv = (float)K / (hi - lo).
hipError_t svr_launch_histogram(const svr_ctx* c, int lod, const int64_t lo[3], const int64_t n[3], float flo, float fhi,
                                float inv, int K, const uint32_t* sel, uint32_t nsel, const svr_histogram_outputs& out,
                                hipStream_t stream) {
    const LodStorage& L = c->lod[lod];
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(out.counts);
    unsigned long long* tail = reinterpret_cast<unsigned long long*>(out.tail);
    uint32_t* keys = reinterpret_cast<uint32_t*>(out.range);
    hipLaunchKernelGGL(hist_init_kernel, dim3((unsigned)(K + 255) / 256u), dim3(256), 0, stream, counts, K, tail, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    if (n[0] > 0 && n[1] > 0 && n[2] > 0) {
        HistArgs a;
        a.density = L.density; a.labels = L.labels;
        a.lo = flo; a.hi = fhi; a.inv = inv; a.K = K;
        a.sel = sel; a.nsel = nsel;
        a.counts = counts; a.tail = tail; a.range_keys = keys;
        for (int ax = 0; ax < 3; ++ax) a.ring[ax] = (uint32_t)L.ring[ax];
        // a workgroup's share: kHistWgPerCu workgroups per CU of the device over the whole box, and at least
        // kHistMinShare bytes of voxels, which keeps the flush (one global atomic per non-zero bin) a small part of its work
        const uint32_t es = (uint32_t)svr_dtype_size(c->density_storage);
        const RingPass pass = {es, 16u / es, reinterpret_cast<uintptr_t>(L.density), ring_workgroups(c->device, kHistWgPerCu), kHistMinShare};
        RingPlan plan;
        if (!ring_plan(a.ring, L.state.offset, lo, n, pass, plan)) return hipErrorInvalidValue;
        a.pieces = plan.pieces;
        const uint32_t blocks = plan.blocks;
        const bool filt = nsel > 0;
        if (c->density_storage == SVR_U8)       hist_launch_typed<uint8_t>(a, filt, blocks, stream);
        else if (c->density_storage == SVR_U16) hist_launch_typed<uint16_t>(a, filt, blocks, stream);
        else                                    hist_launch_typed<float>(a, filt, blocks, stream);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (tail || keys) {
        hipLaunchKernelGGL(hist_finish_kernel, dim3(1), dim3(256), 0, stream, counts, K, tail, keys);
        e = hipGetLastError();
    }
    return e;
}
