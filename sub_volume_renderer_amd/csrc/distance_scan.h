// The 1-D pass of svr_distance (include/svr.h; kernels: distance_kernels.hip): the lower envelope of the parabolas
// g[i] + (u - i)^2 over one column, in integers.  The same text runs in the y / z kernel, one thread per column, and in a
// host program that a test compiles without HIP (tests/test_distance.py).
//
// out[u] = min over the i with g[i] != kDistFar of g[i] + (u - i)^2, or kDistFar when the column has no such i.
//
// The method is the two-scan form of Meijster, Roerdink and Hesselink (2000).  The forward scan keeps a stack of the
// parabolas that own a stretch of the envelope: (vertex s, value g[s], start t), the stretch of entry k being
// [t_k, t_{k+1}).  A new vertex u pops every entry that it beats at that entry's own start, then starts at
//   w = 1 + sep(s, u),   sep(s, u) = (u^2 - s^2 + g[u] - g[s]) div (2 (u - s)),
// the largest position at which the older parabola is still not above the newer one; it is pushed when w < m.  The
// backward scan walks the stack down and evaluates the owner of every position.  Every vertex is pushed once and popped
// at most once, so the work is linear in the column's length whatever the data: nothing searches a neighbourhood.
//
// Ranges (m <= kDistMaxExtent = 2^14, g <= 2 * 2^28 or kDistFar, the most the z pass meets: dx^2 + dy^2):
//   (u - s)^2 + g  <  2^28 + 2 * 2^28 = 3 * 2^28 < 2^31, so every parabola value fits int32 and stays below kDistFar;
//   the numerator of sep: u^2 - s^2 < 2^28 and |g[u] - g[s]| <= 2^29, so it fits int32 too.  It is never negative where
//   it is divided: the pops end at an entry with f(t, s) <= f(t, u), which says t <= sep(s, u), and t >= 0.  So the
//   division is a 32-bit unsigned one, exact, with nothing to round: no 64-bit arithmetic and no float anywhere.
// A kDistFar entry is no parabola: it is skipped, never summed.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DIST_FN __host__ __device__ __forceinline__
#else
#define DIST_FN inline
#endif

constexpr int32_t  kDistFar = 0x7FFFFFFF;         // SVR_DISTANCE_FAR
constexpr uint32_t kDistMaxExtent = 16384;        // SVR_DISTANCE_MAX_EXTENT: vertex and start fit 16 bits each

struct DistEntry {                                // one entry of a column's stack: 8 bytes
    int32_t  value;                               // g at the vertex
    uint32_t st;                                  // vertex | start << 16
};

DIST_FN DistEntry dist_entry(int32_t value, uint32_t s, uint32_t t) { return DistEntry{value, s | (t << 16)}; }

// The entries just below the top of the stack are the ones a pop reads, right after they were written: a small ring of the
// last R entries pushed, kept where reads are cheap (the kernel: LDS), answers most pops.  Entry k lives in slot k % R.
// Every entry k in [lo, top] is the one in its slot: a slot is only overwritten by entry k + R, pushed while k lies below
// it on the stack, and that push raises lo above k for good.  The stack in memory stays complete: the backward scan and
// the pops below lo read it.
template <uint32_t R>
struct DistRing {
    static_assert(R && !(R & (R - 1u)), "R is a power of two");
    DistEntry* slots;                             // slot j at slots[j * stride]
    size_t stride;
    uint32_t lo;
    DIST_FN DistRing(DistEntry* s, size_t st) : slots(s), stride(st), lo(0u) {}
    DIST_FN void put(uint32_t k, DistEntry e) {
        slots[(size_t)(k & (R - 1u)) * stride] = e;
        if (k + 1u > R + lo) lo = k + 1u - R;
    }
    DIST_FN bool has(uint32_t k) const { return k >= lo; }
    DIST_FN DistEntry get(uint32_t k) const { return slots[(size_t)(k & (R - 1u)) * stride]; }
};

constexpr int kDistAhead = 4;                     // entries the backward scan reads ahead of the pop that needs them

constexpr uint32_t kDistNoOwner = 0xFFFFu;        // the owner of a position of a column that has no parabola: no vertex is that large

// g: the column, element u at g[u * gs]; stack: m entries, entry k at stack[k * ss]; ring: a DistRing of any size;
// emit(u, value, owner) is called once for every u, from m - 1 down to 0, after the last read of g: it may store into g.
// owner: the vertex i of the parabola that gives the value, the smallest such i where several do (svr_nearest's tie rule,
// include/svr.h): an older vertex keeps every position at which the newer one is not strictly below it, as the pop test
// (a strict >) and the start 1 + sep say.  kDistNoOwner with kDistFar.
template <class Ring, class Emit>
DIST_FN void dist_scan_column_owner(const int32_t* g, size_t gs, uint32_t m, DistEntry* stack, size_t ss, Ring ring, Emit&& emit) {
    int32_t q = -1;                               // the top of the stack, which also lives in (ts, tv, tt)
    int32_t ts = 0, tv = 0, tt = 0;
    int32_t next = g[0];
    for (uint32_t u = 0; u < m; ++u) {
        const int32_t gv = next;
        if (u + 1 < m) next = g[(size_t)(u + 1) * gs];
        if (gv == kDistFar) continue;
        while (q >= 0) {
            const int32_t a = tt - ts, b = tt - (int32_t)u;
            if (a * a + tv <= b * b + gv) break;
            if (--q >= 0) {
                const DistEntry e = ring.has((uint32_t)q) ? ring.get((uint32_t)q) : stack[(size_t)q * ss];
                tv = e.value; ts = (int32_t)(e.st & 0xFFFFu); tt = (int32_t)(e.st >> 16);
            }
        }
        if (q < 0) {
            q = 0; ts = (int32_t)u; tv = gv; tt = 0;
            stack[0] = dist_entry(tv, (uint32_t)ts, 0u);
            ring.put(0u, dist_entry(tv, (uint32_t)ts, 0u));
        } else {
            const uint32_t num = (uint32_t)(((int32_t)(u * u) - ts * ts) + (gv - tv));
            const uint32_t w = 1u + num / (2u * (u - (uint32_t)ts));
            if (w < m) {
                ++q; ts = (int32_t)u; tv = gv; tt = (int32_t)w;
                stack[(size_t)q * ss] = dist_entry(tv, u, w);
                ring.put((uint32_t)q, dist_entry(tv, u, w));
            }
        }
    }
    if (q < 0) {
        for (uint32_t u = m; u-- > 0u;) emit(u, kDistFar, kDistNoOwner);
        return;
    }
    // the entries below the top, in the order the pops will want them, read kDistAhead pops ahead of their use
    DistEntry below[kDistAhead];
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int j = 0; j < kDistAhead; ++j) below[j] = q - 1 - j >= 0 ? stack[(size_t)(q - 1 - j) * ss] : DistEntry{0, 0u};
    for (uint32_t u = m; u-- > 0u;) {
        const int32_t d = (int32_t)u - ts;
        emit(u, d * d + tv, (uint32_t)ts);
        if ((int32_t)u == tt && q > 0) {
            --q;
            tv = below[0].value; ts = (int32_t)(below[0].st & 0xFFFFu); tt = (int32_t)(below[0].st >> 16);
#ifdef __HIPCC__
#pragma unroll
#endif
            for (int j = 0; j + 1 < kDistAhead; ++j) below[j] = below[j + 1];
            if (q - kDistAhead >= 0) below[kDistAhead - 1] = stack[(size_t)(q - kDistAhead) * ss];
        }
    }
}

// The same without the owner: emit(u, value).  svr_distance's.
template <class Ring, class Emit>
DIST_FN void dist_scan_column(const int32_t* g, size_t gs, uint32_t m, DistEntry* stack, size_t ss, Ring ring, Emit&& emit) {
    dist_scan_column_owner(g, gs, m, stack, ss, ring, [&](uint32_t u, int32_t v, uint32_t) { emit(u, v); });
}
