// Iso-surface render mode (svr_iso, include/svr.h): the first sample along each of the march's rays whose value reaches
// iso_value, refined by a linear sub-sample search, shaded (two-sided Blinn-Phong) from the central-difference gradient
// at the hit.  One lane = one pixel; a workgroup of 256 threads is a 16 x 16 pixel tile of four 8 x 8 wave tiles, placed
// on the XCDs like composite_kernels.hip's (march_simple's layout and fallback placement).
//
// Per wave, coarse samples go in stretches of ISO_UNROLL.  Before a stretch each live lane looks the index box of its
// ISO_UNROLL samples up in the macro-cell maxima the uploads maintain (ring_kernels.hip: `blk`, the maximum over the
// 2 x 2 x 2 block of cells starting at a cell); when no live lane of the wave can reach iso_value the wave moves on
// without a texel fetch.  Otherwise: the LOD and address of every sample of the stretch first, then their gathers (all
// in flight together), then the serial "first >= iso" pick.  A lane is live until it has a candidate or its ray ends;
// a wave leaves the loop when no lane is live.  Refinement, gradient and shading run once per wave, after the loop.
//
// Arithmetic contract: strict IEEE f32 without contraction (-ffp-contract=off), operation order as written in svr.h.
// Ray set-up, LOD test and the small helpers are ray_common.h's; tests/test_gpu_iso.py holds this kernel to
// tests/iso_twin.py.
#include "svr_host.h"
#include "ray_common.h"
#include "linear_sample.h"

namespace {

using namespace svr_common;

struct IsoLod {
    const void*     density;   // ring [z][y][x], element type per the kernel's ESH
    const uint32_t* labels;    // null: no label rings
    const void*     cells;     // `blk` maxima of this LOD's macro cells (element type = the ring's), null: none
    int32_t  off[3];           // current_logical_offset_in_pixels
    uint32_t shape[3];         // current_logical_shape_in_pixels
    uint32_t wrap0[3];         // ring slot of the ROI's first voxel
    uint32_t ring[3];
    float    scale[3];
    uint32_t cdim[3];          // cells per axis
    int32_t  cshift;           // log2 of the cell size
};

struct IsoParams {
    float ndc_to_data[16];     // world_inv * cam_inv * proj_inv, as svr_render forms it
    float pc[16];              // proj * cam
    float world[16];
    float world_inv[16];
    float size[3];
    float rel_step;
    svr_frame frame;
    float opacity;
    uint32_t clip_count;
    int32_t  clip_all;
    float    clip[SVR_MAX_CLIP_PLANES][4];
    uint32_t color_count;
    const float* colors;       // device, color_count x vec4 (h, s, v, pad)
    float    iso;
    int32_t  refine;
    float    base[3];
    int32_t  tint;
    float    ambient, diffuse, specular;
    int32_t  shininess_log2;
    int32_t  headlight;
    float    light[3];
    int32_t  skip;             // 1: test the cell maxima before each stretch
    int32_t  tiles_x, tiles_y;
    float*    rgba;
    float*    depth;
    uint32_t* label;
    uint8_t*  flags;
    uint32_t* steps;
    unsigned long long* pick; uint32_t pick_id;
    float*    normal;
    uint32_t* counters;
    IsoLod L[SVR_MAX_LODS];
    CutParams cut;             // after L[]: every argument above keeps the offset it had before cuts existed
};

using IsoArgs = const IsoParams __attribute__((address_space(4)));     // the kernel arguments' own address space

constexpr int ISO_UNROLL = 8;     // coarse samples per stretch: one cell test, then 8 gathers in flight per lane

// The sample S / D of svr.h for a data point: the first LOD whose ROI holds it gives lod and element index.
template <int NL>
__device__ __forceinline__ bool cascade(const IsoLod* Ls, float dx, float dy, float dz, int& lod, size_t& idx) {
#pragma unroll
    for (int l = 0; l < NL; ++l)
        if (lod_index(Ls[l], dx, dy, dz, idx)) { lod = l; return true; }
    return false;
}

template <int NL, int ESH, bool LIN>
__device__ __forceinline__ bool value_at(const IsoLod* Ls, float dx, float dy, float dz, float& v, int& lod, size_t& idx) {
    if (!cascade<NL>(Ls, dx, dy, dz, lod, idx)) return false;
    if constexpr (!LIN) {
#pragma unroll
    for (int l = 0; l < NL; ++l)
        if (lod == l) v = load_global<ESH>(static_cast<const char*>(Ls[l].density) + (idx << ESH));
    } else {       // the linear sample inside the LOD the nearest sample picked
        svr_linear::LaneLod q = svr_linear::lane_lod_zero();
        const char* base = static_cast<const char*>(Ls[0].density);
#pragma unroll
        for (int l = 0; l < NL; ++l)
            if (lod == l) {
                svr_linear::lane_lod_take(q, Ls[l], dx * Ls[l].scale[0], dy * Ls[l].scale[1], dz * Ls[l].scale[2]);
                base = static_cast<const char*>(Ls[l].density);
            }
        const svr_linear::Cell cell = svr_linear::cell_of(q);
        size_t o[8];
        svr_linear::row_offsets(q, cell, o);
        float c8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c8[k] = load_global<ESH>(base + (o[k] << ESH));
        v = svr_linear::blend(c8, cell.f);
    }
    return true;
}

// a cell maximum as the sample's conversion would deliver it: (float) of u8 / u16 is exact; float rings keep max |v|,
// which bounds v from above (the host turns skipping off unless iso_value > 0)
template <int ESH>
__device__ __forceinline__ float load_cell(const void* cells, uint32_t i) {
    typedef __attribute__((address_space(1))) const uint8_t G8;
    typedef __attribute__((address_space(1))) const uint16_t G16;
    typedef __attribute__((address_space(1))) const float G32;
    if (ESH == 0) return (float)((G8*)cells)[i];
    if (ESH == 1) return (float)((G16*)cells)[i];
    return ((G32*)cells)[i];
}

// Can a sample of the stretch [i0, i0 + ISO_UNROLL) of this lane's ray reach iso?  Along a ray every voxel index is
// monotone per axis (start + iter * step, the two multiplies and the truncation are monotone in iter), so the samples
// of the stretch lie in the index box spanned by its two ends, at every LOD.  A LOD matters while no finer LOD's ROI
// holds the whole box (then every sample resolves there or finer).  For a LOD that matters the part of the box inside
// its ROI is looked up: when it spans at most two cells per axis, the `blk` maximum at the lower cell covers it (on
// the torus, like the ring: ring extents are whole cells); wider boxes, and LODs without a cell grid, answer "maybe".
//
// LIN (linear sampling): a sample that resolves at a LOD reads the voxels floor(s - 0.5) and that plus one per axis,
// clamped to the window: at most one voxel outside the box on each side.  Which LODs matter is decided on the box
// itself (the LOD pick is the nearest sample's); the box that is LOOKED UP is grown by one voxel per side and clamped
// to the window before the two-cell test.  The blend of eight corners of magnitude <= m is, in exact arithmetic, at
// most m; each of the three nested f32 lerps a + f * (b - a), 0 <= f < 1, |a|, |b| <= M, returns at most
// M * (1 + 5u + O(u^2)), u = 2^-24 (two roundings on a term of magnitude <= 2 M, one on the sum), so the computed
// value stays below m * (1 + 2^-19) plus what underflow can add (far below FLT_MIN).  The test compares that bound.
template <int NL, int ESH, bool LIN>
__device__ __forceinline__ bool stretch_may_reach(const IsoLod* Ls, const IsoParams& P, const Ray& R, int i0) {
    const float ia = (float)i0, ib = (float)(i0 + (ISO_UNROLL - 1));
    const float ax = (R.start.x + ia * R.step.x) * P.size[0], bx = (R.start.x + ib * R.step.x) * P.size[0];
    const float ay = (R.start.y + ia * R.step.y) * P.size[1], by = (R.start.y + ib * R.step.y) * P.size[1];
    const float az = (R.start.z + ia * R.step.z) * P.size[2], bz = (R.start.z + ib * R.step.z) * P.size[2];
    bool maybe = false, open = true;
    uint32_t cell[NL];
    bool look[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const IsoLod& L = Ls[l];
        const float a[3] = { ax * L.scale[0], ay * L.scale[1], az * L.scale[2] };
        const float b[3] = { bx * L.scale[0], by * L.scale[1], bz * L.scale[2] };
        bool inter = true, whole = true, wide = false;
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = (int)a[k], q = (int)b[k];
            const int lo = min(p, q), hi = max(p, q);
            const int first = L.off[k], last = L.off[k] + (int)L.shape[k] - 1;
            const int clo = max(lo, first), chi = min(hi, last);
            inter = inter && clo <= chi;
            whole = whole && lo >= first && hi <= last;
            // ring slots before the wrap: below 2 * ring, so the cell coordinate is below 2 * cdim
            const int glo = LIN ? max(lo - 1, first) : clo, ghi = LIN ? min(hi + 1, last) : chi;   // (the looked-up box)
            const uint32_t ulo = (uint32_t)(glo - first) + L.wrap0[k], uhi = (uint32_t)(ghi - first) + L.wrap0[k];
            const uint32_t cl = ulo >> L.cshift, ch = uhi >> L.cshift;
            wide = wide || ch > cl + 1u;
            c[k] = min(cl, cl - L.cdim[k]);
        }
        const bool matters = open && inter;
        look[l] = matters && !wide && L.cells != nullptr;
        maybe = maybe || (matters && !look[l]);
        cell[l] = look[l] ? (c[2] * L.cdim[1] + c[1]) * L.cdim[0] + c[0] : 0u;
        open = open && !whole;
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (Ls[l].cells == nullptr) continue;                            // (uniform)
        const float m = load_cell<ESH>(Ls[l].cells, cell[l]);
        const float bound = LIN ? (m + m * 0x1p-19f) + 1.17549435e-38f : m;
        maybe = maybe || (look[l] && bound >= P.iso);
    }
    return maybe;
}

constexpr int ISO_LIN_GROUP = 4;   // linear sampling: a stretch's samples go in groups of 4 (32 gathers in flight per lane)

// LIN: S(iter) and D(p) are the linear sample of svr.h (svr_set_interpolation); label and LOD of the hit stay the
// nearest sample's.
// CUT: S(iter) has no value where svr_set_cut_planes cuts (coarse and refine searches; D(p) reads the uncut field), and
// a hit whose predecessor in search order was cut is a cap: its normal is the cutting plane's.  The ray's kept (ANY) or
// cut (ALL) index interval is found once (cut_span); a coarse sample is masked by cut_sample, and a stretch in which
// every live lane's samples are cut is passed like an empty one (counted as skipped) before the cell maxima are
// looked at.  The few fractional points (refine, the cap test) evaluate the predicate itself.  Without CUT nothing of
// this is compiled.
template <int NL, int ESH, bool LIN, bool CUT>
__global__ __launch_bounds__(256) void iso_kernel(const IsoParams P) {
    const int nblocks = P.tiles_x * P.tiles_y;
    const int t = xcd_remap((int)blockIdx.x, nblocks);
    const int tile_x = t % P.tiles_x, tile_y = t / P.tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = tile_x * 16 + (wave & 1) * 8 + (lane & 7);
    const int r = tile_y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (c >= P.frame.out_w || r >= P.frame.out_h) return;
    const size_t o = (size_t)r * (size_t)P.frame.out_w + (size_t)c;
    const int x = P.frame.x0 + c;
    const int y = P.frame.y0 + (r / P.frame.band_h) * P.frame.band_pitch + (r % P.frame.band_h);

    Ray R;
    R.start = { 0.f, 0.f, 0.f }; R.step = { 0.f, 0.f, 0.f }; R.nsteps = 0;
    const bool frag = (x < P.frame.frame_w && y < P.frame.frame_h) && setup_ray(P, x, y, R);
    const int nsteps = frag ? R.nsteps : 0;
    const float iso = P.iso;
    const IsoArgs* kq = (const IsoArgs*)__builtin_amdgcn_kernarg_segment_ptr();     // P itself: the only argument

    const CutParams* cq = (const CutParams*)&kq->cut;       // wave-uniform: scalar loads, like the LOD table
    CutRay cr = { { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f } };
    CutSpan span = { 0, 0 };
    bool cut_all = false;
    if constexpr (CUT) {
        cut_all = cq->all != 0;
        cr = cut_ray(R, P.size);
        span = cut_span(*cq, cr, nsteps);
    }

    int cand = -1;                       // the coarse candidate
    uint32_t marched = 0u, skipped = 0u; // wave-uniform
    for (int i0 = 0; ; i0 += ISO_UNROLL) {
        const bool live = cand < 0 && i0 < nsteps;
        if (!__any(live)) break;
        bool work = live;
        if constexpr (CUT) {             // a stretch whose samples are all cut, for every live lane: nothing to fetch
            const int e = min(i0 + ISO_UNROLL, nsteps);
            const bool all_cut = cut_all ? (span.lo <= i0 && e <= span.hi) : (e <= span.lo || i0 >= span.hi);
            work = live && !all_cut;
            if (!__any(work)) { ++skipped; continue; }
        }
        // The LOD table is read from the kernel arguments afresh in each stretch (scalar loads from the constant
        // cache) instead of being held in SGPRs across the loop (composite_kernels.hip does the same).
        asm volatile("" : "+s"(kq));
        const IsoLod* Ls = (const IsoLod*)kq->L;
        if (P.skip) {
            const bool veto = work && stretch_may_reach<NL, ESH, LIN>(Ls, P, R, i0);
            if (!__any(veto)) { ++skipped; continue; }
        }
        ++marched;
        if constexpr (LIN) {
            if (work) {
#pragma unroll
                for (int g0 = 0; g0 < ISO_UNROLL; g0 += ISO_LIN_GROUP) {
                    if (cand >= 0 || i0 + g0 >= nsteps) break;       // the first one wins: later groups cannot
                    const char* addr[ISO_LIN_GROUP][8];
                    float frac[ISO_LIN_GROUP][3];
                    bool held[ISO_LIN_GROUP];
#pragma unroll
                    for (int j = 0; j < ISO_LIN_GROUP; ++j) {
                        const float iter = (float)(i0 + g0 + j);
                        const float cx = R.start.x + iter * R.step.x;
                        const float cy = R.start.y + iter * R.step.y;
                        const float cz = R.start.z + iter * R.step.z;
                        const float dx = cx * P.size[0], dy = cy * P.size[1], dz = cz * P.size[2];
                        held[j] = false;
                        svr_linear::LaneLod q = svr_linear::lane_lod_zero();
                        const char* base = static_cast<const char*>(Ls[0].density);   // a valid address for the unused gathers
                        bool done = i0 + g0 + j >= nsteps;
                        if constexpr (CUT) done = done || cut_sample(span, cut_all, i0 + g0 + j);
#pragma unroll
                        for (int l = 0; l < NL; ++l) {
                            size_t idx;
                            if (done || !lod_index(Ls[l], dx, dy, dz, idx)) continue;
                            done = true;
                            held[j] = true;
                            svr_linear::lane_lod_take(q, Ls[l], dx * Ls[l].scale[0], dy * Ls[l].scale[1], dz * Ls[l].scale[2]);
                            base = static_cast<const char*>(Ls[l].density);
                        }
                        const svr_linear::Cell cell = svr_linear::cell_of(q);
                        size_t o[8];
                        svr_linear::row_offsets(q, cell, o);
#pragma unroll
                        for (int k = 0; k < 8; ++k) addr[j][k] = base + (o[k] << ESH);
#pragma unroll
                        for (int a = 0; a < 3; ++a) frac[j][a] = cell.f[a];
                    }
                    float v8[ISO_LIN_GROUP][8];
#pragma unroll
                    for (int j = 0; j < ISO_LIN_GROUP; ++j)
#pragma unroll
                        for (int k = 0; k < 8; ++k) v8[j][k] = load_global<ESH>(addr[j][k]);
#pragma unroll
                    for (int j = ISO_LIN_GROUP - 1; j >= 0; --j)     // the first one wins
                        if (held[j] && svr_linear::blend(v8[j], frac[j]) >= iso) cand = i0 + g0 + j;
                }
            }
        } else if (work) {
            const char* addr[ISO_UNROLL];
            bool held[ISO_UNROLL];
#pragma unroll
            for (int j = 0; j < ISO_UNROLL; ++j) {
                const float iter = (float)(i0 + j);                  // == the march's float counter (nsteps <= 2^24)
                const float cx = R.start.x + iter * R.step.x;
                const float cy = R.start.y + iter * R.step.y;
                const float cz = R.start.z + iter * R.step.z;
                const float dx = cx * P.size[0], dy = cy * P.size[1], dz = cz * P.size[2];
                held[j] = false;                                     // no LOD holds it (or past the ray's end)
                addr[j] = static_cast<const char*>(Ls[0].density);   // a valid address for the unused gather
                bool done = i0 + j >= nsteps;
                if constexpr (CUT) done = done || cut_sample(span, cut_all, i0 + j);
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    size_t idx;
                    if (done || !lod_index(Ls[l], dx, dy, dz, idx)) continue;
                    done = true;
                    held[j] = true;
                    addr[j] = static_cast<const char*>(Ls[l].density) + (idx << ESH);
                }
            }
            float vals[ISO_UNROLL];
#pragma unroll
            for (int j = 0; j < ISO_UNROLL; ++j) vals[j] = load_global<ESH>(addr[j]);
#pragma unroll
            for (int j = ISO_UNROLL - 1; j >= 0; --j)                // the first one wins
                if (held[j] && vals[j] >= iso) cand = i0 + j;
        }
    }
    if (P.counters && lane == 0) {       // lane 0 is the tile's top-left pixel: inside the frame whenever the wave is
        atomicAdd(P.counters, marched);
        atomicAdd(P.counters + 1, skipped);
    }

    float4 color = make_float4(0.f, 0.f, 0.f, 0.f);
    float depth = 0.0f;
    f3 n = { 0.f, 0.f, 0.f };
    uint32_t label = 0u;
    uint8_t cls = frag ? SVR_PIX_MISS : SVR_PIX_DISCARD;
    unsigned long long pk = 0ull;
    if (cand >= 0) {
        cls = SVR_PIX_HIT;
        const IsoLod* Ls = (const IsoLod*)kq->L;
        // refine: the first sub-sample between the samples cand - 1 and cand that reaches the level
        float iter = (float)cand;
        float pred = (float)(cand - 1);                              // CUT: the point examined just before the hit
        if (cand > 0 && P.refine > 1) {
            const float base = (float)(cand - 1), rf = (float)P.refine;
            for (int k = 1; k < P.refine; ++k) {
                const float it = base + (float)k / rf;
                if constexpr (CUT) { if (cut_at(*cq, cr, it)) { pred = it; continue; } }     // no value here
                const float cx = R.start.x + it * R.step.x, cy = R.start.y + it * R.step.y, cz = R.start.z + it * R.step.z;
                float v = 0.0f; int lod = 0; size_t idx = 0;
                if (value_at<NL, ESH, LIN>(Ls, cx * P.size[0], cy * P.size[1], cz * P.size[2], v, lod, idx) && v >= iso) {
                    iter = it;
                    break;
                }
                pred = it;
            }
        }
        int cap = -1;                                                // CUT: the plane of a cap
        if constexpr (CUT) {
            if (cand > 0 && cut_at(*cq, cr, pred)) {
                for (uint32_t k = cq->count; k-- > 0u; )             // the lowest index wins
                    if (cut_all ? !cut_behind(*cq, k, cr, iter) : cut_behind(*cq, k, cr, pred)) cap = (int)k;
            }
        }
        const float cx = R.start.x + iter * R.step.x, cy = R.start.y + iter * R.step.y, cz = R.start.z + iter * R.step.z;
        const float dx = cx * P.size[0], dy = cy * P.size[1], dz = cz * P.size[2];
        int hl = 0; size_t hidx = 0;
        (void)cascade<NL>(Ls, dx, dy, dz, hl, hidx);                 // holds: this very point gave the hit value
        float sx = 1.0f, sy = 1.0f, sz = 1.0f;
#pragma unroll
        for (int l = 0; l < NL; ++l)
            if (hl == l) {
                sx = Ls[l].scale[0]; sy = Ls[l].scale[1]; sz = Ls[l].scale[2];
                label = Ls[l].labels ? Ls[l].labels[hidx] : 0u;
            }
        // gradient: central differences, one voxel of the hit's LOD per axis
        const float hx = 1.0f / sx, hy = 1.0f / sy, hz = 1.0f / sz;
        float tap[6];
        {
            const float px[6] = { dx + hx, dx - hx, dx, dx, dx, dx };
            const float py[6] = { dy, dy, dy + hy, dy - hy, dy, dy };
            const float pz[6] = { dz, dz, dz, dz, dz + hz, dz - hz };
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                float v = 0.0f; int lod = 0; size_t idx = 0;
                tap[k] = value_at<NL, ESH, LIN>(Ls, px[k], py[k], pz[k], v, lod, idx) ? v : 0.0f;
            }
        }
        const f3 g = { (tap[0] - tap[1]) * sx, (tap[2] - tap[3]) * sy, (tap[4] - tap[5]) * sz };
        const float* m = P.world_inv;
        const f3 G = { (m[0] * g.x + m[1] * g.y) + m[2] * g.z,
                       (m[4] * g.x + m[5] * g.y) + m[6] * g.z,
                       (m[8] * g.x + m[9] * g.y) + m[10] * g.z };
        // towards the viewer along the pixel's ray, in world space
        const f3 sd = { R.step.x * P.size[0], R.step.y * P.size[1], R.step.z * P.size[2] };
        const f3 w = { (P.world[0] * sd.x + P.world[4] * sd.y) + P.world[8] * sd.z,
                       (P.world[1] * sd.x + P.world[5] * sd.y) + P.world[9] * sd.z,
                       (P.world[2] * sd.x + P.world[6] * sd.y) + P.world[10] * sd.z };
        const float vl = sqrtf(dot3(w, w));
        f3 v = { 0.f, 0.f, 0.f };
        if (vl > 0.0f && vl < INFINITY) v = { -w.x / vl, -w.y / vl, -w.z / vl };
        const float gl = sqrtf(dot3(G, G));
        n = v;
        if (gl > 0.0f && gl < INFINITY) n = { -G.x / gl, -G.y / gl, -G.z / gl };
        if constexpr (CUT) {
            if (cap >= 0) {                                          // the cutting plane's unit normal, facing the viewer
                n = { cq->nhat[cap][0], cq->nhat[cap][1], cq->nhat[cap][2] };
                if (dot3(n, v) < 0.0f) n = { -n.x, -n.y, -n.z };
            }
        }
        f3 l = v;
        if (!P.headlight) l = { P.light[0], P.light[1], P.light[2] };
        const f3 hv = { l.x + v.x, l.y + v.y, l.z + v.z };
        const float hlen = sqrtf(dot3(hv, hv));
        f3 h = { 0.f, 0.f, 0.f };
        if (hlen > 0.0f && hlen < INFINITY) h = { hv.x / hlen, hv.y / hlen, hv.z / hlen };
        const float ndl = fabsf(dot3(n, l));
        float sp = fabsf(dot3(n, h));
        for (int k = 0; k < P.shininess_log2; ++k) sp = sp * sp;
        f3 base = { P.base[0], P.base[1], P.base[2] };
        if (P.tint) {
            const float* hs = P.colors + 4u * (label % P.color_count);
            base = hsv_to_rgb(hs[0], hs[1], 1.0f);
        }
        const float tt = P.ambient + P.diffuse * ndl;
        const float ss = P.specular * sp;
        color = make_float4(fminf(fmaxf(base.x * tt + ss, 0.0f), 1.0f), fminf(fmaxf(base.y * tt + ss, 0.0f), 1.0f),
                            fminf(fmaxf(base.z * tt + ss, 0.0f), 1.0f), P.opacity);
        {   // the march's shade_and_store depth formula at the hit coordinate
            const f4 wp = mat_vec(P.world, cx - 0.5f, cy - 0.5f, cz - 0.5f, 1.0f);
            const f4 ndc = mat_vec(P.pc, wp.x, wp.y, wp.z, wp.w);
            depth = ndc.z / fmaxf(ndc.w, 0.001f);
        }
        pk = (unsigned long long)min(P.pick_id, 0xFFFFFu) | ((unsigned long long)pick_field(cx) << 20) |
             ((unsigned long long)pick_field(cy) << 34) | ((unsigned long long)pick_field(cz) << 48);
    }
    reinterpret_cast<float4*>(P.rgba)[o] = color;
    if (P.depth) P.depth[o] = depth;
    if (P.label) P.label[o] = label;
    if (P.flags) P.flags[o] = cls;
    if (P.steps) P.steps[o] = cand >= 0 ? (uint32_t)(cand + 1) : (uint32_t)nsteps;
    if (P.pick) P.pick[o] = pk;
    if (P.normal) { P.normal[3 * o] = n.x; P.normal[3 * o + 1] = n.y; P.normal[3 * o + 2] = n.z; }
}

}  // namespace

// svr_iso has validated the arguments; it orders the launch against the uploads and marks it as a
// render.  interp: SVR_INTERP_*.  cut_planes: cut_count x abcd of svr_set_cut_planes (host), cut_mode: SVR_CUT_*; any
// plane selects the CUT instantiations, which doubles the kernels of this file (8 LOD counts x 3 element sizes x LIN x
// CUT = 96).
hipError_t svr_launch_iso(const svr_ctx* c, const svr_camera& cam, const svr_frame& fr, const svr_iso_params& ip,
                          const svr_outputs& out, int interp, const float* cut_planes, uint32_t cut_count, int cut_mode,
                          hipStream_t stream) {
    IsoParams P;
    memset(&P, 0, sizeof(P));
    CutPlanes cut;
    cut.count = cut_count; cut.mode = cut_mode;
    if (cut_count) memcpy(cut.abcd, cut_planes, sizeof(float) * 4 * cut_count);
    fill_ray_params(c, cam, fr, out, cut, P);
    memcpy(P.world_inv, cam.world_inv, sizeof(P.world_inv));
    P.iso = ip.iso_value; P.refine = ip.refine;
    for (int a = 0; a < 3; ++a) { P.base[a] = ip.iso_color[a]; P.light[a] = ip.light_direction[a]; }
    P.tint = ip.color_by_label != 0 && c->material.color_count > 0;
    P.ambient = ip.ambient; P.diffuse = ip.diffuse; P.specular = ip.specular;
    P.shininess_log2 = ip.shininess_log2; P.headlight = ip.headlight != 0;
    P.normal = ip.normal; P.counters = ip.skip_counters;
    // The cell test compares a maximum converted like a sample ((float) of u8 / u16 is exact) with iso_value itself, so
    // it is exact for integer rings.  Float rings keep max |v|: an upper bound of v, a proof only while iso_value > 0.
    // At iso_value <= 0 integer rings hit at the first resident sample anyway.
    bool any_cells = false;
    for (int l = 0; l < c->num_lods; ++l) {
        const LodStorage& S = c->lod[l];
        IsoLod& Q = P.L[l];
        fill_lod_common(S, Q);
        Q.cells = c->cells_dil_all ? S.cells_dil : nullptr;
        any_cells = any_cells || Q.cells;
        Q.cshift = S.cshift;
        for (int a = 0; a < 3; ++a) Q.cdim[a] = (uint32_t)S.cdim[a];
    }
    P.skip = any_cells && !ip.no_skip && ip.iso_value > 0.0f;
    const dim3 grid((unsigned)(P.tiles_x * P.tiles_y));
    return with_bool(cut_count != 0, [&](auto cutv) {
        return with_bool(interp == SVR_INTERP_LINEAR, [&](auto lin) {
            return with_lods_esh(c->num_lods, esh_of(c), [&](auto nl, auto esh) {
                return launch_tiles(iso_kernel<nl(), esh(), lin(), cutv()>, grid, 0, stream, P);
            });
        });
    });
}
