// What slice_kernels.hip, composite_kernels.hip and iso_kernels.hip share: the small vector helpers, the ring wrap and
// the LOD window test, the colour and pick helpers, the ray set-up of the march, the cut planes of the composite and iso
// kernels (predicate, per-ray index interval), and the host code that fills the parameter blocks and picks an
// instantiation.
//
// Arithmetic contract: strict IEEE f32 without contraction (-ffp-contract=off), operation order as written in svr.h.
// The device helpers restate the march's (march_kernel.hip: `mat_vec`, `wrap`, `lod_texel`, `pick_field`, `hsv_to_rgb`,
// `setup_ray`, `xcd_remap`), which keeps its own: the march sources are the kernel-source stamp bench.py records and
// stay untouched.  Every device helper is __forceinline__: the kernels rely on the expressions being visible to them.
#pragma once

#include <math.h>
#include <string.h>

#include <type_traits>

#include "svr_internal.h"

namespace svr_common {

struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };

// ---- device helpers --------------------------------------------------------------------------------------------------

__device__ __forceinline__ f4 mat_vec(const float* m, float x, float y, float z, float w) {
    f4 r;
    r.x = ((m[0] * x + m[4] * y) + m[8]  * z) + m[12] * w;
    r.y = ((m[1] * x + m[5] * y) + m[9]  * z) + m[13] * w;
    r.z = ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w;
    r.w = ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w;
    return r;
}

__device__ __forceinline__ float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// t in [0, shape), wrap0 in [0, ring) -> (t + wrap0) mod ring
__device__ __forceinline__ uint32_t wrap(uint32_t t, uint32_t wrap0, uint32_t ring) {
    const uint32_t w = t + wrap0;
    return min(w, w - ring);
}

// The LOD window test (sample_vol.wgsl:4-25): does L's ROI hold the data point d, and in which ring slots.  Lod: SliceLod /
// CompLod / IsoLod, which share the fields density, labels, off, shape, wrap0, ring, scale (fill_lod_common); templates
// rather than a common base keep every kernel argument at the offset it had.
template <class Lod>
__device__ __forceinline__ bool lod_slot(const Lod& L, float dx, float dy, float dz, uint32_t& wx, uint32_t& wy,
                                         uint32_t& wz) {
    const float sx = dx * L.scale[0], sy = dy * L.scale[1], sz = dz * L.scale[2];
    const int ix = (int)sx, iy = (int)sy, iz = (int)sz;
    const uint32_t tx = (uint32_t)(ix - L.off[0]), ty = (uint32_t)(iy - L.off[1]), tz = (uint32_t)(iz - L.off[2]);
    if (!(tx < L.shape[0] && ty < L.shape[1] && tz < L.shape[2])) return false;
    wx = wrap(tx, L.wrap0[0], L.ring[0]);
    wy = wrap(ty, L.wrap0[1], L.ring[1]);
    wz = wrap(tz, L.wrap0[2], L.ring[2]);
    return true;
}

// the same with the 64-bit element index in the rows (a float ring can exceed 4 GiB)
template <class Lod>
__device__ __forceinline__ bool lod_index(const Lod& L, float dx, float dy, float dz, size_t& idx) {
    uint32_t wx, wy, wz;
    if (!lod_slot(L, dx, dy, dz, wx, wy, wz)) return false;
    idx = ((size_t)wz * L.ring[1] + wy) * (size_t)L.ring[0] + wx;
    return true;
}

__device__ __forceinline__ uint32_t pick_field(float c) {
    const float f = c * 16383.0f;
    uint32_t u = 0u;
    if (f > 0.0f) u = f >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)f;
    return min(u, 16383u);
}

// (hsv_selection.wgsl:7-41)
__device__ __forceinline__ f3 hsv_to_rgb(float h, float s, float v) {
    f3 r;
    if (s == 0.0f) { r.x = v; r.y = v; r.z = v; return r; }
    const float h_scaled = h * 6.0f;
    const float fl = floorf(h_scaled);
    const int sector = (int)fl;
    const float fr = h_scaled - fl;
    const float p = v * (1.0f - s);
    const float q = v * (1.0f - s * fr);
    const float t = v * (1.0f - s * (1.0f - fr));
    if (sector == 0)      { r.x = v; r.y = t; r.z = p; }
    else if (sector == 1) { r.x = q; r.y = v; r.z = p; }
    else if (sector == 2) { r.x = p; r.y = v; r.z = t; }
    else if (sector == 3) { r.x = p; r.y = q; r.z = v; }
    else if (sector == 4) { r.x = t; r.y = p; r.z = v; }
    else                  { r.x = v; r.y = p; r.z = q; }
    return r;
}

// a texel at a byte address known to be in global memory (global_load rather than flat_load: the ring pointers come
// from the kernel arguments through a pointer the compiler cannot see into)
template <int ESH>
__device__ __forceinline__ float load_global(const char* a) {
    typedef __attribute__((address_space(1))) const uint8_t G8;
    typedef __attribute__((address_space(1))) const uint16_t G16;
    typedef __attribute__((address_space(1))) const float G32;
    if (ESH == 0) return (float)*(G8*)a;
    if (ESH == 1) return (float)*(G16*)a;
    return *(G32*)a;
}

// workgroups b and b + 8 share an XCD; each XCD gets one contiguous run of tiles
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
    const int per = nblocks >> 3;
    const int body = per << 3;
    if (b >= body) return b;
    return (b & 7) * per + (b >> 3);
}

// ---- rays ------------------------------------------------------------------------------------------------------------

struct Ray {
    f3 start, step;            // texture coordinates: sample i sits at start + (float)i * step
    int nsteps;
};

// The ray of the pixel (i, j) of the full frame (vs_main.wgsl:36-47 + fs_main.wgsl:20-48).  Returns false when no
// fragment runs for this pixel (discard).  Params: CompParams / IsoParams, which share the fields fill_ray_params fills.
template <class Params>
__device__ __forceinline__ bool setup_ray(const Params& P, int i, int j, Ray& R) {
    const float W = (float)P.frame.frame_w, H = (float)P.frame.frame_h;
    const float px = (2.0f * ((float)i + 0.5f)) / W - 1.0f;
    const float py = 1.0f - (2.0f * ((float)j + 0.5f)) / H;
    const f4 n4 = mat_vec(P.ndc_to_data, px, py, -1.0f, 1.0f);
    const f4 f4_ = mat_vec(P.ndc_to_data, px, py, 1.0f, 1.0f);
    const f3 far_pos  = { f4_.x / f4_.w, f4_.y / f4_.w, f4_.z / f4_.w };
    const f3 near_pos = { n4.x / n4.w, n4.y / n4.w, n4.z / n4.w };
    const f3 dir = { far_pos.x - near_pos.x, far_pos.y - near_pos.y, far_pos.z - near_pos.z };
    const float len = sqrtf(dot3(dir, dir));
    const f3 ray = { dir.x / len, dir.y / len, dir.z / len };

    const float lo = -0.5f;
    const float hx = P.size[0] - 0.5f, hy = P.size[1] - 0.5f, hz = P.size[2] - 0.5f;
    const float tx1 = (lo - near_pos.x) / ray.x, tx2 = (hx - near_pos.x) / ray.x;
    const float ty1 = (lo - near_pos.y) / ray.y, ty2 = (hy - near_pos.y) / ray.y;
    const float tz1 = (lo - near_pos.z) / ray.z, tz2 = (hz - near_pos.z) / ray.z;
    const float t_exit  = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    const float t_enter = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    if (!(t_enter <= t_exit)) return false;
    const f3 back = { near_pos.x + ray.x * t_exit, near_pos.y + ray.y * t_exit, near_pos.z + ray.z * t_exit };
    const f4 bw = mat_vec(P.world, back.x, back.y, back.z, 1.0f);
    const f4 bc = mat_vec(P.pc, bw.x, bw.y, bw.z, bw.w);
    if (!(bc.w > 0.0f) || !(bc.z >= 0.0f) || !(bc.z <= bc.w)) return false;
    if (P.clip_count) {
        const bool all = P.clip_all != 0;
        bool clipped = all;
        for (uint32_t k = 0; k < P.clip_count; ++k) {
            const bool behind = ((bw.x * P.clip[k][0] + bw.y * P.clip[k][1]) + bw.z * P.clip[k][2]) < P.clip[k][3];
            clipped = all ? (clipped && behind) : (clipped || behind);
        }
        if (clipped) return false;
    }

    const f3 nb = { near_pos.x - back.x, near_pos.y - back.y, near_pos.z - back.z };
    float dist = dot3(nb, ray);
    dist = fmaxf(dist, fminf((-0.5f - back.x) / ray.x, (P.size[0] - 0.5f - back.x) / ray.x));
    dist = fmaxf(dist, fminf((-0.5f - back.y) / ray.y, (P.size[1] - 0.5f - back.y) / ray.y));
    dist = fmaxf(dist, fminf((-0.5f - back.z) / ray.z, (P.size[2] - 0.5f - back.z) / ray.z));
    const f3 front = { back.x + ray.x * dist, back.y + ray.y * dist, back.z + ray.z * dist };
    float nf = -dist / P.rel_step + 0.5f;
    if (!(nf >= 1.0f)) return false;
    if (nf > 16777216.0f) nf = 16777216.0f;
    R.nsteps = (int)nf;
    const float nstepsf = (float)R.nsteps;
    R.start = { (front.x + 0.5f) / P.size[0], (front.y + 0.5f) / P.size[1], (front.z + 0.5f) / P.size[2] };
    R.step = { ((back.x - front.x) / P.size[0]) / nstepsf,
               ((back.y - front.y) / P.size[1]) / nstepsf,
               ((back.z - front.z) / P.size[2]) / nstepsf };
    return true;
}

// ---- cut planes (svr_set_cut_planes, include/svr.h) -------------------------------------------------------------------

// The context's planes as the caller gave them (host state: CutState of svr_host.h).
struct CutPlanes {
    uint32_t count;
    int32_t  mode;                                 // SVR_CUT_ANY / SVR_CUT_ALL
    float    abcd[SVR_MAX_CUT_PLANES][4];          // world space
};

// What the CUT kernels read: the planes carried into data space for this call's world transform, and the unit normals
// of the caps.  Appended to CompParams / IsoParams AFTER L[], so every other kernel argument keeps its offset.
struct CutParams {
    uint32_t count;
    int32_t  all;                                  // 1: SVR_CUT_ALL
    float    gh[SVR_MAX_CUT_PLANES][4];            // g_k.xyz, h_k
    float    nhat[SVR_MAX_CUT_PLANES][3];
};

// The predicate of svr.h along one ray: E_k(iter) = A_k + iter * B_k, behind_k = E_k < 0.  p0 and sd are the ray's
// data-space origin and step.  A_k and B_k are recomputed from the (wave-uniform, scalar) plane data where they are
// needed rather than held per lane: 8 planes would take 16 VGPRs across the sample loop.
struct CutRay { f3 p0, sd; };

__device__ __forceinline__ CutRay cut_ray(const Ray& R, const float* size) {
    CutRay c;
    c.p0 = { R.start.x * size[0] - 0.5f, R.start.y * size[1] - 0.5f, R.start.z * size[2] - 0.5f };
    c.sd = { R.step.x * size[0], R.step.y * size[1], R.step.z * size[2] };
    return c;
}

template <class Cut>
__device__ __forceinline__ bool cut_behind(const Cut& C, uint32_t k, const CutRay& c, float iter) {
    const f3 g = { C.gh[k][0], C.gh[k][1], C.gh[k][2] };
    const float A = dot3(g, c.p0) + C.gh[k][3];
    const float B = dot3(g, c.sd);
    return (A + iter * B) < 0.0f;
}

template <class Cut>
__device__ __forceinline__ bool cut_at(const Cut& C, const CutRay& c, float iter) {
    const bool all = C.all != 0;
    bool cut = all;
    for (uint32_t k = 0; k < C.count; ++k) {
        const bool behind = cut_behind(C, k, c, iter);
        cut = all ? (cut && behind) : (cut || behind);
    }
    return cut;
}

// The integer samples of a ray in one interval: with `all` the samples i in [lo, hi) are the CUT ones, without it they
// are the KEPT ones.  Along a ray E_k is monotone in iter under f32 rounding too (iter * B_k is a monotone rounded
// product, adding A_k is monotone), so each plane's behind-set over i = 0 .. nsteps-1 is a prefix or a suffix: its two
// ends tell which, and a binary search on the predicate itself finds where it flips (at most 24 probes: nsteps <= 2^24).
// Under ANY the kept samples are the intersection of the complements, under ALL the cut samples are the intersection of
// the behind-sets: an interval either way.  The interval agrees with the predicate exactly because it is made of
// nothing else.
struct CutSpan { int lo, hi; };

template <class Cut>
__device__ __forceinline__ CutSpan cut_span(const Cut& C, const CutRay& c, int nsteps) {
    const bool all = C.all != 0;
    CutSpan s = { 0, nsteps };
    for (uint32_t k = 0; k < C.count; ++k) {
        const f3 g = { C.gh[k][0], C.gh[k][1], C.gh[k][2] };
        const float A = dot3(g, c.p0) + C.gh[k][3];
        const float B = dot3(g, c.sd);
        const bool b0 = (A + 0.0f * B) < 0.0f;
        const bool bn = (A + (float)(nsteps - 1) * B) < 0.0f;
        int lo = 0, hi = nsteps;                   // the behind-set [lo, hi)
        if (b0 == bn) {
            if (!b0) hi = 0;
        } else {
            int a = 0, b = nsteps - 1;             // behind(a) == b0, behind(b) != b0
            while (b - a > 1) {
                const int m = a + ((b - a) >> 1);
                const bool bm = (A + (float)m * B) < 0.0f;
                if (bm == b0) a = m; else b = m;
            }
            if (b0) hi = b; else lo = b;
        }
        if (!all) {                                // the kept set of this plane: the complement, an interval too
            if (lo == 0) { lo = hi; hi = nsteps; } else { hi = lo; lo = 0; }
        }
        s.lo = max(s.lo, lo);
        s.hi = min(s.hi, hi);
    }
    if (s.hi <= s.lo) s.lo = s.hi = 0;             // one form for the empty interval
    return s;
}

// two integer compares (one after the subtraction)
__device__ __forceinline__ bool cut_sample(const CutSpan& s, bool all, int i) {
    const bool inside = (uint32_t)(i - s.lo) < (uint32_t)(s.hi - s.lo);
    return inside == all;
}

// ---- host ------------------------------------------------------------------------------------------------------------

// f32 matrix helpers in the contract's operation order (see oracle/lmip_oracle.c header)
inline void mat_vec4(const float* m, const float* v, float* r) {
    for (int i = 0; i < 4; ++i) r[i] = ((m[0 + i] * v[0] + m[4 + i] * v[1]) + m[8 + i] * v[2]) + m[12 + i] * v[3];
}
inline void mat_mul4(const float* a, const float* b, float* out) {
    for (int c = 0; c < 4; ++c) mat_vec4(a, b + 4 * c, out + 4 * c);
}

// log2 of the density element size: 0 u8, 1 u16, 2 f32
inline int esh_of(const svr_ctx* c) { return c->density_storage == SVR_U8 ? 0 : (c->density_storage == SVR_U16 ? 1 : 2); }

template <class Lod>
void fill_lod_common(const LodStorage& S, Lod& Q) {
    Q.density = S.density; Q.labels = S.labels;
    for (int a = 0; a < 3; ++a) {
        Q.off[a] = S.state.offset[a];
        Q.shape[a] = (uint32_t)S.state.shape[a];
        Q.ring[a] = (uint32_t)S.ring[a];
        Q.wrap0[a] = (uint32_t)(S.state.offset[a] % S.ring[a]);     // (svr_set_lod_state: offsets are >= 0)
        Q.scale[a] = S.state.scale[a];
    }
}

// camera, material and outputs of a mode that draws along the march's rays
// the per-call host part of the cut predicate (svr.h): g_k, h_k from the call's world matrix, and the unit normals
inline void fill_cut_params(const CutPlanes& cut, const float* m, CutParams& Q) {
    Q.count = cut.count;
    Q.all = cut.mode == SVR_CUT_ALL;
    for (uint32_t k = 0; k < cut.count; ++k) {
        const float a = cut.abcd[k][0], b = cut.abcd[k][1], c = cut.abcd[k][2], d = cut.abcd[k][3];
        Q.gh[k][0] = (m[0] * a + m[1] * b) + m[2] * c;
        Q.gh[k][1] = (m[4] * a + m[5] * b) + m[6] * c;
        Q.gh[k][2] = (m[8] * a + m[9] * b) + m[10] * c;
        Q.gh[k][3] = ((m[12] * a + m[13] * b) + m[14] * c) - d;
        const float len = sqrtf((a * a + b * b) + c * c);
        Q.nhat[k][0] = a / len; Q.nhat[k][1] = b / len; Q.nhat[k][2] = c / len;
    }
}

template <class Params>
void fill_ray_params(const svr_ctx* c, const svr_camera& cam, const svr_frame& fr, const svr_outputs& out,
                     const CutPlanes& cut, Params& P) {
    fill_cut_params(cut, cam.world, P.cut);
    float tmp[16];
    mat_mul4(cam.world_inv, cam.cam_inv, tmp);               // as svr_render (vs_main.wgsl:22, left-assoc)
    mat_mul4(tmp, cam.proj_inv, P.ndc_to_data);
    mat_mul4(cam.proj, cam.cam, P.pc);
    memcpy(P.world, cam.world, sizeof(P.world));
    for (int a = 0; a < 3; ++a) P.size[a] = cam.volume_dimensions[a];
    const float mx = fmaxf(P.size[0], fmaxf(P.size[1], P.size[2]));
    P.rel_step = fminf(fmaxf(sqrtf(mx) / 20.0f, 0.1f), 0.8f);   // fs_main.wgsl:20
    P.frame = fr;
    const svr_material& m = c->material;
    P.opacity = m.opacity;
    P.clip_count = m.clipping_plane_count; P.clip_all = m.clipping_mode_all;
    for (uint32_t k = 0; k < m.clipping_plane_count; ++k)
        for (int a = 0; a < 4; ++a) P.clip[k][a] = c->clip_host[4 * k + a];
    P.color_count = m.color_count; P.colors = c->colors_dev;
    P.tiles_x = (fr.out_w + 15) / 16; P.tiles_y = (fr.out_h + 15) / 16;
    P.rgba = out.rgba; P.depth = out.depth; P.label = out.label; P.flags = out.flags; P.steps = out.steps;
    P.pick = reinterpret_cast<unsigned long long*>(out.pick); P.pick_id = out.pick_id;
}

// Run-time values into template arguments: f(std::integral_constant<int, NL>, std::integral_constant<int, ESH>) for
// num_lods in 1 .. SVR_MAX_LODS and esh in 0 .. 2; f(std::bool_constant<B>) for a flag.  Each returns what f returns.
template <class F>
auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

template <class F>
auto with_lods_esh(int num_lods, int esh, F&& f) {
    auto with_esh = [&](auto nl) {
        if (esh == 0) return f(nl, std::integral_constant<int, 0>{});
        if (esh == 1) return f(nl, std::integral_constant<int, 1>{});
        return f(nl, std::integral_constant<int, 2>{});
    };
    switch (num_lods) {
        case 1: return with_esh(std::integral_constant<int, 1>{});
        case 2: return with_esh(std::integral_constant<int, 2>{});
        case 3: return with_esh(std::integral_constant<int, 3>{});
        case 4: return with_esh(std::integral_constant<int, 4>{});
        case 5: return with_esh(std::integral_constant<int, 5>{});
        case 6: return with_esh(std::integral_constant<int, 6>{});
        case 7: return with_esh(std::integral_constant<int, 7>{});
        default: return with_esh(std::integral_constant<int, 8>{});
    }
}

// one workgroup of 256 threads per tile
template <class Kernel, class Params>
hipError_t launch_tiles(Kernel kernel, dim3 grid, size_t lds, hipStream_t stream, const Params& P) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, P);
    return hipGetLastError();
}

}  // namespace svr_common
