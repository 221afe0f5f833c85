// Display-side output: what a canvas shows for this object over a background.
// The fragment outputs of the march (out.color before blending, out.depth; fs_main.wgsl:86-87) are blended
// "over" a vertical-gradient background (the reference's tests add gfx.Background(None,
// BackgroundMaterial(bottom, top)), tests/conftest.py:17-22), depth-tested against an optional existing depth
// plane, encoded linear -> sRGB and quantised to 8 bits.  Blending and the final encode are pygfx's, restated
// (parity unpinned).  Pure HBM streaming: 21 B read + 4 B written per pixel, one thread per pixel.
#include <algorithm>

#include "svr_host.h"

namespace {

__device__ __forceinline__ float srgb_encode(float c) {          // IEC 61966-2-1 OETF
    c = fminf(fmaxf(c, 0.0f), 1.0f);
    return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f;
}

__device__ __forceinline__ uint32_t quant8(float v) {
    return (uint32_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f);
}

__global__ __launch_bounds__(256) void compose_kernel(const float4* __restrict__ rgba, const float* __restrict__ depth,
                                                      const uint8_t* __restrict__ flags, int w, int h,
                                                      svr_compose_params q, uint32_t* __restrict__ out8,
                                                      float* __restrict__ zbuf) {
    const size_t n = (size_t)w * (size_t)h;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / (size_t)w);
        const float t = ((float)y + 0.5f) / (float)h;              // 0 at the top row
        float c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = q.bg_top[k] * (1.0f - t) + q.bg_bottom[k] * t;
        bool draw = flags ? flags[i] != SVR_PIX_DISCARD : true;
        if (draw && zbuf && depth) draw = depth[i] < zbuf[i];      // depth_compare "<"
        if (draw) {
            const float4 s = rgba[i];
            const float a = s.w;
            c[0] = s.x * a + c[0] * (1.0f - a);                    // src_alpha, one_minus_src_alpha
            c[1] = s.y * a + c[1] * (1.0f - a);
            c[2] = s.z * a + c[2] * (1.0f - a);
            c[3] = a + c[3] * (1.0f - a);
            if (zbuf && depth) zbuf[i] = depth[i];
        }
        if (q.srgb_encode) { c[0] = srgb_encode(c[0]); c[1] = srgb_encode(c[1]); c[2] = srgb_encode(c[2]); }
        out8[i] = quant8(c[0]) | (quant8(c[1]) << 8) | (quant8(c[2]) << 16) | (quant8(c[3]) << 24);
    }
}

}  // namespace

hipError_t svr_launch_compose(const float* rgba, const float* depth, const uint8_t* flags, int w, int h,
                              const svr_compose_params& q, uint8_t* out_rgba8, float* zbuf, hipStream_t stream) {
    const size_t n = (size_t)w * (size_t)h;
    if (n == 0) return hipSuccess;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(compose_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const float4*>(rgba), depth,
                       flags, w, h, q, reinterpret_cast<uint32_t*>(out_rgba8), zbuf);
    return hipGetLastError();
}

// ---- outline (svr_outline, include/svr.h): label edges of one render over its RGBA, selected-object highlighting.
// One workgroup of 256 threads per 32 x 8 pixel tile, one pixel per thread.  The tile plus an r-pixel halo of hit
// bits, labels and (with a depth tolerance) depths is staged in LDS; halo pixels outside the image take the value
// of the nearest border pixel, which leaves every window minimum and maximum unchanged (they are already in the
// window), so "outside pixels are not neighbours" costs nothing.  The window test is separable:
//   some q in N_r(p) is a miss/discard or has another label  <=>  the window holds a non-hit, or its label minimum
//     over hits is < L(p), or its maximum is > L(p)   (p itself is a hit with label L(p) and does not change either)
//   some hit q has |Z(q) - Z(p)| > tau  <=>  fl(zmax - Z(p)) > tau or fl(Z(p) - zmin) > tau   (f32 rounding is
//     monotone; non-hits stage NaN depths, which fminf / fmaxf skip, as the definition skips their depths)
// so a row pass (2r + 1 reads per cell of the tile's columns over its rows plus halo) and a column pass (2r + 1
// reads per pixel) replace the (2r + 1)^2 window.  rgba is read and written once per pixel (16-byte accesses).
namespace {

constexpr int kOutlineTileW = 32, kOutlineTileH = 8;

struct OutlineLds {                 // carve of the dynamic LDS block (4-byte arrays first, then the byte arrays)
    uint32_t* lab;                  // staged [sh][sw]
    float* z;                       // staged [sh][sw] (depth tolerance on)
    uint32_t *lmin, *lmax;          // row pass [sh][kOutlineTileW]
    float *zmin, *zmax;             // row pass (depth tolerance on)
    uint8_t* hit;                   // staged
    uint8_t* nh;                    // row pass: the row window holds a non-hit
};

__host__ __device__ inline size_t outline_lds_layout(int r, bool use_z, uint8_t* base, OutlineLds* l) {
    const size_t ns = (size_t)(kOutlineTileW + 2 * r) * (kOutlineTileH + 2 * r);
    const size_t nr = (size_t)kOutlineTileW * (kOutlineTileH + 2 * r);
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t* p = base ? base + o : nullptr; o += bytes; return p; };
    uint8_t* lab = take(ns * 4);
    uint8_t* z = use_z ? take(ns * 4) : nullptr;
    uint8_t* lmin = take(nr * 4);
    uint8_t* lmax = take(nr * 4);
    uint8_t* zmin = use_z ? take(nr * 4) : nullptr;
    uint8_t* zmax = use_z ? take(nr * 4) : nullptr;
    uint8_t* hit = take(ns);
    uint8_t* nh = take(nr);
    if (l) {
        l->lab = reinterpret_cast<uint32_t*>(lab); l->z = reinterpret_cast<float*>(z);
        l->lmin = reinterpret_cast<uint32_t*>(lmin); l->lmax = reinterpret_cast<uint32_t*>(lmax);
        l->zmin = reinterpret_cast<float*>(zmin); l->zmax = reinterpret_cast<float*>(zmax);
        l->hit = hit; l->nh = nh;
    }
    return o;
}

// hsv_selection.wgsl:7-41 at v = 1 (march_kernel.hip hsv_to_rgb); the sector is compared as a float, which is the
// same test for every hue whose sector fits an int and sends NaN and huge hues to the last branch
__device__ __forceinline__ float3 outline_hsv_to_rgb(float h, float s, float v) {
    if (s == 0.0f) return make_float3(v, v, v);
    const float h_scaled = h * 6.0f;
    const float fl = floorf(h_scaled);
    const float fr = h_scaled - fl;
    const float p = v * (1.0f - s);
    const float q = v * (1.0f - s * fr);
    const float t = v * (1.0f - s * (1.0f - fr));
    if (fl == 0.0f) return make_float3(v, t, p);
    if (fl == 1.0f) return make_float3(q, v, p);
    if (fl == 2.0f) return make_float3(p, v, t);
    if (fl == 3.0f) return make_float3(p, q, v);
    if (fl == 4.0f) return make_float3(t, p, v);
    return make_float3(v, p, q);
}

// lower-bound search; every probe lies in [0, n) whatever the order of `s`
__device__ __forceinline__ bool outline_in_set(const uint32_t* __restrict__ s, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && s[lo] == v;
}

// rgba and out are not __restrict__: they may be the same plane (each thread reads its pixel before writing it)
__global__ __launch_bounds__(256) void outline_kernel(const float4* rgba, const float* __restrict__ depth,
                                                      const uint32_t* __restrict__ label, const uint8_t* __restrict__ flags,
                                                      int w, int h, svr_outline_params q,
                                                      const float4* __restrict__ colors, uint32_t ncolors,
                                                      const uint32_t* __restrict__ sel, uint32_t nsel, float4* out,
                                                      uint8_t* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) uint8_t outline_lds[];
    const int r = q.radius;
    const float tau = q.depth_tolerance;
    const bool use_z = tau >= 0.0f;
    OutlineLds l;
    outline_lds_layout(r, use_z, outline_lds, &l);
    const int sw = kOutlineTileW + 2 * r, sh = kOutlineTileH + 2 * r;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kOutlineTileW, y0 = blockIdx.y * kOutlineTileH;
    const int tx = tid % kOutlineTileW, ty = tid / kOutlineTileW;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < w && y < h;
    const size_t pix = (size_t)y * (size_t)w + (size_t)x;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) s = rgba[pix];                      // issued first: its latency hides under the staging

    // stage tile + halo (border-replicated)
    for (int c = tid; c < sw * sh; c += 256) {
        const int sy = c / sw, sx = c - sy * sw;
        const int gy = min(max(y0 - r + sy, 0), h - 1), gx = min(max(x0 - r + sx, 0), w - 1);
        const size_t g = (size_t)gy * (size_t)w + (size_t)gx;
        const bool hq = flags[g] == SVR_PIX_HIT;
        l.hit[c] = hq;
        l.lab[c] = label[g];
        if (use_z) l.z[c] = hq ? depth[g] : __builtin_nanf("");
    }
    __syncthreads();

    // row pass: cell (ry, cx) = window over staged row ry, columns cx .. cx + 2r
    for (int c = tid; c < kOutlineTileW * sh; c += 256) {
        const int ry = c / kOutlineTileW, cx = c % kOutlineTileW;
        const int b = ry * sw + cx;
        uint32_t lmin = 0xFFFFFFFFu, lmax = 0u;
        bool nh = false;
        float zmin = __builtin_nanf(""), zmax = __builtin_nanf("");
        for (int k = 0; k <= 2 * r; ++k) {
            const uint32_t lq = l.lab[b + k];
            if (l.hit[b + k]) { lmin = min(lmin, lq); lmax = max(lmax, lq); }
            else nh = true;
        }
        if (use_z)
            for (int k = 0; k <= 2 * r; ++k) { zmin = fminf(zmin, l.z[b + k]); zmax = fmaxf(zmax, l.z[b + k]); }
        l.lmin[c] = lmin; l.lmax[c] = lmax; l.nh[c] = nh;
        if (use_z) { l.zmin[c] = zmin; l.zmax[c] = zmax; }
    }
    __syncthreads();
    if (!inside) return;

    const int centre = (ty + r) * sw + (tx + r);
    float4 o = s;
    bool edge = false;
    if (l.hit[centre]) {
        const uint32_t lp = l.lab[centre];
        const bool selected = nsel == 0 || outline_in_set(sel, nsel, lp);
        if (!selected) { o.x = s.x * q.dim_unselected; o.y = s.y * q.dim_unselected; o.z = s.z * q.dim_unselected; }
        if (!q.only_selected || selected) {
            uint32_t lmin = 0xFFFFFFFFu, lmax = 0u;
            bool nh = false;
            for (int k = 0; k <= 2 * r; ++k) {
                const int c = (ty + k) * kOutlineTileW + tx;
                lmin = min(lmin, l.lmin[c]); lmax = max(lmax, l.lmax[c]); nh |= l.nh[c] != 0;
            }
            edge = nh || lmin < lp || lmax > lp;
            if (use_z && !edge) {
                float zmin = __builtin_nanf(""), zmax = __builtin_nanf("");
                for (int k = 0; k <= 2 * r; ++k) {
                    const int c = (ty + k) * kOutlineTileW + tx;
                    zmin = fminf(zmin, l.zmin[c]); zmax = fmaxf(zmax, l.zmax[c]);
                }
                const float zp = l.z[centre];
                edge = zmax - zp > tau || zp - zmin > tau;
            }
        }
        if (edge) {
            float3 c = make_float3(q.color[0], q.color[1], q.color[2]);
            if (q.color_by_label) {
                const float4 hsv = colors[lp % ncolors];
                c = outline_hsv_to_rgb(hsv.x, hsv.y, 1.0f);
            }
            const float a = q.color[3], oma = 1.0f - a;
            o.x = o.x * oma + c.x * a;
            o.y = o.y * oma + c.y * a;
            o.z = o.z * oma + c.z * a;
            o.w = o.w * oma + a;
        }
    }
    out[pix] = o;
    if (mask) mask[pix] = edge ? 1 : 0;
}

}  // namespace

hipError_t svr_launch_outline(const float* rgba, const float* depth, const uint32_t* label, const uint8_t* flags, int w,
                              int h, const svr_outline_params& q, const float* colors, uint32_t ncolors,
                              const uint32_t* sel, uint32_t nsel, float* out, uint8_t* mask, hipStream_t stream) {
    if (w == 0 || h == 0) return hipSuccess;
    const size_t lds = outline_lds_layout(q.radius, q.depth_tolerance >= 0.0f, nullptr, nullptr);
    const dim3 grid(((unsigned)w + kOutlineTileW - 1) / kOutlineTileW, ((unsigned)h + kOutlineTileH - 1) / kOutlineTileH);
    hipLaunchKernelGGL(outline_kernel, grid, dim3(256), lds, stream, reinterpret_cast<const float4*>(rgba), depth, label,
                       flags, w, h, q, reinterpret_cast<const float4*>(colors), ncolors, sel, nsel,
                       reinterpret_cast<float4*>(out), mask);
    return hipGetLastError();
}
