// Composite render mode (svr_composite, include/svr.h): front-to-back emission-absorption compositing through a
// transfer-function table along the march's own rays.  One lane = one pixel; a workgroup of 256 threads is a 16 x 16
// pixel tile of four 8 x 8 wave tiles (march_simple's layout), placed on the XCDs like march_simple's fallback.  The
// table sits in LDS (K x 16 bytes, at most 64 KiB).
//
// Per lane, samples go in batches of COMP_UNROLL: the LOD and address of every sample of the batch first, then their
// gathers (all in flight together), then the serial compositing in increasing sample order.  Samples past the ray's
// end or past the termination point of the batch are discarded, so the result is that of a serial loop.  A lane leaves
// after its terminating batch; a wave leaves when all its lanes have.
//
// Arithmetic contract: strict IEEE f32 without contraction (-ffp-contract=off), operation order as written in svr.h.
// The device helpers below are copies of the march's (march_kernel.hip), whose bytes are the kernel-source stamp
// bench.py records and stay untouched; tests/test_gpu_composite.py holds this kernel to tests/composite_twin.py.
#include <math.h>
#include <string.h>

#include "svr_internal.h"
#include "linear_sample.h"

namespace {

struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };

struct CompLod {
    const void*     density;   // ring [z][y][x], element type per CompParams::esh
    const uint32_t* labels;    // null: no label rings
    int32_t  off[3];           // current_logical_offset_in_pixels
    uint32_t shape[3];         // current_logical_shape_in_pixels
    uint32_t wrap0[3];         // ring slot of the ROI's first voxel
    uint32_t ring[3];
    float    scale[3];
};

struct CompParams {
    float ndc_to_data[16];     // world_inv * cam_inv * proj_inv, as svr_render forms it
    float pc[16];              // proj * cam
    float world[16];
    float size[3];
    float rel_step;
    svr_frame frame;
    float clim0, clim1, opacity, alpha_cutoff;
    uint32_t clip_count;
    int32_t  clip_all;
    float    clip[SVR_MAX_CLIP_PLANES][4];
    uint32_t color_count;
    const float* colors;       // device, color_count x vec4 (h, s, v, pad)
    const float* table;        // device, K x RGBA
    int32_t  K;
    int32_t  tiles_x, tiles_y;
    float*    rgba;
    float*    depth;
    uint32_t* label;
    uint8_t*  flags;
    uint32_t* steps;
    unsigned long long* pick; uint32_t pick_id;
    CompLod L[SVR_MAX_LODS];
};

// march_kernel.hip `mat_vec`
__device__ __forceinline__ f4 mat_vec(const float* m, float x, float y, float z, float w) {
    f4 r;
    r.x = ((m[0] * x + m[4] * y) + m[8]  * z) + m[12] * w;
    r.y = ((m[1] * x + m[5] * y) + m[9]  * z) + m[13] * w;
    r.z = ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w;
    r.w = ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w;
    return r;
}

__device__ __forceinline__ float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// march_kernel.hip `wrap`
__device__ __forceinline__ uint32_t wrap(uint32_t t, uint32_t wrap0, uint32_t ring) {
    const uint32_t w = t + wrap0;
    return min(w, w - ring);
}

// march_kernel.hip `lod_texel` (sample_vol.wgsl:4-25), with a 64-bit element index (a float ring can exceed 4 GiB)
__device__ __forceinline__ bool lod_index(const CompLod& L, float dx, float dy, float dz, size_t& idx) {
    const float sx = dx * L.scale[0], sy = dy * L.scale[1], sz = dz * L.scale[2];
    const int ix = (int)sx, iy = (int)sy, iz = (int)sz;
    const uint32_t tx = (uint32_t)(ix - L.off[0]), ty = (uint32_t)(iy - L.off[1]), tz = (uint32_t)(iz - L.off[2]);
    if (!(tx < L.shape[0] && ty < L.shape[1] && tz < L.shape[2])) return false;
    const uint32_t wx = wrap(tx, L.wrap0[0], L.ring[0]);
    const uint32_t wy = wrap(ty, L.wrap0[1], L.ring[1]);
    const uint32_t wz = wrap(tz, L.wrap0[2], L.ring[2]);
    idx = ((size_t)wz * L.ring[1] + wy) * (size_t)L.ring[0] + wx;
    return true;
}

// march_kernel.hip `pick_field`
__device__ __forceinline__ uint32_t pick_field(float c) {
    const float f = c * 16383.0f;
    uint32_t u = 0u;
    if (f > 0.0f) u = f >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)f;
    return min(u, 16383u);
}

// march_kernel.hip `hsv_to_rgb` (hsv_selection.wgsl:7-41)
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

struct Ray {
    f3 start, step;
    int nsteps;
};

// march_kernel.hip `setup_ray` (vs_main.wgsl:36-47 + fs_main.wgsl:20-48) for the pixel (i, j) of the full frame.
// Returns false when no fragment runs for this pixel (discard).
__device__ __forceinline__ bool setup_ray(const CompParams& P, int i, int j, Ray& R) {
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

// march_kernel.hip `xcd_remap`: workgroups b and b + 8 share an XCD; each XCD gets one contiguous run of tiles
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
    const int per = nblocks >> 3;
    const int body = per << 3;
    if (b >= body) return b;
    return (b & 7) * per + (b >> 3);
}

// a texel at a byte address known to be in global memory (slice_kernels.hip `load_global`)
template <int ESH>
__device__ __forceinline__ float load_global(const char* a) {
    typedef __attribute__((address_space(1))) const uint8_t G8;
    typedef __attribute__((address_space(1))) const uint16_t G16;
    typedef __attribute__((address_space(1))) const float G32;
    if (ESH == 0) return (float)*(G8*)a;
    if (ESH == 1) return (float)*(G16*)a;
    return *(G32*)a;
}

using CompArgs = const CompParams __attribute__((address_space(4)));     // the kernel arguments' own address space

constexpr int COMP_UNROLL = 8;     // samples whose gathers are in flight together per lane
constexpr int COMP_LIN_UNROLL = 4; // the same under linear sampling: 4 samples x 8 corners = 32 gathers in flight

// LIN: s of every sample is the linear sample of svr.h (svr_set_interpolation); labels stay the nearest sample's.
template <int NL, int ESH, bool TINT, bool LIN>
__global__ __launch_bounds__(256) void composite_kernel(const CompParams P) {
    constexpr int U = LIN ? COMP_LIN_UNROLL : COMP_UNROLL;
    extern __shared__ float4 lut[];
    for (int k = threadIdx.x; k < P.K; k += 256) lut[k] = reinterpret_cast<const float4*>(P.table)[k];
    __syncthreads();

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
    const bool frag = (x < P.frame.frame_w && y < P.frame.frame_h) && setup_ray(P, x, y, R);
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, ca = 0.0f, w_best = 0.0f;
    int best = -1, first = -1;
    uint32_t best_label = 0u, steps = 0u;
    if (frag) {
        const float kmax = (float)(P.K - 1);
        const float inv_lo = P.clim0, span = P.clim1 - P.clim0;
        const CompArgs* kq = (const CompArgs*)__builtin_amdgcn_kernarg_segment_ptr();     // P itself: the only argument
        bool alive = true;
        for (int i0 = 0; alive && i0 < R.nsteps; i0 += U) {
            // The LOD table is read from the kernel arguments afresh in each batch (scalar loads from the constant
            // cache) instead of being held in SGPRs across the loop (slice_kernels.hip does the same).
            asm volatile("" : "+s"(kq));
            const CompLod* Ls = (const CompLod*)kq->L;
            const uint32_t* laddr[U];
            int sl[U];
            float vals[U];
            if constexpr (!LIN) {
            const char* addr[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float iter = (float)(i0 + j);                  // == the march's float counter (nsteps <= 2^24)
                const float cx = R.start.x + iter * R.step.x;
                const float cy = R.start.y + iter * R.step.y;
                const float cz = R.start.z + iter * R.step.z;
                const float dx = cx * P.size[0], dy = cy * P.size[1], dz = cz * P.size[2];
                sl[j] = NL;                                          // no LOD holds it (or past the ray's end)
                addr[j] = static_cast<const char*>(Ls[0].density);   // a valid address for the unused gather
                laddr[j] = nullptr;
                bool done = i0 + j >= R.nsteps;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    size_t idx;
                    if (done || !lod_index(Ls[l], dx, dy, dz, idx)) continue;
                    done = true;
                    sl[j] = l;
                    addr[j] = static_cast<const char*>(Ls[l].density) + (idx << ESH);
                    if (TINT && Ls[l].labels) laddr[j] = Ls[l].labels + idx;
                }
            }
#pragma unroll
            for (int j = 0; j < U; ++j) vals[j] = load_global<ESH>(addr[j]);
            } else {
            const char* addr[U][8];
            float frac[U][3];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float iter = (float)(i0 + j);
                const float cx = R.start.x + iter * R.step.x;
                const float cy = R.start.y + iter * R.step.y;
                const float cz = R.start.z + iter * R.step.z;
                const float dx = cx * P.size[0], dy = cy * P.size[1], dz = cz * P.size[2];
                sl[j] = NL;
                laddr[j] = nullptr;
                svr_linear::LaneLod q = svr_linear::lane_lod_zero();
                const char* base = static_cast<const char*>(Ls[0].density);   // a valid address for the unused gathers
                bool done = i0 + j >= R.nsteps;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    size_t idx;
                    if (done || !lod_index(Ls[l], dx, dy, dz, idx)) continue;
                    done = true;
                    sl[j] = l;
                    svr_linear::lane_lod_take(q, Ls[l], dx * Ls[l].scale[0], dy * Ls[l].scale[1], dz * Ls[l].scale[2]);
                    base = static_cast<const char*>(Ls[l].density);
                    if (TINT && Ls[l].labels) laddr[j] = Ls[l].labels + idx;
                }
                const svr_linear::Cell cell = svr_linear::cell_of(q);
                size_t o[8];
                svr_linear::row_offsets(q, cell, o);
#pragma unroll
                for (int k = 0; k < 8; ++k) addr[j][k] = base + (o[k] << ESH);
#pragma unroll
                for (int a = 0; a < 3; ++a) frac[j][a] = cell.f[a];
            }
            float v8[U][8];
#pragma unroll
            for (int j = 0; j < U; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k) v8[j][k] = load_global<ESH>(addr[j][k]);
#pragma unroll
            for (int j = 0; j < U; ++j) vals[j] = svr_linear::blend(v8[j], frac[j]);
            }
            uint32_t labs[U];
            if (TINT) {
#pragma unroll
                for (int j = 0; j < U; ++j) labs[j] = laddr[j] ? *laddr[j] : 0u;
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                if (!alive || i0 + j >= R.nsteps) break;
                ++steps;
                if (sl[j] == NL) continue;                           // not resident: contributes nothing
                const float v = (vals[j] - inv_lo) / span;
                const float xf = fminf(fmaxf(v * kmax, 0.0f), kmax);
                const int e0 = min((int)xf, P.K - 2);
                const float f = xf - (float)e0;
                const float4 a = lut[e0], b = lut[e0 + 1];
                float er = a.x + f * (b.x - a.x);
                float eg = a.y + f * (b.y - a.y);
                float eb = a.z + f * (b.z - a.z);
                const float ea = a.w + f * (b.w - a.w);
                if (TINT) {
                    const float* hs = P.colors + 4u * (labs[j] % P.color_count);
                    const f3 q = hsv_to_rgb(hs[0], hs[1], 1.0f);
                    er = er * q.x; eg = eg * q.y; eb = eb * q.z;
                }
                const float w = (1.0f - ca) * ea;
                cr = cr + w * er;
                cg = cg + w * eg;
                cb = cb + w * eb;
                ca = ca + w;
                if (w > w_best) { w_best = w; best = i0 + j; if (TINT) best_label = labs[j]; }
                if (first < 0 && w > 0.0f) first = i0 + j;
                if (ca >= P.alpha_cutoff) alive = false;
            }
        }
    }

    float4 color = make_float4(0.f, 0.f, 0.f, 0.f);
    float depth = 0.0f;
    uint32_t label = 0u;
    uint8_t cls = frag ? SVR_PIX_MISS : SVR_PIX_DISCARD;
    unsigned long long pk = 0ull;
    if (ca > 0.0f) {
        cls = SVR_PIX_HIT;
        color = make_float4(cr / ca, cg / ca, cb / ca, ca * P.opacity);
        {   // depth at the first contributing sample (the march's shade_and_store formula)
            const float iter = (float)first;
            const float cx = R.start.x + iter * R.step.x, cy = R.start.y + iter * R.step.y, cz = R.start.z + iter * R.step.z;
            const f4 wp = mat_vec(P.world, cx - 0.5f, cy - 0.5f, cz - 0.5f, 1.0f);
            const f4 ndc = mat_vec(P.pc, wp.x, wp.y, wp.z, wp.w);
            depth = ndc.z / fmaxf(ndc.w, 0.001f);
        }
        const float iter = (float)best;
        const float cx = R.start.x + iter * R.step.x, cy = R.start.y + iter * R.step.y, cz = R.start.z + iter * R.step.z;
        if (TINT) {
            label = best_label;
        } else {   // one label fetch, at the best sample (the same LOD cascade its density came through)
            const float dx = cx * P.size[0], dy = cy * P.size[1], dz = cz * P.size[2];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                size_t idx;
                if (lod_index(P.L[l], dx, dy, dz, idx)) { label = P.L[l].labels ? P.L[l].labels[idx] : 0u; break; }
            }
        }
        pk = (unsigned long long)min(P.pick_id, 0xFFFFFu) | ((unsigned long long)pick_field(cx) << 20) |
             ((unsigned long long)pick_field(cy) << 34) | ((unsigned long long)pick_field(cz) << 48);
    }
    reinterpret_cast<float4*>(P.rgba)[o] = color;
    if (P.depth) P.depth[o] = depth;
    if (P.label) P.label[o] = label;
    if (P.flags) P.flags[o] = cls;
    if (P.steps) P.steps[o] = steps;
    if (P.pick) P.pick[o] = pk;
}

template <int NL, int ESH, bool LIN>
hipError_t launch_esh(const CompParams& P, bool tint, dim3 grid, size_t lds, hipStream_t stream) {
    if (tint) hipLaunchKernelGGL((composite_kernel<NL, ESH, true, LIN>), grid, dim3(256), lds, stream, P);
    else hipLaunchKernelGGL((composite_kernel<NL, ESH, false, LIN>), grid, dim3(256), lds, stream, P);
    return hipGetLastError();
}

template <int NL, bool LIN>
hipError_t launch_nl(const CompParams& P, int esh, bool tint, dim3 grid, size_t lds, hipStream_t stream) {
    if (esh == 0) return launch_esh<NL, 0, LIN>(P, tint, grid, lds, stream);
    if (esh == 1) return launch_esh<NL, 1, LIN>(P, tint, grid, lds, stream);
    return launch_esh<NL, 2, LIN>(P, tint, grid, lds, stream);
}

template <bool LIN>
hipError_t launch_composite(const CompParams& P, int num_lods, int esh, bool tint, dim3 grid, size_t lds, hipStream_t stream) {
    switch (num_lods) {
        case 1: return launch_nl<1, LIN>(P, esh, tint, grid, lds, stream);
        case 2: return launch_nl<2, LIN>(P, esh, tint, grid, lds, stream);
        case 3: return launch_nl<3, LIN>(P, esh, tint, grid, lds, stream);
        case 4: return launch_nl<4, LIN>(P, esh, tint, grid, lds, stream);
        case 5: return launch_nl<5, LIN>(P, esh, tint, grid, lds, stream);
        case 6: return launch_nl<6, LIN>(P, esh, tint, grid, lds, stream);
        case 7: return launch_nl<7, LIN>(P, esh, tint, grid, lds, stream);
        default: return launch_nl<8, LIN>(P, esh, tint, grid, lds, stream);
    }
}

// f32 matrix helpers in the contract's operation order (svr_api.hip's)
void mat_vec4(const float* m, const float* v, float* r) {
    for (int i = 0; i < 4; ++i) r[i] = ((m[0 + i] * v[0] + m[4 + i] * v[1]) + m[8 + i] * v[2]) + m[12 + i] * v[3];
}
void mat_mul4(const float* a, const float* b, float* out) {
    for (int c = 0; c < 4; ++c) mat_vec4(a, b + 4 * c, out + 4 * c);
}

}  // namespace

// Declared in svr_api.hip, which validates the arguments, orders the launch against the uploads and marks it as a
// render.  table: the device copy of the transfer function (K entries of RGBA).  interp: SVR_INTERP_*.
hipError_t svr_launch_composite(const svr_ctx* c, const svr_camera& cam, const svr_frame& fr,
                                const svr_composite_params& cp, const svr_outputs& out, const float* table, int K,
                                int interp, hipStream_t stream) {
    CompParams P;
    memset(&P, 0, sizeof(P));
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
    P.clim0 = m.clim[0]; P.clim1 = m.clim[1]; P.opacity = m.opacity;
    P.alpha_cutoff = cp.alpha_cutoff;
    P.clip_count = m.clipping_plane_count; P.clip_all = m.clipping_mode_all;
    for (uint32_t k = 0; k < m.clipping_plane_count; ++k)
        for (int a = 0; a < 4; ++a) P.clip[k][a] = c->clip_host[4 * k + a];
    P.color_count = m.color_count; P.colors = c->colors_dev;
    P.table = table; P.K = K;
    P.tiles_x = (fr.out_w + 15) / 16; P.tiles_y = (fr.out_h + 15) / 16;
    P.rgba = out.rgba; P.depth = out.depth; P.label = out.label; P.flags = out.flags; P.steps = out.steps;
    P.pick = reinterpret_cast<unsigned long long*>(out.pick); P.pick_id = out.pick_id;
    for (int l = 0; l < c->num_lods; ++l) {
        const LodStorage& S = c->lod[l];
        CompLod& Q = P.L[l];
        Q.density = S.density; Q.labels = S.labels;
        for (int a = 0; a < 3; ++a) {
            Q.off[a] = S.state.offset[a];
            Q.shape[a] = (uint32_t)S.state.shape[a];
            Q.ring[a] = (uint32_t)S.ring[a];
            Q.wrap0[a] = (uint32_t)(S.state.offset[a] % S.ring[a]);     // (svr_set_lod_state: offsets are >= 0)
            Q.scale[a] = S.state.scale[a];
        }
    }
    const int esh = c->density_storage == SVR_U8 ? 0 : (c->density_storage == SVR_U16 ? 1 : 2);
    const bool tint = cp.color_by_label != 0;
    const dim3 grid((unsigned)(P.tiles_x * P.tiles_y));
    const size_t lds = (size_t)K * 4 * sizeof(float);
    return interp == SVR_INTERP_LINEAR ? launch_composite<true>(P, c->num_lods, esh, tint, grid, lds, stream)
                                       : launch_composite<false>(P, c->num_lods, esh, tint, grid, lds, stream);
}
