// Cross-section views (svr_slice, include/svr.h): the march's sampling rule evaluated on a plane of pixels instead of
// along rays.  One lane = one pixel; one wave64 = a 16 x 4 pixel tile, four waves per workgroup stacked into 16 x 16,
// so that planes that are not x-normal still share L2 lines between neighbouring lanes.  No LDS.
//
// Arithmetic contract: strict IEEE f32 without contraction (-ffp-contract=off), operation order as written in svr.h.
// LOD test and the small helpers are ray_common.h's; tests/test_gpu_slice.py holds this kernel and the march to the same
// numpy restatement.
#include "svr_host.h"
#include "ray_common.h"
#include "linear_sample.h"

namespace {

using namespace svr_common;

struct SliceLod {
    const void*     density;   // ring [z][y][x], element type per SliceParams::esh
    const uint32_t* labels;    // null: no label rings
    const void*     twin;      // micro-block copy to read from (svr_lod_desc::blocked_twin), or null: read the rows
    int32_t  off[3];           // current_logical_offset_in_pixels
    uint32_t shape[3];         // current_logical_shape_in_pixels
    uint32_t wrap0[3];         // ring slot of the ROI's first voxel
    uint32_t ring[3];
    float    scale[3];
};

struct SliceParams {
    float world_inv[16];
    float size[3];
    float origin[3], u[3], v[3];
    svr_frame frame;
    float clim0, clim1, gamma, opacity;
    int32_t colorspace_srgb;
    uint32_t color_count;
    const float* colors;       // device, color_count x vec4 (h, s, v, pad)
    int32_t esh;               // log2 of the density element size: 0 u8, 1 u16, 2 f32
    float*    rgba;
    float*    depth;
    uint32_t* label;
    uint8_t*  flags;
    float*    value;
    uint8_t*  lod;
    SliceLod L[SVR_MAX_LODS];
};

// march_kernel.hip `srgb2physical` (pygfx std.wgsl, restated)
__device__ __forceinline__ float srgb2physical(float c) {
    const float f = powf((c + 0.055f) / 1.055f, 2.4f);
    const float t = c / 12.92f;
    return (c <= 0.04045f) ? t : f;
}

template <int ESH>
__device__ __forceinline__ float load_texel(const void* base, size_t i) {
    if (ESH == 0) return (float)static_cast<const uint8_t*>(base)[i];
    if (ESH == 1) return (float)static_cast<const uint16_t*>(base)[i];
    return static_cast<const float*>(base)[i];
}

// LIN: the linear sample of svr.h (svr_set_interpolation) in place of the nearest texel; label and lod stay the
// nearest sample's.  The eight gathers of a pixel are issued together, then blended.
template <int NL, int ESH, bool LIN>
__global__ __launch_bounds__(256) void slice_kernel(const SliceParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 16 + (lane & 15);
    const int r = blockIdx.y * 16 + wave * 4 + (lane >> 4);
    if (c >= P.frame.out_w || r >= P.frame.out_h) return;
    const size_t o = (size_t)r * (size_t)P.frame.out_w + (size_t)c;
    const int x = P.frame.x0 + c;
    const int y = P.frame.y0 + (r / P.frame.band_h) * P.frame.band_pitch + (r % P.frame.band_h);

    float4 color = make_float4(0.f, 0.f, 0.f, 0.f);
    float value = 0.0f;
    uint32_t label = 0u;
    uint8_t cls = SVR_PIX_DISCARD, lod = 255;
    if (x < P.frame.frame_w && y < P.frame.frame_h) {
        const float fx = ((float)x + 0.5f) - 0.5f * (float)P.frame.frame_w;
        const float fy = ((float)y + 0.5f) - 0.5f * (float)P.frame.frame_h;
        const float px = (P.origin[0] + fx * P.u[0]) + fy * P.v[0];
        const float py = (P.origin[1] + fx * P.u[1]) + fy * P.v[1];
        const float pz = (P.origin[2] + fx * P.u[2]) + fy * P.v[2];
        const float* m = P.world_inv;
        const float qx = ((m[0] * px + m[4] * py) + m[8] * pz) + m[12] * 1.0f;
        const float qy = ((m[1] * px + m[5] * py) + m[9] * pz) + m[13] * 1.0f;
        const float qz = ((m[2] * px + m[6] * py) + m[10] * pz) + m[14] * 1.0f;
        const float dx = ((qx + 0.5f) / P.size[0]) * P.size[0];
        const float dy = ((qy + 0.5f) / P.size[1]) * P.size[1];
        const float dz = ((qz + 0.5f) / P.size[2]) * P.size[2];
        if (dx >= 0.0f && dx < P.size[0] && dy >= 0.0f && dy < P.size[1] && dz >= 0.0f && dz < P.size[2]) {
            cls = SVR_PIX_MISS;
            color.w = 1.0f;
            if constexpr (!LIN) {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                uint32_t wx, wy, wz;
                if (!lod_slot(P.L[l], dx, dy, dz, wx, wy, wz)) continue;
                const SliceLod& L = P.L[l];
                const size_t idx = ((size_t)wz * L.ring[1] + wy) * (size_t)L.ring[0] + wx;
                value = L.twin ? load_texel<ESH>(L.twin, svr_blocked_index(ESH, L.ring[0], L.ring[1], wx, wy, wz))
                               : load_texel<ESH>(L.density, idx);
                label = L.labels ? L.labels[idx] : 0u;
                lod = (uint8_t)l;
                cls = SVR_PIX_HIT;
                break;
            }
            } else {
                svr_linear::LaneLod q = svr_linear::lane_lod_zero();
                const char* base = nullptr;
                const uint32_t* labels = nullptr;
                size_t lidx = 0;
                bool blocked = false;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    uint32_t wx, wy, wz;
                    if (cls == SVR_PIX_HIT || !lod_slot(P.L[l], dx, dy, dz, wx, wy, wz)) continue;
                    const SliceLod& L = P.L[l];
                    svr_linear::lane_lod_take(q, L, dx * L.scale[0], dy * L.scale[1], dz * L.scale[2]);
                    blocked = L.twin != nullptr;
                    base = static_cast<const char*>(blocked ? L.twin : L.density);
                    labels = L.labels;
                    lidx = ((size_t)wz * L.ring[1] + wy) * (size_t)L.ring[0] + wx;
                    lod = (uint8_t)l;
                    cls = SVR_PIX_HIT;
                }
                if (cls == SVR_PIX_HIT) {
                    const svr_linear::Cell cell = svr_linear::cell_of(q);
                    size_t o[8];
                    if (blocked) svr_linear::blocked_offsets(ESH, q, cell, o);
                    else svr_linear::row_offsets(q, cell, o);
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = load_global<ESH>(base + (o[k] << ESH));
                    value = svr_linear::blend(v, cell.f);
                    label = labels ? labels[lidx] : 0u;
                }
            }
            if (cls == SVR_PIX_HIT) {
                float s = (value - P.clim0) / (P.clim1 - P.clim0);
                if (P.gamma != 1.0f) s = powf(s, P.gamma);
                const float phys = P.colorspace_srgb ? srgb2physical(s) : s;
                const float* hs = P.colors + 4u * (label % P.color_count);
                const f3 rgb = hsv_to_rgb(hs[0], hs[1], phys);
                color = make_float4(rgb.x, rgb.y, rgb.z, P.opacity);
            }
        }
    }
    reinterpret_cast<float4*>(P.rgba)[o] = color;
    if (P.depth) P.depth[o] = 0.0f;
    if (P.label) P.label[o] = label;
    if (P.flags) P.flags[o] = cls;
    if (P.value) P.value[o] = value;
    if (P.lod) P.lod[o] = lod;
}

// ---- thick slabs (svr_slab, include/svr.h): N samples per pixel along the data-space step dw, reduced to one.
// One kernel for the three modes: MIN is MAX on keys whose sign bit is flipped (an exact bit flip, so ties and NaN
// follow the same strict '>' and the value comes back bit for bit), and the f32 sum MEAN needs is one add per sample
// that MAX and MIN carry unused.  That costs two VALU per sample against three times the code.
struct SlabParams {
    SliceParams S;
    float dw[3];               // data-space step from one sample to the next (svr_slab computes and checks it)
    float half;                // 0.5f * (float)(N - 1): t_k = (float)k - half
    float w_len;
    int32_t samples;
    uint32_t smask;            // 0x80000000 for MIN, else 0
    int32_t mean;
};

using SlabArgs = const SlabParams __attribute__((address_space(4)));     // the kernel arguments' own address space

constexpr int SLAB_UNROLL = 4;     // samples whose gathers are in flight together per lane

// POW2: every size_k is a power of two <= 2^24.  Then ((x / size) * size) == x for every x = q_k + 0.5f: a nonzero
// x is at least 2^-25 in magnitude (q_k + 0.5f is exact by Sterbenz's lemma where it is small), so x / size stays
// normal and both steps are exact scalings; 0, inf and NaN pass through unchanged.  The round trip, three IEEE
// divisions per sample, is skipped.
// LIN: every sample's value_k is the linear sample of svr.h; it runs the general coordinate chain (POW2 = false: results
// are defined by that chain, and the cell needs its s bits).
template <int NL, int ESH, bool POW2, bool LIN>
__global__ __launch_bounds__(256) void slab_kernel(const SlabParams Q) {
    const SliceParams& P = Q.S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 16 + (lane & 15);
    const int r = blockIdx.y * 16 + wave * 4 + (lane >> 4);
    if (c >= P.frame.out_w || r >= P.frame.out_h) return;
    const size_t o = (size_t)r * (size_t)P.frame.out_w + (size_t)c;
    const int x = P.frame.x0 + c;
    const int y = P.frame.y0 + (r / P.frame.band_h) * P.frame.band_pitch + (r % P.frame.band_h);

    float4 color = make_float4(0.f, 0.f, 0.f, 0.f);
    float value = 0.0f, depth = 0.0f;
    uint32_t label = 0u;
    uint8_t cls = SVR_PIX_DISCARD, lod = 255;
    if (x < P.frame.frame_w && y < P.frame.frame_h) {
        const float fx = ((float)x + 0.5f) - 0.5f * (float)P.frame.frame_w;
        const float fy = ((float)y + 0.5f) - 0.5f * (float)P.frame.frame_h;
        const float px = (P.origin[0] + fx * P.u[0]) + fy * P.v[0];
        const float py = (P.origin[1] + fx * P.u[1]) + fy * P.v[1];
        const float pz = (P.origin[2] + fx * P.u[2]) + fy * P.v[2];
        const float* m = P.world_inv;
        const float qx = ((m[0] * px + m[4] * py) + m[8] * pz) + m[12] * 1.0f;
        const float qy = ((m[1] * px + m[5] * py) + m[9] * pz) + m[13] * 1.0f;
        const float qz = ((m[2] * px + m[6] * py) + m[10] * pz) + m[14] * 1.0f;

        bool inside = false;
        int hits = 0, best_k = 0, best_l = 0;
        float sum = 0.0f, best = 0.0f;
        size_t best_idx = 0;
        const SlabArgs* kq = (const SlabArgs*)__builtin_amdgcn_kernarg_segment_ptr();     // Q itself: the only argument
        for (int k0 = 0; k0 < Q.samples; k0 += SLAB_UNROLL) {
            // The LOD table is read from the kernel arguments afresh in each iteration (scalar loads from the constant
            // cache): held in SGPRs across the loop, its 21 dwords per LOD spill SGPRs from NL = 3 on.
            asm volatile("" : "+s"(kq));
            const SliceLod* Ls = (const SliceLod*)kq->S.L;
            // addresses of SLAB_UNROLL samples first, then their gathers, then the compares in increasing k
            size_t ridx[SLAB_UNROLL];
            int sl[SLAB_UNROLL];
            bool in[SLAB_UNROLL];
            float vals[SLAB_UNROLL];
            if constexpr (!LIN) {
            const char* addr[SLAB_UNROLL];
#pragma unroll
            for (int j = 0; j < SLAB_UNROLL; ++j) {
                const float t = (float)(k0 + j) - Q.half;
                const float ax = qx + t * Q.dw[0], ay = qy + t * Q.dw[1], az = qz + t * Q.dw[2];
                const float dx = POW2 ? ax + 0.5f : ((ax + 0.5f) / P.size[0]) * P.size[0];
                const float dy = POW2 ? ay + 0.5f : ((ay + 0.5f) / P.size[1]) * P.size[1];
                const float dz = POW2 ? az + 0.5f : ((az + 0.5f) / P.size[2]) * P.size[2];
                in[j] = k0 + j < Q.samples && dx >= 0.0f && dx < P.size[0] && dy >= 0.0f && dy < P.size[1] &&
                        dz >= 0.0f && dz < P.size[2];
                sl[j] = NL;                                        // no LOD holds it
                addr[j] = static_cast<const char*>(Ls[0].density);    // a valid address for the unused gather
                ridx[j] = 0;
                bool done = !in[j];
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    uint32_t wx, wy, wz;
                    if (done || !lod_slot(Ls[l], dx, dy, dz, wx, wy, wz)) continue;
                    const SliceLod& L = Ls[l];
                    done = true;
                    sl[j] = l;
                    ridx[j] = ((size_t)wz * L.ring[1] + wy) * (size_t)L.ring[0] + wx;
                    addr[j] = L.twin ? static_cast<const char*>(L.twin) + (svr_blocked_index(ESH, L.ring[0], L.ring[1], wx, wy, wz) << ESH)
                                     : static_cast<const char*>(L.density) + (ridx[j] << ESH);
                }
            }
#pragma unroll
            for (int j = 0; j < SLAB_UNROLL; ++j) vals[j] = load_global<ESH>(addr[j]);
            } else {
            const char* addr[SLAB_UNROLL][8];
            float frac[SLAB_UNROLL][3];
#pragma unroll
            for (int j = 0; j < SLAB_UNROLL; ++j) {
                const float t = (float)(k0 + j) - Q.half;
                const float ax = qx + t * Q.dw[0], ay = qy + t * Q.dw[1], az = qz + t * Q.dw[2];
                const float dx = ((ax + 0.5f) / P.size[0]) * P.size[0];
                const float dy = ((ay + 0.5f) / P.size[1]) * P.size[1];
                const float dz = ((az + 0.5f) / P.size[2]) * P.size[2];
                in[j] = k0 + j < Q.samples && dx >= 0.0f && dx < P.size[0] && dy >= 0.0f && dy < P.size[1] &&
                        dz >= 0.0f && dz < P.size[2];
                sl[j] = NL;                                        // no LOD holds it
                ridx[j] = 0;
                svr_linear::LaneLod q = svr_linear::lane_lod_zero();
                const char* base = static_cast<const char*>(Ls[0].density);   // a valid address for the unused gathers
                bool blocked = false;
                bool done = !in[j];
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    uint32_t wx, wy, wz;
                    if (done || !lod_slot(Ls[l], dx, dy, dz, wx, wy, wz)) continue;
                    const SliceLod& L = Ls[l];
                    done = true;
                    sl[j] = l;
                    ridx[j] = ((size_t)wz * L.ring[1] + wy) * (size_t)L.ring[0] + wx;
                    svr_linear::lane_lod_take(q, L, dx * L.scale[0], dy * L.scale[1], dz * L.scale[2]);
                    blocked = L.twin != nullptr;
                    base = static_cast<const char*>(blocked ? L.twin : L.density);
                }
                const svr_linear::Cell cell = svr_linear::cell_of(q);
                size_t o[8];
                if (blocked) svr_linear::blocked_offsets(ESH, q, cell, o);
                else svr_linear::row_offsets(q, cell, o);
#pragma unroll
                for (int k = 0; k < 8; ++k) addr[j][k] = base + (o[k] << ESH);
#pragma unroll
                for (int a = 0; a < 3; ++a) frac[j][a] = cell.f[a];
            }
            float v8[SLAB_UNROLL][8];
#pragma unroll
            for (int j = 0; j < SLAB_UNROLL; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k) v8[j][k] = load_global<ESH>(addr[j][k]);
#pragma unroll
            for (int j = 0; j < SLAB_UNROLL; ++j) vals[j] = svr_linear::blend(v8[j], frac[j]);
            }
#pragma unroll
            for (int j = 0; j < SLAB_UNROLL; ++j) {
                inside |= in[j];
                if (sl[j] == NL) continue;
                const float key = __uint_as_float(__float_as_uint(vals[j]) ^ Q.smask);
                if (hits == 0 || key > best) { best = key; best_k = k0 + j; best_l = sl[j]; best_idx = ridx[j]; }
                sum += vals[j];
                ++hits;
            }
        }
        if (hits > 0) {
            cls = SVR_PIX_HIT;
            value = Q.mean ? sum / (float)hits : __uint_as_float(__float_as_uint(best) ^ Q.smask);
            lod = (uint8_t)best_l;
#pragma unroll
            for (int l = 0; l < NL; ++l)
                if (best_l == l && P.L[l].labels) label = P.L[l].labels[best_idx];
            depth = ((float)best_k - Q.half) * Q.w_len;
            float s = (value - P.clim0) / (P.clim1 - P.clim0);
            if (P.gamma != 1.0f) s = powf(s, P.gamma);
            const float phys = P.colorspace_srgb ? srgb2physical(s) : s;
            const float* hs = P.colors + 4u * (label % P.color_count);
            const f3 rgb = hsv_to_rgb(hs[0], hs[1], phys);
            color = make_float4(rgb.x, rgb.y, rgb.z, P.opacity);
        } else if (inside) {
            cls = SVR_PIX_MISS;
            color.w = 1.0f;
        }
    }
    reinterpret_cast<float4*>(P.rgba)[o] = color;
    if (P.depth) P.depth[o] = depth;
    if (P.label) P.label[o] = label;
    if (P.flags) P.flags[o] = cls;
    if (P.value) P.value[o] = value;
    if (P.lod) P.lod[o] = lod;
}

// 128-byte lines a 16 x 4 wave tile touches, estimated from the bounding box of its footprint in ring voxels (extent
// e per axis) for a layout of b-voxel lines: prod(e_k / b_k + 1), at most one per lane (cap 64; a slab's N gathers: 64 N)
float lines_per_tile(const float e[3], float bx, float by, float bz, float cap = 64.0f) {
    return fminf(cap, (e[0] / bx + 1.0f) * (e[1] / by + 1.0f) * (e[2] / bz + 1.0f));
}

}  // namespace

namespace {

// The kernel arguments svr_slice and svr_slab share (everything but the micro-block copy routing), and the data-space
// voxel steps per column (du) and per row (dv): the linear part of world_inv applied to u and v.
void fill_slice_params(const svr_ctx* c, const svr_slice_plane& pl, const svr_frame& fr, const svr_slice_outputs& out,
                       SliceParams& P, float du[3], float dv[3]) {
    memset(&P, 0, sizeof(P));
    memcpy(P.world_inv, pl.world_inv, sizeof(P.world_inv));
    for (int a = 0; a < 3; ++a) {
        P.size[a] = pl.volume_dimensions[a];
        P.origin[a] = pl.origin[a]; P.u[a] = pl.u[a]; P.v[a] = pl.v[a];
    }
    P.frame = fr;
    const svr_material& m = c->material;
    P.clim0 = m.clim[0]; P.clim1 = m.clim[1]; P.gamma = m.gamma; P.opacity = m.opacity;
    P.colorspace_srgb = m.colorspace_srgb;
    P.color_count = m.color_count; P.colors = c->colors_dev;
    P.esh = esh_of(c);
    P.rgba = out.rgba; P.depth = out.depth; P.label = out.label; P.flags = out.flags; P.value = out.value; P.lod = out.lod;
    for (int k = 0; k < 3; ++k) {
        du[k] = (pl.world_inv[k] * pl.u[0] + pl.world_inv[4 + k] * pl.u[1]) + pl.world_inv[8 + k] * pl.u[2];
        dv[k] = (pl.world_inv[k] * pl.v[0] + pl.world_inv[4 + k] * pl.v[1]) + pl.world_inv[8 + k] * pl.v[2];
    }
    for (int l = 0; l < c->num_lods; ++l) fill_lod_common(c->lod[l], P.L[l]);     // (twin stays null: the launchers route)
}

// 128-byte lines of the micro-block copy / of the rows that a footprint of extent e (ring voxels) touches
float block_lines(int esh, const float e[3], float cap = 64.0f) {
    return esh == 0 ? lines_per_tile(e, 8.0f, 4.0f, 4.0f, cap)
         : esh == 1 ? lines_per_tile(e, 4.0f, 4.0f, 4.0f, cap) : lines_per_tile(e, 4.0f, 4.0f, 2.0f, cap);
}
float row_lines(int esh, const float e[3], float cap = 64.0f) {
    return lines_per_tile(e, 128.0f / (float)(1 << esh), 1.0f, 1.0f, cap);
}

}  // namespace

// svr_slice has validated the arguments; it orders the launch against the uploads and marks it as a
// render.  twin_mode: 0 rows only, 2 the micro-block copy wherever there is one, 1 per LOD the fewer lines (the
// estimate is the nearest sample's under either interpolation: a cell adds one voxel per axis to the footprint).
// interp: SVR_INTERP_*.
hipError_t svr_launch_slice(const svr_ctx* c, const svr_slice_plane& pl, const svr_frame& fr, const svr_slice_outputs& out,
                            int twin_mode, int interp, hipStream_t stream) {
    SliceParams P;
    float du[3], dv[3];
    fill_slice_params(c, pl, fr, out, P, du, dv);
    for (int l = 0; l < c->num_lods; ++l) {
        const LodStorage& S = c->lod[l];
        SliceLod& Q = P.L[l];
        if (S.twin && twin_mode == 2) Q.twin = S.twin;
        if (S.twin && twin_mode == 1) {
            float e[3];
            for (int k = 0; k < 3; ++k) e[k] = (15.0f * fabsf(du[k]) + 3.0f * fabsf(dv[k])) * Q.scale[k];
            if (block_lines(P.esh, e) < row_lines(P.esh, e)) Q.twin = S.twin;
        }
    }
    const dim3 grid((unsigned)((fr.out_w + 15) / 16), (unsigned)((fr.out_h + 15) / 16));
    return with_bool(interp == SVR_INTERP_LINEAR, [&](auto lin) {
        return with_lods_esh(c->num_lods, P.esh, [&](auto nl, auto esh) {
            return launch_tiles(slice_kernel<nl(), esh(), lin()>, grid, 0, stream, P);
        });
    });
}

// Like svr_launch_slice; svr_slab has validated the arguments and computed dw.
// Micro-block copy routing per LOD over the whole slab (twin_mode 1).  A wave's N gathers of 64 lanes cost, per layout,
//   the lines each gather walks (the slice's estimate of the tile on one plane: a gather touching 64 lines takes the
//   texture unit 64 passes even when they are cached), summed over the N samples, plus
//   the distinct lines of the bounding box of the 16 x 4 tile x N samples (what has to reach the CU at least once).
// The copy is read where that total is lower.
hipError_t svr_launch_slab(const svr_ctx* c, const svr_slab_params& sp, const float dw[3], const svr_frame& fr,
                           const svr_slice_outputs& out, int twin_mode, int interp, hipStream_t stream) {
    SlabParams Q;
    memset(&Q, 0, sizeof(Q));
    float du[3], dv[3];
    fill_slice_params(c, sp.plane, fr, out, Q.S, du, dv);
    const int N = sp.samples;
    for (int k = 0; k < 3; ++k) Q.dw[k] = dw[k];
    Q.half = 0.5f * (float)(N - 1);
    Q.w_len = sp.w_len;
    Q.samples = N;
    Q.smask = sp.mode == SVR_SLAB_MIN ? 0x80000000u : 0u;
    Q.mean = sp.mode == SVR_SLAB_MEAN;
    for (int l = 0; l < c->num_lods; ++l) {
        const LodStorage& S = c->lod[l];
        SliceLod& L = Q.S.L[l];
        if (S.twin && twin_mode == 2) L.twin = S.twin;
        if (S.twin && twin_mode == 1) {
            float plane[3], slab[3];
            for (int k = 0; k < 3; ++k) {
                plane[k] = (15.0f * fabsf(du[k]) + 3.0f * fabsf(dv[k])) * L.scale[k];
                slab[k] = plane[k] + (float)(N - 1) * fabsf(dw[k]) * L.scale[k];
            }
            const float lanes = 64.0f * (float)N;
            const float rows = (float)N * row_lines(Q.S.esh, plane) + row_lines(Q.S.esh, slab, lanes);
            const float blocks = (float)N * block_lines(Q.S.esh, plane) + block_lines(Q.S.esh, slab, lanes);
            if (blocks < rows) L.twin = S.twin;
        }
    }
    // sizes that are powers of two up to 2^24 let the kernel skip the (x / size) * size round trip (exact there)
    bool pow2 = true;
    for (int a = 0; a < 3; ++a) {
        int e2;
        const float mant = frexpf(Q.S.size[a], &e2);
        pow2 = pow2 && mant == 0.5f && e2 <= 25;
    }
    const dim3 grid((unsigned)((fr.out_w + 15) / 16), (unsigned)((fr.out_h + 15) / 16));
    if (interp == SVR_INTERP_LINEAR)                                                          // the general chain
        return with_lods_esh(c->num_lods, Q.S.esh, [&](auto nl, auto esh) {
            return launch_tiles(slab_kernel<nl(), esh(), false, true>, grid, 0, stream, Q);
        });
    return with_bool(pow2, [&](auto p2) {
        return with_lods_esh(c->num_lods, Q.S.esh, [&](auto nl, auto esh) {
            return launch_tiles(slab_kernel<nl(), esh(), p2(), false>, grid, 0, stream, Q);
        });
    });
}
