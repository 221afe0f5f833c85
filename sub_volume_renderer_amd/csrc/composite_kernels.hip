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
// Ray set-up, LOD test and the small helpers are ray_common.h's; tests/test_gpu_composite.py holds this kernel to
// tests/composite_twin.py.
#include "svr_host.h"
#include "ray_common.h"
#include "linear_sample.h"

namespace {

using namespace svr_common;

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
    CutParams cut;             // after L[]: every argument above keeps the offset it had before cuts existed
};

using CompArgs = const CompParams __attribute__((address_space(4)));     // the kernel arguments' own address space

constexpr int COMP_UNROLL = 8;     // samples whose gathers are in flight together per lane
constexpr int COMP_LIN_UNROLL = 4; // the same under linear sampling: 4 samples x 8 corners = 32 gathers in flight

// LIN: s of every sample is the linear sample of svr.h (svr_set_interpolation); labels stay the nearest sample's.
// CUT: the samples svr_set_cut_planes cuts away are treated like samples no LOD holds.  The ray's kept (ANY) or cut
// (ALL) index interval is found once (cut_span); the loop starts at the batch of the first kept sample and, under ANY,
// ends after the last one, and a sample is masked by cut_sample.  Without CUT nothing of this is compiled.
template <int NL, int ESH, bool TINT, bool LIN, bool CUT>
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
        int i_begin = 0, i_end = R.nsteps;
        CutSpan cspan = { 0, 0 };
        bool cut_all = false;
        if constexpr (CUT) {
            const CutParams* cq = (const CutParams*)&kq->cut;       // wave-uniform: scalar loads, like the LOD table
            cut_all = cq->all != 0;
            cspan = cut_span(*cq, cut_ray(R, P.size), R.nsteps);
            // the first kept sample (nsteps: none) and one past the last
            const int kept0 = cut_all ? (cspan.lo > 0 ? 0 : cspan.hi) : (cspan.lo < cspan.hi ? cspan.lo : R.nsteps);
            i_begin = min((kept0 / U) * U, R.nsteps);
            if (!cut_all) i_end = cspan.lo < cspan.hi ? cspan.hi : 0;
            steps = (uint32_t)i_begin;                               // cut samples are counted
        }
        for (int i0 = i_begin; alive && i0 < i_end; i0 += U) {
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
                if constexpr (CUT) done = done || cut_sample(cspan, cut_all, i0 + j);
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
                if constexpr (CUT) done = done || cut_sample(cspan, cut_all, i0 + j);
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
        if constexpr (CUT) { if (alive) steps = (uint32_t)R.nsteps; }    // the cut samples after the last kept one
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

}  // namespace

// svr_composite has validated the arguments; it orders the launch against the uploads and marks it as a
// render.  table: the device copy of the transfer function (K entries of RGBA).  interp: SVR_INTERP_*.  cut_planes:
// cut_count x abcd of svr_set_cut_planes (host), cut_mode: SVR_CUT_*; any plane selects the CUT instantiations, which
// doubles the kernels of this file (8 LOD counts x 3 element sizes x TINT x LIN x CUT = 192).
hipError_t svr_launch_composite(const svr_ctx* c, const svr_camera& cam, const svr_frame& fr,
                                const svr_composite_params& cp, const svr_outputs& out, const float* table, int K,
                                int interp, const float* cut_planes, uint32_t cut_count, int cut_mode,
                                hipStream_t stream) {
    CompParams P;
    memset(&P, 0, sizeof(P));
    CutPlanes cut;
    cut.count = cut_count; cut.mode = cut_mode;
    if (cut_count) memcpy(cut.abcd, cut_planes, sizeof(float) * 4 * cut_count);
    fill_ray_params(c, cam, fr, out, cut, P);
    const svr_material& m = c->material;
    P.clim0 = m.clim[0]; P.clim1 = m.clim[1];
    P.alpha_cutoff = cp.alpha_cutoff;
    P.table = table; P.K = K;
    for (int l = 0; l < c->num_lods; ++l) fill_lod_common(c->lod[l], P.L[l]);
    const dim3 grid((unsigned)(P.tiles_x * P.tiles_y));
    const size_t lds = (size_t)K * 4 * sizeof(float);
    return with_bool(cut_count != 0, [&](auto cutv) {
        return with_bool(interp == SVR_INTERP_LINEAR, [&](auto lin) {
            return with_bool(cp.color_by_label != 0, [&](auto tint) {
                return with_lods_esh(c->num_lods, esh_of(c), [&](auto nl, auto esh) {
                    return launch_tiles(composite_kernel<nl(), esh(), tint(), lin(), cutv()>, grid, lds, stream, P);
                });
            });
        });
    });
}
