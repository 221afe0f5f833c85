// The draw of the C ABI (include/svr.h): svr_render and svr_time_render.  The block -> tile tables (tile_order.h) cached
// per context, how the rings are cut into buffer resources (ring_parts.h), and fill_params, which turns the context, the
// camera and the frame into the march's MarchParams.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "svr_host.h"
#include "ray_common.h"
#include "ring_parts.h"
#include "march_pow2.h"
#include "twin_address.h"
#include "slab_box.h"
#include "tile_order.h"

using svr_common::mat_mul4;
using svr_common::mat_vec4;

static int floor_div(int a, int b) { int q = a / b, r = a % b; return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q; }

// ---- block -> tile tables ---------------------------------------------------
static int tile_order_for(svr_ctx* c, int tx, int ty, int tile_w, int tile_h, int mode, const uint32_t** out) {
    *out = nullptr;
    if (mode == 1 || tx * ty <= 0) return SVR_OK;             // in-kernel contiguous mapping
    const int cw = std::max(1, kChunk[mode][0] / tile_w), ch = std::max(1, kChunk[mode][1] / tile_h);
    const int key = mode | cw << 8 | ch << 16;
    for (const auto& t : c->tile_orders)
        if (t.tiles_x == tx && t.tiles_y == ty && t.mode == key) { *out = t.dev; return SVR_OK; }
    std::vector<uint32_t> order;
    build_tile_order(tx, ty, cw, ch, order);
    DeviceGuard guard(c->device);
    uint32_t* dev = nullptr;
    SVR_HIP_TRY(hipMalloc((void**)&dev, order.size() * sizeof(uint32_t)));
    SVR_HIP_TRY(hipMemcpy(dev, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (c->tile_orders.size() >= 64) {                        // bounded cache: drop the oldest table once idle
        (void)hipDeviceSynchronize();
        (void)hipFree(c->tile_orders.front().dev);
        c->tile_orders.erase(c->tile_orders.begin());
    }
    c->tile_orders.push_back({ tx, ty, key, dev });
    *out = dev;
    return SVR_OK;
}

// The cost-sorted table of this draw: kept per stream, recomputed only when the camera / frame region changed.
// The new table is written into the stream's pinned buffer and copied on that same stream, i.e. behind the
// previous draw of that stream (which may still read the old table) and before this one.
static int tile_order_by_cost_for(svr_ctx* c, const MarchParams& P, int tile_w, int tile_h, hipStream_t stream,
                                  const uint32_t** out) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
    mix(P.ndc_to_data, sizeof(P.ndc_to_data)); mix(P.size, sizeof(P.size)); mix(&P.frame, sizeof(P.frame));
    mix(&tile_w, sizeof(tile_w)); mix(&tile_h, sizeof(tile_h)); mix(&P.tiles_x, sizeof(P.tiles_x)); mix(&P.tiles_y, sizeof(P.tiles_y));
    svr_ctx::CostOrder* slot = nullptr;
    for (auto& t : c->cost_orders) if (t.stream == stream) { slot = &t; break; }
    DeviceGuard guard(c->device);
    if (!slot) {
        if (c->cost_orders.size() >= 64) {                   // a caller cycling through many streams: recycle the oldest slot
            // (wait for the last draw that read the old table, through the slot's own event: the stream it ran on may
            // be gone by now)
            svr_ctx::CostOrder old = c->cost_orders.front();
            if (old.drawn_set) SVR_HIP_TRY(hipEventSynchronize(old.drawn));
            else if (old.valid) SVR_HIP_TRY(hipEventSynchronize(old.copied));
            c->cost_orders.erase(c->cost_orders.begin());
            old.stream = stream; old.valid = false; old.drawn_set = false;
            c->cost_orders.push_back(old);
        } else {
            svr_ctx::CostOrder t{ stream, nullptr, nullptr, 0, nullptr, 0, false, nullptr, false };
            SVR_HIP_TRY(hipEventCreateWithFlags(&t.copied, hipEventDisableTiming));
            SVR_HIP_TRY(hipEventCreateWithFlags(&t.drawn, hipEventDisableTiming));
            c->cost_orders.push_back(t);
        }
        slot = &c->cost_orders.back();
    }
    const size_t n = (size_t)P.tiles_x * (size_t)P.tiles_y;
    if (slot->valid && slot->key == h && slot->cap >= n) { *out = slot->dev; return SVR_OK; }
    if (slot->cap < n) {
        if (slot->dev) { SVR_HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(slot->dev); (void)hipHostFree(slot->host); slot->dev = slot->host = nullptr; slot->cap = 0; }
        const size_t cap = n + n / 4 + 64;
        if (hipMalloc((void**)&slot->dev, cap * sizeof(uint32_t)) != hipSuccess ||
            hipHostMalloc((void**)&slot->host, cap * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
            svr_set_error("svr_render: out of memory for the block -> tile table"); return SVR_ERR_NOMEM;
        }
        slot->cap = cap;
    } else if (slot->valid) {
        SVR_HIP_TRY(hipEventSynchronize(slot->copied));      // the pinned buffer's previous contents have left for the device
    }
    const svr_frame& F = P.frame;
    const TileCostView view{ P.ndc_to_data, P.size, F.frame_w, F.frame_h, F.x0, F.y0, F.out_w, F.out_h, F.band_h, F.band_pitch };
    std::vector<uint32_t> order;
    build_tile_order_by_cost(view, P.tiles_x, P.tiles_y, tile_w, tile_h, std::max(1, 64 / tile_w), std::max(1, 64 / tile_h), order);
    memcpy(slot->host, order.data(), n * sizeof(uint32_t));
    SVR_HIP_TRY(hipMemcpyAsync(slot->dev, slot->host, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    SVR_HIP_TRY(hipEventRecord(slot->copied, stream));
    slot->key = h; slot->valid = true;
    *out = slot->dev;
    return SVR_OK;
}

// Behind a draw that may have read a cost-sorted table: mark the stream's slot (see CostOrder::drawn).
static int cost_order_drawn(svr_ctx* c, const MarchParams& P, hipStream_t stream) {
    for (auto& t : c->cost_orders)
        if (t.stream == stream && t.dev == P.tile_order) {
            SVR_HIP_TRY(hipEventRecord(t.drawn, stream));
            t.drawn_set = true;
            break;
        }
    return SVR_OK;
}

// ---- how the rings are addressed --------------------------------------------
// The experiments-only part size of SVR_FORCE_ZSPLIT (see rings_need_big); 0 in production builds.
static int forced_zsplit() {
    static const int force_zsplit = svr_exp_env_int("SVR_FORCE_ZSPLIT", 0);
    return force_zsplit;
}

// How LOD l's density ring is cut into buffer resources (ring_parts.h decides; nothing else re-derives the split).
static RingParts lod_ring_parts(const svr_ctx* c, int l) {
    const LodStorage& L = c->lod[l];
    return ring_parts((uint32_t)L.ring[0], (uint32_t)L.ring[1], (uint32_t)L.ring[2], (uint32_t)svr_dtype_size(c->density_storage),
                      L.twin != nullptr, forced_zsplit());
}

// Can the span kernel address this context's rings?  Every LOD's ring must be reached through at most 8 resources of
// whole z planes, each below 4 GiB (32-bit byte offsets), and stay within the 24-bit row index and row pitch of the
// exact general path; otherwise every render takes the straightforward kernel's 64-bit addressing.
static bool span_addressable(const svr_ctx* c) {
    for (int l = 0; l < c->num_lods; ++l)
        if (!lod_ring_parts(c, l).span_ok) return false;
    return true;
}

// Rings of 4 GiB or more in total take the BIG build of the march (one buffer resource per LOD, several for a ring of
// 4 GiB or more).  -DSVR_EXPERIMENTS builds can force that path onto small rings (SVR_FORCE_BIG=1) and cut them into
// parts of SVR_FORCE_ZSPLIT planes, so that the fuzzer reaches the multi-resource addressing with part boundaries everywhere.
static bool rings_need_big(const svr_ctx* c) {
    static const bool force_big = svr_exp_env_int("SVR_FORCE_BIG", 0) != 0;
    return c->density_all_bytes >= ((size_t)1 << 32) || force_big;
}

// ---- fill_params, one step per concern, in the order fill_params runs them --
// Camera, frame, material and outputs: what the kernel reads as the caller or svr_set_material gave it.
static int fill_camera_and_material(svr_ctx* c, const svr_camera* cam, const svr_frame* fr, const svr_outputs* out, MarchParams& P) {
    float tmp[16];
    mat_mul4(cam->world_inv, cam->cam_inv, tmp);            // vs_main.wgsl:22 (left-assoc)
    mat_mul4(tmp, cam->proj_inv, P.ndc_to_data);
    mat_mul4(cam->proj, cam->cam, P.pc);                    // vs_main.wgsl:19
    memcpy(P.world, cam->world, sizeof(P.world));
    for (int a = 0; a < 3; ++a) {
        SVR_REQUIRE(cam->volume_dimensions[a] >= 1.0f, "svr_render: volume_dimensions must be >= 1");
        P.size[a] = cam->volume_dimensions[a];
    }
    const float mx = fmaxf(P.size[0], fmaxf(P.size[1], P.size[2]));
    P.rel_step = fminf(fmaxf(sqrtf(mx) / 20.0f, 0.1f), 0.8f);   // fs_main.wgsl:20
    P.frame = *fr;
    if (P.frame.band_h <= 0) { P.frame.band_h = fr->out_h; P.frame.band_pitch = fr->out_h; }
    const svr_material& m = c->material;
    P.clim0 = m.clim[0]; P.clim1 = m.clim[1]; P.gamma = m.gamma; P.opacity = m.opacity;
    P.lmip_threshold = m.lmip_threshold; P.lmip_fall_off = m.lmip_fall_off;
    {   // integer rings: "(f32)v >= threshold" as an integer compare; NaN or beyond the largest value: never
        const float vmax = c->density_storage == SVR_U16 ? 65535.0f : 255.0f;
        P.lmip_threshold_raw = (uint32_t)vmax + 1u;
        if (m.lmip_threshold <= 0.0f) P.lmip_threshold_raw = 0u;
        else if (m.lmip_threshold <= vmax) P.lmip_threshold_raw = (uint32_t)ceilf(m.lmip_threshold);
    }
    P.clip_count = m.clipping_plane_count; P.clip_all = m.clipping_mode_all;
    for (uint32_t k = 0; k < m.clipping_plane_count; ++k)
        for (int a = 0; a < 4; ++a) P.clip[k][a] = c->clip_host[4 * k + a];
    P.lmip_max_samples = m.lmip_max_samples; P.fog_density = m.fog_density;
    P.render_mode = m.render_mode; P.weight_falloff = m.weight_falloff;
    for (int a = 0; a < 3; ++a) P.fog_color[a] = m.fog_color[a];
    P.color_count = m.color_count; P.colors = c->colors_dev; P.colorspace_srgb = m.colorspace_srgb;
    P.num_lods = c->num_lods;
    if (out->steps && !c->dbg_dev && hipMalloc((void**)&c->dbg_dev, 40 * sizeof(uint32_t)) == hipSuccess)
        (void)hipMemset(c->dbg_dev, 0, 40 * sizeof(uint32_t));      // 8 census counters + 16 u64 cycle sums
    P.dbg = out->steps ? c->dbg_dev : nullptr;
    P.rgba = out->rgba; P.depth = out->depth; P.label = out->label; P.flags = out->flags; P.steps = out->steps;
    P.pick = reinterpret_cast<unsigned long long*>(out->pick); P.pick_id = out->pick_id;
    return SVR_OK;
}

// svr_set_variant's bits as the kernel's switches, and the kernel kind and wave tile they choose for these rings.
static void fill_variant(svr_ctx* c, const svr_camera* cam, MarchParams& P) {
    // variant: bits 0-3 kernel kind (0 batched U=8, 1 simple, 2 batched U=4), bits 4-7 = 1 + log2 of the
    // wave tile width (0 = default 8x8), bit 8 = disable the LDS brick path
    int lw = ((c->variant >> 4) & 15) ? ((c->variant >> 4) & 15) - 1 : 3;
    if (lw > 6) lw = 6;
    // the weighted-average mode rides the span march (another reducer over the same batches); rings the span march
    // cannot address, and variant 1, take march_wavg, which is laid out like the simple kernel
    const bool wavg_simple = c->material.render_mode == SVR_MODE_WEIGHTED_AVERAGE &&
                             ((c->variant & 3) == 1 || !span_addressable(c) || rings_need_big(c));
    if ((c->variant & 3) == 1 || wavg_simple) lw = 3;         // the simple kernels are 8x8 only
    P.tile_log2w = lw;
    P.brick = (c->variant & 256) ? 0 : ((c->variant & 512) ? 2 : 1);     // never / always / auto (per wave)
    P.brick_lines = ((c->variant >> 16) & 0xFF) ? ((c->variant >> 16) & 0xFF) : 32;
    P.orient = (c->variant & 1024) ? 0 : 1;
    P.dbg_nowait = ((c->variant & SVR_EXP_VARIANT_BITS) >> 11) & 3;      // -DSVR_EXPERIMENTS builds: bit 11 no brick wait, bit 12 skip the march loop
    P.brick_lod_mask = ((c->variant >> 24) & 0xFF) ? ((c->variant >> 24) & 0xFF) : 0xFF;
    // Every wave starts with brick slabs of twice the plain length (the staged bytes per sample fall with the
    // slab length) and drops to the plain length at its first box that does not fit; variant bit 2: never long.
    P.slab_long = (c->variant & 4) ? 0 : 1;
    static const bool brick_pow2 = svr_exp_env_set("SVR_BRICK_POW2");         // A/B measurements (-DSVR_EXPERIMENTS builds)
    P.brick_pow2 = brick_pow2 ? 1 : 0;
    {   // vanishing point of the volume's x axis: (proj*cam) * (world * (1,0,0,0))
        const float ex[4] = { 1.0f, 0.0f, 0.0f, 0.0f };
        float wx[4];
        mat_vec4(cam->world, ex, wx);
        mat_vec4(P.pc, wx, P.xdir);
    }
    // kernel kind 0: span march, one wave per block; 2: span march, 2 x 2 waves per block; 1: simple (2 x 2)
    // (rings of 4 GiB or more fall back to the simple kernel's 64-bit addressing, see launch_nl)
    P.block_waves_log2 = ((c->variant & 3) == 0 && span_addressable(c) && !wavg_simple) ? 0 : 1;
}

// The frame in blocks, and the block -> tile table of this draw.
static int fill_placement(svr_ctx* c, const svr_frame* fr, hipStream_t stream, MarchParams& P) {
    const int lw = P.tile_log2w;
    const int bw = (1 << P.block_waves_log2) << lw, bh = (1 << P.block_waves_log2) * (64 >> lw);
    P.tiles_x = (fr->out_w + bw - 1) / bw; P.tiles_y = (fr->out_h + bh - 1) / bh;
    // variant bits 13-15: block -> tile policy (0 default = 64x64-pixel chunks dealt to the XCDs, 1 contiguous, 2.. other chunks)
    const int rc_order = tile_order_for(c, P.tiles_x, P.tiles_y, bw, bh, (c->variant >> 13) & 7, &P.tile_order);
    if (rc_order) return rc_order;
    // default placement: the same 64x64-pixel chunks, but sorted by the length of their rays for THIS camera
    // (longest first, snake-dealt to the XCDs); SVR_STATIC_PLACEMENT keeps the camera-independent table (A/B)
    static const bool static_placement = svr_exp_env_set("SVR_STATIC_PLACEMENT");
    if (!static_placement && ((c->variant >> 13) & 7) == 0 && P.tiles_x * P.tiles_y > 0)
        return tile_order_by_cost_for(c, P, bw, bh, stream, &P.tile_order);
    return SVR_OK;
}

// The per-LOD table: window, ring and scale of every LOD, which of the march's fast paths its numbers allow, its brick
// slab length and how often its cells are tested.  (The resources it is fetched through: fill_resources.)
static void fill_lod_table(const svr_ctx* c, MarchParams& P) {
    for (int l = 0; l < c->num_lods; ++l) {
        const LodStorage& L = c->lod[l];
        LodParams& Q = P.lod[l];
        Q.density = L.density; Q.labels = L.labels;
        for (int a = 0; a < 3; ++a) {
            Q.off[a] = L.state.offset[a];
            Q.shape[a] = (uint32_t)L.state.shape[a];
            Q.ring[a] = (uint32_t)L.ring[a];
            Q.wrap0[a] = (uint32_t)(L.state.offset[a] - floor_div(L.state.offset[a], L.ring[a]) * L.ring[a]);
            Q.scale[a] = L.state.scale[a];
            Q.addw[a] = (int32_t)Q.wrap0[a] - Q.off[a];
        }
        {
            bool ok = true;
            for (int a = 0; a < 3; ++a) {
                int e = 0;
                const float m = frexpf(Q.scale[a], &e);
                ok = ok && m == 0.5f && Q.scale[a] > 0.0f && Q.scale[a] <= 1.0f;    // exactly 2^-k
                ok = ok && P.size[a] * Q.scale[a] < 8388608.0f;                      // indices < 2^23
                ok = ok && Q.ring[a] < (1u << 15);                                   // packed i16 brick boxes
            }
            ok = ok && (double)P.size[1] * Q.scale[1] * Q.ring[1] < 16777216.0;      // row index < 2^24
            P.lod_pow2[l] = ok ? 1 : 0;
        }
        const uint32_t des = (uint32_t)svr_dtype_size(c->density_storage);
        Q.rx4 = Q.ring[0] * des;
        Q.base_bytes = (uint32_t)(c->lod_base_bytes[l] * des);
        for (int a = 0; a < 3; ++a) Q.ss[a] = P.size[a] * Q.scale[a];          // one IEEE multiply, as the kernel did
        for (int a = 0; a < 3; ++a) Q.rss[a] = 1.0f / Q.ss[a];
        {   // brick slabs (u8 rings): about 12 ring voxels of travel per slab (coarser LODs advance less per
            // iteration); rows in 16-byte groups, indices below 2^15 for the packed (y, z) brick address
            const float smax = fmaxf(Q.scale[0], fmaxf(Q.scale[1], Q.scale[2]));
            static const int slab_shift = svr_exp_env_int("SVR_SLAB_SHIFT", 0);     // A/B measurements (-DSVR_EXPERIMENTS builds)
            const int slab = std::max(8, (smax > 0.75f ? 16 : (smax > 0.375f ? 32 : 64)) >> slab_shift);
            // (ring rows must be whole 16-byte groups: 16 / 8 / 4 voxels for u8 / u16 / f32 rings)
            bool ok = ((Q.ring[0] * des) & 15u) == 0u && (P.brick_lod_mask >> l & 1);
            // (the wave's box is reduced as packed 16-bit halves, slab_box.h: a LOD whose window leaves [0, 32767] stages none)
            ok = ok && svr_slab_box_mode_of(Q.off, Q.shape) == SVR_SLAB_BOX_PACKED;
            Q.slab = ok ? slab : 0;
            // empty-space skipping: cell tests every `skip_batches` batches of 8 iterations, such that a ray
            // (0.8 voxels of the finest level per iteration, fs_main.wgsl:20) travels at most one cell between two
            // tests on every axis (checked again per lane in the kernel): 8^3 cells at scale 1 and 4^3 cells at scale
            // 1/2 -> every batch; 4^3 cells at scale 1/4 -> every other batch
            Q.cell_base = (uint32_t)(L.cell_base * des);
            for (int a = 0; a < 3; ++a) Q.cdim[a] = (uint32_t)L.cdim[a];
            Q.cshift = L.cshift;
            Q.skip_batches = 0;
            if (L.cells_dil && P.lod_pow2[l]) {
                const float room = (float)(1 << L.cshift) - 0.5f, per_batch = smax * 8.0f * P.rel_step;
                Q.skip_batches = per_batch * 4.0f <= room ? 4 : (per_batch * 2.0f <= room ? 2 : (per_batch <= room ? 1 : 0));
            }
        }
    }
    P.ss_pow2 = 1;
    for (int l = 0; l < c->num_lods; ++l)
        for (int a = 0; a < 3; ++a) P.ss_pow2 = P.ss_pow2 && svr_ss_pow2(P.lod[l].ss[a]);
}

// Empty-space skipping: does this draw test the macro cells at all, and with which policy bits?  -> whether it does.
static bool fill_skip_policy(const svr_ctx* c, MarchParams& P) {
    const svr_material& m = c->material;
    // skip only when some texel value can reach the threshold and not every one does: threshold = +inf (or NaN)
    // is the "full" march, whose point is the traversal itself; variant bit 3 switches skipping off (A/B)
    // A state machine that can never stop (no fall-off, no sample limit: MIP, _material.py lmip_uniforms) is the running
    // maximum of the ray; a lane that follows one can then pass every block that cannot beat it, like an empty one.
    const bool mip_like = m.lmip_fall_off == 0.0f && m.lmip_max_samples == INT32_MAX;
    const bool skip = c->cells_dil_all && !(c->variant & 8) && m.render_mode == SVR_MODE_LMIP &&       // (a mean needs every sample)
                      (mip_like || (P.lmip_threshold_raw > 0u &&
                      (c->density_storage == SVR_F32 ? (m.lmip_threshold > 0.0f && m.lmip_threshold < INFINITY)
                                                     : P.lmip_threshold_raw <= (c->density_storage == SVR_U16 ? 65535u : 255u))));
    static const int skip_flags_env = svr_exp_env_int("SVR_SKIP_FLAGS", 1);      // A/B measurements (-DSVR_EXPERIMENTS builds)
    P.skip_flags = (skip_flags_env & 1) | (mip_like ? 2 : 0);
    P.cells_all = skip ? c->cells_dil_all : nullptr;
    P.cells_all_bytes = skip ? (uint32_t)c->cells_all_bytes : 0u;
    return skip;
}

// LDS bytes per wave for brick staging.
static void fill_brick_size(const svr_camera* cam, const svr_frame* fr, bool skip, MarchParams& P) {
    // LDS per wave: 8 KiB holds the box of a 16..64-iteration slab of byte voxels and lets 20 one-wave blocks share
    // a CU's 160 KiB.  2- and 4-byte voxels fit shorter slabs in the same 8 KiB; 16 KiB for them (10 waves per CU)
    // measured slower: K1 full, f32 rings 1.60 ms against 1.31 ms (SVR_BRICK_BYTES: experiments)
    static const int brick_bytes_env = svr_exp_env_int("SVR_BRICK_BYTES", 0);
    P.brick_bytes = brick_bytes_env >= 1024 && brick_bytes_env <= 65536 ? (brick_bytes_env & ~15) : 8192;
    if (!brick_bytes_env && !skip) {
        // When a pixel is wider than about 1.5 finest-level voxels at the volume's centre (a 2048^3 volume seen
        // whole at 1080p: 1.8), the 64 rays of a wave are that far apart and the box of even a short slab outgrows
        // 8 KiB; 16 KiB per wave (10 waves per CU) then wins: config 5, K1, full mode 5.28 -> 4.70 ms.  Not while
        // empty-space skipping is active: its cell tests want the occupancy (config 5 LMIP: 0.80 ms at 8 KiB, 1.08 at 16)
        // (32 KiB: 5.61, 64 KiB: 9.35; at config 2's 0.9 voxels per pixel 16 KiB loses 20 %).
        const float centre[4] = { 0.5f * P.size[0] - 0.5f, 0.5f * P.size[1] - 0.5f, 0.5f * P.size[2] - 0.5f, 1.0f };
        float w[4], q[4];
        mat_vec4(cam->world, centre, w);
        mat_vec4(P.pc, w, q);
        if (q[3] > 0.0f) {
            const float a[4] = { q[0] / q[3], q[1] / q[3], q[2] / q[3], 1.0f };
            const float b[4] = { a[0] + 2.0f / (float)fr->frame_w, a[1], a[2], 1.0f };
            float da[4], db[4];
            mat_vec4(P.ndc_to_data, a, da);
            mat_vec4(P.ndc_to_data, b, db);
            float d2 = 0.0f;
            for (int k = 0; k < 3; ++k) { const float d = db[k] / db[3] - da[k] / da[3]; d2 += d * d; }
            if (d2 >= 2.25f && d2 < 1e12f) P.brick_bytes = 16384;
        }
    }
}

// The buffer resources every LOD's texels are fetched through, and its micro-block copy.
static void fill_resources(const svr_ctx* c, MarchParams& P) {
    P.density_all = c->density_all;
    P.span_ok = span_addressable(c) ? 1 : 0;
    P.per_lod_rsrc = rings_need_big(c) ? 1 : 0;
    P.density_all_bytes = P.per_lod_rsrc ? 0u : (uint32_t)c->density_all_bytes;
    for (int l = 0; l < c->num_lods; ++l) {
        LodParams& Q = P.lod[l];
        Q.nparts = 1u; Q.zsplit = Q.ring[2]; Q.part_bytes = 0u; Q.rbytes_last = 0u;
        // the micro-block copy of the ring (svr_lod_desc::blocked_twin): always behind a resource of its own, which is cut
        // into parts exactly like the ring's where that is (the march may use it only where the parts hold whole blocks)
        // (the march addresses it from the packed voxel index y | z << 16: both below 2^16, whatever the ray)
        Q.twin = (c->lod[l].twin && P.size[1] * Q.scale[1] < 65536.0f && P.size[2] * Q.scale[2] < 65536.0f) ? (uint32_t)c->lod[l].twin_policy : 0u;
        Q.twin_rbase = c->lod[l].twin;
        Q.twin_rbytes = (uint32_t)std::min<uint64_t>((uint64_t)c->lod[l].voxels * svr_dtype_size(c->density_storage) + 64, 0xFFFFFFFFull);
        if (P.per_lod_rsrc) {
            // one resource per LOD, or parts of whole ring z planes for a ring of 4 GiB or more (span_addressable checked the count)
            const RingParts R = lod_ring_parts(c, l);
            Q.rbase = c->lod[l].density; Q.base_bytes = 0u;
            Q.nparts = R.nparts; Q.zsplit = R.zsplit; Q.part_bytes = R.part_bytes;
            Q.rbytes = R.rbytes; Q.rbytes_last = R.rbytes_last;
            Q.twin_rbytes = Q.rbytes;                       // (a full part's size where the ring is cut; part_rsrc sizes the last one)
            if (!R.twin_ok) Q.twin = 0u;                    // a part boundary inside a block: the march reads rows
        } else {
            Q.rbase = c->density_all; Q.rbytes = P.density_all_bytes;
        }
        Q.twin_w = Q.twin ? svr_twin_weights(c->density_storage == SVR_U8 ? 0 : (c->density_storage == SVR_U16 ? 1 : 2), Q.ring[0], Q.ring[1]) : 0u;
    }
    P.density_esh = c->density_storage == SVR_U8 ? 0 : (c->density_storage == SVR_U16 ? 1 : 2);
}

static int fill_params(svr_ctx* c, const svr_camera* cam, const svr_frame* fr, const svr_outputs* out, hipStream_t stream,
                       MarchParams& P) {
    SVR_REQUIRE(c && cam && fr && out && out->rgba, "svr_render: null argument");
    SVR_REQUIRE(c->material_set, "svr_render: svr_set_material has not been called");
    SVR_REQUIRE(fr->frame_w > 0 && fr->frame_h > 0 && fr->out_w > 0 && fr->out_h > 0, "svr_render: empty frame");
    SVR_REQUIRE(fr->x0 >= 0 && fr->y0 >= 0, "svr_render: negative tile origin");
    memset(&P, 0, sizeof(P));
    { const int rc = fill_camera_and_material(c, cam, fr, out, P); if (rc) return rc; }
    fill_variant(c, cam, P);
    { const int rc = fill_placement(c, fr, stream, P); if (rc) return rc; }
    fill_lod_table(c, P);
    const bool skip = fill_skip_policy(c, P);
    fill_brick_size(cam, fr, skip, P);
    fill_resources(c, P);
    return SVR_OK;
}

// What svr_render and svr_time_render enqueue on stream s: behind the published uploads, `iters` marches (between the
// context's two timing events if `timed`), then the marks that order later table rewrites and uploads behind them.
static int enqueue_march(svr_ctx* c, const MarchParams& P, hipStream_t s, int iters, bool timed) {
    if (c->have_published) SVR_HIP_TRY(hipStreamWaitEvent(s, c->uploads_published, 0));
    if (timed) SVR_HIP_TRY(hipEventRecord(c->ev_a, s));
    for (int i = 0; i < iters; ++i) SVR_HIP_TRY(svr_launch_march(P, (c->variant & 3) == 1 ? 1 : 0, s));
    if (timed) SVR_HIP_TRY(hipEventRecord(c->ev_b, s));
    { const int rco = cost_order_drawn(c, P, s); if (rco) return rco; }
    return mark_render(c, s);
}

extern "C" {

int svr_render(svr_ctx* c, const svr_camera* cam, const svr_frame* fr, const svr_outputs* out, void* stream) {
    // the caller's stream; NULL is the device's default stream (what torch.cuda.current_stream() is
    // unless the caller switched streams), so the draw is ordered with the caller's other work on it
    hipStream_t s = static_cast<hipStream_t>(stream);
    MarchParams P;
    int rc = fill_params(c, cam, fr, out, s, P);
    if (rc) return rc;
    DeviceGuard guard(c->device);
    return enqueue_march(c, P, s, 1, false);
}

int svr_time_render(svr_ctx* c, const svr_camera* cam, const svr_frame* fr, const svr_outputs* out,
                    int iters, float* avg_ms) {
    SVR_REQUIRE(avg_ms && iters >= 1, "svr_time_render: bad arguments");
    MarchParams P;
    int rc = fill_params(c, cam, fr, out, c->render_stream, P);
    if (rc) return rc;
    DeviceGuard guard(c->device);
    rc = enqueue_march(c, P, c->render_stream, iters, true);
    if (rc) return rc;
    SVR_HIP_TRY(hipEventSynchronize(c->ev_b));
    float ms = 0.f;
    SVR_HIP_TRY(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
    *avg_ms = ms / (float)iters;
    return SVR_OK;
}

}  // extern "C"
