// Host side of the C ABI declared in include/svr.h: the error text, the context's lifetime, LOD state, material,
// variant, the small pass-through entry points (untile, pool2x, compose, outline), sync, debug counters and pointers.
// The rest of the ABI's host side:
//   svr_upload.hip   staging and uploads, publish / mark / pending / stats / tickets, clear and read-back
//                    (pack_rows.h: the threaded gather into the staging slot)
//   svr_render.hip   svr_render and svr_time_render: fill_params, how the rings are cut into resources, and the
//                    block -> tile placement that march_kernel.hip's comments look for here (tile_order.h builds the tables)
//   svr_modes.hip    slice, slab, composite, iso, histogram and objects, and the setters of their state
//   svr_host.h       what these units share: the kernel units' launchers, the context's extension, SVR_REQUIRE
#include <math.h>
#include <string.h>

#include <algorithm>

#include "svr_host.h"

static thread_local std::string g_err;
void svr_set_error(const std::string& msg) { g_err = msg; }

extern "C" {

const char* svr_last_error(void) { return g_err.c_str(); }
int svr_abi_version(void) { return SVR_ABI_VERSION; }

int svr_create(int device, int num_lods, const svr_lod_desc* lods, svr_ctx** out_ctx) {
    SVR_REQUIRE(out_ctx && lods, "svr_create: null argument");
    SVR_REQUIRE(num_lods >= 1 && num_lods <= SVR_MAX_LODS, "svr_create: num_lods out of range");
    int ndev = 0;
    SVR_HIP_TRY(hipGetDeviceCount(&ndev));
    SVR_REQUIRE(device >= 0 && device < ndev, "svr_create: no such HIP device (is a GPU visible?)");
    for (int l = 0; l < num_lods; ++l) {
        for (int a = 0; a < 3; ++a)
            SVR_REQUIRE(lods[l].ring_dims[a] >= 1 && lods[l].ring_dims[a] < (1 << 24),
                        "svr_create: ring extent must be in [1, 2^24)");
        SVR_REQUIRE(lods[l].density_storage == SVR_F32 || lods[l].density_storage == SVR_U8 ||
                    lods[l].density_storage == SVR_U16,
                    "svr_create: density_storage must be SVR_F32, SVR_U8 or SVR_U16");
        SVR_REQUIRE(lods[l].density_storage == lods[0].density_storage,
                    "svr_create: all LODs must use the same density_storage");
        SVR_REQUIRE(lods[l].blocked_twin >= 0 && lods[l].blocked_twin <= 2, "svr_create: blocked_twin must be 0, 1 or 2");
        SVR_REQUIRE(!lods[l].blocked_twin ||
                    (lods[l].ring_dims[0] % 8 == 0 && lods[l].ring_dims[1] % 4 == 0 && lods[l].ring_dims[2] % 4 == 0),
                    "svr_create: blocked_twin needs ring extents that are multiples of (8, 4, 4)");
        SVR_REQUIRE((lods[l].no_labels != 0) == (lods[0].no_labels != 0), "svr_create: all LODs must agree on no_labels");
    }
    DeviceGuard guard(device);
    svr_ctx* c = new svr_ctx_ext();       // (no table, SVR_INTERP_NEAREST, no planes: the extension's own initialisers)
    c->device = device; c->num_lods = num_lods;
    c->render_stream = nullptr; c->upload_stream = nullptr; c->uploads_published = nullptr;
    c->have_published = false; c->colors_dev = nullptr; c->colors_cap = 0; c->material_set = false;
    c->variant = 0; c->slot_bytes = 0; c->next_slot = 0; c->ev_a = c->ev_b = nullptr;
    c->next_ticket = 1;
    c->comm = nullptr; c->comm_rank = 0; c->comm_size = 1;
    for (auto& t : c->tickets) t = nullptr;
    c->uploads_marker = nullptr; c->marker_set = false; c->dbg_dev = nullptr;
    for (auto& s : c->slot) { s.host = s.dev = nullptr; s.done = nullptr; s.used = false; }
    for (int l = 0; l < SVR_MAX_LODS; ++l) { c->lod[l].density = nullptr; c->lod[l].twin = nullptr; c->lod[l].labels = nullptr; c->lod[l].voxels = 0; }
    c->density_all = nullptr; c->labels_all = nullptr; c->density_all_bytes = 0; c->twin_all = nullptr; c->twin_all_bytes = 0;
    c->cells_raw_all = c->cells_dil_all = nullptr; c->cells_all_bytes = 0;
    c->density_storage = lods[0].density_storage;
    c->no_labels = lods[0].no_labels != 0 ? 1 : 0;
    c->density_u8 = lods[0].density_storage == SVR_U8 ? 1 : 0;
    c->staged_bytes = 0; c->upload_seconds = 0.0;

    auto fail = [&](int code) { svr_destroy(c); return code; };
    if (hipStreamCreateWithFlags(&c->render_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->uploads_published, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->uploads_marker, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->ev_a) != hipSuccess || hipEventCreate(&c->ev_b) != hipSuccess) {
        svr_set_error("svr_create: stream/event creation failed");
        return fail(SVR_ERR_HIP);
    }
    size_t total = 0;   // in VOXELS (256-voxel aligned): the same offsets serve the u8/f32 density and the u32 labels
    for (int l = 0; l < num_lods; ++l) {
        LodStorage& L = c->lod[l];
        for (int a = 0; a < 3; ++a) L.ring[a] = lods[l].ring_dims[a];
        L.voxels = (size_t)L.ring[0] * (size_t)L.ring[1] * (size_t)L.ring[2];
        memset(&L.state, 0, sizeof(L.state));
        L.state.scale[0] = L.state.scale[1] = L.state.scale[2] = 1.0f;
        c->lod_base_bytes[l] = total;                         // voxel offset of this LOD
        total += (L.voxels + 255) & ~(size_t)255;
    }
    // the micro-block copies (svr_lod_desc::blocked_twin) live in an allocation of their own, each behind a buffer resource
    // of its own: the copies must not push the RINGS over the 4 GiB below which one resource reaches every LOD (the faster
    // build of the march; config 5's byte rings are 2.4 GB, with their copies 4.8)
    const size_t ring_voxels = total;
    size_t twin_base[SVR_MAX_LODS] = {0}, twin_voxels = 0;
    for (int l = 0; l < num_lods; ++l) {
        if (!lods[l].blocked_twin) continue;
        twin_base[l] = twin_voxels;
        twin_voxels += (c->lod[l].voxels + 255) & ~(size_t)255;
    }
    const size_t des = svr_dtype_size(c->density_storage);
    c->density_all_bytes = total * des + 64;                 // + slack: 16-byte brick loads may overrun a row end
    c->twin_all_bytes = twin_voxels ? twin_voxels * des + 64 : 0;
    // one allocation per plane type; zero-initialised textures (_wrapping_buffer.py:50-59)
    if (hipMalloc((void**)&c->density_all, c->density_all_bytes) != hipSuccess ||
        (c->twin_all_bytes && hipMalloc((void**)&c->twin_all, c->twin_all_bytes) != hipSuccess) ||
        (!c->no_labels && hipMalloc((void**)&c->labels_all, ring_voxels * sizeof(uint32_t)) != hipSuccess)) {
        svr_set_error("svr_create: out of device memory for ring textures");
        return fail(SVR_ERR_NOMEM);
    }
    if (hipMemsetAsync(c->density_all, 0, c->density_all_bytes, c->upload_stream) != hipSuccess ||
        (c->twin_all_bytes && hipMemsetAsync(c->twin_all, 0, c->twin_all_bytes, c->upload_stream) != hipSuccess) ||
        (!c->no_labels && hipMemsetAsync(c->labels_all, 0, ring_voxels * sizeof(uint32_t), c->upload_stream) != hipSuccess)) {
        svr_set_error("svr_create: memset failed");
        return fail(SVR_ERR_HIP);
    }
    for (int l = 0; l < num_lods; ++l) {
        c->lod[l].density = static_cast<char*>(c->density_all) + c->lod_base_bytes[l] * des;
        c->lod[l].labels = c->no_labels ? nullptr : c->labels_all + c->lod_base_bytes[l];
        c->lod[l].twin = lods[l].blocked_twin ? static_cast<char*>(c->twin_all) + twin_base[l] * des : nullptr;
        c->lod[l].twin_policy = lods[l].blocked_twin;
    }
    {   // macro-cell maxima (empty-space skipping): one grid of cells per LOD whose extents are multiples of 8.
        // The finest level gets 8^3-slot cells, the coarser ones 4^3: their structures are half / a quarter the size
        // in slots, and a ray advances less per iteration there, so the finer grid costs no extra tests.
        size_t cells = 0;
        for (int l = 0; l < num_lods; ++l) {
            LodStorage& L = c->lod[l];
            L.cells_raw = L.cells_dil = nullptr; L.cell_base = 0;
            L.cshift = l == 0 ? 3 : 2;
            for (int a = 0; a < 3; ++a) L.cdim[a] = L.ring[a] >> L.cshift;
            if ((L.ring[0] | L.ring[1] | L.ring[2]) & 7) continue;
            L.cell_base = cells;
            cells += ((size_t)L.cdim[0] * L.cdim[1] * L.cdim[2] + 63) & ~(size_t)63;
        }
        c->cells_all_bytes = cells * des;
        if (cells && c->cells_all_bytes < ((size_t)1 << 31)) {
            if (hipMalloc(&c->cells_raw_all, c->cells_all_bytes) != hipSuccess ||
                hipMalloc(&c->cells_dil_all, c->cells_all_bytes) != hipSuccess) {
                svr_set_error("svr_create: out of device memory for the macro-cell grids");
                return fail(SVR_ERR_NOMEM);
            }
            if (hipMemsetAsync(c->cells_raw_all, 0, c->cells_all_bytes, c->upload_stream) != hipSuccess ||
                hipMemsetAsync(c->cells_dil_all, 0, c->cells_all_bytes, c->upload_stream) != hipSuccess) {
                svr_set_error("svr_create: memset failed");
                return fail(SVR_ERR_HIP);
            }
            for (int l = 0; l < num_lods; ++l) {
                LodStorage& L = c->lod[l];
                if ((L.ring[0] | L.ring[1] | L.ring[2]) & 7) continue;
                L.cells_raw = static_cast<char*>(c->cells_raw_all) + L.cell_base * des;
                L.cells_dil = static_cast<char*>(c->cells_dil_all) + L.cell_base * des;
            }
        } else {
            c->cells_all_bytes = 0;
        }
    }
    if (hipEventRecord(c->uploads_published, c->upload_stream) != hipSuccess) return fail(SVR_ERR_HIP);
    c->have_published = true;
    *out_ctx = c;
    return SVR_OK;
}

int svr_destroy(svr_ctx* c) {
    if (!c) return SVR_OK;
    DeviceGuard guard(c->device);
    if (c->comm) (void)svr_comm_destroy(c);
    if (c->render_stream) (void)hipStreamSynchronize(c->render_stream);
    if (c->upload_stream) (void)hipStreamSynchronize(c->upload_stream);
    if (c->density_all) (void)hipFree(c->density_all);
    if (c->twin_all) (void)hipFree(c->twin_all);
    if (c->labels_all) (void)hipFree(c->labels_all);
    if (c->cells_raw_all) (void)hipFree(c->cells_raw_all);
    if (c->cells_dil_all) (void)hipFree(c->cells_dil_all);
    for (auto& s : c->slot) {
        if (s.host) (void)hipHostFree(s.host);
        if (s.dev) (void)hipFree(s.dev);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    if (c->colors_dev) (void)hipFree(c->colors_dev);
    for (float* p : c->colors_retired) (void)hipFree(p);
    if (svr_ext(c)->tf_dev) (void)hipFree(svr_ext(c)->tf_dev);
    for (float* p : svr_ext(c)->tf_retired) (void)hipFree(p);
    svr_ext(c)->mesh.release(); svr_ext(c)->comp.release(); svr_ext(c)->dist.release(); svr_ext(c)->split.release();
    if (c->dbg_dev) (void)hipFree(c->dbg_dev);
    for (auto& t : c->tile_orders) if (t.dev) (void)hipFree(t.dev);
    for (auto& t : c->cost_orders) {
        if (t.dev) (void)hipFree(t.dev);
        if (t.host) (void)hipHostFree(t.host);
        if (t.copied) (void)hipEventDestroy(t.copied);
        if (t.drawn) (void)hipEventDestroy(t.drawn);
    }
    if (c->uploads_published) (void)hipEventDestroy(c->uploads_published);
    for (auto& m : c->render_marks) if (m.done) (void)hipEventDestroy(m.done);
    for (auto& t : c->tickets) if (t) (void)hipEventDestroy(t);
    if (c->uploads_marker) (void)hipEventDestroy(c->uploads_marker);
    if (c->ev_a) (void)hipEventDestroy(c->ev_a);
    if (c->ev_b) (void)hipEventDestroy(c->ev_b);
    if (c->render_stream) (void)hipStreamDestroy(c->render_stream);
    if (c->upload_stream) (void)hipStreamDestroy(c->upload_stream);
    delete svr_ext(c);
    return SVR_OK;
}

int svr_set_lod_state(svr_ctx* c, int lod, const svr_lod_state* st) {
    SVR_REQUIRE(c && st, "svr_set_lod_state: null argument");
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, "svr_set_lod_state: lod out of range");
    for (int a = 0; a < 3; ++a) {
        SVR_REQUIRE(st->offset[a] >= 0 && st->shape[a] >= 0, "svr_set_lod_state: negative offset/shape");
        SVR_REQUIRE(st->shape[a] <= c->lod[lod].ring[a], "svr_set_lod_state: ROI larger than the ring");
    }
    c->lod[lod].state = *st;
    return SVR_OK;
}

int svr_get_lod_state(svr_ctx* c, int lod, svr_lod_state* st) {
    SVR_REQUIRE(c && st, "svr_get_lod_state: null argument");
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, "svr_get_lod_state: lod out of range");
    *st = c->lod[lod].state;
    return SVR_OK;
}

int svr_set_material(svr_ctx* c, const svr_material* m) {
    SVR_REQUIRE(c && m, "svr_set_material: null argument");
    SVR_REQUIRE(m->color_count >= 1 && m->colors, "svr_set_material: at least one colour is required");
    SVR_REQUIRE(m->clipping_plane_count <= SVR_MAX_CLIP_PLANES, "svr_set_material: too many clipping planes");
    SVR_REQUIRE(m->clipping_plane_count == 0 || m->clipping_planes, "svr_set_material: clipping_planes is null");
    SVR_REQUIRE(m->render_mode == SVR_MODE_LMIP || m->render_mode == SVR_MODE_WEIGHTED_AVERAGE, "svr_set_material: unknown render_mode");
    SVR_REQUIRE(m->render_mode != SVR_MODE_WEIGHTED_AVERAGE || (m->weight_falloff >= 0.0f && m->weight_falloff < INFINITY),
                "svr_set_material: weight_falloff must be finite and >= 0");
    DeviceGuard guard(c->device);
    const size_t ncol = (size_t)m->color_count * 4;
    const bool same_colors = c->material_set && c->colors_host.size() == ncol &&
                             memcmp(c->colors_host.data(), m->colors, ncol * sizeof(float)) == 0;
    c->material = *m;
    c->material.colors = nullptr;
    c->material.clipping_planes = nullptr;
    c->clip_host.assign(m->clipping_planes, m->clipping_planes + (size_t)m->clipping_plane_count * 4);
    if (same_colors) return SVR_OK;
    c->colors_host.assign(m->colors, m->colors + ncol);
    // The colour table of renders still in flight must not change under them: every new table goes into a
    // fresh device buffer (the old one is freed once the device has drained; tables are tiny and change
    // rarely), so no device-wide synchronisation is needed here.
    float* fresh = nullptr;
    const uint32_t cap = std::max<uint32_t>(256u, m->color_count);
    if (hipMalloc((void**)&fresh, (size_t)cap * 4 * sizeof(float)) != hipSuccess) {
        svr_set_error("svr_set_material: out of device memory"); return SVR_ERR_NOMEM;
    }
    SVR_HIP_TRY(hipMemcpy(fresh, c->colors_host.data(), c->colors_host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (c->colors_dev) c->colors_retired.push_back(c->colors_dev);
    if (c->colors_retired.size() > 32) {                 // bounded: drain once in a long while
        SVR_HIP_TRY(hipDeviceSynchronize());
        for (float* p : c->colors_retired) (void)hipFree(p);
        c->colors_retired.clear();
    }
    c->colors_dev = fresh;
    c->colors_cap = cap;
    c->material_set = true;
    return SVR_OK;
}

int svr_set_variant(svr_ctx* c, int variant) {
    SVR_REQUIRE(c, "svr_set_variant: null ctx");
    // bits 11-12 are timing experiments that render WRONG pixels: only a -DSVR_EXPERIMENTS build knows them
    SVR_REQUIRE((variant & 0x1800 & ~SVR_EXP_VARIANT_BITS) == 0,
                "svr_set_variant: bits 11-12 (timing experiments) exist only in builds made with -DSVR_EXPERIMENTS");
    c->variant = variant;
    return SVR_OK;
}

}  // extern "C"

// ---- helpers of the other host units (svr_host.h) ---------------------------
int check_region(svr_ctx* c, int lod, const int32_t off[3], const int32_t shape[3], const char* who) {
    if (!c || !off || !shape) { svr_set_error(std::string(who) + ": null argument"); return SVR_ERR_INVALID; }
    if (lod < 0 || lod >= c->num_lods) { svr_set_error(std::string(who) + ": lod out of range"); return SVR_ERR_INVALID; }
    for (int a = 0; a < 3; ++a) {
        if (off[a] < 0 || shape[a] < 0 || (int64_t)off[a] + shape[a] > c->lod[lod].ring[a]) {
            svr_set_error(std::string(who) + ": region outside the ring");
            return SVR_ERR_RANGE;
        }
    }
    return SVR_OK;
}

// A render enqueued earlier may still be reading the ring slots an upload is
// about to overwrite: order the upload stream behind it (the reference gets this
// ordering from running everything on one queue).
int uploads_after_render(svr_ctx* c) {
    std::lock_guard<std::mutex> lock(c->marks_mu);
    for (auto& m : c->render_marks)
        if (m.pending) {
            SVR_HIP_TRY(hipStreamWaitEvent(c->upload_stream, m.done, 0));
            m.pending = false;
        }
    return SVR_OK;
}

// Remember that stream `s` carries a render enqueued just now (one event per stream; a stream's later
// render re-records its event, which then covers the earlier ones on that stream too).
int mark_render(svr_ctx* c, hipStream_t s) {
    std::lock_guard<std::mutex> lock(c->marks_mu);
    svr_ctx::RenderMark* mark = nullptr;
    for (auto& m : c->render_marks) if (m.stream == s) { mark = &m; break; }
    if (!mark) {
        if (c->render_marks.size() >= 64) {
            // a caller cycling through many short-lived streams: recycle the oldest entry, after ordering the
            // upload stream behind the render it still stands for
            svr_ctx::RenderMark old = c->render_marks.front();
            if (old.pending) SVR_HIP_TRY(hipStreamWaitEvent(c->upload_stream, old.done, 0));
            c->render_marks.erase(c->render_marks.begin());
            old.stream = s; old.pending = false;
            c->render_marks.push_back(old);
        } else {
            svr_ctx::RenderMark m{ s, nullptr, false };
            SVR_HIP_TRY(hipEventCreateWithFlags(&m.done, hipEventDisableTiming));
            c->render_marks.push_back(m);
        }
        mark = &c->render_marks.back();
    }
    SVR_HIP_TRY(hipEventRecord(mark->done, s));
    mark->pending = true;
    return SVR_OK;
}

extern "C" {

int svr_untile_stripes(svr_ctx* c, const void* gathered, void* frame_out, int frame_w, int frame_h,
                       int band_h, int nranks, int out_h, int elem_bytes, void* stream) {
    SVR_REQUIRE(c && gathered && frame_out, "svr_untile_stripes: null argument");
    SVR_REQUIRE(frame_w > 0 && frame_h > 0 && band_h > 0 && nranks > 0, "svr_untile_stripes: bad geometry");
    const int nbands = (frame_h + band_h - 1) / band_h;
    SVR_REQUIRE(out_h >= ((nbands + nranks - 1) / nranks) * band_h, "svr_untile_stripes: out_h too small for the frame");
    DeviceGuard guard(c->device);
    hipStream_t s = static_cast<hipStream_t>(stream);       // NULL = default stream, as in svr_render
    SVR_HIP_TRY(svr_launch_untile(gathered, frame_out, frame_w, frame_h, band_h, nranks, out_h, elem_bytes, s));
    return SVR_OK;
}

int svr_untile_grid(svr_ctx* c, const void* gathered, void* frame_out, int frame_w, int frame_h,
                    int tile_w, int tile_h, int grid_x, int grid_y, int elem_bytes, void* stream) {
    SVR_REQUIRE(c && gathered && frame_out, "svr_untile_grid: null argument");
    SVR_REQUIRE(frame_w > 0 && frame_h > 0 && tile_w > 0 && tile_h > 0 && grid_x > 0 && grid_y > 0, "svr_untile_grid: bad geometry");
    SVR_REQUIRE((int64_t)tile_w * grid_x >= frame_w && (int64_t)tile_h * grid_y >= frame_h, "svr_untile_grid: the tiles do not cover the frame");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(svr_launch_untile_grid(gathered, frame_out, frame_w, frame_h, tile_w, tile_h, grid_x, grid_y, elem_bytes,
                                       static_cast<hipStream_t>(stream)));
    return SVR_OK;
}

int svr_pool2x(int device, const void* src, void* dst, const int32_t src_dims[3], int dtype, int mode, void* stream) {
    SVR_REQUIRE(src && dst && src_dims, "svr_pool2x: null argument");
    for (int a = 0; a < 3; ++a)
        SVR_REQUIRE(src_dims[a] >= 2 && (src_dims[a] & 1) == 0, "svr_pool2x: every source extent must be even and >= 2");
    SVR_REQUIRE((dtype == SVR_U8 && mode == 0) || (dtype == SVR_F32 && mode == 0) || (dtype == SVR_U32 && mode == 1),
                "svr_pool2x: supported: mean of u8 / f32 (mode 0), max of u32 (mode 1)");
    if (dtype != SVR_U8) {                     // 8-byte loads of x pairs, 4-byte stores; the u8 kernel has a scalar path
        SVR_REQUIRE((uintptr_t)src % 8 == 0, "svr_pool2x: src must be 8-byte aligned for SVR_F32 / SVR_U32");
        SVR_REQUIRE((uintptr_t)dst % 4 == 0, "svr_pool2x: dst must be 4-byte aligned for SVR_F32 / SVR_U32");
    }
    DeviceGuard guard(device);
    SVR_HIP_TRY(svr_launch_pool2x(src, dst, src_dims, dtype, mode, static_cast<hipStream_t>(stream)));
    return SVR_OK;
}

int svr_compose(svr_ctx* c, const float* rgba, const float* depth, const uint8_t* flags, int width, int height,
                const svr_compose_params* params, uint8_t* out_rgba8, float* inout_depth, void* stream) {
    SVR_REQUIRE(c && rgba && params && out_rgba8, "svr_compose: null argument");
    SVR_REQUIRE(width >= 0 && height >= 0, "svr_compose: negative size");
    SVR_REQUIRE(!inout_depth || depth, "svr_compose: a depth test needs the render's depth plane");
    SVR_REQUIRE((uintptr_t)rgba % 16 == 0, "svr_compose: rgba must be 16-byte aligned");
    SVR_REQUIRE((uintptr_t)out_rgba8 % 4 == 0, "svr_compose: out_rgba8 must be 4-byte aligned");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(svr_launch_compose(rgba, depth, flags, width, height, *params, out_rgba8, inout_depth,
                                   static_cast<hipStream_t>(stream)));
    return SVR_OK;
}

int svr_outline(svr_ctx* c, const float* rgba, const float* depth, const uint32_t* label, const uint8_t* flags,
                int width, int height, const svr_outline_params* params, const float* colors, uint32_t color_count,
                const uint32_t* selected, uint32_t selected_count, float* out_rgba, uint8_t* edge_mask, void* stream) {
    SVR_REQUIRE(c && rgba && label && flags && params && out_rgba, "svr_outline: null argument");
    SVR_REQUIRE(width >= 0 && height >= 0, "svr_outline: negative size");
    const svr_outline_params& q = *params;
    SVR_REQUIRE(q.radius >= 1 && q.radius <= 16, "svr_outline: radius must be in [1, 16]");
    SVR_REQUIRE(!isnan(q.depth_tolerance), "svr_outline: depth_tolerance is NaN (< 0 turns the depth test off)");
    SVR_REQUIRE(q.depth_tolerance < 0.0f || depth, "svr_outline: a depth tolerance needs the render's depth plane");
    SVR_REQUIRE(!q.color_by_label || (colors && color_count > 0), "svr_outline: color_by_label needs at least one color");
    SVR_REQUIRE(q.color[3] >= 0.0f && q.color[3] <= 1.0f, "svr_outline: outline opacity color[3] must be in [0, 1]");
    SVR_REQUIRE(q.dim_unselected >= 0.0f && q.dim_unselected <= 1.0f, "svr_outline: dim_unselected must be in [0, 1]");
    SVR_REQUIRE(selected_count == 0 || selected, "svr_outline: selected_count > 0 with a NULL selected pointer");
    SVR_REQUIRE(((uintptr_t)rgba | (uintptr_t)out_rgba | (uintptr_t)colors) % 16 == 0,
                "svr_outline: rgba, out_rgba and colors must be 16-byte aligned");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(svr_launch_outline(rgba, depth, label, flags, width, height, q, colors, color_count, selected,
                                   selected_count, out_rgba, edge_mask, static_cast<hipStream_t>(stream)));
    return SVR_OK;
}

int svr_sync(svr_ctx* c) {
    SVR_REQUIRE(c, "svr_sync: null ctx");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(hipStreamSynchronize(c->upload_stream));
    SVR_HIP_TRY(hipStreamSynchronize(c->render_stream));
    return SVR_OK;
}

int svr_sync_uploads(svr_ctx* c) {
    SVR_REQUIRE(c, "svr_sync_uploads: null ctx");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(hipStreamSynchronize(c->upload_stream));
    return SVR_OK;
}

int svr_debug_counters(svr_ctx* c, uint32_t out[8], int reset) {
    SVR_REQUIRE(c && out, "svr_debug_counters: null argument");
    memset(out, 0, 8 * sizeof(uint32_t));
    if (!c->dbg_dev) return SVR_OK;
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(hipDeviceSynchronize());
    SVR_HIP_TRY(hipMemcpy(out, c->dbg_dev, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (reset) SVR_HIP_TRY(hipMemset(c->dbg_dev, 0, 8 * sizeof(uint32_t)));
    return SVR_OK;
}

int svr_debug_timers(svr_ctx* c, uint64_t out[16], int reset) {
    SVR_REQUIRE(c && out, "svr_debug_timers: null argument");
    memset(out, 0, 16 * sizeof(uint64_t));
    if (!c->dbg_dev) return SVR_OK;
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(hipDeviceSynchronize());
    SVR_HIP_TRY(hipMemcpy(out, c->dbg_dev + 8, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) SVR_HIP_TRY(hipMemset(c->dbg_dev + 8, 0, 16 * sizeof(uint64_t)));
    return SVR_OK;
}

int svr_lod_twin_ptr(svr_ctx* c, int lod, void** twin) {
    SVR_REQUIRE(c && twin, "svr_lod_twin_ptr: null argument");
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, "svr_lod_twin_ptr: lod out of range");
    *twin = c->lod[lod].twin;
    return SVR_OK;
}

int svr_lod_cell_ptrs(svr_ctx* c, int lod, void** raw, void** blk, int32_t cdim[3], int32_t* cshift) {
    SVR_REQUIRE(c && raw && blk && cdim && cshift, "svr_lod_cell_ptrs: null argument");
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, "svr_lod_cell_ptrs: lod out of range");
    const LodStorage& L = c->lod[lod];
    *raw = L.cells_raw; *blk = L.cells_dil;         // both null for a LOD without a grid
    for (int a = 0; a < 3; ++a) cdim[a] = L.cdim[a];
    *cshift = L.cshift;
    return SVR_OK;
}

int svr_lod_device_ptrs(svr_ctx* c, int lod, void** density, void** labels) {
    SVR_REQUIRE(c, "svr_lod_device_ptrs: null ctx");
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, "svr_lod_device_ptrs: lod out of range");
    if (density) *density = c->lod[lod].density;
    if (labels) *labels = c->lod[lod].labels;
    return SVR_OK;
}

}  // extern "C"
