// The render modes and passes of the C ABI (include/svr.h) beside the march: slices, slabs, composite and iso renders,
// histograms, object and contact tables, surface meshes, connected components, distance transforms and their watershed, and the three setters of the
// state they share (svr_ctx_ext, svr_host.h).  Each entry point checks its arguments and hands the launch of its kernel
// unit to draw_ordered; svr_mesh, svr_components, svr_distance, svr_nearest and svr_split besides keep the scratch memory their kernels work in.
#include <math.h>

#include <algorithm>

#include "svr_host.h"
#include "box_units.h"
#include "mesh_plan.h"
#include "components_plan.h"
#include "distance_plan.h"
#include "split_plan.h"

// What svr_slice, svr_slab, svr_composite and svr_iso check first, in this order (who: the entry point's name, the
// prefix of its error texts; args_ok: its own null test), and the frame with band_h defaulted to one band.
static int draw_prologue(const char* who, bool args_ok, const svr_ctx* c, const svr_frame* fr, svr_frame& f) {
    const std::string w(who);
    SVR_REQUIRE(args_ok, w + ": null argument");
    SVR_REQUIRE(c->material_set, w + ": svr_set_material has not been called");
    SVR_REQUIRE(fr->frame_w > 0 && fr->frame_h > 0 && fr->out_w > 0 && fr->out_h > 0, w + ": empty frame");
    SVR_REQUIRE(fr->x0 >= 0 && fr->y0 >= 0, w + ": negative tile origin");
    f = *fr;
    if (f.band_h <= 0) { f.band_h = fr->out_h; f.band_pitch = fr->out_h; }
    return SVR_OK;
}

// ... and what they end with: launch(s) on the caller's stream (NULL = default stream, as in svr_render), ordered like
// a render: behind the published uploads, and later uploads behind this draw (mark_render).  what: the launch as the
// error text of a failed one names it.
template <class Launch>
static int draw_ordered(svr_ctx* c, void* stream, const char* what, Launch&& launch) {
    DeviceGuard guard(c->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->have_published) SVR_HIP_TRY(hipStreamWaitEvent(s, c->uploads_published, 0));
    const hipError_t e = launch(s);
    if (e != hipSuccess) {
        svr_set_error(std::string(what) + ": " + hipGetErrorString(e));
        return SVR_ERR_HIP;
    }
    return mark_render(c, s);
}
// (the launch is named `s` in `call`; its text is the prefix of a failed launch's error, as SVR_HIP_TRY would form it)
#define SVR_DRAW_ORDERED(c, stream, call) draw_ordered(c, stream, #call, [&](hipStream_t s) { return call; })

// The context's mode state as one draw sees it: copied under the lock, so that the launch runs outside it.
struct ModeState { const float* table; int K, interp; CutState cut; };
static ModeState mode_state_of(svr_ctx* c) {
    svr_ctx_ext* x = svr_ext(c);
    std::lock_guard<std::mutex> lock(x->modes_mu);
    return ModeState{ x->tf_dev, x->tf_K, x->interp, x->cut };
}

// What svr_histogram and svr_objects check before and after their own checks (who: the entry point's name, the prefix
// of its error texts): the lod; then a box's shape, the id list, and lo, n: the intersection of box and window in the
// LOD's logical voxels.  In 64 bits (box_off + box_shape may pass 2^31); a window of None has shape 0 and holds
// nothing, so an n may be <= 0.
static int box_lod(const char* who, const svr_ctx* c, int lod) {
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, std::string(who) + ": lod out of range");
    return SVR_OK;
}
static int box_window(const char* who, const svr_ctx* c, int lod, int use_box, const int32_t box_off[3], const int32_t box_shape[3],
                      const uint32_t* selected, uint32_t selected_count, int64_t lo[3], int64_t n[3]) {
    if (use_box)
        for (int a = 0; a < 3; ++a) SVR_REQUIRE(box_shape[a] >= 0, std::string(who) + ": negative box_shape");
    SVR_REQUIRE(selected_count == 0 || selected, std::string(who) + ": selected_count > 0 with a NULL selected pointer");
    const svr_lod_state& st = c->lod[lod].state;
    for (int a = 0; a < 3; ++a) {
        int64_t b = st.offset[a], e = (int64_t)st.offset[a] + st.shape[a];
        if (use_box) {
            b = std::max<int64_t>(b, box_off[a]);
            e = std::min<int64_t>(e, (int64_t)box_off[a] + box_shape[a]);
        }
        lo[a] = b; n[a] = e - b;
    }
    return SVR_OK;
}

// What svr_mesh, svr_components, svr_distance, svr_nearest and svr_split end with (who: the entry point, the prefix of the error text; what:
// the launch as draw_ordered names it): launch(scratch, s) as draw_ordered runs it, in the pass's scratch (ScratchSlot)
// grown to `bytes` (0: an empty box needs none), behind the pass's call before it.  Under the slot's lock throughout.
template <class Launch>
static int scratch_ordered(svr_ctx* c, ScratchSlot& slot, uint64_t bytes, void* stream, const char* who, const char* what, Launch&& launch) {
    std::lock_guard<std::mutex> lock(slot.mu);
    {
        DeviceGuard guard(c->device);
        if (!slot.done) SVR_HIP_TRY(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
        if (bytes > slot.bytes) {
            // the call that may still be working in the old scratch ends first
            if (slot.pending) SVR_HIP_TRY(hipEventSynchronize(slot.done));
            if (slot.mem) (void)hipFree(slot.mem);
            slot.mem = nullptr; slot.bytes = 0;
            if (hipMalloc(&slot.mem, (size_t)bytes) != hipSuccess) {
                slot.mem = nullptr;
                (void)hipGetLastError();
                svr_set_error(std::string(who) + ": out of device memory for the scratch of " + std::to_string(bytes) + " bytes");
                return SVR_ERR_NOMEM;
            }
            slot.bytes = (size_t)bytes;
        }
    }
    return draw_ordered(c, stream, what, [&](hipStream_t s) {
        hipError_t e = slot.pending ? hipStreamWaitEvent(s, slot.done, 0) : hipSuccess;
        if (e != hipSuccess) return e;
        e = launch(slot.mem, s);
        // recorded behind whatever was enqueued, a failed chain's kernels too: the next call waits for them
        const hipError_t r = hipEventRecord(slot.done, s);
        if (r == hipSuccess) slot.pending = true;
        return e != hipSuccess ? e : r;
    });
}

extern "C" {

int svr_slice(svr_ctx* c, const svr_slice_plane* plane, const svr_frame* fr, const svr_slice_outputs* out, void* stream) {
    svr_frame f;
    { const int rc = draw_prologue("svr_slice", c && plane && fr && out && out->rgba, c, fr, f); if (rc) return rc; }
    for (int a = 0; a < 3; ++a) {
        SVR_REQUIRE(plane->volume_dimensions[a] >= 1.0f, "svr_slice: volume_dimensions must be >= 1");
        SVR_REQUIRE(isfinite(plane->origin[a]) && isfinite(plane->u[a]) && isfinite(plane->v[a]),
                    "svr_slice: origin, u and v must be finite");
    }
    SVR_REQUIRE((uintptr_t)out->rgba % 16 == 0, "svr_slice: rgba must be 16-byte aligned");
    const int twin_mode = (c->variant & 256) ? 0 : ((c->variant & 512) ? 2 : 1);
    const int interp = mode_state_of(c).interp;
    return SVR_DRAW_ORDERED(c, stream, svr_launch_slice(c, *plane, f, *out, twin_mode, interp, s));
}

int svr_slab(svr_ctx* c, const svr_slab_params* sp, const svr_frame* fr, const svr_slice_outputs* out, void* stream) {
    svr_frame f;
    { const int rc = draw_prologue("svr_slab", c && sp && fr && out && out->rgba, c, fr, f); if (rc) return rc; }
    const svr_slice_plane& plane = sp->plane;
    for (int a = 0; a < 3; ++a) {
        SVR_REQUIRE(plane.volume_dimensions[a] >= 1.0f, "svr_slab: volume_dimensions must be >= 1");
        SVR_REQUIRE(isfinite(plane.origin[a]) && isfinite(plane.u[a]) && isfinite(plane.v[a]),
                    "svr_slab: origin, u and v must be finite");
        SVR_REQUIRE(isfinite(sp->w[a]), "svr_slab: w must be finite");
    }
    SVR_REQUIRE(isfinite(sp->w_len) && sp->w_len >= 0.0f, "svr_slab: w_len must be finite and >= 0");
    SVR_REQUIRE(sp->samples >= 1 && sp->samples <= SVR_SLAB_MAX_SAMPLES, "svr_slab: samples must be in 1 .. 4096");
    SVR_REQUIRE(sp->mode == SVR_SLAB_MAX || sp->mode == SVR_SLAB_MIN || sp->mode == SVR_SLAB_MEAN,
                "svr_slab: unknown mode");
    // the data-space sample step (include/svr.h), as the slice launcher forms du / dv: an overflow to inf would make
    // 0 * dw NaN and break the N = 1 identity with svr_slice
    float dw[3];
    const float* m = plane.world_inv;
    for (int k = 0; k < 3; ++k) {
        dw[k] = (m[k] * sp->w[0] + m[4 + k] * sp->w[1]) + m[8 + k] * sp->w[2];
        SVR_REQUIRE(isfinite(dw[k]), "svr_slab: the data-space step of w must be finite");
    }
    SVR_REQUIRE((uintptr_t)out->rgba % 16 == 0, "svr_slab: rgba must be 16-byte aligned");
    const int twin_mode = (c->variant & 256) ? 0 : ((c->variant & 512) ? 2 : 1);
    const int interp = mode_state_of(c).interp;
    return SVR_DRAW_ORDERED(c, stream, svr_launch_slab(c, *sp, dw, f, *out, twin_mode, interp, s));
}

int svr_histogram(svr_ctx* c, const svr_histogram_params* hp, const svr_histogram_outputs* out, void* stream) {
    SVR_REQUIRE(c && hp && out && out->counts, "svr_histogram: null argument");
    { const int rc = box_lod("svr_histogram", c, hp->lod); if (rc) return rc; }
    SVR_REQUIRE(hp->bins >= 1 && hp->bins <= SVR_HIST_MAX_BINS, "svr_histogram: bins must be in 1 .. 4096");
    SVR_REQUIRE(isfinite(hp->lo) && isfinite(hp->hi) && hp->lo < hp->hi, "svr_histogram: lo and hi must be finite, lo < hi");
    const float inv = (float)hp->bins / (hp->hi - hp->lo);
    SVR_REQUIRE(isfinite(inv), "svr_histogram: bins / (hi - lo) is not finite in f32");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_histogram", c, hp->lod, hp->use_box, hp->box_off, hp->box_shape, hp->selected, hp->selected_count, lo, n); if (rc) return rc; }
    const int lod = hp->lod, K = hp->bins;
    const float flo = hp->lo, fhi = hp->hi;
    const uint32_t* sel = hp->selected; const uint32_t nsel = hp->selected_count;
    return SVR_DRAW_ORDERED(c, stream, svr_launch_histogram(c, lod, lo, n, flo, fhi, inv, K, sel, nsel, *out, s));
}

int svr_objects(svr_ctx* c, const svr_objects_params* op, const svr_objects_outputs* out, void* stream) {
    SVR_REQUIRE(c && op && out && out->records && out->header, "svr_objects: null argument");
    { const int rc = box_lod("svr_objects", c, op->lod); if (rc) return rc; }
    SVR_REQUIRE(op->capacity >= 1 && op->capacity <= SVR_OBJECTS_MAX_CAPACITY, "svr_objects: capacity must be in 1 .. 2^26");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_objects", c, op->lod, op->use_box, op->box_off, op->box_shape, op->selected, op->selected_count, lo, n); if (rc) return rc; }
    const int lod = op->lod, ignore_zero = op->ignore_zero;
    const uint32_t* sel = op->selected; const uint32_t nsel = op->selected_count, capacity = op->capacity;
    return SVR_DRAW_ORDERED(c, stream, svr_launch_objects(c, lod, lo, n, sel, nsel, ignore_zero, capacity, *out, s));
}

int svr_contacts(svr_ctx* c, const svr_contacts_params* cp, const svr_contacts_outputs* out, void* stream) {
    SVR_REQUIRE(c && cp && out && out->records && out->header, "svr_contacts: null argument");
    { const int rc = box_lod("svr_contacts", c, cp->lod); if (rc) return rc; }
    SVR_REQUIRE(cp->capacity >= 1 && cp->capacity <= SVR_CONTACTS_MAX_CAPACITY, "svr_contacts: capacity must be in 1 .. 2^26");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_contacts", c, cp->lod, cp->use_box, cp->box_off, cp->box_shape, cp->selected, cp->selected_count, lo, n); if (rc) return rc; }
    const int lod = cp->lod, ignore_zero = cp->ignore_zero;
    const uint32_t* sel = cp->selected; const uint32_t nsel = cp->selected_count, capacity = cp->capacity;
    return SVR_DRAW_ORDERED(c, stream, svr_launch_contacts(c, lod, lo, n, sel, nsel, ignore_zero, capacity, *out, s));
}

int svr_mesh(svr_ctx* c, const svr_mesh_params* mp, const svr_mesh_outputs* out, void* stream) {
    SVR_REQUIRE(c && mp && out && out->header, "svr_mesh: null argument");
    { const int rc = box_lod("svr_mesh", c, mp->lod); if (rc) return rc; }
    SVR_REQUIRE(mp->mode == SVR_MESH_LABELS || mp->mode == SVR_MESH_LEVEL, "svr_mesh: unknown mode");
    const bool labels = mp->mode == SVR_MESH_LABELS;
    if (labels) SVR_REQUIRE(mp->selected_count >= 1 && mp->selected, "svr_mesh: SVR_MESH_LABELS needs at least one selected id");
    else        SVR_REQUIRE(mp->level == mp->level, "svr_mesh: level must not be NaN");
    SVR_REQUIRE(out->vertices || out->vertex_capacity == 0, "svr_mesh: NULL vertices with a non-zero vertex_capacity");
    SVR_REQUIRE(out->triangles || out->triangle_capacity == 0, "svr_mesh: NULL triangles with a non-zero triangle_capacity");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_mesh", c, mp->lod, mp->use_box, mp->box_off, mp->box_shape, nullptr, 0, lo, n); if (rc) return rc; }
    MeshPlan plan;
    bool too_many = false;
    const bool any = mesh_plan(n, n[0] > 0 ? box_head(lo[0], (uint32_t)c->lod[mp->lod].ring[0]) : 0u, plan, &too_many);
    SVR_REQUIRE(!too_many, "svr_mesh: more than SVR_MESH_MAX_CELLS cells");

    const uint32_t* sel = labels ? mp->selected : nullptr; const uint32_t nsel = labels ? mp->selected_count : 0u;
    return scratch_ordered(c, svr_ext(c)->mesh, any ? plan.bytes : 0u, stream, "svr_mesh", "svr_launch_mesh", [&](void* scratch, hipStream_t s) {
        return svr_launch_mesh(c, mp->lod, lo, any ? &plan : nullptr, mp->mode, mp->level, sel, nsel, scratch, *out, s);
    });
}

int svr_components(svr_ctx* c, const svr_components_params* cp, const svr_components_outputs* out, void* stream) {
    SVR_REQUIRE(c && cp && out && out->header, "svr_components: null argument");
    { const int rc = box_lod("svr_components", c, cp->lod); if (rc) return rc; }
    SVR_REQUIRE(cp->mode == SVR_COMPONENTS_LABELS || cp->mode == SVR_COMPONENTS_LEVEL, "svr_components: unknown mode");
    SVR_REQUIRE(cp->connectivity == 6 || cp->connectivity == 26, "svr_components: connectivity must be 6 or 26");
    if (cp->mode == SVR_COMPONENTS_LEVEL) SVR_REQUIRE(cp->level == cp->level, "svr_components: level must not be NaN");
    SVR_REQUIRE(out->ids || out->ids_capacity == 0, "svr_components: NULL ids with a non-zero ids_capacity");
    SVR_REQUIRE(out->records || out->record_capacity == 0, "svr_components: NULL records with a non-zero record_capacity");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_components", c, cp->lod, cp->use_box, cp->box_off, cp->box_shape, cp->selected, cp->selected_count, lo, n); if (rc) return rc; }
    CompPlan plan;
    bool too_many = false;
    const bool any = comp_plan(n, n[0] > 0 ? box_head(lo[0], (uint32_t)c->lod[cp->lod].ring[0]) : 0u, plan, &too_many);
    SVR_REQUIRE(!too_many, "svr_components: more than SVR_COMPONENTS_MAX_VOXELS voxels");

    return scratch_ordered(c, svr_ext(c)->comp, any ? plan.bytes : 0u, stream, "svr_components", "svr_launch_components", [&](void* scratch, hipStream_t s) {
        return svr_launch_components(c, cp->lod, lo, any ? &plan : nullptr, *cp, scratch, *out, s);
    });
}

int svr_distance(svr_ctx* c, const svr_distance_params* dp, const svr_distance_outputs* out, void* stream) {
    SVR_REQUIRE(c && dp && out && out->header, "svr_distance: null argument");
    { const int rc = box_lod("svr_distance", c, dp->lod); if (rc) return rc; }
    SVR_REQUIRE(dp->mode == SVR_COMPONENTS_LABELS || dp->mode == SVR_COMPONENTS_LEVEL, "svr_distance: unknown mode");
    if (dp->mode == SVR_COMPONENTS_LEVEL) SVR_REQUIRE(dp->level == dp->level, "svr_distance: level must not be NaN");
    SVR_REQUIRE(out->d2 || out->d2_capacity == 0, "svr_distance: NULL d2 with a non-zero d2_capacity");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_distance", c, dp->lod, dp->use_box, dp->box_off, dp->box_shape, dp->selected, dp->selected_count, lo, n); if (rc) return rc; }
    DistPlan plan;
    int refused = 0;
    const bool any = dist_plan(n, n[0] > 0 ? box_head(lo[0], (uint32_t)c->lod[dp->lod].ring[0]) : 0u, plan, &refused);
    SVR_REQUIRE(refused != 1, "svr_distance: an extent of more than SVR_DISTANCE_MAX_EXTENT voxels");
    SVR_REQUIRE(refused != 2, "svr_distance: more than SVR_DISTANCE_MAX_VOXELS voxels");

    // the count-only call works in the bits alone, but sizes the scratch for the call that follows it
    return scratch_ordered(c, svr_ext(c)->dist, any ? plan.bytes : 0u, stream, "svr_distance", "svr_launch_distance", [&](void* scratch, hipStream_t s) {
        return svr_launch_distance(c, dp->lod, lo, any ? &plan : nullptr, *dp, scratch, *out, s);
    });
}

int svr_nearest(svr_ctx* c, const svr_nearest_params* np, const svr_nearest_outputs* out, void* stream) {
    SVR_REQUIRE(c && np && out && out->header, "svr_nearest: null argument");
    { const int rc = box_lod("svr_nearest", c, np->lod); if (rc) return rc; }
    SVR_REQUIRE(np->mode == SVR_COMPONENTS_LABELS || np->mode == SVR_COMPONENTS_LEVEL, "svr_nearest: unknown mode");
    if (np->mode == SVR_COMPONENTS_LEVEL) SVR_REQUIRE(np->level == np->level, "svr_nearest: level must not be NaN");
    SVR_REQUIRE(out->d2 || out->capacity == 0, "svr_nearest: NULL d2 with a non-zero capacity");
    SVR_REQUIRE(out->index || out->capacity == 0, "svr_nearest: NULL index with a non-zero capacity");
    int64_t lo[3], n[3];
    { const int rc = box_window("svr_nearest", c, np->lod, np->use_box, np->box_off, np->box_shape, np->selected, np->selected_count, lo, n); if (rc) return rc; }
    NearPlan plan;
    int refused = 0;
    const bool any = near_plan(n, n[0] > 0 ? box_head(lo[0], (uint32_t)c->lod[np->lod].ring[0]) : 0u, plan, &refused);
    SVR_REQUIRE(refused != 1, "svr_nearest: an extent of more than SVR_DISTANCE_MAX_EXTENT voxels");
    SVR_REQUIRE(refused != 2, "svr_nearest: more than SVR_DISTANCE_MAX_VOXELS voxels");

    // svr_distance's slot: the two are ordered behind one another
    return scratch_ordered(c, svr_ext(c)->dist, any ? plan.bytes : 0u, stream, "svr_nearest", "svr_launch_nearest", [&](void* scratch, hipStream_t s) {
        return svr_launch_nearest(c, np->lod, lo, any ? &plan : nullptr, *np, scratch, *out, s);
    });
}

int svr_split(svr_ctx* c, const svr_split_params* sp, const svr_split_outputs* out, void* stream) {
    SVR_REQUIRE(c && sp && out && out->header && sp->height, "svr_split: null argument");
    SVR_REQUIRE(sp->connectivity == 6 || sp->connectivity == 26, "svr_split: connectivity must be 6 or 26");
    SVR_REQUIRE(sp->merge_squared <= SVR_SPLIT_MAX_MERGE, "svr_split: merge_squared above SVR_SPLIT_MAX_MERGE");
    SVR_REQUIRE(sp->n[0] > 0 && sp->n[1] > 0 && sp->n[2] > 0, "svr_split: every extent must be > 0");
    SVR_REQUIRE(out->ids || out->ids_capacity == 0, "svr_split: NULL ids with a non-zero ids_capacity");
    SVR_REQUIRE(out->records || out->record_capacity == 0, "svr_split: NULL records with a non-zero record_capacity");
    SplitPlan plan;
    SVR_REQUIRE(split_plan(sp->n, plan), "svr_split: more than SVR_SPLIT_MAX_VOXELS voxels");

    // no ring is read; scratch_ordered orders the call like a draw all the same, which costs a wait that has long passed
    return scratch_ordered(c, svr_ext(c)->split, plan.bytes, stream, "svr_split", "svr_launch_split", [&](void* scratch, hipStream_t s) {
        return svr_launch_split(plan, *sp, scratch, *out, s);
    });
}

int svr_set_transfer_function(svr_ctx* c, const float* rgba, int32_t K) {
    SVR_REQUIRE(c && rgba, "svr_set_transfer_function: null argument");
    SVR_REQUIRE(K >= 2 && K <= SVR_TF_MAX_ENTRIES, "svr_set_transfer_function: K must be in 2 .. 4096");
    for (int32_t k = 0; k < 4 * K; ++k)
        SVR_REQUIRE(rgba[k] >= 0.0f && rgba[k] <= 1.0f, "svr_set_transfer_function: every entry must be finite and in [0, 1]");
    DeviceGuard guard(c->device);
    float* fresh = nullptr;
    if (hipMalloc((void**)&fresh, (size_t)K * 4 * sizeof(float)) != hipSuccess) {
        svr_set_error("svr_set_transfer_function: out of device memory"); return SVR_ERR_NOMEM;
    }
    if (hipMemcpy(fresh, rgba, (size_t)K * 4 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(fresh);
        svr_set_error("svr_set_transfer_function: hipMemcpy failed"); return SVR_ERR_HIP;
    }
    svr_ctx_ext* x = svr_ext(c);
    std::lock_guard<std::mutex> lock(x->modes_mu);
    if (x->tf_dev) x->tf_retired.push_back(x->tf_dev);   // composites still in flight keep reading the old table
    if (x->tf_retired.size() > 32) {                     // bounded: drain once in a long while
        SVR_HIP_TRY(hipDeviceSynchronize());
        for (float* p : x->tf_retired) (void)hipFree(p);
        x->tf_retired.clear();
    }
    x->tf_dev = fresh;
    x->tf_K = K;
    return SVR_OK;
}

int svr_set_interpolation(svr_ctx* c, int mode) {
    SVR_REQUIRE(c, "svr_set_interpolation: null ctx");
    SVR_REQUIRE(mode == SVR_INTERP_NEAREST || mode == SVR_INTERP_LINEAR,
                "svr_set_interpolation: mode must be SVR_INTERP_NEAREST or SVR_INTERP_LINEAR");
    svr_ctx_ext* x = svr_ext(c);
    std::lock_guard<std::mutex> lock(x->modes_mu);
    x->interp = mode;
    return SVR_OK;
}

int svr_set_cut_planes(svr_ctx* c, const float* planes, uint32_t count, int mode) {
    SVR_REQUIRE(c, "svr_set_cut_planes: null ctx");
    SVR_REQUIRE(count <= SVR_MAX_CUT_PLANES, "svr_set_cut_planes: at most SVR_MAX_CUT_PLANES planes");
    SVR_REQUIRE(planes || count == 0, "svr_set_cut_planes: null planes with a non-zero count");
    SVR_REQUIRE(mode == SVR_CUT_ANY || mode == SVR_CUT_ALL, "svr_set_cut_planes: mode must be SVR_CUT_ANY or SVR_CUT_ALL");
    CutState fresh{};
    fresh.count = count; fresh.mode = mode;
    for (uint32_t k = 0; k < count; ++k) {
        const float* p = planes + 4 * k;
        for (int a = 0; a < 4; ++a) {
            SVR_REQUIRE(fabsf(p[a]) < INFINITY, "svr_set_cut_planes: every component must be finite");
            fresh.planes[k][a] = p[a];
        }
        const float len = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
        SVR_REQUIRE(len > 0.0f && len < INFINITY, "svr_set_cut_planes: a plane's normal must have a finite, non-zero length");
    }
    svr_ctx_ext* x = svr_ext(c);
    std::lock_guard<std::mutex> lock(x->modes_mu);
    x->cut = fresh;
    return SVR_OK;
}

int svr_composite(svr_ctx* c, const svr_camera* cam, const svr_frame* fr, const svr_composite_params* cp,
                  const svr_outputs* out, void* stream) {
    svr_frame f;
    { const int rc = draw_prologue("svr_composite", c && cam && fr && cp && out && out->rgba, c, fr, f); if (rc) return rc; }
    for (int a = 0; a < 3; ++a)
        SVR_REQUIRE(cam->volume_dimensions[a] >= 1.0f, "svr_composite: volume_dimensions must be >= 1");
    SVR_REQUIRE(cp->alpha_cutoff > 0.0f && cp->alpha_cutoff <= 1.0f, "svr_composite: alpha_cutoff must be in (0, 1]");
    const ModeState st = mode_state_of(c);
    SVR_REQUIRE(st.table, "svr_composite: svr_set_transfer_function has not been called");
    return SVR_DRAW_ORDERED(c, stream, svr_launch_composite(c, *cam, f, *cp, *out, st.table, st.K, st.interp, &st.cut.planes[0][0],
                                                            st.cut.count, st.cut.mode, s));
}

int svr_iso(svr_ctx* c, const svr_camera* cam, const svr_frame* fr, const svr_iso_params* ip, const svr_outputs* out,
            void* stream) {
    svr_frame f;
    { const int rc = draw_prologue("svr_iso", c && cam && fr && ip && out && out->rgba, c, fr, f); if (rc) return rc; }
    for (int a = 0; a < 3; ++a)
        SVR_REQUIRE(cam->volume_dimensions[a] >= 1.0f, "svr_iso: volume_dimensions must be >= 1");
    SVR_REQUIRE(ip->iso_value == ip->iso_value, "svr_iso: iso_value must not be NaN");
    SVR_REQUIRE(ip->refine >= 0 && ip->refine <= SVR_ISO_MAX_REFINE, "svr_iso: refine must be in 0 .. 16");
    SVR_REQUIRE(ip->shininess_log2 >= 0 && ip->shininess_log2 <= SVR_ISO_MAX_SHININESS_LOG2,
                "svr_iso: shininess_log2 must be in 0 .. 10");
    SVR_REQUIRE(ip->ambient >= 0.0f && ip->ambient < INFINITY && ip->diffuse >= 0.0f && ip->diffuse < INFINITY &&
                ip->specular >= 0.0f && ip->specular < INFINITY,
                "svr_iso: ambient, diffuse and specular must be finite and >= 0");
    for (int a = 0; a < 3; ++a)
        SVR_REQUIRE(ip->iso_color[a] >= 0.0f && ip->iso_color[a] <= 1.0f, "svr_iso: iso_color must be in [0, 1]");
    if (!ip->headlight) {
        const float* d = ip->light_direction;
        const float len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        SVR_REQUIRE(fabsf(sqrtf(len2) - 1.0f) <= 1e-3f, "svr_iso: light_direction must be finite and of unit length");
    }
    const ModeState st = mode_state_of(c);
    return SVR_DRAW_ORDERED(c, stream, svr_launch_iso(c, *cam, f, *ip, *out, st.interp, &st.cut.planes[0][0],
                                                      st.cut.count, st.cut.mode, s));
}

}  // extern "C"
