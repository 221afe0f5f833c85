// What the host units of the C ABI (svr_api.hip, svr_upload.hip, svr_render.hip, svr_modes.hip) share with one another
// and with the kernel units whose launchers they call.  Kept apart from svr_internal.h, whose bytes are part of the
// kernel-source stamp bench.py checks its traffic profile against.
#pragma once

#include <mutex>
#include <string>
#include <vector>

#include "svr_internal.h"

#define SVR_REQUIRE(cond, msg)                    \
    do {                                          \
        if (!(cond)) {                            \
            svr_set_error(msg);                   \
            return SVR_ERR_INVALID;               \
        }                                         \
    } while (0)

// launchers of the kernel units, which include this header too --------------------------------------------------------
// compose_kernels.hip
hipError_t svr_launch_outline(const float* rgba, const float* depth, const uint32_t* label, const uint8_t* flags, int w,
                              int h, const svr_outline_params& q, const float* colors, uint32_t ncolors,
                              const uint32_t* sel, uint32_t nsel, float* out, uint8_t* mask, hipStream_t stream);
// slice_kernels.hip.  twin_mode: 0 rows only, 1 per LOD the layout with fewer lines per wave, 2 the copy.
hipError_t svr_launch_slice(const svr_ctx* c, const svr_slice_plane& pl, const svr_frame& fr, const svr_slice_outputs& out,
                            int twin_mode, int interp, hipStream_t stream);
// slice_kernels.hip.  dw: the data-space sample step, computed and checked by svr_slab.
hipError_t svr_launch_slab(const svr_ctx* c, const svr_slab_params& sp, const float dw[3], const svr_frame& fr,
                           const svr_slice_outputs& out, int twin_mode, int interp, hipStream_t stream);
// composite_kernels.hip.  table: the device copy of the transfer function, K entries of RGBA.
hipError_t svr_launch_composite(const svr_ctx* c, const svr_camera& cam, const svr_frame& fr,
                                const svr_composite_params& cp, const svr_outputs& out, const float* table, int K,
                                int interp, const float* cut_planes, uint32_t cut_count, int cut_mode,
                                hipStream_t stream);
// iso_kernels.hip.  cut_planes: cut_count x abcd of svr_set_cut_planes (host), cut_mode: SVR_CUT_*.
hipError_t svr_launch_iso(const svr_ctx* c, const svr_camera& cam, const svr_frame& fr, const svr_iso_params& ip,
                          const svr_outputs& out, int interp, const float* cut_planes, uint32_t cut_count, int cut_mode,
                          hipStream_t stream);
// histogram_kernels.hip.  lo, n: box and window intersected, in the LOD's logical voxels (an n <= 0: nothing
// to count); inv = (float)K / (hi - lo); everything checked by svr_histogram.
hipError_t svr_launch_histogram(const svr_ctx* c, int lod, const int64_t lo[3], const int64_t n[3], float flo, float fhi,
                                float inv, int K, const uint32_t* sel, uint32_t nsel, const svr_histogram_outputs& out,
                                hipStream_t stream);
// object_kernels.hip.  lo, n as above; everything checked by svr_objects.
hipError_t svr_launch_objects(const svr_ctx* c, int lod, const int64_t lo[3], const int64_t n[3], const uint32_t* sel, uint32_t nsel,
                              int ignore_zero, uint32_t capacity, const svr_objects_outputs& out, hipStream_t stream);
// contacts_kernels.hip.  lo, n as above; everything checked by svr_contacts.
hipError_t svr_launch_contacts(const svr_ctx* c, int lod, const int64_t lo[3], const int64_t n[3], const uint32_t* sel, uint32_t nsel,
                               int ignore_zero, uint32_t capacity, const svr_contacts_outputs& out, hipStream_t stream);
// mesh_kernels.hip.  lo: the first voxel of box and window intersected; plan: mesh_plan (mesh_plan.h) of its extent, null
// for an empty box; scratch: plan->bytes of the context's mesh scratch; everything checked by svr_mesh.
struct MeshPlan;
hipError_t svr_launch_mesh(const svr_ctx* c, int lod, const int64_t lo[3], const MeshPlan* plan, int mode, float level,
                           const uint32_t* sel, uint32_t nsel, void* scratch, const svr_mesh_outputs& out, hipStream_t stream);
// components_kernels.hip.  lo as for the mesh; plan: comp_plan (components_plan.h) of the box's extent, null for an empty
// box; scratch: plan->bytes of the context's components scratch; everything checked by svr_components.
struct CompPlan;
hipError_t svr_launch_components(const svr_ctx* c, int lod, const int64_t lo[3], const CompPlan* plan, const svr_components_params& cp,
                                 void* scratch, const svr_components_outputs& out, hipStream_t stream);
// distance_kernels.hip.  lo as for the mesh; plan: dist_plan (distance_plan.h) of the box's extent, null for an empty box;
// scratch: plan->bytes of the context's distance scratch; everything checked by svr_distance.
struct DistPlan;
hipError_t svr_launch_distance(const svr_ctx* c, int lod, const int64_t lo[3], const DistPlan* plan, const svr_distance_params& dp,
                               void* scratch, const svr_distance_outputs& out, hipStream_t stream);
// The same unit.  plan: near_plan (distance_plan.h), null for an empty box; scratch: plan->bytes of the same scratch;
// everything checked by svr_nearest.
struct NearPlan;
hipError_t svr_launch_nearest(const svr_ctx* c, int lod, const int64_t lo[3], const NearPlan* plan, const svr_nearest_params& np,
                              void* scratch, const svr_nearest_outputs& out, hipStream_t stream);
// split_kernels.hip.  plan: split_plan (split_plan.h) of sp.n; scratch: plan.bytes of the context's split scratch;
// everything checked by svr_split.  No ring is read, so there is no context among the arguments.
struct SplitPlan;
hipError_t svr_launch_split(const SplitPlan& plan, const svr_split_params& sp, void* scratch, const svr_split_outputs& out,
                            hipStream_t stream);

// the context as svr_create really allocates it ------------------------------------------------------------------------
// The state of svr_set_transfer_function, svr_set_interpolation and svr_set_cut_planes (svr_modes.hip).  Like the colour
// table of svr_set_material, every new transfer function goes into a fresh device buffer; the replaced ones are freed
// once the device has drained (or with the context).  A context starts with no table (tf_dev null),
// SVR_INTERP_NEAREST and no planes.
struct CutState {
    uint32_t count;
    int mode;
    float planes[SVR_MAX_CUT_PLANES][4];
};
// The scratch the kernels of one box pass work in (svr_modes.hip: scratch_ordered), grown on demand and shared by every
// call of that pass, so a call waits for the one before (done, recorded behind its last kernel) whatever its stream.
struct ScratchSlot {
    std::mutex mu;                         // one call at a time sizes the scratch and enqueues
    void* mem = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool pending = false;                  // done has been recorded
    void release() { if (mem) (void)hipFree(mem); if (done) (void)hipEventDestroy(done); }     // svr_destroy's
};
struct svr_ctx_ext : svr_ctx {
    std::mutex modes_mu;                   // setters write under it; a draw copies what it needs under it and launches outside
    float* tf_dev = nullptr;
    int tf_K = 0;
    std::vector<float*> tf_retired;
    int interp = SVR_INTERP_NEAREST;
    CutState cut = {};
    ScratchSlot mesh, comp, dist, split;   // of svr_mesh, svr_components, svr_distance (and svr_nearest) and svr_split
};
// (every svr_ctx* of the ABI comes from svr_create)
inline svr_ctx_ext* svr_ext(svr_ctx* c) { return static_cast<svr_ctx_ext*>(c); }

// helpers of more than one unit (svr_api.hip) ---------------------------------------------------------------------------
// off, shape inside LOD lod's ring?  who: the entry point's name, the prefix of the error texts.
int check_region(svr_ctx* c, int lod, const int32_t off[3], const int32_t shape[3], const char* who);
// Before an upload's first enqueue: order the upload stream behind every render still in flight ...
int uploads_after_render(svr_ctx* c);
// ... which every draw that reads the rings registers, right behind its launch on stream s.
int mark_render(svr_ctx* c, hipStream_t s);
