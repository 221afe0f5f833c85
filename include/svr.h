/*
 * svr.h — C ABI of the MI355X-native sub-volume LMIP ray-march renderer.
 *
 * The reference (gyoge0/sub_volume_renderer) has no FFI boundary of its own:
 * its hot path sits behind pygfx's plugin hooks — uniform buffers, texture
 * bindings and a WGSL fragment shader (src/sub_volume/_shader.py:75-127).
 * This header is the C-ABI replacement of exactly those hooks.  Every entry
 * point cites the reference interface it replaces.  All vectors at this
 * boundary are in SHADER ORDER (x, y, z) = reversed numpy order, exactly as
 * the reference writes them into its uniform buffers
 * (_wrapping_buffer.py:84-96,113-115; _wobject.py:121-123).  Ring memory is
 * C-contiguous [z][y][x] (texel (x,y,z) == numpy data[z,y,x], KNOWLEDGE.md:81-133).
 *
 * Plain pointers and sizes only; no torch / HIP types in any signature
 * (streams travel as void*).  Every function returns 0 on success and a
 * negative svr_status on failure; svr_last_error() gives the message.
 *
 * Threads.  A context has ONE render thread: svr_set_lod_state, svr_set_material, svr_set_variant, svr_render,
 * svr_time_render, svr_gather_tiles and the svr_comm_* calls of one context must not run concurrently with one
 * another (renders may go to different HIP streams, one after the other).  svr_upload_region / _device,
 * svr_upload_ticket, svr_ticket_pending, svr_mark_uploads and svr_uploads_pending may be called from ONE other
 * thread at the same time (the streaming worker): uploads of a context are serialised by a mutex, and they are
 * ordered on the device behind every render still in flight.  Different contexts are independent.
 * svr_last_error() is per thread.
 */
#ifndef SVR_H
#define SVR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_MAX_LODS 8
#define SVR_MAX_CLIP_PLANES 8
#define SVR_ABI_VERSION 9

typedef enum svr_status {
    SVR_OK = 0,
    SVR_ERR_INVALID = -1,   /* bad argument (maps to ValueError in the Python mirror) */
    SVR_ERR_HIP = -2,       /* a HIP runtime call failed */
    SVR_ERR_NOMEM = -3,     /* device or pinned allocation failed */
    SVR_ERR_RANGE = -4      /* region outside the ring / frame */
} svr_status;

/* element types accepted for source arrays (np.array(src, dtype=f32/u32) in
 * _wrapping_buffer.py:325,330 accepts anything numpy can cast) */
typedef enum svr_dtype {
    SVR_U8 = 0, SVR_U16 = 1, SVR_U32 = 2, SVR_U64 = 3,
    SVR_I8 = 4, SVR_I16 = 5, SVR_I32 = 6, SVR_I64 = 7,
    SVR_F32 = 8, SVR_F64 = 9
} svr_dtype;

/* One LOD's ring buffer = the two gfx.Texture objects of a WrappingBuffer
 * (_wrapping_buffer.py:50-59): r32float density + r32uint labels, both of
 * extent ring_dims (shader order), zero-initialised. */
typedef struct svr_lod_desc {
    int32_t ring_dims[3];          /* (x, y, z) voxels = reversed shape_in_pixels */
    int32_t density_storage;       /* SVR_F32: the reference's r32float texture.  SVR_U8 / SVR_U16: store
                                      the density ring in the sources' own integer type — allowed only when
                                      every upload's source has that dtype, so that texel values (exact in
                                      f32) and therefore all results are identical; 4x / 2x less HBM / L2 /
                                      LDS per voxel.  All LODs of a context use the same storage. */
    int32_t no_labels;             /* 1: the volume has no segmentation (FUTURE.md:178-193 "make this optional"): no label
                                      ring is allocated (4 of the 5 bytes per slot), uploads must pass labels = NULL,
                                      every hit gets label 0 (-> colors[0], like unlabelled voxels: FUTURE.md:170-176).
                                      All LODs of a context alike. */
    int32_t blocked_twin;          /* 1 or 2: keep a SECOND copy of this LOD's density ring, laid out in 128-byte micro-blocks that
                                      are compact in 3-D (8 x 4 x 4 one-byte voxels, 4 x 4 x 4 two-byte, 4 x 4 x 2 four-byte;
                                      blocks in [bz][by][bx] order) — the locality a texture unit's tiled 3-D layout gives the
                                      reference's textureLoad (sample_vol.wgsl:24).  Every upload writes both copies; the march
                                      reads the same texels from whichever copy suits a wave's view: waves whose gathers would
                                      touch many 128-byte ROWS per load (the per-wave probe that otherwise stages LDS bricks)
                                      gather from the micro-blocks — with 1 INSTEAD of staging bricks from the rows (what pays on
                                      the finest LOD), with 2 only where the wave stages none (the LOD cannot, or the wave's boxes
                                      stopped fitting its LDS region: what pays on the coarser LODs).  Costs one more density
                                      element per voxel of HBM and of upload traffic; results are identical.  The copies have an
                                      allocation of their own (they never push the rings over the 4 GiB below which one buffer
                                      resource reaches every LOD).  ring_dims must be multiples of (8, 4, 4), else SVR_ERR_INVALID.
                                      A ring of 4 GiB or more is reached through parts of whole z planes, and the copy through
                                      the same parts: the march uses the copy only where every part holds whole blocks (one
                                      part, or parts of a multiple of 4 planes for 1- and 2-byte voxels, of 2 for 4-byte), and
                                      otherwise reads that LOD's rows (planes of 1 GiB or more can give parts of 1 - 3 planes);
                                      results are the same.  svr_slice and svr_slab index the copy with 64-bit offsets and use
                                      it at any split.
                                      The Python mirror's "auto": 1 on the finest LOD; "all": also 2 on the others. */
} svr_lod_desc;

/* == u_wrapping_buffer_i uniform (_wrapping_buffer.py:15-19), shader order.
 * offset == shape == 0 means "ROI is None": nothing is in bounds (:90-96). */
typedef struct svr_lod_state {
    int32_t offset[3];             /* current_logical_offset_in_pixels */
    int32_t shape[3];              /* current_logical_shape_in_pixels  */
    float   scale[3];              /* scale_factor                     */
} svr_lod_state;

/* == u_material uniform (_material.py:6-24 + inherited VolumeMipMaterial
 * clim/gamma/opacity). colors is n x vec4 (h, s, v, pad) as the reference
 * pads it (_material.py:139-159). */
typedef struct svr_material {
    float    clim[2];
    float    gamma;
    float    opacity;
    float    lmip_threshold;
    float    lmip_fall_off;
    int32_t  lmip_max_samples;     /* i32 in the reference (_material.py:10-11) */
    float    fog_density;
    float    fog_color[3];
    uint32_t color_count;
    const float* colors;           /* host pointer, color_count * 4 floats */
    int32_t  colorspace_srgb;      /* 1: apply srgb2physical (raycast.wgsl:71-72; texture default) */
    /* Material.clipping_planes / clipping_mode of pygfx (the `pygfx.clipping_planes.wgsl` include at
     * fs_main.wgsl:8): world-space planes (a, b, c, d); the fragment — here: the whole ray, because the
     * tested position is the interpolated world position of the proxy box's BACK face (vs_main.wgsl:27) —
     * is discarded when dot(world_pos, abc) < d holds for ANY plane (clipping_mode_all = 0) or for ALL of
     * them (1).  No planes (the default): nothing is clipped.  pygfx text restated: assumption A6. */
    uint32_t clipping_plane_count; /* 0 .. SVR_MAX_CLIP_PLANES */
    int32_t  clipping_mode_all;
    const float* clipping_planes;  /* host pointer, clipping_plane_count * 4 floats (may be NULL when the count is 0) */
    /* Which raycast runs (FUTURE.md:111-120 "swappable rendering pipeline": a material-level switch).
     * SVR_MODE_LMIP: raycast.wgsl as it stands (MIP is LMIP with threshold -inf, fall-off 0 and no sample limit).
     * SVR_MODE_WEIGHTED_AVERAGE: the mode FUTURE.md:97-109 asks for and leaves without a formula; defined HERE
     * (oracle twin: oracle/lmip_oracle.c `raycast_weighted_average`) as
     *     d_i = f32(i) * |step|          distance of sample i from the ray's entry, in the units of the fog distance
     *     t_i = max(1 - weight_falloff * d_i, 0),  w_i = t_i * t_i
     *     value = (sum w_i * s_i) / (sum w_i)      over the samples of the ray, in order, f32
     * shown at the sample with the largest w_i * |s_i| (first one wins; it gives depth, label and fog distance);
     * nothing but zeros along the ray: a miss.  The ray ends at the first sample with t_i == 0.
     *
     * Signed and non-finite samples (float rings hold any f32; oracle/lmip_oracle.c, IEEE comparisons, decides):
     *   - the intensity of a sample s is |s|: a negative voxel counts by its magnitude and -inf counts as +inf;
     *     the value shown is s itself, sign included.
     *   - a NaN sample fails every comparison: it does not reach lmip_threshold (|s| >= threshold is false, also
     *     for threshold -inf, so under MIP too), it does not raise a running maximum (|s| > max is false) and it
     *     does not end a run through the fall-off test (|s| < max * lmip_fall_off is false); it still counts
     *     towards lmip_max_samples.  MIP therefore shows the first occurrence of the largest |s| among the ray's
     *     non-NaN samples, and a ray with no non-NaN sample is a MISS under LMIP and MIP alike.
     *   - -0.0 has intensity 0: it starts a run under a threshold <= 0 and is never replaced by +0.0 (strict >).
     *   - SVR_MODE_WEIGHTED_AVERAGE: num and den are plain f32 sums.  A NaN sample makes num, and so the value,
     *     NaN; +inf and -inf in one ray make num NaN, one of them alone makes the value that infinity; a sum of
     *     finite products that overflows is an infinity like any other.  The sample shown is the first with the
     *     largest w_i * |s_i| among those whose product is not NaN (a NaN product fails >); the ray is a HIT when
     *     that largest product is > 0, whatever the value.
     *   - shading takes the winning s through v = (s - clim[0]) / (clim[1] - clim[0]), powf(v, gamma),
     *     srgb2physical, hsv_to_rgb and the fog mix in that order with no clamp in between, so the colour of a
     *     negative, infinite or NaN s (or of an s - clim[0] that overflows) is whatever those operations give:
     *     powf of a negative base with a fractional gamma is NaN, an infinite v gives infinite or NaN channels
     *     (inf * 0 in hsv_to_rgb).  Label, depth and the pick word come from the sample's position and stay
     *     finite. */
    int32_t  render_mode;          /* svr_render_mode */
    float    weight_falloff;       /* >= 0; only read in SVR_MODE_WEIGHTED_AVERAGE */
} svr_material;

typedef enum svr_render_mode { SVR_MODE_LMIP = 0, SVR_MODE_WEIGHTED_AVERAGE = 1 } svr_render_mode;

/* == the six mat4 of u_stdinfo / u_wobject that the shaders read
 * (vs_main.wgsl:18-22, fs_main.wgsl:62-63) + u_wobject.volume_dimensions
 * (_wobject.py:14-17).  Matrices are COLUMN-MAJOR float[16] (m[c*4+r]) like
 * WGSL mat4x4<f32>. */
typedef struct svr_camera {
    float world[16];
    float world_inv[16];
    float cam[16];
    float cam_inv[16];
    float proj[16];
    float proj_inv[16];
    float volume_dimensions[3];    /* shader order (x, y, z) */
} svr_camera;

/* Which pixels of the full frame this call renders.  Output row r (0..out_h)
 * and column c (0..out_w) map to the frame pixel
 *     x = x0 + c
 *     y = y0 + (r / band_h) * band_pitch + (r % band_h)
 * A plain tile is band_h = out_h (band_pitch unused).  Interleaved stripes
 * for multi-GPU load balance use band_h = stripe height and
 * band_pitch = stripe height * number of ranks.  Rows with y >= frame_h are
 * padding: written as "discarded". */
typedef struct svr_frame {
    int32_t frame_w, frame_h;      /* full frame: NDC uses these (vs_main.wgsl:19) */
    int32_t x0, y0;
    int32_t out_w, out_h;
    int32_t band_h, band_pitch;
} svr_frame;

/* pixel classification written to svr_outputs.flags */
#define SVR_PIX_DISCARD 0   /* no back-face fragment, or nsteps < 1 (fs_main.wgsl:44) */
#define SVR_PIX_MISS    1   /* fragment ran, no significant value (fs_main.wgsl:93-98) */
#define SVR_PIX_HIT     2   /* fragment ran, LMIP found a local maximum (fs_main.wgsl:56-87) */

/* DEVICE pointers, caller-allocated, each out_h*out_w elements (rgba: x4).
 * rgba is the fragment's out.color before blending (fs_main.wgsl:86,95);
 * discarded pixels get (0,0,0,0).  Any pointer except rgba may be NULL. */
typedef struct svr_outputs {
    float*    rgba;
    float*    depth;               /* out.depth (fs_main.wgsl:72,97) */
    uint32_t* label;               /* render_out.segmentation (raycast.wgsl:81) */
    uint8_t*  flags;               /* SVR_PIX_* */
    uint32_t* steps;               /* executed iterations of raycast.wgsl:29-62 per pixel
                                      (instrumented build of the kernel; NULL in production) */
    uint64_t* pick;                /* out.pick of the `write_pick` shader variant (fs_main.wgsl:89-92): the 64 bits of
                                      pygfx's rgba16uint pick target, component k = bits 16k..16k+15:
                                      [0,20) wobject id, [20,34) u32(coord.x*16383), [34,48) .y, [48,62) .z, each
                                      clipped to its width (pygfx `pick_pack`, restated); 0 where nothing was hit */
    uint32_t  pick_id;             /* u_wobject.id */
} svr_outputs;

typedef struct svr_ctx svr_ctx;

/* ---- lifecycle: replaces WrappingBuffer.__init__ texture/uniform creation
 * (_wrapping_buffer.py:47-70) for all LODs of one SubVolume (_wobject.py:72-91) */
int  svr_create(int device, int num_lods, const svr_lod_desc* lods, svr_ctx** out_ctx);
int  svr_destroy(svr_ctx* ctx);
const char* svr_last_error(void);
int  svr_abi_version(void);

/* ---- uniforms */
/* _current_logical_roi_in_pixels setter + scale_factor setter
 * (_wrapping_buffer.py:77-97,105-116).  Takes effect for renders enqueued
 * after the call. */
int  svr_set_lod_state(svr_ctx* ctx, int lod, const svr_lod_state* st);
int  svr_get_lod_state(svr_ctx* ctx, int lod, svr_lod_state* st);
/* SubVolumeMaterial uniform block (_material.py:60-159) */
int  svr_set_material(svr_ctx* ctx, const svr_material* m);

/* ---- texture upload: replaces texture.data[dst] = np.array(src, f32|u32);
 * texture.update_range(...) for BOTH textures (_wrapping_buffer.py:325-335).
 * dst_off/shape: ring voxels, shader order; must lie inside the ring.
 * density/labels: HOST pointers to element (0,0,0) of the source block;
 * strides in BYTES per (x, y, z) step.  Conversion is numpy's cast (to f32 /
 * to u32 with wrap-around).  The copy is staged through pinned memory and
 * enqueued on the context's upload stream; the call returns once the source
 * has been consumed (source may be freed), not when the device copy is done.
 * Either source may be NULL to leave that texture untouched.
 * A stride may be negative (a flipped axis: the pointer is still element (0,0,0), the last one of that axis in memory)
 * or zero (one element, row or plane broadcast along that axis); every pointer is a multiple of its element size.
 * The casts, bit for bit (tests/ring_transfer_cases.py, tests/test_gpu_ring_transfer.py): integers to f32 round to
 * nearest, ties to even (u64 2^24 + 1 -> 2^24, 2^64 - 1 -> 2^64); f64 to f32 the same, beyond the f32 range +-inf,
 * below it subnormals and +-0; the NaN payload of an f64 source is not preserved.
 * Integer labels wrap modulo 2^32 (i8 -128 -> 4294967168, i64 2^32 + 5 -> 5).  Float label sources are defined on
 * [0, 2^32), truncating toward zero (4294967295.9 -> 4294967295); outside it and for NaN the label is undefined.
 * SVR_ERR_RANGE for a region outside the ring; SVR_ERR_INVALID, with nothing enqueued, for a NULL ctx / offset /
 * shape, a lod out of range, an unknown dtype code, NULL strides beside a source, labels into a context without label
 * rings, a source of another dtype into SVR_U8 / SVR_U16 rings, and (host sources) one row of the region, density plus
 * labels in their source types, wider than a staging slot less 32 bytes. */
int  svr_upload_region(svr_ctx* ctx, int lod,
                       const int32_t dst_off[3], const int32_t shape[3],
                       const void* density, int density_dtype, const int64_t density_strides[3],
                       const void* labels,  int labels_dtype,  const int64_t labels_strides[3]);
/* same, but the sources are DEVICE pointers (backing volume resident in HBM) */
int  svr_upload_region_device(svr_ctx* ctx, int lod,
                       const int32_t dst_off[3], const int32_t shape[3],
                       const void* density, int density_dtype, const int64_t density_strides[3],
                       const void* labels,  int labels_dtype,  const int64_t labels_strides[3]);
/* Make everything uploaded so far visible to subsequent renders: the render
 * stream waits (device-side) on an event recorded on the upload stream.  The
 * reference has no equivalent: pygfx flushes update_range uploads before the
 * next draw on the same queue (FUTURE.md:47-58). */
int  svr_publish_uploads(svr_ctx* ctx);

/* ---- asynchronous streaming (the reference has none: FUTURE.md:3-67 lists it as future work).
 * Protocol, driven by the host (SubVolume.center_on_position(..., asynchronous=True)):
 *   1. svr_set_lod_state(ROI := old ROI intersected with the new one)  -- renders enqueued from now on
 *      never touch a ring slot that is about to be overwritten; coarser LODs cover the gap;
 *   2. svr_upload_region(...) for the new chunks, from a worker thread: the copies are ordered
 *      behind the last render that was enqueued with the old ROI, and run beside later renders;
 *   3. svr_mark_uploads(); when svr_uploads_pending() reports 0, svr_set_lod_state(ROI := new).
 * svr_render never waits for marked-but-unpublished uploads. */
int  svr_mark_uploads(svr_ctx* ctx);
int  svr_uploads_pending(svr_ctx* ctx, int* pending);
/* The same, for several loads in flight at once (one per LOD: the coarse levels are uploaded first and
 * published as soon as THEY have landed, FUTURE.md:86-95): svr_upload_ticket records an event behind
 * everything enqueued on the upload stream so far and returns its ticket (> 0); svr_ticket_pending
 * reports 1 while that event has not been reached.  Tickets older than the 64 most recent ones are
 * reported as done only after the oldest live one is (their event has been reused). */
/* diagnostics: bytes that went through the pinned staging slots so far and the host wall-clock seconds spent
 * inside svr_upload_region (packing rows, waiting for a free slot, enqueueing); reset = 1 zeroes both */
int  svr_upload_stats(svr_ctx* ctx, uint64_t* staged_bytes, double* seconds_in_calls, int reset);
int  svr_upload_ticket(svr_ctx* ctx, uint64_t* ticket);
int  svr_ticket_pending(svr_ctx* ctx, uint64_t ticket, int* pending);

/* ---- readback of a ring region into packed host arrays (shader-order
 * shape, x fastest): the texture.data numpy mirror the reference's tests read
 * (tests/wrapping_buffer/test_load_logical_roi.py:5-76).  Synchronous.
 * SVR_U8 / SVR_U16 rings read back as f32 (exact).  Either output may be NULL (it is not written); both NULL, or an
 * extent of 0, reads nothing.  A context without label rings reads every label as 0.  Refusals as for the uploads. */
int  svr_read_region(svr_ctx* ctx, int lod, const int32_t off[3], const int32_t shape[3],
                     float* density_out, uint32_t* labels_out);
/* zero both textures of one LOD (fresh WrappingBuffer state) */
int  svr_clear_lod(svr_ctx* ctx, int lod);

/* ---- the draw: replaces renderer.render(scene, camera) for the
 * (SubVolume, SubVolumeMaterial) pair — vs_main.wgsl:6-50 + fs_main.wgsl:4-101
 * + raycast.wgsl:11-88 + sample_vol.wgsl + hsv_selection.wgsl.
 * Enqueued on `stream` (a hipStream_t passed as void*; NULL = the device's default
 * stream), i.e. ordered with the caller's other work on that stream.  Asynchronous. */
int  svr_render(svr_ctx* ctx, const svr_camera* cam, const svr_frame* frame,
                const svr_outputs* out, void* stream);
/* kernel variant selector for A/B measurement (results are identical for every value):
 * bits 0-3  kernel: 0 = default span march (one wave per workgroup), 1 = straightforward one-load-per-step
 *            march, 2 = span march with 2x2 waves per workgroup; +4 = brick slabs never start longer
 *            than their plain length (default: twice), +8 = no empty-space skipping in LMIP mode (default: waves skip
 *            stretches whose macro-cell maxima stay below the threshold while no lane tracks a maximum)
 * bits 4-7  1 + log2(wave tile width): wave tile = 2^k x 64/2^k pixels (0 = default 8x8)
 * bit  8    never stage LDS bricks nor gather from a micro-block twin (linear gathers only); bit 9: always
 *            (default: per-wave probe).  svr_slice reads these two bits too: 8 = rows only, 9 = the micro-block copy
 *            wherever a LOD keeps one (default: per LOD, the layout whose 128-byte lines a wave's tile touches fewer of)
 * bit  10   keep row-major lane order (default: lanes follow the projected x axis)
 * bits 11-12 reserved: SVR_ERR_INVALID.  (Builds made with -DSVR_EXPERIMENTS — tools/ab_build.py, never the shipped
 *            library — use them for timing experiments that render WRONG pixels, and read the SVR_* environment
 *            switches listed in tools/README.md; the shipped library reads only SVR_PACK_THREADS, the number of host
 *            threads that pack upload blocks.)
 * bits 13-15 block -> tile placement: 0 = 64x64-pixel chunks of tiles sorted by the length of their rays for the draw's
 *            camera, longest first, dealt to the XCDs in snake order (default),
 *            1 = one contiguous run of tiles per XCD, 2..6 = single tiles, 64x32, 32x32, 128x64, 32x16 chunks in raster order,
 *            7 = 64x64 chunks in raster order (camera-independent; about 1 % faster than 0 when several frames are kept in
 *            flight on separate streams, 4 % slower for one frame at a time)
 * bits 16-23 probe threshold in L1 lookups per wave-load (0 = default 32)
 * bits 24-31 mask of LODs allowed to stage bricks (0 = default: all) */
int  svr_set_variant(svr_ctx* ctx, int variant);

/* ---- multi-GPU helper: scatter a rank-major gathered stripe buffer back
 * into a full frame (device pointers).  gathered holds nranks blocks of
 * out_h*out_w*elem_bytes each, laid out by svr_frame with x0 = 0,
 * y0 = rank*band_h, band_pitch = band_h*nranks. */
int  svr_untile_stripes(svr_ctx* ctx, const void* gathered, void* frame_out,
                        int frame_w, int frame_h, int band_h, int nranks,
                        int out_h, int elem_bytes, void* stream);

/* The same for config 3's literal geometry: a grid of grid_x x grid_y tiles of tile_w x tile_h pixels, tile
 * (tx, ty) rendered by rank ty * grid_x + tx (svr_frame with x0 = tx * tile_w, y0 = ty * tile_h, band_h = out_h =
 * tile_h, out_w = tile_w); gathered holds grid_x * grid_y blocks of tile_h * tile_w elements.  Tiles of the
 * last column / row may hang over the frame edge (their excess pixels are padding). */
int  svr_untile_grid(svr_ctx* ctx, const void* gathered, void* frame_out, int frame_w, int frame_h,
                     int tile_w, int tile_h, int grid_x, int grid_y, int elem_bytes, void* stream);

/* ---- the collective (the reference has none): every rank's rendered region -> root, over RCCL
 * (xGMI on one node).  One process per GPU, one context per process.  Rank 0 makes an id
 * (svr_comm_unique_id == ncclGetUniqueId, /opt/rocm/include/rccl/rccl.h:187), hands its SVR_COMM_ID_BYTES bytes to
 * the other ranks by any channel (a file, MPI, torch.distributed), and every rank calls svr_comm_init
 * (ncclCommInitRank, rccl.h:220; collective: returns once all ranks have joined).
 * svr_gather_tiles enqueues on `stream`, for each of `nplanes` planes (RGBA, and depth / label / flags when they
 * are wanted), the transfer of bytes_per_rank[p] bytes from every rank's local[p] into root's
 * gathered[p] + rank * bytes_per_rank[p]: grouped ncclSend / ncclRecv (rccl.h:700,722 — what ncclGather, rccl.h:745,
 * is made of), all planes and peers in one group.  DEVICE pointers; `gathered` is only read on root.  The call is
 * ordered after the work already on `stream` (the render that wrote local) and asynchronous. */
#define SVR_COMM_ID_BYTES 128
int  svr_comm_unique_id(char out_id[SVR_COMM_ID_BYTES]);
int  svr_comm_init(svr_ctx* ctx, const char id[SVR_COMM_ID_BYTES], int rank, int nranks);
int  svr_comm_destroy(svr_ctx* ctx);
int  svr_gather_tiles(svr_ctx* ctx, int nplanes, const void* const* local, void* const* gathered,
                      const size_t* bytes_per_rank, int root, void* stream);

/* ---- LOD pyramid builder (device pointers): one 2x2x2 pooling step with the rules of the reference's
 * offline builders — mode 0 = mean (scripts/create_mouse_multiscale.py:23-54; SVR_U8: floor(sum/8),
 * SVR_F32: pairwise sum * 0.125), mode 1 = max (SVR_U32 labels, scripts/create_platynereis_multiscale.py:86-134).
 * src_dims (x, y, z) must be even; dst has half the extent per axis.  Enqueued on `stream`.
 * Alignment: the SVR_F32 / SVR_U32 kernels read pairs along x with 8-byte loads, so `src` must be 8-byte aligned for
 * them (every row then is, the x extent being even); `dst` must be 4-byte aligned for them.  SVR_U8 takes any
 * address (rows that are not 8-byte aligned are read byte by byte).  A misaligned pointer is refused with
 * SVR_ERR_INVALID before anything is launched.
 * SVR_F32 is IEEE f32 in the written order, ((a000+a001)+(a010+a011)) + ((a100+a101)+(a110+a111)) with x fastest,
 * times 0.125f: NaN and +-inf propagate, a sum that overflows stays inf, subnormals are kept. */
int  svr_pool2x(int device, const void* src, void* dst, const int32_t src_dims[3], int dtype, int mode, void* stream);

/* ---- display side: blend one render "over" a vertical-gradient background (top row =
 * bg_top), optional depth test (fragment passes if depth < inout_depth, then writes it), linear -> sRGB,
 * 8 bits per channel.  Restates what pygfx does after the fragment shader (blending src_alpha /
 * one_minus_src_alpha, depth_compare "<", sRGB canvas); the reference's own tests draw over
 * gfx.Background(None, BackgroundMaterial(bottom, top)) (tests/conftest.py:17-22).  DEVICE pointers;
 * depth / flags / inout_depth may be NULL (NULL flags: every pixel is a fragment).  Parity unpinned.
 * Arithmetic is IEEE f32 in the written order, nothing contracted: t = (y + 0.5f) / height,
 * c = bg_top * (1 - t) + bg_bottom * t, over a fragment c.rgb = s.rgb * a + c.rgb * (1 - a) and
 * c.a = a + c.a * (1 - a), the OETF on c' = fminf(fmaxf(c, 0), 1) (12.92 c' up to 0.0031308f, else
 * 1.055 powf(c', 1 / 2.4f) - 0.055), and each channel stored as (uint8)(fminf(fmaxf(v, 0), 1) * 255 + 0.5f).
 * fmaxf / fminf return their other operand for a NaN, so a NaN channel quantises to 0 (and inf to 255, -inf to 0).
 * A NaN depth, or a NaN in inout_depth, fails "<": the fragment is not drawn and inout_depth keeps its bits.
 * Only powf may differ from a correctly rounded restatement.
 * rgba must be 16-byte aligned and out_rgba8 4-byte aligned (refused with SVR_ERR_INVALID otherwise);
 * width or height 0 is accepted and writes nothing. */
typedef struct svr_compose_params {
    float   bg_bottom[4];
    float   bg_top[4];
    int32_t srgb_encode;           /* 1: encode rgb with the sRGB OETF before quantising */
} svr_compose_params;
int  svr_compose(svr_ctx* ctx, const float* rgba, const float* depth, const uint8_t* flags, int width, int height,
                 const svr_compose_params* params, uint8_t* out_rgba8, float* inout_depth, void* stream);

/* ---- display side: segmentation outlines and selected-object highlighting (FUTURE.md "Tracing Objects": a second
 * pass that finds label edges in the rendered label image and draws them over the intensity image).  Inputs are the
 * planes of one render, each height x width: F = flags (SVR_PIX_*), L = label, Z = depth (optional), S = rgba.
 * Defined HERE (numpy restatement: tests/test_outline.py `outline_reference`) as
 *     hit(p)       F(p) == SVR_PIX_HIT
 *     N_r(p)       the pixels q != p INSIDE the image with max(|dy|, |dx|) <= r  (the image border draws no outline)
 *     selected(p)  selected_count == 0, or L(p) is one of selected[0 .. selected_count)
 *     edge(p)      hit(p) and (!only_selected or selected(p)) and some q in N_r(p) has
 *                    !hit(q)                                   (silhouette against a miss or a discard), or
 *                    hit(q) and L(q) != L(p), or
 *                    depth_tolerance >= 0 and hit(q) and |Z(q) - Z(p)| > depth_tolerance   (units of the depth plane)
 *     out(p)       f32, in this order:
 *                    !hit(p): S(p), bit for bit;
 *                    else b = S(p), and if selected_count > 0 and !selected(p): b.rgb = S.rgb * dim_unselected;
 *                    edge(p): c = color.rgb, or with color_by_label hsv_to_rgb(h, s, 1.0f) of colors[L(p) % color_count]
 *                             (hsv_selection.wgsl: no fog, no srgb2physical), a = color[3],
 *                             out.rgb = b.rgb * (1 - a) + c * a,  out.a = b.a * (1 - a) + a;
 *                    otherwise out = b.
 *     edge_mask(p) 1 where edge(p), else 0 (u8).
 * depth_tolerance -0.0 is not < 0: the depth test is ON, with tolerance 0 (+inf: on, and no step exceeds it; NaN:
 * refused).  A NaN depth, of p or of q, is no step.  A flag byte other than SVR_PIX_HIT (0, 1, or any other value) is
 * a non-hit.  L(p) % color_count is unsigned.
 * DEVICE pointers; depth may be NULL when depth_tolerance < 0, edge_mask may be NULL.  rgba, out_rgba and colors are
 * 16-byte aligned (else SVR_ERR_INVALID, with nothing launched).  `selected` is sorted ascending (an unsorted set
 * gives wrong highlighting but never reads outside it).  out_rgba may be rgba itself (in place): a pixel's output depends on its own rgba alone.  A plane rendered with
 * a region (svr_frame) is outlined as an image of its own: pixels outside it are not neighbours.  Enqueued on
 * `stream`. */
typedef struct svr_outline_params {
    int32_t radius;                /* r, 1 .. 16 */
    float   depth_tolerance;       /* < 0: off */
    int32_t color_by_label;
    float   color[4];              /* rgb used unless color_by_label; [3] = outline opacity in [0, 1] */
    float   dim_unselected;        /* [0, 1]; only used when selected_count > 0 */
    int32_t only_selected;
} svr_outline_params;
int  svr_outline(svr_ctx* ctx, const float* rgba, const float* depth, const uint32_t* label, const uint8_t* flags,
                 int width, int height, const svr_outline_params* params,
                 const float* colors, uint32_t color_count,          /* color_count x vec4 (h, s, v, pad) */
                 const uint32_t* selected, uint32_t selected_count,
                 float* out_rgba, uint8_t* edge_mask, void* stream);

/* ---- cross-section views: the LOD rings sampled on a world-space plane (no counterpart in the reference; the planar
 * view that EM viewers pair with the 3-D one).  A slice is an image of frame_w x frame_h pixels on the plane through
 * `origin` (world position of the image centre) spanned by `u` (world step from one column to the next) and `v` (from
 * one row to the next; rows go down the image).  Output pixels map to frame pixels (x, y) through svr_frame exactly as
 * in svr_render (tiles and stripes alike; frame pixels outside the frame are DISCARD).  Defined HERE (numpy
 * restatement: tests/slice_twin.py) as, in f32, in this order, with no fused operations:
 *     fx   = ((float)x + 0.5f) - 0.5f * (float)frame_w,   fy = ((float)y + 0.5f) - 0.5f * (float)frame_h
 *     p_k  = (origin_k + fx * u_k) + fy * v_k                         world position
 *     q    = world_inv * (p, 1)  in the march's mat_vec summation order ((m0 x + m4 y) + m8 z) + m12;  d = q.xyz
 *     c_k  = (d_k + 0.5f) / size_k                                    the march's normalised coordinate
 *     dx_k = c_k * size_k                                             as sample_vol.wgsl:6 computes it
 * classified from dx:
 *     DISCARD  not 0 <= dx_k < size_k on every axis (NaN is outside):  rgba (0,0,0,0), value 0, label 0, lod 255
 *     HIT      the first LOD l whose ROI holds dx (the march's try_sample_scale_i test, sample_vol.wgsl:4-25):
 *                value = that LOD's density texel (f32), label = its label texel (0 without label rings), lod = l
 *                (the texel passes through bit for bit: NaN with its payload, +-inf, -0.0 and subnormals included),
 *                v = (value - clim[0]) / (clim[1] - clim[0]);  v = powf(v, gamma) if gamma != 1;
 *                v = srgb2physical(v) if colorspace_srgb;  rgb = hsv_to_rgb(h, s, v) of colors[label % color_count];
 *                rgba = (rgb, opacity)                             (the march's shading without fog)
 *     MISS     inside the box, but no LOD's ROI holds it (not resident): rgba (0,0,0,1), value 0, label 0, lod 255
 * depth is 0 everywhere (a slice has no camera).  The material's fog, LMIP uniforms, render mode and clipping planes
 * are not read.  A slice pixel thus shows exactly the voxel a ray sample at that point would read.
 * Reads the LOD state of svr_set_lod_state and the material of svr_set_material.  A render-thread call: it waits for
 * published uploads and later uploads are ordered behind it, like svr_render.  Enqueued on `stream`; asynchronous. */
typedef struct svr_slice_plane {
    float world_inv[16];           /* column-major, like svr_camera */
    float volume_dimensions[3];    /* shader order (x, y, z) */
    float origin[3];               /* world space */
    float u[3];
    float v[3];
} svr_slice_plane;
/* DEVICE pointers, out_h*out_w elements each (rgba: x4, 16-byte aligned).  Any pointer except rgba may be NULL. */
typedef struct svr_slice_outputs {
    float*    rgba;
    float*    depth;               /* 0 */
    uint32_t* label;
    uint8_t*  flags;               /* SVR_PIX_* */
    float*    value;               /* the density texel, 0 where nothing was hit */
    uint8_t*  lod;                 /* the LOD the texel came from, 255 where nothing was hit */
} svr_slice_outputs;
int  svr_slice(svr_ctx* ctx, const svr_slice_plane* plane, const svr_frame* frame, const svr_slice_outputs* out,
               void* stream);

/* ---- thick-slab projections: the maximum, minimum or mean of N samples stacked along a slice's normal (no
 * counterpart in the reference; the thick slices of napari, Fiji's Z-project of a sub-stack).  An addition within ABI
 * version 9: svr_slab is a new symbol, nothing older changes.  Defined HERE (numpy restatement: tests/slab_twin.py),
 * in f32, in this order, with no fused operations.  Each pixel starts from svr_slice's chain: fx, fy, p and
 * q = world_inv * (p, 1) exactly as there.  With the data-space sample step
 *     dw_k = (m[k] * w_x + m[4+k] * w_y) + m[8+k] * w_z                the linear part of world_inv applied to w
 * sample k = 0 .. N-1 sits at t_k = (float)k - 0.5f * (float)(N-1) steps from the plane:
 *     q_k  = q + t_k * dw                                               per component, multiply then add
 *     dx_k = ((q_k + 0.5f) / size) * size
 * and is classified DISCARD / MISS / HIT from dx_k exactly as a slice pixel (outside the box; inside with nothing
 * resident; the first LOD whose ROI holds it, giving value_k, label_k, lod_k).  Reduced over the HIT samples only:
 *     MAX / MIN  best = the first HIT sample; a later HIT sample replaces it iff value_k > best (MAX) or
 *                value_k < best (MIN).  Ties keep the lowest k; a NaN first HIT stays, a later NaN never wins.
 *                IEEE comparisons: -0.0 and +0.0 tie (the lower k stays), +inf beats every finite value under MAX
 *                and -inf under MIN.
 *                value, label, lod and depth are those of the chosen sample.
 *     MEAN       value = (the sum of the HIT values, accumulated in f32 in increasing k) / (float)hits;
 *                a NaN sample, or +inf and -inf in one column, make it NaN; a sum that overflows stays infinite;
 *                label, lod and depth are those of the sample MAX would choose.
 *     depth      t_k * w_len of the chosen sample: the signed world offset from the centre plane (w_len = |w|, the
 *                f32 of its float64 norm, given by the caller), so svr_outline's depth test applies to slabs.
 * The pixel is HIT if any sample hit, shaded from (value, label) exactly as a slice HIT; else MISS if any sample lay
 * inside the box (rgba (0,0,0,1), value 0, label 0, lod 255, depth 0); else svr_slice's DISCARD.  Since t_0 = 0 when
 * N = 1, q_0 = q: N = 1 with MAX is bit-identical to svr_slice on every plane.  Output planes and pointer rules are
 * svr_slice_outputs'; ordering and variant bits 8 / 9 (micro-block copy routing) are svr_slice's.  SVR_ERR_INVALID,
 * with nothing enqueued, for: samples outside 1 .. 4096, an unknown mode, a w, dw or w_len that is not finite (or a
 * negative w_len), and svr_slice's own refusals. */
#define SVR_SLAB_MAX  0
#define SVR_SLAB_MIN  1
#define SVR_SLAB_MEAN 2
#define SVR_SLAB_MAX_SAMPLES 4096
typedef struct svr_slab_params {
    svr_slice_plane plane;         /* as svr_slice: the centre plane */
    float   w[3];                  /* world step from one sample to the next */
    float   w_len;                 /* |w|, for the depth plane */
    int32_t samples;               /* N, 1 .. SVR_SLAB_MAX_SAMPLES */
    int32_t mode;                  /* SVR_SLAB_* */
} svr_slab_params;
int  svr_slab(svr_ctx* ctx, const svr_slab_params* params, const svr_frame* frame, const svr_slice_outputs* out,
              void* stream);

/* ---- composite render mode: front-to-back emission-absorption compositing (direct volume rendering) through a
 * transfer function, along the march's rays (no counterpart in the reference; FUTURE.md's "swappable rendering
 * pipeline").  An addition within ABI version 9: new symbols only; svr_material, svr_outputs and svr_render keep their
 * layout and behaviour.  Defined HERE (numpy restatement: tests/composite_twin.py), in f32, in this order, with no
 * fused operations.  Per pixel:
 *   ray      the march's: pixel -> frame through svr_frame, the DISCARD rules, the clipping planes (ANY / ALL), start,
 *            step and nsteps exactly as svr_render's setup (orthographic cameras included).
 *   samples  i = 0 .. nsteps-1 where the march puts them: off = iter * step, coord = start + off (iter the float
 *            counter of the march), dx = coord * size; the first LOD whose ROI holds dx gives the value s and the label
 *            lab (0 without label rings).  A sample that no LOD holds contributes nothing (it is counted in steps).
 *   table    T of K entries (2 <= K <= SVR_TF_MAX_ENTRIES), RGBA with RGB in linear light and alpha already corrected
 *            for the step (svr_set_transfer_function):
 *              v   = (s - clim[0]) / (clim[1] - clim[0])
 *              x   = fminf(fmaxf(v * (float)(K-1), 0.0f), (float)(K-1))          (NaN -> 0)
 *                                                              (fmaxf drops the NaN; +inf -> K-1, -inf and v < 0 -> 0)
 *              j   = min((int)x, K-2);  f = x - (float)j
 *              e_c = T[j].c + f * (T[j+1].c - T[j].c)                              c = r, g, b, a
 *   tint     color_by_label: q = hsv_to_rgb(h, s, 1.0f) of colors[lab % color_count];  e_rgb = e_rgb * q per component
 *   compose  R = G = B = A = 0, w_best = 0, then per sample in order:
 *              w = (1.0f - A) * e_a
 *              R = R + w * e_r;  G = G + w * e_g;  B = B + w * e_b;  A = A + w
 *              if (w > w_best)  { w_best = w; best = i }                           (strict: the first wins)
 *              if (first unset and w > 0)  first = i
 *              if (A >= alpha_cutoff)  stop after this sample
 *   outputs  HIT when A > 0: rgba = (R/A, G/A, B/A, A * opacity) (straight alpha); depth = the march's depth formula
 *              at the coordinate of `first`; label = the label at the coordinate of `best`; pick = the march's packing
 *              of `best`'s coordinate.
 *            MISS when the ray ran but A == 0: rgba (0,0,0,0) (transparent, unlike LMIP's opaque black), depth, label
 *              and pick 0.
 *            DISCARD as in the march.
 *            steps (when not NULL; written by this kernel, no instrumented build): the samples visited.
 * The material's clim, opacity, colors and clipping planes are read; gamma, fog, colorspace_srgb, the lmip_* fields
 * and render_mode are not.  A render-thread call like svr_render: it waits for published uploads, later uploads wait
 * for it.  Enqueued on `stream`; asynchronous.  SVR_ERR_INVALID, with nothing enqueued, when no material or no table
 * has been set, alpha_cutoff is not in (0, 1], or any frame or camera check of svr_render fails. */
#define SVR_TF_MAX_ENTRIES 4096
/* rgba: HOST pointer to K x 4 floats, each finite and in [0, 1], else SVR_ERR_INVALID.  Copied to the device; ordered
 * like svr_set_material (composites enqueued earlier keep the table they were enqueued with). */
int  svr_set_transfer_function(svr_ctx* ctx, const float* rgba, int32_t K);
typedef struct svr_composite_params {
    float   alpha_cutoff;          /* (0, 1]: the ray stops once its accumulated opacity reaches it */
    int32_t color_by_label;        /* 1: tint each sample's colour by its label's hue */
} svr_composite_params;
int  svr_composite(svr_ctx* ctx, const svr_camera* cam, const svr_frame* frame, const svr_composite_params* params,
                   const svr_outputs* out, void* stream);

/* ---- iso-surface render mode: the first point along each of the march's rays where the density reaches a level,
 * shaded from the local gradient (pygfx's VolumeIsoMaterial; no counterpart in the reference; FUTURE.md's "swappable
 * rendering pipeline").  An addition within ABI version 9: new symbols only; svr_material, svr_outputs, svr_camera,
 * svr_frame and svr_render keep their layout and behaviour.  Defined HERE (numpy restatement: tests/iso_twin.py), in
 * f32, in this order, with no fused operations; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  Per pixel:
 *   ray      the march's, exactly as svr_composite takes it: pixel -> frame through svr_frame, the DISCARD rules, the
 *            clipping planes (ANY / ALL), start, step and nsteps (orthographic cameras included).
 *   S(iter)  the sample at the float counter iter: coord = start + iter * step, d = coord * size (per component); the
 *            first LOD l whose ROI holds (int)(d * scale_l) gives the value s (the ring's element converted to f32: u8
 *            and u16 exactly, unnormalised like lmip_threshold) and the label (0 without label rings).  A point that
 *            no LOD holds has no value and cannot hit.
 *   coarse   i = 0 .. nsteps-1 in order, iter = (float)i; the candidate is the first i with s >= iso_value.  s is
 *            signed (not |s|) and the comparison is IEEE: a NaN sample is never a candidate and is passed over, +inf
 *            reaches every level, -inf only iso_value = -inf (which every sample but a NaN reaches).  Skipping by the
 *            macro-cell maxima (of |s|, a NaN never wins: an all-NaN cell has maximum 0) changes no plane.
 *   refine   none when i == 0 or refine <= 1: the hit is at iter = (float)i.  Else k = 1 .. refine-1 in order,
 *            iter = (float)(i-1) + (float)k / (float)refine; the first with s >= iso_value is the hit, else iter =
 *            (float)i (a refinement sample that is NaN fails >= like a coarse one).
 *            A linear search: sampling is nearest-texel, the field along a ray is a step function and a
 *            bisection may miss the first crossing.
 *   gradient at the hit (coordinate c, data point d = c * size, LOD l that gave its value), central differences of one
 *            voxel of that LOD per axis: h_a = 1.0f / scale_l[a];  D(p) = the value the LOD cascade gives for the data
 *            point p (computed like d above from p directly), 0 where no LOD holds it;
 *              g_x = (D(d.x + h_x, d.y, d.z) - D(d.x - h_x, d.y, d.z)) * scale_l[x]      (y, z alike)
 *            to world space with the inverse-transpose of world (m = cam->world_inv, column-major):
 *              G_x = (m[0]*g_x + m[1]*g_y) + m[2]*g_z;  G_y = (m[4]*g_x + m[5]*g_y) + m[6]*g_z;  G_z = (m[8].. m[10])
 *              len = sqrtf(dot(G, G));  n = (-G_x / len, -G_y / len, -G_z / len)   (towards falling density)
 *            A len that is 0 or not finite gives n = v (below).
 *   view     sd = step * size (per component);  w = world's upper 3 x 3 times sd:
 *              w_x = (world[0]*sd_x + world[4]*sd_y) + world[8]*sd_z  (w_y from world[1], [5], [9]; w_z from [2], [6], [10])
 *              vl = sqrtf(dot(w, w));  v = (-w_x / vl, -w_y / vl, -w_z / vl)   (towards the viewer along the pixel's ray)
 *            A vl that is 0 or not finite gives v = (0, 0, 0).
 *   light    l = v (a headlight) when headlight != 0, else light_direction (world space, from the surface towards the
 *            light).  hv = l + v per component;  hl = sqrtf(dot(hv, hv));  h = hv / hl, or (0,0,0) when hl is 0 or
 *            not finite.
 *   shading  two-sided Blinn-Phong in linear light:
 *              ndl = fabsf(dot(n, l));  sp = fabsf(dot(n, h));  repeat shininess_log2 times: sp = sp * sp
 *              t = ambient + diffuse * ndl
 *              rgb_c = fminf(fmaxf(base_c * t + specular * sp, 0.0f), 1.0f)
 *            base = iso_color, or with color_by_label hsv_to_rgb(h, s, 1.0f) of colors[label % color_count] (the hue
 *            conversion of the other modes).  The specular power is repeated squaring, not powf.
 *   outputs  HIT: rgba = (rgb, opacity); depth = the march's depth formula at c; label = the label S gave at the hit;
 *              pick = the march's packing of c; normal = n.
 *            MISS when the ray ran and nothing reached the level: rgba (0,0,0,0) (transparent, like svr_composite),
 *              depth, label, pick and normal 0.
 *            DISCARD as in the march (normal 0).
 *            steps (when not NULL; written by this kernel, no instrumented build): the coarse samples up to and
 *              including the candidate, i + 1, or nsteps on a MISS; independent of refine and of skipping.
 * Empty-space skipping: before each stretch of 8 coarse samples the kernel looks the stretch's index box up in the
 * macro-cell maxima the uploads maintain ("iso_kernel"); a stretch in which no lane of the wave can reach
 * iso_value is passed without fetching texels.  It never changes an output plane; no_skip switches it off (A/B).
 * The material's opacity, colors and clipping planes are read; clim, gamma, fog, colorspace_srgb, the lmip_* fields,
 * render_mode and the transfer function are not.  A render-thread call like svr_render: it waits for published
 * uploads, later uploads wait for it.  Enqueued on `stream`; asynchronous.  SVR_ERR_INVALID, with nothing enqueued,
 * when no material has been set, iso_value is NaN, refine is outside 0 .. SVR_ISO_MAX_REFINE, shininess_log2 is
 * outside 0 .. SVR_ISO_MAX_SHININESS_LOG2, ambient, diffuse, specular or a component of iso_color is negative or not
 * finite (iso_color: above 1), headlight is 0 and light_direction is not finite or not of unit length (within 1e-3),
 * or any frame or camera check of svr_render fails. */
#define SVR_ISO_MAX_REFINE 16
#define SVR_ISO_MAX_SHININESS_LOG2 10
typedef struct svr_iso_params {
    float    iso_value;            /* the level, in the ring's own units (compared like lmip_threshold) */
    int32_t  refine;               /* 0 .. 16: sub-samples per coarse step searched before the candidate (<= 1: none) */
    float    iso_color[3];         /* base colour, linear light, each in [0, 1] */
    int32_t  color_by_label;       /* 1: base colour = the hue of the hit's label */
    float    ambient, diffuse, specular;   /* each finite and >= 0 */
    int32_t  shininess_log2;       /* 0 .. 10: the specular exponent is 2^shininess_log2 */
    int32_t  headlight;            /* != 0: the light sits at the viewer; 0: light_direction */
    float    light_direction[3];   /* world space, unit length, towards the light (read when headlight == 0) */
    int32_t  no_skip;              /* != 0: march every stretch (same planes, bit for bit) */
    float*   normal;               /* device, out_h * out_w * 3 floats, or NULL: the unit world-space normal n */
    uint32_t* skip_counters;       /* device, 2 words, or NULL: the kernel ADDS the wave-stretches it [0] marched and
                                      [1] skipped (diagnostics: the share of empty space passed) */
} svr_iso_params;
int  svr_iso(svr_ctx* ctx, const svr_camera* cam, const svr_frame* frame, const svr_iso_params* params,
             const svr_outputs* out, void* stream);

/* ---- interpolation: an opt-in trilinear sample for svr_slice, svr_slab, svr_composite and svr_iso (pygfx's volume
 * materials carry `interpolation`; the reference samples nearest texels because a hardware sampler cannot follow a
 * wrapping ring, KNOWLEDGE.md "textureLoad vs textureSample" - here the wrap is software in every kernel).  An addition
 * within ABI version 9: one new symbol, no struct changes.  svr_render (LMIP, weighted average) is not affected: the
 * march samples nearest texels, the contract with the reference.
 * THE LINEAR SAMPLE, defined HERE (numpy restatement: tests/linear_twin.py), in f32, in this order, with no fused
 * operations, for a data point d (what the definitions above call dx = coord * size):
 *   LOD    unchanged: with s_a = d_a * scale_l[a], the first LOD l whose ROI holds (int)s_a on every axis.  A point no
 *          LOD holds has no value, as before.  label and lod are the nearest sample's (labels are never interpolated).
 *   cell   p_a = s_a - 0.5f;  b_a = floorf(p_a);  f_a = p_a - b_a;  i0_a = (int)b_a;  i1_a = i0_a + 1
 *          (floorf, not a cast: p_a is negative in the first half voxel).
 *   clamp  i0_a and i1_a each clamped to [offset_l[a], offset_l[a] + shape_l[a] - 1], the LOD's resident window: all
 *          eight corners come from LOD l, through the same ring wrap as the nearest texel.  Clamp-to-edge at the window
 *          (which is clipped to the data extent and grown to the chunk grid: at a volume face it ends at, or a partial
 *          chunk past, the last voxel).  The seam nearest sampling shows at a LOD border remains; fading LODs into one
 *          another is a different feature.
 *   blend  v_xyz = the corner texel converted to f32 as for the nearest sample; x first, then y, then z, each as
 *          a + f * (b - a):
 *            c00 = v000 + f_x * (v100 - v000);  c10 = v010 + f_x * (v110 - v010)
 *            c01 = v001 + f_x * (v101 - v001);  c11 = v011 + f_x * (v111 - v011)
 *            c0  = c00 + f_y * (c10 - c00);     c1  = c01 + f_y * (c11 - c01)
 *            value = c0 + f_z * (c1 - c0)
 * At a voxel centre every f_a is 0 and the value is the nearest texel bit for bit (finite data).
 * A corner that is not finite yields whatever these seven expressions yield, weights of 0 included: a NaN corner makes
 * the value NaN at any weight (0 * NaN).  In a step a + f * (b - a), an infinite b gives that infinity for f > 0 and
 * NaN at f == 0 (0 * inf); an infinite a gives NaN at every f (b - a is the other infinity: 0 * inf, or inf - inf);
 * so do two infinities, equal or opposite.  The voxel-centre identity above therefore holds for finite cells only.
 * With SVR_INTERP_LINEAR the sample replaces the nearest texel, and nothing else in each definition changes, in:
 *   svr_slice      the value plane and the shading input.
 *   svr_slab       every sample's value_k; reductions, tie rules and depth are unchanged.
 *   svr_composite  s of every sample.
 *   svr_iso        S(iter) of the coarse and refine searches, and D(p) of the gradient (the linear sample at p with its
 *                  own LOD pick, 0 where no LOD holds p; h_a and the final * scale_l[a] stay those of the hit's LOD).
 *                  The refine search stays a linear search; the field along a ray is now continuous inside a LOD, so it
 *                  locates the crossing inside a voxel (to 1 / refine of a step) instead of the face of a voxel.
 *                  Empty-space skipping stays invisible: the looked-up index box grows by one voxel per side and the
 *                  cell maximum is compared with a rounding margin ("linear sampling").
 * Read by the svr_slice, svr_slab, svr_composite and svr_iso calls enqueued after it; a render-thread call like
 * svr_set_material.  A fresh context is SVR_INTERP_NEAREST.  An unknown mode: SVR_ERR_INVALID, state unchanged. */
#define SVR_INTERP_NEAREST 0
#define SVR_INTERP_LINEAR  1
int  svr_set_interpolation(svr_ctx* ctx, int mode);

/* ---- cut planes: trimmed rays and flat lit caps for svr_composite and svr_iso (the cut-away view of a volume viewer;
 * the material's clipping planes, pygfx's rule, discard whole pixels by where the ray LEAVES the box and never shorten
 * a ray).  An addition within ABI version 9: one new symbol, no struct changes.  svr_render, svr_slice and svr_slab
 * are not affected: the march keeps the contract with the reference.
 *   planes   HOST pointer to count x (a, b, c, d) in world space, copied.  count == 0 clears the planes (planes may
 *            then be NULL).  A world point w is BEHIND plane k when dot(w, abc_k) < d_k: the sense of clipping_planes.
 *   mode     a point is CUT AWAY when it is behind ANY plane (SVR_CUT_ANY: what stays is the intersection of the
 *            half-spaces) or behind ALL of them (SVR_CUT_ALL: a convex wedge is removed).
 * THE CUT PREDICATE, defined HERE (numpy restatement: tests/cut_twin.py), in f32, in this order, with no fused
 * operations; m = cam->world, column-major as the iso view vector reads it.  Per call, on the host:
 *     g_k.x = (m[0]*a + m[1]*b) + m[2]*c;   g_k.y = (m[4]*a + m[5]*b) + m[6]*c;   g_k.z = (m[8]*a + m[9]*b) + m[10]*c
 *     h_k   = ((m[12]*a + m[13]*b) + m[14]*c) - d
 *     len_k = sqrtf(dot(abc_k, abc_k));  nhat_k = (a/len_k, b/len_k, c/len_k)
 * per ray, from the start, step and size of the ray set-up:
 *     p0_a = start_a*size_a - 0.5f;  sd_a = step_a*size_a  (the iso definition's sd)
 *     A_k  = dot(g_k, p0) + h_k;     B_k  = dot(g_k, sd)
 * per float counter iter:
 *     E_k(iter) = A_k + iter*B_k;  behind_k(iter) = E_k(iter) < 0.0f;  cut(iter) = OR (ANY) or AND (ALL) over k
 * Along one ray E_k is monotone in iter, under f32 rounding too (iter*B_k is a monotone rounded product, adding A_k is
 * monotone).  So each plane's behind-set over i = 0 .. nsteps-1 is a prefix or a suffix; under ANY the kept samples
 * form one index interval, under ALL the cut samples do.  The kernels use that: they find the interval once per ray
 * (a binary search on the predicate itself, so it agrees with it exactly) and mask samples by integer compares.
 *   svr_composite  a sample i with cut((float)i) is treated exactly like a sample no LOD holds: it contributes nothing
 *                  and is counted in steps.  Nothing else in the definition changes.
 *   svr_iso        S(iter) has no value where cut(iter), in the coarse search and in the refine search.  D(p) of the
 *                  gradient reads the uncut field.  steps keeps its definition: i + 1 on a hit, nsteps on a MISS.
 *                  Label, depth, pick and colour rules are unchanged.
 *   caps (svr_iso) pred = the point examined immediately before the hit in search order:
 *                    hit at refine sub-sample k >= 2:                  pred = (float)(i-1) + (float)(k-1)/(float)refine
 *                    hit at k == 1:                                    pred = (float)(i-1)
 *                    hit at (float)i after a refine search found none: pred = (float)(i-1) + (float)(refine-1)/(float)refine
 *                    hit at (float)i with refine <= 1 and i > 0:       pred = (float)(i-1)
 *                    i == 0:                                           there is no pred
 *                  The hit is a CAP when pred exists and cut(pred).  On a cap the normal is the cutting plane's: under
 *                  ANY k is the lowest index with behind_k(pred), under ALL the lowest with !behind_k(hit);
 *                  n = nhat_k, negated when dot(n, v) < 0.0f (v the view vector; a zero v leaves n as it is).  Shading
 *                  proceeds with that n and the normal plane receives it.  A ray that enters at the box face (i == 0)
 *                  keeps the gradient normal.
 *   skipping       a wave-stretch in which every live lane's eight coarse samples are cut is passed without fetching
 *                  texels or cell maxima and counted under skip_counters[1] (with no_skip too: it is exact).  Skipping
 *                  stays invisible in every output plane.
 * Read by the svr_composite and svr_iso calls enqueued after it; a render-thread call like svr_set_interpolation.  A
 * fresh context has no planes.  SVR_ERR_INVALID, with the state unchanged, for: count > SVR_MAX_CUT_PLANES, NULL planes
 * with count > 0, an unknown mode, any component not finite, a len_k that is 0 or not finite. */
#define SVR_MAX_CUT_PLANES 8
#define SVR_CUT_ANY 0
#define SVR_CUT_ALL 1
int  svr_set_cut_planes(svr_ctx* ctx, const float* planes, uint32_t count, int mode);

/* ---- intensity histograms of the resident rings: what values does a window hold?  (No counterpart in the reference;
 * the histogram panel behind a transfer-function editor, an auto-contrast button, a first iso_value, the distribution
 * of a selected object.)  An addition within ABI version 9: one new symbol and two new structs, nothing older changes.
 * One streaming pass over the ring in HBM; nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/histogram_twin.py):
 *   considered  the logical voxels (x, y, z) of LOD `lod` in the intersection of box and window, the window being [offset, offset + shape) of
 *               svr_set_lod_state and the box [box_off, box_off + box_shape) (use_box == 0: the whole window).  A window
 *               of None (offset == shape == 0) and a box that misses the window consider nothing.  With
 *               selected_count > 0 only the voxels whose label texel is one of selected[0 .. selected_count); without
 *               label rings every label reads as 0, as in svr_read_region.
 *   texel       ring slot (x % ring_x, y % ring_y, z % ring_z) of the row-major ring (the micro-block copy is never
 *               read); v = the element converted to f32, exactly for u8 and u16, as the nearest sample of the other
 *               modes converts it.
 *   binning     in f32, in this order, with no fused operations; inv = (float)K / (hi - lo), computed once on the host:
 *                 v is NaN   tail[2] += 1
 *                 v < lo     tail[0] += 1
 *                 v > hi     tail[1] += 1
 *                 otherwise  j = min((int)((v - lo) * inv), K - 1);  counts[j] += 1      (closed at hi, as numpy's is)
 *               A range wider than f32 (hi - lo overflows to inf) is accepted: inv is then 0 and every value inside the
 *               range counts in bin 0, those whose v - lo overflows too (the product inf * 0 is NaN) included.
 *   range       the minimum and maximum of the considered values that are not NaN, those under and over included;
 *               (+inf, -inf) when there are none.
 *   tail[3]     the number of considered voxels = sum(counts) + tail[0] + tail[1] + tail[2].
 * The call OVERWRITES its outputs: it zeroes them on `stream`, then fills them.  Counts are integers, so the result
 * does not depend on the order in which the device visits the voxels.  A render-thread call ordered like svr_slice: it
 * waits for published uploads, and later uploads are ordered behind it.  Enqueued on `stream`; asynchronous.  The
 * material, the variant, the interpolation and the cut planes are not read.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL params, outputs or counts; lod out of
 * range; bins outside 1 .. SVR_HIST_MAX_BINS; lo or hi not finite, or lo >= hi; an inv that is not finite; a negative
 * box_shape component (with use_box != 0); selected == NULL with selected_count > 0. */
#define SVR_HIST_MAX_BINS 4096          /* = SVR_TF_MAX_ENTRIES: one bin per transfer-function entry */
typedef struct svr_histogram_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: the coordinates of svr_lod_state */
    float   lo, hi;                     /* finite, lo < hi */
    int32_t bins;                       /* K, 1 .. SVR_HIST_MAX_BINS */
    const uint32_t* selected;           /* DEVICE, sorted ascending, like svr_outline's; NULL when the count is 0 */
    uint32_t selected_count;            /* 0: every voxel */
} svr_histogram_params;
typedef struct svr_histogram_outputs {  /* DEVICE pointers; counts required, the others may be NULL */
    uint64_t* counts;                   /* K */
    uint64_t* tail;                     /* 4: [0] under, [1] over, [2] NaN, [3] voxels considered */
    float*    range;                    /* 2: min and max of the considered non-NaN values; (+inf, -inf) when there are none */
} svr_histogram_outputs;
int  svr_histogram(svr_ctx* ctx, const svr_histogram_params* params, const svr_histogram_outputs* out, void* stream);

/* ---- per-object measurements of the resident rings: which objects are resident, how big is each, where is it, what
 * is its mean intensity?  (No counterpart in the reference; the rows of a segment table, the box that crops a view to a
 * picked object, the point to fly to.)  An addition within ABI version 9: one new symbol and three new structs, nothing
 * older changes.  One streaming pass over the label and density rings in HBM fills a table of records, one per label;
 * nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/objects_twin.py):
 *   considered  exactly svr_histogram's voxels: the logical voxels (x, y, z) of LOD `lod` in the intersection of box and
 *               window, read from ring slot (x % ring_x, y % ring_y, z % ring_z) of the row-major ring (the micro-block
 *               copy is never read); without label rings every label reads as 0.  Then, with selected_count > 0, only
 *               the voxels whose label is one of selected[0 .. selected_count).  Then, with ignore_zero != 0, the
 *               voxels of label 0 are dropped: they are counted in header[3] and nowhere else.  A window of None and a
 *               box that misses the window consider nothing.
 *   records     `capacity` records of 96 bytes.  One record per distinct considered label that found a slot, in no
 *               particular order; every byte of an unused record is 0.  Labels 0 and 0xFFFFFFFF are ordinary labels.
 *   header      8 x uint64_t:
 *                 [0] occupied records
 *                 [1] considered voxels
 *                 [2] overflow: the considered voxels whose label found no slot
 *                 [3] label-0 voxels dropped by ignore_zero (they passed box and `selected`; not part of [1])
 *                 [4..6] the window offset (x, y, z) of the LOD the call used, as int64 bit patterns; sum[] is relative to it
 *                 [7] 0
 *   slots       an insertion can reach every record (linear probing over the whole table), so header[2] != 0 if and
 *               only if more than `capacity` distinct labels are considered.  Then exactly `capacity` records are
 *               occupied, every one of them is complete and exact for its label (a label that owns a record never
 *               loses voxels), and sum(voxels) + header[2] == header[1].  Which labels got records is unspecified.
 *   value       the raw ring element.  u8 / u16 rings: value_sum is the u64 sum, finite == voxels, vmin / vmax the
 *               extremes as f32 (exact).  float32 rings: only finite values count in finite, value_sum, vmin and vmax;
 *               value_sum holds the BITS of an f64 sum whose every partial sum is held in f64.
 * The call OVERWRITES its outputs: it zeroes them on `stream`, then fills them.  On integer rings every field is an
 * integer sum, a minimum or a maximum: the result does not depend on the order in which the device visits the voxels.
 * On float32 rings value_sum is the one order-dependent field (f64 additions in any order).  A render-thread call
 * ordered like svr_histogram: it waits for published uploads, and later uploads are ordered behind it.  Enqueued on
 * `stream`; asynchronous.  The material, the variant, the interpolation and the cut planes are not read.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL ctx, params, outputs, records or
 * header; lod out of range; capacity 0 or above SVR_OBJECTS_MAX_CAPACITY; a negative box_shape component (with
 * use_box != 0); selected == NULL with selected_count > 0. */
#define SVR_OBJECTS_MAX_CAPACITY (1u << 26)
typedef struct svr_objects_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: svr_histogram_params' */
    const uint32_t* selected;           /* DEVICE, sorted ascending; NULL when the count is 0 */
    uint32_t selected_count;            /* 0: every label */
    int32_t  ignore_zero;               /* != 0: voxels of label 0 take no part; they are counted in header[3] */
    uint32_t capacity;                  /* records in svr_objects_outputs::records, 1 .. SVR_OBJECTS_MAX_CAPACITY (any integer) */
} svr_objects_params;
typedef struct svr_object_record {
    uint32_t label;
    uint32_t used;        /* 1: occupied; 0: empty, every byte of the record is 0 */
    uint64_t voxels;      /* considered voxels with this label */
    uint64_t sum[3];      /* sum over them of (x - off_x), (y - off_y), (z - off_z); off = header[4..6] */
    int32_t  lo[3], hi[3];/* smallest and largest logical voxel coordinate, both inclusive, shader order, LOD voxels */
    uint64_t finite;      /* those whose value is finite (u8 / u16 rings: == voxels) */
    uint64_t value_sum;   /* u8 / u16 rings: the u64 sum of the raw values.  float32 rings: the BITS of an f64 sum
                             of the finite values, every partial sum held in f64 */
    float    vmin, vmax;  /* over the finite values; (+inf, -inf) when finite == 0 */
    uint64_t reserved;    /* 0 */
} svr_object_record;
typedef struct svr_objects_outputs {    /* DEVICE pointers, both required */
    svr_object_record* records;         /* capacity */
    uint64_t* header;                   /* 8 */
} svr_objects_outputs;
int  svr_objects(svr_ctx* ctx, const svr_objects_params* params, const svr_objects_outputs* out, void* stream);

/* ---- surface meshes of the resident rings: a picked object, or a level set, as vertices and triangles.  (No
 * counterpart in the reference; what an exporter, a surface-area or volume measurement, or a mesh renderer beside the
 * volume needs.)  An addition within ABI version 9: one new symbol and two new structs, nothing older changes.  The
 * mesh is extracted in HBM; nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/mesh_twin.py).  The method is naive surface nets: one vertex per mixed cell,
 * one quad per crossing lattice edge; there is no case table.
 *   coordinates LOD-`lod` logical voxels in shader order (x, y, z); integer c is the CENTRE of voxel c (the convention
 *               of the Python side's lod_center_to_data).
 *   box B       [lo, lo + n): the intersection of box and window exactly as in svr_histogram (use_box, box_off,
 *               box_shape).  A window of None and a box that misses the window give an empty mesh.
 *   inside(p)   p is in B, and
 *                 SVR_MESH_LABELS  the label texel of p is one of selected[0 .. selected_count) (sorted ascending,
 *                                  selected_count >= 1); without label rings every label reads as 0;
 *                 SVR_MESH_LEVEL   v >= level, v being the density element converted to f32 exactly as svr_histogram
 *                                  converts it.  A NaN is outside.  `level` is in the ring's own units, like iso_value.
 *               Every voxel outside B is outside, so surfaces are closed, with flat caps half a voxel beyond B's faces.
 *               The texel is ring slot (x % ring_x, y % ring_y, z % ring_z) of the row-major ring (the micro-block
 *               copy is never read).
 *   cells       cell c has the 8 corners c + d, d in {0, 1}^3; c ranges over [lo - 1, lo + n - 1] on every axis:
 *               (n_x + 1)(n_y + 1)(n_z + 1) cells.  A cell is ACTIVE when its corners are neither all inside nor all
 *               outside.  An edge CROSSES when inside() differs at its two ends.
 *   vertex      of an active cell c: (float)(c - window offset) + q per axis (one f32 add), where q is the f32 sum,
 *               added one by one in a fixed order, of the crossing points of the cell's crossing edges, divided by
 *               (float)k, k being their number.  The order: the 4 x-edges, the 4 y-edges, the 4 z-edges; within an
 *               axis by the corner offsets on the two other axes, the higher of those axes being the major key
 *               (x-edges: (dy, dz) = (0,0), (1,0), (0,1), (1,1)).  A crossing point has t on the edge's own axis and
 *               the edge's corner offsets (0 or 1) on the others.  t = 0.5, except in SVR_MESH_LEVEL when both ends
 *               lie in B and both values are finite: then, with v0 the value at the lower end, r = (level - v0) /
 *               (v1 - v0) in f32, t = r clamped to [0, 1], and t = 0.5 when r is not finite.  No fused operations.
 *   vertices    in ascending order of the cell (z, then y, then x).
 *   quads       edge (p, a) runs from voxel p to p + e_a, p in the cell range, a in {x, y, z}.  When it crosses, with
 *               (b, c) the axes that follow a cyclically (x: (y, z), y: (z, x), z: (x, y)), the four cells around it
 *               are k0 = p - e_b - e_c, k1 = p - e_c, k2 = p, k3 = p - e_b; all four are active and in the cell range
 *               (an end outside B is outside, so no edge crosses on the low border of the range).  The quad is
 *               (k0, k1, k2, k3) when inside(p), whose normal +a points out of the object, else (k0, k3, k2, k1); it
 *               gives the triangles (q0, q1, q2) and (q0, q2, q3), vertex indices as int32.
 *               Quads in ascending order of p (z, then y, then x), then axis x, y, z; a quad's two triangles adjacent.
 *   header      8 x uint64_t:
 *                 [0] vertices V        [1] triangles T
 *                 [2] vertices written  [3] triangles written
 *                 [4..6] the window offset (x, y, z) of the LOD the call used, as int64 bit patterns
 *                 [7] the number of inside voxels
 *               If V > vertex_capacity or T > triangle_capacity NEITHER array is written and [2] = [3] = 0; else
 *               [2] = V, [3] = T.  Capacities of 0 with NULL arrays are the count-only call.  The header is overwritten
 *               by every call.
 * The output is fully specified, order included: two calls on the same rings give identical bytes.  Ordered like
 * svr_objects: it waits for published uploads, and later uploads are ordered behind it.  Enqueued on `stream`;
 * asynchronous.  The call works in scratch memory owned by the context (about 1 byte per cell, grown on demand,
 * SVR_ERR_NOMEM when it cannot be, released by svr_destroy); a call is ordered behind the previous svr_mesh of the same
 * context, whatever its stream.  The material, the variant, the interpolation and the cut planes are not read.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL ctx, params, outputs or header; lod out of
 * range; an unknown mode; SVR_MESH_LABELS with selected_count == 0 or selected == NULL; a NaN level (SVR_MESH_LEVEL); a
 * negative box_shape component (with use_box != 0); more than SVR_MESH_MAX_CELLS cells; a NULL array with a non-zero
 * capacity. */
#define SVR_MESH_LABELS 0
#define SVR_MESH_LEVEL  1
#define SVR_MESH_MAX_CELLS (1u << 28)
typedef struct svr_mesh_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: svr_histogram_params' */
    int32_t mode;                       /* SVR_MESH_LABELS or SVR_MESH_LEVEL */
    float   level;                      /* SVR_MESH_LEVEL: inside is v >= level; not NaN */
    const uint32_t* selected;           /* SVR_MESH_LABELS: DEVICE, sorted ascending */
    uint32_t selected_count;            /* SVR_MESH_LABELS: >= 1 */
} svr_mesh_params;
typedef struct svr_mesh_outputs {       /* DEVICE pointers; header required */
    float*    vertices;                 /* 3 * vertex_capacity: x, y, z relative to header[4..6] */
    int32_t*  triangles;                /* 3 * triangle_capacity */
    uint64_t* header;                   /* 8 */
    uint64_t  vertex_capacity;          /* 0: vertices may be NULL */
    uint64_t  triangle_capacity;        /* 0: triangles may be NULL */
} svr_mesh_outputs;
int  svr_mesh(svr_ctx* ctx, const svr_mesh_params* params, const svr_mesh_outputs* out, void* stream);

/* ---- connected components of the resident rings: how many blobs does a level set have, how big is each, where is the
 * biggest, which one lies under a picked point; is a label one piece or five?  (No counterpart in the reference; what a
 * viewer answers today by reading the window back and labelling it on the CPU.)  An addition within ABI version 9: one
 * new symbol and three new structs, nothing older changes.  The window is labelled in HBM (union-find over atomic
 * minima); nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/components_twin.py):
 *   box B       [lo, lo + n): the intersection of box and window exactly as in svr_histogram (use_box, box_off,
 *               box_shape).  A window of None and a box that misses the window give no component.  The texel of voxel
 *               (x, y, z) is ring slot (x % ring_x, y % ring_y, z % ring_z) of the row-major ring (the micro-block copy is
 *               never read).
 *   inside(p)   p is in B, and
 *                 SVR_COMPONENTS_LEVEL   v >= level, v being the density element converted to f32 exactly as svr_mesh
 *                                        converts it.  A NaN is outside.  selected, ignore_zero and join_labels are not
 *                                        read, and every label below reads as 0.
 *                 SVR_COMPONENTS_LABELS  the label texel of p is one of selected[0 .. selected_count) (sorted
 *                                        ascending), or any label when selected_count == 0; and, with ignore_zero != 0,
 *                                        it is not 0: the voxels of label 0 that passed `selected` are outside and are
 *                                        counted in header[13].  Without label rings every label reads as 0.
 *   connect(p, q)  p and q are neighbours under `connectivity` (6: they differ by one on one axis; 26: by at most one on
 *               every axis, and are not equal), both are inside, and, in SVR_COMPONENTS_LABELS with join_labels == 0,
 *               their labels are equal.  Nothing connects across B's border.
 *   component   a class of the transitive closure of connect().  Its FIRST voxel is its smallest in (z, then y, then x)
 *               order.
 *   numbering   components are numbered 1 .. N in ascending order of their first voxels (the numbering of
 *               scipy.ndimage.label).
 *   ids         dense [n_z][n_y][n_x] over B (not ring-shaped): 0 for a voxel that is outside, else the number of its
 *               component.  Written, whole, only when ids_capacity >= n_x n_y n_z; else not touched.
 *   records     N records of 80 bytes in id order.  Written, all of them, only when record_capacity >= N; else not
 *               touched.  sum[] is relative to the window offset (header[4..6]); first, lo and hi are logical voxel
 *               coordinates of the LOD in shader order (x, y, z), lo and hi both inclusive.
 *   header      16 x uint64_t:
 *                 [0] N                          [1] inside voxels
 *                 [2] elements of ids written    [3] records written
 *                 [4..6] the window offset (x, y, z) of the LOD the call used, as int64 bit patterns
 *                 [7..9] B's first voxel (x, y, z), as int64 bit patterns      [10..12] n_x, n_y, n_z
 *                 [13] label-0 voxels dropped by ignore_zero
 *                 [14..15] 0
 *               An empty B gives [7..12] = 0.  The header is overwritten by every call.  Capacities of 0 with NULL
 *               arrays are the count-only call.
 * Everything is an integer and fully specified: two calls on the same rings give identical bytes.  Ordered like svr_mesh:
 * it waits for published uploads, and later uploads are ordered behind it.  Enqueued on `stream`; asynchronous.  The
 * call works in scratch memory owned by the context (8 bytes per voxel of B, grown on demand, SVR_ERR_NOMEM when it
 * cannot be, released by svr_destroy); a call is ordered behind the previous svr_components of the same context,
 * whatever its stream.  The material, the variant, the interpolation and the cut planes are not read.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL ctx, params, outputs or header; lod out of
 * range; an unknown mode; a connectivity other than 6 or 26; a NaN level (SVR_COMPONENTS_LEVEL); selected == NULL with
 * selected_count > 0; a negative box_shape component (with use_box != 0); more than SVR_COMPONENTS_MAX_VOXELS voxels in
 * B; a NULL array with a non-zero capacity. */
#define SVR_COMPONENTS_LABELS 0
#define SVR_COMPONENTS_LEVEL  1
#define SVR_COMPONENTS_MAX_VOXELS (1u << 30)
typedef struct svr_components_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: svr_histogram_params' */
    int32_t mode;                       /* SVR_COMPONENTS_LABELS or SVR_COMPONENTS_LEVEL */
    float   level;                      /* SVR_COMPONENTS_LEVEL: inside is v >= level; not NaN */
    const uint32_t* selected;           /* SVR_COMPONENTS_LABELS: DEVICE, sorted ascending; NULL when the count is 0 */
    uint32_t selected_count;            /* 0: every label */
    int32_t  ignore_zero;               /* SVR_COMPONENTS_LABELS: != 0: label-0 voxels are outside; counted in header[13] */
    int32_t  join_labels;               /* SVR_COMPONENTS_LABELS: != 0: inside neighbours connect whatever their labels */
    int32_t  connectivity;              /* 6 (faces) or 26 (faces, edges, corners) */
} svr_components_params;
typedef struct svr_component_record {   /* 80 bytes */
    uint32_t id;          /* 1 .. N */
    uint32_t label;       /* the label of the first voxel (SVR_COMPONENTS_LEVEL: 0) */
    uint64_t voxels;
    uint64_t sum[3];      /* sum over them of (x - off_x), (y - off_y), (z - off_z); off = header[4..6] */
    int32_t  first[3];    /* the first voxel in (z, y, x) order, as (x, y, z) */
    int32_t  lo[3], hi[3];/* smallest and largest logical voxel coordinate, both inclusive */
    uint32_t reserved;    /* 0 */
} svr_component_record;
typedef struct svr_components_outputs { /* DEVICE pointers; header required */
    uint32_t* ids;                      /* ids_capacity elements */
    uint64_t  ids_capacity;             /* 0: ids may be NULL */
    svr_component_record* records;      /* record_capacity records */
    uint64_t  record_capacity;          /* 0: records may be NULL */
    uint64_t* header;                   /* 16 */
} svr_components_outputs;
int  svr_components(svr_ctx* ctx, const svr_components_params* params, const svr_components_outputs* out, void* stream);

/* ---- exact Euclidean distance transform of the resident rings: how thick is an object, where is its deepest point, what
 * is left of it after eroding by r voxels, what does it touch after dilating by r?  (No counterpart in the reference; what a
 * viewer answers today by reading the window back and running scipy.ndimage.distance_transform_edt on the CPU.)  An
 * addition within ABI version 9: one new symbol and two new structs, nothing older changes.  The squared distances are
 * integers in voxel units, computed in HBM axis by axis; nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/distance_twin.py):
 *   box B       [lo, lo + n): exactly svr_components' (use_box, box_off, box_shape, the ring-slot rule; the micro-block
 *               copy is never read).  A window of None and a box that misses the window give an empty B.
 *   inside(p)   exactly svr_components', with the same two mode constants: SVR_COMPONENTS_LEVEL (v >= level, a NaN is
 *               outside; selected and ignore_zero are not read) or SVR_COMPONENTS_LABELS (selected, selected_count,
 *               ignore_zero; the dropped label-0 voxels are counted in header[13]).  There is no connectivity and no join.
 *   targets, sources
 *               invert == 0: the targets are the inside voxels of B, the sources the voxels of B that are not inside.
 *               invert != 0: the two are swapped: the distance of every outside voxel to the nearest inside one.
 *               invert == 0 and border != 0: every lattice point beyond B is a source too ("everything outside box
 *               and window is outside", as in svr_mesh), so an object that the box or the window cuts is thin there.
 *               border == 0: nothing beyond B is known (the convention of scipy).  invert != 0: border is not read.
 *   d2          dense int32 [n_z][n_y][n_x] over B (not ring-shaped).  For a target p the minimum over the sources q of
 *               (p_x - q_x)^2 + (p_y - q_y)^2 + (p_z - q_z)^2; for a voxel that is no target 0; for a target where
 *               there is no source at all SVR_DISTANCE_FAR.  Written, whole, only when d2_capacity >= n_x n_y n_z;
 *               else not touched, and the call is the count-only call.
 *   limits      every extent of B is at most SVR_DISTANCE_MAX_EXTENT, so that d2 <= 3 * 2^28 fits int32 below
 *               SVR_DISTANCE_FAR, and B holds at most 2^30 voxels.
 *   header      16 x uint64_t:
 *                 [0] targets                    [1] inside voxels
 *                 [2] elements of d2 written     [3] the largest d2 over the targets that are not FAR (0 if none)
 *                 [4..6] the window offset (x, y, z) of the LOD the call used, as int64 bit patterns
 *                 [7..9] B's first voxel (x, y, z), as int64 bit patterns      [10..12] n_x, n_y, n_z
 *                 [13] label-0 voxels dropped by ignore_zero
 *                 [14] the linear index (z n_y + y) n_x + x in B of the first voxel, in (z, y, x) order, that attains
 *                      [3] (0 if none)
 *                 [15] targets whose d2 is FAR
 *               An empty B gives [7..12] = 0.  The header is overwritten by every call.  A capacity of 0 with a NULL
 *               array is the count-only call: it runs the pass over the ring alone, fills [0], [1], [4..13] and leaves
 *               [2], [3], [14], [15] at 0; so does a call whose capacity is too small.
 * Everything is an integer and fully specified, whatever algorithm computes it: two calls on the same rings give
 * identical bytes.  Distances are in voxels of the chosen LOD (no anisotropic spacing); the nearest source itself is
 * not returned (it is not unique at ties; svr_nearest returns it, under a tie rule).  Ordered like svr_components: it waits for published uploads, and later
 * uploads are ordered behind it.  Enqueued on `stream`; asynchronous.  The call works in scratch memory owned by the
 * context (8 bytes and 1 bit per voxel of B, grown on demand, SVR_ERR_NOMEM when it cannot be, released by svr_destroy);
 * a call is ordered behind the previous svr_distance of the same context, whatever its stream.  The material, the
 * variant, the interpolation and the cut planes are not read.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL ctx, params, outputs or header; lod out of
 * range; an unknown mode; a NaN level (SVR_COMPONENTS_LEVEL); selected == NULL with selected_count > 0; a negative
 * box_shape component (with use_box != 0); an extent of B above SVR_DISTANCE_MAX_EXTENT; more than
 * SVR_DISTANCE_MAX_VOXELS voxels in B; a NULL array with a non-zero capacity. */
#define SVR_DISTANCE_FAR 0x7FFFFFFF
#define SVR_DISTANCE_MAX_EXTENT 16384
#define SVR_DISTANCE_MAX_VOXELS (1u << 30)
typedef struct svr_distance_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: svr_histogram_params' */
    int32_t mode;                       /* SVR_COMPONENTS_LABELS or SVR_COMPONENTS_LEVEL */
    float   level;                      /* SVR_COMPONENTS_LEVEL: inside is v >= level; not NaN */
    const uint32_t* selected;           /* SVR_COMPONENTS_LABELS: DEVICE, sorted ascending; NULL when the count is 0 */
    uint32_t selected_count;            /* 0: every label */
    int32_t  ignore_zero;               /* SVR_COMPONENTS_LABELS: != 0: label-0 voxels are outside; counted in header[13] */
    int32_t  invert;                    /* != 0: targets and sources are swapped */
    int32_t  border;                    /* invert == 0: != 0: every lattice point beyond B is a source */
} svr_distance_params;
typedef struct svr_distance_outputs {   /* DEVICE pointers; header required */
    int32_t*  d2;                       /* d2_capacity elements */
    uint64_t  d2_capacity;              /* 0: d2 may be NULL */
    uint64_t* header;                   /* 16 */
} svr_distance_outputs;
int  svr_distance(svr_ctx* ctx, const svr_distance_params* params, const svr_distance_outputs* out, void* stream);

/* ---- nearest source of every voxel (the exact feature transform): which object is this background voxel nearest to, what
 * are the objects grown by r voxels without merging them (skimage.segmentation.expand_labels: the Voronoi partition of
 * the labels), which surface voxel lies nearest a picked point?  (No counterpart in the reference; what a viewer answers
 * today by reading the window back and running scipy.ndimage.distance_transform_edt(return_indices=True) on the CPU.)  An
 * addition within ABI version 9: one new symbol and two new structs, nothing older changes.
 * Defined HERE (numpy restatement: tests/nearest_twin.py):
 *   params      the fields of svr_distance_params but for border, with their meanings.  B, inside(), targets and sources
 *               are svr_distance's with border == 0: nothing beyond B is a source, a lattice point beyond B has no voxel
 *               to name.
 *   d2, header  byte for byte what svr_distance gives for the same parameters with border = 0, all 16 words.
 *   index       dense int32 [n_z][n_y][n_x] over B.  index[i] is, for a voxel that is no target (a source), i itself;
 *               for a target with at least one source, the dense index (z n_y + y) n_x + x in B of the nearest source;
 *               for a target whose d2 is SVR_DISTANCE_FAR, -1.
 *   tie rule    among the sources at the minimum distance, the one with the smallest dense index wins.  This is stated
 *               without reference to an algorithm and makes the answer unique: two calls give identical bytes.
 *   label       dense uint32 over B: the label ring's value at voxel index[i]; 0 where index[i] == -1; 0 everywhere in
 *               a context without label rings.  Defined in both modes.  With SVR_COMPONENTS_LABELS, invert != 0,
 *               selected_count == 0 and ignore_zero != 0 every label-0 voxel gets the label of the nearest object and
 *               an object voxel keeps its own.  label may always be NULL and is then not written.
 *   capacity    in elements, common to the three arrays.  They are written, whole, only when capacity >= n_x n_y n_z;
 *               otherwise nothing is touched and the call is svr_distance's count-only call, with the same header
 *               words left at 0.
 * Ordered like svr_distance, whose scratch memory it shares (14 bytes and 1 bit per voxel of B here): a call is ordered
 * behind the previous svr_distance or svr_nearest of the same context, whatever its stream.
 * Not in it: anisotropic spacing; sources beyond the box; writing the grown labels back into a label ring
 * (svr_upload_region_device with labels alone takes a device array, and the wrap split of a logical box is the caller's).
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for what svr_distance refuses, and for a NULL d2 or
 * index with a non-zero capacity.  The error texts start with "svr_nearest: ". */
typedef struct svr_nearest_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: svr_histogram_params' */
    int32_t mode;                       /* SVR_COMPONENTS_LABELS or SVR_COMPONENTS_LEVEL */
    float   level;                      /* SVR_COMPONENTS_LEVEL: inside is v >= level; not NaN */
    const uint32_t* selected;           /* SVR_COMPONENTS_LABELS: DEVICE, sorted ascending; NULL when the count is 0 */
    uint32_t selected_count;            /* 0: every label */
    int32_t  ignore_zero;               /* SVR_COMPONENTS_LABELS: != 0: label-0 voxels are outside; counted in header[13] */
    int32_t  invert;                    /* != 0: targets and sources are swapped */
} svr_nearest_params;
typedef struct svr_nearest_outputs {    /* DEVICE pointers; header required */
    int32_t*  d2;                       /* capacity elements */
    int32_t*  index;                    /* capacity elements */
    uint32_t* label;                    /* capacity elements, or NULL: not written */
    uint64_t  capacity;                 /* 0: d2 and index may be NULL */
    uint64_t* header;                   /* 16 */
} svr_nearest_outputs;
int  svr_nearest(svr_ctx* ctx, const svr_nearest_params* params, const svr_nearest_outputs* out, void* stream);

/* ---- contacts between resident objects: what does an object touch, over how much surface, where, and what does the
 * data look like along that contact?  (No counterpart in the reference; the region adjacency graph of a segmentation:
 * the neighbours of a picked object, its free and total surface, the edge scores of proof-reading and agglomeration.)
 * An addition within ABI version 9: one new symbol and three new structs, nothing older changes.  One streaming pass
 * over the label ring in HBM fills a table of records, one per unordered pair of touching labels; the density ring is
 * read only beside a face; nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/contacts_twin.py):
 *   voxels B    exactly svr_objects' voxels before its label filters: the logical voxels (x, y, z) of LOD `lod` in the
 *               intersection of box and window, read from ring slot (x % ring_x, y % ring_y, z % ring_z) of the
 *               row-major ring (the micro-block copy is never read); without label rings every label reads as 0.  A
 *               window of None and a box that misses the window hold no voxel.
 *   face        a voxel p of B, an axis k of x, y, z, and q = p + e_k also in B, with L(p) != L(q).  The face is owned
 *               by p, so every face is seen once.  Nothing beyond B is known: a voxel on the border of box or window
 *               has no face outward.  The pair is unordered: label_lo = min(L(p), L(q)), label_hi = max(L(p), L(q)),
 *               and always label_lo < label_hi.
 *   considered  with selected_count > 0, only the faces of which at least one label is one of
 *               selected[0 .. selected_count).  Then, with ignore_zero != 0, the faces with label_lo == 0 are dropped:
 *               they are counted in header[3] and nowhere else.
 *   records     `capacity` records of 112 bytes.  One record per distinct considered pair that found a slot, in no
 *               particular order; every byte of an unused record is 0.  The first 8 bytes, label_lo then label_hi as
 *               one little-endian u64, are the key: label_hi >= 1 always, so the key of a pair is never 0 and 0 means
 *               empty; there is no `used` word.  Labels 0 and 0xFFFFFFFF are ordinary labels.
 *   header      8 x uint64_t:
 *                 [0] occupied records
 *                 [1] considered faces
 *                 [2] overflow: the considered faces whose pair found no slot
 *                 [3] faces dropped by ignore_zero (they passed `selected`; not part of [1])
 *                 [4..6] the window offset (x, y, z) of the LOD the call used, as int64 bit patterns; sum2[] is relative to it
 *                 [7] the voxels of B
 *   slots       an insertion can reach every record (linear probing over the whole table), so header[2] != 0 if and
 *               only if more than `capacity` distinct pairs are considered.  Then exactly `capacity` records are
 *               occupied, every one of them is complete and exact for its pair (a pair that owns a record never
 *               loses faces), and sum(faces[0] + faces[1] + faces[2]) + header[2] == header[1].  Which pairs got
 *               records is unspecified.
 *   value       the raw ring element; every face offers two, v(p) and v(q).  u8 / u16 rings: value_sum is the u64 sum,
 *               finite == 2 * (faces[0] + faces[1] + faces[2]), vmin / vmax the extremes as f32 (exact).  float32
 *               rings: only finite values count in finite, value_sum, vmin and vmax; value_sum holds the BITS of an
 *               f64 sum whose every partial sum is held in f64.
 * The call OVERWRITES its outputs: it zeroes them on `stream`, then fills them.  Every field is an integer sum, a
 * minimum or a maximum, but value_sum on float32 rings (f64 additions in any order): on integer rings the result does
 * not depend on the order in which the device visits the faces.  A render-thread call ordered like svr_objects: it
 * waits for published uploads, and later uploads are ordered behind it.  Enqueued on `stream`; asynchronous.  The
 * material, the variant, the interpolation and the cut planes are not read.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL ctx, params, outputs, records or
 * header; lod out of range; capacity 0 or above SVR_CONTACTS_MAX_CAPACITY; a negative box_shape component (with
 * use_box != 0); selected == NULL with selected_count > 0. */
#define SVR_CONTACTS_MAX_CAPACITY (1u << 26)
typedef struct svr_contacts_params {
    int32_t lod;
    int32_t use_box;                    /* 0: the LOD's whole resident window */
    int32_t box_off[3], box_shape[3];   /* LOD-l logical voxels, shader order: svr_objects_params' */
    const uint32_t* selected;           /* DEVICE, sorted ascending; NULL when the count is 0 */
    uint32_t selected_count;            /* 0: every face */
    int32_t  ignore_zero;               /* != 0: faces with label 0 take no part; they are counted in header[3] */
    uint32_t capacity;                  /* records in svr_contacts_outputs::records, 1 .. SVR_CONTACTS_MAX_CAPACITY (any integer) */
} svr_contacts_params;
typedef struct svr_contact_record {
    uint32_t label_lo, label_hi;  /* lo < hi; both 0: empty record, every byte of it is 0 */
    uint64_t faces[3];            /* considered faces of the pair whose normal is x, y, z */
    uint64_t sum2[3];             /* sum over the faces of 2 * (p - off) + e_k, per axis (x, y, z): twice the face
                                     centre's coordinate relative to the window offset header[4..6], an integer */
    int32_t  lo[3], hi[3];        /* smallest and largest coordinate of the owning voxel p, inclusive, shader order, LOD voxels */
    uint64_t finite;              /* face-voxel values that are finite: each face offers v(p) and v(q) */
    uint64_t value_sum;           /* u8 / u16 rings: u64 sum of those raw values; float32 rings: the BITS of an f64 sum */
    float    vmin, vmax;          /* over those values; (+inf, -inf) when finite == 0 */
    uint64_t reserved;            /* 0 */
} svr_contact_record;             /* 112 bytes */
typedef struct svr_contacts_outputs {   /* DEVICE pointers, both required */
    svr_contact_record* records;        /* capacity */
    uint64_t* header;                   /* 8 */
} svr_contacts_outputs;
int  svr_contacts(svr_ctx* ctx, const svr_contacts_params* params, const svr_contacts_outputs* out, void* stream);

/* ---- split touching objects: the watershed of a height field, normally the d2 of svr_distance: which of the objects
 * that touch in one blob of a level set is this voxel part of, how many are there, where is the deepest point of each?
 * (No counterpart in the reference; the last step of threshold, distance transform, watershed, which a viewer runs today
 * on the CPU after reading the distance field back.)  An addition within ABI version 9: one new symbol and three new
 * structs, nothing older changes.  The positive voxels of the field are partitioned in HBM into regions, one per
 * significant summit; nothing is copied to the host.
 * Defined HERE (numpy restatement: tests/split_twin.py):
 *   height      a DEVICE pointer to int32 [n_z][n_y][n_x], dense over a box B of n[0] x n[1] x n[2] = n_x x n_y x n_z
 *               voxels, at most SVR_SPLIT_MAX_VOXELS; voxel (x, y, z) has the linear index i = (z n_y + y) n_x + x.
 *               The call reads no ring: B is the caller's, usually header[10..12] of the svr_distance call that wrote
 *               the field.  Nothing beyond B exists.
 *   inside(i)   height[i] > 0: the negative half of a signed field is outside.  SVR_DISTANCE_FAR is an ordinary value
 *               (a plateau).
 *   neighbours  under `connectivity`, 6 (they differ by one on one axis) or 26 (by at most one on every axis, and are
 *               not equal); it governs both the ascent and the links.
 *   order       i BEATS j iff height[i] > height[j], or the two are equal and i < j: a strict total order.
 *   ascent      up(i) is the voxel that beats all others among i and its neighbours in B (an outside neighbour has a
 *               height <= 0 and never wins); summit(i) is the fixed point of up from i, which exists because every
 *               step of the chain beats the one before.  A BASIN is the set of inside voxels that share one summit S;
 *               peak(S) = height[S].
 *   links       two neighbouring inside voxels p, q with different summits LINK their basins iff, with
 *                 s = min(height[p], height[q]),  a = min(peak(summit(p)), peak(summit(q)))  (always a >= s),
 *                 H = merge_squared,  t = a - s - H:      t <= 0  or  t * t <= 4 * H * s      in 64-bit integers,
 *               which is exactly sqrt(a) - sqrt(s) <= sqrt(H): the lower of the two peaks stands less than sqrt(H)
 *               above the pass.  H <= SVR_SPLIT_MAX_MERGE keeps both sides at or below 2^62.  The test reads the field
 *               and the summits of the ascent alone, never another link, and it is monotone in s, so the highest pass
 *               between two basins passes it iff any pair of voxels between them does.  With H = 0 basins of equal peak
 *               that meet at that height still link: a plateau of any shape is one region.
 *   regions     the classes of the transitive closure of the links.  The SEED of a region is its smallest summit index;
 *               regions are numbered 1 .. N in ascending order of their seeds.  Its TOP is the summit of it that beats
 *               its others: the region's deepest point.
 *   ids         dense uint32 [n_z][n_y][n_x] over B: 0 for a voxel that is outside, else the number of its region.
 *               Written, whole, only when ids_capacity >= n_x n_y n_z; else not touched.
 *   records     N records of 80 bytes in id order.  Written, all of them, only when record_capacity >= N; else not
 *               touched.  Every coordinate is relative to B, in shader order (x, y, z); lo and hi are both inclusive.
 *   header      16 x uint64_t:
 *                 [0] N                          [1] inside voxels
 *                 [2] elements of ids written    [3] records written
 *                 [4] basins                     [5..9] 0
 *                 [10..12] n_x, n_y, n_z         [13..15] 0
 *               The header is overwritten by every call.  Capacities of 0 with NULL arrays are the count-only call.
 * Everything is an integer and fully specified: the result does not depend on the order in which the device visits the
 * voxels, and two calls on the same field give identical bytes.  Enqueued on `stream`; asynchronous.  The call reads no
 * ring, so no ordering against uploads is promised: the caller orders it behind whatever wrote `height`, as usual for a
 * stream.  It works in scratch memory owned by the context (12 bytes per voxel of B, grown on demand, SVR_ERR_NOMEM when
 * it cannot be, released by svr_destroy); a call is ordered behind the previous svr_split of the same context, whatever
 * its stream.  The material, the variant, the interpolation and the cut planes are not read.
 * Not in this call: heights read from the density ring (an intensity watershed); regions that stop at label borders;
 * markers given by the caller; the h-maxima hierarchy (the link rule is ONE round on the original basins, and links can
 * chain); writing the regions back into a label ring.
 * SVR_ERR_INVALID, with nothing enqueued and the outputs untouched, for: a NULL ctx, params, outputs, header or height;
 * a connectivity other than 6 or 26; merge_squared above SVR_SPLIT_MAX_MERGE; an extent <= 0 or more than
 * SVR_SPLIT_MAX_VOXELS voxels; a NULL array with a non-zero capacity. */
#define SVR_SPLIT_MAX_VOXELS (1u << 30)
#define SVR_SPLIT_MAX_MERGE  (1u << 29)
typedef struct svr_split_params {
    const int32_t* height;              /* DEVICE, n[2] x n[1] x n[0] elements, x fastest */
    int32_t  n[3];                      /* n_x, n_y, n_z: each > 0, the product at most SVR_SPLIT_MAX_VOXELS */
    int32_t  connectivity;              /* 6 (faces) or 26 (faces, edges, corners) */
    uint32_t merge_squared;             /* H, at most SVR_SPLIT_MAX_MERGE */
    uint32_t reserved;                  /* not read */
} svr_split_params;
typedef struct svr_split_record {       /* 80 bytes */
    uint32_t id;          /* 1 .. N */
    uint32_t basins;      /* the summits of the region */
    uint64_t voxels;
    uint64_t sum[3];      /* sum over them of x, y, z in B */
    int32_t  top[3];      /* the region's best summit, as (x, y, z) in B */
    int32_t  lo[3], hi[3];/* smallest and largest coordinate in B, both inclusive */
    int32_t  peak;        /* height at top */
} svr_split_record;
typedef struct svr_split_outputs {      /* DEVICE pointers; header required */
    uint32_t* ids;                      /* ids_capacity elements */
    uint64_t  ids_capacity;             /* 0: ids may be NULL */
    svr_split_record* records;          /* record_capacity records */
    uint64_t  record_capacity;          /* 0: records may be NULL */
    uint64_t* header;                   /* 16 */
} svr_split_outputs;
int  svr_split(svr_ctx* ctx, const svr_split_params* params, const svr_split_outputs* out, void* stream);

/* ---- sync */
int  svr_sync(svr_ctx* ctx);                 /* both streams idle */
int  svr_sync_uploads(svr_ctx* ctx);         /* upload stream idle */
/* raw device pointers of one LOD's ring textures (for diagnostics / RCCL) */
int  svr_lod_device_ptrs(svr_ctx* ctx, int lod, void** density, void** labels);
/* the micro-block copy of the LOD's density ring (svr_lod_desc::blocked_twin), or NULL: tests compare it with the ring */
int  svr_lod_twin_ptr(svr_ctx* ctx, int lod, void** twin);
/* The macro-cell maxima of the LOD's density ring, which decide where the LMIP march and the iso kernel skip empty
 * space: two DEVICE tables of cdim[2] x cdim[1] x cdim[0] elements of the ring's type (u8 / u16 / f32), x fastest,
 * over cells of S^3 ring slots, S = 1 << *cshift (8 at LOD 0, 4 at the coarser LODs).  Once the upload stream is idle:
 *   raw[cz][cy][cx] = fmax over the S^3 slots of the cell of |ring|, starting from 0 (a NaN never wins)
 *   blk[cz][cy][cx] = max of raw[(cz+dz) % cdim[2]][(cy+dy) % cdim[1]][(cx+dx) % cdim[0]], d* in {0, 1}
 * EXACTLY, over the ring as it lies in memory: a slot counts whether or not the published ROI maps it, stale slots of
 * chunks that left the window too.  Holds after any sequence of svr_upload_region, svr_upload_region_device and
 * svr_clear_lod (which zeroes both).  The kernels read blk.  A LOD whose ring extents are not all multiples of 8 has
 * no tables: *raw = *blk = NULL (cdim and *cshift are still written).  Tests compare the tables with the ring. */
int  svr_lod_cell_ptrs(svr_ctx* ctx, int lod, void** raw, void** blk, int32_t cdim[3], int32_t* cshift);

/* diagnostics: batch census accumulated by instrumented renders (outputs.steps != NULL):
 * [0] general batches, [1] direct fast batches, [2] brick batches, [3] brick slabs, [4] runs,
 * [5] all-zero batches, [6] waves, [7] batches skipped as empty space; batches are per wave, 8 iterations each */
int  svr_debug_counters(svr_ctx* ctx, uint32_t out[8], int reset);
/* diagnostics: shader-clock cycles of wave residency per kernel section, summed over the waves of the
 * instrumented renders: [0] prologue (ray set-up, event search), [1] span refresh + run length, [2] general
 * batches, [3] brick slab set-up + load issue, [4] wait for the brick loads, [5] brick batches, [6] direct
 * batches, [7] epilogue (shading, stores); [8..14] finer splits used while tuning (see march_kernel.hip);
 * [15] is a COUNT, not cycles: the direct batches that gathered from a micro-block copy (svr_lod_desc::blocked_twin) */
int  svr_debug_timers(svr_ctx* ctx, uint64_t out[16], int reset);

/* timing helper: run `iters` back-to-back renders on the context's render
 * stream bracketed by HIP events on that same stream; returns the average
 * kernel time in milliseconds (used by bench.py's roofline block). */
int  svr_time_render(svr_ctx* ctx, const svr_camera* cam, const svr_frame* frame,
                     const svr_outputs* out, int iters, float* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* SVR_H */
