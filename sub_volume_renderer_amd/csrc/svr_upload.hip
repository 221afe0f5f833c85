// Uploads of the C ABI (include/svr.h): host blocks through the pinned staging slots, device blocks directly, and what
// orders, counts and reads back what was uploaded.
#include <string.h>

#include <algorithm>
#include <chrono>

#include "svr_host.h"
#include "pack_rows.h"

// How a region is cut into staged blocks (tests/test_gpu_macro_cells.py reads these three to prove which path a shape takes)
static const size_t kStagingSlotBytes = (size_t)48 << 20;     // per slot; 3 slots -> 144 MiB pinned
static const size_t kMinBlockBytes = (size_t)4 << 20;         // the smallest staging block
static const size_t kBlocksPerRegion = 8;                     // a block is about this fraction of the region

static int ensure_staging(svr_ctx* c) {
    if (c->slot_bytes) return SVR_OK;
    const size_t bytes = kStagingSlotBytes;
    for (auto& s : c->slot) {
        if (hipHostMalloc(&s.host, bytes, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&s.dev, bytes) != hipSuccess ||
            hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) {
            svr_set_error("staging allocation failed");
            return SVR_ERR_NOMEM;
        }
        s.used = false;
    }
    c->slot_bytes = bytes;
    return SVR_OK;
}

// The ring half of a scatter into LOD lod; the source half, dst_off, shape and packed are the caller's.
static ScatterArgs scatter_args_of(const svr_ctx* c, int lod) {
    const LodStorage& L = c->lod[lod];
    ScatterArgs a;
    a.ring_density = L.density; a.ring_labels = L.labels; a.ring_storage = c->density_storage; a.ring_twin = L.twin;
    for (int i = 0; i < 3; ++i) a.ring[i] = L.ring[i];
    return a;
}

// Scatter one block into a LOD's rings and bring the macro-cell maxima of the touched cells up to date
// (same stream, right behind the scatter: a render that can see the new voxels sees their maxima too).
static hipError_t scatter_into_ring(svr_ctx* c, int lod, const ScatterArgs& a, bool wrote_density) {
    hipError_t e = svr_launch_scatter(a, c->upload_stream);
    const LodStorage& L = c->lod[lod];
    if (e == hipSuccess && wrote_density && L.cells_raw)
        e = svr_launch_cell_update(L.density, c->density_storage, L.ring, L.cells_raw, L.cells_dil, L.cdim, L.cshift,
                                   a.dst_off, a.shape, c->upload_stream);
    return e;
}

extern "C" {

int svr_upload_region(svr_ctx* c, int lod, const int32_t dst_off[3], const int32_t shape[3],
                      const void* density, int density_dtype, const int64_t density_strides[3],
                      const void* labels, int labels_dtype, const int64_t labels_strides[3]) {
    int rc = check_region(c, lod, dst_off, shape, "svr_upload_region");
    if (rc) return rc;
    const size_t des = density ? svr_dtype_size(density_dtype) : 0;
    const size_t les = labels ? svr_dtype_size(labels_dtype) : 0;
    SVR_REQUIRE(!density || (des && density_strides), "svr_upload_region: bad density dtype/strides");
    SVR_REQUIRE(!labels || (les && labels_strides), "svr_upload_region: bad labels dtype/strides");
    if (!density && !labels) return SVR_OK;
    SVR_REQUIRE(!labels || !c->no_labels, "svr_upload_region: the context was created without label rings (no_labels)");
    SVR_REQUIRE(!density || storage_accepts(c->density_storage, density_dtype),
                "svr_upload_region: the context's integer density storage only accepts sources of that same dtype");
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return SVR_OK;
    DeviceGuard guard(c->device);
    // one uploader at a time: the staging slots and the enqueue order on the upload stream are shared
    // (the render thread may load synchronously while the streaming worker is inside this call)
    std::lock_guard<std::mutex> upload_lock(c->upload_mu);
    struct Clock {                                          // time inside this call, for svr_upload_stats
        svr_ctx* c; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~Clock() { c->upload_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    } clock{ c };
    rc = ensure_staging(c);
    if (rc) return rc;
    rc = uploads_after_render(c);
    if (rc) return rc;
    // The region travels in blocks of whole rows, as many as fit a staging slot: whole z-planes when one
    // fits (the scatter kernel then sees a box), else runs of rows inside one plane.  Labels are placed
    // after the density block, 16-byte aligned.
    const size_t row_bytes = (size_t)shape[0] * (des + les);
    SVR_REQUIRE(row_bytes + 32 <= c->slot_bytes, "svr_upload_region: one row of the region exceeds the staging slot");
    // Blocks of about an eighth of the region (4 MiB .. one slot): the pack of block k+1 runs while block k is on
    // the bus and block k-1 is being scattered, so a region of one or two slots' worth still overlaps the three.
    const size_t region_bytes = row_bytes * (size_t)shape[1] * (size_t)shape[2];
    size_t block_bytes = std::min(c->slot_bytes - 32, std::max<size_t>(kMinBlockBytes, region_bytes / kBlocksPerRegion));
    if (const int mib = svr_exp_env_int("SVR_UPLOAD_BLOCK_MIB", 0)) block_bytes = std::min(c->slot_bytes - 32, std::max<size_t>(1, (size_t)mib) << 20);
    const int64_t rows_max = std::max<int64_t>(1, (int64_t)(block_bytes / row_bytes));
    const int64_t plane_rows = shape[1];
    const int64_t total_rows = plane_rows * shape[2];
    ScatterArgs a = scatter_args_of(c, lod);
    a.density_dtype = density_dtype; a.labels_dtype = labels_dtype; a.packed = 1;
    for (int64_t r0 = 0; r0 < total_rows;) {
        int64_t nrows;
        if (rows_max >= plane_rows && r0 % plane_rows == 0)
            nrows = std::min(total_rows - r0, (rows_max / plane_rows) * plane_rows);        // whole planes
        else
            nrows = std::min(rows_max, plane_rows - r0 % plane_rows);                        // rows of one plane
        const int64_t r1 = r0 + nrows;
        StagingSlot& S = c->slot[c->next_slot];
        c->next_slot = (c->next_slot + 1) % svr_ctx::kSlots;
        if (S.used) SVR_HIP_TRY(hipEventSynchronize(S.done));
        const size_t dbytes = (size_t)shape[0] * (size_t)nrows * des;
        const size_t lofs = (dbytes + 15) & ~(size_t)15;
        const size_t lbytes = (size_t)shape[0] * (size_t)nrows * les;
        pack_rows(static_cast<const char*>(density), des, density_strides, static_cast<char*>(S.host),
                  static_cast<const char*>(labels), les, labels_strides, static_cast<char*>(S.host) + lofs, shape, r0, r1);
        SVR_HIP_TRY(hipMemcpyAsync(S.dev, S.host, lofs + lbytes, hipMemcpyHostToDevice, c->upload_stream));
        // the staged block as a box of the ring
        const int32_t z0 = (int32_t)(r0 / plane_rows), y0 = (int32_t)(r0 % plane_rows);
        const int32_t bz = nrows >= plane_rows ? (int32_t)(nrows / plane_rows) : 1;
        const int32_t by = nrows >= plane_rows ? shape[1] : (int32_t)nrows;
        a.src_density = density ? S.dev : nullptr;
        a.dstride[0] = (int64_t)des; a.dstride[1] = (int64_t)des * shape[0]; a.dstride[2] = (int64_t)des * shape[0] * by;
        a.src_labels = labels ? static_cast<char*>(S.dev) + lofs : nullptr;
        a.lstride[0] = (int64_t)les; a.lstride[1] = (int64_t)les * shape[0]; a.lstride[2] = (int64_t)les * shape[0] * by;
        a.dst_off[0] = dst_off[0]; a.dst_off[1] = dst_off[1] + y0; a.dst_off[2] = dst_off[2] + z0;
        a.shape[0] = shape[0]; a.shape[1] = by; a.shape[2] = bz;
        SVR_HIP_TRY(scatter_into_ring(c, lod, a, density != nullptr));
        SVR_HIP_TRY(hipEventRecord(S.done, c->upload_stream));
        S.used = true;
        c->staged_bytes += lofs + lbytes;
        r0 = r1;
    }
    return SVR_OK;
}

int svr_upload_region_device(svr_ctx* c, int lod, const int32_t dst_off[3], const int32_t shape[3],
                             const void* density, int density_dtype, const int64_t density_strides[3],
                             const void* labels, int labels_dtype, const int64_t labels_strides[3]) {
    int rc = check_region(c, lod, dst_off, shape, "svr_upload_region_device");
    if (rc) return rc;
    SVR_REQUIRE(!density || (svr_dtype_size(density_dtype) && density_strides), "svr_upload_region_device: bad density dtype/strides");
    SVR_REQUIRE(!labels || (svr_dtype_size(labels_dtype) && labels_strides), "svr_upload_region_device: bad labels dtype/strides");
    if (!density && !labels) return SVR_OK;
    SVR_REQUIRE(!labels || !c->no_labels, "svr_upload_region_device: the context was created without label rings (no_labels)");
    SVR_REQUIRE(!density || storage_accepts(c->density_storage, density_dtype),
                "svr_upload_region_device: the context's integer density storage only accepts sources of that same dtype");
    DeviceGuard guard(c->device);
    std::lock_guard<std::mutex> upload_lock(c->upload_mu);
    rc = uploads_after_render(c);
    if (rc) return rc;
    ScatterArgs a = scatter_args_of(c, lod);
    a.packed = 0;
    a.src_density = density; a.density_dtype = density_dtype;
    a.src_labels = labels; a.labels_dtype = labels_dtype;
    for (int i = 0; i < 3; ++i) {
        a.dstride[i] = density ? density_strides[i] : 0;
        a.lstride[i] = labels ? labels_strides[i] : 0;
        a.dst_off[i] = dst_off[i]; a.shape[i] = shape[i];
    }
    SVR_HIP_TRY(scatter_into_ring(c, lod, a, density != nullptr));
    return SVR_OK;
}

int svr_publish_uploads(svr_ctx* c) {
    SVR_REQUIRE(c, "svr_publish_uploads: null ctx");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(hipEventRecord(c->uploads_published, c->upload_stream));
    c->have_published = true;
    return SVR_OK;
}

int svr_mark_uploads(svr_ctx* c) {
    SVR_REQUIRE(c, "svr_mark_uploads: null ctx");
    DeviceGuard guard(c->device);
    SVR_HIP_TRY(hipEventRecord(c->uploads_marker, c->upload_stream));
    c->marker_set = true;
    return SVR_OK;
}

int svr_uploads_pending(svr_ctx* c, int* pending) {
    SVR_REQUIRE(c && pending, "svr_uploads_pending: null argument");
    *pending = 0;
    if (!c->marker_set) return SVR_OK;
    DeviceGuard guard(c->device);
    const hipError_t e = hipEventQuery(c->uploads_marker);
    if (e == hipErrorNotReady) { *pending = 1; return SVR_OK; }
    SVR_HIP_TRY(e);
    return SVR_OK;
}

int svr_upload_stats(svr_ctx* c, uint64_t* staged_bytes, double* seconds_in_calls, int reset) {
    SVR_REQUIRE(c, "svr_upload_stats: null ctx");
    std::lock_guard<std::mutex> upload_lock(c->upload_mu);
    if (staged_bytes) *staged_bytes = c->staged_bytes;
    if (seconds_in_calls) *seconds_in_calls = c->upload_seconds;
    if (reset) { c->staged_bytes = 0; c->upload_seconds = 0.0; }
    return SVR_OK;
}

int svr_upload_ticket(svr_ctx* c, uint64_t* ticket) {
    SVR_REQUIRE(c && ticket, "svr_upload_ticket: null argument");
    DeviceGuard guard(c->device);
    std::lock_guard<std::mutex> upload_lock(c->upload_mu);      // behind whatever an uploader is enqueueing right now
    std::lock_guard<std::mutex> lock(c->ticket_mu);
    hipEvent_t& ev = c->tickets[c->next_ticket % svr_ctx::kTickets];
    if (!ev) SVR_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    SVR_HIP_TRY(hipEventRecord(ev, c->upload_stream));
    *ticket = c->next_ticket++;
    return SVR_OK;
}

int svr_ticket_pending(svr_ctx* c, uint64_t ticket, int* pending) {
    SVR_REQUIRE(c && pending, "svr_ticket_pending: null argument");
    *pending = 0;
    std::lock_guard<std::mutex> lock(c->ticket_mu);
    SVR_REQUIRE(ticket >= 1 && ticket < c->next_ticket, "svr_ticket_pending: no such ticket");
    // a recycled slot holds a LATER event of the same stream: done there implies done here
    DeviceGuard guard(c->device);
    const hipError_t e = hipEventQuery(c->tickets[ticket % svr_ctx::kTickets]);
    if (e == hipErrorNotReady) { *pending = 1; return SVR_OK; }
    SVR_HIP_TRY(e);
    return SVR_OK;
}

int svr_clear_lod(svr_ctx* c, int lod) {
    SVR_REQUIRE(c, "svr_clear_lod: null ctx");
    SVR_REQUIRE(lod >= 0 && lod < c->num_lods, "svr_clear_lod: lod out of range");
    DeviceGuard guard(c->device);
    int rc = uploads_after_render(c);
    if (rc) return rc;
    LodStorage& L = c->lod[lod];
    std::lock_guard<std::mutex> upload_lock(c->upload_mu);
    SVR_HIP_TRY(hipMemsetAsync(L.density, 0, L.voxels * svr_dtype_size(c->density_storage), c->upload_stream));
    if (L.twin) SVR_HIP_TRY(hipMemsetAsync(L.twin, 0, L.voxels * svr_dtype_size(c->density_storage), c->upload_stream));
    if (L.labels) SVR_HIP_TRY(hipMemsetAsync(L.labels, 0, L.voxels * sizeof(uint32_t), c->upload_stream));
    if (L.cells_raw) {
        const size_t cb = (size_t)L.cdim[0] * L.cdim[1] * L.cdim[2] * svr_dtype_size(c->density_storage);
        SVR_HIP_TRY(hipMemsetAsync(L.cells_raw, 0, cb, c->upload_stream));
        SVR_HIP_TRY(hipMemsetAsync(L.cells_dil, 0, cb, c->upload_stream));
    }
    return SVR_OK;
}

int svr_read_region(svr_ctx* c, int lod, const int32_t off[3], const int32_t shape[3],
                    float* density_out, uint32_t* labels_out) {
    int rc = check_region(c, lod, off, shape, "svr_read_region");
    if (rc) return rc;
    const size_t n = (size_t)shape[0] * (size_t)shape[1] * (size_t)shape[2];
    if (n == 0 || (!density_out && !labels_out)) return SVR_OK;
    DeviceGuard guard(c->device);
    LodStorage& L = c->lod[lod];
    float* dtmp = nullptr; uint32_t* ltmp = nullptr;
    if (labels_out && !L.labels) {                     // no label rings: every label reads as 0
        memset(labels_out, 0, n * sizeof(uint32_t));
        labels_out = nullptr;
        if (!density_out) return SVR_OK;
    }
    SVR_HIP_TRY(hipStreamSynchronize(c->upload_stream));
    if (density_out) SVR_HIP_TRY(hipMalloc((void**)&dtmp, n * sizeof(float)));
    if (labels_out && hipMalloc((void**)&ltmp, n * sizeof(uint32_t)) != hipSuccess) {
        if (dtmp) (void)hipFree(dtmp);
        svr_set_error("svr_read_region: out of device memory"); return SVR_ERR_NOMEM;
    }
    hipError_t e = svr_launch_gather(L.density, c->density_storage, L.labels, L.ring, off, shape, dtmp, ltmp, c->upload_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->upload_stream);
    if (e == hipSuccess && dtmp) e = hipMemcpy(density_out, dtmp, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && ltmp) e = hipMemcpy(labels_out, ltmp, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (dtmp) (void)hipFree(dtmp);
    if (ltmp) (void)hipFree(ltmp);
    if (e != hipSuccess) { svr_set_error(std::string("svr_read_region: ") + hipGetErrorString(e)); return SVR_ERR_HIP; }
    return SVR_OK;
}

}  // extern "C"
