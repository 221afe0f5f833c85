// How the march reaches one LOD's density ring: through one buffer resource, or, for a ring of 4 GiB or more, through
// up to 8 resources of `zsplit` whole ring z planes each (LodParams::nparts / zsplit / part_bytes / rbytes_last in
// svr_internal.h).  Plain host C++ on plain integers, so that a test can compile it without HIP: svr_render.hip decides the
// split here and nowhere else.
#pragma once

#include <stdint.h>

struct RingParts {
    uint32_t nparts;        // resources the ring is reached through (1: one resource holds the whole ring)
    uint32_t zsplit;        // ring z planes per part (the last part holds the rest); ring z where nparts == 1
    uint32_t part_bytes;    // part p starts p * part_bytes into the ring (0 where nparts == 1)
    uint32_t rbytes;        // size of the resource of a full part (of the whole ring + 64 bytes where nparts == 1)
    uint32_t rbytes_last;   // size of the resource of the last part: its bytes + 64 of slack
    bool span_ok;           // the span kernel can address the ring: nparts <= 8, row index and row pitch below 2^24
    bool twin_ok;           // the march may gather from the micro-block copy through these parts: every part holds whole
                            // blocks of it (include/svr.h, svr_lod_desc::blocked_twin); false where there is no copy
};

// rx, ry, rz: ring extents (shader order x, y, z); esize: bytes per density element (1, 2 or 4); twin: the LOD keeps a
// micro-block copy; force_zsplit: parts of (at least) that many planes for rings of any size (-DSVR_EXPERIMENTS
// builds, SVR_FORCE_ZSPLIT; 0 otherwise)
inline RingParts ring_parts(uint32_t rx, uint32_t ry, uint32_t rz, uint32_t esize, bool twin, int force_zsplit) {
    const uint64_t limit = ((uint64_t)1 << 32) - 128;        // a part's bytes and its 64 bytes of slack stay below 2^32
    const uint64_t plane = (uint64_t)rx * (uint64_t)ry * (uint64_t)esize, bytes = plane * (uint64_t)rz;
    const uint32_t block_z = esize == 4 ? 2u : 4u;          // ring z planes per micro-block of the copy
    RingParts r;
    r.nparts = 1u; r.zsplit = rz; r.part_bytes = 0u;
    r.rbytes = r.rbytes_last = (uint32_t)(bytes + 64 < ((uint64_t)1 << 32) ? bytes + 64 : 0xFFFFFFFFull);
    r.span_ok = false; r.twin_ok = false;
    if (plane == 0 || plane > limit) return r;               // not even one plane fits a resource: 64-bit addressing only
    uint64_t zsplit = 0;
    if (force_zsplit > 0 && rz > 1u) {
        zsplit = (uint64_t)force_zsplit > ((uint64_t)rz + 7) / 8 ? (uint64_t)force_zsplit : ((uint64_t)rz + 7) / 8;
        if (twin) zsplit = (zsplit + 3) & ~(uint64_t)3;      // whole blocks of the copy, for u8 / u16 and f32 alike
        if (zsplit > rz) zsplit = rz;
        if (zsplit * plane > limit) zsplit = 0;              // (parts that large: the production split below)
    }
    if (zsplit == 0 && bytes + 64 >= ((uint64_t)1 << 32)) {
        zsplit = limit / plane < rz ? limit / plane : rz;    // (< rz here: the ring does not fit one resource)
        if (zsplit >= 4) zsplit &= ~(uint64_t)3;
    }
    if (zsplit) {
        r.zsplit = (uint32_t)zsplit;
        r.nparts = (uint32_t)(((uint64_t)rz + zsplit - 1) / zsplit);
        r.part_bytes = r.rbytes = (uint32_t)(zsplit * plane);
        r.rbytes_last = (uint32_t)(bytes - (uint64_t)(r.nparts - 1) * zsplit * plane + 64);
        if (r.nparts == 1u) { r.rbytes = r.rbytes_last; r.part_bytes = 0u; }
    }
    r.span_ok = r.nparts <= 8u && (uint64_t)ry * (uint64_t)rz < ((uint64_t)1 << 24) && (uint64_t)rx * esize < ((uint64_t)1 << 24);
    // the march indexes part p of the copy like part p of the ring (p * part_bytes in, offsets relative to it): right only
    // where a part boundary never falls inside a block, i.e. where zsplit is a whole number of blocks
    r.twin_ok = twin && (r.nparts == 1u || r.zsplit % block_z == 0u);
    return r;
}
