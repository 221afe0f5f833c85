// Block -> tile tables of the march (MarchParams::tile_order): which tile workgroup b draws.  Plain host C++ on plain
// integers and floats, so that a test can compile it without HIP (tests/test_tile_order.py); svr_render.hip caches the
// tables per context and copies them to the device.
//
// Workgroup b runs on XCD b % 8 (round-robin dispatch) and every XCD has its own
// L2, so (1) tiles that sample neighbouring voxels should share an XCD and (2) every XCD should get the
// same amount of work.  A contiguous run of tiles per XCD (mode 1) is best for (1) but gives each XCD
// one horizontal band of the frame, and the bands differ in cost; instead deal CHUNKS of cw x ch tiles
// round-robin to the XCDs, so each XCD samples the whole frame.  Placement never affects results.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// chunk size in pixels per policy (variant bits 13-15; policy 1 is the in-kernel contiguous mapping: no table)
// (policy 7: the camera-independent 64x64 table of round 1 — what policy 0 falls back to with SVR_STATIC_PLACEMENT)
static const int kChunk[8][2] = { { 64, 64 }, { 0, 0 }, { 1, 1 }, { 64, 32 }, { 32, 32 }, { 128, 64 }, { 32, 16 }, { 64, 64 } };

// What both builders end with: lists[k] holds the tiles meant for XCD k, n tiles in all.
// XCD k runs blocks k, k + 8, ...: exactly ceil((n - k) / 8) of them; surplus tiles (list tails: the cheapest of a
// cost-sorted list) move over to the lists that are short, then the lists are interleaved.
static inline void interleave_balanced(std::vector<uint32_t> lists[8], int n, std::vector<uint32_t>& order) {
    std::vector<uint32_t> spare;
    for (int k = 0; k < 8; ++k) {
        const size_t need = n > k ? (size_t)((n - k + 7) / 8) : 0;
        while (lists[k].size() > need) { spare.push_back(lists[k].back()); lists[k].pop_back(); }
    }
    for (int k = 0; k < 8; ++k) {
        const size_t need = n > k ? (size_t)((n - k + 7) / 8) : 0;
        while (lists[k].size() < need) { lists[k].push_back(spare.back()); spare.pop_back(); }
    }
    order.assign((size_t)n, 0u);
    for (int k = 0; k < 8; ++k)
        for (size_t j = 0; j < lists[k].size(); ++j) order[8 * j + (size_t)k] = lists[k][j];
}

// Static placement: the chunks in raster order, dealt round-robin to the XCDs.
static inline void build_tile_order(int tx, int ty, int cw, int ch, std::vector<uint32_t>& order) {
    const int n = tx * ty;
    std::vector<uint32_t> seq;
    seq.reserve((size_t)n);
    for (int cy = 0; cy < ty; cy += ch)
        for (int cx = 0; cx < tx; cx += cw)
            for (int y = cy; y < std::min(cy + ch, ty); ++y)
                for (int x = cx; x < std::min(cx + cw, tx); ++x) seq.push_back((uint32_t)(y * tx + x));
    std::vector<uint32_t> lists[8];
    const int run = cw * ch;
    for (int i = 0; i < n; ++i) lists[(i / run) % 8].push_back(seq[(size_t)i]);
    interleave_balanced(lists, n, order);
}

// What the cost-sorted table reads of a draw: MarchParams' ndc_to_data and size, and the fields of its svr_frame
// (band_h > 0: fill_params has defaulted it).
struct TileCostView {
    const float* ndc_to_data;      // 16, column-major
    const float* size;             // 3
    int32_t frame_w, frame_h, x0, y0, out_w, out_h, band_h, band_pitch;
};

// Length (in finest-level voxels) of the part of the pixel's ray inside the proxy box: what a full march of that
// pixel costs, up to the constant step.  Same geometry as setup_ray, evaluated loosely (placement only).
static inline float ray_cost(const TileCostView& V, float px_frame, float py_frame) {
    const float ndcx = 2.0f * px_frame / (float)V.frame_w - 1.0f, ndcy = 1.0f - 2.0f * py_frame / (float)V.frame_h;
    const float nv[4] = { ndcx, ndcy, -1.0f, 1.0f }, fv[4] = { ndcx, ndcy, 1.0f, 1.0f };
    float n4[4], f4[4];
    const float* m = V.ndc_to_data;                // (svr_common::mat_vec4 of ray_common.h, term by term)
    for (int i = 0; i < 4; ++i) {
        n4[i] = ((m[0 + i] * nv[0] + m[4 + i] * nv[1]) + m[8 + i] * nv[2]) + m[12 + i] * nv[3];
        f4[i] = ((m[0 + i] * fv[0] + m[4 + i] * fv[1]) + m[8 + i] * fv[2]) + m[12 + i] * fv[3];
    }
    float o[3], d[3], len = 0.0f;
    for (int a = 0; a < 3; ++a) { o[a] = n4[a] / n4[3]; d[a] = f4[a] / f4[3] - o[a]; len += d[a] * d[a]; }
    len = sqrtf(len);
    if (!(len > 0.0f)) return 0.0f;
    float t0 = 0.0f, t1 = len;
    for (int a = 0; a < 3; ++a) {
        const float r = d[a] / len, lo = -0.5f, hi = V.size[a] - 0.5f;
        if (fabsf(r) < 1e-12f) { if (o[a] < lo || o[a] > hi) return 0.0f; continue; }
        const float ta = (lo - o[a]) / r, tb = (hi - o[a]) / r;
        t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    }
    return t1 > t0 ? t1 - t0 : 0.0f;
}

// Cost-sorted placement: chunks of tiles ordered by the length of their rays, longest first, and dealt to the XCDs
// in snake order (0..7, 7..0, ...): every XCD gets the same share of the work, the expensive tiles start first and
// the cheap ones fill the end of the frame (longest-processing-time-first scheduling of the frame's tail).
static inline void build_tile_order_by_cost(const TileCostView& V, int tx, int ty, int tile_w, int tile_h, int cw, int ch,
                                            std::vector<uint32_t>& order) {
    struct Chunk { float cost; int cx, cy; };
    std::vector<Chunk> chunks;
    for (int cy = 0; cy < ty; cy += ch)
        for (int cx = 0; cx < tx; cx += cw) {
            // output pixel of the chunk's centre -> frame pixel (svr_frame mapping)
            const int ox = std::min(V.out_w - 1, (cx + cw / 2) * tile_w + tile_w / 2);
            const int oy = std::min(V.out_h - 1, (cy + ch / 2) * tile_h + tile_h / 2);
            const float fx = (float)(V.x0 + ox) + 0.5f;
            const float fy = (float)(V.y0 + (oy / V.band_h) * V.band_pitch + oy % V.band_h) + 0.5f;
            chunks.push_back({ ray_cost(V, fx, fy), cx, cy });
        }
    std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk& a, const Chunk& b) { return a.cost > b.cost; });
    std::vector<uint32_t> lists[8];
    for (size_t i = 0; i < chunks.size(); ++i) {
        const int round = (int)(i / 8), pos = (int)(i % 8), k = (round & 1) ? 7 - pos : pos;
        for (int y = chunks[i].cy; y < std::min(chunks[i].cy + ch, ty); ++y)
            for (int x = chunks[i].cx; x < std::min(chunks[i].cx + cw, tx); ++x) lists[k].push_back((uint32_t)(y * tx + x));
    }
    interleave_balanced(lists, tx * ty, order);
}
