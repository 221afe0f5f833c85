"""The block -> tile tables of the march (csrc/tile_order.h): static chunk placement per policy and the cost-sorted
placement of the default policy.  The header is plain host C++; it is compiled here on its own with the host compiler.
The driver reads commands from stdin and prints tables and ray costs; the tests hold them to properties worked out
here: a table is a permutation that gives every XCD its exact share, chunks stay on one XCD up to the tiles the
balancing step has to move (counted from the list lengths), and cost-sorted chunks are dealt longest ray first, in snake
order, ties in raster order, with the ray length restated in numpy float32."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]

# commands, one per line (floats travel as their 32 bits):
#   K                                   -> the 16 entries of kChunk
#   S tx ty cw ch                       -> n, then the static table
#   V m[16] size[3] frame[8]            -> sets the view (ndc_to_data, size; frame_w frame_h x0 y0 out_w out_h band_h band_pitch)
#   R npix (fx fy) * npix               -> the ray cost of each frame pixel, as bits
#   C tx ty tile_w tile_h cw ch         -> n, then the cost-sorted table of the view
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "tile_order.h"
static float rdf() { uint32_t u = 0; if (scanf("%" SCNu32, &u) != 1) return 0.0f; float f; memcpy(&f, &u, 4); return f; }
static void print_table(const std::vector<uint32_t>& order) {
    printf("%zu", order.size());
    for (uint32_t t : order) printf(" %" PRIu32, t);
    printf("\n");
}
int main() {
    float m[16] = {0}, size[3] = {0};
    TileCostView V{ m, size, 0, 0, 0, 0, 0, 0, 0, 0 };
    char cmd[4];
    while (scanf("%3s", cmd) == 1) {
        std::vector<uint32_t> order;
        if (cmd[0] == 'K') {
            for (int p = 0; p < 8; ++p) printf("%d %d ", kChunk[p][0], kChunk[p][1]);
            printf("\n");
        } else if (cmd[0] == 'S') {
            int tx, ty, cw, ch;
            if (scanf("%d %d %d %d", &tx, &ty, &cw, &ch) != 4) return 1;
            build_tile_order(tx, ty, cw, ch, order);
            print_table(order);
        } else if (cmd[0] == 'V') {
            for (float& x : m) x = rdf();
            for (float& x : size) x = rdf();
            if (scanf("%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd32, &V.frame_w, &V.frame_h, &V.x0, &V.y0,
                      &V.out_w, &V.out_h, &V.band_h, &V.band_pitch) != 8) return 1;
        } else if (cmd[0] == 'R') {
            int npix;
            if (scanf("%d", &npix) != 1) return 1;
            for (int i = 0; i < npix; ++i) {
                const float fx = rdf(), fy = rdf(), cost = ray_cost(V, fx, fy);
                uint32_t u; memcpy(&u, &cost, 4);
                printf("%" PRIu32 " ", u);
            }
            printf("\n");
        } else if (cmd[0] == 'C') {
            int tx, ty, tw, th, cw, ch;
            if (scanf("%d %d %d %d %d %d", &tx, &ty, &tw, &th, &cw, &ch) != 6) return 1;
            build_tile_order_by_cost(V, tx, ty, tw, th, cw, ch, order);
            print_table(order);
        } else return 1;
    }
    return 0;
}
"""

# svr_set_variant bits 13-15 -> chunk size in pixels; policy 1 is the in-kernel contiguous mapping and has no table
K_CHUNK = [(64, 64), (0, 0), (1, 1), (64, 32), (32, 32), (128, 64), (32, 16), (64, 64)]
TABLE_POLICIES = [0, 2, 3, 4, 5, 6, 7]
TILES = [(8, 8), (16, 16), (64, 1), (128, 2)]
GRIDS = [(1, 1), (3, 2), (7, 5), (9, 8), (17, 13)]


def build_driver(directory, extra_flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = os.path.join(directory, "drv.cpp"), os.path.join(directory, "drv")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([cxx, *CXXFLAGS, *extra_flags, "-I", HEADER_DIR, src, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("tile_order")))


def run(driver, commands):
    """-> one list of ints per command that prints (every command but V)."""
    out = subprocess.run([driver], input="\n".join(commands) + "\n", capture_output=True, text=True, check=True).stdout
    lines = [[int(x) for x in ln.split()] for ln in out.split("\n") if ln.strip()]
    assert len(lines) == sum(1 for c in commands if not c.startswith("V"))
    return lines


def table_of(line, n):
    assert line[0] == n and len(line) == n + 1
    return line[1:]


def bits(a):
    return " ".join(str(int(u)) for u in np.asarray(a, np.float32).ravel().view(np.uint32))


def chunk_dims(policy, tile_w, tile_h):
    """Chunk size in tiles, as the host forms it from the policy table: at least one tile."""
    return max(1, K_CHUNK[policy][0] // tile_w), max(1, K_CHUNK[policy][1] // tile_h)


def need(n, k):
    """Workgroup b runs on XCD b % 8: of n workgroups, XCD k gets ceil((n - k) / 8)."""
    return max(0, -(-(n - k) // 8))


def moved_bound(lengths, n):
    """The balancing step trims every list to its XCD's share and hands the surplus to the short ones: exactly this many
    tiles change XCD, and no tile of a list at or below its share does."""
    assert sum(lengths) == n
    return sum(max(0, lengths[k] - need(n, k)) for k in range(8))


def check_shares(table, n):
    assert sorted(table) == list(range(n))
    for k in range(8):
        assert len(table[k::8]) == need(n, k)            # order[8 j + k] is XCD k's j-th tile


def chunks_of(tx, ty, cw, ch):
    """The chunks in raster order, each the raster order of its tiles (clipped at the grid's edges)."""
    return [[y * tx + x for y in range(cy, min(cy + ch, ty)) for x in range(cx, min(cx + cw, tx))]
            for cy in range(0, ty, ch) for cx in range(0, tx, cw)]


def test_policy_table(driver):
    (line,) = run(driver, ["K"])
    assert [tuple(line[2 * p: 2 * p + 2]) for p in range(8)] == K_CHUNK


def test_static_tables(driver):
    cases = [(tx, ty, *chunk_dims(p, tw, th)) for tw, th in TILES for tx, ty in GRIDS for p in TABLE_POLICIES]
    cases = sorted(set(cases))
    assert any(cw > tx and ch > ty for tx, ty, cw, ch in cases) and any(cw == 1 and ch == 1 for _, _, cw, ch in cases)
    lines = run(driver, ["S %d %d %d %d" % c for c in cases])
    for (tx, ty, cw, ch), line in zip(cases, lines):
        n = tx * ty
        table = table_of(line, n)
        check_shares(table, n)
        # the builder deals RUNS of cw * ch tiles of the chunk-raster sequence (a run is a chunk wherever the grid is a
        # multiple of the chunk; clipped chunks at the edges make later runs straddle two chunks)
        seq = [t for chunk in chunks_of(tx, ty, cw, ch) for t in chunk]
        run_of = {t: i // (cw * ch) for i, t in enumerate(seq)}
        lengths = [sum(1 for t in seq if run_of[t] % 8 == k) for k in range(8)]
        xcd = {t: b % 8 for b, t in enumerate(table)}
        strays = [t for t in seq if xcd[t] != run_of[t] % 8]
        assert len(strays) == moved_bound(lengths, n), (tx, ty, cw, ch)
        for t in strays:                                 # from a list above its share to one below it
            assert lengths[run_of[t] % 8] > need(n, run_of[t] % 8) and lengths[xcd[t]] < need(n, xcd[t]), (tx, ty, cw, ch, t)
        for k in range(8):                               # what stayed keeps the sequence's order
            kept = [t for t in table[k::8] if run_of[t] % 8 == k]
            assert kept == [t for t in seq if run_of[t] % 8 == k][:len(kept)], (tx, ty, cw, ch, k)


# ---- cost-sorted placement -------------------------------------------------------------------------------------------

def look_at(eye, target, up):
    f = np.asarray(target, float) - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def view_matrix(kind, size):
    """ndc_to_data (column-major float32[16]) of a camera that sees the whole box with a margin around it, so that the
    outer pixels' rays miss it.  Data space = world space here."""
    c = (np.asarray(size, float) - 1.0) / 2.0
    r = float(np.linalg.norm(size))
    if kind == "perspective":
        cam = look_at(c + np.array([0.55, 0.3, 0.95]) * r, c, (0.0, 1.0, 0.0))
        near, far, t = 0.1 * r, 6.0 * r, np.tan(np.radians(25.0))
        proj = np.array([[1 / (t * 16 / 9), 0, 0, 0], [0, 1 / t, 0, 0],
                         [0, 0, -(far + near) / (far - near), -2 * far * near / (far - near)], [0, 0, -1, 0]])
    else:
        cam = look_at(c + np.array([0.0, 0.0, 2.0]) * r, c, (0.0, 1.0, 0.0))      # along -z: equal costs across the box
        hw, hh, near, far = 0.9 * r, 0.6 * r, 0.1 * r, 6.0 * r
        proj = np.array([[1 / hw, 0, 0, 0], [0, 1 / hh, 0, 0], [0, 0, -2 / (far - near), -(far + near) / (far - near)], [0, 0, 0, 1]])
    m = np.linalg.inv(proj @ cam).astype(np.float32)
    if kind == "orthographic":
        assert np.allclose(m[3], (0, 0, 0, 1), atol=1e-6)
        m[3] = (0, 0, 0, 1)                                                       # n4[3] == f4[3] == 1
    return m.T.ravel().copy()


def ray_cost_np(m, size, frame_w, frame_h, px, py):
    """tile_order.h's ray_cost for arrays of frame pixels, operation by operation in float32."""
    f32 = np.float32
    m, size, px, py = np.asarray(m, f32), np.asarray(size, f32), np.asarray(px, f32), np.asarray(py, f32)
    with np.errstate(all="ignore"):
        ndcx = f32(2) * px / f32(frame_w) - f32(1)
        ndcy = f32(1) - f32(2) * py / f32(frame_h)
        n4 = [((m[i] * ndcx + m[4 + i] * ndcy) + m[8 + i] * f32(-1)) + m[12 + i] * f32(1) for i in range(4)]
        f4 = [((m[i] * ndcx + m[4 + i] * ndcy) + m[8 + i] * f32(1)) + m[12 + i] * f32(1) for i in range(4)]
        o = [n4[a] / n4[3] for a in range(3)]
        d = [f4[a] / f4[3] - o[a] for a in range(3)]
        ln = np.zeros_like(px)
        for a in range(3):
            ln = ln + d[a] * d[a]
        ln = np.sqrt(ln)
        dead = ~(ln > 0)
        t0, t1 = np.zeros_like(px), ln.copy()
        for a in range(3):
            r, lo, hi = d[a] / ln, f32(-0.5), size[a] - f32(0.5)
            parallel = np.abs(r) < f32(1e-12)
            dead |= parallel & ((o[a] < lo) | (o[a] > hi))
            ta, tb = (lo - o[a]) / r, (hi - o[a]) / r
            t0 = np.where(parallel, t0, np.fmax(t0, np.fmin(ta, tb)))
            t1 = np.where(parallel, t1, np.fmin(t1, np.fmax(ta, tb)))
        cost = np.where(t1 > t0, t1 - t0, f32(0))
    cost[dead] = 0
    assert cost.dtype == np.float32
    return cost


SIZE = (96.0, 64.0, 80.0)
VIEWS = {kind: view_matrix(kind, SIZE) for kind in ("perspective", "orthographic")}


def view_command(m, frame):
    return "V %s %s %s" % (bits(m), bits(SIZE), " ".join(str(v) for v in frame))


@pytest.mark.parametrize("kind", sorted(VIEWS))
def test_ray_cost_against_numpy_float32(driver, kind):
    m = VIEWS[kind]
    frame_w, frame_h = 133, 77
    ys, xs = np.meshgrid(np.arange(frame_h, dtype=np.float32) + np.float32(0.5),
                         np.arange(0, frame_w, 1, dtype=np.float32) + np.float32(0.5), indexing="ij")
    px, py = xs.ravel()[::3], ys.ravel()[::3]
    (line,) = run(driver, [view_command(m, (frame_w, frame_h, 0, 0, frame_w, frame_h, frame_h, frame_h)),
                           "R %d %s" % (px.size, bits(np.stack([px, py], 1)))])
    got = np.array(line, np.uint32).view(np.float32)
    want = ray_cost_np(m, SIZE, frame_w, frame_h, px, py)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the grid holds rays through the box and rays that miss it; no ray is longer than the box's diagonal
    assert np.count_nonzero(want == 0) > px.size // 10 and np.count_nonzero(want > 0) > px.size // 10
    assert want.max() <= np.float32(np.linalg.norm(SIZE)) * np.float32(1.0001)
    if kind == "orthographic":                                   # along z: every ray through the box crosses its depth
        assert np.all(np.abs(want[want > 0] - np.float32(SIZE[2])) < 1e-2)


def snake(i):
    return 7 - i % 8 if (i // 8) & 1 else i % 8


def cost_cases():
    """(kind, frame, tx, ty, tile_w, tile_h, cw, ch): every tile size and grid with the default policy's 64 x 64-pixel
    chunks; the last output column / row of tiles is cut short; one case per kind is a band-interleaved region."""
    cases = []
    for kind in sorted(VIEWS):
        for tw, th in TILES:
            for tx, ty in GRIDS:
                out_w, out_h = tx * tw - tw // 3, ty * th - th // 3
                cases.append((kind, (out_w, out_h, 0, 0, out_w, out_h, out_h, out_h), tx, ty, tw, th, *chunk_dims(0, tw, th)))
        # stripes of 16 rows out of every 48, from row 16, and columns from 40: a region of a 300 x 400 frame
        cases.append((kind, (300, 400, 40, 16, 17 * 8 - 2, 13 * 8, 16, 48), 17, 13, 8, 8, 2, 2))
    return cases


def test_cost_sorted_tables(driver):
    cases = cost_cases()
    commands = []
    for kind, frame, tx, ty, tw, th, cw, ch in cases:
        commands += [view_command(VIEWS[kind], frame), "C %d %d %d %d %d %d" % (tx, ty, tw, th, cw, ch)]
    lines = run(driver, commands)
    ties = strays_seen = 0
    for (kind, frame, tx, ty, tw, th, cw, ch), line in zip(cases, lines):
        frame_w, frame_h, x0, y0, out_w, out_h, band_h, band_pitch = frame
        n = tx * ty
        table = table_of(line, n)
        check_shares(table, n)
        chunks = chunks_of(tx, ty, cw, ch)
        # a chunk costs what the ray of its centre pixel costs (output pixel -> frame pixel by the svr_frame mapping)
        origin = [(cx, cy) for cy in range(0, ty, ch) for cx in range(0, tx, cw)]
        ox = np.array([min(out_w - 1, (cx + cw // 2) * tw + tw // 2) for cx, _ in origin])
        oy = np.array([min(out_h - 1, (cy + ch // 2) * th + th // 2) for _, cy in origin])
        cost = ray_cost_np(VIEWS[kind], SIZE, frame_w, frame_h, (x0 + ox).astype(np.float32) + np.float32(0.5),
                           (y0 + (oy // band_h) * band_pitch + oy % band_h).astype(np.float32) + np.float32(0.5))
        # dealt in non-increasing cost, equal costs in raster order, to XCDs 0..7, 7..0, ...
        dealt = sorted(range(len(chunks)), key=lambda i: (-float(cost[i]), i))
        ties += len(chunks) - len(set(cost.tolist()))
        home = {}
        for pos, i in enumerate(dealt):
            for t in chunks[i]:
                home[t] = (snake(pos), pos)
        lengths = [sum(1 for t in home if home[t][0] == k) for k in range(8)]
        xcd = {t: b % 8 for b, t in enumerate(table)}
        strays = [t for t in range(n) if xcd[t] != home[t][0]]
        assert len(strays) == moved_bound(lengths, n), (kind, frame, tx, ty, tw, th)
        strays_seen += len(strays)
        for k in range(8):
            mine = [t for t in range(n) if home[t][0] == k]
            expect = sorted(mine, key=lambda t: home[t][1])         # stable: a chunk's tiles stay in raster order
            kept = [t for t in table[k::8] if home[t][0] == k]
            # what stays is the head of the list in dealing order, so what moved away is its tail: the cheapest tiles
            assert kept == expect[:len(kept)], (kind, frame, tx, ty, tw, th, k)
            assert len(kept) == min(len(mine), need(n, k))
            costs = [float(cost[dealt[home[t][1]]]) for t in kept]
            assert costs == sorted(costs, reverse=True)
    assert ties > 0 and strays_seen > 0
