"""CPU: the numpy restatement of svr_contacts (tests/contacts_twin.py) against a triple loop on small wrapped rings, known
answers, the ``selected`` and ``ignore_zero`` arithmetic, a cross-check with the mesh twin, a stand-alone host program
over csrc/contacts_faces.h built with -fsanitize=address,undefined, ``ContactTable``'s host arithmetic on a table built
from the twin, the argument checks of ``SubVolume.contacts`` that need no device, and the ctypes mirrors of the structs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contacts_twin import (RECORD, box_twin, brute_force, centroid_twin, contacts_twin, data_area_twin, neighbours_twin, position_twin,
                           records_of_pairs)
from mesh_twin import mesh_twin
from sub_volume_renderer_amd import ContactTable, SubVolume, SubVolumeMaterial, _native as N
from sub_volume_renderer_amd.contacts import table_from_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
HIGH = 0xFFFFFFFF


def small_ring(labels=True, seed=5):
    """A 6 x 5 x 4 ring (x, y, z) whose window (5 x 4 x 3 from (4, 3, 2)) wraps on every axis."""
    rng = np.random.default_rng(seed)
    density = rng.integers(0, 256, (4, 5, 6), dtype=np.uint8)
    lab = rng.choice(np.array([0, 0, 1, 7, HIGH, 2**31 + 3], np.uint32), (4, 5, 6)) if labels else None
    return dict(density=density, labels=lab, offset=(4, 3, 2), shape=(5, 4, 3), scale=(1.0, 1.0, 1.0))


def dense_ring(labels, density=None, offset=(0, 0, 0)):
    """A ring that holds exactly its window: labels [z][y][x] at logical ``offset`` (a multiple of the ring: no wrap)."""
    labels = np.asarray(labels, np.uint32)
    if density is None:
        density = (np.arange(labels.size, dtype=np.uint32).reshape(labels.shape) * 7 % 251).astype(np.uint8)
    return dict(density=density, labels=labels, offset=offset, shape=labels.shape[::-1], scale=(1.0, 1.0, 1.0))


# ---- the twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [None, ((5, 3, 3), (3, 9, 1)), ((4, 4, 2), (2, 1, 9)), ((0, 0, 0), (3, 3, 3)), ((6, 5, 4), (1, 1, 1))])
@pytest.mark.parametrize("labels", [None, [7], [0, HIGH, 12345]])
@pytest.mark.parametrize("ignore_zero", [False, True])
def test_twin_equals_the_triple_loop(box, labels, ignore_zero):
    for seed in (5, 6):
        ring = small_ring(seed=seed)
        twin, brute = contacts_twin(ring, box, labels, ignore_zero), brute_force(ring, box, labels, ignore_zero)
        assert twin["header"] == brute["header"]
        assert twin["records"].tobytes() == records_of_pairs(brute["pairs"]).tobytes()
        assert twin["integer"] and (twin["records"]["label_lo"] < twin["records"]["label_hi"]).all()
        if box is None and labels is None:
            assert twin["header"][7] == 60 and twin["header"][0] == (6 if ignore_zero else 10) and (twin["header"][3] > 0) == ignore_zero
            assert twin["header"][1] + twin["header"][3] == contacts_twin(ring)["header"][1]
        if box == ((0, 0, 0), (3, 3, 3)):
            assert twin["header"][:4] == [0, 0, 0, 0] and twin["header"][7] == 0      # the box misses the window
        if box == ((6, 5, 4), (1, 1, 1)):
            assert twin["header"][:4] == [0, 0, 0, 0] and twin["header"][7] == 1      # one voxel has no face


def test_two_abutting_boxes():
    """Two boxes of 4 x 3 x 2 side by side in x, window offset (8, 6, 4) in a ring of that size: one record."""
    lab = np.zeros((2, 3, 8), np.uint32)
    lab[:, :, :4], lab[:, :, 4:] = 5, 9
    ring = dense_ring(lab, offset=(8, 6, 4))
    twin = contacts_twin(ring, ignore_zero=True)
    assert twin["header"] == [1, 6, 0, 0, 8, 6, 4, 48]
    r = twin["records"][0]
    assert (int(r["label_lo"]), int(r["label_hi"])) == (5, 9) and r["faces"].tolist() == [6, 0, 0]
    # the owning voxels are x = 8 + 3, y = 6 .. 8, z = 4 .. 5: twice the face centres relative to the offset
    assert r["sum2"].tolist() == [6 * (2 * 3 + 1), 2 * 2 * (0 + 1 + 2), 3 * 2 * (0 + 1)]
    assert r["lo"].tolist() == [11, 6, 4] and r["hi"].tolist() == [11, 8, 5]
    assert int(r["finite"]) == 12
    d = ring["density"].astype(np.int64)
    assert int(r["value_sum"]) == int(d[:, :, 3].sum() + d[:, :, 4].sum())
    assert float(r["vmin"]) == float(min(d[:, :, 3:5].min(), 255)) and float(r["vmax"]) == float(d[:, :, 3:5].max())
    assert centroid_twin(r, (8, 6, 4)) == (11.5, 7.0, 4.5)


@pytest.mark.parametrize("shape", [(3, 4, 5), (1, 1, 6), (2, 1, 1), (1, 1, 1)])
def test_every_voxel_its_own_label(shape):
    nz, ny, nx = shape
    lab = np.arange(1, nz * ny * nx + 1, dtype=np.uint32).reshape(shape)
    twin = contacts_twin(dense_ring(lab))
    pairs = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    assert twin["header"][:4] == [pairs, pairs, 0, 0] and twin["header"][7] == nx * ny * nz
    assert (twin["records"]["faces"].sum(axis=1) == 1).all() and (twin["records"]["finite"] == 2).all()
    assert np.array_equal(twin["records"]["lo"], twin["records"]["hi"])


def test_nothing_to_find():
    constant = contacts_twin(dense_ring(np.full((3, 4, 5), 7, np.uint32)))
    assert constant["header"] == [0, 0, 0, 0, 0, 0, 0, 60] and constant["records"].size == 0
    ring = small_ring(labels=False)
    for ignore_zero in (False, True):
        assert contacts_twin(ring, ignore_zero=ignore_zero)["header"] == [0, 0, 0, 0, 4, 3, 2, 60]
    assert contacts_twin(ring, labels=[0])["header"][:4] == [0, 0, 0, 0]


def test_keys_of_label_zero_and_the_highest_label():
    lab = np.array([[[0, 1, 0, HIGH, 2**31]]], np.uint32)
    twin = contacts_twin(dense_ring(lab))
    rec = twin["records"]
    assert list(zip(rec["label_lo"].tolist(), rec["label_hi"].tolist())) == [(0, 1), (0, HIGH), (2**31, HIGH)]
    keys = rec.view(np.uint8).reshape(-1, 112)[:, :8].copy().view("<u8").reshape(-1)
    assert keys.tolist() == [1 << 32, HIGH << 32, (HIGH << 32) | 2**31] and (keys != 0).all()
    assert rec["faces"].tolist() == [[2, 0, 0], [1, 0, 0], [1, 0, 0]]


def test_face_counts_are_the_unequal_neighbours():
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        lab = rng.integers(0, 4, (5, 6, 7)).astype(np.uint32)
        rec = contacts_twin(dense_ring(lab))["records"]
        want = [int((lab[:, :, 1:] != lab[:, :, :-1]).sum()), int((lab[:, 1:] != lab[:, :-1]).sum()), int((lab[1:] != lab[:-1]).sum())]
        assert rec["faces"].sum(axis=0).tolist() == want and (rec["finite"] == 2 * rec["faces"].sum(axis=1)).all()


def test_selected_and_ignore_zero_arithmetic():
    ring = small_ring()
    everything = contacts_twin(ring)
    pairs = {(int(r["label_lo"]), int(r["label_hi"])): r for r in everything["records"]}
    zero_faces = sum(int(r["faces"].sum()) for (lo, _), r in pairs.items() if lo == 0)
    assert zero_faces > 0
    dropped = contacts_twin(ring, ignore_zero=True)
    assert dropped["header"][3] == zero_faces and dropped["header"][1] == everything["header"][1] - zero_faces
    assert dropped["records"].tobytes() == everything["records"][everything["records"]["label_lo"] != 0].tobytes()
    # selected: a pair is kept when either label is listed; an id nobody has selects nothing
    for ids in ([7], [0], [HIGH, 1], [12345], [12345, 7]):
        got = contacts_twin(ring, labels=ids)
        want = [k for k in sorted(pairs) if k[0] in ids or k[1] in ids]
        assert list(zip(got["records"]["label_lo"].tolist(), got["records"]["label_hi"].tolist())) == want
        assert got["header"][1] == sum(int(pairs[k]["faces"].sum()) for k in want) and got["header"][3] == 0
        assert all(r.tobytes() == pairs[(int(r["label_lo"]), int(r["label_hi"]))].tobytes() for r in got["records"])
        # the label-0 drop comes second: it counts only faces that `selected` kept
        both = contacts_twin(ring, labels=ids, ignore_zero=True)
        assert both["header"][3] == sum(int(pairs[k]["faces"].sum()) for k in want if k[0] == 0)
        assert both["header"][1] + both["header"][3] == got["header"][1]
    assert contacts_twin(ring, labels=[12345])["header"][:4] == [0, 0, 0, 0]


def test_float_values():
    ring = small_ring()
    ring["density"] = ring["density"].astype(np.float32) - np.float32(100.0)
    ring["density"][0, 0, 0], ring["density"][3, 4, 5], ring["density"][2, 3, 4] = np.nan, np.inf, -np.inf
    twin = contacts_twin(ring)
    rec, whole = twin["records"], contacts_twin(small_ring())["records"]
    assert not twin["integer"] and np.array_equal(rec["faces"], whole["faces"])
    area = rec["faces"].sum(axis=1)
    assert (rec["finite"] <= 2 * area).all() and (rec["finite"] < 2 * area).any()
    assert np.isfinite(rec["value_sum"].view(np.float64)).all() and (twin["abs_sum"] >= np.abs(rec["value_sum"].view(np.float64))).all()
    assert np.isfinite(rec["vmin"][rec["finite"] > 0]).all() and (rec["vmin"] <= rec["vmax"])[rec["finite"] > 0].all()


def test_surface_is_the_quads_of_the_mesh_twin():
    """An object that does not touch the box border, background=True: its faces with anything are the quads of the
    label-mode surface-nets mesh of that object (two triangles per quad)."""
    rng = np.random.default_rng(11)
    lab = rng.choice(np.array([0, 3, 4], np.uint32), (9, 10, 11))
    lab[2:7, 3:8, 2:9][rng.random((5, 5, 7)) < 0.7] = 21
    lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1] = 0, 0, 0, 0, 0, 0
    ring = dense_ring(lab, offset=(11, 10, 9))
    table = table_of(contacts_twin(ring))
    mesh = mesh_twin((11, 10, 9), ring["density"].astype(np.float32), lab, selected=[21])
    assert len(mesh["triangles"]) % 2 == 0 and len(mesh["triangles"]) > 100
    assert table.surface(21) == len(mesh["triangles"]) // 2
    boxed = ((12, 11, 10), (9, 8, 7))
    mesh = mesh_twin((11, 10, 9), ring["density"].astype(np.float32), lab, box=boxed, selected=[21])
    assert table_of(contacts_twin(ring, box=boxed)).surface(21) == len(mesh["triangles"]) // 2


# ---- contacts_faces.h on the host ------------------------------------------------------------------------------------------
# Walks boxes unit by unit as the kernel does and holds con_unit_updates to brute force; exit status 0: everything held.
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <map>
#include <set>
#include <tuple>
#include <vector>
#include "contacts_faces.h"

static uint64_t state = 88172645463325252ull;
static uint32_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)(state >> 11); }
static const uint32_t kLabels[6] = {0u, 1u, 2u, 0x80000000u, 0xFFFFFFFFu, 1u};
static uint32_t some_label() { return kLabels[rnd() % 6u]; }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

typedef std::tuple<int, uint64_t, uint32_t> Update;                     // axis, key, mask

static std::vector<Update> updates_of(const ConUnit& u, std::vector<uint64_t>* asked) {
    std::vector<Update> out;
    con_unit_updates(u, [&](uint64_t key) { if (asked) asked->push_back(key); return true; },
                     [&](int axis, uint64_t key, uint32_t m) { out.push_back(Update(axis, key, m)); });
    return out;
}

// every `have` mask against the definition, face by face
static int masks() {
    for (uint32_t round = 0; round < 40; ++round)
        for (uint32_t have = 0; have < 16; ++have)
            for (uint32_t other = 0; other < 64; ++other) {
                ConUnit u = {};
                for (int j = 0; j < 4; ++j) { u.lab[j] = some_label(); u.ylab[j] = some_label(); u.zlab[j] = some_label(); }
                u.xlab = some_label();
                u.have = have; u.xhave = other & 1u;
                u.yhave = (other & 2u) ? have : (other & 8u) ? rnd() % 16u : 0u;
                u.zhave = (other & 4u) ? have : (other & 16u) ? rnd() % 16u : 0u;
                std::map<std::pair<int, uint64_t>, uint32_t> want;
                std::vector<uint64_t> order;
                for (int axis = 0; axis < 3; ++axis)
                    for (int j = 0; j < 4; ++j) {
                        if (!(u.have >> j & 1u)) continue;
                        uint32_t nb; bool there;
                        if (axis == 0) { nb = j < 3 ? u.lab[j + 1] : u.xlab; there = j < 3 ? (u.have >> (j + 1) & 1u) != 0u : u.xhave != 0u; }
                        else if (axis == 1) { nb = u.ylab[j]; there = (u.yhave >> j & 1u) != 0u; }
                        else { nb = u.zlab[j]; there = (u.zhave >> j & 1u) != 0u; }
                        if (!there || nb == u.lab[j]) continue;
                        want[std::make_pair(axis, con_key(u.lab[j], nb))] |= 1u << j;
                        order.push_back(con_key(u.lab[j], nb));
                    }
                std::vector<uint64_t> asked;
                const std::vector<Update> got = updates_of(u, &asked);
                CHECK(asked == order);                                  // keep() once per face: x, y, z, ascending voxel
                CHECK(got.size() == want.size());                       // one update per axis and pair: merged
                CHECK(con_unit_any(u) == !want.empty());
                for (const Update& g : got) {
                    const auto it = want.find(std::make_pair(std::get<0>(g), std::get<1>(g)));
                    CHECK(it != want.end() && it->second == std::get<2>(g) && std::get<1>(g) != 0ull);
                    want.erase(it);
                }
                CHECK(want.empty());
                // a keep() that refuses some faces: they reach no update, the others are as before
                std::vector<Update> kept;
                uint32_t calls = 0;
                con_unit_updates(u, [&](uint64_t key) { ++calls; return con_key_lo(key) != 0u; },
                                 [&](int axis, uint64_t key, uint32_t m) { kept.push_back(Update(axis, key, m)); });
                CHECK(calls == order.size());
                std::vector<Update> expect;
                for (const Update& g : got) if (con_key_lo(std::get<1>(g)) != 0u) expect.push_back(g);
                CHECK(kept == expect);
            }
    return 0;
}

// a box of nx x ny x nz voxels, its first voxel `head` elements into a unit, walked unit by unit
static int box(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t head) {
    std::vector<uint32_t> lab((size_t)nx * ny * nz);
    for (uint32_t& l : lab) l = some_label();
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return lab[((size_t)z * ny + y) * nx + x]; };
    typedef std::tuple<int, uint32_t, uint32_t, uint32_t> Face;         // axis, x, y, z of the owning voxel
    std::map<Face, uint64_t> want, got;
    for (uint32_t z = 0; z < nz; ++z) for (uint32_t y = 0; y < ny; ++y) for (uint32_t x = 0; x < nx; ++x) {
        if (x + 1 < nx && at(x, y, z) != at(x + 1, y, z)) want[Face(0, x, y, z)] = con_key(at(x, y, z), at(x + 1, y, z));
        if (y + 1 < ny && at(x, y, z) != at(x, y + 1, z)) want[Face(1, x, y, z)] = con_key(at(x, y, z), at(x, y + 1, z));
        if (z + 1 < nz && at(x, y, z) != at(x, y, z + 1)) want[Face(2, x, y, z)] = con_key(at(x, y, z), at(x, y, z + 1));
    }
    const int64_t n[3] = {nx, ny, nz};
    const ConPlan p = con_plan(n, head, 256u, 16u, 768u);
    CHECK(p.upr == (head + nx + 3u) / 4u && p.units == (uint64_t)p.upr * ny * nz);
    CHECK(p.share % 256u == 0u && p.share >= 4096u && (uint64_t)p.blocks * p.share >= p.units && (uint64_t)(p.blocks - 1u) * p.share < p.units);
    for (uint64_t unit = 0; unit < p.units; ++unit) {
        const uint32_t row = (uint32_t)(unit / p.upr), w = (uint32_t)(unit % p.upr), y = row % ny, z = row / ny;
        const int32_t r0 = (int32_t)(4u * w) - (int32_t)head;
        ConUnit u = {};
        for (int j = 0; j < 4; ++j) {
            const int32_t r = r0 + j;
            if (r < 0 || r >= (int32_t)nx) continue;
            u.have |= 1u << j; u.lab[j] = at((uint32_t)r, y, z);
            if (y + 1 < ny) { u.yhave |= 1u << j; u.ylab[j] = at((uint32_t)r, y + 1, z); }
            if (z + 1 < nz) { u.zhave |= 1u << j; u.zlab[j] = at((uint32_t)r, y, z + 1); }
        }
        if (r0 + 4 < (int32_t)nx) { u.xhave = 1u; u.xlab = at((uint32_t)(r0 + 4), y, z); }
        CHECK(u.have != 0u);                                            // no unit lies outside its row
        for (const Update& g : updates_of(u, nullptr)) {
            const uint32_t m = std::get<2>(g);
            uint32_t count = 0, sum = 0, first = 4, last = 0;
            for (uint32_t j = 0; j < 4; ++j)
                if (m >> j & 1u) {
                    const Face f(std::get<0>(g), (uint32_t)(r0 + (int32_t)j), y, z);
                    CHECK(!got.count(f));                               // every face once
                    got[f] = std::get<1>(g);
                    ++count; sum += j; if (first == 4) first = j; last = j;
                }
            CHECK(m != 0u && m < 16u && con_mask_count(m) == count && con_mask_sum(m) == sum && con_mask_first(m) == first && con_mask_last(m) == last);
        }
    }
    CHECK(got == want);
    return 0;
}

int main() {
    // the key: label_lo in the low word, never 0 for a face, the same for both orders
    const uint32_t edge[4] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
    std::set<uint32_t> hashes;
    for (uint32_t a : edge) for (uint32_t b : edge) {
        if (a == b) continue;
        const uint64_t k = con_key(a, b);
        CHECK(k == con_key(b, a) && k != 0ull && con_key_lo(k) == (a < b ? a : b) && con_key_hi(k) == (a < b ? b : a));
        CHECK(con_key_lo(k) < con_key_hi(k) && k == ((uint64_t)con_key_hi(k) << 32 | con_key_lo(k)));
        hashes.insert(con_hash(k));
    }
    CHECK(con_key(0u, 1u) == 1ull << 32 && con_key(0xFFFFFFFFu, 0u) == 0xFFFFFFFFull << 32 && hashes.size() == 6u);
    if (masks()) return 1;
    const uint32_t rows[6] = {1u, 2u, 3u, 4u, 5u, 9u};
    for (uint32_t round = 0; round < 6; ++round)
        for (uint32_t nx : rows)
            for (uint32_t head = 0; head < 4; ++head) {
                if (box(nx, 3, 2, head)) return 1;
                if (box(nx, 1, 2, head)) return 1;                      // no +y neighbour anywhere
                if (box(nx, 3, 1, head)) return 1;                      // no +z neighbour
                if (box(nx, 1, 1, head)) return 1;                      // nx == 1: no neighbour at all
            }
    if (box(1100, 3, 2, 3)) return 1;                                    // a row longer than one step of 256 units
    printf("ok\n");
    return 0;
}
"""


def test_unit_faces_are_brute_force_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "faces.cpp", tmp_path / "faces"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HEADER_DIR,
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stderr[-2000:])


# ---- ContactTable on the host ------------------------------------------------------------------------------------------
class _World:
    matrix = np.diag([2.0, 1.0, 0.5, 1.0])


class _Volume:
    world = _World()


_Volume.world.matrix[:3, 3] = (3.0, -2.0, 7.0)


def table_of(twin, scale=(1.0, 1.0, 1.0), spare=3, lod=0):
    """The twin's records, shuffled into a table with ``spare`` empty records, as ``SubVolume.contacts`` builds its result."""
    import torch

    rec = twin["records"]
    slots = np.zeros(rec.size + spare, RECORD)
    slots[np.random.default_rng(3).permutation(slots.size)[:rec.size]] = rec
    words = torch.from_numpy(slots.view("<i8").reshape(-1, 14).copy())
    return table_from_records(words, twin["header"], not twin["integer"], lod, scale, _Volume())


def test_contact_table_answers_on_the_cpu():
    import torch

    rng = np.random.default_rng(21)
    lab = rng.choice(np.array([0, 1, 2, 3, 2**31 + 1, HIGH], np.uint32), (6, 7, 9))
    lab[:, :3, :4] = 2                                                    # one big object
    ring = dense_ring(lab, offset=(9, 14, 12))
    scale = (1.0, 0.5, 0.25)
    twin = contacts_twin(ring)
    rec = twin["records"]
    table = table_of(twin, scale, lod=2)
    assert isinstance(table, ContactTable) and len(table) == rec.size == 15 and table.lod == 2
    # sorted by (a, b) as unsigned labels: 2^31 + 1 and 0xFFFFFFFF come last, not first
    assert table.a.dtype == torch.int64 and table.a.tolist() == rec["label_lo"].tolist() and table.b.tolist() == rec["label_hi"].tolist()
    assert table.a.tolist() == sorted(table.a.tolist()) and table.b.tolist()[-1] == HIGH and table.a.tolist()[-1] == 2**31 + 1
    assert table.faces.tolist() == rec["faces"][:, ::-1].tolist() and table.area.tolist() == rec["faces"].sum(axis=1).tolist()
    assert table.begin.tolist() == rec["lo"][:, ::-1].tolist() and table.end.tolist() == (rec["hi"][:, ::-1] + 1).tolist()
    assert table.finite.tolist() == rec["finite"].tolist()
    assert np.array_equal(table.min.numpy(), rec["vmin"]) and np.array_equal(table.max.numpy(), rec["vmax"])
    assert np.array_equal(table.mean.numpy(), rec["value_sum"].astype(np.float64) / rec["finite"].astype(np.float64))
    assert (table.considered, table.background, table.voxels) == (twin["header"][1], 0, 6 * 7 * 9)
    assert table.centroid.tolist() == [list(centroid_twin(r, ring["offset"])[::-1]) for r in rec]
    assert table.data_area().tolist() == [data_area_twin(r, scale) for r in rec]
    world = _Volume.world.matrix.tolist()
    for i, r in enumerate(rec):
        a, b = int(r["label_lo"]), int(r["label_hi"])
        assert table.index(a, b) == table.index(b, a) == i
        assert table.box(a, b) == table.box(b, a) == box_twin(r, scale)
        assert table.position(b, a) == position_twin(r, ring["offset"], scale, world)
    for id in (0, 2, HIGH, 2**31 + 1):
        want = neighbours_twin(rec, id)
        ids, areas = table.neighbours(id)
        assert list(zip(ids.tolist(), areas.tolist())) == want and len(want) == 5
        assert table.surface(id) == sum(a for _, a in want)
    assert table.neighbours(12345)[0].size == 0 and table.surface(12345) == 0
    # the largest area first (7 touches 4 twice), ties in area go to the smaller id
    tie = table_of(contacts_twin(dense_ring(np.array([[[9, 4, 7], [3, 4, 4]]], np.uint32))))
    assert [v.tolist() for v in tie.neighbours(4)] == [[7, 3, 9], [2, 1, 1]]
    for pair in ((1, 1), (0, 12345), (7, 2)):
        with pytest.raises(KeyError):
            table.index(*pair)
    # float rings: the f64 bits, and NaN where no value is finite
    ring["density"] = np.full(lab.shape, np.nan, np.float32)
    ring["density"][lab == 1] = 2.5
    ftable, frec = table_of(contacts_twin(ring)), contacts_twin(ring)["records"]
    mean = ftable.mean.numpy()
    assert np.array_equal(np.isnan(mean), frec["finite"] == 0) and np.isnan(mean).any() and (mean[~np.isnan(mean)] == 2.5).all()
    assert np.isinf(ftable.min.numpy()[np.isnan(mean)]).all()
    empty = table_of(contacts_twin(small_ring(labels=False)))
    assert len(empty) == 0 and empty.voxels == 60 and empty.neighbours(0)[0].size == 0 and empty.data_area().numel() == 0


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_surface_pins():
    assert "svr_contacts" in N.SIGNATURES and N.CONTACTS_MAX_CAPACITY == 1 << 26 and N.CONTACT_RECORD_BYTES == 112 == RECORD.itemsize
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", header).group(1)) == 9
    assert re.search(r"#define SVR_CONTACTS_MAX_CAPACITY \(1u << 26\)", header) and "tests/contacts_twin.py" in header
    assert "ContactTable" in __import__("sub_volume_renderer_amd").__all__ and hasattr(SubVolume, "contacts")
    import __graft_entry__ as g
    import inspect

    assert "contacts_kernels.hip" in g.HIP_SOURCES and "contacts_faces.h" in inspect.getsource(g.build_hip)


def test_struct_sizes_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    fields = ("label_lo", "label_hi", "faces", "sum2", "lo", "hi", "finite", "value_sum", "vmin", "vmax", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu'
                   + " %zu" * len(fields) + '\\n", sizeof(svr_contacts_params), sizeof(svr_objects_params), sizeof(svr_contact_record), '
                   "sizeof(svr_contacts_outputs), offsetof(svr_contacts_params, selected), offsetof(svr_contacts_params, capacity), "
                   + ", ".join(f"offsetof(svr_contact_record, {f})" for f in fields) + "); return 0; }\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:6] == [C.sizeof(N.ContactsParams), C.sizeof(N.ObjectsParams), C.sizeof(N.ContactRecord), C.sizeof(N.ContactsOutputs),
                       N.ContactsParams.selected.offset, N.ContactsParams.capacity.offset]
    assert got[2:4] == [112, 16]
    assert got[6:] == [getattr(N.ContactRecord, f).offset for f in fields] == [RECORD.fields[f][1] for f in fields]


def test_argument_errors_fire_without_a_gpu():
    pairs = [(np.zeros((16, 16, 16), np.uint8), np.zeros((16, 16, 16), np.uint32))]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs, (2, 2, 2), (8, 8, 8))
    for kw in (dict(lod=1), dict(lod=-1), dict(lod=True), dict(capacity=0), dict(capacity=(1 << 26) + 1), dict(capacity=2.0), dict(capacity=True),
               dict(labels=[]), dict(labels="12"), dict(labels=[-1]), dict(labels=[1.5]), dict(box=((0, 0, 0),)), dict(box=((0, 0, 0), (0, 4, 4)))):
        with pytest.raises(ValueError):
            vol.contacts(**kw)
