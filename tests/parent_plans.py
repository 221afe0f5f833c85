"""The scratch layouts of svr_mesh, svr_components and svr_split as the plan headers gave them before the prefix scan moved to
csrc/box_scan.h (tests/golden/box_scan_parent_plans.json: per unit and extent, every byte offset and `bytes`, printed by
that commit's mesh_plan.h, components_plan.h and split_plan.h).  The plan tests hold today's headers to it."""
import json
import os

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_scan_parent_plans.json")) as f:
    PARENT_PLANS = json.load(f)


def held_to_parent(unit, case, offsets):
    """unit: "mesh" (nib_off, cnt_off[4], bit_off, bytes of "nx ny nz head"), "components" (parent_off, aux_off, cnt_off[3],
    bytes of "nx ny nz head") or "split" (up_off, uf_off, aux_off, cnt_off[3], bytes of "nx ny nz")."""
    want = PARENT_PLANS[unit][" ".join(str(v) for v in case)]
    assert want == list(offsets), (unit, case, want, offsets)
