"""CPU suite for the filament tracing (``--trace``): pins of the definition on tests/filament_oracle.py (the shapes whose branches are
known by hand, lengths of straight lines, brute-force invariants on small random volumes, the node / branch balance of skeleton
graphs), the host functions of ``analysis.filaments`` on hand-made tables, the CSV and STAR writers, the options record and both
entry points, the place of the tracing in the pipeline, and what the C entries refuse before they touch the device."""

from __future__ import annotations

import ctypes as C
import dataclasses
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ccl_oracle as co
import filament_cases as fc
import filament_oracle as fo
import shape_oracle as so

from cryovit_amd import io

ROOT = Path(__file__).resolve().parent.parent
V = {name: i for i, name in enumerate(fo.VOXEL_COLS)}
B = {name: i for i, name in enumerate(fo.BRANCH_COLS)}


def flat(shape2d, voxels):
    """The voxels (z, y, x) in a volume of one plane more on either side."""
    return fc.volume((3, *shape2d), voxels)


def degrees(voxels):
    return voxels[:, V["degree"]].tolist()


# ---- pins of the definition: the shapes checked by hand ----

@pytest.mark.parametrize("n", [3, 4, 9, 64])
@pytest.mark.parametrize("step, cls", [((0, 0, 1), "f"), ((0, 1, 0), "f"), ((1, 0, 0), "f"), ((0, 1, 1), "e"), ((1, 0, -1), "e"),
                                       ((1, 1, 1), "c"), ((1, -1, 1), "c")])
def test_a_straight_line_is_one_chain(n, step, cls):
    start = tuple(0 if d >= 0 else n - 1 for d in step)
    vox, br = fo.trace(fc.line((n, n, n), start, step, n), 1)
    assert degrees(vox) == [1] + [2] * (n - 2) + [1] and br.shape == (1, 16)
    row = dict(zip(fo.BRANCH_COLS, br[0].tolist()))
    assert (row["id"], row["kind"], row["path_voxels"], row["start_degree"], row["end_degree"]) == (1, 0, n - 2, 1, 1)
    assert {c: row[c] for c in "fec"} == {c: (n - 1 if c == cls else 0) for c in "fec"}
    assert row["chord2"] == (n - 1) ** 2 * sum(d * d for d in step)  # the squared extent
    length = (row["f"] + math.sqrt(2.0) * row["e"]) + math.sqrt(3.0) * row["c"]
    assert length == (n - 1) * {"f": 1.0, "e": math.sqrt(2.0), "c": math.sqrt(3.0)}[cls]
    # ranks 1..n-2 from the start node on, the counts grow by one step per rank
    assert vox[1:-1, V["rank"]].tolist() == list(range(1, n - 1)) and vox[1:-1, V[cls]].tolist() == list(range(1, n - 1))
    assert vox[[0, -1], V["branch"]].tolist() == [0, 0] and set(vox[1:-1, V["branch"]].tolist()) == {1}
    assert row["start_index"] == 0 or step[2] < 0 or step[1] < 0  # the head is the path voxel with the smaller index


def test_two_voxels_are_one_link_and_one_voxel_is_a_point():
    vox, br = fo.trace(fc.line((2, 3, 4), (0, 1, 1), (1, 1, 1), 2), 1)
    assert degrees(vox) == [1, 1] and br.tolist() == [[1, 0, 0, 0, 0, 1, 5, 22, 1, 1, 0, 0, 0, -1, -1, 3]]
    vox, br = fo.trace(fc.line((2, 3, 4), (0, 1, 1), (1, 1, 1), 1), 1)
    assert vox.tolist() == [[0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]] and br.shape == (0, 16)
    vox, br = fo.trace(np.zeros((2, 3, 4), np.int32), 1)
    assert vox.shape == (0, 12) and br.shape == (0, 16)


def test_the_square_outline_has_one_voxel_corner_chains():
    vox, br = fo.trace(flat((8, 8), fc.square_outline(6)), 1)
    assert sorted(degrees(vox)) == [2] * 12 + [3] * 8 and br.shape[0] == 8
    assert sorted(br[:, B["path_voxels"]].tolist()) == [1] * 4 + [2] * 4 and set(br[:, B["kind"]].tolist()) == {2}
    corners = br[br[:, B["path_voxels"]] == 1]
    assert (corners[:, B["chord2"]] == 2).all()  # the two terminals of a corner are junction voxels next to each other
    assert (corners[:, B["start_index"]] < corners[:, B["end_index"]]).all()  # a one-voxel chain starts at its smaller neighbour
    assert (corners[:, B["e"]] == 0).all() and (corners[:, B["f"]] == 2).all()
    keys = br[:, B["head_index"]].tolist()
    assert keys == sorted(keys)


@pytest.mark.parametrize("voxels, count", [(fc.cut_corner_square(), 20), (fc.diamond(3), 12), (fc.diamond(1, (1, 2, 2)), 4)])
def test_pure_rings(voxels, count):
    vox, br = fo.trace(flat((9, 9), voxels), 1)
    assert degrees(vox) == [2] * count and vox[:, V["ring"]].all() and br.shape == (1, 16)
    row = dict(zip(fo.BRANCH_COLS, br[0].tolist()))
    m = 1 * 81 + vox[0, 1] * 9 + vox[0, 2]
    assert (row["kind"], row["path_voxels"], row["start_index"], row["end_index"], row["head_index"], row["chord2"]) == (3, count, m, m, m, 0)
    assert (row["start_degree"], row["end_degree"]) == (2, 2) and row["f"] + row["e"] + row["c"] == count  # with the closing step
    ranks = vox[:, V["rank"]]
    assert sorted(ranks.tolist()) == list(range(1, count + 1)) and ranks[0] == 1
    second, last = vox[ranks == 2][0], vox[ranks == count][0]
    around = [r for r in vox if max(abs(r[:3] - vox[0, :3])) == 1]
    assert len(around) == 2 and (second == around[0]).all() and (last == around[1]).all()  # first to the neighbour with the smaller index
    assert vox[0, V["f"]:V["c"] + 1].tolist() == [0, 0, 0]


def test_tee_bump_stem_and_lollipop():
    vox, br = fo.trace(flat((7, 11), fc.tee(4)), 1)
    assert sorted(degrees(vox)) == [1] * 3 + [2] * 6 + [3, 3, 3, 4] and br[:, B["path_voxels"]].tolist() == [2, 2, 2] and br[:, B["kind"]].tolist() == [1] * 3
    # a one-voxel bump on a line has three neighbours: a junction voxel, no end
    bump = [(1, 1, 1 + x) for x in range(9)] + [(1, 2, 5)]
    vox, br = fo.trace(flat((4, 11), bump), 1)
    assert vox[-1, :3].tolist() == [1, 2, 5] and vox[-1, V["degree"]] == 3 and degrees(vox).count(1) == 2
    # a stem of 2: its tip is an end on a junction voxel, a link
    vox, br = fo.trace(flat((5, 11), fc.tee(2)), 1)
    links = br[br[:, B["path_voxels"]] == 0]
    assert links.shape[0] == 1 and links[0, B["kind"]] == 1 and links[0, B["start_degree"]] == 1 and links[0, B["end_degree"]] == 4
    assert links[0, B["head_index"]] == links[0, B["last_index"]] == -1 and links[0, B["chord2"]] == 1 and links[0, B["f"]] == 1
    # the lollipop: one junction voxel, a chain of 11 from it back to itself, a chain of 4 to the end
    vox, br = fo.trace(flat((9, 14), fc.lollipop()), 1)
    assert sorted(degrees(vox)) == [1] + [2] * 15 + [3] and sorted(br[:, B["path_voxels"]].tolist()) == [4, 11]
    loop = br[br[:, B["path_voxels"]] == 11][0]
    assert loop[B["start_index"]] == loop[B["end_index"]] and loop[B["chord2"]] == 0 and loop[B["kind"]] == 2
    assert loop[B["head_index"]] < loop[B["last_index"]] and not vox[:, V["ring"]].any()


def test_only_the_same_id_is_a_neighbour_and_ids_past_k_are_nothing():
    v = fc.line((1, 3, 9), (0, 0, 0), (0, 0, 1), 9, 1) + fc.line((1, 3, 9), (0, 1, 0), (0, 0, 1), 9, 2)
    vox, br = fo.trace(v, 2)
    assert degrees(vox) == ([1] + [2] * 7 + [1]) * 2 and br[:, B["id"]].tolist() == [1, 2] and br[:, B["path_voxels"]].tolist() == [7, 7]
    vox, br = fo.trace(v, 1)
    assert vox.shape[0] == 9 and br[:, B["id"]].tolist() == [1]
    assert fo.trace(v, 0)[0].shape == (0, 12)


def test_the_serpentine_is_one_chain():
    v = fc.serpentine()
    vox, br = fo.trace(v, 1)
    assert br.shape[0] == 1 and br[0, B["path_voxels"]] == vox.shape[0] - 2 == int(v.sum()) - 2 > 5 * 5 * 128
    assert degrees(vox).count(1) == 2 and degrees(vox).count(2) == vox.shape[0] - 2


def test_d2_goes_into_both_tables():
    v = flat((4, 9), [(1, 1, 1 + x) for x in range(7)])
    d2 = (np.arange(v.size, dtype=np.int32).reshape(v.shape) % 11) + 1
    d2[1, 1, 3] = fo.EDT_NONE  # no distance counts as 0
    vox, br = fo.trace(v, 1, d2)
    want = [0 if x == 3 else int(d2[1, 1, x]) for x in range(1, 8)]
    assert vox[:, V["d2"]].tolist() == want
    assert br[0, B["sum_d2"]:B["max_d2"] + 1].tolist() == [sum(want[1:-1]), min(want[1:-1]), max(want[1:-1])]


# ---- brute force on small random volumes ----

def neighbours(a, b):
    return a[3] == b[3] and max(abs(int(p) - int(q)) for p, q in zip(a[:3], b[:3])) == 1


def step_class(a, b):
    return sum(abs(int(p) - int(q)) for p, q in zip(a[:3], b[:3]))


@pytest.mark.parametrize("density", [0.1, 0.3, 0.6])
def test_invariants_by_brute_force(density):
    shape = (3, 4, 5)
    for seed in range(100):
        v = fc.salt(shape, density, 2, 1000 * seed + int(density * 10))
        vox, br = fo.trace(v, 2)
        assert vox[:, :4].tolist() == [[*p, v[tuple(p)]] for p in np.argwhere(v != 0).tolist()]
        for i, r in enumerate(vox):  # the degree, again, by brute force
            assert r[V["degree"]] == sum(neighbours(r, o) for j, o in enumerate(vox) if j != i)
        node = vox[:, V["degree"]] != 2
        assert not vox[node][:, V["branch"]:V["c"] + 1].any() and (vox[~node, V["branch"]] >= 1).all()  # a node or on exactly one branch
        index = lambda r: (int(r[0]) * shape[1] + int(r[1])) * shape[2] + int(r[2])
        where = {index(r): r for r in vox}
        keys = []
        for b, row in enumerate(br, start=1):
            mine = vox[vox[:, V["branch"]] == b]
            mine = mine[np.argsort(mine[:, V["rank"]])]
            n = int(row[B["path_voxels"]])
            assert mine[:, V["rank"]].tolist() == list(range(1, n + 1)) and (mine[:, V["id"]] == row[B["id"]]).all()
            start, end = where[int(row[B["start_index"]])], where[int(row[B["end_index"]])]
            assert (start[V["degree"]], end[V["degree"]]) == (row[B["start_degree"]], row[B["end_degree"]])
            walk = [start, *mine, end] if row[B["kind"]] != 3 else [*mine, mine[0]]
            counts = [0, 0, 0, 0]
            for a, c in zip(walk, walk[1:]):
                assert neighbours(a, c)  # consecutive ranks, and both terminals
                counts[step_class(a, c)] += 1
                if c is not walk[-1]:
                    assert c[V["f"]:V["c"] + 1].tolist() == counts[1:]
            assert row[B["f"]:B["c"] + 1].tolist() == counts[1:]  # the last voxel's counts and the closing step
            assert row[B["chord2"]] == sum((int(p) - int(q)) ** 2 for p, q in zip(start[:3], end[:3]))
            if n:
                assert (index(mine[0]), index(mine[-1])) == (row[B["head_index"]], row[B["last_index"]])
                assert (mine[:, V["ring"]] == (row[B["kind"]] == 3)).all()
                if row[B["kind"]] != 3 and n > 1:
                    assert index(mine[0]) < index(mine[-1])  # the head is the smaller extremal voxel
                if row[B["kind"]] == 3:
                    assert index(mine[0]) == min(index(r) for r in mine) and (start == mine[0]).all()
                keys.append(index(mine[0]))
            else:
                assert start[V["degree"]] == 1 and end[V["degree"]] != 2 and row[B["head_index"]] == -1
                assert end[V["degree"]] != 1 or index(start) < index(end)
                keys.append(index(start))
            assert row[B["kind"]] == (3 if n and mine[0, V["ring"]] else int(start[V["degree"]] >= 3) + int(end[V["degree"]] >= 3))
        assert keys == sorted(keys) and len(set(keys)) == len(keys)  # the branch numbers ascend with the key voxel
        # every end with a node neighbour is in a link, from one side
        ends_on_nodes = sum(1 for r in vox if r[V["degree"]] == 1 and any(neighbours(r, o) and o[V["degree"]] != 2 for o in vox if o is not r))
        pairs = sum(1 for r in vox if r[V["degree"]] == 1 and any(neighbours(r, o) and o[V["degree"]] == 1 for o in vox if o is not r)) // 2
        assert int((br[:, B["path_voxels"]] == 0).sum()) == ends_on_nodes - pairs


SKELETONS = {
    "line": [(1, 1, 1 + x) for x in range(7)], "pair": [(1, 1, 1), (1, 2, 2)], "point": [(1, 2, 2)], "tee": fc.tee(4), "stem": fc.tee(2),
    "ring": fc.cut_corner_square(), "diamond": fc.diamond(3), "lollipop": fc.lollipop(), "theta": fc.theta(),
    "two": [(1, 1, 1 + x) for x in range(5)] + fc.diamond(2, (1, 5, 8)),
}


@pytest.mark.parametrize("name", sorted(SKELETONS))
def test_nodes_minus_branches_is_components_minus_cycles(name):
    """On a skeleton graph, per id: nodes - non-ring branches = the Euler number of the voxel set (26-connected: components - tunnels, a
    thin line has no cavity).  The second id is the same shape shifted, so both are counted apart."""
    from cryovit_amd.analysis.filaments import junction_nodes

    one = flat((9, 14), SKELETONS[name])
    v = np.concatenate([one, 2 * one], axis=0)
    vox, br = fo.trace(v, 2)
    nodes, _ = junction_nodes(vox)
    for ident in (1, 2):
        mine = br[br[:, B["id"]] == ident]
        balance = sum(n["id"] == ident for n in nodes) - int((mine[:, B["kind"]] != 3).sum())
        assert balance == so.euler(v == ident, 26), name


# ---- the host functions on hand-made tables ----

def straight(n=21, ident=1):
    """A line of n voxels along x at (1, 1, 1..n): one chain of length n - 1."""
    return fo.trace(fc.line((3, 3, n + 2), (1, 1, 1), (0, 0, 1), n, ident), ident, np.full((3, 3, n + 2), 4, np.int32))


def test_junction_nodes_and_branch_records():
    from cryovit_amd.analysis.filaments import KINDS, branch_records, junction_nodes

    vox, br = fo.trace(flat((7, 11), fc.tee(4)), 1, np.full((3, 7, 11), 9, np.int32))
    nodes, node_of = junction_nodes(vox)
    assert [(n["node"], n["kind"], n["voxels"]) for n in nodes] == [(1, "end", 1), (2, "junction", 4), (3, "end", 1), (4, "end", 1)]
    assert (nodes[1]["z"], nodes[1]["y"], nodes[1]["x"]) == (1.0, (1 + 1 + 1 + 2) / 4, (4 + 5 + 6 + 5) / 4)
    assert sorted(node_of) == [i for i, d in enumerate(degrees(vox)) if d != 2] and set(node_of.values()) == {1, 2, 3, 4}
    records = branch_records(vox, br)
    assert [(r["branch"], r["kind"], r["start_node"], r["end_node"], r["voxels"]) for r in records] == [
        (1, "end-junction", 1, 2, 2), (2, "end-junction", 2, 3, 2), (3, "end-junction", 2, 4, 2)]
    assert all(r["length"] == 3.0 and r["chord"] == 3.0 and r["tortuosity"] == 1.0 and r["radius_mean"] == r["radius_min"] == r["radius_max"] == 3.0
               for r in records)
    assert (records[0]["sz"], records[0]["sy"], records[0]["sx"], records[0]["ez"], records[0]["ey"], records[0]["ex"]) == (1, 1, 1, 1, 1, 4)
    assert KINDS == ["end-end", "end-junction", "junction-junction", "ring"]
    # a ring has no nodes and no tortuosity; a link no radius; a loop back to one voxel a chord of 0
    ring = branch_records(*fo.trace(flat((9, 9), fc.diamond(3)), 1))[0]
    assert (ring["kind"], ring["start_node"], ring["end_node"]) == ("ring", 0, 0) and math.isnan(ring["tortuosity"])
    assert ring["length"] == (0.0 + math.sqrt(2.0) * 12) + 0.0 and (ring["sz"], ring["sy"], ring["sx"]) == (ring["ez"], ring["ey"], ring["ex"]) == (1, 1, 4)
    link = branch_records(*fo.trace(fc.line((2, 3, 4), (0, 1, 1), (1, 1, 1), 2), 1))[0]
    assert link["voxels"] == 0 and all(math.isnan(link[c]) for c in ("radius_mean", "radius_min", "radius_max"))
    assert link["length"] == link["chord"] == math.sqrt(3.0) and (link["start_node"], link["end_node"]) == (1, 2)
    loop = [r for r in branch_records(*fo.trace(flat((9, 14), fc.lollipop()), 1)) if r["voxels"] == 11][0]
    assert loop["chord"] == 0.0 and math.isnan(loop["tortuosity"]) and loop["start_node"] == loop["end_node"]
    # the square outline: the two junction voxels at a corner are neighbours, one node
    vox, br = fo.trace(flat((8, 8), fc.square_outline(6)), 1)
    assert len(junction_nodes(vox)[0]) == 4 and all(n["voxels"] == 2 for n in junction_nodes(vox)[0])
    corner = [r for r in branch_records(vox, br) if r["voxels"] == 1]
    assert len(corner) == 4 and all(r["start_node"] == r["end_node"] for r in corner)


def test_filament_rows():
    from cryovit_amd.analysis.filaments import FILAMENT_COLUMNS, filament_rows

    v = flat((9, 14), fc.lollipop())
    v[0, 0, 0] = 1  # a point
    v = np.concatenate([v, 3 * flat((9, 14), fc.diamond(3))], axis=0)
    rows = filament_rows(*fo.trace(v, 3), 3)
    assert [list(r) for r in rows] == [FILAMENT_COLUMNS] * 3
    stick, loop = 5.0, (0.0 + math.sqrt(2.0) * 12) + 0.0  # every step of a diamond is an edge step
    assert list(rows[0].values())[:4] == [2, 0, 1, 1] and rows[0]["filament_longest"] == loop and math.isnan(rows[0]["filament_tortuosity"])
    assert rows[0]["filament_length"] in (stick + loop, loop + stick)
    assert list(rows[1].values())[:6] == [0, 0, 0, 0, 0.0, 0.0] and math.isnan(rows[1]["filament_tortuosity"])
    assert list(rows[2].values())[:4] == [1, 1, 0, 0] and rows[2]["filament_length"] == rows[2]["filament_longest"] == math.sqrt(2.0) * 12
    tee = filament_rows(*fo.trace(flat((7, 11), fc.tee(4)), 1), 1)[0]
    assert tee == dict(zip(FILAMENT_COLUMNS, (3, 0, 1, 0, 9.0, 3.0, 1.0)))  # 9, where skeleton_length counts the clique's pairs too
    with pytest.raises(ValueError, match="ids outside 1..2"):
        filament_rows(*fo.trace(v, 3), 2)


def test_points_along_a_straight_chain():
    from cryovit_amd.analysis.filaments import TraceOptions, sample_points

    vox, br = straight(21)
    pts = sample_points(vox, br, TraceOptions(trace=True, trace_scale=4.0, trace_angpix=2.5))
    assert [p["arc"] for p in pts] == [0.0, 8.0, 16.0] and [p["point"] for p in pts] == [1, 2, 3] and {p["branch"] for p in pts} == {1}
    assert [(p["z"], p["y"], p["x"]) for p in pts] == [(1.0, 1.0, 1.0), (1.0, 1.0, 9.0), (1.0, 1.0, 17.0)]
    assert all((p["tz"], p["ty"], abs(p["tx"])) == (0.0, 0.0, 1.0) for p in pts) and len({p["tx"] for p in pts}) == 1
    assert [p["track"] for p in pts] == [0.0, 8 * 4.0 * 2.5, 16 * 4.0 * 2.5]
    assert [(p["pz"], p["py"], p["px"]) for p in pts] == [(5.5, 5.5, (x + 0.5) * 4 - 0.5) for x in (1.0, 9.0, 17.0)]
    assert all((p["rot"], p["tilt"], p["psi"], p["radius"]) == (0.0 if p["tx"] > 0 else 180.0, 90.0, 0.0, 2.0) for p in pts)
    # at a spacing the length is a multiple of, the last position is the end node; a fractional spacing lies between voxels
    assert [p["x"] for p in sample_points(vox, br, TraceOptions(trace_spacing=5.0))] == [1.0, 6.0, 11.0, 16.0, 21.0]
    assert [p["x"] for p in sample_points(vox, br, TraceOptions(trace_spacing=7.5))] == [1.0, 8.5, 16.0]
    # along z the tilt is 0 or 180
    pts = sample_points(*fo.trace(fc.line((12, 3, 3), (0, 1, 1), (1, 0, 0), 12), 1), TraceOptions())
    assert [p["arc"] for p in pts] == [0.0, 8.0] and all(abs(p["tz"]) == 1.0 and p["tilt"] in (0.0, 180.0) for p in pts)


def circle(radius):
    """(y, x) of a thin digital circle about (0, 0): one voxel per column in the octant next to the y axis, and its 8 images, so no
    voxel has a third neighbour."""
    octant = [(round(math.sqrt(radius * radius - x * x)), x) for x in range(int(radius / math.sqrt(2.0)) + 2)]
    out = set()
    for y, x in octant:
        if x <= y:
            out |= {(a, b) for p, q in ((y, x), (x, y)) for a in (p, -p) for b in (q, -q)}
    return sorted(out)


def quarter_circle(radius=24):
    """The quarter of ``circle`` with y, x >= 0 in the plane z = 1: a chain with face and edge steps."""
    return [(1, 1 + y, 1 + x) for y, x in circle(radius) if y >= 0 and x >= 0]


def test_tangents_on_a_quarter_circle_against_a_restatement():
    from cryovit_amd.analysis.filaments import TraceOptions, sample_points

    vox, br = fo.trace(flat((28, 28), quarter_circle()), 1)
    assert br.shape[0] == 1 and br[0, B["kind"]] == 0, "the drawing must be one chain: thin, without a junction"
    opts = TraceOptions(trace_spacing=3.0, trace_window=5.0)
    pts = sample_points(vox, br, opts)
    # the restatement: the polyline in rank order with numpy's interpolation
    path = vox[vox[:, V["degree"]] == 2]
    path = path[np.argsort(path[:, V["rank"]])][:, :3].astype(np.float64)
    ends = vox[vox[:, V["degree"]] == 1][:, :3].astype(np.float64)
    near = 0 if np.abs(ends[0] - path[0]).max() == 1 else 1
    line = np.vstack([ends[near], path, ends[1 - near]])
    arc = np.concatenate([[0.0], np.cumsum(np.sqrt(((line[1:] - line[:-1]) ** 2).sum(1)))])
    at = lambda s: np.array([np.interp(min(max(s, 0.0), arc[-1]), arc, line[:, c]) for c in range(3)])
    assert len(pts) == int(arc[-1] // 3) + 1 and abs(arc[-1] - ((br[0, B["f"]] + math.sqrt(2.0) * br[0, B["e"]]) + math.sqrt(3.0) * br[0, B["c"]])) < 1e-9
    for j, p in enumerate(pts):
        d = at(3.0 * j + 5.0) - at(3.0 * j - 5.0)
        t = d / np.sqrt((d * d).sum())
        assert np.abs(np.array([p["tz"], p["ty"], p["tx"]]) - t).max() <= 1e-12 and np.abs(np.array([p["z"], p["y"], p["x"]]) - at(3.0 * j)).max() <= 1e-12
    # and it turns by a quarter: from along y to along x (either polarity)
    assert abs(abs(pts[0]["ty"]) - 1) < 0.05 and abs(abs(pts[-1]["tx"]) - 1) < 0.05


def test_a_rings_tangent_is_continuous_across_m():
    from cryovit_amd.analysis.filaments import TraceOptions, sample_points

    vox, br = fo.trace(flat((27, 27), [(1, 13 + y, 13 + x) for y, x in circle(12)]), 1)
    assert br.shape[0] == 1 and br[0, B["kind"]] == 3, "the drawing must be a pure ring"
    pts = sample_points(vox, br, TraceOptions(trace_spacing=1.0, trace_window=4.0))
    total = (br[0, B["f"]] + math.sqrt(2.0) * br[0, B["e"]]) + 0.0
    assert len(pts) == int(total) + 1 and (pts[0]["z"], pts[0]["y"], pts[0]["x"]) == tuple(float(c) for c in vox[0, :3])
    turn = [sum(a[c] * b[c] for c in ("tz", "ty", "tx")) for a, b in zip(pts, pts[1:] + pts[:1])]
    assert min(turn) > 0.9, min(turn)  # neighbouring tangents agree all the way round, across the first voxel too
    assert not any(math.isnan(p["tx"]) for p in pts)
    # a spacing that divides the ring: no position at the length itself, which is the first voxel again
    vox, br = fo.trace(flat((9, 9), fc.diamond(3)), 1)
    pts = sample_points(vox, br, TraceOptions(trace_spacing=3 * math.sqrt(2.0), trace_window=1.0))
    assert len(pts) == 4 and len({(p["y"], p["x"]) for p in pts}) == 4 and pts[0]["arc"] == 0.0


def test_min_length_drops_short_branches_from_the_points_only():
    from cryovit_amd.analysis.filaments import TraceOptions, branch_records, filament_rows, sample_points

    vox, br = fo.trace(flat((9, 14), fc.lollipop()), 1)
    every = sample_points(vox, br, TraceOptions(trace_spacing=2.0))
    assert {p["branch"] for p in every} == {1, 2}
    long_only = sample_points(vox, br, TraceOptions(trace_spacing=2.0, trace_min_length=6.0))
    kept = {r["branch"] for r in branch_records(vox, br) if r["length"] >= 6.0}
    assert len(kept) == 1 and {p["branch"] for p in long_only} == kept and [p["point"] for p in long_only] == list(range(1, len(long_only) + 1))
    assert len(branch_records(vox, br)) == 2 and filament_rows(vox, br, 1)[0]["filament_branches"] == 2
    assert sample_points(vox, br, TraceOptions(trace_min_length=1000.0)) == []


def test_filament_volume():
    from cryovit_amd.analysis.filaments import filament_volume

    v = flat((7, 11), fc.tee(4))
    vox, _ = fo.trace(v, 1)
    out = filament_volume(vox, v.shape)
    assert out.dtype == np.int32 and ((out != 0) == (v != 0)).all() and sorted(np.unique(out).tolist()) == [-1, 0, 1, 2, 3]
    assert (out == -1).sum() == 7 and filament_volume(vox[:0], v.shape).any() == False  # noqa: E712


# ---- the writers ----

def test_writers_round_trip_and_are_reproducible(tmp_path):
    from cryovit_amd.analysis.filaments import (BRANCH_CSV_COLUMNS, HELICAL_STAR_COLUMNS, POINT_CSV_COLUMNS, TraceOptions, branch_records,
                                                read_branches_csv, read_points_csv, read_star, sample_points, write_branches_csv,
                                                write_helical_star, write_points_csv)

    v = flat((9, 14), fc.lollipop())
    v[1, 8, 0], v[2, 8, 1] = 1, 1  # a link
    vox, br = fo.trace(v, 1, np.full(v.shape, 5, np.int32))
    opts = TraceOptions(trace=True, trace_spacing=3.0, trace_scale=2.0, trace_angpix=1.7)
    records, points = branch_records(vox, br), sample_points(vox, br, opts)
    paths = (write_branches_csv(tmp_path / "a" / "b.csv", records), write_points_csv(tmp_path / "a" / "p.csv", points),
             write_helical_star(tmp_path / "a" / "p.star", points, "tomo_1"))
    first = [p.read_bytes() for p in paths]
    assert not list((tmp_path / "a").glob("*.tmp"))
    back = read_branches_csv(paths[0])
    assert [list(r) for r in back] == [BRANCH_CSV_COLUMNS] * len(records) == [BRANCH_CSV_COLUMNS] * 3
    for r, w in zip(back, records):
        for c in BRANCH_CSV_COLUMNS:
            assert r[c] == w[c] if isinstance(w[c], (int, str)) else (math.isnan(r[c]) and math.isnan(w[c])) or abs(r[c] - w[c]) <= 5e-7, c
    back = read_points_csv(paths[1])
    assert [list(r) for r in back] == [POINT_CSV_COLUMNS] * len(points) and len(points) > 6
    for r, w in zip(back, points):
        assert all(r[c] == w[c] if isinstance(w[c], int) else abs(r[c] - w[c]) <= 5e-7 for c in POINT_CSV_COLUMNS)
    names, rows = read_star(paths[2])
    assert names == HELICAL_STAR_COLUMNS and names[-2:] == ["_rlnHelicalTubeID", "_rlnHelicalTrackLengthAngst"] and len(rows) == len(points)
    for row, w in zip(rows, points):
        assert row[0] == "tomo_1" and [float(c) for c in row[1:7]] == [round(w[c], 6) for c in ("px", "py", "pz", "rot", "tilt", "psi")]
        assert int(row[7]) == w["branch"] and abs(float(row[8]) - w["arc"] * 2.0 * 1.7) <= 5e-7
    assert paths[2].read_text().startswith("\n# version 30001\n\ndata_particles\n\nloop_\n_rlnMicrographName #1\n")
    again = (write_branches_csv(paths[0], branch_records(vox.copy(), br.copy())), write_points_csv(paths[1], sample_points(vox, br, opts)),
             write_helical_star(paths[2], sample_points(vox, br, opts), "tomo_1"))
    assert [p.read_bytes() for p in again] == first
    with pytest.raises(ValueError, match="white space"):
        write_helical_star(tmp_path / "x.star", points, "a b")
    # no branches: headers only
    assert write_branches_csv(tmp_path / "e.csv", []).read_text() == ",".join(BRANCH_CSV_COLUMNS) + "\n"
    assert read_points_csv(write_points_csv(tmp_path / "f.csv", [])) == []


# ---- the options record and both entry points ----

BAD = [(dict(trace_spacing=0.5), "trace_spacing must be a finite number >= 1, got 0.5"),
       (dict(trace_spacing=math.inf), "trace_spacing must be a finite number >= 1, got inf"),
       (dict(trace_spacing="8"), "trace_spacing must be a finite number >= 1, got '8'"),
       (dict(trace_window=0.0), "trace_window must be a finite number >= 1, got 0.0"),
       (dict(trace_window=math.nan), "trace_window must be a finite number >= 1, got nan"),
       (dict(trace_min_length=-1.0), "trace_min_length must be a finite number >= 0, got -1.0"),
       (dict(trace_scale=0.0), "trace_scale must be a finite number > 0, got 0.0"),
       (dict(trace_scale=True), "trace_scale must be a finite number > 0, got True"),
       (dict(trace_angpix=-2.0), "trace_angpix must be a finite number > 0, got -2.0")]


def test_options_record():
    from cryovit_amd.analysis.filaments import TraceOptions

    assert dataclasses.astuple(TraceOptions()) == (False, 8.0, 4.0, 0.0, 1.0, 1.0)
    assert [f.name for f in dataclasses.fields(TraceOptions)] == ["trace", "trace_spacing", "trace_window", "trace_min_length", "trace_scale", "trace_angpix"]
    for good in (dict(), dict(trace=True, trace_spacing=1, trace_window=1.0, trace_min_length=0), dict(trace_spacing=np.float32(2.5), trace_scale=0.25, trace_angpix=13.33)):
        opts = TraceOptions(**good)
        assert opts.validate() is opts
    with pytest.raises(dataclasses.FrozenInstanceError):
        TraceOptions().trace = True
    for on in (False, True):
        for bad, message in BAD:
            with pytest.raises(ValueError) as e:
                TraceOptions(trace=on, **bad).validate()
            assert str(e.value) == message


def test_every_field_is_a_parameter_of_both_entry_points():
    from cryovit_amd.analysis.filaments import TraceOptions
    from cryovit_amd.analysis.instances import InstanceOptions, label_file, measure
    from cryovit_amd.run.infer_model import run_inference

    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(TraceOptions):
            assert params[f.name].default == f.default and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)
    assert inspect.signature(measure).parameters["trace"].default is None
    assert not any(f.name.startswith("trace") for f in dataclasses.fields(InstanceOptions)) and "trace" not in InstanceOptions.MEASUREMENTS


@pytest.mark.parametrize("bad, message", BAD[::2])
def test_both_entry_points_refuse_a_bad_value_with_the_same_words(tmp_path, bad, message):
    """Before anything is read: neither the prediction file nor the model file exists."""
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError) as from_file:
        label_file(tmp_path / "none.hdf", "mito", result_dir=tmp_path / "out", trace=True, **bad)
    with pytest.raises(ValueError) as from_infer:
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", instances=True, trace=True, **bad)
    assert str(from_file.value) == str(from_infer.value) == message and not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="^trace=True needs instances=True: the filaments are traced along the skeletons of the labelled instances$"):
        run_inference([tmp_path / "none.hdf"], tmp_path / "none.model", tmp_path / "out", trace=True)


FLAGS = ("--trace", "--trace-spacing", "--trace-window", "--trace-min-length", "--trace-scale", "--trace-angpix")


def test_cli_surface_and_refusals(tmp_path, monkeypatch):
    import sys

    from typer.testing import CliRunner

    from cryovit_amd import cli as cli_module
    from cryovit_amd.cli import cli

    for command in ("infer", "instances"):
        res = CliRunner().invoke(cli, [command, "--help"], terminal_width=200)
        assert res.exit_code == 0, res.output
        for word in FLAGS:
            assert word in res.output, (command, word)
    assert "[--trace [--trace-spacing S] [--trace-window H] [--trace-min-length L] [--trace-scale F] [--trace-angpix A]]" in cli_module.__doc__
    for name in ("cryovit_amd.run.infer_model", "cryovit_amd.analysis.instances"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    model = ["--model", str(tmp_path / "m.model")]
    inst = ["instances", str(tmp_path), "--label", "mito", "--trace"]
    cases = [(["infer", str(tmp_path), *model, "--trace"], "--trace needs --instances"), ([*inst, "--trace-spacing", "x"], "--trace-spacing")]
    # the words of TraceOptions.validate, from the command line
    for flag, value, message in (("--trace-spacing", "0.5", BAD[0][1]), ("--trace-spacing", "inf", BAD[1][1]), ("--trace-window", "0.0", BAD[3][1]),
                                 ("--trace-window", "nan", BAD[4][1]), ("--trace-min-length", "-1.0", BAD[5][1]), ("--trace-scale", "0.0", BAD[6][1]),
                                 ("--trace-angpix", "-2.0", BAD[8][1])):
        cases.append(([*inst, flag, value], message))
        cases.append((["infer", str(tmp_path), *model, "--instances", "--trace", flag, value], message))
    for args, words in cases:
        res = CliRunner().invoke(cli, args, terminal_width=200)
        assert res.exit_code == 2, (args, res.output)  # a usage error while the arguments are parsed
        said = " ".join(res.output.replace("│", " ").split())  # the error box breaks lines
        assert words in said, (args, res.output)
        assert "cryovit_amd.run.infer_model" not in sys.modules and "cryovit_amd.analysis.instances" not in sys.modules


def test_cli_passes_the_options_on(tmp_path, monkeypatch):
    import importlib

    from typer.testing import CliRunner

    from cryovit_amd.cli import cli

    instances = importlib.import_module("cryovit_amd.analysis.instances")  # the module the command imports from
    infer_model = importlib.import_module("cryovit_amd.run.infer_model")
    seen = []
    monkeypatch.setattr(instances, "label_file", lambda f, label, **kw: seen.append(kw) or f)
    monkeypatch.setattr(infer_model, "run_inference", lambda files, model, result, **kw: seen.append(kw) or [])
    (tmp_path / "t.hdf").write_bytes(b"")
    (tmp_path / "m.model").write_bytes(b"")
    names = ("trace", "trace_spacing", "trace_window", "trace_min_length", "trace_scale", "trace_angpix")
    for extra, want in (([], (False, 8.0, 4.0, 0.0, 1.0, 1.0)), (["--trace"], (True, 8.0, 4.0, 0.0, 1.0, 1.0)),
                        (["--trace", "--trace-spacing", "12.5", "--trace-window", "3", "--trace-min-length", "20", "--trace-scale", "4", "--trace-angpix", "3.42"],
                         (True, 12.5, 3.0, 20.0, 4.0, 3.42))):
        res = CliRunner().invoke(cli, ["instances", str(tmp_path), "--label", "mito", *extra])
        assert res.exit_code == 0, res.output
        assert tuple(seen[-1][n] for n in names) == want
        res = CliRunner().invoke(cli, ["infer", str(tmp_path), "--model", str(tmp_path / "m.model"), "--result-folder", str(tmp_path / "r"), "--instances", *extra])
        assert res.exit_code == 0, res.output
        assert tuple(seen[-1][n] for n in names) == want and seen[-1]["instances"] is True


# ---- the place of the tracing in the pipeline ----

@pytest.fixture
def recorded(monkeypatch):
    """The ``engine.ops`` entry points of the pipeline replaced by stand-ins that return host tensors of the right shape and dtype and
    append (name, the scalar arguments) to the returned list (as tests/test_cpu_picks.py does).  The skeleton of the stand-in is the
    labelled volume itself: the prediction is drawn one voxel thin."""
    from cryovit_amd.engine import ops
    from cryovit_amd.run import sharding

    calls = []

    def label_components(mask, *, connectivity=26, min_size=0):
        calls.append(("label_components", connectivity, min_size))
        lab, tab = co.components(mask.numpy(), connectivity, min_size)
        return torch.from_numpy(lab), torch.from_numpy(tab)

    def edt_squared(src, *, sites="zero", slices=False):
        calls.append(("edt_squared", sites))
        return torch.full(src.shape, 4, dtype=torch.int32)

    def skeletonize_instances(labels, k, *, d2=None, end_radius=2.0, max_cycles=4096):
        calls.append(("skeletonize_instances", k, d2 is not None, end_radius))
        table = torch.zeros((k, 8), dtype=torch.int64)
        table[:, 0] = torch.bincount(labels.flatten().long(), minlength=k + 1)[1:]
        return labels.clone(), table

    def instance_thickness(labels, k, *, d2=None):
        calls.append(("instance_thickness", k, d2 is not None))
        return torch.zeros(labels.shape, dtype=torch.int32), torch.zeros((k, 5), dtype=torch.int64)

    def trace_skeleton(skeleton, k, *, d2=None, counters=None):
        calls.append(("trace_skeleton", k, d2 is not None))
        vox, br = fo.trace(skeleton.numpy(), k, None if d2 is None else d2.numpy())
        return torch.from_numpy(vox), torch.from_numpy(br)

    def pick_surface(labels, k, *, spacing, radius, seed, max_rounds=4096):
        calls.append(("pick_surface", k))
        return torch.zeros((0, 8), dtype=torch.int32)

    for stub in (label_components, edt_squared, skeletonize_instances, instance_thickness, trace_skeleton, pick_surface):
        monkeypatch.setattr(ops, stub.__name__, stub)
    monkeypatch.setattr(sharding, "select_device", lambda device=None: torch.device("cpu"))
    return calls


@pytest.fixture
def prediction(tmp_path):
    m = fc.volume((5, 7, 11), fc.tee(4)).astype(np.uint8)
    m[4, 0, 0:9] = 1  # a second instance: a line
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("data", np.zeros(m.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", m, compression="gzip")
        f.create_dataset("mito_filaments", np.ones(m.shape, np.int32), compression="gzip")  # of an earlier run
    return tmp_path / "t.hdf"


def test_trace_turns_the_skeleton_on_and_its_columns_follow_the_skeletons(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import FILAMENT_COLUMNS, INSTANCE_COLUMNS, PICK_COLUMNS, SKELETON_COLUMNS, THICKNESS_COLUMNS, label_file
    from cryovit_amd.analysis.filaments import TraceOptions, branch_records, read_branches_csv, read_points_csv, read_star, sample_points

    options = dict(trace=True, trace_spacing=2.0, trace_window=1.5, trace_scale=2.0, trace_angpix=3.0)
    out = label_file(prediction, "mito", result_dir=tmp_path / "out", thickness=True, pick=True, skeleton_end_radius=1.5, **options)
    assert recorded == [("label_components", 26, 0), ("edt_squared", "zero"), ("skeletonize_instances", 2, True, 1.5), ("trace_skeleton", 2, True),
                        ("instance_thickness", 2, True), ("pick_surface", 2)]  # one distance map for all three
    found = io.read_all_flat(out)
    assert sorted(found) == ["data", "mito_filaments", "mito_instances", "mito_preds", "mito_skeleton", "mito_thickness"]
    lines = (tmp_path / "out" / "instances" / "t_mito.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + SKELETON_COLUMNS + FILAMENT_COLUMNS + THICKNESS_COLUMNS + PICK_COLUMNS
    skeleton = found["mito_skeleton"]
    vox, br = fo.trace(skeleton, 2, np.full(skeleton.shape, 4, np.int32))
    volume = found["mito_filaments"]
    assert volume.dtype == np.int32 and ((volume != 0) == (skeleton != 0)).all() and (volume == -1).sum() == 7 + 2 and volume.max() == br.shape[0] == 4
    assert (volume[vox[:, 0], vox[:, 1], vox[:, 2]] == np.where(vox[:, 4] == 2, vox[:, 5], -1)).all()
    base = tmp_path / "out" / "filaments"
    assert sorted(p.name for p in base.iterdir()) == ["t_mito.csv", "t_mito.star", "t_mito_branches.csv"]
    want = branch_records(vox, br)
    got = read_branches_csv(base / "t_mito_branches.csv")
    assert [(g["branch"], g["id"], g["kind"], g["voxels"]) for g in got] == [(w["branch"], w["id"], w["kind"], w["voxels"]) for w in want]
    assert sorted(g["id"] for g in got) == [1, 2, 2, 2] or sorted(g["id"] for g in got) == [1, 1, 1, 2]
    points = sample_points(vox, br, TraceOptions(**options))
    got = read_points_csv(base / "t_mito.csv")
    assert len(got) == len(points) > 8 and all(abs(g["px"] - w["px"]) <= 5e-7 and g["branch"] == w["branch"] for g, w in zip(got, points))
    names, rows = read_star(base / "t_mito.star")
    assert len(rows) == len(points) and {row[0] for row in rows} == {"t"} and [float(r[8]) for r in rows[:2]] == [0.0, 2.0 * 2.0 * 3.0]
    per_id = {int(line.split(",")[0]): line.split(",") for line in lines[1:]}
    at = lines[0].split(",").index("filament_branches")
    assert sorted(row[at] for row in per_id.values()) == ["1", "3"]


def test_without_trace_nothing_is_issued_and_nothing_changes(prediction, recorded, tmp_path):
    """``trace=False`` is the code path of before: the same calls, and the same bytes in the instance CSV and in the HDF file, whatever
    the other trace options say; the dataset of an earlier run is dropped either way."""
    from cryovit_amd.analysis import label_file

    bare = label_file(prediction, "mito", result_dir=tmp_path / "bare", skeleton=True, thickness=True)
    calls = list(recorded)
    del recorded[:]
    off = label_file(prediction, "mito", result_dir=tmp_path / "off", skeleton=True, thickness=True, trace=False, trace_spacing=3.0, trace_window=2.0,
                     trace_min_length=5.0, trace_scale=3.0, trace_angpix=2.0)
    assert recorded == calls == [("label_components", 26, 0), ("edt_squared", "zero"), ("skeletonize_instances", 2, True, 2.0), ("instance_thickness", 2, True)]
    assert Path(bare).read_bytes() == Path(off).read_bytes()
    assert sorted(io.read_all_flat(off)) == ["data", "mito_instances", "mito_preds", "mito_skeleton", "mito_thickness"]
    assert (tmp_path / "bare" / "instances" / "t_mito.csv").read_bytes() == (tmp_path / "off" / "instances" / "t_mito.csv").read_bytes()
    assert "filament" not in (tmp_path / "off" / "instances" / "t_mito.csv").read_text()
    assert not (tmp_path / "bare" / "filaments").exists() and not (tmp_path / "off" / "filaments").exists()
    del recorded[:]
    label_file(prediction, "mito", result_dir=tmp_path / "plain")
    assert recorded == [("label_components", 26, 0)]


def test_measure_as_infer_calls_it(recorded):
    from cryovit_amd.analysis.filaments import FILAMENT_COLUMNS, TraceOptions
    from cryovit_amd.analysis.instances import InstanceOptions, Measured, measure
    from cryovit_amd.analysis.skeleton import SKELETON_COLUMNS

    labels = torch.from_numpy(flat((7, 11), fc.tee(4)))
    found = measure(labels, 1, None, InstanceOptions(), trace=TraceOptions(trace=True))
    assert recorded == [("edt_squared", "zero"), ("skeletonize_instances", 1, True, 2.0), ("trace_skeleton", 1, True)]
    assert [list(e) for e in found.extra] == [SKELETON_COLUMNS + FILAMENT_COLUMNS]
    assert found.filament_voxels.dtype == torch.int32 and tuple(found.filament_voxels.shape) == (13, 12)
    assert found.filament_branches.dtype == torch.int64 and tuple(found.filament_branches.shape) == (3, 16) and found.skeleton is not None
    host = found.arrays(lambda a: a.numpy())
    assert isinstance(host.filament_voxels, np.ndarray) and isinstance(host.filament_branches, np.ndarray)
    del recorded[:]
    before = measure(labels, 1, None, InstanceOptions())
    for off in (None, TraceOptions(), TraceOptions(trace_spacing=3.0, trace_scale=2.0)):
        none = measure(labels, 1, None, InstanceOptions(), trace=off)
        assert recorded == [] and none == before and none.filament_voxels is None and none.filament_branches is None and none.extra == [{}]
    assert {"filament_voxels", "filament_branches"} <= {f.name for f in dataclasses.fields(Measured)}


# ---- the library's entries, before the device ----

@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


A = 1 << 20  # a made-up, 16-B aligned address: no call of the table dereferences a pointer
BIG = 1 << 40
WORDS = 9 * 9 * 2  # of one bitmap of a 9 x 9 x 70 volume
NV = 100  # voxels of the made-up tables
STATE = 2 * NV * 20  # the bytes of the states of NV voxels

ENTRIES = {
    "cvx_trace_workspace_bytes": dict(D=9, H=9, W=70),
    "cvx_trace_count": dict(sk=A, D=9, H=9, W=70, k=1, bits=A + 4096, workspace_bytes=BIG, row_first=A + 8192, totals=A + 16384),
    "cvx_trace_emit": dict(sk=A, d2=A + 65536, bits=A + 4096, row_first=A + 8192, D=9, H=9, W=70, k=1, workspace_bytes=BIG, N=NV, voxels=A + 16384,
                           nbrs=A + 32768),
    "cvx_trace_rank": dict(voxels=A, nbrs=A + 8192, cut=None, N=NV, rounds=7, state_a=A + 16384, state_b=A + 32768),
    "cvx_trace_rings": dict(voxels=A, state=A + 16384, N=NV, cut=A + 8192, any=A + 4096),
    "cvx_trace_keys": dict(voxels=A, nbrs=A + 8192, state=A + 16384, cut=None, N=NV, keys=A + 32768, total=A + 4096),
    "cvx_trace_branches": dict(voxels=A, nbrs=A + 8192, state=A + 16384, cut=None, first=A + 32768, D=9, H=9, W=70, N=NV, B=10, branches=A + 65536),
}
EXTENTS = [(dict(D=-1), "negative extent"), (dict(H=-1), "negative extent"), (dict(W=-1), "negative extent"),
           (dict(D=32769), "an extent above 32768"), (dict(W=32769, H=1, D=1), "an extent above 32768"),
           (dict(D=2048, H=1024, W=1024), "D*H*W must be <= 2^31 - 2")]
SHORT = [(dict(workspace_bytes=8 * WORDS - 1), "workspace shorter than cvx_trace_workspace_bytes"), (dict(workspace_bytes=0), "workspace shorter than cvx_trace_workspace_bytes"),
         (dict(workspace_bytes=-1), "workspace shorter than cvx_trace_workspace_bytes")]
COUNT = [(dict(N=-1), "N outside [0, 2^31 - 2]"), (dict(N=2**31 - 1), "N outside [0, 2^31 - 2]")]
REFUSED = {
    "cvx_trace_count": EXTENTS + SHORT + [
        (dict(k=-1), "k < 0"), (dict(D=-1, k=-1), "negative extent"), (dict(sk=None), "null pointer"), (dict(bits=None), "null pointer"),
        (dict(row_first=None), "null pointer"), (dict(totals=None), "null pointer"), (dict(k=0, totals=None), "null pointer"),
        (dict(sk=A + 2), "misaligned pointer"), (dict(bits=A + 4100), "misaligned pointer"), (dict(row_first=A + 8194), "misaligned pointer"),
        (dict(totals=A + 16388), "misaligned pointer")],
    "cvx_trace_emit": EXTENTS + SHORT + [
        (dict(k=-1), "k < 0"), (dict(N=-1), "N outside [0, D*H*W]"), (dict(N=9 * 9 * 70 + 1), "N outside [0, D*H*W]"), (dict(D=0, N=1), "N outside [0, D*H*W]"),
        (dict(sk=None), "null pointer"), (dict(bits=None), "null pointer"), (dict(row_first=None), "null pointer"), (dict(voxels=None), "null pointer"),
        (dict(nbrs=None), "null pointer"), (dict(sk=A + 2), "misaligned pointer"), (dict(d2=A + 65537), "misaligned pointer"),
        (dict(bits=A + 4100), "misaligned pointer"), (dict(row_first=A + 8193), "misaligned pointer"), (dict(voxels=A + 16386), "misaligned pointer"),
        (dict(nbrs=A + 32770), "misaligned pointer")],
    "cvx_trace_rank": COUNT + [
        (dict(rounds=-1), "rounds outside [0, 32]"), (dict(rounds=33), "rounds outside [0, 32]"), (dict(voxels=None), "null pointer"),
        (dict(nbrs=None), "null pointer"), (dict(state_a=None), "null pointer"), (dict(state_b=None), "null pointer"),
        (dict(voxels=A + 1), "misaligned pointer"), (dict(nbrs=A + 8194), "misaligned pointer"), (dict(cut=A + 4097), "misaligned pointer"),
        (dict(state_a=A + 16386), "misaligned pointer"), (dict(state_b=A + 32769), "misaligned pointer"),
        (dict(state_b=A + 16384), "state_a and state_b must not overlap"), (dict(state_b=A + 16384 + STATE - 4), "state_a and state_b must not overlap"),
        (dict(state_b=A + 16384 - STATE + 4), "state_a and state_b must not overlap")],
    "cvx_trace_rings": COUNT + [
        (dict(voxels=None), "null pointer"), (dict(state=None), "null pointer"), (dict(cut=None), "null pointer"), (dict(any=None), "null pointer"),
        (dict(N=0, any=None), "null pointer"), (dict(voxels=A + 2), "misaligned pointer"), (dict(state=A + 16385), "misaligned pointer"),
        (dict(cut=A + 8195), "misaligned pointer"), (dict(any=A + 4098), "misaligned pointer")],
    "cvx_trace_keys": COUNT + [
        (dict(voxels=None), "null pointer"), (dict(nbrs=None), "null pointer"), (dict(keys=None), "null pointer"), (dict(total=None), "null pointer"),
        (dict(N=0, total=None), "null pointer"), (dict(state=None, cut=A + 65536), "a cut without a state"),
        (dict(voxels=A + 2), "misaligned pointer"), (dict(nbrs=A + 8193), "misaligned pointer"), (dict(state=A + 16386), "misaligned pointer"),
        (dict(cut=A + 65538), "misaligned pointer"), (dict(keys=A + 32770), "misaligned pointer"), (dict(total=A + 4100), "misaligned pointer")],
    "cvx_trace_branches": EXTENTS + [
        (dict(N=-1), "N outside [0, D*H*W]"), (dict(N=9 * 9 * 70 + 1), "N outside [0, D*H*W]"), (dict(B=-1), "B outside [0, N]"),
        (dict(B=NV + 1), "B outside [0, N]"), (dict(voxels=None), "null pointer"), (dict(nbrs=None), "null pointer"), (dict(first=None), "null pointer"),
        (dict(branches=None), "null pointer"), (dict(state=None, cut=A + 131072), "a cut without a state"),
        (dict(voxels=A + 2), "misaligned pointer"), (dict(nbrs=A + 8193), "misaligned pointer"), (dict(state=A + 16386), "misaligned pointer"),
        (dict(cut=A + 131074), "misaligned pointer"), (dict(first=A + 32770), "misaligned pointer"), (dict(branches=A + 65540), "misaligned pointer")],
}
# what returns 0 before any HIP call
ACCEPTED = {
    "cvx_trace_emit": [dict(N=0), dict(k=0), dict(N=0, sk=None, bits=None, row_first=None, voxels=None, nbrs=None, workspace_bytes=0), dict(D=0, N=0)],
    "cvx_trace_rank": [dict(N=0), dict(N=0, voxels=None, nbrs=None, state_a=None, state_b=None)],
    "cvx_trace_branches": [dict(N=0, B=0), dict(N=0, B=0, voxels=None, nbrs=None, state=None, first=None, branches=None), dict(D=0, N=0, B=0)],
}


def call(lib, name, over):
    lib.cvx_device_arch(None, 0)  # resets the text to a known one: "cvx_device_arch: bad buffer"
    rc = getattr(lib, name)(*{**ENTRIES[name], **over}.values(), None)
    return rc, lib.cvx_last_error().decode()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_entries_refuse_before_the_device(lib, name):
    for over, why in REFUSED[name]:
        rc, text = call(lib, name, over)
        assert (rc, text) == (-1, f"{name.removeprefix('cvx_')}: {why}"), (name, over)  # CVX_ERR_ARG, not a HIP error
    for over in ACCEPTED.get(name, []):
        rc, text = call(lib, name, over)
        assert rc == 0 and text.startswith("cvx_device_arch"), (name, over, rc, text)  # and no text recorded


def test_workspace_bytes(lib):
    fn = lib.cvx_trace_workspace_bytes
    assert fn(9, 9, 70) == 8 * WORDS and fn(1, 1, 64) == 8 and fn(1, 1, 65) == 16 and fn(0, 4, 4) == 0 and fn(128, 512, 512) == 128 * 512 * 64
    assert fn(-1, 4, 4) == fn(4, 32769, 4) == fn(2048, 1024, 1024) == -1


def test_header_and_signatures_agree():
    from cryovit_amd import _lib

    header = (ROOT / "include" / "cryovit_hip.h").read_text()
    declared = dict(re.findall(r"^(?:int|long) (cvx_trace_\w+)\(([^;]*)\);", header, flags=re.M | re.S))
    assert sorted(declared) == sorted(n for n in _lib.SIGNATURES if n.startswith("cvx_trace_")) == sorted(ENTRIES)
    kinds = {"int": C.c_int, "long": C.c_long, "hipStream_t": C.c_void_p}
    for name, params in declared.items():
        want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in (" ".join(q.split()) for q in params.split(","))]
        res, args = _lib.SIGNATURES[name]
        assert args == want, name
        assert res is (C.c_long if re.search(rf"^long {name}\(", header, flags=re.M) else C.c_int)
        assert len(ENTRIES[name]) + (0 if name.endswith("_bytes") else 1) == len(args)
    for macro, value in (("CVX_TRACE_VOXEL_COLS", _lib.TRACE_VOXEL_COLS), ("CVX_TRACE_BRANCH_COLS", _lib.TRACE_BRANCH_COLS),
                         ("CVX_TRACE_STATE_BYTES", _lib.TRACE_STATE_BYTES)):
        assert re.search(rf"^#define {macro} {value}$", header, flags=re.M), macro
    assert (_lib.TRACE_VOXEL_COLS, _lib.TRACE_BRANCH_COLS) == (len(fo.VOXEL_COLS), len(fo.BRANCH_COLS)) == (12, 16)
    # the definitions stand in the header literally
    for words in ("z, y, x, id, degree, branch, rank, f, e,", "id, kind (0 end-end, 1 end-junction, 2 junction-junction, 3 ring), path_voxels,",
                  "head_index, last_index (-1 for a link), chord2", "26-adjacent and carry the same id", "in raster order of their key voxels"):
        assert words in header, words


def test_the_ops_wrappers_check_their_operands_without_a_device():
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((8, 8, 16), dtype=torch.int32)
    with pytest.raises(_lib.CvxError, match="trace_skeleton: skeleton must be int32 \\[D, H, W\\]"):
        ops.trace_skeleton(t.to(torch.uint8), 1)
    with pytest.raises(_lib.CvxError, match="trace_skeleton: d2 must be int32 \\[D, H, W\\]"):
        ops.trace_skeleton(t, 1, d2=t.to(torch.int64))
    with pytest.raises(_lib.CvxError, match="trace_skeleton: d2 \\(8, 8, 8\\) differs in shape"):
        ops.trace_skeleton(t, 1, d2=t[:, :, :8].contiguous())
    with pytest.raises(_lib.CvxError, match="need device"):
        ops.trace_skeleton(t, 1)  # there is no CPU path
    with pytest.raises(_lib.CvxError, match="need device"):
        ops.trace_emit(t, 1)
    vox, nbrs = torch.zeros((5, 12), dtype=torch.int32), torch.zeros((5, 2), dtype=torch.int32)
    with pytest.raises(_lib.CvxError, match="trace_rank: nbrs must be int32 \\[5, 2\\]"):
        ops.trace_rank(vox, nbrs[:4], 3)
    with pytest.raises(_lib.CvxError, match="trace_rank: rounds must lie in \\[0, 32\\]"):
        ops.trace_rank(vox, nbrs, 33)
    with pytest.raises(_lib.CvxError, match="need device"):
        ops.trace_rank(vox, nbrs, 3)
    with pytest.raises(_lib.CvxError, match="trace_rings: state must be int32 \\[5, 10\\]"):
        ops.trace_rings(vox, torch.zeros((9, 5), dtype=torch.int32))
    with pytest.raises(_lib.CvxError, match="trace_finalise: a cut needs the states"):
        ops.trace_finalise(vox, nbrs, None, torch.zeros(5, dtype=torch.int32), (8, 8, 16))
    assert [ops.trace_rounds(n) for n in (0, 1, 2, 3, 4, 5, 8, 9, 64, 65, 128, 129, 68000)] == [1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 7, 8, 17]
