"""csrc/trace.hip on the device against tests/filament_oracle.py: both tables of ``ops.trace_skeleton``, for equality.

The volumes are chosen against the 64-voxel word and the 4x8x64 tile the rows are counted in, and against the round count
ceil(log2 Np) of the pointer doubling: lines with 1 .. 128 path voxels at row 0 of volumes of one and of several rows, along every
axis and diagonal, a serpentine longer than a row, rings whose first voxel lies in another tile than most of them, every shape of
tests/test_cpu_filaments.py, salt noise, and skeletons of solids as ``ops.skeletonize_instances`` leaves them.  Every volume is
small enough for the oracle to walk it in a fraction of a second, so each case computes its own tables."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import filament_cases as fc
import filament_oracle as fo

pytestmark = pytest.mark.gpu

V = {name: i for i, name in enumerate(fo.VOXEL_COLS)}
B = {name: i for i, name in enumerate(fo.BRANCH_COLS)}


def run(gpu, volume: np.ndarray, k: int, d2=None, counters=None):
    from cryovit_amd.engine import ops

    dist = None if d2 is None else torch.from_numpy(np.array(d2, np.int32)).to(gpu)
    voxels, branches = ops.trace_skeleton(torch.from_numpy(np.array(volume, np.int32)).to(gpu), k, d2=dist, counters=counters)
    assert voxels.dtype == torch.int32 and voxels.dim() == 2 and voxels.shape[1] == 12 and voxels.device.type == "cuda"
    assert branches.dtype == torch.int64 and branches.dim() == 2 and branches.shape[1] == 16 and branches.device.type == "cuda"
    return voxels.cpu().numpy(), branches.cpu().numpy()


def check(gpu, volume: np.ndarray, k: int, d2=None, counters=None):
    """The device's tables, after they have been found equal to the oracle's."""
    want_v, want_b = fo.trace(volume, k, d2)
    got_v, got_b = run(gpu, volume, k, d2, counters)
    print(f"{volume.shape}: N {len(got_v)} (oracle {len(want_v)}), B {len(got_b)} (oracle {len(want_b)})")
    if got_v.shape == want_v.shape:
        print("voxel rows that differ:", np.flatnonzero((got_v != want_v).any(1))[:8], "columns:", np.flatnonzero((got_v != want_v).any(0)))
    if got_b.shape == want_b.shape:
        print("branch rows that differ:", np.flatnonzero((got_b != want_b).any(1))[:8], "columns:", np.flatnonzero((got_b != want_b).any(0)))
    assert np.array_equal(got_v, want_v) and got_v.dtype == want_v.dtype
    assert np.array_equal(got_b, want_b) and got_b.dtype == want_b.dtype
    return got_v, got_b


def distances(shape) -> np.ndarray:
    """A made-up distance map with every value distinct along a row, EDT_NONE here and there."""
    d2 = (np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape) * 7919 % 1009 + 1).astype(np.int32)
    d2[..., ::13] = fo.EDT_NONE
    return d2


# ---- nothing, and next to nothing ----

def test_empty_volumes_no_ids_and_single_voxels(gpu):
    for shape in ((0, 4, 4), (3, 0, 5), (2, 3, 0)):
        v, b = run(gpu, np.zeros(shape, np.int32), 3)
        assert v.shape == (0, 12) and b.shape == (0, 16)
    seen = {}
    check(gpu, np.zeros((5, 9, 70), np.int32), 2, counters=seen)
    assert seen == {"N": 0, "Np": 0, "B": 0, "rounds": 0, "rings": False, "passes": 0}
    line = fc.line((5, 9, 70), (1, 1, 1), (0, 0, 1), 9)
    v, b = check(gpu, line, 0)  # k == 0
    assert v.shape == (0, 12) and b.shape == (0, 16)
    check(gpu, line * 5, 4)  # all ids above k
    one = fc.line((5, 9, 70), (4, 8, 69), (0, 0, 1), 1)
    v, b = check(gpu, one, 1, counters=seen)
    assert v.tolist() == [[4, 8, 69, 1, 0, 0, 0, 0, 0, 0, 0, 0]] and b.shape == (0, 16) and seen["passes"] == 0
    for step in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 1, -1)):
        v, b = check(gpu, fc.line((5, 9, 70), (1, 1, 63), step, 2), 1, counters=seen)  # two voxels: a link, Np == 0 with N > 0
        assert b.shape == (1, 16) and b[0, B["path_voxels"]] == 0 and b[0, B["head_index"]] == -1 and seen["passes"] == 0 and seen["N"] == 2


# ---- lines: the round count at and around its steps, the word and tile edges ----

PATH_VOXELS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 128)


@pytest.mark.parametrize("shape", [(1, 1, 130), (2, 3, 130), (5, 9, 130)])
def test_lines_along_x_at_row_0(gpu, shape):
    from cryovit_amd.engine import ops

    for n in PATH_VOXELS:
        seen = {}
        v, b = check(gpu, fc.line(shape, (0, 0, 0), (0, 0, 1), n + 2), 1, distances(shape), counters=seen)
        assert (seen["N"], seen["Np"], seen["B"], seen["rounds"], seen["rings"], seen["passes"]) == (n + 2, n, 1, ops.trace_rounds(n), False, 1)
        assert b[0, B["path_voxels"]] == n and b[0, B["f"]] == n + 1 and v[1:-1, V["rank"]].tolist() == list(range(1, n + 1))
    assert [ops.trace_rounds(n) for n in PATH_VOXELS] == [1, 1, 2, 2, 3, 3, 3, 4, 6, 6, 7, 7]


@pytest.mark.parametrize("step, shape", [((0, 1, 0), (5, 17, 70)), ((1, 0, 0), (9, 9, 70)), ((0, 1, 1), (5, 17, 70)), ((1, 0, 1), (9, 9, 70)),
                                         ((1, 1, 0), (9, 17, 70)), ((1, 1, 1), (9, 17, 70)), ((1, -1, 1), (9, 17, 70)), ((0, 1, -1), (5, 17, 70)),
                                         ((1, 1, -1), (9, 17, 130))])
def test_lines_across_the_row_and_slice_edges(gpu, step, shape):
    """Along y over the 8-row tile edge, along z over the 4-slice edge, and the face, edge and corner diagonals; each at two places,
    one of them ending in the volume's last voxel of that direction."""
    longest = min(s for s, d in zip(shape, step) if d)
    for n in sorted({3, 5, 9, longest}):
        for base in (0, 1):
            if n + base > longest:
                continue
            start = tuple((base if d >= 0 else s - 1 - base) if d else min(3, s - 1) for s, d in zip(shape, step))
            if step[2] and start[2] in (0, shape[2] - 1):
                start = (start[0], start[1], 60 if step[2] > 0 else 67)  # across x = 63 | 64
            if start[2] + step[2] * (n - 1) not in range(shape[2]):
                continue
            check(gpu, fc.line(shape, start, step, n), 1, distances(shape))


def test_the_serpentine_is_one_chain_through_every_tile(gpu):
    v = fc.serpentine((9, 17, 130))
    seen = {}
    got_v, got_b = check(gpu, v, 1, distances(v.shape), counters=seen)
    assert got_b.shape[0] == 1 and got_b[0, B["path_voxels"]] == len(got_v) - 2 > 25 * 128 and seen["passes"] == 1 and seen["rounds"] == 12
    tiles = {(r[0] // 4, r[1] // 8, r[2] // 64) for r in got_v.tolist()}
    assert len(tiles) == 3 * 3 * 3


# ---- rings ----

def ring_scenes():
    """name -> (volume, k, rings, no-ring branches)"""
    out = {}
    # m in another tile than most of the ring: the first voxel sits in the tile above (y 7 | 8) the rest, the ring across x = 63 | 64
    out["diamond"] = (fc.volume((5, 17, 130), fc.diamond(3, (4, 10, 65))), 1, 1, 0)
    out["diamond_zx"] = (fc.volume((9, 9, 130), fc.diamond(3, (5, 4, 64), "zx")), 1, 1, 0)
    out["square"] = (fc.volume((5, 17, 130), fc.cut_corner_square((1, 7, 61))), 1, 1, 0)
    out["interlocked"] = (fc.interlocked_rings(), 2, 2, 0)
    both = fc.volume((5, 17, 130), fc.cut_corner_square((1, 7, 61)))
    both += fc.line((5, 17, 130), (3, 2, 3), (0, 0, 1), 120, 1) + fc.line((5, 17, 130), (4, 16, 129), (0, -1, -1), 9, 2)
    out["ring_and_chains"] = (both, 2, 1, 2)
    many = np.zeros((9, 17, 130), np.int32)
    for i, x in enumerate(range(2, 120, 9)):
        for p in fc.diamond(1 + i % 3, (2 + i % 5, 8, x + 3)):
            many[p] = 1 + i % 2
    out["many"] = (many, 2, len(range(2, 120, 9)), 0)
    return out


@pytest.mark.parametrize("name", ["diamond", "diamond_zx", "square", "interlocked", "ring_and_chains", "many"])
def test_rings(gpu, name):
    volume, k, rings, others = ring_scenes()[name]
    seen = {}
    v, b = check(gpu, volume, k, distances(volume.shape), counters=seen)
    assert int((b[:, B["kind"]] == 3).sum()) == rings and int((b[:, B["kind"]] != 3).sum()) == others
    assert seen["rings"] is True and seen["passes"] == 2
    ring_voxels = v[v[:, V["ring"]] == 1]
    assert len(ring_voxels) == int(b[b[:, B["kind"]] == 3][:, B["path_voxels"]].sum())
    if name in ("diamond", "square"):
        first = ring_voxels[ring_voxels[:, V["rank"]] == 1][0]
        rest = ring_voxels[ring_voxels[:, V["rank"]] != 1]
        tile = lambda r: (r[0] // 4, r[1] // 8, r[2] // 64)
        assert sum(tile(r) != tile(first) for r in rest.tolist()) > len(rest) / 2


def test_without_a_ring_the_second_pass_is_not_launched(gpu, monkeypatch):
    from cryovit_amd.engine import ops

    ranks = []
    rank = ops.trace_rank
    monkeypatch.setattr(ops, "trace_rank", lambda voxels, nbrs, rounds, cut=None: ranks.append((rounds, cut is not None)) or rank(voxels, nbrs, rounds, cut))
    seen = {}
    chains = fc.volume((5, 9, 70), fc.tee(4)) + fc.line((5, 9, 70), (3, 0, 2), (0, 0, 1), 66, 2)
    check(gpu, chains, 2, counters=seen)
    assert ranks == [(7, False)] and seen["passes"] == 1 and seen["rings"] is False and seen["Np"] == 6 + 64
    del ranks[:]
    check(gpu, chains + fc.volume((5, 9, 70), fc.diamond(2, (4, 6, 30)), 2), 2, counters=seen)
    assert ranks == [(7, False), (7, True)] and seen["passes"] == 2 and seen["rings"] is True and seen["Np"] == 6 + 64 + 8


# ---- junctions, links, ids ----

def shape_scenes():
    out = {
        "square_outline": fc.volume((5, 9, 70), fc.square_outline(6, (1, 2, 60))),  # across x = 63 | 64
        "tee": fc.volume((5, 9, 70), [(z, y, x + 55) for z, y, x in fc.tee(4)]),
        "stem_of_2": fc.volume((5, 9, 70), [(z + 2, y + 5, x + 58) for z, y, x in fc.tee(2)]),
        "bump": fc.volume((5, 9, 70), [(3, 7, 59 + x) for x in range(9)] + [(4, 8, 63)]),
        "lollipop": fc.volume((5, 9, 70), [(z, y, x + 56) for z, y, x in fc.lollipop()]),
        "theta": fc.volume((5, 9, 70), [(z + 3, y, x + 59) for z, y, x in fc.theta()]),
        "parallel_ids": fc.line((2, 3, 130), (0, 0, 0), (0, 0, 1), 130, 1) + fc.line((2, 3, 130), (0, 1, 0), (0, 0, 1), 130, 2)
                        + fc.line((2, 3, 130), (1, 2, 1), (0, 0, 1), 128, 1),
    }
    return out


@pytest.mark.parametrize("name", ["square_outline", "tee", "stem_of_2", "bump", "lollipop", "theta", "parallel_ids"])
def test_shapes(gpu, name):
    volume = shape_scenes()[name]
    v, b = check(gpu, volume, 2, distances(volume.shape))
    paths = sorted(b[:, B["path_voxels"]].tolist())
    if name == "square_outline":
        assert paths == [1] * 4 + [2] * 4 and (v[:, V["degree"]] == 3).sum() == 8
    if name == "tee":
        assert paths == [2, 2, 2] and b[:, B["kind"]].tolist() == [1, 1, 1]
    if name == "stem_of_2":
        assert paths == [0, 2, 2] and b[b[:, B["path_voxels"]] == 0][0, B["end_degree"]] == 4
    if name == "lollipop":
        loop = b[b[:, B["path_voxels"]] == 11][0]
        assert paths == [4, 11] and loop[B["start_index"]] == loop[B["end_index"]] and loop[B["chord2"]] == 0
    if name == "theta":
        assert len(paths) == 3 and set(b[:, B["kind"]].tolist()) == {2} and not v[:, V["ring"]].any()
    if name == "parallel_ids":
        assert b[:, B["id"]].tolist() == [1, 2, 1] and paths == [126, 128, 128]  # one voxel apart, different ids: no neighbours


# ---- salt noise ----

@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("density", [0.05, 0.2, 0.5])
@pytest.mark.parametrize("shape", [(5, 9, 70), (9, 17, 130)])
def test_salt_noise_of_three_ids(gpu, shape, density, seed):
    volume = fc.salt(shape, density, 3, seed)
    check(gpu, volume, 3, distances(shape))
    check(gpu, volume, 2)  # the third id is nobody's, and no distance map


# ---- composition with the thinning ----

def capsule() -> np.ndarray:
    z, y, x = np.mgrid[:9, :17, :100]
    t = np.clip(x, 48, 82)
    return ((z - 4.2) ** 2 + (y - 8.3) ** 2 + (x - t) ** 2 <= 3.0 ** 2).astype(np.int32)


def torus() -> np.ndarray:
    """Tube radius 2: at ``end_radius`` 2 it thins to a clean ring."""
    z, y, x = np.mgrid[:7, :24, :80]
    return ((np.sqrt((y - 11.5) ** 2 + (x - 62.5) ** 2) - 8) ** 2 + (z - 3.0) ** 2 <= 2.0 ** 2).astype(np.int32)


def tee_of_tubes() -> np.ndarray:
    z, y, x = np.mgrid[:9, :30, :100]
    bar = (z - 4.0) ** 2 + (y - 6.0) ** 2 + (x - np.clip(x, 40, 90)) ** 2 <= 3.0 ** 2
    stem = (z - 4.0) ** 2 + (x - 65.0) ** 2 + (y - np.clip(y, 6, 25)) ** 2 <= 3.0 ** 2
    return (bar | stem).astype(np.int32)


def dumbbell() -> np.ndarray:
    """Two balls of radius 5 whose centres are 9 apart: one instance that splits into two at its neck."""
    z, y, x = np.mgrid[:13, :14, :90]
    return (((z - 6) ** 2 + (y - 7) ** 2 + (x - 59.5) ** 2 <= 25) | ((z - 6) ** 2 + (y - 7) ** 2 + (x - 68.5) ** 2 <= 25)).astype(np.int32)


@pytest.mark.parametrize("name", ["capsule", "torus", "tee_of_tubes", "dumbbell"])
def test_composition_with_the_thinning(gpu, name):
    from cryovit_amd.analysis.filaments import junction_nodes
    from cryovit_amd.engine import ops

    labels = torch.from_numpy({"capsule": capsule, "torus": torus, "tee_of_tubes": tee_of_tubes, "dumbbell": dumbbell}[name]()).to(gpu)
    k = 1
    if name == "dumbbell":
        labels, table, _ = ops.split_instances(labels, 1, radius=3.0)
        k = int(table.shape[0])
        assert k == 2, "the drawing must split into its two balls"
    d2 = ops.edt_squared(labels, sites="zero")
    skeleton, stats = ops.skeletonize_instances(labels, k, d2=d2, end_radius=2.0)
    stats = stats.cpu().numpy()
    v, b = check(gpu, skeleton.cpu().numpy(), k, d2.cpu().numpy())
    euler = ops.instance_shape_stats(skeleton, k, connectivity=26)[:, 10].cpu().numpy()
    nodes, _ = junction_nodes(v)
    assert len(v) == int(stats[:, 0].sum())
    for ident in range(1, k + 1):
        mine = v[v[:, V["id"]] == ident]
        assert int((mine[:, V["degree"]] == 1).sum()) == stats[ident - 1, 1]
        assert int((mine[:, V["degree"]] >= 3).sum()) == stats[ident - 1, 2] and int((mine[:, V["degree"]] == 0).sum()) == stats[ident - 1, 3]
        assert int(mine[:, V["d2"]].sum()) == stats[ident - 1, 7]
        open_branches = int(((b[:, B["id"]] == ident) & (b[:, B["kind"]] != 3)).sum())
        assert sum(n["id"] == ident for n in nodes) - open_branches == euler[ident - 1], (name, ident)
    if name == "capsule":
        assert b.shape[0] == 1 and b[0, B["kind"]] == 0 and b[0, B["path_voxels"]] > 25
    if name == "torus":
        assert b.shape[0] == 1 and b[0, B["kind"]] == 3 and v[:, V["ring"]].all()
    if name == "tee_of_tubes":
        assert int((b[:, B["path_voxels"]] > 8).sum()) == 3 and len([n for n in nodes if n["kind"] == "junction"]) >= 1


def test_two_runs_are_bit_equal(gpu):
    volume = fc.salt((9, 17, 130), 0.2, 3, 7) + fc.volume((9, 17, 130), [])
    for p in fc.cut_corner_square((8, 2, 60)):
        volume[p] = 3
    d2 = distances(volume.shape)
    a, b = run(gpu, volume, 3, d2), run(gpu, volume, 3, d2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[1]) > 50


def test_operand_checks(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    t = torch.zeros((4, 8, 70), dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.trace_skeleton(t[:, :, ::2], 1)
    with pytest.raises(_lib.CvxError, match="k must be >= 0"):
        ops.trace_skeleton(t, -1)
    with pytest.raises(_lib.CvxError, match="differs in shape"):
        ops.trace_skeleton(t, 1, d2=t[:2].contiguous())
    with pytest.raises(_lib.CvxError, match="different devices|need device"):
        ops.trace_skeleton(t, 1, d2=t.cpu())


# ---- the pipeline ----

def test_label_file_with_trace(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import FILAMENT_COLUMNS, INSTANCE_COLUMNS, SKELETON_COLUMNS, label_file
    from cryovit_amd.analysis.filaments import (TraceOptions, branch_records, filament_rows, filament_volume, read_points_csv, read_star,
                                                sample_points, write_branches_csv)

    mask = (tee_of_tubes() != 0).astype(np.uint8)
    mask[1:8, 0:24, 0:30] |= (torus()[:, :, 50:80] != 0).astype(np.uint8)  # a second instance: the torus
    with io.FileWriter(tmp_path / "tomo0.hdf") as f:
        f.create_dataset("data", np.zeros(mask.shape, np.float32), compression="gzip")
        f.create_dataset("tube_preds", mask, compression="gzip")
    options = dict(trace=True, trace_spacing=4.0, trace_window=3.0, trace_scale=2.0, trace_angpix=5.0)
    out = label_file(tmp_path / "tomo0.hdf", "tube", result_dir=tmp_path / "out", **options)
    found = io.read_all_flat(out)
    assert sorted(found) == ["data", "tube_filaments", "tube_instances", "tube_preds", "tube_skeleton"]
    k = int(found["tube_instances"].max())
    assert k == 2
    skeleton = found["tube_skeleton"]
    # the distance map of the run, from the device as well: the oracle is the tracing's, not the transform's
    from cryovit_amd.engine import ops

    d2 = ops.edt_squared(torch.from_numpy(found["tube_instances"].astype(np.int32)).to(gpu), sites="zero").cpu().numpy()
    want_v, want_b = fo.trace(skeleton, k, d2)
    assert np.array_equal(found["tube_filaments"], filament_volume(want_v, skeleton.shape)) and found["tube_filaments"].dtype == np.int32
    lines = (tmp_path / "out" / "instances" / "tomo0_tube.csv").read_text().splitlines()
    assert lines[0].split(",") == INSTANCE_COLUMNS + SKELETON_COLUMNS + FILAMENT_COLUMNS
    rows = filament_rows(want_v, want_b, k)
    assert [line.split(",")[-7:] for line in lines[1:]] == [[repr(v) if isinstance(v, float) else str(v) for v in r.values()] for r in rows]
    assert sorted(r["filament_rings"] for r in rows) == [0, 1]
    base = tmp_path / "out" / "filaments"
    want = write_branches_csv(tmp_path / "want.csv", branch_records(want_v, want_b))
    assert (base / "tomo0_tube_branches.csv").read_bytes() == want.read_bytes()
    points = sample_points(want_v, want_b, TraceOptions(**options))
    got = read_points_csv(base / "tomo0_tube.csv")
    assert len(got) == len(points) > 20 and all(g["branch"] == w["branch"] and abs(g["pz"] - w["pz"]) <= 5e-7 for g, w in zip(got, points))
    names, star = read_star(base / "tomo0_tube.star")
    assert names[-2:] == ["_rlnHelicalTubeID", "_rlnHelicalTrackLengthAngst"] and len(star) == len(points) and {r[0] for r in star} == {"tomo0"}
    # without the option nothing of it is written and the rest is the same bytes
    bare = label_file(tmp_path / "tomo0.hdf", "tube", result_dir=tmp_path / "bare", skeleton=True)
    plain = io.read_all_flat(bare)
    assert sorted(plain) == ["data", "tube_instances", "tube_preds", "tube_skeleton"] and not (tmp_path / "bare" / "filaments").exists()
    assert all(np.array_equal(plain[n], found[n]) for n in plain)
