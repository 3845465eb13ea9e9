"""GPU suite for the nearest-instance map and the pair table (``csrc/nearest.hip`` through ``ops.nearest_instance`` and
``ops.instance_pair_contacts``) and ``label_file(..., contacts_with=...)`` against tests/contact_oracle.py.  Everything is
compared with ``torch.equal`` / ``np.array_equal`` on every voxel and every table entry: the feature has no tolerance.

The shapes are those of tests/test_gpu_edt.py (rows unaligned; 64-voxel site bitmaps and 64-wide slabs in x, 8 outputs per
thread and up to 16 waves per line, more than 64 bitmaps per row) plus the edge of this file's own slab rule: lines of at most
256 keys are staged in LDS (2x256x3 in y, 256x3x5 in z are the longest staged lines), longer ones take the two in-place sweeps
in y (2x257x3, 2x512x3, 2x513x3, 3x700x37) and the single sweep from global memory in z (257x3x5, 300x5x40, 520x3x5)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import ccl_oracle as co
import contact_oracle as xo
import edt_oracle as eo

pytestmark = pytest.mark.gpu

SHAPES = {"A": (5, 33, 70), "B": (9, 64, 130), "Ylong": (3, 700, 37), "Zlong": (300, 5, 40), "Y512": (2, 512, 3),
          "Y513": (2, 513, 3), "Z520": (520, 3, 5), "Xwide": (1, 2, 4200), "Y256": (2, 256, 3), "Y257": (2, 257, 3),
          "Z256": (256, 3, 5), "Z257": (257, 3, 5)}
NONE = xo.NONE
TOP = 7  # ids of the salt volumes


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def salt_case(shape_name: str, density: float):
    """(labels with random ids 1..TOP on a fraction ``density`` of the voxels, oracle d2, oracle nearest): computed once."""
    rng = np.random.default_rng(0)
    shape = SHAPES[shape_name]
    labels = np.where(rng.random(shape) < density, rng.integers(1, TOP + 1, size=shape), 0).astype(np.int32)
    return frozen(labels, *xo.nearest(labels, TOP))


@functools.lru_cache(maxsize=None)
def blob_case(shape_name: str, seed: int):
    """(flood-fill labels of a mask of random boxes, k, oracle d2, oracle nearest)."""
    labels, table = co.components(xo.blob_mask(SHAPES[shape_name], seed, 12), 26)
    return (*frozen(labels), len(table), *frozen(*xo.nearest(labels, len(table))))


@functools.lru_cache(maxsize=None)
def pair_case(shape_name: str):
    """(labels a, ka, labels b, kb, oracle d2 of b, oracle nearest of b) of two independent masks of 60 random boxes each: some
    twenty to forty instances a side, several of them with more than one partner."""
    a, ta = co.components(xo.blob_mask(SHAPES[shape_name], 1, 60), 26)
    b, tb = co.components(xo.blob_mask(SHAPES[shape_name], 2, 60), 26)
    d2, who = frozen(*xo.nearest(b, len(tb)))
    return (*frozen(a), len(ta), *frozen(b), len(tb), d2, who)


def dev(gpu, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(gpu)  # a copy: the cached cases are read-only


def run(gpu, labels: np.ndarray, k: int):
    from cryovit_amd.engine import ops

    d2, who = ops.nearest_instance(dev(gpu, labels), k)
    for t in (d2, who):
        assert t.dtype == torch.int32 and t.shape == labels.shape and t.device == gpu and t.is_contiguous()
    return d2, who


def same(got: torch.Tensor, want: np.ndarray) -> bool:
    return torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want)))


@pytest.mark.parametrize("density", [0.001, 0.5])
@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_salt_ids(gpu, shape_name, density):
    from cryovit_amd.engine import ops

    labels, want_d2, want_who = salt_case(shape_name, density)
    d2, who = run(gpu, labels, TOP)
    assert same(d2, want_d2), int((d2.cpu().numpy() != want_d2).sum())
    assert same(who, want_who), int((who.cpu().numpy() != want_who).sum())
    assert torch.equal(d2, ops.edt_squared(dev(gpu, labels), sites="nonzero"))  # the distance half, bit for bit
    assert density < 0.1 or int((who.cpu().numpy()[labels > 0] == labels[labels > 0]).all())  # a site keeps its own id


@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_blobs(gpu, shape_name):
    from cryovit_amd.engine import ops

    labels, k, want_d2, want_who = blob_case(shape_name, 1)
    assert k >= 2
    d2, who = run(gpu, labels, k)
    assert same(d2, want_d2) and same(who, want_who)
    assert torch.equal(d2, ops.edt_squared(dev(gpu, labels), sites="nonzero"))


@pytest.mark.parametrize("shape_name", ["A", "Ylong", "Z257"])
def test_ids_past_k_are_not_sites(gpu, shape_name):
    labels = salt_case(shape_name, 0.5)[0]
    for k in (3, 1):
        want_d2, want_who = xo.nearest(np.where(labels <= k, labels, 0), k)
        d2, who = run(gpu, labels, k)
        assert same(d2, want_d2) and same(who, want_who) and int(who.max()) == k
    odd = labels.copy()
    odd[odd == 2] = -2  # negative values are nobody's either
    want_d2, want_who = xo.nearest(np.where(odd > 0, odd, 0), TOP)
    d2, who = run(gpu, odd, TOP)
    assert same(d2, want_d2) and same(who, want_who)
    d2, who = run(gpu, labels, 0)  # no site at all
    assert same(d2, np.full(labels.shape, NONE, np.int32)) and same(who, np.zeros(labels.shape, np.int32))


def test_two_runs_are_bit_equal(gpu):
    labels, k, want_d2, want_who = blob_case("B", 1)
    a, b = run(gpu, labels, k), run(gpu, labels, k)
    assert a[0].data_ptr() != b[0].data_ptr()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and same(a[0], want_d2) and same(a[1], want_who)


def test_empty_volume_and_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    d2, who = ops.nearest_instance(torch.zeros((0, 8, 8), dtype=torch.int32, device=gpu), 3)
    assert d2.shape == who.shape == (0, 8, 8) and d2.dtype == who.dtype == torch.int32
    zeros = np.zeros(SHAPES["A"], np.int32)
    d2, who = run(gpu, zeros, 5)
    assert same(d2, np.full(zeros.shape, NONE, np.int32)) and same(who, zeros)
    labels, want_d2, want_who = salt_case("A", 0.5)
    t = dev(gpu, labels)
    with pytest.raises(_lib.CvxError, match="non-contiguous"):
        ops.nearest_instance(t[:, :, ::2], TOP)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.nearest_instance(t.to(torch.uint8), TOP)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.nearest_instance(t[0], TOP)
    with pytest.raises(_lib.CvxError, match="k must"):
        ops.nearest_instance(t, -1)
    with pytest.raises(_lib.CvxError):
        ops.nearest_instance(torch.zeros(4, 4, 4, dtype=torch.int32), 1)  # a host tensor
    d2, who = ops.nearest_instance(t, TOP)
    with pytest.raises(_lib.CvxError, match="int32 \\[D, H, W\\]"):
        ops.instance_pair_contacts(t, TOP, who.long(), d2, 1)
    with pytest.raises(_lib.CvxError, match="shape"):
        ops.instance_pair_contacts(t, TOP, who, d2[:, :, :8].contiguous(), 1)
    with pytest.raises(_lib.CvxError, match="ka must"):
        ops.instance_pair_contacts(t, -1, who, d2, 1)
    with pytest.raises(_lib.CvxError, match="threshold_d2 must"):
        ops.instance_pair_contacts(t, TOP, who, d2, -1)
    with pytest.raises(_lib.CvxError, match="capacity must"):
        ops.instance_pair_contacts(t, TOP, who, d2, 1, capacity=0)
    assert same(d2, want_d2) and same(who, want_who)
    assert ops.instance_pair_contacts(t, 0, who, d2, 1).shape == (0, 5)  # nobody to pair
    empty = torch.zeros((0, 8, 8), dtype=torch.int32, device=gpu)
    assert ops.instance_pair_contacts(empty, 3, empty, empty, 1).shape == (0, 5)


# ---- the pair table ----

def pairs(gpu, a: np.ndarray, ka: int, who: np.ndarray, d2: np.ndarray, thr: int, **kw) -> torch.Tensor:
    from cryovit_amd.engine import ops

    out = ops.instance_pair_contacts(dev(gpu, a), ka, dev(gpu, who), dev(gpu, d2), thr, **kw)
    assert out.dtype == torch.int64 and out.dim() == 2 and out.shape[1] == 5 and out.device == gpu
    return out


@pytest.mark.parametrize("thr", [0, 1, 2, 9])
@pytest.mark.parametrize("shape_name", ["B", "Ylong"])
def test_pair_table_against_oracle(gpu, shape_name, thr):
    from cryovit_amd.engine import ops

    a, ka, _, _, d2, who = pair_case(shape_name)
    want = xo.pair_table(a, ka, who, d2, thr)
    assert len(want) >= 20 and (thr > 0 or not want[:, 3].any()) and max(np.bincount(want[:, 0])) >= 2
    got = pairs(gpu, a, ka, who, d2, thr)
    assert same(got, want)
    assert same(pairs(gpu, a, ka, who, d2, thr, capacity=1), want)  # a table that has to grow gives the same rows
    assert same(pairs(gpu, a, ka, who, d2, thr, capacity=len(want)), want)  # and one that ends up (nearly) full
    assert torch.equal(pairs(gpu, a, ka, who, d2, thr), got)
    # the existing reduction over the union of the other label: the pairs of an instance add up to its row there
    stats = ops.instance_distance_stats(dev(gpu, a), dev(gpu, d2), ka, thr).cpu().numpy()
    rows = got.cpu().numpy()
    for i in range(1, ka + 1):
        mine = rows[rows[:, 0] == i]
        assert mine[:, 2].sum() == stats[i - 1, 0]
        assert stats[i - 1, 0] == 0 or mine[:, 3].min() == stats[i - 1, 1]
    # ids past ka are nobody's
    assert same(pairs(gpu, a, ka // 2, who, d2, thr), want[want[:, 0] <= ka // 2])


def test_overlapping_volumes_have_gap_zero(gpu):
    a, ka, b, _, d2, who = pair_case("B")
    assert ((a > 0) & (b > 0)).any()
    got = pairs(gpu, a, ka, who, d2, 2).cpu().numpy()
    want = xo.pair_table(a, ka, who, d2, 2)
    assert np.array_equal(got, want)
    over = {(int(x), int(y)) for x, y in zip(a[(a > 0) & (b > 0)], b[(a > 0) & (b > 0)])}
    zero = {(int(r[0]), int(r[1])) for r in got if r[3] == 0}
    assert over == zero and all(b.ravel()[r[4]] == r[1] and a.ravel()[r[4]] == r[0] for r in got if r[3] == 0)


def test_many_pairs_outgrow_the_default_table(gpu):
    """Every voxel an instance of its own against salt ids: more pairs than the default table has slots, most slots contested."""
    from cryovit_amd.engine import ops

    b, d2, who = salt_case("A", 0.5)
    a = np.arange(1, b.size + 1, dtype=np.int32).reshape(b.shape)
    want = xo.pair_table(a, a.size, who, d2, 9)
    assert len(want) == a.size > ops.PAIR_CAPACITY
    got = pairs(gpu, a, a.size, who, d2, 9)
    assert same(got, want) and same(pairs(gpu, a, a.size, who, d2, 9, capacity=3), want)
    # few ids on both sides: long runs, every thread after the same few slots
    a7 = salt_case("A", 0.001)[2]  # the nearest map of a sparse volume: large regions of one id
    want = xo.pair_table(a7, TOP, who, d2, 9)
    assert same(pairs(gpu, a7, TOP, who, d2, 9), want) and same(pairs(gpu, a7, TOP, who, d2, 9, capacity=1), want)


# ---- label_file ----

def csv_lines(header: list[str], rows: list[dict]) -> list[str]:
    """The CSV the writers must produce for these rows (floats with ``repr``)."""
    return [",".join(header)] + [",".join(repr(v) if isinstance(v, float) else str(v) for v in r.values()) for r in rows]


def test_label_file_with_contacts(gpu, tmp_path):
    from cryovit_amd import io
    from cryovit_amd.analysis import INSTANCE_COLUMNS, PAIR_COLUMNS, instance_rows, label_file

    shape = SHAPES["B"]
    mito, er = xo.blob_mask(shape, 1, 60), xo.blob_mask(shape, 2, 60)
    labels, table = co.components(mito, 26, 4)
    k, base = len(table), instance_rows(table)
    # the ids of the ER's own CSV: labelled with a min_size, so they differ from a fresh labelling of er_preds
    er_own, er_own_table = co.components(er, 26, 40)
    er_fresh, er_fresh_table = co.components(er, 26)
    assert 2 <= len(er_own_table) < len(er_fresh_table) and k >= 3
    (tmp_path / "mito").mkdir()
    (tmp_path / "er").mkdir()
    with io.FileWriter(tmp_path / "mito" / "tomo0.hdf") as f:
        f.create_dataset("mito_preds", mito, compression="gzip")
    with io.FileWriter(tmp_path / "er" / "tomo0.hdf") as f:
        f.create_dataset("er_preds", er, compression="gzip")
        f.create_dataset("er_instances", er_own.astype(np.uint16), compression="gzip")
    (tmp_path / "preds").mkdir()
    with io.FileWriter(tmp_path / "preds" / "tomo0.hdf") as f:
        f.create_dataset("er_preds", er, compression="gzip")

    def check(result_dir, other, other_k, radius):
        want = xo.pair_rows(labels, k, other, other_k, radius)
        assert len(want) >= 20 and any(r["gap_d2"] == 0 for r in want) and any(r["gap_d2"] > 0 for r in want)
        assert (result_dir / "contacts" / "tomo0_mito_er.csv").read_text().splitlines() == csv_lines(PAIR_COLUMNS, want)
        rows = [{**b, "partners_er": n} for b, n in zip(base, xo.partner_counts(want, k))]
        assert max(r["partners_er"] for r in rows) >= 3 and min(r["partners_er"] for r in rows) == 0
        assert (result_dir / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(INSTANCE_COLUMNS + ["partners_er"], rows)
        assert np.array_equal(io.read_dataset(result_dir / "tomo0.hdf", "mito_instances"), labels)

    # er_instances of the other folder's file: that label's own ids
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "own", contacts_with="er",
               distance_to_dir=tmp_path / "er", contact_radius=1.5)
    check(tmp_path / "own", er_own, len(er_own_table), 1.5)
    # only er_preds: a fresh labelling under the call's connectivity, nothing dropped
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "fresh", contacts_with="er",
               distance_to_dir=tmp_path / "preds")
    check(tmp_path / "fresh", er_fresh, len(er_fresh_table), 1.0)
    # together with --distance-to: the partners come after its columns
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "both", contacts_with="er", distance_to="er",
               distance_to_dir=tmp_path / "er", contact_radius=1.5)
    header = (tmp_path / "both" / "instances" / "tomo0_mito.csv").read_text().splitlines()[0].split(",")
    assert header == INSTANCE_COLUMNS + ["gap_d2_er", "gap_er", "contact_voxels_er", "partners_er"]
    # without the option: no contacts folder, no partners column
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "plain", distance_to="er",
               distance_to_dir=tmp_path / "er")
    assert not (tmp_path / "plain" / "contacts").exists()
    assert "partners_" not in (tmp_path / "plain" / "instances" / "tomo0_mito.csv").read_text()
    label_file(tmp_path / "mito" / "tomo0.hdf", "mito", min_size=4, result_dir=tmp_path / "bare")
    assert not (tmp_path / "bare" / "contacts").exists()
    assert (tmp_path / "bare" / "instances" / "tomo0_mito.csv").read_text().splitlines() == csv_lines(INSTANCE_COLUMNS, base)
