"""CPU suite for the instance-measurement pipeline that ``label_file`` and ``run_inference`` share (``analysis.instances``): the
sequence of ``engine.ops`` calls it issues, with recording stand-ins for the device ops, and the options record."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import ccl_oracle as co

from cryovit_amd import io


@pytest.fixture
def recorded(monkeypatch):
    """Every ``engine.ops`` entry point of the pipeline replaced by a stand-in that returns host tensors of the right shape and
    dtype and appends (name, the scalar arguments) to the returned list; ``recorded.d2`` collects the ``d2`` each of the skeleton
    and thickness stand-ins was handed."""
    from cryovit_amd.engine import ops
    from cryovit_amd.run import sharding

    class Calls(list):
        d2 = None

    calls = Calls()
    calls.d2 = {}

    def zeros(*shape, dtype=torch.int64):
        return torch.zeros(shape, dtype=dtype)

    def label_components(mask, *, connectivity=26, min_size=0):
        calls.append(("label_components", connectivity, min_size))
        lab, tab = co.components(mask.numpy(), connectivity, min_size)
        return torch.from_numpy(lab), torch.from_numpy(tab)

    def split_instances(labels, k, *, radius, min_core=0, connectivity=26):
        calls.append(("split_instances", k, radius, min_core, connectivity))
        return labels.clone(), torch.from_numpy(co.table(labels.numpy())), torch.arange(1, k + 1)

    def edt_squared(src, *, sites="zero"):
        calls.append(("edt_squared", str(src.dtype).removeprefix("torch."), sites))
        return zeros(*src.shape, dtype=torch.int32)

    def instance_distance_stats(labels, d2, k, threshold_d2):
        calls.append(("instance_distance_stats", k, threshold_d2))
        return zeros(k, 4)

    def nearest_instance(labels, k):
        calls.append(("nearest_instance", k))
        return zeros(*labels.shape, dtype=torch.int32), zeros(*labels.shape, dtype=torch.int32)

    def instance_pair_contacts(labels_a, ka, nearest_b, d2_b, threshold_d2, capacity=None):
        calls.append(("instance_pair_contacts", ka, threshold_d2))
        return torch.tensor([[1, 1, 3, 0, 0]], dtype=torch.int64)

    def instance_shape_stats(labels, k, *, connectivity=26):
        calls.append(("instance_shape_stats", k, connectivity))
        return zeros(k, 24)

    def skeletonize_instances(labels, k, *, d2=None, end_radius=2.0):
        calls.append(("skeletonize_instances", k, end_radius))
        calls.d2["skeleton"] = d2
        return zeros(*labels.shape, dtype=torch.int32), zeros(k, 8)

    def instance_thickness(labels, k, *, d2=None):
        calls.append(("instance_thickness", k))
        calls.d2["thickness"] = d2
        return zeros(*labels.shape, dtype=torch.int32), zeros(k, 5)

    def mesh_surface(labels):
        calls.append(("mesh_surface",))
        return zeros(3, 3, dtype=torch.int32), torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.ones(1, dtype=torch.int32)

    def mesh_smooth(vertices, triangles, iterations):
        calls.append(("mesh_smooth", iterations))
        return vertices.clone()

    def mesh_stats(vertices, triangles, ids, k):
        calls.append(("mesh_stats", k))
        return zeros(k, 3)

    for stub in (label_components, split_instances, edt_squared, instance_distance_stats, nearest_instance, instance_pair_contacts,
                 instance_shape_stats, skeletonize_instances, instance_thickness, mesh_surface, mesh_smooth, mesh_stats):
        monkeypatch.setattr(ops, stub.__name__, stub)
    monkeypatch.setattr(sharding, "select_device", lambda device=None: torch.device("cpu"))
    return calls


def two_boxes() -> np.ndarray:
    m = np.zeros((4, 6, 8), np.uint8)
    m[1:3, 1:4, 1:3] = 1
    m[0:4, 2:6, 5:8] = 1
    return m


@pytest.fixture
def prediction(tmp_path):
    """A [4, 6, 8] prediction file with two instances of ``mito`` and the masks of two other labels."""
    m = two_boxes()
    with io.FileWriter(tmp_path / "t.hdf") as f:
        f.create_dataset("data", np.zeros(m.shape, np.float32), compression="gzip")
        f.create_dataset("mito_preds", m, compression="gzip")
        f.create_dataset("er_preds", np.ascontiguousarray(m[:, :, ::-1]), compression="gzip")
        f.create_dataset("golgi_preds", np.ascontiguousarray(m[:, ::-1]), compression="gzip")
    return tmp_path / "t.hdf"


EVERYTHING = dict(connectivity=6, min_size=2, morphology=True, contact_radius=1.5, split_radius=1.0, split_min_core=1, shape=True,
                  skeleton=True, skeleton_end_radius=3.0, thickness=True, mesh=True, mesh_smooth=2)

# what the two hand-written pipelines issued before they became one (taken from a run of these stand-ins against them)
MEASURE_HEAD = [("edt_squared", "int32", "zero"), ("instance_distance_stats", 2, 1)]
MEASURE_TAIL = [("instance_shape_stats", 2, 6),
                ("edt_squared", "int32", "zero"),
                ("skeletonize_instances", 2, 3.0),
                ("instance_thickness", 2),
                ("mesh_surface",), ("mesh_smooth", 2), ("mesh_stats", 2)]
LABEL_FILE_SEQUENCE = [("label_components", 6, 2),
                       ("split_instances", 2, 1.0, 1, 6),
                       *MEASURE_HEAD,
                       ("edt_squared", "uint8", "nonzero"), ("instance_distance_stats", 2, 2),
                       ("label_components", 6, 0),
                       ("nearest_instance", 2),
                       ("instance_pair_contacts", 2, 2),
                       *MEASURE_TAIL]


def test_label_file_issues_the_pinned_sequence(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import label_file

    out = label_file(prediction, "mito", result_dir=tmp_path / "out", distance_to="er", contacts_with="golgi", **EVERYTHING)
    assert list(recorded) == LABEL_FILE_SEQUENCE
    assert recorded.d2["skeleton"] is not None and recorded.d2["skeleton"] is recorded.d2["thickness"]  # one map for both
    assert sorted(io.list_keys(out)) == ["data", "er_preds", "golgi_preds", "mito_instances", "mito_preds", "mito_skeleton", "mito_thickness"]
    for rel in ("instances/t_mito.csv", "contacts/t_mito_golgi.csv", "meshes/t_mito.ply"):
        assert (tmp_path / "out" / rel).stat().st_size > 0, rel


@pytest.mark.parametrize("one", ["skeleton", "thickness"])
def test_one_of_skeleton_and_thickness_computes_its_own_map(prediction, recorded, tmp_path, one):
    from cryovit_amd.analysis import label_file

    label_file(prediction, "mito", result_dir=tmp_path / "out", **{one: True})
    assert list(recorded) == [("label_components", 26, 0), ("skeletonize_instances", 2, 2.0) if one == "skeleton" else ("instance_thickness", 2)]
    assert recorded.d2 == {one: None}


def test_no_option_only_labels(prediction, recorded, tmp_path):
    from cryovit_amd.analysis import label_file

    label_file(prediction, "mito", result_dir=tmp_path / "out")
    assert list(recorded) == [("label_components", 26, 0)]


def test_measure_as_infer_calls_it(recorded):
    """``run_inference`` hands ``measure`` no other mask and no partner: the ``label_file`` sequence without those steps, and the
    columns in the same order."""
    from cryovit_amd.analysis import MESH_COLUMNS, SHAPE_COLUMNS, SKELETON_COLUMNS, THICKNESS_COLUMNS
    from cryovit_amd.analysis.distances import MORPHOLOGY_COLUMNS
    from cryovit_amd.analysis.instances import InstanceOptions, label_and_split, measure

    opts = InstanceOptions(**EVERYTHING)
    labels, table, component = label_and_split(torch.from_numpy(two_boxes()), opts)
    assert list(recorded) == LABEL_FILE_SEQUENCE[:2] and component.tolist() == [1, 2]
    del recorded[:]
    found = measure(labels, int(table.shape[0]), component, opts)
    assert list(recorded) == MEASURE_HEAD + MEASURE_TAIL
    assert recorded.d2["skeleton"] is not None and recorded.d2["skeleton"] is recorded.d2["thickness"]
    assert [list(e) for e in found.extra] == 2 * [["component", *MORPHOLOGY_COLUMNS, *SHAPE_COLUMNS, *SKELETON_COLUMNS, *THICKNESS_COLUMNS,
                                                   *MESH_COLUMNS]]
    assert found.pairs is None and found.skeleton.dtype == found.t2.dtype == torch.int32 and len(found.mesh) == 3
    host = found.arrays(lambda a: a.numpy())
    assert isinstance(host.skeleton, np.ndarray) and isinstance(host.t2, np.ndarray) and all(isinstance(a, np.ndarray) for a in host.mesh)
    assert host.extra is found.extra

    del recorded[:]
    none = measure(labels, 2, None, InstanceOptions())
    assert list(recorded) == [] and none.extra == [{}, {}] and none.skeleton is None and none.t2 is None and none.mesh is None


# ---- the options record ----

BAD_VALUES = [({"connectivity": 18}, "connectivity must be 6 or 26, got 18"),
              ({"min_size": -1}, "min_size must be >= 0, got -1"),
              ({"split_radius": -1.0}, "split_radius must be >= 0, got -1.0"),
              ({"split_radius": float("nan")}, "split_radius must be >= 0, got nan"),
              ({"split_radius": 1.0, "split_min_core": -2}, "split_min_core must be >= 0, got -2"),
              ({"skeleton_end_radius": -0.5}, "skeleton_end_radius must be >= 0, got -0.5"),
              ({"skeleton_end_radius": float("nan")}, "skeleton_end_radius must be >= 0, got nan"),
              ({"mesh_smooth": -1}, "mesh_smooth must be >= 0, got -1"),
              ({"mesh_format": "obj"}, "mesh_format must be 'ply' or 'stl', got 'obj'")]


def test_options_defaults_are_those_of_both_entry_points():
    import dataclasses
    import inspect

    from cryovit_amd.analysis.instances import InstanceOptions, label_file
    from cryovit_amd.run.infer_model import run_inference

    opts = InstanceOptions()
    assert opts.validate() is opts
    assert dataclasses.asdict(opts) == dict(connectivity=26, min_size=0, morphology=False, split_radius=None, split_min_core=0, shape=False,
                                            skeleton=False, skeleton_end_radius=2.0, thickness=False, mesh=False, mesh_smooth=0,
                                            mesh_format="ply", contact_radius=1.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        opts.mesh = True
    for fn in (label_file, run_inference):
        params = inspect.signature(fn).parameters
        for f in dataclasses.fields(opts):
            if f.name in params:
                assert params[f.name].default == f.default and params[f.name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, f.name)
        assert set(InstanceOptions.MEASUREMENTS) < set(params)
    assert "contact_radius" in inspect.signature(label_file).parameters


@pytest.mark.parametrize("bad, message", BAD_VALUES + [({"contact_radius": -1.0}, "contact_radius must be >= 0, got -1.0"),
                                                       ({"contact_radius": float("nan")}, "contact_radius must be >= 0, got nan")])
def test_options_validate_refuses(bad, message):
    from cryovit_amd.analysis.instances import InstanceOptions

    with pytest.raises(ValueError) as err:
        InstanceOptions(**bad).validate()
    assert str(err.value) == message


@pytest.mark.parametrize("bad, message", BAD_VALUES)
def test_both_entry_points_refuse_with_the_same_words(prediction, recorded, tmp_path, bad, message):
    """The record's message, from ``label_file`` before anything is labelled and from ``run_inference`` before the model file is
    opened (there is none)."""
    from cryovit_amd.analysis import label_file
    from cryovit_amd.run.infer_model import run_inference

    with pytest.raises(ValueError) as from_file:
        label_file(prediction, "mito", result_dir=tmp_path / "out", **bad)
    with pytest.raises(ValueError) as from_infer:
        run_inference([prediction], tmp_path / "none.model", tmp_path / "out", instances=True, **bad)
    assert str(from_file.value) == str(from_infer.value) == message
    assert list(recorded) == [] and not (tmp_path / "out").exists()


def test_run_inference_needs_instances_for_every_measurement(tmp_path):
    from cryovit_amd.analysis.instances import InstanceOptions
    from cryovit_amd.run.infer_model import run_inference

    for name in InstanceOptions.MEASUREMENTS:
        with pytest.raises(ValueError, match=f"^{name}=True needs instances=True"):
            run_inference([tmp_path / "t.hdf"], tmp_path / "none.model", tmp_path / "out", **{name: True})
    with pytest.raises(ValueError, match="^split_radius needs instances=True"):
        run_inference([tmp_path / "t.hdf"], tmp_path / "none.model", tmp_path / "out", split_radius=1.0)
