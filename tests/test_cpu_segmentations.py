"""CPU suite of the multi-label segmentation overlays: the numpy oracle (tests/seg_oracle.py) on hand-computed pixels, the
animated-PNG writer decoded by Pillow, file discovery / grouping / key fallback of
``cryovit_amd.visualization.segmentations`` with the renderer stubbed by the oracle, and the ``visualize_results`` entry point."""

import io as _io
import logging
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import seg_oracle as so

A, B = (1.0, 0.5, 0.25), (0.0, 0.5, 1.0)  # colours whose products below are exact


def _vol(values, dtype=np.float32):
    return np.array(values, dtype=dtype).reshape(1, 1, -1)


def test_oracle_hand_pixels_threshold_half():
    #            mixed  below  overlap  low    high
    data = _vol([0.5, 0.25, 0.0, -0.5, 1.5])
    seg_a = _vol([1.0, 0.25, 1.0, 0.0, 0.0])
    seg_b = _vol([0.0, 0.0, 1.0, 0.0, 0.0])
    out = so.overlay_frames(data, [seg_a, seg_b], [A, B], 0.5)
    assert out.shape == (1, 1, 10, 3) and out.dtype == np.uint8
    left, right = out[0, 0, :5], out[0, 0, 5:]
    # left half: clip(data) * 255 truncated, on all three channels
    assert left.tolist() == [[127] * 3, [63] * 3, [0] * 3, [0] * 3, [255] * 3]
    # px0: sum (1, .5, .25): red 1 > .5 -> 255; green .5 is not > .5 and blue is below -> grey 127 (channels on both sides)
    assert right[0].tolist() == [255, 127, 127]
    # px1: sum (.25, .125, .0625), all below -> the grey 63
    assert right[1].tolist() == [63, 63, 63]
    # px2: two labels, sum (1, 1, 1.25) clips to (1, 1, 1) -> white over data 0
    assert right[2].tolist() == [255, 255, 255]
    # px3 / px4: no label; data outside [0, 1] clips to 0 / 1
    assert right[3].tolist() == [0, 0, 0] and right[4].tolist() == [255, 255, 255]


def test_oracle_hand_pixels_threshold_point_three():
    t32 = np.float32(0.3)
    up = np.nextafter(t32, np.float32(1))
    data = _vol([0.5, 0.5, 0.5, 0.5])
    seg = _vol([t32, up, 0.75, 1.0])
    out = so.overlay_frames(data, [seg], [A], 0.3)
    right = out[0, 0, 4:]
    # a sum equal to float32(0.3) does not pass `>`: the Python-float threshold compares as float32 (as a double 0.3 it would)
    assert float(t32) > 0.3 and right[0].tolist() == [127, 127, 127]
    # one ulp above passes on the red channel: (uint8)(0.30000004 * 255) = 76; green (.15) and blue (.075) stay grey
    assert right[1].tolist() == [76, 127, 127]
    # .75 * (1, .5, .25) = (.75, .375, .1875): red 191, green .375 > .3 -> 95 (95.625), blue grey
    assert right[2].tolist() == [191, 95, 127]
    # 1 * (1, .5, .25): 255, 127 (127.5), .25 is below .3 -> grey 127
    assert right[3].tolist() == [255, 127, 127]
    # uint8 masks read as 0 / 1
    out8 = so.overlay_frames(data[:, :, :2], [_vol([0, 1], np.uint8)], [A], 0.3)
    assert out8[0, 0, 2:].tolist() == [[127, 127, 127], [255, 127, 127]]


def test_oracle_no_labels_is_grey_twice():
    data = np.linspace(-0.5, 1.5, 24, dtype=np.float32).reshape(2, 3, 4)
    out = so.overlay_frames(data, [], [], 0.5)
    assert np.array_equal(out[:, :, :4], out[:, :, 4:])
    assert np.array_equal(out[..., 0], np.concatenate([(np.clip(data, 0, 1) * 255).astype(np.uint8)] * 2, axis=2))


def test_palette_is_the_published_deep_colours():
    from cryovit_amd.visualization import segmentations as seg

    codes = {"mito": "#4C72B0", "cristae": "#DD8452", "microtubule": "#55A868", "granule": "#C44E52"}
    assert list(seg.PALETTE) == list(codes)
    for name, code in codes.items():
        want = tuple(int(code[i:i + 2], 16) / 255 for i in (1, 3, 5))
        assert seg.PALETTE[name] == want == so.PALETTE[name]
        assert all(type(v) is float for v in seg.PALETTE[name])


# ---- animated PNG ----

@pytest.mark.parametrize("shape", [(5, 7, 9), (1, 3, 5), (3, 1, 1), (4, 6, 10), (2, 33, 17)])
def test_encode_apng_decodes_with_pillow(shape):
    from cryovit_amd.io.png import encode_apng

    N, H, W = shape
    frames = np.random.default_rng(N * 100 + W).integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    im = Image.open(_io.BytesIO(encode_apng(frames)))
    assert im.format == "PNG" and im.size == (W, H)
    assert getattr(im, "n_frames", 1) == N
    assert abs(im.info["duration"] - 1000 / 30) < 1e-9
    assert im.info.get("loop") == 0
    for i in range(N):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert("RGB")), frames[i]), f"frame {i}"


def test_apng_chunk_layout_and_writer(tmp_path):
    import struct
    import zlib

    from cryovit_amd.io.png import encode_apng, encode_png, write_apng

    frames = np.arange(3 * 2 * 4 * 3, dtype=np.uint8).reshape(3, 2, 4, 3)
    blob = encode_apng(frames, fps=30, level=1)
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n, kind = struct.unpack(">I4s", blob[pos:pos + 8])
        body = blob[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert struct.unpack(">II", chunks[1][1]) == (3, 0)  # 3 frames, loop forever
    seqs = [struct.unpack(">I", body[:4])[0] for kind, body in chunks if kind in (b"fcTL", b"fdAT")]
    assert seqs == list(range(5))
    for kind, body in chunks:
        if kind == b"fcTL":
            assert struct.unpack(">IIIIIHHBB", body)[1:] == (4, 2, 0, 0, 1, 30, 0, 0)
    # frame 0 is what a plain PNG of the same image holds
    assert chunks[3][1] == zlib.compress(b"".join(b"\0" + frames[0, y].tobytes() for y in range(2)), 1)
    assert encode_png(frames[0], level=1).count(chunks[3][1]) == 1
    write_apng(tmp_path / "a.apng", frames, level=1)
    assert (tmp_path / "a.apng").read_bytes() == blob
    with pytest.raises(ValueError):
        encode_apng(frames[0])
    with pytest.raises(ValueError):
        encode_apng(frames.astype(np.float32))


# ---- discovery, grouping, key fallback ----

def _write_pred(path: Path, label: str, data, pred, nested=False):
    from cryovit_amd import io

    with io.FileWriter(path) as fh:
        fh.create_dataset("data", data)
        fh.create_dataset(f"predictions/{label}" if nested else f"{label}_preds", pred, compression="gzip")


@pytest.fixture
def stub_renderer(monkeypatch):
    from cryovit_amd.visualization import segmentations as seg

    calls = []

    def fake(data, volumes, colours, threshold=0.5, device=None):
        calls.append({"data": data, "volumes": volumes, "colours": colours, "threshold": threshold})
        return so.overlay_frames(data, volumes, colours, threshold)

    monkeypatch.setattr(seg, "render_frames", fake)
    return calls


def _tree(root: Path, shape=(2, 4, 6)):
    """exp_dir with mito / cristae / bacteria experiments of template single_hd_cryovit, one of another template, and a file."""
    rng = np.random.default_rng(3)
    vols = {}
    for exp, label, sample, stems in [("single_hd_cryovit_mito", "mito", "Q18", ["t1.hdf", "t2.hdf"]),
                                      ("single_hd_cryovit_cristae", "cristae", "Q18", ["t1.hdf"]),
                                      ("single_hd_cryovit_bacteria", "bacteria", "Q18", ["t1.hdf"]),
                                      ("single_hd_unet3d_mito", "mito", "Q18", ["t9.hdf"])]:
        for stem in stems:
            data = rng.uniform(-0.2, 1.2, shape).astype(np.float32)
            pred = rng.random(shape, dtype=np.float32)
            vols[(exp, stem)] = (data, pred)
            _write_pred(root / exp / sample / stem, label, data, pred)
    (root / "single_hd_cryovit_notes.txt").write_text("not a directory")
    return vols


def _decode(path: Path) -> np.ndarray:
    im = Image.open(path)
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


def test_discovery_all_palette_labels(tmp_path, stub_renderer, caplog):
    from cryovit_amd.visualization import process_experiment
    from cryovit_amd.visualization import segmentations as seg

    exp, res = tmp_path / "exp", tmp_path / "res"
    vols = _tree(exp)
    with caplog.at_level(logging.WARNING):
        process_experiment(exp, res, "single_hd_cryovit", None)
    # bacteria is outside the palette: with labels=None its directory is not even used, so there is nothing to warn about
    assert "bacteria" not in caplog.text
    out_dir = res / "single_hd_cryovit_cristae_mito_segmentations"  # labels in the order found (directories in name order)
    assert sorted(p.relative_to(out_dir).as_posix() for p in out_dir.rglob("*.apng")) == ["Q18/t1.apng", "Q18/t2.apng"]
    assert [d.name for d in res.iterdir()] == [out_dir.name]
    by_shape = {len(c["volumes"]): c for c in stub_renderer}
    assert sorted(by_shape) == [1, 2]
    # t1: cristae then mito, data from the first label's (cristae) file; t2: mito alone
    c_data, c_pred = vols[("single_hd_cryovit_cristae", "t1.hdf")]
    _, m_pred = vols[("single_hd_cryovit_mito", "t1.hdf")]
    assert by_shape[2]["colours"] == [seg.PALETTE["cristae"], seg.PALETTE["mito"]] and by_shape[2]["threshold"] == 0.5
    assert np.array_equal(by_shape[2]["data"], c_data)
    assert np.array_equal(by_shape[2]["volumes"][0], c_pred) and np.array_equal(by_shape[2]["volumes"][1], m_pred)
    assert np.array_equal(_decode(out_dir / "Q18" / "t1.apng"), so.overlay_frames(c_data, [c_pred, m_pred], by_shape[2]["colours"]))
    d2, p2 = vols[("single_hd_cryovit_mito", "t2.hdf")]
    assert np.array_equal(_decode(out_dir / "Q18" / "t2.apng"), so.overlay_frames(d2, [p2], [seg.PALETTE["mito"]]))
    assert abs(Image.open(out_dir / "Q18" / "t2.apng").info["duration"] - 1000 / 30) < 1e-9


def test_discovery_explicit_labels_and_unknown_colour(tmp_path, stub_renderer, caplog):
    from cryovit_amd.visualization import segmentations as seg

    exp, res = tmp_path / "exp", tmp_path / "res"
    _tree(exp)
    found, files = seg.discover(exp, "single_hd_cryovit", ["mito"])
    assert found == ["mito"] and sorted(files) == ["t1", "t2"] and all(list(v) == ["mito"] for v in files.values())
    assert files["t1"]["mito"] == (exp / "single_hd_cryovit_mito" / "Q18" / "t1.hdf").resolve()
    found, files = seg.discover(exp, "single_hd_unet3d", None)
    assert found == ["mito"] and list(files) == ["t9"]
    assert seg.discover(exp, "single_hd_sam2", None) == ([], {})
    # an explicit label without a colour: its directory is used, the label is warned about and not drawn; every label is
    # paired with its own directory whatever the order of the list
    with caplog.at_level(logging.WARNING):
        seg.process_experiment(exp, res, "single_hd_cryovit", ["mito", "bacteria"])
    assert "Couldn't find color for label bacteria" in caplog.text
    out_dir = res / "single_hd_cryovit_bacteria_mito_segmentations"
    assert sorted(p.name for p in out_dir.rglob("*.apng")) == ["t1.apng", "t2.apng"]
    assert all(c["colours"] == [seg.PALETTE["mito"]] and len(c["volumes"]) == 1 for c in stub_renderer)


def test_mismatched_shapes_raise(tmp_path, stub_renderer):
    from cryovit_amd.visualization import process_experiment

    exp = tmp_path / "exp"
    rng = np.random.default_rng(0)
    _write_pred(exp / "single_hd_cryovit_mito" / "S" / "t.hdf", "mito", rng.random((2, 4, 6), dtype=np.float32), rng.random((2, 4, 6), dtype=np.float32))
    _write_pred(exp / "single_hd_cryovit_cristae" / "S" / "t.hdf", "cristae", rng.random((2, 4, 5), dtype=np.float32),
                rng.random((2, 4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="does not match"):
        process_experiment(exp, tmp_path / "res", "single_hd_cryovit", None)
    assert stub_renderer == []


def test_prediction_key_fallback(tmp_path, stub_renderer, caplog):
    from cryovit_amd import io
    from cryovit_amd.visualization import segmentations as seg

    exp = tmp_path / "exp"
    rng = np.random.default_rng(1)
    data = rng.random((2, 3, 4), dtype=np.float32)
    nested, flat = rng.random((2, 3, 4), dtype=np.float32), rng.integers(0, 2, (2, 3, 4), dtype=np.uint8)
    f_nested = exp / "single_hd_cryovit_mito" / "S" / "t.hdf"
    f_flat = exp / "single_hd_cryovit_cristae" / "S" / "t.hdf"
    f_none = exp / "single_hd_cryovit_granule" / "S" / "t.hdf"
    _write_pred(f_nested, "mito", data, nested, nested=True)
    _write_pred(f_flat, "cristae", data, flat)
    with io.FileWriter(f_none) as fh:
        fh.create_dataset("data", data)
        fh.create_dataset("granule", flat)
    # a file that has both layouts: predictions/<label> wins
    f_both = tmp_path / "both.hdf"
    with io.FileWriter(f_both) as fh:
        fh.create_dataset("data", data)
        fh.create_dataset("predictions/mito", nested)
        fh.create_dataset("mito_preds", flat)
    assert seg.prediction_key(f_nested, "mito") == "predictions/mito"
    assert seg.prediction_key(f_flat, "cristae") == "cristae_preds"
    assert seg.prediction_key(f_none, "granule") is None
    assert seg.prediction_key(f_both, "mito") == "predictions/mito"
    assert seg.prediction_key(f_nested, "cristae") is None
    with caplog.at_level(logging.WARNING):
        seg.process_experiment(exp, tmp_path / "res", "single_hd_cryovit", None)
    assert "granule_preds" in caplog.text and "skipped" in caplog.text
    (call,) = stub_renderer
    assert call["colours"] == [seg.PALETTE["cristae"], seg.PALETTE["mito"]]
    # the uint8 mask reaches the renderer as uint8, the probabilities as fp32
    assert call["volumes"][0].dtype == np.uint8 and np.array_equal(call["volumes"][0], flat)
    assert call["volumes"][1].dtype == np.float32 and np.array_equal(call["volumes"][1], nested)
    out = tmp_path / "res" / "single_hd_cryovit_cristae_granule_mito_segmentations" / "S" / "t.apng"
    assert np.array_equal(_decode(out), so.overlay_frames(data, [flat, nested], call["colours"]))


# ---- entry point ----

def test_entry_point_reaches_process_experiment(tmp_path, monkeypatch):
    import cryovit_amd.visualization as vis
    from cryovit_amd.training import visualize_results as vr

    calls = []
    monkeypatch.setattr(vis, "process_experiment", lambda exp_dir, result_dir, exp_template, labels: calls.append((exp_dir, result_dir, exp_template, labels)))
    exp = tmp_path / "exp"
    exp.mkdir()
    vr.main(["--exp_dir", str(exp), "--result_dir", str(tmp_path / "res"), "--exp_type", "segmentations"])
    assert [c[2] for c in calls] == ["single_hd_cryovit", "single_hd_unet3d", "single_hd_sam2"]
    assert all(c[0] == exp and c[1] == tmp_path / "res" and c[3] is None for c in calls)
    calls.clear()
    vr.main(["--exp_dir", str(exp), "--result_dir", str(tmp_path / "res"), "--exp_type", "segmentations", "--exp_group", "HD", "--labels", "mito",
             "cristae"])
    assert len(calls) == 3 and all(c[3] == ["mito", "cristae"] for c in calls)
    with pytest.raises(AssertionError, match="Experiment group"):
        vr.main(["--exp_dir", str(exp), "--result_dir", str(tmp_path / "res"), "--exp_type", "segmentations", "--exp_group", "AD"])


@pytest.mark.parametrize("exp_type", ["dino_pca", "single", "multi", "multi_label", "multi_label_sample", "fractional", "sparse"])
def test_entry_point_unbuilt_types_exit_with_message(tmp_path, exp_type):
    from cryovit_amd.training import visualize_results as vr

    with pytest.raises(SystemExit) as e:
        vr.main(["--exp_dir", str(tmp_path), "--result_dir", str(tmp_path / "res"), "--exp_type", exp_type])
    msg = str(e.value)
    assert "not built" in msg and exp_type in msg and "segmentations" in msg
    for other in ("single", "multi_label_sample", "fractional", "sparse"):
        assert other in msg


def test_entry_point_asserts_on_missing_exp_dir(tmp_path):
    from cryovit_amd.training import visualize_results as vr

    for exp_type in ("segmentations", "single"):
        with pytest.raises(AssertionError, match="Experiment directory"):
            vr.main(["--exp_dir", str(tmp_path / "absent"), "--result_dir", str(tmp_path / "res"), "--exp_type", exp_type])
    with pytest.raises(SystemExit):  # argparse rejects a type the reference does not have
        vr.main(["--exp_dir", str(tmp_path), "--result_dir", str(tmp_path / "res"), "--exp_type", "umap"])
