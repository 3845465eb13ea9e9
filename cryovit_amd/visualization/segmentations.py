"""Multi-label segmentation overlays as animations (mirror of the reference's ``cryovit/visualization/segmentations.py``,
reached through ``python -m cryovit_amd.training.visualize_results --exp_type segmentations``): the prediction files that
several single-label experiments wrote for one tomogram become one animation, a frame per slice, the grey data next to
the data with every label laid over it in its colour.

  discovery   directories of ``exp_dir`` named ``<exp_template>..._<label>``, their ``**/*.hdf`` grouped by stem  (``discover``)
  read        ``data`` of the first label's file + one volume per label, uint8 masks kept as uint8          (``read_volumes``)
  frames      colour sum, clip, threshold, overlay, uint8 ``[D, H, 2W, 3]`` in one kernel                   (cvx_seg_overlay)
  file        ``<result_dir>/<exp_template>_<labels>_segmentations/<sample>/<stem>.apng``, 30 fps           (``io.png.write_apng``)

The next file is read and the previous animation is compressed on worker threads while the GPU renders the current one;
under ``torch.distributed.run`` the tomograms are shared out over the ranks.

Deliberate divergences from the reference:

* the container is an animated PNG, not an ``mp4v`` video (OpenCV is not a dependency); frames, order and rate are the same;
* the reference reads ``fh["predictions"][<label>]``, a layout no writer of either code base produces.  Here
  ``predictions/<label>`` is used when the file has it, else ``<label>_preds`` (what ``TestPredictionWriter`` and ``cryovit infer``
  write); a file with neither is skipped with a warning;
* the reference pairs a user-given ``labels`` list with the directories in ``iterdir`` order, which can pair a label with
  another label's directory.  Here every directory is paired with its own suffix (directories in name order) and the output
  folder lists the labels in the order they were found;
* the reference's colouring loop also meets its own ``data`` entry and warns that it has no colour; that warning is not kept.

The palette is seaborn's published "deep" colours 0-3 (seaborn is not a dependency: parity unpinned against the package).
"""

from __future__ import annotations

import logging
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from cryovit_amd import io
from cryovit_amd.io.png import write_apng
from cryovit_amd.run.sharding import shard_records, world_info

FPS = 30
THRESHOLD = 0.5


def _rgb(code: str) -> tuple[float, float, float]:
    return tuple(int(code[i:i + 2], 16) / 255 for i in (1, 3, 5))


# sns.color_palette("deep")[:4]
PALETTE = {"mito": _rgb("#4C72B0"), "cristae": _rgb("#DD8452"), "microtubule": _rgb("#55A868"), "granule": _rgb("#C44E52")}


def discover(exp_dir: Path, exp_template: str, labels: list[str] | None) -> tuple[list[str], dict[str, dict[str, Path]]]:
    """(labels found, ``{stem: {label: path}}``): the ``**/*.hdf`` files of every directory ``<exp_template>..._<label>`` of
    ``exp_dir`` whose label is wanted (in the palette when ``labels`` is None, else in ``labels``)."""
    wanted = PALETTE if labels is None else labels
    found: list[str] = []
    files: dict[str, dict[str, Path]] = {}
    for d in sorted(p for p in Path(exp_dir).iterdir() if p.is_dir() and p.name.startswith(exp_template)):
        label = d.name.split("_")[-1]
        if label not in wanted:
            continue
        tomo_files = sorted(d.glob("**/*.hdf"))
        logging.info("Found %d .hdf files for label %s in experiment directory %s", len(tomo_files), label, d.name)
        if label not in found:
            found.append(label)
        for f in tomo_files:
            files.setdefault(f.stem, {})[label] = f.resolve()
    return found, files


def prediction_key(path: Path, label: str) -> str | None:
    """The dataset holding ``label``'s prediction in ``path``: ``predictions/<label>``, else ``<label>_preds``, else None."""
    top = io.list_keys(path)
    if "predictions" in top:
        try:
            if label in io.list_keys(path, "predictions"):
                return f"predictions/{label}"
        except Exception:  # noqa: BLE001 - `predictions` is a dataset, not a group
            pass
    return f"{label}_preds" if f"{label}_preds" in top else None


def read_volumes(stem: str, label_dict: dict[str, Path]) -> tuple[str, np.ndarray, list[tuple[str, np.ndarray]]]:
    """(sample, data fp32 [D, H, W], [(label, volume)]) of one tomogram.  ``data`` comes from the first label's file; a uint8
    volume stays uint8 and any other dtype becomes fp32; labels without a colour or without a prediction are left out."""
    sample, data, volumes = "unknown", None, []
    for label, path in label_dict.items():
        sample = path.parent.name
        if data is None:
            data = np.ascontiguousarray(io.read_dataset(path, "data"), dtype=np.float32)
        if label not in PALETTE:
            logging.warning("Couldn't find color for label %s", label)
            continue
        key = prediction_key(path, label)
        if key is None:
            logging.warning("%s holds neither predictions/%s nor %s_preds: skipped", path, label, label)
            continue
        vol = io.read_dataset(path, key)
        vol = np.ascontiguousarray(vol if vol.dtype == np.uint8 else vol.astype(np.float32, copy=False))
        if vol.shape != data.shape:
            raise ValueError(f"{stem}: the {label} volume {vol.shape} of {path} does not match the data {data.shape}")
        volumes.append((label, vol))
    if data is None or data.ndim != 3:
        raise ValueError(f"{stem}: no [D, H, W] data volume")
    return sample, data, volumes


def render_frames(data: np.ndarray, volumes: list[np.ndarray], colours: list[tuple[float, float, float]],
                  threshold: float = THRESHOLD, device=None) -> np.ndarray:
    """uint8 ``[D, H, 2W, 3]`` frames (pinned host memory) of one tomogram: upload, one kernel call, download."""
    import torch

    from cryovit_amd.engine import ops

    dev = ops.norm_device(device or "cuda")
    with torch.cuda.device(dev):
        data_d = torch.from_numpy(data).to(dev)
        vols_d = [torch.from_numpy(v).to(dev) for v in volumes]
        D, H, W = data.shape
        frames = torch.empty(D, H, 2 * W, 3, dtype=torch.uint8, device=dev)
        ops.seg_overlay(data_d, vols_d, colours, frames, threshold=threshold)
        host = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(frames, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    return host.numpy()


def _write(path: Path, frames: np.ndarray) -> Path:
    path.parent.mkdir(parents=True, exist_ok=True)
    write_apng(path, frames, fps=FPS)
    logging.info("Saved animation to %s", path)
    return path


def process_files(file_dict: dict[str, dict[str, Path]], result_dir: Path, threshold: float = THRESHOLD, device=None) -> list[Path]:
    """Renders this rank's share of ``{stem: {label: path}}`` to ``result_dir/<sample>/<stem>.apng``."""
    result_dir.mkdir(parents=True, exist_ok=True)
    stems = list(file_dict)
    rank, _, world = world_info()
    mine = [stems[i] for i in shard_records(stems, rank, world)]
    if not mine:
        return []
    if device is None and world > 1:
        from cryovit_amd.run.sharding import select_device

        device = select_device()
    futures = []
    with ThreadPoolExecutor(max_workers=1) as reader, ThreadPoolExecutor(max_workers=2) as writer:
        nxt = reader.submit(read_volumes, mine[0], file_dict[mine[0]])
        for k, stem in enumerate(mine):
            logging.info("Processing file %s", stem)
            sample, data, volumes = nxt.result()
            if k + 1 < len(mine):
                nxt = reader.submit(read_volumes, mine[k + 1], file_dict[mine[k + 1]])
            frames = render_frames(data, [v for _, v in volumes], [PALETTE[lab] for lab, _ in volumes], threshold, device)
            futures.append(writer.submit(_write, result_dir / sample / (stem + ".apng"), frames))
            del frames
            for fut in futures[:-2]:  # at most two animations being compressed: a frame stack is 6 B per voxel
                fut.result()
        return [fut.result() for fut in futures]


def process_experiment(exp_dir: Path, result_dir: Path, exp_template: str, labels: list[str] | None) -> None:
    """Process segmentation results from multiple labels and save the combined visualisations as animations.

    exp_dir: directory of experiment results; result_dir: where to save; exp_template: prefix of the experiment directories to
    use, their label being the text after the last underscore; labels: the labels to draw, None for every palette label found."""
    exp_dir, result_dir = Path(exp_dir), Path(result_dir)
    result_dir.mkdir(parents=True, exist_ok=True)
    found, files = discover(exp_dir, exp_template, labels)
    process_files(files, result_dir / f"{exp_template}_{'_'.join(found)}_segmentations")
