"""Wall time of the label side of one `cryovit evaluate` step: a 128x512x512 int16 .mrc label map with 3 named values (plus
background and -1), decoded for one name and scored with DiceMetric + F1Metric, on the host path (utils.load_labels ->
collated labels -> the two metric classes) and on the GPU path (raw read -> cvx_label_census -> cvx_label_metrics).

    python tools/bench_eval_labels.py [--reps 3]

Prints one JSON line; times are medians over the repetitions, in ms, from host call to host result."""

from __future__ import annotations

import argparse
import json
import struct
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _write_mrc(path: Path, vol: np.ndarray) -> None:
    hdr = bytearray(1024)
    nz, ny, nx = vol.shape
    hdr[0:16] = struct.pack("<4i", nx, ny, nz, 1)
    hdr[208:216] = b"MAP " + bytes([0x44, 0x44, 0, 0])
    path.write_bytes(bytes(hdr) + vol.astype("<i2").tobytes())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from cryovit_amd.models.metrics import DiceMetric, F1Metric
    from cryovit_amd.run.eval_model import label_plan, score_labels
    from cryovit_amd.utils import load_labels, read_label_volume

    dev = torch.device("cuda:0")
    keys, key = ["a", "mito", "c"], "mito"
    rng = np.random.default_rng(0)
    # piecewise-constant map: 8x8x8 blocks of {-1, 0, 1, 2, 3}
    lab = np.kron(rng.choice(np.array([-1, 0, 1, 2, 3], np.int16), size=(16, 64, 64)), np.ones((8, 8, 8), np.int16)).astype(np.int16)
    probs = torch.from_numpy(rng.random(lab.shape, dtype=np.float32)).to(dev)
    metric_fns = {"dice_metric": DiceMetric(threshold=0.5), "f1_metric": F1Metric()}
    res = {"host_decode_ms": [], "host_metrics_ms": [], "gpu_decode_ms": [], "gpu_metrics_ms": []}
    with tempfile.TemporaryDirectory() as td:
        path = Path(td) / "labels.mrc"
        _write_mrc(path, lab)
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            y = load_labels(path, keys, key=key)[key]
            labels = torch.from_numpy(y.astype(np.float32))  # collate_fn: labels are fp32
            t1 = time.perf_counter()
            yd = labels.to(dev)
            host = {n: float(m(probs, yd)) for n, m in metric_fns.items()}
            for m in metric_fns.values():
                m.reset()
            t2 = time.perf_counter()
            raw = read_label_volume(path, key=key)
            labels_dev = torch.from_numpy(np.ascontiguousarray(raw)).to(dev)
            mode, value = label_plan(labels_dev, path, keys, key)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            gpu, _ = score_labels(probs, labels_dev, mode, value, metric_fns)
            t4 = time.perf_counter()
            for k, v in zip(res, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                res[k].append(1e3 * v)
    out = {k: round(float(np.median(v[1:])), 2) for k, v in res.items()}  # the first repetition warms up
    out.update(shape=list(lab.shape), host=host, gpu=gpu)  # (the host path sums 33 M voxels with fp32 atomics)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
