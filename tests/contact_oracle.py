"""Plain restatement of the pairwise-contact feature (``csrc/nearest.hip`` through ``ops.nearest_instance`` /
``ops.instance_pair_contacts`` and ``analysis.distances``): the checker for the CPU tests (against a brute force over all
sites) and the GPU tests (against the kernels).  The nearest-instance map is one ``edt_oracle.edt_sq`` per id, the pair table a
loop over the voxels."""

from __future__ import annotations

import math

import numpy as np

import edt_oracle as eo

NONE = eo.NONE


def nearest(labels: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """(d2, nearest), int32, shape of ``labels``: the squared distance to the nearest voxel with a value in 1..k and the smallest
    id among the values at that distance; NONE and 0 without such a voxel."""
    labels = np.asarray(labels)
    if k == 0 or labels.size == 0:
        return np.full(labels.shape, NONE, np.int32), np.zeros(labels.shape, np.int32)
    per_id = np.stack([eo.edt_sq(labels == i, "nonzero") for i in range(1, k + 1)])
    d2 = per_id.min(axis=0)
    ids = (np.argmin(per_id, axis=0) + 1).astype(np.int32)  # argmin: the first, i.e. the smallest, id among equals
    ids[d2 == NONE] = 0
    return d2.astype(np.int32), ids


def brute_force(labels: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """The definition itself, O(voxels x sites): for tiny volumes."""
    labels = np.asarray(labels)
    pts = np.argwhere((labels >= 1) & (labels <= k))
    ids = labels[tuple(pts.T)].astype(np.int64) if len(pts) else np.zeros(0, np.int64)
    d2 = np.full(labels.shape, NONE, np.int64)
    who = np.zeros(labels.shape, np.int64)
    for v in np.ndindex(labels.shape):
        if len(pts):
            d = ((pts - np.asarray(v)) ** 2).sum(axis=1)
            d2[v] = d.min()
            who[v] = ids[d == d.min()].min()
    return d2.astype(np.int32), who.astype(np.int32)


def pair_table(labels_a: np.ndarray, ka: int, nearest_b: np.ndarray, d2_b: np.ndarray, thr: int) -> np.ndarray:
    """int64 [P, 5], rows a, b, contact_voxels, gap_d2, at in (a, b) order, over the voxels with a = labels_a in 1..ka, b =
    nearest_b != 0 and d2_b <= thr: their number, the smallest d2_b and the smallest linear index attaining it."""
    pairs: dict[tuple[int, int], list[int]] = {}
    flat = zip(labels_a.ravel().tolist(), nearest_b.ravel().tolist(), d2_b.ravel().tolist())
    for v, (a, b, d) in enumerate(flat):
        if not (1 <= a <= ka and b != 0 and d <= thr):
            continue
        row = pairs.setdefault((a, b), [0, d, v])
        row[0] += 1
        if d < row[1]:  # voxels come in ascending index: an equal d keeps the earlier one
            row[1], row[2] = d, v
    return np.array([[a, b, *pairs[a, b]] for a, b in sorted(pairs)], dtype=np.int64).reshape(-1, 5)


def pair_rows(labels: np.ndarray, k: int, other_labels: np.ndarray, other_k: int, radius: float) -> list[dict]:
    """The rows of the contacts CSV: what ``analysis.distances.instance_pair_contacts`` must return."""
    _, H, W = labels.shape
    d2, who = nearest(other_labels, other_k)
    rows = []
    for a, b, n, d, at in pair_table(labels, k, who, d2, int(math.floor(radius * radius))).tolist():
        rows.append({"id": a, "other_id": b, "contact_voxels": n, "gap_d2": d, "gap": math.sqrt(d), "at_z": at // (H * W),
                     "at_y": at // W % H, "at_x": at % W})
    return rows


def partner_counts(rows: list[dict], k: int) -> list[int]:
    """Per id 1..k the number of distinct other ids among ``rows``."""
    return [len({r["other_id"] for r in rows if r["id"] == i}) for i in range(1, k + 1)]


def blob_mask(shape, seed: int, count: int) -> np.ndarray:
    """uint8 mask of ``count`` random boxes: a few instances of several voxels each, some of them touching."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = [int(rng.integers(0, n)) for n in shape]
        r = [int(rng.integers(1, 4)), int(rng.integers(2, 7)), int(rng.integers(2, 9))]
        m[max(0, c[0] - r[0]): c[0] + r[0], max(0, c[1] - r[1]): c[1] + r[1], max(0, c[2] - r[2]): c[2] + r[2]] = 1
    return m
