"""Plain restatement of the connected-component kernels of ``csrc/components.hip`` (``ops.label_components``): the checker
for the CPU tests (against ``scipy.ndimage.label`` where scipy is installed) and the GPU tests (against the kernels).

A raster scan in C order; every foreground voxel met without a label starts the next component and a flood fill with an
explicit stack labels everything joined to it.  The scan meets a component first at its smallest linear index, so ids come
out 1..K in ascending order of that index.  Meant to be read, not to be fast: the test volumes hold at most ~75k voxels."""

from __future__ import annotations

import numpy as np


def offsets(connectivity: int) -> list[tuple[int, int, int]]:
    """The neighbour steps (dz, dy, dx): 6 = faces, 26 = faces, edges and corners."""
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity must be 6 or 26, got {connectivity}")
    steps = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    return [s for s in steps if connectivity == 26 or abs(s[0]) + abs(s[1]) + abs(s[2]) == 1]


def label(mask: np.ndarray, connectivity: int = 26) -> np.ndarray:
    """int32 [D, H, W]: 0 for background (mask == 0), 1..K for the components in raster order of their first voxel."""
    fg = np.asarray(mask) != 0
    D, H, W = fg.shape
    # one layer of background around the volume: no step leaves the array, and nothing wraps around a face
    pad = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = fg
    sy, sz = W + 2, (H + 2) * (W + 2)
    steps = [dz * sz + dy * sy + dx for dz, dy, dx in offsets(connectivity)]
    todo = pad.ravel().tolist()  # True: foreground that has no label yet
    out = [0] * len(todo)
    k = 0
    for seed in np.flatnonzero(pad).tolist():  # ascending padded index = ascending (z, y, x) = ascending linear index
        if not todo[seed]:
            continue
        k += 1
        todo[seed] = False
        out[seed] = k
        stack = [seed]
        while stack:
            v = stack.pop()
            for s in steps:
                u = v + s
                if todo[u]:
                    todo[u] = False
                    out[u] = k
                    stack.append(u)
    return np.asarray(out, dtype=np.int32).reshape(pad.shape)[1:-1, 1:-1, 1:-1].copy()


def table(labels: np.ndarray) -> np.ndarray:
    """int64 [K, 10]: voxels, sum_z, sum_y, sum_x, z0, z1, y0, y1, x0, x1 (inclusive) of the labels 1..K."""
    k = int(labels.max()) if labels.size else 0
    out = np.zeros((k, 10), dtype=np.int64)
    if k == 0:
        return out
    z, y, x = np.nonzero(labels)
    row = labels[z, y, x].astype(np.int64) - 1
    np.add.at(out[:, 0], row, 1)
    for c, coord in enumerate((z, y, x)):
        np.add.at(out[:, 1 + c], row, coord)
        out[:, 4 + 2 * c] = labels.shape[c]
        out[:, 5 + 2 * c] = -1
        np.minimum.at(out[:, 4 + 2 * c], row, coord)
        np.maximum.at(out[:, 5 + 2 * c], row, coord)
    return out


def drop_small(labels: np.ndarray, tab: np.ndarray, min_size: int) -> tuple[np.ndarray, np.ndarray]:
    """Components with fewer than ``min_size`` voxels become background; the others are renumbered 1..K' in the same order."""
    keep = tab[:, 0] >= min_size
    remap = np.zeros(len(tab) + 1, dtype=np.int32)
    remap[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return remap[labels], tab[keep]


def components(mask: np.ndarray, connectivity: int = 26, min_size: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """(labels int32 [D, H, W], table int64 [K, 10]): what ``ops.label_components`` must return, bit for bit."""
    lab = label(mask, connectivity)
    return drop_small(lab, table(lab), min_size)
