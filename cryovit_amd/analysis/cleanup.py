"""Cleaning a predicted mask on the device before it is labelled: close, fill, open.

Network masks come with pinholes, enclosed cavities and one-voxel gaps, and the measurements are sensitive to them: a cavity
raises the Euler number by one, turns a centreline into a shell and adds an inner surface to the mesh; a crack cuts an instance
in two.  ``CleanupOptions`` names the three repairs, ``clean_mask`` applies them in the fixed order close, fill, open: closing
seals pinholes so that cavities become fillable, opening runs last and removes spurs and specks.  ``label_file`` and
``run_inference(instances=True)`` call it before ``label_and_split``; with no option given nothing is launched.
"""

from __future__ import annotations

from dataclasses import dataclass

from cryovit_amd.analysis._tables import host_table

FILL_MODES = ("3d", "slices")
ADDED_COLUMN = "added_voxels"


@dataclass(frozen=True)
class CleanupOptions:
    """What is repaired in the thresholded mask of one label before its instances are labelled, in this order.  With any of them
    the file gains ``<label>_cleaned`` (uint8, the mask that was labelled; ``<label>_preds`` stays as predicted) and the CSV the
    column ``added_voxels`` right after ``INSTANCE_COLUMNS``: the voxels of the instance that the mask as predicted did not have.

    ``close_radius``  morphological closing by the discrete ball {v : |v|^2 <= floor(R^2)} (the floor(R^2) convention of
                      ``split_radius``), as in unbounded space with background outside the volume, cropped back to the volume
                      (``engine.ops.mask_close``).  floor(R^2) == 0 is the identity.
    ``fill_holes``    ``"3d"``: fill every background voxel that is not connected to the six faces of the volume through
                      background, under the connectivity dual to the instances' (background 6 for connectivity 26, background 26
                      for 6).  ``"slices"``: every z-slice on its own as a 2-D image, the border its four edges, background 4 for
                      connectivity 26 and 8 for 6 (Fiji's per-slice "Fill Holes": for tomograms, where the missing wedge leaves
                      structures open along z).  No size limit on what is filled (``engine.ops.mask_fill_holes``).
    ``open_radius``   morphological opening by the same kind of ball; the erosion wears the foreground down from the volume's
                      border as from any background (``engine.ops.mask_open``).  floor(R^2) == 0 is the identity."""

    close_radius: float | None = None
    fill_holes: str | None = None
    open_radius: float | None = None

    @property
    def any(self) -> bool:
        """Is any of the three given (a radius of 0 is given)?"""
        return self.close_radius is not None or self.fill_holes is not None or self.open_radius is not None

    def validate(self) -> "CleanupOptions":
        """Raises ``ValueError`` for the first value out of range; returns the record."""
        if self.close_radius is not None and not self.close_radius >= 0:
            raise ValueError(f"close_radius must be >= 0, got {self.close_radius}")
        if self.fill_holes is not None and self.fill_holes not in FILL_MODES:
            raise ValueError(f"fill_holes must be '3d' or 'slices', got {self.fill_holes!r}")
        if self.open_radius is not None and not self.open_radius >= 0:
            raise ValueError(f"open_radius must be >= 0, got {self.open_radius}")
        return self


def clean_mask(mask, cleanup: CleanupOptions, connectivity: int = 26):
    """(cleaned, totals) of a uint8 device mask (nonzero = foreground): ``cleaned`` (uint8, 0 / 1) after the steps ``cleanup`` asks
    for, in the order close, fill, open, and ``totals``, an int64 device tensor [3]: the voxels added by closing, the voxels filled,
    the voxels removed by opening (0 for a step that is not asked for).  ``connectivity`` is the instances': the fill floods the
    background under its dual.  Without any option ``mask`` itself comes back, ``totals`` is None and nothing is launched."""
    if not cleanup.any:
        return mask, None
    import torch

    from cryovit_amd.engine import ops

    def count(m):
        return torch.count_nonzero(m)

    totals = torch.zeros(3, dtype=torch.int64, device=mask.device)
    cleaned, voxels = mask, count(mask)
    steps = ((cleanup.close_radius, lambda m: ops.mask_close(m, cleanup.close_radius)),
             (cleanup.fill_holes, lambda m: ops.mask_fill_holes(m, connectivity=connectivity, slices=cleanup.fill_holes == "slices")),
             (cleanup.open_radius, lambda m: ops.mask_open(m, cleanup.open_radius)))
    for i, (wanted, step) in enumerate(steps):
        if wanted is None:
            continue
        cleaned = step(cleaned)  # the step before is freed here
        after = count(cleaned)
        totals[i] = voxels - after if i == 2 else after - voxels
        voxels = after
    return cleaned, totals


def log_totals(what: str, totals) -> None:
    """One line with the three totals of ``clean_mask`` (a host read of three numbers)."""
    import logging

    closed, filled, opened = host_table(totals, 0).tolist()
    logging.info("%s: cleaning added %d voxels by closing, filled %d, removed %d by opening", what, closed, filled, opened)


def added_voxels(labels, before, k: int):
    """int64 [k] on the device: per instance 1..k of ``labels`` the voxels that ``before``, the mask as predicted, did not have."""
    from cryovit_amd.engine import ops

    return ops.instance_added_voxels(labels, before, k)


def added_rows(added, extra: list[dict]) -> list[dict]:
    """``extra`` with the key ``added_voxels`` in front: the CSV column right after the standard ones, before ``component``."""
    return [{ADDED_COLUMN: a, **e} for a, e in zip(host_table(added, 0).tolist(), extra)]
