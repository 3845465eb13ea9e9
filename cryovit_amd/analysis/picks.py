"""Where to cut subtomograms out of a segmented membrane: evenly spaced positions on the surface of every instance, each with the
membrane normal as orientation prior, as a RELION STAR file and a CSV (ATP synthase on cristae, ribosomes on the ER, anything picked
"on a surface at a spacing").  The picks carry the instance ids of ``<label>_instances`` and sit on voxels of its surface.

``engine.ops.pick_surface`` (csrc/picks.hip) selects them on the device and returns the int32 pick table, one row z, y, x, id, Mz,
My, Mx, n per pick in raster order (the definition is in include/cryovit_hip.h); ``pick_rows`` counts the picks per instance for
the instance CSV, ``pick_records`` turns the table into one record per pick, ``write_picks_csv`` and ``write_star`` write them.
Only ``pick_records`` uses floating point, in float64 and row by row, and the writers print fixed ``%.6f`` formats, so equal
tables give equal bytes.

What the numbers mean:

* The picks.  The candidates are the surface voxels of the labelled mask that belong to an instance and lie at least
  ``pick_radius`` voxels inside the volume on every axis.  They are taken in a pseudo-random order fixed by ``pick_seed`` (the order
  of murmur3's finaliser of voxel index XOR seed), each unless a pick of the same instance lies closer than ``pick_spacing`` voxels
  (centre to centre).  So within an instance no two picks are closer than the spacing, every candidate has a pick of its instance
  closer than the spacing, and picks of different instances ignore each other (a random sequential packing of the surface).
  Another seed gives another set of the same kind; the same seed the same set, bit by bit.
* Ids play no part in what is surface.  After ``--split-radius`` the pieces share faces and the plane between them holds no pick.
* The normal.  M is the sum of the offsets of the ball of ``pick_radius`` voxels around the pick that fall inside the object; it
  points into the object, and the outward unit normal is n = -M / |M|.  On the host reference, at ``pick_radius`` 5, the normals of
  a ball of radius 14.3 are off the true ones by 0.8 degrees on average and 2.0 at most; those of an oblique plane by 0.54 and
  0.91.  A larger radius is quieter and blurs folds smaller than it; a membrane thinner than the radius still gives the right axis
  as long as one side holds more of it.
* Unoriented picks.  M = 0 where the ball sees as much of the object on either side: a sheet one voxel thin.  Such a pick has no
  normal (NaN in the CSV, ``picks_unoriented`` in the instance CSV, no ``pick_offset``) and is left out of the STAR file.
* ``inside`` is n / N, the share of the ball inside the object: about 1/2 on a thick, flat wall, less on a thin or convex one.
* Position.  q = (z, y, x) + ``pick_offset`` * n in voxels of the segmented volume (a negative offset moves into the object: the
  membrane's mid-plane for a wall of known thickness; a positive one to the head of a protruding complex).  Written is
  (q + 0.5) * ``pick_scale`` - 0.5: ``pick_scale`` = the bin factor of ``preprocess --bin`` gives voxel-centre coordinates of the
  unbinned tomogram.
* Angles.  rot = atan2(ny, nx), tilt = acos(nz), psi = 0, in degrees, so that RELION's Euler_angles2direction(rot, tilt) =
  (cos rot sin tilt, sin rot sin tilt, cos tilt) equals (nx, ny, nz): the particle's z axis is the membrane normal, the in-plane
  angle is free.  The normals of the CSV (``nz, ny, nx``) are the authoritative orientation; the Euler conventions of other
  packages (Dynamo, Warp/M, emClarity) are to be derived from them, not from the STAR angles.

Out of scope: spacings above 16 voxels, sampling of the smoothed mesh, particle formats other than RELION's.  Positions along
filaments are ``analysis.filaments``' (``--trace``).
"""

from __future__ import annotations

import csv
import math
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from cryovit_amd.analysis._tables import host_table

PICK_COLUMNS = ["picks", "picks_unoriented"]
PICK_CSV_COLUMNS = ["pick", "id", "z", "y", "x", "pz", "py", "px", "nz", "ny", "nx", "rot", "tilt", "psi", "mz", "my", "mx", "inside"]
STAR_COLUMNS = ["_rlnMicrographName", "_rlnCoordinateX", "_rlnCoordinateY", "_rlnCoordinateZ", "_rlnAngleRot", "_rlnAngleTilt", "_rlnAnglePsi"]
RADIUS_MIN, RADIUS_MAX = 2, 16  # _lib.PICK_RADIUS_MIN / MAX
SPACING_MIN, SPACING_MAX = 2, 16  # _lib.PICK_SPACING_MIN / MAX


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)


@dataclass(frozen=True)
class PickOptions:
    """Whether picks are placed on the membranes of one label's instances, and how.  With ``pick`` each file gains
    ``picks/<tomo stem>_<label>.csv`` and ``.star`` and the instance CSV ``PICK_COLUMNS`` after every other column.

    ``pick``          place them.
    ``pick_spacing``  the least distance between two picks of one instance, voxel centre to voxel centre: an integer in 2..16.
    ``pick_radius``   the radius of the ball the normal is read from, in voxels, an integer in 2..16.
    ``pick_offset``   picks are moved this far along their outward normal (voxels; negative: into the object).
    ``pick_scale``    written coordinates are (q + 0.5) * scale - 0.5: the bin factor of ``preprocess --bin`` (> 0).
    ``pick_seed``     the seed of the order the candidates are taken in, 0 .. 2^32 - 1."""

    pick: bool = False
    pick_spacing: int = 8
    pick_radius: int = 5
    pick_offset: float = 0.0
    pick_scale: float = 1.0
    pick_seed: int = 0

    def validate(self) -> "PickOptions":
        """Raises ``ValueError`` for a value out of range (whether or not ``pick`` is on); returns the record."""
        if not _is_int(self.pick_spacing) or not SPACING_MIN <= self.pick_spacing <= SPACING_MAX:
            raise ValueError(f"pick_spacing must be an integer in [{SPACING_MIN}, {SPACING_MAX}], got {self.pick_spacing!r}")
        if not _is_int(self.pick_radius) or not RADIUS_MIN <= self.pick_radius <= RADIUS_MAX:
            raise ValueError(f"pick_radius must be an integer in [{RADIUS_MIN}, {RADIUS_MAX}], got {self.pick_radius!r}")
        if not _is_number(self.pick_offset):
            raise ValueError(f"pick_offset must be a finite number of voxels, got {self.pick_offset!r}")
        if not _is_number(self.pick_scale) or not self.pick_scale > 0:
            raise ValueError(f"pick_scale must be a finite number > 0, got {self.pick_scale!r}")
        if not _is_int(self.pick_seed) or not 0 <= self.pick_seed < 2**32:
            raise ValueError(f"pick_seed must be an integer in [0, 2^32 - 1], got {self.pick_seed!r}")
        return self


def pick_table(labels, k: int, opts: PickOptions):
    """The int32 [P, 8] pick table of the instances 1..k of the int32 device volume ``labels`` under ``opts``; it stays on the device."""
    from cryovit_amd.engine import ops

    return ops.pick_surface(labels, k, spacing=opts.pick_spacing, radius=opts.pick_radius, seed=opts.pick_seed)


def pick_rows(table, k: int) -> list[dict]:
    """Rows (``PICK_COLUMNS``), one dict per instance 1..k in id order, from the int32 [P, 8] pick table (a host array or a tensor):
    ``picks``, the picks that carry the id, and ``picks_unoriented``, those of them with M == 0."""
    t = host_table(table, 8)
    ids = t[:, 3].astype(np.int64)
    if ids.size and (ids.min() < 1 or ids.max() > k):
        raise ValueError(f"the pick table holds ids outside 1..{k}")
    total = np.bincount(ids, minlength=k + 1)
    flat = np.bincount(ids[(t[:, 4:7] == 0).all(1)], minlength=k + 1)
    return [{"picks": int(total[i]), "picks_unoriented": int(flat[i])} for i in range(1, k + 1)]


def ball_voxels(r: int) -> int:
    """The voxels of the ball |o|^2 <= r^2."""
    a = np.arange(-r, r + 1)
    return int((a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2 <= r * r).sum())


def pick_records(table, opts: PickOptions) -> list[dict]:
    """One dict (``PICK_CSV_COLUMNS``) per row of the int32 [P, 8] pick table (a host array or a tensor), in its order:

    ``pick``            1..P
    ``id, z, y, x``     the instance and the voxel, as in ``<label>_instances``
    ``nz, ny, nx``      the outward unit normal -M / |M| in float64; nan when M == 0
    ``pz, py, px``      ((z, y, x) + pick_offset * n + 0.5) * pick_scale - 0.5; without a normal there is no offset
    ``rot, tilt, psi``  atan2(ny, nx), acos(nz), 0 in degrees; nan without a normal
    ``mz, my, mx``      M
    ``inside``          n / N, the share of the ball of ``pick_radius`` inside the object"""
    N = ball_voxels(opts.pick_radius)
    records = []
    for i, (z, y, x, ident, mz, my, mx, n) in enumerate(host_table(table, 8).tolist()):
        length = math.sqrt(mz * mz + my * my + mx * mx)
        if length > 0:
            normal = (-mz / length, -my / length, -mx / length)
            shift = tuple(opts.pick_offset * c for c in normal)
            rot = math.degrees(math.atan2(normal[1], normal[2]))
            tilt = math.degrees(math.acos(max(-1.0, min(1.0, normal[0]))))
            psi = 0.0
        else:
            normal, shift, rot, tilt, psi = 3 * (math.nan,), (0.0, 0.0, 0.0), math.nan, math.nan, math.nan
        pz, py, px = ((c + d + 0.5) * opts.pick_scale - 0.5 for c, d in zip((z, y, x), shift))
        records.append({"pick": i + 1, "id": ident, "z": z, "y": y, "x": x, "pz": pz, "py": py, "px": px,
                        "nz": normal[0], "ny": normal[1], "nx": normal[2], "rot": rot, "tilt": tilt, "psi": psi,
                        "mz": mz, "my": my, "mx": mx, "inside": n / N})
    return records


def _fixed(v) -> str:
    return str(v) if isinstance(v, int) else "nan" if math.isnan(v) else f"{v:.6f}"


def _replace(path: Path, text: str) -> Path:
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(path.name + ".tmp")
    tmp.write_text(text, newline="")
    os.replace(tmp, path)
    return path


def write_picks_csv(path, records: list[dict]) -> Path:
    """``records`` (``pick_records``) as CSV with the header ``PICK_CSV_COLUMNS``: every pick, integers as they are, every other
    value as %.6f, nan for an unoriented pick's normal and angles.  Written beside its final name and moved there."""
    lines = [",".join(PICK_CSV_COLUMNS)] + [",".join(_fixed(r[c]) for c in PICK_CSV_COLUMNS) for r in records]
    return _replace(Path(path), "\n".join(lines) + "\n")


def write_star(path, records: list[dict], micrograph: str) -> Path:
    """The oriented picks of ``records`` (``pick_records``), in their order, as a RELION STAR file: one ``data_particles`` loop with
    ``STAR_COLUMNS``; ``_rlnMicrographName`` = ``micrograph`` (the tomogram's stem), the coordinates px, py, pz and the angles in
    degrees as %.6f.  Written beside its final name and moved there."""
    if not micrograph or any(c.isspace() for c in micrograph):
        raise ValueError(f"a STAR value cannot be empty or hold white space, got {micrograph!r}")
    lines = ["", "# version 30001", "", "data_particles", "", "loop_"] + [f"{c} #{i + 1}" for i, c in enumerate(STAR_COLUMNS)]
    for r in records:
        if not math.isnan(r["nz"]):
            lines.append(" ".join([micrograph] + [f"{r[c]:.6f}" for c in ("px", "py", "pz", "rot", "tilt", "psi")]))
    return _replace(Path(path), "\n".join(lines) + "\n\n")


def read_picks_csv(path) -> list[dict]:
    """The records of a file of ``write_picks_csv``: integers for the integer columns, floats (nan included) for the others."""
    whole = {"pick", "id", "z", "y", "x", "mz", "my", "mx"}
    with open(path, newline="") as fh:
        return [{c: int(v) if c in whole else float(v) for c, v in row.items()} for row in csv.DictReader(fh)]


def read_star(path) -> tuple[list[str], list[list[str]]]:
    """(column names, rows of strings) of the one loop of a file of ``write_star``."""
    names, rows = [], []
    for line in Path(path).read_text().splitlines():
        line = line.strip()
        if line.startswith("_"):
            names.append(line.split()[0])
        elif line and not line.startswith(("#", "data_", "loop_")):
            rows.append(line.split())
    return names, rows
