"""Oriented subtomograms at the picks of ``--pick`` or the filament points of ``--trace``: a box around every position, rotated so that
its z axis is the membrane normal or the filament tangent, cut out of the tomogram while it is in HBM; the boxes as an MRC stack
with a RELION STAR file, their average, and the density profile along the axis per instance.  The first thing anyone does with a
pick set is average the boxes and look: does the normal point out of the membrane, does the offset sit on the bilayer?

``engine.ops.extract_subtomograms`` (csrc/subtomo.hip) samples the boxes in fixed point and returns them as int32 in units of 2^-21
grey level (the definition is in include/cryovit_hip.h); ``subtomogram_sums`` adds them up in int64 and ``subtomogram_profiles`` sums
the disc of every z slab.  All three are exact, so equal tables give equal bytes in every file.  The host part here is float64 in a
fixed order: the frames, the quantisation of the table, the division of the sums.

What the numbers mean:

* The frame.  From a unit axis a = (a_z, a_y, a_x): rot = atan2(a_y, a_x), tilt = acos(a_z), and the box axes are the columns of
  Rz(rot) Ry(tilt), in xyz: x' = (cos rot cos tilt, sin rot cos tilt, -sin tilt), y' = (-sin rot, cos rot, 0), z' = a.  These are
  the angles the pick and the helical STAR files carry (psi = 0), so the box is what RELION would cut with those priors: the box z
  axis is the normal or the tangent, the in-plane angle is free.  At a = +z the frame is the identity; at a = -z (rot = 0 or pi, tilt = pi) it
  is finite, a half turn about y.  ``extract_orient="none"`` cuts axis-parallel boxes.
* The centre.  Picks: (z, y, x) + ``pick_offset`` * n.  Filament points: the sampled position.  Both in voxels of the segmented
  volume, which is the volume that is cut: ``pick_scale`` and ``trace_scale`` change the coordinates written to the STAR file, not
  where the box is taken.
* Quantisation.  The centre is rounded to 1/256 voxel, the matrix to 1/65536 (``rint``); the kernel then truncates every sample
  position to 1/128 voxel.  Against ``scipy.ndimage.map_coordinates(order=1, mode="nearest")`` at the quantised centre and matrix the
  box differs by at most (L_z + L_y + L_x) / 128 grey levels, L_a the largest difference between neighbours along axis a.
* Left out.  With ``"aligned"`` a pick without a normal (M = 0) and a filament point without a tangent have no frame: they are left out
  and counted per instance (``extract_skipped``).  With ``"none"`` they are kept.
* The average is the sum of all boxes divided by their number, in float64, then float32.  The profile of an instance is, per z slab
  of the box, the mean grey level over the disc o_y^2 + o_x^2 <= ``extract_profile_radius``^2 and over the instance's particles;
  slab B/2 holds the centre, slabs above it lie along +a (outside the object for a pick, whose normal points outwards).
* The STAR file holds the columns of the pick or helical STAR file plus ``_rlnImageName`` = ``%06d@<stack file>``.  With
  ``"aligned"`` the angles are written as 0: the images are already rotated.  With ``"none"`` they are the priors (0 where there is none).

Out of scope: float or 16-bit tomograms (``cryovit preprocess`` makes the uint8 volume), boxes above 128, one file per particle, CTF or
missing-wedge handling, classification (the alignment about the axis is ``analysis.alignment``), per-instance average volumes, thickness read off the profile, formats other
than MRC and RELION's STAR.
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from cryovit_amd.analysis.filaments import HELICAL_STAR_COLUMNS
from cryovit_amd.analysis.picks import STAR_COLUMNS, _fixed, _is_int, _is_number, _replace

EXTRACT_COLUMNS = ["extracted", "extract_skipped"]
BOX_MIN, BOX_MAX = 8, 128  # _lib.SUBTOMO_BOX_MIN / MAX
UNIT = 2.0 ** -21  # grey levels per unit of the int32 boxes
CALL_MAX = 1 << 20  # _lib.SUBTOMO_MAX_PARTICLES


@dataclass(frozen=True)
class ExtractOptions:
    """Whether oriented subtomograms are cut at one label's picks or filament points, and how.  With ``extract`` each file gains
    ``subtomograms/<tomo stem>_<label>.mrcs``, ``_average.mrc``, ``.star`` and ``_profiles.csv`` and the instance CSV
    ``EXTRACT_COLUMNS`` as its last columns.

    ``extract``                 None, ``"picks"`` (turns ``pick`` on) or ``"filaments"`` (turns ``trace`` on).
    ``extract_box``             the box edge B in voxels: an even integer in 8..128.
    ``extract_orient``          ``"aligned"``: box z along the normal / tangent; ``"none"``: axis-parallel boxes.
    ``extract_profile_radius``  the radius of the disc the profile averages over, in voxels (>= 0); None: B / 4.
    ``extract_chunk_bytes``     the device stack of one chunk of particles holds at most this many bytes (at least one particle)."""

    extract: str | None = None
    extract_box: int = 32
    extract_orient: str = "aligned"
    extract_profile_radius: float | None = None
    extract_chunk_bytes: int = 256 << 20

    def validate(self) -> "ExtractOptions":
        """Raises ``ValueError`` for a value out of range (whether or not ``extract`` is set); returns the record."""
        if self.extract not in (None, "picks", "filaments"):
            raise ValueError(f"extract must be None, 'picks' or 'filaments', got {self.extract!r}")
        if not _is_int(self.extract_box) or self.extract_box % 2 or not BOX_MIN <= self.extract_box <= BOX_MAX:
            raise ValueError(f"extract_box must be an even integer in [{BOX_MIN}, {BOX_MAX}], got {self.extract_box!r}")
        if self.extract_orient not in ("aligned", "none"):
            raise ValueError(f"extract_orient must be 'aligned' or 'none', got {self.extract_orient!r}")
        if self.extract_profile_radius is not None and (not _is_number(self.extract_profile_radius) or self.extract_profile_radius < 0):
            raise ValueError(f"extract_profile_radius must be a finite number >= 0, got {self.extract_profile_radius!r}")
        if not _is_int(self.extract_chunk_bytes) or self.extract_chunk_bytes < 1:
            raise ValueError(f"extract_chunk_bytes must be an integer >= 1, got {self.extract_chunk_bytes!r}")
        return self

    @property
    def radius2(self) -> int:
        """The largest integer o_y^2 + o_x^2 inside the profile's disc."""
        r = self.extract_box / 4 if self.extract_profile_radius is None else self.extract_profile_radius
        return int(math.floor(r * r + 1e-9))


def disc_voxels(box: int, radius2: int) -> int:
    """The voxels of a slab with o_y^2 + o_x^2 <= radius2, o = index - box / 2."""
    o = np.arange(box, dtype=np.int64) - box // 2
    return int((o[:, None] ** 2 + o[None, :] ** 2 <= radius2).sum())


def particle_frames(axes, orient: str = "aligned") -> np.ndarray:
    """float64 [P, 3, 3]: per unit axis (a_z, a_y, a_x) of ``axes`` ([P, 3]) the matrix whose row is the source axis z, y, x and whose
    column is the box axis z, y, x: the columns of Rz(rot) Ry(tilt) with rot = atan2(a_y, a_x), tilt = acos(a_z), re-indexed from xyz.
    ``orient="none"``: the identity for every particle."""
    axes = np.asarray(axes, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(axes), 3, 3), np.float64)
    for p, (az, ay, ax) in enumerate(axes.tolist()):
        if orient == "none":
            out[p] = np.eye(3)
            continue
        rot, tilt = math.atan2(ay, ax), math.acos(max(-1.0, min(1.0, az)))
        cr, sr, ct, st = math.cos(rot), math.sin(rot), math.cos(tilt), math.sin(tilt)
        cols = ((cr * st, sr * st, ct), (-sr, cr, 0.0), (cr * ct, sr * ct, -st))  # box z, y, x, each in source xyz
        for j, c in enumerate(cols):
            out[p, :, j] = (c[2], c[1], c[0])
    return out


def particle_table(centres, frames) -> np.ndarray:
    """int32 [P, 12], the table of ``engine.ops.extract_subtomograms``: ``rint(centre * 256)``, then ``rint(frame * 65536)`` row by row."""
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 9)
    q = np.rint(centres * 256.0)
    if q.size and np.abs(q).max() >= 2**31:
        raise ValueError("a particle centre lies beyond 2^23 voxels")
    return np.concatenate([q, np.rint(frames * 65536.0)], axis=1).astype(np.int32)


@dataclass
class Particles:
    """The particles of one extraction, in the order of their source records: ``ids`` (int64 [P], the instance), ``centres`` and ``axes``
    (float64 [P, 3], zyx; the axis is nan where there is none), ``star`` (per particle the cells of its STAR row before the image
    name), ``columns`` (the STAR columns before it) and ``skipped`` (int64 [k + 1]: per instance id the records that were left out).
    ``scale`` is the factor of the written coordinates ((c + 0.5) * scale - 0.5, ``pick_scale`` or ``trace_scale``) and
    ``alignment`` the ``analysis.alignment.Alignment`` of these particles once ``--extract-align`` has run."""

    ids: np.ndarray
    centres: np.ndarray
    axes: np.ndarray
    star: list[list[str]]
    columns: list[str]
    skipped: np.ndarray = field(default_factory=lambda: np.zeros(1, np.int64))
    scale: float = 1.0
    alignment: object | None = None


def _angles(record: dict, aligned: bool) -> list[str]:
    return [f"{0.0 if aligned or math.isnan(record[c]) else record[c]:.6f}" for c in ("rot", "tilt", "psi")]


def _gather(records: list[dict], k: int, orient: str, centre, axis, cells, columns: list[str], scale: float) -> Particles:
    aligned = orient == "aligned"
    ids, centres, axes, star = [], [], [], []
    skipped = np.zeros(k + 1, np.int64)
    for r in records:
        a = axis(r)
        if aligned and math.isnan(a[0]):
            skipped[r["id"]] += 1
            continue
        ids.append(r["id"])
        centres.append(centre(r))
        axes.append(a)
        star.append([f"{r[c]:.6f}" for c in ("px", "py", "pz")] + _angles(r, aligned) + cells(r))
    return Particles(np.asarray(ids, np.int64), np.asarray(centres, np.float64).reshape(-1, 3), np.asarray(axes, np.float64).reshape(-1, 3),
                     star, columns, skipped, scale)


def pick_particles(records: list[dict], k: int, pick_offset: float, orient: str, scale: float = 1.0) -> Particles:
    """The particles at the picks ``records`` (``analysis.picks.pick_records``) of the instances 1..k: the centre is
    (z, y, x) + ``pick_offset`` * n (no offset without a normal), the axis the outward normal.  ``scale`` is the ``pick_scale`` the
    records were made with: the alignment writes its refined coordinates under it."""
    def centre(r):
        n = (0.0, 0.0, 0.0) if math.isnan(r["nz"]) else (r["nz"], r["ny"], r["nx"])
        return tuple(c + pick_offset * d for c, d in zip((r["z"], r["y"], r["x"]), n))

    return _gather(records, k, orient, centre, lambda r: (r["nz"], r["ny"], r["nx"]), lambda r: [], STAR_COLUMNS, scale)


def filament_particles(points: list[dict], k: int, orient: str, scale: float = 1.0) -> Particles:
    """The particles at the filament points ``points`` (``analysis.filaments.sample_points``) of the instances 1..k: the centre is the
    sampled position, the axis the tangent.  ``scale`` is the ``trace_scale`` the points were made with: the alignment writes its
    refined coordinates under it."""
    return _gather(points, k, orient, lambda p: (p["z"], p["y"], p["x"]), lambda p: (p["tz"], p["ty"], p["tx"]),
                   lambda p: [str(p["branch"]), f"{p['track']:.6f}"], HELICAL_STAR_COLUMNS, scale)


def tomogram_bytes(data, shape, where: str) -> np.ndarray:
    """The uint8 volume that is cut: ``data`` as it is when it is uint8 of ``shape``.  ``utils.load_data`` hands ``infer`` a uint8
    tomogram as float32(v) / 255, and ``infer`` writes that into its prediction files: a float32 ``data`` in which every voxel is
    exactly such a quotient, v = 0..255, is turned back into v without loss.  Anything else raises."""
    data = np.asarray(data)
    if data.ndim == 4 and data.shape[0] == 1:
        data = data[0]
    got = f"{data.dtype} {tuple(data.shape)}"
    ok = tuple(data.shape) == tuple(shape) and data.dtype in (np.uint8, np.float32)
    if ok and data.dtype == np.float32:
        as_bytes = np.rint(np.clip(np.nan_to_num(data), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
        ok = bool((as_bytes.astype(np.float32) / 255.0 == data).all())
        got += " that is no uint8 volume over 255"
        data = as_bytes
    if not ok:
        raise ValueError(f"extract needs 'data' of {where} as a uint8 volume of shape {tuple(shape)} (got {got}): "
                         f"bring the tomogram to 8 bits with `cryovit preprocess` first")
    return np.ascontiguousarray(data)


def extract_rows(particles: Particles, k: int) -> list[dict]:
    """Rows (``EXTRACT_COLUMNS``), one dict per instance 1..k in id order: the particles cut and the records left out; after an
    alignment also ``analysis.alignment.ALIGN_COLUMNS``: the aligned particles and their mean score (nan without any)."""
    done = np.bincount(particles.ids, minlength=k + 1)
    rows = [{"extracted": int(done[i]), "extract_skipped": int(particles.skipped[i])} for i in range(1, k + 1)]
    if particles.alignment is not None:
        for row, more in zip(rows, particles.alignment.instance_rows(particles.ids, k)):
            row.update(more)
    return rows


def instance_profiles(ids, profile, k: int, box: int, radius2: int) -> list[dict]:
    """One dict (``id``, ``particles``, ``p_0`` .. ``p_{B-1}``) for id 0 (all particles) and every instance 1..k from the int64 [P, B]
    table of ``engine.ops.subtomogram_profiles``: the mean grey level of each slab's disc over the particles; nan without any."""
    ids, profile = np.asarray(ids, np.int64), np.asarray(profile, np.int64).reshape(-1, box)
    sums = np.zeros((k + 1, box), np.int64)
    np.add.at(sums, ids, profile)
    sums[0] = profile.sum(axis=0)
    count = np.bincount(ids, minlength=k + 1)
    count[0] = len(ids)
    area = disc_voxels(box, radius2)
    rows = []
    for i in range(k + 1):
        n = int(count[i])
        means = [float(s) * UNIT / (n * area) if n else math.nan for s in sums[i].tolist()]
        rows.append({"id": i, "particles": n, **{f"p_{j}": m for j, m in enumerate(means)}})
    return rows


def write_profiles_csv(path, rows: list[dict], box: int) -> Path:
    """``rows`` (``instance_profiles``) as CSV: ``id, particles, p_0 .. p_{B-1}``, the means as %.6f or nan.  Written beside its final
    name and moved there."""
    columns = ["id", "particles"] + [f"p_{j}" for j in range(box)]
    lines = [",".join(columns)] + [",".join(_fixed(r[c]) for c in columns) for r in rows]
    return _replace(Path(path), "\n".join(lines) + "\n")


def write_particle_star(path, particles: Particles, micrograph: str, stack_name: str) -> Path:
    """The particles as a RELION STAR file: one ``data_particles`` loop with the particles' own columns and ``_rlnImageName`` =
    ``%06d@<stack_name>``, counted from 1 in the order of the stack.  Written beside its final name and moved there."""
    for value in (micrograph, stack_name):
        if not value or any(c.isspace() for c in value):
            raise ValueError(f"a STAR value cannot be empty or hold white space, got {value!r}")
    columns = particles.columns + ["_rlnImageName"]
    lines = ["", "# version 30001", "", "data_particles", "", "loop_"] + [f"{c} #{i + 1}" for i, c in enumerate(columns)]
    lines += [" ".join([micrograph] + cells + [f"{i + 1:06d}@{stack_name}"]) for i, cells in enumerate(particles.star)]
    return _replace(Path(path), "\n".join(lines) + "\n\n")


def average_volume(sums, count: int) -> np.ndarray:
    """float32 [B, B, B]: the int64 sums of ``count`` boxes divided by it, in float64 grey levels, then rounded once."""
    return (np.asarray(sums, np.int64).astype(np.float64) * UNIT / count).astype(np.float32)


def chunk_particles(opts: ExtractOptions, per_particle_bytes: int) -> int:
    """The particles of one device chunk: ``extract_chunk_bytes`` over the bytes one particle takes, at least one, at most one call's."""
    return max(1, min(CALL_MAX, opts.extract_chunk_bytes // per_particle_bytes))


def cut_stack(volume, table: np.ndarray, box: int, per: int, stack_path: Path, voxel_size: float | None, radius2: int | None = None):
    """Cuts the rows of ``table`` (``particle_table``; at least one) out of the uint8 device ``volume``, ``per`` particles at a time
    through a pinned buffer, and writes them as the float32 stack ``stack_path`` (beside its final name, then moved there; a failure
    leaves no temporary file).  Returns (the int64 [B, B, B] sums of the boxes, the int64 [P, B] profile over the disc ``radius2``
    or None without one).  A frame that the kernel refuses raises ``RuntimeError``."""
    import torch

    from cryovit_amd.engine import ops
    from cryovit_amd.utils import mrc_header

    P = len(table)
    profile = None if radius2 is None else np.zeros((P, box), np.int64)
    sums = torch.zeros((1, box, box, box), dtype=torch.int64, device=volume.device)
    pinned = torch.empty((min(per, P), box, box, box), dtype=torch.int32, pin_memory=True)
    tmp = stack_path.with_name(stack_path.name + ".tmp")
    low, high, refused = math.inf, -math.inf, 0
    try:
        with open(tmp, "wb") as fh:
            fh.write(bytes(1024))
            for p0 in range(0, P, per):
                rows = torch.from_numpy(table[p0:p0 + per]).to(volume.device)
                stack, status = ops.extract_subtomograms(volume, rows, box)
                ops.subtomogram_sums(stack, torch.zeros(len(rows), dtype=torch.int32, device=volume.device), 1, sums)
                part = None if radius2 is None else ops.subtomogram_profiles(stack, radius2)
                host = pinned[:len(rows)]
                host.copy_(stack, non_blocking=True)
                if part is not None:
                    profile[p0:p0 + per] = part.cpu().numpy()
                refused += int(status.item())  # waits for the stream, the copy above included
                images = host.numpy().astype(np.float32) * np.float32(UNIT)  # one rounding, then an exact scale
                low, high = min(low, float(images.min())), max(high, float(images.max()))
                fh.write(images.tobytes())
            total = sums.cpu().numpy()[0]
            if refused:
                raise RuntimeError(f"{refused} particle frames were refused by the extraction kernel: they are no rotations")
            fh.seek(0)
            fh.write(mrc_header(box, box, P * box, mz=box, ispg=401, voxel_size=voxel_size, dmin=low, dmax=high,
                                dmean=float(int(total.sum())) * UNIT / (P * box**3)))
        os.replace(tmp, stack_path)
    finally:
        tmp.unlink(missing_ok=True)  # a failure leaves no half-written stack behind
    return total, profile


def extract_to_files(volume, particles: Particles, k: int, opts: ExtractOptions, results_dir, tomo_name: str, label_key: str,
                     voxel_size: float | None = None, align=None) -> dict[str, Path]:
    """Cuts ``particles`` out of the uint8 device ``volume`` under ``opts`` and writes ``subtomograms/<tomo stem>_<label>.mrcs`` (float32,
    a stack of volumes; chunk by chunk through a pinned buffer, at most ``extract_chunk_bytes`` of boxes on the device at a time),
    ``_average.mrc``, ``.star`` and ``_profiles.csv`` under ``results_dir``; every file is written beside its final name and moved
    there, and a run that fails leaves no temporary file.  Without particles the two MRC files are not written and those of an
    earlier run are removed, so the folder never holds boxes that the STAR file does not list.  ``align`` (an
    ``analysis.alignment.AlignOptions`` with ``extract_align`` set) then refines every box about its axis and adds the files of
    ``analysis.alignment.align_to_files``; without it no alignment call is made.  Returns the paths by suffix."""
    from cryovit_amd.utils import write_mrc

    box, radius2 = opts.extract_box, opts.radius2
    stem = Path(tomo_name).stem
    base = Path(results_dir) / "subtomograms" / f"{stem}_{label_key}"
    base.parent.mkdir(parents=True, exist_ok=True)
    stack_path, average_path = base.with_name(base.name + ".mrcs"), base.with_name(base.name + "_average.mrc")
    frames = particle_frames(particles.axes, opts.extract_orient)
    table = particle_table(particles.centres, frames)
    P = len(table)
    out = {}
    profile = np.zeros((P, box), np.int64)
    if P:
        total, profile = cut_stack(volume, table, box, chunk_particles(opts, 4 * box**3), stack_path, voxel_size, radius2)
        out["mrcs"] = stack_path
        out["average"] = write_mrc(average_path, average_volume(total, P), voxel_size)
    else:  # an earlier run's boxes would not belong to the STAR file written below
        stack_path.unlink(missing_ok=True)
        average_path.unlink(missing_ok=True)
    out["star"] = write_particle_star(base.with_name(base.name + ".star"), particles, stem, stack_path.name)
    out["profiles"] = write_profiles_csv(base.with_name(base.name + "_profiles.csv"), instance_profiles(particles.ids, profile, k, box, radius2), box)
    if align is not None and align.extract_align is not None:
        from cryovit_amd.analysis.alignment import align_to_files

        out.update(align_to_files(volume, particles, frames, opts, align, base, stem, voxel_size))
    return out
