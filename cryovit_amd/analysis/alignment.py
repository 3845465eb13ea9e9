"""Alignment of the oriented subtomograms of ``--extract`` about their axis (``--extract-align``): the boxes of ``analysis.subtomograms``
have their z axis along the membrane normal or the filament tangent, the angle about it is free and the position along it is as
good as the segmentation's surface voxel.  This is the first refinement of subtomogram averaging: a search over the in-plane angle
(T steps of 360 / T degrees) and the shift along the axis (-S..S voxels) against a reference that is the average of the particles as
they were aligned in the iteration before.

``engine.ops.subtomogram_polar`` resamples every slab of a box on rings around the axis and ``subtomogram_correlate`` correlates
the quantised rings with a reference table at every (shift, step), with the ring-weighted moments of the particle (csrc/align.hip;
the definition is in include/cryovit_hip.h).  Both are exact.  The host part here is float64, element by element in a fixed order.

* The score of a candidate (d, k) is the normalised correlation (C - a1 r1 / N) / sqrt((a2 - a1 a1 / N) (r2 - r1 r1 / N)):
  N = T (2 zh + 1) rmax (rmax + 1) / 2 the ring-weighted number of samples, a1 and a2 the integer sums of the two moments over the
  window's slabs at the shift d, r1 = sum r ref and r2 = sum r ref^2 exact integers; every integer becomes a float64 once and the
  expression is evaluated as written.  A variance that is not positive or a score that is not finite makes the candidate nan; a
  particle without a finite candidate is unaligned: psi = 0, shift = 0, score nan; it keeps its frame and is counted.
* The best candidate has the largest score; ties go to the smallest |d|, then the smallest d, then the smallest k.
* The reference table.  A reference box is int32 in 2^-21 grey level (sums // count, or clip(rint(v * 2^21), 0, 255 * 2^21) of an
  MRC file); its rings come from ``subtomogram_polar``; over the window's slabs mean = floor(sum r pol / N) and
  ref = clip((pol - mean + 2^14) >> 15, -32768, 32767): 1/64 grey level.
* The refinement of (d, k), psi = 2 pi k / T, of a frame F whose columns are the box axes z, y, x: x' = cos psi x + sin psi y,
  y' = -sin psi x + cos psi y, z unchanged, centre + d z: F Rz(psi) under the convention of ``subtomograms.particle_frames``.
  A particle cut with F0 Rz(psi_j) at c0 + d_j a answers k = -k_j mod T and d = -d_j against a reference cut with F0 at c0.
* The loop.  Without ``align_reference`` the start is the best-scoring particle against the plain average (lowest index on ties),
  cut again at its own shift.  Every iteration scores all particles as they were first cut (their rings never change), refines
  their frames, cuts them again with the refined frames and takes ``sums // count`` as the next reference; it stops early once no
  particle changes (d, k).  The last refined frames give the aligned stack: every box is interpolated once from the tomogram.

Out of scope: in-plane shifts, tilt refinement, missing-wedge or CTF weighting, classification, per-instance averages, helical
symmetry, resolution estimates.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from cryovit_amd.analysis.picks import _fixed, _is_int, _replace
from cryovit_amd.analysis.subtomograms import (UNIT, ExtractOptions, Particles, average_volume, chunk_particles, cut_stack, particle_table,
                                               write_particle_star)

ALIGN_COLUMNS = ["aligned", "align_score"]
ALIGNMENT_CSV_COLUMNS = ["particle", "id", "psi", "shift", "score", "cz", "cy", "cx", "rot", "tilt"]
ALIGNMENT_LOG_COLUMNS = ["iteration", "mean_score", "changed", "unaligned"]
ANGLES = (32, 64, 128)  # engine.ops.ALIGN_ANGLES
SHIFT_MAX = 8  # _lib.ALIGN_SHIFT_MAX
ITERATIONS_MAX = 20
GREY_MAX = 255 << 21  # the largest value of a box


@dataclass(frozen=True)
class AlignOptions:
    """Whether the boxes of ``--extract`` are aligned about their axis, and how.  With ``extract_align`` each file gains
    ``subtomograms/<tomo stem>_<label>_aligned.mrcs``, ``_aligned_average.mrc``, ``_aligned.star``, ``_alignment.csv`` and
    ``_alignment_log.csv`` and the instance CSV ``ALIGN_COLUMNS`` as its last columns.

    ``extract_align``    None (off) or the number of iterations, 1..20; needs ``extract_orient="aligned"``.
    ``align_angles``     T, the angular samples: 32, 64 or 128; the step is 360 / T degrees.
    ``align_shift``      S, the search range along the axis in voxels, 0..8.
    ``align_radius``     R: the rings 1..R are scored, 1 <= R <= B/2 - 1; None: B/2 - 2.
    ``align_height``     Z: the slabs B/2 - Z .. B/2 + Z of the reference are scored, Z >= 0 and Z + S <= B/2 - 1; None: B/2 - 1 - S.
    ``align_reference``  a float32 MRC volume of B^3 voxels in grey levels to start from; None: the start is bootstrapped."""

    extract_align: int | None = None
    align_angles: int = 64
    align_shift: int = 2
    align_radius: int | None = None
    align_height: int | None = None
    align_reference: str | None = None

    def validate(self, extract: ExtractOptions | None = None) -> "AlignOptions":
        """Raises ``ValueError`` for a value out of range (whether or not ``extract_align`` is set); with ``extract`` (validated) also
        for what does not fit its box or its orientation.  Returns the record."""
        if self.extract_align is not None and (not _is_int(self.extract_align) or not 1 <= self.extract_align <= ITERATIONS_MAX):
            raise ValueError(f"extract_align must be None or an integer in [1, {ITERATIONS_MAX}], got {self.extract_align!r}")
        if not _is_int(self.align_angles) or self.align_angles not in ANGLES:
            raise ValueError(f"align_angles must be 32, 64 or 128, got {self.align_angles!r}")
        if not _is_int(self.align_shift) or not 0 <= self.align_shift <= SHIFT_MAX:
            raise ValueError(f"align_shift must be an integer in [0, {SHIFT_MAX}], got {self.align_shift!r}")
        if self.align_radius is not None and (not _is_int(self.align_radius) or self.align_radius < 1):
            raise ValueError(f"align_radius must be an integer >= 1, got {self.align_radius!r}")
        if self.align_height is not None and (not _is_int(self.align_height) or self.align_height < 0):
            raise ValueError(f"align_height must be an integer >= 0, got {self.align_height!r}")
        if self.align_reference is not None and not isinstance(self.align_reference, (str, Path)):
            raise ValueError(f"align_reference must be a path, got {self.align_reference!r}")
        if extract is not None and self.extract_align is not None:
            if extract.extract is None:
                raise ValueError("extract_align needs extract: it aligns the boxes that extract cuts")
            if extract.extract_orient != "aligned":
                raise ValueError("extract_align needs extract_orient='aligned': axis-parallel boxes have no axis to turn about")
            self.search(extract.extract_box)
        return self

    def search(self, box: int) -> tuple[int, int, int, int]:
        """(T, S, R, Z) for boxes of edge ``box``, the defaults filled in; raises ``ValueError`` where they do not fit the box."""
        half = box // 2
        S = self.align_shift
        R = half - 2 if self.align_radius is None else self.align_radius
        Z = half - 1 - S if self.align_height is None else self.align_height
        if not 1 <= R <= half - 1:
            raise ValueError(f"align_radius must lie in [1, {half - 1}] for a box of {box}, got {R}")
        if Z < 0 or Z + S > half - 1:
            raise ValueError(f"align_height + align_shift must be <= {half - 1} for a box of {box} (and align_height >= 0), got {Z} + {S}")
        return self.align_angles, S, R, Z


def trig_table(angles: int) -> np.ndarray:
    """int32 [T, 2], the table of ``engine.ops.subtomogram_polar``: (rint(sin(2 pi t / T) * 2^14), rint(cos(2 pi t / T) * 2^14))."""
    return np.array([[round(math.sin(2 * math.pi * t / angles) * 16384), round(math.cos(2 * math.pi * t / angles) * 16384)]
                     for t in range(angles)], np.int32)


def samples(angles: int, rmax: int, zh: int) -> int:
    """N: the ring-weighted number of samples of a window."""
    return angles * (2 * zh + 1) * rmax * (rmax + 1) // 2


def box_from_sums(sums, count: int) -> np.ndarray:
    """int32 [B, B, B]: the reference box of the int64 sums of ``count`` boxes, ``sums // count``."""
    return (np.asarray(sums, np.int64) // count).astype(np.int32)


def box_from_grey(volume) -> np.ndarray:
    """int32 [B, B, B]: a float volume in grey levels as a box, clip(rint(v * 2^21), 0, 255 * 2^21)."""
    return np.clip(np.rint(np.asarray(volume, np.float64) * 2.0**21), 0, GREY_MAX).astype(np.int32)


def read_reference(path, box: int) -> np.ndarray:
    """The reference box of the MRC file ``path``: a float32 (mode 2) volume of ``box``^3 voxels; anything else raises ``ValueError``."""
    from cryovit_amd.utils import read_mrc

    data, _ = read_mrc(path)
    if data.dtype != np.float32 or tuple(data.shape) != (box, box, box):
        raise ValueError(f"align_reference {path} must be a float32 (mode 2) volume of shape {(box, box, box)}, got {data.dtype} {tuple(data.shape)}")
    if not np.isfinite(data).all():
        raise ValueError(f"align_reference {path} holds values that are not finite")
    return box_from_grey(data)


def reference_table(polar, zh: int) -> tuple[np.ndarray, int, int]:
    """(ref int16 [2 zh + 1, rmax, T], r1, r2) of the rings ``polar`` (int32 [B, rmax, T], ``subtomogram_polar`` of the reference box):
    the window's slabs minus their ring-weighted mean, in 1/64 grey level, and the exact integers sum r ref and sum r ref^2."""
    polar = np.asarray(polar, np.int64)
    box, rmax, angles = polar.shape
    window = polar[box // 2 - zh:box // 2 + zh + 1]
    weight = np.arange(1, rmax + 1, dtype=np.int64)[None, :, None]
    mean = int((weight * window).sum()) // samples(angles, rmax, zh)
    ref = np.clip((window - mean + (1 << 14)) >> 15, -32768, 32767)
    r1, r2 = int((weight * ref).sum()), int((weight * ref * ref).sum())
    return ref.astype(np.int16), r1, r2


def score_table(corr, moments, r1: int, r2: int, rmax: int, zh: int) -> np.ndarray:
    """float64 [P, 2 S + 1, T]: the normalised correlation of every candidate from ``corr`` (int64 [P, 2 S + 1, T]) and ``moments``
    (int64 [P, B, 2]) of ``engine.ops.subtomogram_correlate`` and the reference's r1, r2; nan where a variance is not positive or the
    score is not finite."""
    corr, moments = np.asarray(corr, np.int64), np.asarray(moments, np.int64)
    P, nd, angles = corr.shape
    box, S = moments.shape[1], nd // 2
    n = float(samples(angles, rmax, zh))
    lo = box // 2 - zh
    a = np.stack([moments[:, lo + d:lo + d + 2 * zh + 1].sum(axis=1) for d in range(-S, S + 1)], axis=1).astype(np.float64)  # [P, nd, 2], integer sums
    a1, a2 = a[:, :, 0], a[:, :, 1]
    f1, f2 = float(r1), float(r2)
    var_a, var_r = a2 - a1 * a1 / n, f2 - f1 * f1 / n
    with np.errstate(all="ignore"):
        score = (corr.astype(np.float64) - (a1 * f1 / n)[:, :, None]) / np.sqrt(var_a * var_r)[:, :, None]
    score[~np.isfinite(score)] = math.nan
    if not var_r > 0:
        score[:] = math.nan
    score[~(var_a > 0)] = math.nan
    return score


def best_candidates(score) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(d int64 [P], k int64 [P], score float64 [P]) of the float64 [P, 2 S + 1, T] table of ``score_table``: per particle the largest
    score, ties to the smallest |d|, then the smallest d, then the smallest k; (0, 0, nan) for a particle without a finite score."""
    score = np.asarray(score, np.float64)
    P, nd, angles = score.shape
    S = nd // 2
    order = sorted(range(-S, S + 1), key=lambda d: (abs(d), d))  # argmax takes the first of equals
    ranked = np.where(np.isnan(score), -math.inf, score)[:, [d + S for d in order]].reshape(P, nd * angles)
    at = ranked.argmax(axis=1) if P else np.zeros(0, np.int64)
    top = ranked[np.arange(P), at] if P else np.zeros(0)
    found = top > -math.inf
    d = np.where(found, np.asarray(order, np.int64)[at // angles], 0)
    k = np.where(found, at % angles, 0)
    return d.astype(np.int64), k.astype(np.int64), np.where(found, top, math.nan)


def refine_frames(frames, centres, d, k, angles: int) -> tuple[np.ndarray, np.ndarray]:
    """(frames float64 [P, 3, 3], centres float64 [P, 3]) after the shift ``d`` [P] along the box z axis and the turn by ``k`` [P] steps
    of 2 pi / ``angles`` about it: F Rz(psi), centre + d z (the columns of a frame are the box axes z, y, x)."""
    frames, centres = np.array(frames, np.float64).reshape(-1, 3, 3), np.array(centres, np.float64).reshape(-1, 3)
    for p, (dp, kp) in enumerate(zip(np.asarray(d).tolist(), np.asarray(k).tolist())):
        psi = 2 * math.pi * (kp % angles) / angles
        c, s = math.cos(psi), math.sin(psi)
        z, y, x = frames[p, :, 0].copy(), frames[p, :, 1].copy(), frames[p, :, 2].copy()
        frames[p, :, 2] = c * x + s * y
        frames[p, :, 1] = -s * x + c * y
        centres[p] = centres[p] + dp * z
    return frames, centres


def psi_degrees(k: int, angles: int) -> float:
    """The turn of ``k`` steps in degrees in (-180, 180]."""
    k %= angles
    return 360.0 * (k if 2 * k <= angles else k - angles) / angles


def euler_frame(rot: float, tilt: float, psi: float) -> np.ndarray:
    """float64 [3, 3]: Rz(rot) Ry(tilt) Rz(psi) (degrees) as a frame of ``subtomograms.particle_frames``: row = the source axis z, y, x,
    column = the box axis z, y, x."""
    a, b, g = (math.radians(v) for v in (rot, tilt, psi))
    rz = lambda t: np.array([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]])  # noqa: E731
    ry = np.array([[math.cos(b), 0.0, math.sin(b)], [0.0, 1.0, 0.0], [-math.sin(b), 0.0, math.cos(b)]])
    return (rz(a) @ ry @ rz(g))[::-1, ::-1].copy()  # xyz -> zyx on both sides


@dataclass
class Alignment:
    """What the alignment found, per particle: ``d`` and ``k`` (int64 [P]: the shift in voxels and the turn in steps), ``score`` (float64
    [P], nan = unaligned), the refined ``frames`` and ``centres``; ``angles`` = T and ``log``, one dict of ``ALIGNMENT_LOG_COLUMNS`` per
    iteration that ran."""

    d: np.ndarray
    k: np.ndarray
    score: np.ndarray
    frames: np.ndarray
    centres: np.ndarray
    angles: int
    log: list[dict]

    def instance_rows(self, ids, k: int) -> list[dict]:
        """Rows (``ALIGN_COLUMNS``), one per instance 1..k: the aligned particles and the mean of their scores (nan without any)."""
        rows = []
        ids = np.asarray(ids, np.int64)
        for i in range(1, k + 1):
            mine = self.score[ids == i]
            good = mine[~np.isnan(mine)]
            rows.append({"aligned": int(len(good)), "align_score": math.fsum(good.tolist()) / len(good) if len(good) else math.nan})
        return rows


def alignment_records(particles: Particles, found: Alignment) -> list[dict]:
    """One dict of ``ALIGNMENT_CSV_COLUMNS`` per particle: psi in degrees in (-180, 180], the shift in voxels, the final score, the
    refined centre and the angles rot, tilt (with psi: the refined frame is Rz(rot) Ry(tilt) Rz(psi)), coordinates written as
    (c + 0.5) * scale - 0.5 like those of the pick and the helical STAR files."""
    records = []
    for p in range(len(found.d)):
        az, ay, ax = particles.axes[p].tolist()
        cz, cy, cx = ((c + 0.5) * particles.scale - 0.5 for c in found.centres[p].tolist())
        records.append({"particle": p + 1, "id": int(particles.ids[p]), "psi": psi_degrees(int(found.k[p]), found.angles), "shift": int(found.d[p]),
                        "score": float(found.score[p]), "cz": cz, "cy": cy, "cx": cx, "rot": math.degrees(math.atan2(ay, ax)),
                        "tilt": math.degrees(math.acos(max(-1.0, min(1.0, az))))})
    return records


def write_alignment_csv(path, records: list[dict]) -> Path:
    """``records`` (``alignment_records``) as CSV, floats as %.6f or nan.  Written beside its final name and moved there."""
    lines = [",".join(ALIGNMENT_CSV_COLUMNS)] + [",".join(_fixed(r[c]) for c in ALIGNMENT_CSV_COLUMNS) for r in records]
    return _replace(Path(path), "\n".join(lines) + "\n")


def write_alignment_log(path, log: list[dict]) -> Path:
    """The iterations that ran (``ALIGNMENT_LOG_COLUMNS``) as CSV; an early stop shows as a last row with ``changed`` = 0 before the
    number of iterations asked for.  Written beside its final name and moved there."""
    lines = [",".join(ALIGNMENT_LOG_COLUMNS)] + [",".join(_fixed(r[c]) for c in ALIGNMENT_LOG_COLUMNS) for r in log]
    return _replace(Path(path), "\n".join(lines) + "\n")


def aligned_particles(particles: Particles, found: Alignment) -> Particles:
    """The particles as the aligned stack holds them, for ``write_particle_star``: the refined centres as coordinates, angles 0."""
    star = []
    for p, cells in enumerate(particles.star):
        cz, cy, cx = ((c + 0.5) * particles.scale - 0.5 for c in found.centres[p].tolist())
        star.append([f"{cx:.6f}", f"{cy:.6f}", f"{cz:.6f}", "0.000000", "0.000000", "0.000000"] + cells[6:])
    return Particles(particles.ids, found.centres, particles.axes, star, particles.columns, particles.skipped, particles.scale)


class _Scorer:
    """The device side of the loop: the particles as they were first cut, scored chunk by chunk against a reference box."""

    def __init__(self, volume, table: np.ndarray, box: int, angles: int, S: int, rmax: int, zh: int, per: int):
        import torch

        self.volume, self.table, self.box, self.angles, self.S, self.rmax, self.zh, self.per = volume, table, box, angles, S, rmax, zh, per
        self.trig = torch.from_numpy(trig_table(angles)).to(volume.device)

    def cut(self, table: np.ndarray):
        """The device stacks of the rows of ``table``, chunk by chunk."""
        import torch

        from cryovit_amd.engine import ops

        for p0 in range(0, len(table), self.per):
            stack, status = ops.extract_subtomograms(self.volume, torch.from_numpy(table[p0:p0 + self.per]).to(self.volume.device), self.box)
            yield p0, stack, status

    def sums(self, table: np.ndarray) -> np.ndarray:
        """int64 [B, B, B]: the sum of the boxes of ``table``."""
        import torch

        from cryovit_amd.engine import ops

        sums = torch.zeros((1, self.box, self.box, self.box), dtype=torch.int64, device=self.volume.device)
        refused = 0
        for _, stack, status in self.cut(table):
            ops.subtomogram_sums(stack, torch.zeros(len(stack), dtype=torch.int32, device=self.volume.device), 1, sums)
            refused += int(status.item())
        if refused:
            raise RuntimeError(f"{refused} particle frames were refused by the extraction kernel: they are no rotations")
        return sums.cpu().numpy()[0]

    def scores(self, reference: np.ndarray) -> np.ndarray:
        """float64 [P, 2 S + 1, T]: every particle's candidates against the reference box ``reference`` (int32 [B, B, B])."""
        import torch

        from cryovit_amd.engine import ops

        dev = self.volume.device
        rings = ops.subtomogram_polar(torch.from_numpy(np.ascontiguousarray(reference[None])).to(dev), self.trig, self.rmax)
        ref, r1, r2 = reference_table(rings[0].cpu().numpy(), self.zh)
        ref_dev = torch.from_numpy(ref).to(dev)
        out = np.zeros((len(self.table), 2 * self.S + 1, self.angles), np.float64)
        for p0, stack, _ in self.cut(self.table):
            corr, moments = ops.subtomogram_correlate(ops.subtomogram_polar(stack, self.trig, self.rmax), ref_dev, self.S)
            out[p0:p0 + len(stack)] = score_table(corr.cpu().numpy(), moments.cpu().numpy(), r1, r2, self.rmax, self.zh)
        return out


def align_particles(volume, centres, frames, box: int, align: AlignOptions, per: int, reference: np.ndarray | None = None) -> Alignment:
    """Runs the loop of the module text on the particles at ``centres`` (float64 [P, 3], P >= 1) with the frames ``frames`` ([P, 3, 3]) in
    the uint8 device ``volume``: ``align.extract_align`` iterations at most, ``per`` particles on the device at a time, from the
    reference box ``reference`` (int32 [B, B, B]) or, without one, the bootstrapped start."""
    angles, S, rmax, zh = align.search(box)
    centres, frames = np.asarray(centres, np.float64).reshape(-1, 3), np.asarray(frames, np.float64).reshape(-1, 3, 3)
    P = len(centres)
    scorer = _Scorer(volume, particle_table(centres, frames), box, angles, S, rmax, zh, per)
    if reference is None:
        d, _, score = best_candidates(scorer.scores(box_from_sums(scorer.sums(scorer.table), P)))
        first = int(np.nanargmax(score)) if not np.isnan(score).all() else 0  # the first of equals
        start_frames, start_centres = refine_frames(frames[first:first + 1], centres[first:first + 1], d[first:first + 1], [0], angles)
        reference = box_from_sums(scorer.sums(particle_table(start_centres, start_frames)), 1)
    d, k = np.zeros(P, np.int64), np.zeros(P, np.int64)
    log = []
    for iteration in range(1, align.extract_align + 1):
        new_d, new_k, score = best_candidates(scorer.scores(reference))
        changed = int(((new_d != d) | (new_k != k)).sum())
        d, k = new_d, new_k
        good = score[~np.isnan(score)]
        log.append({"iteration": iteration, "mean_score": math.fsum(good.tolist()) / len(good) if len(good) else math.nan, "changed": changed,
                    "unaligned": int(P - len(good))})
        new_frames, new_centres = refine_frames(frames, centres, d, k, angles)
        if changed == 0 and iteration > 1:
            break  # the same frames as before: the same reference, the same answer from here on
        if iteration < align.extract_align:
            reference = box_from_sums(scorer.sums(particle_table(new_centres, new_frames)), P)
    return Alignment(d, k, score, new_frames, new_centres, angles, log)


def align_to_files(volume, particles: Particles, frames, opts: ExtractOptions, align: AlignOptions, base: Path, stem: str,
                   voxel_size: float | None = None) -> dict[str, Path]:
    """Aligns ``particles`` (cut with ``frames`` under ``opts``) in the uint8 device ``volume`` under ``align`` and writes, beside the
    files of the extraction ``base``, ``_aligned.mrcs`` (every box cut again with its refined frame and centre), ``_aligned_average.mrc``,
    ``_aligned.star``, ``_alignment.csv`` and ``_alignment_log.csv``; every file is written beside its final name and moved there.
    Without particles the two MRC files of an earlier run are removed.  Sets ``particles.alignment``.  Returns the paths by suffix."""
    from cryovit_amd.utils import write_mrc

    align.validate(opts)
    box = opts.extract_box
    angles, _, rmax, _ = align.search(box)
    reference = None if align.align_reference is None else read_reference(align.align_reference, box)
    name = lambda suffix: base.with_name(base.name + suffix)  # noqa: E731
    stack_path, average_path = name("_aligned.mrcs"), name("_aligned_average.mrc")
    P = len(particles.ids)
    out = {}
    if P:
        found = align_particles(volume, particles.centres, frames, box, align, chunk_particles(opts, 4 * box**3 + 4 * box * rmax * angles), reference)
        total, _ = cut_stack(volume, particle_table(found.centres, found.frames), box, chunk_particles(opts, 4 * box**3), stack_path, voxel_size)
        out["aligned_mrcs"] = stack_path
        out["aligned_average"] = write_mrc(average_path, average_volume(total, P), voxel_size)
    else:
        found = Alignment(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3)), angles, [])
        stack_path.unlink(missing_ok=True)
        average_path.unlink(missing_ok=True)
    particles.alignment = found
    out["aligned_star"] = write_particle_star(name("_aligned.star"), aligned_particles(particles, found), stem, stack_path.name)
    out["alignment"] = write_alignment_csv(name("_alignment.csv"), alignment_records(particles, found))
    out["alignment_log"] = write_alignment_log(name("_alignment_log.csv"), found.log)
    return out
