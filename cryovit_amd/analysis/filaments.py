"""Filaments along the skeleton of every instance: how many branches there are and how long and how straight each is, which branches
meet at which junction, and where to cut segments for helical averaging (microtubules, actin, any tube), as CSV and a RELION STAR
file.  All lengths are in voxels of the segmented volume unless a scale is named.

``engine.ops.trace_skeleton`` (csrc/trace.hip) turns the skeleton volume of ``analysis.skeleton`` into two integer tables on the
device (the definition is in include/cryovit_hip.h): the voxel table, one row z, y, x, id, degree, branch, rank, f, e, c, d2, ring
per skeleton voxel in raster order, and the branch table, one row id, kind, path_voxels, f, e, c, start_index, end_index,
start_degree, end_degree, sum_d2, min_d2, max_d2, head_index, last_index, chord2 per branch.  Everything here works on those two
tables on the host.  Floating point appears only here, in float64 and in a fixed order, and the writers print fixed ``%.6f``
formats, so equal tables give equal bytes.

What the numbers mean:

* Voxels.  A path voxel has exactly two neighbours (26-adjacent, same id); every other skeleton voxel is a node voxel: an end (one
  neighbour), a point (none) or a junction voxel (three or more).  Junction voxels that touch form one junction (``junction_nodes``).
* Branches.  A chain is a run of path voxels between two node voxels, a ring a closed run without a node, a link an end that sits
  directly on a node voxel.  ``kind`` says what a branch connects: ``end-end``, ``end-junction``, ``junction-junction``, ``ring``.
* ``length`` is (f + sqrt 2 e) + sqrt 3 c over the steps from the start node through the path voxels to the end node (a ring: back
  to its first voxel).  Unlike ``skeleton_length`` it counts no pair of a junction's clique twice: steps between junction voxels
  belong to no branch.  ``chord`` is the distance between the two node voxels, ``tortuosity`` = length / chord (nan for a ring).
* ``radius_*`` come from the distance map of the run (the distance to the background at the path voxels).
* Points.  ``sample_points`` walks every branch as the polyline start node, path voxels by rank, end node and places a position
  every ``trace_spacing`` voxels of arc length from the start; the tangent is the direction between the positions ``trace_window``
  before and after it (clamped to the branch; wrapped around on a ring).
* Polarity is arbitrary: a branch starts at the end whose first path voxel has the smaller raster index, so the tangent of a
  filament may point either way along it, and two branches of one microtubule may disagree.  The CSV tangents are authoritative;
  the STAR angles follow the picks' convention (rot = atan2(ty, tx), tilt = acos(tz), psi = 0: the particle's z axis lies along
  the filament) and the conventions of other packages are to be derived from the tangents.
* Position.  Written coordinates are (q + 0.5) * ``trace_scale`` - 0.5, as the picks; ``_rlnHelicalTrackLengthAngst`` is arc *
  ``trace_scale`` * ``trace_angpix``.

Out of scope: pruning spurs and joining branches across a junction (a microtubule with a side spur yields two tube ids beside
the spur), longest-path or graph-diameter filaments, smoothing of the polyline beyond the tangent window, particle formats other
than RELION's.
"""

from __future__ import annotations

import bisect
import csv
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from cryovit_amd.analysis._tables import host_table
from cryovit_amd.analysis.picks import STAR_COLUMNS, _fixed, _is_number, _replace, read_star  # noqa: F401  (read_star: the round trip)

VOXEL_COLS, BRANCH_COLS = 12, 16  # _lib.TRACE_VOXEL_COLS / TRACE_BRANCH_COLS
KINDS = ["end-end", "end-junction", "junction-junction", "ring"]
FILAMENT_COLUMNS = ["filament_branches", "filament_rings", "filament_junctions", "filament_points", "filament_length", "filament_longest",
                    "filament_tortuosity"]
BRANCH_CSV_COLUMNS = ["branch", "id", "kind", "start_node", "end_node", "voxels", "length", "chord", "tortuosity", "radius_mean", "radius_min",
                      "radius_max", "sz", "sy", "sx", "ez", "ey", "ex"]
POINT_CSV_COLUMNS = ["point", "branch", "id", "arc", "z", "y", "x", "pz", "py", "px", "tz", "ty", "tx", "rot", "tilt", "psi", "radius"]
HELICAL_STAR_COLUMNS = STAR_COLUMNS + ["_rlnHelicalTubeID", "_rlnHelicalTrackLengthAngst"]

_SQRT2, _SQRT3 = math.sqrt(2.0), math.sqrt(3.0)


@dataclass(frozen=True)
class TraceOptions:
    """Whether the skeletons of one label's instances are traced into filaments, and how they are sampled.  With ``trace`` each file
    gains ``filaments/<tomo stem>_<label>_branches.csv``, ``filaments/<tomo stem>_<label>.csv`` and ``.star``, the dataset
    ``<label>_filaments`` and the instance CSV ``FILAMENT_COLUMNS`` directly after the skeleton's columns.

    ``trace``             trace them (turns ``skeleton`` on).
    ``trace_spacing``     the arc length between two sampled positions of a branch, in voxels (>= 1).
    ``trace_window``      the tangent at a position is taken between the points this far before and after it, in voxels (>= 1).
    ``trace_min_length``  branches shorter than this get no positions (>= 0); they stay in the branch CSV and the columns.
    ``trace_scale``       written coordinates are (q + 0.5) * scale - 0.5: the bin factor of ``preprocess --bin`` (> 0).
    ``trace_angpix``      Angstrom per voxel of the unbinned tomogram, for ``_rlnHelicalTrackLengthAngst`` (> 0)."""

    trace: bool = False
    trace_spacing: float = 8.0
    trace_window: float = 4.0
    trace_min_length: float = 0.0
    trace_scale: float = 1.0
    trace_angpix: float = 1.0

    def validate(self) -> "TraceOptions":
        """Raises ``ValueError`` for a value out of range (whether or not ``trace`` is on); returns the record."""
        if not _is_number(self.trace_spacing) or not self.trace_spacing >= 1:
            raise ValueError(f"trace_spacing must be a finite number >= 1, got {self.trace_spacing!r}")
        if not _is_number(self.trace_window) or not self.trace_window >= 1:
            raise ValueError(f"trace_window must be a finite number >= 1, got {self.trace_window!r}")
        if not _is_number(self.trace_min_length) or not self.trace_min_length >= 0:
            raise ValueError(f"trace_min_length must be a finite number >= 0, got {self.trace_min_length!r}")
        if not _is_number(self.trace_scale) or not self.trace_scale > 0:
            raise ValueError(f"trace_scale must be a finite number > 0, got {self.trace_scale!r}")
        if not _is_number(self.trace_angpix) or not self.trace_angpix > 0:
            raise ValueError(f"trace_angpix must be a finite number > 0, got {self.trace_angpix!r}")
        return self


def trace_tables(skeleton, k: int, d2=None):
    """(voxels int32 [N, 12], branches int64 [B, 16]) of the ids 1..k of the int32 device volume ``skeleton``; both stay on the device."""
    from cryovit_amd.engine import ops

    return ops.trace_skeleton(skeleton, k, d2=d2)


def _length(f: int, e: int, c: int) -> float:
    return (float(f) + _SQRT2 * e) + _SQRT3 * c


class _Graph:
    """The voxel table with the same-id neighbours of a voxel looked up by coordinate."""

    def __init__(self, voxels):
        self.rows = host_table(voxels, VOXEL_COLS).tolist()
        self.slot = {(r[0], r[1], r[2]): i for i, r in enumerate(self.rows)}

    def around(self, i: int) -> list[int]:
        """The slots of the neighbours of voxel i, ascending."""
        z, y, x, ident = self.rows[i][:4]
        found = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    j = self.slot.get((z + dz, y + dy, x + dx))
                    if j is not None and j != i and self.rows[j][3] == ident:
                        found.append(j)
        return found

    def by_branch(self) -> dict[int, list[int]]:
        """branch -> the slots of its path voxels by rank."""
        out: dict[int, list[int]] = {}
        for i, r in enumerate(self.rows):
            if r[5] > 0:
                out.setdefault(r[5], []).append(i)
        for members in out.values():
            members.sort(key=lambda i: self.rows[i][6])
        return out


def _nodes(g: _Graph) -> tuple[list[dict], dict[int, int]]:
    rows = g.rows
    parent = {i: i for i, r in enumerate(rows) if r[4] >= 3}

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in parent:
        for j in g.around(i):
            if j in parent:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)  # the root of a cluster is its smallest voxel
    members: dict[int, list[int]] = {}
    for i, r in enumerate(rows):
        if r[4] != 2:
            members.setdefault(find(i) if r[4] >= 3 else i, []).append(i)
    nodes, node_of = [], {}
    for n, root in enumerate(sorted(members)):
        group = members[root]
        deg = rows[root][4]
        count = len(group)
        nodes.append({"node": n + 1, "id": rows[root][3], "kind": "junction" if deg >= 3 else "end" if deg == 1 else "point", "voxels": count,
                      "z": sum(rows[i][0] for i in group) / count, "y": sum(rows[i][1] for i in group) / count,
                      "x": sum(rows[i][2] for i in group) / count})
        for i in group:
            node_of[i] = n + 1
    return nodes, node_of


def junction_nodes(voxels) -> tuple[list[dict], dict[int, int]]:
    """(nodes, node_of) of the voxel table (a host array or a tensor).  A node is an end voxel, a point or a cluster of junction
    voxels that are neighbours (a small union-find: there are few such voxels); nodes are numbered 1.. in raster order of their
    smallest voxel.  ``nodes``: one dict ``node, id, kind`` (``end``, ``point``, ``junction``), ``voxels``, ``z, y, x`` (the mean of
    its voxels) per node; ``node_of``: row of the voxel table -> node number, for every node voxel."""
    return _nodes(_Graph(voxels))


def _branch_ends(g: _Graph, branches: list[list[int]]) -> list[tuple[int, list[int], int]]:
    """Per branch (start slot, path slots by rank, end slot).  The branch table names its node voxels by linear index, which needs
    the volume's extents to resolve; here they are found from the voxel table alone: next to the first and last path voxel of a
    chain, and for the links, whose keys are the ends that sit on a node voxel, by their raster order."""
    rows = g.rows
    paths = g.by_branch()
    links = []
    for i, r in enumerate(rows):
        if r[4] == 1:
            (w,) = g.around(i)
            if rows[w][4] != 2 and not (rows[w][4] == 1 and w < i):
                links.append((i, w))
    out, taken = [], 0
    for b, row in enumerate(branches):
        members = paths.get(b + 1, [])
        if len(members) != row[2]:
            raise ValueError(f"branch {b + 1} has {row[2]} path voxels in the branch table and {len(members)} in the voxel table")
        if row[1] == 3:
            out.append((members[0], members, members[0]))
        elif not members:
            if taken >= len(links):
                raise ValueError("the branch table holds more links than the voxel table")
            out.append((links[taken][0], [], links[taken][1]))
            taken += 1
        elif len(members) == 1:
            a, c = g.around(members[0])
            out.append((a, members, c))
        else:
            (a,) = [j for j in g.around(members[0]) if j != members[1]]
            (c,) = [j for j in g.around(members[-1]) if j != members[-2]]
            out.append((a, members, c))
    return out


def _records(g: _Graph, branches: list[list[int]], node_of: dict[int, int]) -> list[dict]:
    rows = g.rows
    records = []
    for b, ((a, members, c), row) in enumerate(zip(_branch_ends(g, branches), branches)):
        ident, kind, n, f, e, cc = row[:6]
        length = _length(f, e, cc)
        chord = math.sqrt(row[15])
        ring = kind == 3
        records.append({"branch": b + 1, "id": ident, "kind": KINDS[kind], "start_node": 0 if ring else node_of[a],
                        "end_node": 0 if ring else node_of[c], "voxels": n, "length": length, "chord": chord,
                        "tortuosity": math.nan if ring or chord == 0 else length / chord,
                        "radius_mean": math.sqrt(row[10] / n) if n else math.nan, "radius_min": math.sqrt(row[11]) if n else math.nan,
                        "radius_max": math.sqrt(row[12]) if n else math.nan,
                        "sz": rows[a][0], "sy": rows[a][1], "sx": rows[a][2], "ez": rows[c][0], "ey": rows[c][1], "ex": rows[c][2]})
    return records


def branch_records(voxels, branches) -> list[dict]:
    """One dict (``BRANCH_CSV_COLUMNS``) per row of the branch table, in its order, from both tables (host arrays or tensors):

    ``branch``                 1..B
    ``id``                     the instance
    ``kind``                   ``end-end``, ``end-junction``, ``junction-junction`` or ``ring``
    ``start_node, end_node``   the nodes of ``junction_nodes`` it runs between; 0 for a ring, which has none
    ``voxels``                 its path voxels
    ``length, chord``          (f + sqrt 2 e) + sqrt 3 c in that order; sqrt(chord2)
    ``tortuosity``             length / chord; nan for a ring and where the chord is 0 (a loop back to the same voxel)
    ``radius_mean/min/max``    sqrt(sum_d2 / voxels), sqrt(min_d2), sqrt(max_d2); nan without path voxels
    ``sz, sy, sx, ez, ey, ex`` the start and end node voxels (of a ring both its first voxel)"""
    g = _Graph(voxels)
    return _records(g, host_table(branches, BRANCH_COLS).tolist(), _nodes(g)[1])


def filament_rows(voxels, branches, k: int) -> list[dict]:
    """Rows (``FILAMENT_COLUMNS``), one dict per instance 1..k in id order: ``filament_branches``, the branches with the id;
    ``filament_rings`` of them; ``filament_junctions``, the junction clusters; ``filament_points``, the isolated voxels;
    ``filament_length``, the sum of the branch lengths in branch order; ``filament_longest``, the largest of them;
    ``filament_tortuosity`` of that branch (the first of equals; nan without a branch)."""
    g = _Graph(voxels)
    nodes, node_of = _nodes(g)
    rows = [dict(zip(FILAMENT_COLUMNS, (0, 0, 0, 0, 0.0, 0.0, math.nan))) for _ in range(k)]
    for node in nodes:
        if not 1 <= node["id"] <= k:
            raise ValueError(f"the voxel table holds ids outside 1..{k}")
        if node["kind"] != "end":
            rows[node["id"] - 1]["filament_junctions" if node["kind"] == "junction" else "filament_points"] += 1
    for r in _records(g, host_table(branches, BRANCH_COLS).tolist(), node_of):
        if not 1 <= r["id"] <= k:
            raise ValueError(f"the branch table holds ids outside 1..{k}")
        row = rows[r["id"] - 1]
        row["filament_branches"] += 1
        row["filament_rings"] += r["kind"] == "ring"
        row["filament_length"] += r["length"]
        if r["length"] > row["filament_longest"]:
            row["filament_longest"], row["filament_tortuosity"] = r["length"], r["tortuosity"]
    return rows


class _Polyline:
    """Vertices with a value each, walked by arc length: linear between vertices."""

    def __init__(self, points: list[tuple], values: list[float], closed: bool):
        self.points, self.values, self.closed = points, values, closed
        self.arc = [0.0]
        for p, q in zip(points, points[1:]):
            self.arc.append(self.arc[-1] + math.sqrt(sum((a - b) * (a - b) for a, b in zip(p, q))))
        self.total = self.arc[-1]

    def _place(self, s: float) -> tuple[int, float]:
        if self.closed:
            s = math.fmod(s, self.total)
            s = s + self.total if s < 0 else s
        s = min(max(s, 0.0), self.total)
        i = min(max(bisect.bisect_right(self.arc, s) - 1, 0), len(self.points) - 2)
        return i, (s - self.arc[i]) / (self.arc[i + 1] - self.arc[i])

    def at(self, s: float) -> tuple:
        i, t = self._place(s)
        return tuple(a + t * (b - a) for a, b in zip(self.points[i], self.points[i + 1]))

    def value(self, s: float) -> float:
        i, t = self._place(s)
        return self.values[i] + t * (self.values[i + 1] - self.values[i])


def sample_points(voxels, branches, opts: TraceOptions) -> list[dict]:
    """One dict (``POINT_CSV_COLUMNS`` and ``track``) per sampled position, branch by branch, from both tables (host arrays or tensors).
    Every branch of length >= ``trace_min_length`` is the polyline start node, path voxels by rank, end node (a ring closes on its
    first voxel); positions lie at the arc lengths 0, S, 2 S, ... up to its length, S = ``trace_spacing`` (on a ring below it: the
    length itself is the first voxel again).

    ``point``           1.. over all branches
    ``branch, id``      the branch (the helical tube id) and the instance
    ``arc``             the arc length from the start node, in voxels
    ``z, y, x``         the position q in voxels of the segmented volume, linear between voxel centres
    ``pz, py, px``      (q + 0.5) * trace_scale - 0.5
    ``tz, ty, tx``      the unit tangent (P(arc + h) - P(arc - h)) / |...|, h = ``trace_window``, the arguments clamped to the branch
                        and on a ring wrapped around it; nan where the two points coincide
    ``rot, tilt, psi``  atan2(ty, tx), acos(tz), 0 in degrees; nan without a tangent
    ``radius``          sqrt(d2) linear between the vertices
    ``track``           arc * trace_scale * trace_angpix"""
    g = _Graph(voxels)
    rows = g.rows
    table = host_table(branches, BRANCH_COLS).tolist()
    points = []
    for b, ((a, members, c), row) in enumerate(zip(_branch_ends(g, table), table)):
        if _length(*row[3:6]) < opts.trace_min_length:
            continue
        ring = row[1] == 3
        walk = members + [members[0]] if ring else [a] + members + [c]
        line = _Polyline([tuple(float(v) for v in rows[i][:3]) for i in walk], [math.sqrt(rows[i][10]) for i in walk], ring)
        j = 0
        while j * opts.trace_spacing <= line.total:
            s = j * opts.trace_spacing
            if ring and line.total - s < 1e-9:  # the first voxel again (the length is a sum of roots: equal up to rounding)
                break
            q = line.at(s)
            d = tuple(u - v for u, v in zip(line.at(s + opts.trace_window), line.at(s - opts.trace_window)))
            norm = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if norm > 0:
                t = (d[0] / norm, d[1] / norm, d[2] / norm)
                rot, tilt, psi = math.degrees(math.atan2(t[1], t[2])), math.degrees(math.acos(max(-1.0, min(1.0, t[0])))), 0.0
            else:
                t, rot, tilt, psi = 3 * (math.nan,), math.nan, math.nan, math.nan
            pz, py, px = ((v + 0.5) * opts.trace_scale - 0.5 for v in q)
            points.append({"point": len(points) + 1, "branch": b + 1, "id": row[0], "arc": s, "z": q[0], "y": q[1], "x": q[2],
                           "pz": pz, "py": py, "px": px, "tz": t[0], "ty": t[1], "tx": t[2], "rot": rot, "tilt": tilt, "psi": psi,
                           "radius": line.value(s), "track": s * opts.trace_scale * opts.trace_angpix})
            j += 1
    return points


def filament_volume(voxels, shape) -> np.ndarray:
    """int32 [D, H, W]: the branch number on path and ring voxels, -1 on node voxels, 0 elsewhere, from the voxel table."""
    t = host_table(voxels, VOXEL_COLS)
    out = np.zeros(tuple(shape), np.int32)
    out[t[:, 0], t[:, 1], t[:, 2]] = np.where(t[:, 4] == 2, t[:, 5], -1)
    return out


def _cell(v) -> str:
    return v if isinstance(v, str) else _fixed(v)


def write_branches_csv(path, records: list[dict]) -> Path:
    """``records`` (``branch_records``) as CSV with the header ``BRANCH_CSV_COLUMNS``: integers and words as they are, every other
    value as %.6f or nan.  Written beside its final name and moved there."""
    lines = [",".join(BRANCH_CSV_COLUMNS)] + [",".join(_cell(r[c]) for c in BRANCH_CSV_COLUMNS) for r in records]
    return _replace(Path(path), "\n".join(lines) + "\n")


def write_points_csv(path, points: list[dict]) -> Path:
    """``points`` (``sample_points``) as CSV with the header ``POINT_CSV_COLUMNS``: integers as they are, every other value as %.6f
    or nan.  Written beside its final name and moved there."""
    lines = [",".join(POINT_CSV_COLUMNS)] + [",".join(_cell(p[c]) for c in POINT_CSV_COLUMNS) for p in points]
    return _replace(Path(path), "\n".join(lines) + "\n")


def write_helical_star(path, points: list[dict], micrograph: str) -> Path:
    """The positions of ``points`` (``sample_points``) that have a tangent, in their order, as a RELION STAR file: one
    ``data_particles`` loop with ``HELICAL_STAR_COLUMNS``; ``_rlnMicrographName`` = ``micrograph`` (the tomogram's stem), the
    coordinates px, py, pz and the angles in degrees as %.6f, ``_rlnHelicalTubeID`` the branch number and
    ``_rlnHelicalTrackLengthAngst`` the track length as %.6f.  Written beside its final name and moved there."""
    if not micrograph or any(c.isspace() for c in micrograph):
        raise ValueError(f"a STAR value cannot be empty or hold white space, got {micrograph!r}")
    lines = ["", "# version 30001", "", "data_particles", "", "loop_"] + [f"{c} #{i + 1}" for i, c in enumerate(HELICAL_STAR_COLUMNS)]
    for p in points:
        if not math.isnan(p["tz"]):
            lines.append(" ".join([micrograph] + [f"{p[c]:.6f}" for c in ("px", "py", "pz", "rot", "tilt", "psi")] + [str(p["branch"]), f"{p['track']:.6f}"]))
    return _replace(Path(path), "\n".join(lines) + "\n\n")


def read_branches_csv(path) -> list[dict]:
    """The records of a file of ``write_branches_csv``: integers, the kind as a word, floats (nan included) for the others."""
    whole = {"branch", "id", "start_node", "end_node", "voxels", "sz", "sy", "sx", "ez", "ey", "ex"}
    with open(path, newline="") as fh:
        return [{c: v if c == "kind" else int(v) if c in whole else float(v) for c, v in row.items()} for row in csv.DictReader(fh)]


def read_points_csv(path) -> list[dict]:
    """The records of a file of ``write_points_csv``: integers for point, branch and id, floats (nan included) for the others."""
    whole = {"point", "branch", "id"}
    with open(path, newline="") as fh:
        return [{c: int(v) if c in whole else float(v) for c, v in row.items()} for row in csv.DictReader(fh)]
