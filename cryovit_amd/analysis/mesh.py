"""The surface of a labelled mask as a triangle mesh, for ChimeraX, IMOD, Blender or ParaView, and what the mesh says about each
instance: its triangles, its surface area and the volume it encloses.  All quantities are in voxels.

``engine.ops.mesh_surface`` (csrc/mesh.hip) builds the mesh on the device in integers: marching tetrahedra on the Kuhn decomposition
of the voxel lattice, one watertight, consistently oriented, indexed mesh per volume with every vertex stored once.
``engine.ops.mesh_smooth`` optionally relaxes it by integer Taubin smoothing and ``engine.ops.mesh_stats`` reduces it to 3 integers
per instance.  ``mesh_rows`` turns that table into the extra columns of the instance CSV, one dict per instance 1..k in id order;
``mesh_arrays`` returns mesh and table, ``instance_mesh`` the rows; ``write_ply`` and ``write_stl`` write the files.  Only the
writers and ``mesh_rows`` use floating point, in a fixed order, so equal arrays give equal files and rows.

What the numbers mean, and where they bend:

* The vertices are midpoint vertices: each sits halfway between a foreground and a background voxel centre, in units of 1/256
  voxel, so the raw mesh is a staircase of facets in a few fixed directions.  Its enclosed volume is close to the voxel count, but
  its ``mesh_area`` over-reads on slanted surfaces (the raw mesh of a ball of radius 4.5 reads 1.23 times the sphere's area, 1.07 times after 10 smoothing iterations).
  ``surface_area`` of ``--shape`` is the Crofton estimate, which has no such bias; the smoothed mesh (``--mesh-smooth N``, N about 10)
  is the one to quote beside it, the raw one is the one that reproduces the mask.  Smoothing moves vertices only: topology,
  triangle order and ids stay, the volume changes by little (Taubin's pair of steps does not shrink as plain averaging does).
* The 14-connectivity.  The six tetrahedra of a cell share its diagonal from (0, 0, 0) to (1, 1, 1), so two voxels are joined by
  the mesh where they share a face, or lie across one of the face diagonals (0, 1, 1), (1, 0, 1), (1, 1, 0) or the body diagonal
  (1, 1, 1) (in z, y, x; and their opposites): 14 neighbours, the same for foreground and background.  An instance of
  ``--connectivity 26`` whose parts meet only across one of the other diagonals shows as two shells under one id; two instances of
  ``--connectivity 6`` that meet across one of the 8 diagonal neighbours of the mesh share a shell.  The CSV rows stay per id.
* The union of touching pieces.  Ids play no part in where the surface lies: it is the surface of ``labels > 0``.  After
  ``--split-radius`` the pieces share faces and the cut plane carries no triangles; the pieces are meshed as their union, each
  triangle under the id of its tetrahedron's first foreground corner.  ``mesh_triangles`` and ``mesh_area`` of a piece are then
  those of its part of the common shell, and ``mesh_volume`` is only meaningful for an instance whose shell is closed by its own
  triangles: it is not for touching pieces (nor for ids that share a shell for any other reason).
* The border treated as background.  The volume is taken as surrounded by one layer of background, so every surface closes and a
  structure cut by the volume's face gets a flat cap there.  This differs from ``engine.ops.edt_squared`` and the thickness, where
  the border is no site.  A coordinate can therefore be -0.5.

Files.  PLY: binary little-endian, vertices float32 x, y, z in voxels, faces ``list uchar int vertex_indices`` plus ``int instance``.
STL: binary, the instance id in the attribute word, saturated at 65535.  The device arrays are in z, y, x order with the normal
``(p1 - p0) x (p2 - p0)`` pointing out of the foreground; writing x, y, z mirrors the handedness, so the writers exchange the
second and third index of every face and the files' normals point outward too.
"""

from __future__ import annotations

import os
from pathlib import Path

import numpy as np

from cryovit_amd.analysis._tables import host_table

MESH_COLUMNS = ["mesh_triangles", "mesh_area", "mesh_volume"]
MESH_FORMATS = ("ply", "stl")
UNIT = 256  # vertex units per voxel


def mesh_rows(table) -> list[dict]:
    """Rows (``MESH_COLUMNS``) from the int64 [k, 3] table of ``engine.ops.mesh_stats`` (a host array or a tensor; columns: triangles,
    sum of floor(|n|), sum of det(p0, p1, p2)):

    ``mesh_triangles``  c0
    ``mesh_area``       c1 / 2 / 65536
    ``mesh_volume``     c2 / 6 / 256^3

    An id without a triangle gives 0, 0.0, 0.0."""
    return [dict(zip(MESH_COLUMNS, (int(n), area2 / 2 / 65536, det / 6 / 256**3))) for n, area2, det in host_table(table, 3).tolist()]


def mesh_arrays(labels, k: int, smooth: int = 0, raw: bool = False):
    """(vertices int32 [V, 3], triangles int32 [T, 3], ids int32 [T], table int64 [k, 3]) of the int32 device volume ``labels``
    with the instances 1..k; all stay on the device.  ``smooth``: pairs of Taubin steps applied before the table is taken.
    ``raw``: a fifth entry, the vertices before smoothing (the midpoints, from which a vertex's two voxels can be recovered)."""
    from cryovit_amd.engine import ops

    if smooth < 0:
        raise ValueError(f"smooth must be >= 0, got {smooth}")
    vertices, triangles, ids = ops.mesh_surface(labels)
    unsmoothed = vertices
    if smooth:
        vertices = ops.mesh_smooth(vertices, triangles, smooth)
    out = (vertices, triangles, ids, ops.mesh_stats(vertices, triangles, ids, k))
    return (*out, unsmoothed) if raw else out


def instance_mesh(labels, k: int, smooth: int = 0) -> list[dict]:
    """The mesh columns of the instances 1..k of the int32 device volume ``labels``."""
    return mesh_rows(mesh_arrays(labels, k, smooth)[3])


def _file_arrays(vertices, triangles, ids):
    """(float32 [V, 3] in x, y, z and voxels, int32 [T, 3] with outward winding in that order, int32 [T])"""
    v = host_table(vertices, 3, np.int32)
    t = host_table(triangles, 3, np.int32)
    i = host_table(ids, 0, np.int32)
    if len(i) != len(t):
        raise ValueError(f"{len(i)} ids for {len(t)} triangles")
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("a triangle index lies outside the vertex array")
    xyz = (v[:, ::-1].astype(np.float64) / UNIT).astype(np.float32)
    return xyz, np.ascontiguousarray(t[:, [0, 2, 1]]), i


def _replace_into(path, write) -> Path:
    """``write(file)`` beside ``path``, then moved there: a reader never sees half a file."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(path.name + ".tmp")
    with open(tmp, "wb") as fh:
        write(fh)
    os.replace(tmp, path)
    return path


def write_ply(path, vertices, triangles, ids, vertex_values=None) -> Path:
    """Binary little-endian PLY of a mesh as ``engine.ops.mesh_surface`` returns it (host arrays or tensors).  ``vertex_values``
    (float [V], ``analysis.curvature.vertex_curvature``): written as ``property float curvature`` after x, y, z of every vertex;
    without it the file is the one it always was."""
    xyz, faces, inst = _file_arrays(vertices, triangles, ids)
    points = xyz.astype("<f4")
    if vertex_values is not None:
        values = host_table(vertex_values, 0, np.float32)
        if len(values) != len(xyz):
            raise ValueError(f"{len(values)} vertex values for {len(xyz)} vertices")
        points = np.concatenate([points, values.astype("<f4")[:, None]], axis=1)
    header = ("ply\nformat binary_little_endian 1.0\ncomment cryovit_amd surface mesh, voxel units\n"
              f"element vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\n"
              + ("property float curvature\n" if vertex_values is not None else "") +
              f"element face {len(faces)}\nproperty list uchar int vertex_indices\nproperty int instance\nend_header\n")
    rec = np.zeros(len(faces), dtype=np.dtype([("n", "u1"), ("v", "<i4", 3), ("instance", "<i4")]))
    rec["n"], rec["v"], rec["instance"] = 3, faces, inst

    def write(fh):
        fh.write(header.encode("ascii"))
        fh.write(points.tobytes())
        fh.write(rec.tobytes())

    return _replace_into(path, write)


def write_stl(path, vertices, triangles, ids) -> Path:
    """Binary STL (one unit normal and three corners per triangle; vertices are not shared in this format) with the instance id in
    the attribute word, saturated at 65535."""
    xyz, faces, inst = _file_arrays(vertices, triangles, ids)
    p = xyz[faces]  # [T, 3, 3]
    n = np.cross(p[:, 1].astype(np.float64) - p[:, 0], p[:, 2].astype(np.float64) - p[:, 0])
    length = np.sqrt((n * n).sum(1, keepdims=True))
    n = np.divide(n, length, out=np.zeros_like(n), where=length > 0)
    rec = np.zeros(len(faces), dtype=np.dtype([("normal", "<f4", 3), ("p", "<f4", (3, 3)), ("attribute", "<u2")]))
    rec["normal"], rec["p"], rec["attribute"] = n, p, np.clip(inst, 0, 65535)
    head = b"cryovit_amd surface mesh, voxel units, attribute = instance id".ljust(80, b" ")

    def write(fh):
        fh.write(head)
        fh.write(np.array(len(faces), "<u4").tobytes())
        fh.write(rec.tobytes())

    return _replace_into(path, write)


def write_mesh(path, vertices, triangles, ids, fmt: str = "ply", vertex_values=None) -> Path:
    if fmt not in MESH_FORMATS:
        raise ValueError(f"mesh format must be one of {MESH_FORMATS}, got {fmt!r}")
    if vertex_values is None:
        return (write_ply if fmt == "ply" else write_stl)(path, vertices, triangles, ids)
    if fmt != "ply":
        raise ValueError("an STL file has no per-vertex data: vertex values need the format 'ply'")
    return write_ply(path, vertices, triangles, ids, vertex_values)
