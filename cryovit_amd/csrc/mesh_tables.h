// The tables of marching tetrahedra on the Kuhn decomposition (mesh.hip), built in plain C++ at compile time from the conventions of
// include/cryovit_hip.h; host and device read the same values, and a host program can print them.
//
// A corner of a cell is the code dz << 2 | dy << 1 | dx.  Tet t follows the t-th axis order of (z,y,x), (z,x,y), (y,z,x), (y,x,z),
// (x,z,y), (x,y,z): corner 0 is code 0, every further corner adds the next axis' bit, corner 3 is code 7.  An edge of the lattice
// runs from a voxel to the voxel at one of 7 offsets; edge type e has the offset code kMeshEdgeCode[e] (z, y, x, zy, zx, yx, zyx).
#pragma once
#include <stdint.h>

namespace cvx {

#define CVX_MESH_HD __host__ __device__

constexpr int kMeshEdgeCode[7] = {4, 2, 1, 6, 5, 3, 7};
constexpr int kMeshAxisOrder[6][3] = {{4, 2, 1}, {4, 1, 2}, {2, 4, 1}, {2, 1, 4}, {1, 4, 2}, {1, 2, 4}};  // the bit each step adds

CVX_MESH_HD constexpr int mesh_edge_type(int code) {
    for (int e = 0; e < 7; ++e)
        if (kMeshEdgeCode[e] == code) return e;
    return -1;
}

// corner i (0..3) of tet t, as a code
CVX_MESH_HD constexpr int mesh_tet_corner(int t, int i) {
    int c = 0;
    for (int s = 0; s < i; ++s) c |= kMeshAxisOrder[t][s];
    return c;
}

// A vertex of a triangle: the edge between the tet's corners i < j, as (code of corner i) << 3 | edge type.  The lower end of the
// edge is the cell's voxel + corner i.
CVX_MESH_HD constexpr int mesh_vertex_ref(int t, int i, int j) {
    const int lo = mesh_tet_corner(t, i < j ? i : j), hi = mesh_tet_corner(t, i < j ? j : i);
    return lo << 3 | mesh_edge_type(hi ^ lo);
}

// One entry per (tet, 4-bit case; bit i = corner i along the path is foreground):
//   bits 0..1   triangles (0, 1 or 2)
//   bits 2..4   the code of the first foreground corner along the path (whose label is the triangles' id)
//   bits 8..43  six vertex references of 6 bits: triangle 0 then triangle 1, each p0, p1, p2, already wound so that
//               (p1 - p0) x (p2 - p0) points from the foreground to the background
struct MeshCases {
    uint64_t entry[6][16];
};

CVX_MESH_HD constexpr uint64_t mesh_case_entry(int t, int m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
    for (int i = 0; i < 4; ++i) {
        if (m >> i & 1) in[nin++] = i;
        else out[nout++] = i;
    }
    if (nin == 0 || nin == 4) return 0;
    // the edges (a, b) of the triangles, three per triangle
    int ea[6] = {0, 0, 0, 0, 0, 0}, eb[6] = {0, 0, 0, 0, 0, 0}, ntri = 1;
    if (nin == 1) {
        for (int v = 0; v < 3; ++v) ea[v] = in[0], eb[v] = out[v];
    } else if (nin == 3) {
        for (int v = 0; v < 3; ++v) ea[v] = in[v], eb[v] = out[0];
    } else {  // the quad (ac, ad, bd, bc), cut along ac - bd
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        ntri = 2;
        ea[0] = a, eb[0] = c, ea[1] = a, eb[1] = d, ea[2] = b, eb[2] = d;
        ea[3] = a, eb[3] = c, ea[4] = b, eb[4] = d, ea[5] = b, eb[5] = c;
    }
    // from the centre of the foreground corners to the centre of the background corners, scaled to integers
    int towards[3] = {0, 0, 0};
    for (int ax = 0; ax < 3; ++ax) {
        for (int i = 0; i < nout; ++i) towards[ax] += nin * (mesh_tet_corner(t, out[i]) >> (2 - ax) & 1);
        for (int i = 0; i < nin; ++i) towards[ax] -= nout * (mesh_tet_corner(t, in[i]) >> (2 - ax) & 1);
    }
    uint64_t e = (uint64_t)ntri | (uint64_t)mesh_tet_corner(t, in[0]) << 2;
    for (int tri = 0; tri < ntri; ++tri) {
        int p[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // twice the midpoints
        for (int v = 0; v < 3; ++v)
            for (int ax = 0; ax < 3; ++ax)
                p[v][ax] = (mesh_tet_corner(t, ea[3 * tri + v]) >> (2 - ax) & 1) + (mesh_tet_corner(t, eb[3 * tri + v]) >> (2 - ax) & 1);
        int u[3] = {0, 0, 0}, w[3] = {0, 0, 0};
        for (int ax = 0; ax < 3; ++ax) u[ax] = p[1][ax] - p[0][ax], w[ax] = p[2][ax] - p[0][ax];
        const int side = (u[1] * w[2] - u[2] * w[1]) * towards[0] + (u[2] * w[0] - u[0] * w[2]) * towards[1] +
                         (u[0] * w[1] - u[1] * w[0]) * towards[2];
        for (int v = 0; v < 3; ++v) {
            const int s = side < 0 && v ? 3 - v : v;  // p1 and p2 exchanged
            e |= (uint64_t)mesh_vertex_ref(t, ea[3 * tri + s], eb[3 * tri + s]) << (8 + 6 * (3 * tri + v));
        }
    }
    return e;
}

CVX_MESH_HD constexpr MeshCases mesh_cases() {
    MeshCases c{};
    for (int t = 0; t < 6; ++t)
        for (int m = 0; m < 16; ++m) c.entry[t][m] = mesh_case_entry(t, m);
    return c;
}

// triangles of a tet with `fg` foreground corners
CVX_MESH_HD constexpr int mesh_case_triangles(int fg) { return fg == 2 ? 2 : (fg == 1 || fg == 3) ? 1 : 0; }

}  // namespace cvx
