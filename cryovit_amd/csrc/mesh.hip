// Surface mesh of a label volume (`--mesh`): marching tetrahedra on the Kuhn decomposition of the voxel lattice, as stream
// compaction in integers.  The conventions (lattice, tets, vertex and triangle order, winding, ids) are in include/cryovit_hip.h; the
// case table is mesh_tables.h.  Every output index follows from counts and prefix sums in a fixed order and leaves by a plain store, so
// two calls give the same bytes.
//
// THE LATTICE.  The mask labels > 0 gets one layer of background around it.  Cell (cz, cy, cx), 0 <= cz <= D etc., is the cube
// between the padded voxels c + {0,1}^3 (padded p = unpadded p - 1); the voxel with a cell's index is also the lower end of the 7
// edges that cell "owns".  Cells are walked in 4x8x64 tiles like every other volume pass; a wave owns the 64 cells of one row of the
// tile, a SEGMENT: (cz, cy, x-tile).  Segments in (cz, cy, x-tile) order are the raster order of cells and of lower ends, so
//   1. k_mesh_classify: the tile's labels with a one-voxel halo in LDS (6x10x66, the halo_cell layout); per cell the 8 corner bits,
//      from them the active edges of the voxel (7 bits) and the triangles of the 6 tets (0..12); a wave sum each; two int32 per
//      segment into the workspace.
//   2. k_mesh_scan: one workgroup turns both arrays into exclusive prefix sums in segment order (k_ccl_scan's form, four segments per
//      thread) and writes the totals V, T as int64: to the caller, who reads them on the host to size the outputs (the one wait
//      of the op), and behind the workspace, where the emit pass checks them.
//   3. k_mesh_emit: the same tile; a wave recomputes the edge masks of a row and scans them over its lanes: base of the segment +
//      prefix = the index of the voxel's first vertex.  It does so for the 5x9 rows x 65 columns that the tile's triangles can reach
//      (a vertex's lower end is the cell + a tet corner, up to one row, plane or column further; column 64 is lane 0 of the next
//      segment, whose prefix is 0) and keeps base and mask in LDS; vertices of the own 4x8x64 voxels are written on the way.  Then per
//      cell the triangle count, a wave scan, and per tet the case entry (LDS copy of the table): each vertex is base-of-voxel +
//      popcount(mask below the edge type).
// Nothing per voxel is kept between the passes: the workspace is 8 bytes per segment (0.125 bytes per voxel) + 16, and the emit pass
// pays for it by classifying again, from LDS.  No atomics in these three.
//
// The table pass reads triangles; a thread's normal is exact in 128-bit integers (coordinates within +-2^24: differences below 2^25,
// cross products below 2^51, |n|^2 below 2^104) and its root is the double-precision root corrected by integer comparisons.  Thread,
// wave and workgroup combine before the 64-bit integer atomics; the workgroup's stage is a 64-slot table in LDS keyed by id, because
// the triangles of one row of cells change id every few dozen (a row crosses several instances): with only thickness.hip's "a
// wave of one id" stage most waves fell through to global atomics on a few dozen hot rows (30 ms for 9e6 triangles).  The smoothing step accumulates the neighbour sums
// by 64-bit integer atomics (order-independent) and applies them per vertex with a floor division.
#include "entry_checks.h"
#include "mesh_tables.h"

namespace cvx {

constexpr int kMeshScanThreads = 1024, kMeshScanPer = 4;
constexpr int kMeshRows = (TZ + 1) * (TY + 1), kMeshRowLen = TX + 1;  // the voxels whose vertices a tile's triangles use
constexpr long kMeshIndexEnd = 1L << 31;                              // V and T stay below
constexpr int kMeshStatsPer = 16;                                     // triangles per thread of the table pass
constexpr int kMeshSlots = 64;                                        // ids a workgroup of the table pass combines in LDS

__device__ const MeshCases kMeshCases = mesh_cases();

// ids[] = the labels (> 0, else 0) of the padded voxels (z0, y0, x0) + [0,6) x [0,10) x [0,66); z0.. is the tile's first cell
__device__ __forceinline__ void mesh_load_ids(const int* __restrict__ labels, int D, int H, int W, int z0, int y0, int x0, int* ids) {
    for (int c = threadIdx.x; c < kHaloCells; c += kCclThreads) {
        const int x = x0 - 1 + c % kHaloX, y = y0 - 1 + c / kHaloX % kHaloY, z = z0 - 1 + c / (kHaloX * kHaloY);
        const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && (unsigned)z < (unsigned)D;
        const int l = in ? labels[((long)z * H + y) * W + x] : 0;
        ids[c] = l > 0 ? l : 0;
    }
}

// bit (dz << 2 | dy << 1 | dx) = the padded voxel (a + dz, b + dy, c + dx) of the LDS tile is foreground; a <= 4, b <= 8, c <= 64
__device__ __forceinline__ unsigned mesh_cube(const int* ids, int a, int b, int c) {
    const int* p = ids + (a * kHaloY + b) * kHaloX + c;
    unsigned cube = 0;
#pragma unroll
    for (int code = 0; code < 8; ++code)
        cube |= (unsigned)(p[((code >> 2) * kHaloY + (code >> 1 & 1)) * kHaloX + (code & 1)] > 0) << code;
    return cube;
}

// bit e = the edge of type e that starts at the cube's corner 0 joins foreground and background
__device__ __forceinline__ unsigned mesh_edge_mask(unsigned cube) {
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < 7; ++e) m |= ((cube >> kMeshEdgeCode[e] ^ cube) & 1u) << e;
    return m;
}

// bit i = corner i of tet t is foreground
template <int T>
__device__ __forceinline__ unsigned mesh_tet_case(unsigned cube) {
    return (cube >> mesh_tet_corner(T, 0) & 1u) | (cube >> mesh_tet_corner(T, 1) & 1u) << 1 | (cube >> mesh_tet_corner(T, 2) & 1u) << 2 |
           (cube >> mesh_tet_corner(T, 3) & 1u) << 3;
}

__device__ __forceinline__ int mesh_cell_triangles(unsigned cube) {
    return mesh_case_triangles(__popc(mesh_tet_case<0>(cube))) + mesh_case_triangles(__popc(mesh_tet_case<1>(cube))) +
           mesh_case_triangles(__popc(mesh_tet_case<2>(cube))) + mesh_case_triangles(__popc(mesh_tet_case<3>(cube))) +
           mesh_case_triangles(__popc(mesh_tet_case<4>(cube))) + mesh_case_triangles(__popc(mesh_tet_case<5>(cube)));
}

// cd: the extents of the cell lattice (D + 1, H + 1, W + 1) and its tiles
__global__ __launch_bounds__(kCclThreads) void k_mesh_classify(const int* __restrict__ labels, int D, int H, int W, Dims cd,
                                                               int* __restrict__ seg_v, int* __restrict__ seg_t) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    __shared__ int ids[kHaloCells];
    int z0, y0, x0;
    tile_origin(cd, z0, y0, x0);
    mesh_load_ids(labels, D, H, W, z0, y0, x0, ids);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cz = z0 + wave;
    if (cz >= cd.D) return;
    for (int yy = 0; yy < TY && y0 + yy < cd.H; ++yy) {
        // a cell past the lattice along x has only background corners: it counts nothing
        const unsigned cube = mesh_cube(ids, wave, yy, lane);
        const int nv = wave_sum((int)__popc(mesh_edge_mask(cube)));
        const int nt = wave_sum(mesh_cell_triangles(cube));
        if (lane == 0) {
            const long seg = ((long)cz * cd.H + y0 + yy) * cd.tx + x0 / TX;
            seg_v[seg] = nv;
            seg_t[seg] = nt;
        }
    }
}

// a[i] = the sum of a[0..i) for both arrays, in place; totals = the two sums
__global__ __launch_bounds__(kMeshScanThreads) void k_mesh_scan(int* __restrict__ seg_v, int* __restrict__ seg_t, long nseg,
                                                                long long* __restrict__ totals, long long* __restrict__ totals_copy) {
    constexpr int kWaves = kMeshScanThreads / 64;
    __shared__ int wsum_v[kWaves], wsum_t[kWaves];
    const int wave = threadIdx.x >> 6;
    long long carry_v = 0, carry_t = 0;
    for (long base = 0; base < nseg; base += kMeshScanThreads * kMeshScanPer) {
        const long i0 = base + (long)threadIdx.x * kMeshScanPer;
        int v[kMeshScanPer], t[kMeshScanPer], sv = 0, st = 0;
#pragma unroll
        for (int j = 0; j < kMeshScanPer; ++j) {
            v[j] = i0 + j < nseg ? seg_v[i0 + j] : 0;
            t[j] = i0 + j < nseg ? seg_t[i0 + j] : 0;
            sv += v[j];
            st += t[j];
        }
        const int incl_v = wave_scan_incl(sv), incl_t = wave_scan_incl(st);  // below 4096 * 64 * 12
        if ((threadIdx.x & 63) == 63) wsum_v[wave] = incl_v, wsum_t[wave] = incl_t;
        __syncthreads();
        int woff_v = 0, woff_t = 0, total_v = 0, total_t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int a = wsum_v[w], b = wsum_t[w];
            if (w < wave) woff_v += a, woff_t += b;
            total_v += a, total_t += b;
        }
        long long run_v = carry_v + woff_v + incl_v - sv, run_t = carry_t + woff_t + incl_t - st;
#pragma unroll
        for (int j = 0; j < kMeshScanPer; ++j)
            if (i0 + j < nseg) {
                seg_v[i0 + j] = (int)run_v;  // meaningful while the totals stay below 2^31; cvx_mesh_emit refuses the others
                seg_t[i0 + j] = (int)run_t;
                run_v += v[j];
                run_t += t[j];
            }
        carry_v += total_v;
        carry_t += total_t;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        totals[0] = totals_copy[0] = carry_v;
        totals[1] = totals_copy[1] = carry_t;
    }
}

__global__ __launch_bounds__(kCclThreads) void k_mesh_emit(const int* __restrict__ labels, int D, int H, int W, Dims cd,
                                                           const int* __restrict__ seg_v, const int* __restrict__ seg_t,
                                                           const long long* __restrict__ counted, int nv_total, int nt_total,
                                                           int* __restrict__ vertices, int* __restrict__ triangles, int* __restrict__ tri_ids) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    static_assert(kMeshRows <= kCclThreads, "one thread per row for column 64");
    __shared__ int ids[kHaloCells];
    __shared__ int vbase[kMeshRows * kMeshRowLen];
    __shared__ unsigned char vmask[kMeshRows * kMeshRowLen];
    __shared__ unsigned long long cases[6 * 16];
    if (counted[0] != nv_total || counted[1] != nt_total) return;  // the arrays are not of the counted sizes: nothing is written
    int z0, y0, x0;
    tile_origin(cd, z0, y0, x0);
    mesh_load_ids(labels, D, H, W, z0, y0, x0, ids);
    if (threadIdx.x < 6 * 16) cases[threadIdx.x] = kMeshCases.entry[threadIdx.x / 16][threadIdx.x % 16];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xt = x0 / TX;
    // the first vertex and the active edges of the voxels (z0, y0, x0) + [0,5) x [0,9) x [0,65); the own voxels' vertices leave
    for (int r = wave; r < kMeshRows; r += TZ) {
        const int a = r / (TY + 1), b = r % (TY + 1);
        const int cz = z0 + a, cy = y0 + b;
        const bool row = cz < cd.D && cy < cd.H;  // the whole wave alike; a voxel past the lattice has no active edge
        const unsigned mask = row ? mesh_edge_mask(mesh_cube(ids, a, b, lane)) : 0u;
        const int cnt = __popc(mask);
        const int first = (row ? seg_v[((long)cz * cd.H + cy) * cd.tx + xt] : 0) + wave_scan_incl(cnt) - cnt;
        vbase[r * kMeshRowLen + lane] = first;
        vmask[r * kMeshRowLen + lane] = (unsigned char)mask;
        if (a < TZ && b < TY && mask) {
            int slot = first;
            // (a + b) * 128 of the unpadded ends: 2 * (padded - 1) + offset, in 1/256 voxel
            const int pz = 2 * (cz - 1) * 128, py = 2 * (cy - 1) * 128, px = 2 * (x0 + lane - 1) * 128;
#pragma unroll
            for (int e = 0; e < 7; ++e)
                if (mask >> e & 1) {
                    if ((unsigned)slot < (unsigned)nv_total) {  // holds when the workspace is the one cvx_mesh_count left for these labels
                        int* v = vertices + (long)slot * 3;
                        v[0] = pz + (kMeshEdgeCode[e] >> 2) * 128;
                        v[1] = py + (kMeshEdgeCode[e] >> 1 & 1) * 128;
                        v[2] = px + (kMeshEdgeCode[e] & 1) * 128;
                    }
                    ++slot;
                }
        }
    }
    if (threadIdx.x < kMeshRows) {  // column 64: lane 0 of the next segment of the row
        const int r = threadIdx.x, a = r / (TY + 1), b = r % (TY + 1);
        const int cz = z0 + a, cy = y0 + b;
        const bool in = cz < cd.D && cy < cd.H && xt + 1 < cd.tx;
        vbase[r * kMeshRowLen + TX] = in ? seg_v[((long)cz * cd.H + cy) * cd.tx + xt + 1] : 0;
        vmask[r * kMeshRowLen + TX] = in ? (unsigned char)mesh_edge_mask(mesh_cube(ids, a, b, TX)) : 0;
    }
    __syncthreads();
    const int cz = z0 + wave;
    if (cz >= cd.D) return;
    for (int yy = 0; yy < TY && y0 + yy < cd.H; ++yy) {
        const unsigned cube = mesh_cube(ids, wave, yy, lane);
        const int nt = mesh_cell_triangles(cube);
        int slot = seg_t[((long)cz * cd.H + y0 + yy) * cd.tx + xt] + wave_scan_incl(nt) - nt;
        if (nt == 0) continue;
        const int vcell = (wave * (TY + 1) + yy) * kMeshRowLen + lane;  // the cell's corner 0 in vbase / vmask
        const int icell = (wave * kHaloY + yy) * kHaloX + lane;         // and in ids
        // the vertex on the edge `ref` (mesh_vertex_ref) of this cell
        auto vertex = [&](unsigned ref) {
            const int code = ref >> 3 & 7, type = ref & 7;
            const int at = vcell + ((code >> 2) * (TY + 1) + (code >> 1 & 1)) * kMeshRowLen + (code & 1);
            return vbase[at] + __popc(vmask[at] & ((1u << type) - 1));
        };
        auto tet = [&](unsigned m, int t) {
            const unsigned long long e = cases[t * 16 + m];
            const int n = (int)(e & 3);
            if (n == 0) return;
            const int code = (int)(e >> 2 & 7);
            const int id = ids[icell + ((code >> 2) * kHaloY + (code >> 1 & 1)) * kHaloX + (code & 1)];
            for (int j = 0; j < n; ++j) {
                if ((unsigned)slot < (unsigned)nt_total) {
                    int* tri = triangles + (long)slot * 3;
                    tri[0] = vertex((unsigned)(e >> (8 + 18 * j)));
                    tri[1] = vertex((unsigned)(e >> (14 + 18 * j)));
                    tri[2] = vertex((unsigned)(e >> (20 + 18 * j)));
                    tri_ids[slot] = id;
                }
                ++slot;
            }
        };
        tet(mesh_tet_case<0>(cube), 0);
        tet(mesh_tet_case<1>(cube), 1);
        tet(mesh_tet_case<2>(cube), 2);
        tet(mesh_tet_case<3>(cube), 3);
        tet(mesh_tet_case<4>(cube), 4);
        tet(mesh_tet_case<5>(cube), 5);
    }
}

// ---- the per-instance table ----

struct MeshAcc {
    long long n;
    unsigned long long area2, det;
};

// floor(sqrt(v)), v < 2^104: the double-precision root of the nearest double, corrected with integer comparisons
__device__ __forceinline__ unsigned long long mesh_isqrt(unsigned __int128 v) {
    const double d = (double)(unsigned long long)(v >> 64) * 18446744073709551616.0 + (double)(unsigned long long)v;
    unsigned long long r = (unsigned long long)sqrt(d);
    while ((unsigned __int128)r * r > v) --r;
    while ((unsigned __int128)(r + 1) * (r + 1) <= v) ++r;
    return r;
}

__device__ __forceinline__ void mesh_flush(long long* __restrict__ out, int id, const MeshAcc& acc) {
    if (!acc.n) return;
    auto* u = (unsigned long long*)(out + (long)(id - 1) * CVX_MESH_COLS);
    atomicAdd(u + 0, (unsigned long long)acc.n);
    atomicAdd(u + 1, acc.area2);
    atomicAdd(u + 2, acc.det);
}

__global__ __launch_bounds__(kCclThreads) void k_mesh_stats(const int* __restrict__ vertices, const int* __restrict__ triangles,
                                                            const int* __restrict__ tri_ids, long nv, long nt, int k,
                                                            long long* __restrict__ out) {
    // the workgroup's sums per id: a small open-addressed table in LDS, filled by LDS atomics
    __shared__ int slot_id[kMeshSlots];
    __shared__ unsigned long long slot_acc[kMeshSlots * CVX_MESH_COLS];
    if (threadIdx.x < kMeshSlots) slot_id[threadIdx.x] = 0;
    if (threadIdx.x < kMeshSlots * CVX_MESH_COLS) slot_acc[threadIdx.x] = 0;
    __syncthreads();
    // acc joins the slot of its id; when four probes find neither it nor a free one, the global table directly
    auto deposit = [&](int id, const MeshAcc& a) {
        if (!a.n) return;
        const unsigned h = (unsigned)id * 2654435761u >> 26;
        for (int probe = 0; probe < 4; ++probe) {
            const int slot = (h + probe) & (kMeshSlots - 1);
            const int prev = atomicCAS(&slot_id[slot], 0, id);
            if (prev == 0 || prev == id) {
                atomicAdd(&slot_acc[slot * CVX_MESH_COLS + 0], (unsigned long long)a.n);
                atomicAdd(&slot_acc[slot * CVX_MESH_COLS + 1], a.area2);
                atomicAdd(&slot_acc[slot * CVX_MESH_COLS + 2], a.det);
                return;
            }
        }
        mesh_flush(out, id, a);
    };
    const long base = (long)blockIdx.x * (kCclThreads * kMeshStatsPer) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    MeshAcc acc{0, 0, 0};
    int cur = 0;  // the id acc belongs to; 0: none yet
    // a workgroup's triangles are consecutive (coalesced reads) and so, in raster order, of few ids: a thread sums while the id
    // stays the same
    for (int j = 0; j < kMeshStatsPer; ++j) {
        const long i = base + (long)j * kCclThreads;
        if (i >= nt) break;
        const int id = tri_ids[i];
        const long a = triangles[3 * i], b = triangles[3 * i + 1], c = triangles[3 * i + 2];
        if (id < 1 || id > k || (unsigned long)a >= (unsigned long)nv || (unsigned long)b >= (unsigned long)nv ||
            (unsigned long)c >= (unsigned long)nv)
            continue;
        long long p[3][3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) p[0][ax] = vertices[3 * a + ax], p[1][ax] = vertices[3 * b + ax], p[2][ax] = vertices[3 * c + ax];
        const long long uz = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], ux = p[1][2] - p[0][2];
        const long long wz = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wx = p[2][2] - p[0][2];
        const long long nz = uy * wx - ux * wy, ny = ux * wz - uz * wx, nx = uz * wy - uy * wz;
        const unsigned __int128 n2 = (unsigned __int128)((__int128)nz * nz) + (unsigned __int128)((__int128)ny * ny) +
                                     (unsigned __int128)((__int128)nx * nx);
        auto U = [](long long v) { return (unsigned long long)v; };  // the determinant wraps modulo 2^64
        if (id != cur) {
            if (cur) deposit(cur, acc);
            acc = MeshAcc{0, 0, 0};
            cur = id;
        }
        acc.n += 1;
        acc.area2 += mesh_isqrt(n2);
        acc.det += U(p[0][0]) * (U(p[1][1]) * U(p[2][2]) - U(p[1][2]) * U(p[2][1])) +
                   U(p[0][1]) * (U(p[1][2]) * U(p[2][0]) - U(p[1][0]) * U(p[2][2])) +
                   U(p[0][2]) * (U(p[1][0]) * U(p[2][1]) - U(p[1][1]) * U(p[2][0]));
    }
    // the wave: one id among the threads that hold one?  Then lane 0 deposits the wave's sums; else every thread its own
    const int one = wave_single_id(cur);
    if (!one) {
        if (cur) deposit(cur, acc);
    } else {
        acc.n = wave_sum(acc.n);
        acc.area2 = (unsigned long long)wave_sum((long long)acc.area2);
        acc.det = (unsigned long long)wave_sum((long long)acc.det);
        if (lane == 0) deposit(one, acc);
    }
    __syncthreads();
    // the workgroup: one set of 64-bit integer atomics per id it met
    if (threadIdx.x < kMeshSlots && slot_id[threadIdx.x])
        mesh_flush(out, slot_id[threadIdx.x],
                   MeshAcc{(long long)slot_acc[threadIdx.x * CVX_MESH_COLS], slot_acc[threadIdx.x * CVX_MESH_COLS + 1],
                           slot_acc[threadIdx.x * CVX_MESH_COLS + 2]});
}

// ---- one smoothing step ----

// acc[4 * a + 0..2] += the coordinates of b, acc[4 * a + 3] += 1 for every directed edge a -> b
__global__ __launch_bounds__(kCclThreads) void k_mesh_smooth_gather(const int* __restrict__ vertices, const int* __restrict__ triangles,
                                                                    long nv, long nt, unsigned long long* __restrict__ acc) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i >= nt) return;
    const long a = triangles[3 * i], b = triangles[3 * i + 1], c = triangles[3 * i + 2];
    if ((unsigned long)a >= (unsigned long)nv || (unsigned long)b >= (unsigned long)nv || (unsigned long)c >= (unsigned long)nv) return;
    auto edge = [&](long from, long to) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) atomicAdd(acc + 4 * from + ax, (unsigned long long)(long long)vertices[3 * to + ax]);
        atomicAdd(acc + 4 * from + 3, 1ull);
    };
    edge(a, b);
    edge(b, c);
    edge(c, a);
}

// x' = x + floor((S - n x) c / (n 65536)) per axis; a vertex without a neighbour stays
__global__ __launch_bounds__(kCclThreads) void k_mesh_smooth_apply(const int* vin, int* vout, long nv, long long c,  // may be one array
                                                                   const long long* __restrict__ acc) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i >= nv) return;
    const long long n = acc[4 * i + 3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const long long x = vin[3 * i + ax];
        long long step = 0;
        if (n > 0) {
            const long long num = (acc[4 * i + ax] - n * x) * c, den = n * 65536;
            step = num / den;
            if (num % den < 0) --step;  // towards minus infinity
        }
        vout[3 * i + ax] = (int)(x + step);
    }
}

}  // namespace cvx

using namespace cvx;

namespace {

struct MeshLayout {
    long n, nseg, tiles;       // voxels; segments and tiles of the cell lattice
    long off_t, off_totals, bytes;
};

// what every entry refuses about the volume.  nullptr: fine
const char* mesh_extents(int D, int H, int W, MeshLayout& L) {
    if (const char* why = extents_fault(D, H, W, kExtentMax, L.n)) return why;
    const Dims cd = ccl_dims(D + 1, H + 1, W + 1);
    L.nseg = (long)cd.D * cd.H * cd.tx;
    L.tiles = tile_count(cd);
    L.off_t = (L.nseg * (long)sizeof(int) + 15) / 16 * 16;
    L.off_totals = 2 * L.off_t;
    L.bytes = L.off_totals + 2 * (long)sizeof(long long);
    return nullptr;
}

}  // namespace

extern "C" long cvx_mesh_workspace_bytes(int D, int H, int W) {
    MeshLayout L;
    if (mesh_extents(D, H, W, L)) return -1;
    return L.n == 0 ? 2 * (long)sizeof(long long) : L.bytes;
}

extern "C" int cvx_mesh_count(const int32_t* labels, int D, int H, int W, void* workspace, long workspace_bytes, int64_t* totals,
                              hipStream_t st) {
    MeshLayout L;
    if (const char* why = mesh_extents(D, H, W, L)) return cvx_fail("mesh_count", why);
    if (!totals || !workspace || (L.n > 0 && !labels)) return cvx_fail("mesh_count", "null pointer");
    if (((uintptr_t)labels & 3) || ((uintptr_t)totals & 7) || ((uintptr_t)workspace & 15)) return cvx_fail("mesh_count", "misaligned pointer");
    if (workspace_bytes < cvx_mesh_workspace_bytes(D, H, W)) return cvx_fail("mesh_count", "workspace shorter than cvx_mesh_workspace_bytes");
    if (L.n == 0) {  // no voxel, no surface
        CVX_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
        CVX_HIP(hipMemsetAsync(workspace, 0, 2 * sizeof(long long), st));
        return 0;
    }
    int* seg_v = (int*)workspace;
    int* seg_t = (int*)((char*)workspace + L.off_t);
    const Dims cd = ccl_dims(D + 1, H + 1, W + 1);
    hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)L.tiles), dim3(kCclThreads), 0, st, labels, D, H, W, cd, seg_v, seg_t);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMeshScanThreads), 0, st, seg_v, seg_t, L.nseg, (long long*)totals,
                       (long long*)((char*)workspace + L.off_totals));
    return cvx_check_launch();
}

extern "C" int cvx_mesh_emit(const int32_t* labels, int D, int H, int W, const void* workspace, long workspace_bytes, long V, long T,
                             int32_t* vertices, int32_t* triangles, int32_t* ids, hipStream_t st) {
    MeshLayout L;
    if (const char* why = mesh_extents(D, H, W, L)) return cvx_fail("mesh_emit", why);
    if (V < 0 || T < 0) return cvx_fail("mesh_emit", "V or T < 0");
    if (V >= kMeshIndexEnd || T >= kMeshIndexEnd) return cvx_fail("mesh_emit", "V and T must stay below 2^31 (int32 indices)");
    if (!workspace || (L.n > 0 && !labels) || (V > 0 && !vertices) || (T > 0 && (!triangles || !ids))) return cvx_fail("mesh_emit", "null pointer");
    if ((((uintptr_t)labels | (uintptr_t)vertices | (uintptr_t)triangles | (uintptr_t)ids) & 3) || ((uintptr_t)workspace & 15))
        return cvx_fail("mesh_emit", "misaligned pointer");
    if (workspace_bytes < cvx_mesh_workspace_bytes(D, H, W)) return cvx_fail("mesh_emit", "workspace shorter than cvx_mesh_workspace_bytes");
    if (L.n == 0) return (V || T) ? cvx_fail("mesh_emit", "an empty volume has no vertices and no triangles") : 0;
    if (V == 0 && T == 0) return 0;
    const int* seg_v = (const int*)workspace;
    const int* seg_t = (const int*)((const char*)workspace + L.off_t);
    const Dims cd = ccl_dims(D + 1, H + 1, W + 1);
    hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)L.tiles), dim3(kCclThreads), 0, st, labels, D, H, W, cd, seg_v, seg_t,
                       (const long long*)((const char*)workspace + L.off_totals), (int)V, (int)T, vertices, triangles, ids);
    return cvx_check_launch();
}

namespace {

const char* mesh_arrays(const int32_t* vertices, const int32_t* triangles, long V, long T) {
    if (V < 0 || T < 0) return "V or T < 0";
    if (V >= kMeshIndexEnd || T >= kMeshIndexEnd) return "V and T must stay below 2^31 (int32 indices)";
    if ((V > 0 && !vertices) || (T > 0 && !triangles)) return "null pointer";
    if (((uintptr_t)vertices | (uintptr_t)triangles) & 3) return "misaligned pointer";
    return nullptr;
}

}  // namespace

extern "C" int cvx_mesh_stats(const int32_t* vertices, const int32_t* triangles, const int32_t* ids, long V, long T, long k, int64_t* table,
                              hipStream_t st) {
    if (const char* why = mesh_arrays(vertices, triangles, V, T)) return cvx_fail("mesh_stats", why);
    if (k < 0) return cvx_fail("mesh_stats", "k < 0");
    if (!rows_fit(k, CVX_MESH_COLS)) return cvx_fail("mesh_stats", "k rows do not fit in memory");
    if (k == 0) return 0;
    if (!table || (T > 0 && !ids)) return cvx_fail("mesh_stats", "null pointer");
    if (((uintptr_t)table & 7) || ((uintptr_t)ids & 3)) return cvx_fail("mesh_stats", "misaligned pointer");
    CVX_HIP(hipMemsetAsync(table, 0, (size_t)k * CVX_MESH_COLS * sizeof(int64_t), st));
    if (T == 0) return 0;
    hipLaunchKernelGGL(k_mesh_stats, dim3(blocks_of((T + kMeshStatsPer - 1) / kMeshStatsPer)), dim3(kCclThreads), 0, st, vertices, triangles, ids, V, T,
                       clamp_int(k), (long long*)table);
    return cvx_check_launch();
}

extern "C" long cvx_mesh_smooth_workspace_bytes(long V) {
    if (V < 0 || V >= kMeshIndexEnd) return -1;
    return (V > 0 ? V : 1) * 4 * (long)sizeof(long long);
}

extern "C" int cvx_mesh_smooth_step(const int32_t* vertices, int32_t* moved, const int32_t* triangles, long V, long T, int c, void* workspace,
                                    long workspace_bytes, hipStream_t st) {
    if (const char* why = mesh_arrays(vertices, triangles, V, T)) return cvx_fail("mesh_smooth_step", why);
    if (c < -CVX_MESH_FACTOR_MAX || c > CVX_MESH_FACTOR_MAX) return cvx_fail("mesh_smooth_step", "factor outside [-2, 2] (c = factor * 65536)");
    if (V == 0) return 0;
    if (!moved || !workspace) return cvx_fail("mesh_smooth_step", "null pointer");
    if (((uintptr_t)moved & 3) || ((uintptr_t)workspace & 7)) return cvx_fail("mesh_smooth_step", "misaligned pointer");
    if (workspace_bytes < cvx_mesh_smooth_workspace_bytes(V))
        return cvx_fail("mesh_smooth_step", "workspace shorter than cvx_mesh_smooth_workspace_bytes");
    CVX_HIP(hipMemsetAsync(workspace, 0, (size_t)V * 4 * sizeof(long long), st));
    if (T > 0) {
        hipLaunchKernelGGL(k_mesh_smooth_gather, dim3(blocks_of(T)), dim3(kCclThreads), 0, st, vertices, triangles, V, T,
                           (unsigned long long*)workspace);
        if (const int rc = cvx_check_launch()) return rc;
    }
    hipLaunchKernelGGL(k_mesh_smooth_apply, dim3(blocks_of(V)), dim3(kCclThreads), 0, st, vertices, moved, V, (long long)c,
                       (const long long*)workspace);
    return cvx_check_launch();
}
