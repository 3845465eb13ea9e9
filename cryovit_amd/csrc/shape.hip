// Per-instance shape of an int32 label volume (`--shape`): voxel count, first and second coordinate moments, Euler number and
// the boundary crossings along the 13 lattice directions (the discrete Crofton surface estimate is a weighted sum of them, taken
// on the host).  One pass: a workgroup reads a 4x8x64 tile with its one-voxel halo into LDS, every thread takes the 26 "same id"
// bits of its voxels' neighbourhoods from there, and everything a voxel contributes is an integer function of those bits and its
// coordinates.  64-bit integer atomic adds only: the table does not depend on scheduling.
//
// For an instance i everything that is not i is outside: background, other ids, ids outside 1..k, positions beyond the volume.
// A neighbourhood is held as a 27-bit mask m, bit (dz+1)*9 + (dy+1)*3 + (dx+1) set iff v + (dz,dy,dx) is in i (bit 13 = v).  The
// index order is the lexicographic order of (dz,dy,dx) = raster order: bits below 13 are the voxels before v, bits 14..26 the 13
// directions of the crossing counts in the order of the table, N[j] += !bit(14 + j).
//
// EULER NUMBER, CONNECTIVITY 6.  The complex whose cells are the voxels of i, the pairs of face-adjacent voxels, the full 2x2
// squares and the full 2x2x2 cubes is homotopy equivalent to the 6-connected instance, so
//     chi = #voxels - #pairs + #squares - #cubes.
// Each such cell is v + {0,1}^A for one subset A of the axes and one voxel v, its raster-first voxel: v counts the cell for
// A iff all its 2^|A| voxels (offsets >= 0 only) are in i, with sign (-1)^|A|.  Eight mask tests; no cell is seen twice.
//
// EULER NUMBER, CONNECTIVITY 26.  The union of the CLOSED unit cubes of i joins voxels that share a face, an edge or a corner, so
// it is the 26-connected instance.  Its cells are the lattice corners, edges, faces and cubes that touch a voxel of i:
//     chi = #corners - #edges + #faces - #voxels.
// A voxel has 27 cells, one per t in {low, high, spans}^3 (per axis the cell sits on the voxel's low side, on its high side, or
// spans it): 8 corners, 12 edges, 6 faces, itself; sign (-1)^(spanned axes).  The voxels around the cell are v + o with o_a = 0
// on a spanned axis, o_a in {-1, 0} on a low side, {0, 1} on a high side.  The cell is OWNED by the raster-first voxel OF i among
// them (not by the raster-first voxel around it, which may be foreign and would lose it): v counts it iff none of those v + o
// with o before (0,0,0) is in i, i.e. (m & earlier(t)) == 0.  27 mask tests; every cell that touches i has exactly one owner.
//
// EVERY SUM FITS IN int64.  Extents are at most 32768 and an instance has n <= D*H*W <= CVX_COMPONENT_MAX_VOXELS < 2^31 voxels.
// Coordinates are < 2^15: a first moment is < 2^31 * 2^15 = 2^46, a second moment < 2^31 * 2^30 = 2^61.  A voxel adds at most 1
// to a crossing count and between -13 (12 edges and itself) and +13 (8 corners, 6 faces, less itself) to the Euler number, so
// those stay below 2^35 in magnitude.  Negative Euler terms are added as two's complement, which wraps to the signed sum.
//
// COMBINING.  24 global atomics per voxel would make the pass atomic-bound on few large instances.  Integer addition can be
// regrouped freely, so: a thread sums over the 8 voxels it owns while the id stays the same (a change of id sends the finished
// sums straight to the table); a wave whose threads all end on one id (threads without a voxel aside) sums over its lanes; the
// waves of a workgroup that hold the same id are summed through LDS, and the workgroup sends one add per nonzero column and id.  A
// tile inside one instance costs at most 24 atomics.  The threads of a wave that ends on several ids send their own sums.
// Zero terms are never sent.  kShapeCombine = false (timing only) sends every voxel's terms on their own.
#include "entry_checks.h"

namespace cvx {

#ifdef CVX_SHAPE_NO_COMBINE  // the ablation build of tools/bench_shape.py; not an option of the library
constexpr bool kShapeCombine = false;
#else
constexpr bool kShapeCombine = true;
#endif

// columns of a row
constexpr int kColN = 0, kColSum = 1, kColSq = 4, kColEuler = 10, kColCross = 11;

__host__ __device__ constexpr uint32_t nb_bit(int dz, int dy, int dx) { return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1); }

// connectivity 6: the voxels of the cell v + {0,1}^A, A given as one bit per axis (4 = z, 2 = y, 1 = x)
__host__ __device__ constexpr uint32_t cell6_mask(int a) {
    uint32_t m = 0;
    for (int o = 0; o < 8; ++o)
        if ((o & ~a) == 0) m |= nb_bit(o >> 2 & 1, o >> 1 & 1, o & 1);
    return m;
}

// connectivity 26: the voxels BEFORE v around the cell t = (tz, ty, tx) of v; per axis 0 = low side, 1 = high side, 2 = spans
__host__ __device__ constexpr uint32_t cell26_earlier(int tz, int ty, int tx) {
    uint32_t m = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const bool around = (tz == 2 ? dz == 0 : dz == tz - 1 || dz == tz) && (ty == 2 ? dy == 0 : dy == ty - 1 || dy == ty) &&
                                    (tx == 2 ? dx == 0 : dx == tx - 1 || dx == tx);
                const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                if (around && before) m |= nb_bit(dz, dy, dx);
            }
    return m;
}

template <int CONN>
__device__ __forceinline__ int euler_term(uint32_t m) {
    int e = 0;
    if (CONN == 6) {
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const uint32_t cell = cell6_mask(a);
            const int sign = (((a >> 2) + (a >> 1) + a) & 1) ? -1 : 1;
            e += (m & cell) == cell ? sign : 0;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            const int tz = t / 9, ty = t / 3 % 3, tx = t % 3;
            const int sign = (((tz == 2) + (ty == 2) + (tx == 2)) & 1) ? -1 : 1;
            e += (m & cell26_earlier(tz, ty, tx)) == 0 ? sign : 0;
        }
    }
    return e;
}

// acc += what the voxel (z, y, x) with the neighbourhood m adds to its row
template <int CONN>
__device__ __forceinline__ void shape_voxel(uint32_t m, int z, int y, int x, long long (&acc)[CVX_SHAPE_COLS]) {
    acc[kColN] += 1;
    acc[kColSum] += z; acc[kColSum + 1] += y; acc[kColSum + 2] += x;
    acc[kColSq] += z * z; acc[kColSq + 1] += y * y; acc[kColSq + 2] += x * x;  // coordinates < 2^15: products fit in int32
    acc[kColSq + 3] += z * y; acc[kColSq + 4] += z * x; acc[kColSq + 5] += y * x;
    acc[kColEuler] += euler_term<CONN>(m);
#pragma unroll
    for (int j = 0; j < 13; ++j) acc[kColCross + j] += (~m >> (14 + j)) & 1;
}

template <int CONN>
__global__ __launch_bounds__(kCclThreads) void k_shape_stats(const int* __restrict__ labels, long long* __restrict__ out, Dims d, int k) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    __shared__ int ids[kHaloCells];
    __shared__ long long wave_acc[TZ][CVX_SHAPE_COLS];
    __shared__ int wave_id_of[TZ];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    tile_load_ids(labels, d, z0, y0, x0, k, ids);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long acc[CVX_SHAPE_COLS];
#pragma unroll
    for (int c = 0; c < CVX_SHAPE_COLS; ++c) acc[c] = 0;
    int cur = 0;  // the id acc belongs to; 0: none yet
    for (int yy = 0; yy < TY; ++yy) {
        const int c = halo_cell(wave, yy, lane);
        const int id = ids[c];  // 0 outside the volume as well
        if (id == 0) continue;
        if (id != cur) {
            if (cur) table_flush(out, cur, acc);
            cur = id;
        }
        uint32_t m = 0;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
                    if (ids[c + (dz * kHaloY + dy) * kHaloX + dx] == id) m |= nb_bit(dz, dy, dx);
        shape_voxel<CONN>(m, z0 + wave, y0 + yy, x0 + lane, acc);
        if (!kShapeCombine) {
            table_flush(out, cur, acc);
            cur = 0;
        }
    }
    if (!kShapeCombine) return;
    // the wave: one id among the threads that hold one?  Then its sums meet in LDS; else every thread sends its own
    const int one = wave_single_id(cur);
    if (one) {
#pragma unroll
        for (int c = 0; c < CVX_SHAPE_COLS; ++c) {
            const long long s = wave_sum(acc[c]);
            if (lane == 0) wave_acc[wave][c] = s;
        }
    } else if (cur) {
        table_flush(out, cur, acc);
    }
    if (lane == 0) wave_id_of[wave] = one;
    __syncthreads();
    // the workgroup: thread c adds column c of the waves that hold the same id, once per id
    if (threadIdx.x >= CVX_SHAPE_COLS) return;
    for (int w = 0; w < TZ; ++w) {
        if (!first_wave_of_id(wave_id_of, w)) continue;
        const int id = wave_id_of[w];
        long long s = 0;
        for (int u = w; u < TZ; ++u)
            if (wave_id_of[u] == id) s += wave_acc[u][threadIdx.x];
        if (s) atomicAdd((unsigned long long*)(out + (long)(id - 1) * CVX_SHAPE_COLS) + threadIdx.x, (unsigned long long)s);
    }
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_instance_shape_stats(const int32_t* labels, int D, int H, int W, long k, int connectivity, int64_t* out,
                                        hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return cvx_fail("instance_shape_stats", why);
    if (k < 0) return cvx_fail("instance_shape_stats: k < 0");
    if (!rows_fit(k, CVX_SHAPE_COLS)) return cvx_fail("instance_shape_stats: k rows do not fit in memory");
    if (connectivity != 6 && connectivity != 26) return cvx_fail("instance_shape_stats: connectivity must be 6 or 26");
    if (k == 0) return 0;
    if (!out || (n > 0 && !labels)) return cvx_fail("instance_shape_stats: null pointer");
    if (((uintptr_t)out & 7) || ((uintptr_t)labels & 3)) return cvx_fail("instance_shape_stats: misaligned pointer");
    CVX_HIP(hipMemsetAsync(out, 0, (size_t)k * CVX_SHAPE_COLS * sizeof(int64_t), st));
    if (n == 0) return 0;
    const Dims d = ccl_dims(D, H, W);
    const dim3 tiles((unsigned)tile_count(d));
    if (connectivity == 26) hipLaunchKernelGGL(k_shape_stats<26>, tiles, dim3(kCclThreads), 0, st, labels, (long long*)out, d, clamp_int(k));
    else hipLaunchKernelGGL(k_shape_stats<6>, tiles, dim3(kCclThreads), 0, st, labels, (long long*)out, d, clamp_int(k));
    return cvx_check_launch();
}
