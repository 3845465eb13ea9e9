// Pieces shared by the passes over an int32 [D][H][W] volume that build a per-instance table.  For the passes that walk it in
// 16-voxel row pieces (components.hip, split.hip, cleanup.hip, the reductions of edt.hip and nearest.hip): the piece a thread owns, its 16-B
// loads / stores, the kernel that fills a component table with the empty box, and the integer add / min / max into a table row.
// For the passes that walk it in 4x8x64 tiles (shape.hip, skeleton.hip, thickness.hip, mesh.hip, cleanup.hip, curvature.hip): a tile's ids with their
// one-voxel halo in LDS, and the stages of the per-id reduction: a thread's sums to a table row (table_flush), the wave's
// single-id test (wave_single_id), the first wave of a workgroup that holds an id (first_wave_of_id), and for a row that is more
// than sums (thickness.hip, curvature.hip: sums with a min and a max) the wave and workgroup stages as a whole, over the pass's own
// accumulator struct and flush (table_reduce).  shape.hip (columns combined in parallel), skeleton.hip and cleanup.hip's added
// voxels (they stop at the wave) and mesh.hip (an LDS hash) keep their own stages on purpose.  And the sums, the min / max and the
// scan over the lanes of a wave.  The bit-packed volumes of cleanup.hip, curvature.hip and picks.hip are in bit_rows.h.  Device
// code only; every includer compiles its own copy.
#pragma once
#include "common.h"
#include "../../include/cryovit_hip.h"

namespace cvx {

constexpr int kCclThreads = 256;
constexpr int TZ = 4, TY = 8, TX = 64;  // tile: one wave reads 64 B of one mask row; 2048 labels = 8 KB of LDS
constexpr int kTileVox = TZ * TY * TX;
constexpr int kPerThread = kTileVox / kCclThreads;
constexpr int RV = 16;                  // voxels of one row per thread in the run-combining passes

struct Dims {
    int D, H, W;
    int tx, ty;  // tiles along x and y
};

inline Dims ccl_dims(int D, int H, int W) { return Dims{D, H, W, (W + TX - 1) / TX, (H + TY - 1) / TY}; }

__device__ __forceinline__ void tile_origin(const Dims& d, int& z0, int& y0, int& x0) {
    const int b = blockIdx.x;
    x0 = (b % d.tx) * TX;
    y0 = (b / d.tx % d.ty) * TY;
    z0 = (b / d.tx / d.ty) * TZ;
}

// v[0..cnt) = p[0..cnt): 16-B accesses for a full, 16-B aligned group, element accesses otherwise
__device__ __forceinline__ void row_load(const int* __restrict__ p, int cnt, int (&v)[RV]) {
    if (cnt == RV && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < RV / 4; ++q) {
            const int4 f = ((const int4*)p)[q];
            v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < RV; ++i) v[i] = i < cnt ? p[i] : 0;
    }
}
__device__ __forceinline__ void row_store(int* __restrict__ p, int cnt, const int (&v)[RV]) {
    if (cnt == RV && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < RV / 4; ++q) ((int4*)p)[q] = int4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    } else {
#pragma unroll
        for (int i = 0; i < RV; ++i)
            if (i < cnt) p[i] = v[i];
    }
}

// thread -> RV voxels of one row: x0 .. x0 + cnt of row z * H + y, whose first voxel is row * W; false past the volume
__device__ __forceinline__ bool row_piece(const Dims& d, int segs, long& row, int& x0, int& cnt) {
    const long t = (long)blockIdx.x * kCclThreads + threadIdx.x;
    row = t / segs;
    if (row >= (long)d.D * d.H) return false;
    x0 = (int)(t % segs) * RV;
    cnt = min(RV, d.W - x0);
    return true;
}
__device__ __forceinline__ bool row_piece(const Dims& d, int segs, int& z, int& y, int& x0, int& cnt) {
    long row;
    if (!row_piece(d, segs, row, x0, cnt)) return false;
    y = (int)(row % d.H);
    z = (int)(row / d.H);
    return true;
}

// the value a table entry starts from: counts and sums 0, lower bounds past the volume, upper bounds -1 (the empty box)
__device__ __forceinline__ long long table_empty(int col, const Dims& d) {
    return col < 4 ? 0 : col == 4 ? d.D : col == 6 ? d.H : col == 8 ? d.W : -1;
}

// min / max into a table entry; the plain read first skips the atomic when it cannot change anything (entries move one way
// only, so a stale read errs towards issuing the atomic)
__device__ __forceinline__ void table_min(long long* p, long long v) {
    if (v < *(volatile long long*)p) atomicMin(p, v);
}
__device__ __forceinline__ void table_max(long long* p, long long v) {
    if (v > *(volatile long long*)p) atomicMax(p, v);
}

// the rows of a component table start as the empty box
template <int COLS>
__global__ __launch_bounds__(kCclThreads) void k_table_init(long long* __restrict__ table, long k, Dims d) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < k * COLS) table[i] = table_empty((int)(i % COLS), d);
}

__device__ __forceinline__ void table_add_run(long long* __restrict__ table, int id, int z, int y, int xa, int xb) {
    long long* row = table + (long)(id - 1) * CVX_COMPONENT_COLS;
    const unsigned long long m = (unsigned long long)(xb - xa + 1);
    auto* u = (unsigned long long*)row;
    atomicAdd(u + 0, m);
    atomicAdd(u + 1, m * (unsigned long long)z);
    atomicAdd(u + 2, m * (unsigned long long)y);
    atomicAdd(u + 3, m * (unsigned long long)(xa + xb) / 2);  // xa + ... + xb
    table_min(row + 4, z); table_max(row + 5, z);
    table_min(row + 6, y); table_max(row + 7, y);
    table_min(row + 8, xa); table_max(row + 9, xb);
}

// the table rows of the runs of one id along a thread's row piece (id 0 = background)
__device__ __forceinline__ void table_add_piece(long long* __restrict__ table, const int (&id)[RV], int z, int y, int x0, int cnt) {
    int cur = 0, xa = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        const int c = i < cnt ? id[i] : 0;
        if (c != cur) {
            if (cur) table_add_run(table, cur, z, y, xa, x0 + i - 1);
            cur = c;
            xa = x0 + i;
        }
    }
    if (cur) table_add_run(table, cur, z, y, xa, x0 + cnt - 1);
}

// ---- a tile with its one-voxel halo in LDS (shape.hip; any pass that reads a voxel's 3x3x3 neighbourhood) ----

constexpr int kHaloZ = TZ + 2, kHaloY = TY + 2, kHaloX = TX + 2;
constexpr int kHaloCells = kHaloZ * kHaloY * kHaloX;  // 3960 int32 = 15.5 KB

// the LDS cell of the tile's own voxel (z, y, x), 0 <= z < TZ etc.; a neighbour is at + (dz * kHaloY + dy) * kHaloX + dx
__device__ __forceinline__ int halo_cell(int z, int y, int x) { return ((z + 1) * kHaloY + y + 1) * kHaloX + x + 1; }

// ids[kHaloCells] = the labels of the tile at (z0, y0, x0) and of the voxels around it; a value outside 1..k and a cell outside
// the volume read 0 (nobody's).  Global reads stay inside the volume.  The caller synchronises before it reads ids.
__device__ __forceinline__ void tile_load_ids(const int* __restrict__ labels, const Dims& d, int z0, int y0, int x0, int k, int* ids) {
    for (int c = threadIdx.x; c < kHaloCells; c += kCclThreads) {
        const int x = x0 - 1 + c % kHaloX, y = y0 - 1 + c / kHaloX % kHaloY, z = z0 - 1 + c / (kHaloX * kHaloY);
        const bool in = (unsigned)x < (unsigned)d.W && (unsigned)y < (unsigned)d.H && (unsigned)z < (unsigned)d.D;
        const int l = in ? labels[((long)z * d.H + y) * d.W + x] : 0;
        ids[c] = l >= 1 && l <= k ? l : 0;
    }
}

// ---- over the lanes of a wave (all 64 call these) ----

// the sum of v, in every lane
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the smallest / largest v, in every lane
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// the sum of v over this lane and the lanes below it
__device__ __forceinline__ int wave_scan_incl(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// ---- the per-id reduction of the tile passes: thread, wave, workgroup ----

// the nonzero sums of acc go to row id - 1 of a table of COLS columns; acc = 0
template <int COLS>
__device__ __forceinline__ void table_flush(long long* __restrict__ out, int id, long long (&acc)[COLS]) {
    auto* row = (unsigned long long*)(out + (long)(id - 1) * COLS);
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        if (acc[c]) atomicAdd(row + c, (unsigned long long)acc[c]);
        acc[c] = 0;
    }
}

// cur = the id a thread's sums belong to, 0: it has none.  The id, when every lane that holds one holds the same; else 0
__device__ __forceinline__ int wave_single_id(int cur) {
    const unsigned long long has = __ballot(cur != 0);
    const int first = has ? __shfl(cur, __ffsll((long long)has) - 1) : 0;
    return __all(cur == 0 || cur == first) ? first : 0;
}

// ids[w] = the single id of wave w of the workgroup (0: none).  Is w the first wave that holds its id?
__device__ __forceinline__ bool first_wave_of_id(const int* ids, int w) {
    bool first = ids[w] != 0;
    for (int u = 0; u < w; ++u) first &= ids[u] != ids[w];
    return first;
}

// The wave and workgroup stages for a table whose row is not plain sums (thickness.hip, curvature.hip: sums with a min and a max).
// acc = a thread's accumulator, cur = the id it belongs to (0: none).  Acc::wave_combine() leaves the wave's in every lane,
// Acc::merge(a) takes in another wave's, flush(id, acc) sends one to row id - 1.  A wave whose threads hold one id combines over
// its lanes, else every thread flushes its own; thread 0 then merges the waves of the workgroup that hold the same id and flushes
// once per id.  Every thread of the workgroup calls it, once.
template <class Acc, class Flush>
__device__ __forceinline__ void table_reduce(Acc& acc, int cur, Flush flush) {
    static_assert(kCclThreads == TZ * 64, "TZ waves");
    __shared__ Acc wave_acc[TZ];
    __shared__ int wave_id_of[TZ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int one = wave_single_id(cur);
    if (!one) {
        if (cur) flush(cur, acc);
    } else {
        acc.wave_combine();
        if (lane == 0) wave_acc[wave] = acc;
    }
    if (lane == 0) wave_id_of[wave] = one;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 0; w < TZ; ++w) {
        if (!first_wave_of_id(wave_id_of, w)) continue;
        const int id = wave_id_of[w];
        Acc s = wave_acc[w];
        for (int u = w + 1; u < TZ; ++u)
            if (wave_id_of[u] == id) s.merge(wave_acc[u]);
        flush(id, s);
    }
}

}  // namespace cvx
