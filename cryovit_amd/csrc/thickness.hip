// Local thickness of an int32 distance map (`--thickness`): t2[p] = the largest d2[c] over the centres c whose OPEN ball
// |p - c|^2 < d2[c] holds p (Hildebrand & Ruegsegger; the definition is in include/cryovit_hip.h), and the per-instance table over
// it.  Integers only; a maximum does not depend on the order of its terms, so two calls give the same bits.
//
// THE MAP IS A GATHER PER OUTPUT TILE, NOT A SCATTER PER CENTRE.  The work is the sum of the ball volumes of all foreground
// voxels.  A scatter (one thread per centre, atomicMax into t2 in global memory) sends every one of those terms through the L2
// atomic units, most of them to lose against a value that is already larger, and a wave's 64 balls touch 64 unrelated rows at a
// time.  Here a workgroup owns one 4x8x64 output tile and keeps it in LDS for the whole kernel:
//   1. k_thickness_tilemax writes the largest d2 of every tile, and of the volume, into the workspace.
//   2. k_thickness_map, one workgroup per output tile: the volume's maximum bounds the tiles that can reach it at all; of those
//      it visits the source tiles S whose box distance to its own box is below tilemax(S) (one scalar load and a few scalar
//      operations for a tile that is skipped).  The 256 threads test the 2048 centres of S, one coalesced row per wave and step
//      (squared distance from c to the own box < d2[c]) and queue the ones that reach the tile in LDS (one LDS atomic per wave
//      and row: ballot + prefix count).  When the queue could not take another tile it is drained: a wave takes a queued centre
//      and sweeps the rows of the tile that the ball cuts; a lane reads the cell and issues an LDS atomic max only where the
//      cell is lower (two waves may sweep the same cell).  Balls are small against a 64-wide row, so the sweep folds the lanes
//      to the ball: 8 rows x 8 columns per step up to d2 = 16, 4 x 16 up to 64, 2 x 32 up to 256, one full row beyond; the rows of
//      the LDS tile are 72 words apart so that the folded rows fall into different banks.
//   3. THE FLOOR.  t2 only grows, so a centre whose d2 is at or below the smallest value among the tile's own foreground cells can
//      raise nothing here, and neither can a source tile whose maximum is: after every drain the workgroup takes that minimum
//      (8 LDS reads per thread, a shuffle, four words through LDS) and tests against it.  The own tile is visited first; in the
//      interior of a thick structure the floor starts at the tile's smallest own d2 and most centres around never enter the
//      queue.  Lossless; CVX_THICKNESS_NO_FLOOR (the ablation build of tools/bench_thickness.py) keeps it at 0.
//   4. the tile leaves with plain coalesced stores; background voxels (own d2 == 0) are written as 0.
// No global atomic in the map (one per tile in pass 1, behind a plain read).  A tile without foreground returns after its zeros.
// LDS: 9 KB tile + 30 KB queue (2560 entries of d2, z|y, x) = 39 KB, four workgroups per CU.
//
// ARITHMETIC.  Extents are at most 32768, so a coordinate difference is below 2^15, its square below 2^30 and the sum of three
// below 3 * 2^30 < 2^32: squared distances are compared as uint32 against d2 < 2^31.  CVX_EDT_NONE anywhere (the volume's
// maximum) takes its own path: every nonzero voxel gets CVX_EDT_NONE, nothing is gathered.
//
// The table pass reads labels and t2 directly (no neighbourhood, no halo): a thread sums along y while the id stays the same, then
// table_reduce of voxel_rows.h: a wave whose threads end on one id combines over its lanes, the waves of a workgroup that hold the
// same id combine through LDS, then 64-bit integer atomics.  r_fx = floor(sqrt(t2 << 16)) starts from the double-precision root (t2 << 16 < 2^47 is exact in a
// double) and is corrected with integer comparisons.
#include "entry_checks.h"

namespace cvx {

#ifdef CVX_THICKNESS_NO_FLOOR  // the ablation build of tools/bench_thickness.py; not an option of the library
constexpr bool kThFloor = false;
#else
constexpr bool kThFloor = true;
#endif

constexpr int kThRow = TX + 8;                   // words between two rows of the LDS tile
constexpr int kThCells = TZ * TY * kThRow;
constexpr int kThQueue = 2560;                   // queued centres
constexpr int kThDrainAt = kThQueue - kTileVox;  // above this the next source tile might not fit

// distance along one axis from c, or from [alo, ahi], to [lo, hi]
__device__ __forceinline__ int axis_gap(int c, int lo, int hi) { return c < lo ? lo - c : c > hi ? c - hi : 0; }
__device__ __forceinline__ int box_gap(int alo, int ahi, int lo, int hi) { return ahi < lo ? lo - ahi : alo > hi ? alo - hi : 0; }

__global__ __launch_bounds__(kCclThreads) void k_thickness_tilemax(const int* __restrict__ d2, Dims d, int tiles, int* __restrict__ tilemax) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    __shared__ int wave_max[TZ];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + wave, x = x0 + lane;
    int m = 0;
    if (z < d.D && x < d.W)
        for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) m = max(m, d2[((long)z * d.H + y0 + yy) * d.W + x]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < TZ; ++w) m = max(m, wave_max[w]);
    tilemax[blockIdx.x] = m;
    if (m > *(volatile int*)(tilemax + tiles)) atomicMax(tilemax + tiles, m);  // the volume's; cleared by the caller
}

// the n queued centres into the tile: wave w takes the entries w, w + TZ, ...
__device__ __forceinline__ void thickness_drain(int n, int* best, const int* q_d2, const int* q_zy, const int* q_x, int z0, int y0, int x0,
                                                int lane, int wave) {
    for (int i = wave; i < n; i += TZ) {
        const int r2 = q_d2[i], zy = q_zy[i], cx = q_x[i];
        const int cz = zy >> 16, cy = zy & 0xffff;
        // the ball's x extent is |dx| <= r with r*r < r2: at most 3, 7, 15 for r2 <= 16, 64, 256
        const int sh = r2 <= 16 ? 3 : r2 <= 64 ? 4 : r2 <= 256 ? 5 : 6;
        const int w = 1 << sh, rows = TX >> sh;
        const int yi = lane >> sh;
        const int x = sh == 6 ? lane : cx - (w / 2 - 1) - x0 + (lane & (w - 1));  // within the tile; columns cx - (w/2 - 1) .. cx + w/2
        const bool xin = (unsigned)x < (unsigned)TX;
        const int dx = xin ? x0 + x - cx : 0;
        const unsigned ax = (unsigned)(dx * dx);
        for (int zz = 0; zz < TZ; ++zz) {
            const int dz = z0 + zz - cz;
            const unsigned az = (unsigned)(dz * dz);
            if (az >= (unsigned)r2) continue;
            for (int yg = 0; yg < TY; yg += rows) {
                const int y = yg + yi, dy = y0 + y - cy;
                if (xin && az + (unsigned)(dy * dy) + ax < (unsigned)r2) {
                    int* p = best + (zz * TY + y) * kThRow + x;
                    if (*(volatile int*)p < r2) atomicMax(p, r2);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kCclThreads) void k_thickness_map(const int* __restrict__ d2, const int* __restrict__ tilemax, Dims d, int tiles,
                                                               int* __restrict__ t2) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    static_assert(kThDrainAt > 0, "the queue holds more than one tile");
    __shared__ int best[kThCells];
    __shared__ int q_d2[kThQueue], q_zy[kThQueue], q_x[kThQueue];
    __shared__ int q_n;
    __shared__ int wave_floor[TZ];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + wave, x = x0 + lane;
    const bool column = z < d.D && x < d.W;
    const int gmax = tilemax[tiles];
    unsigned fg = 0;  // bit yy: the own voxel (z, y0 + yy, x) is foreground
    for (int yy = 0; yy < TY; ++yy) {
        const int v = column && y0 + yy < d.H ? d2[((long)z * d.H + y0 + yy) * d.W + x] : 0;
        best[(wave * TY + yy) * kThRow + lane] = v;  // c = p always qualifies
        fg |= (unsigned)(v > 0) << yy;
    }
    if (gmax == CVX_EDT_NONE || tilemax[blockIdx.x] == 0) {  // no distance anywhere, or nothing to measure in this tile
        if (column)
            for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) t2[((long)z * d.H + y0 + yy) * d.W + x] = (fg >> yy & 1) ? CVX_EDT_NONE : 0;
        return;
    }
    // the smallest value among the own foreground cells, in every thread; between two barriers of its own
    auto tile_floor = [&]() {
        int m = INT_MAX;
        for (int yy = 0; yy < TY; ++yy)
            if (fg >> yy & 1) m = min(m, best[(wave * TY + yy) * kThRow + lane]);
        m = wave_min(m);
        if (lane == 0) wave_floor[wave] = m;
        __syncthreads();
        m = wave_floor[0];
        for (int w = 1; w < TZ; ++w) m = min(m, wave_floor[w]);
        __syncthreads();  // wave_floor may be written again
        return kThFloor ? m : 0;  // some cell is foreground (the tile's maximum is not 0), so m is a value of the tile
    };
    if (threadIdx.x == 0) q_n = 0;
    __syncthreads();
    int floor = tile_floor();
    // the own box, and R = the smallest integer with R*R >= gmax: a tile at R or more along one axis reaches nothing here
    const int zl = z0, zh = min(z0 + TZ, d.D) - 1, yl = y0, yh = min(y0 + TY, d.H) - 1, xl = x0, xh = min(x0 + TX, d.W) - 1;
    int R = (int)sqrtf((float)gmax);
    while ((long long)R * R < gmax) ++R;
    while (R > 1 && (long long)(R - 1) * (R - 1) >= gmax) --R;
    const int sz_lo = max(0, zl - R + 1) / TZ, sz_hi = min(d.D - 1, zh + R - 1) / TZ;
    const int sy_lo = max(0, yl - R + 1) / TY, sy_hi = min(d.H - 1, yh + R - 1) / TY;
    const int sx_lo = max(0, xl - R + 1) / TX, sx_hi = min(d.W - 1, xh + R - 1) / TX;
    // the centres of the source tile (sz, sy, sx) that reach the own box and lie above the floor join the queue
    auto visit = [&](int sz, int sy, int sx) {
        const int gz = box_gap(sz * TZ, min(sz * TZ + TZ, d.D) - 1, zl, zh);
        const int gy = box_gap(sy * TY, min(sy * TY + TY, d.H) - 1, yl, yh);
        const int gx = box_gap(sx * TX, min(sx * TX + TX, d.W) - 1, xl, xh);
        const unsigned reach = (unsigned)tilemax[((long)sz * d.ty + sy) * d.tx + sx];
        if ((unsigned)(gz * gz) + (unsigned)(gy * gy) + (unsigned)(gx * gx) >= reach || reach <= (unsigned)floor) return;  // the whole workgroup alike
        const int cz = sz * TZ + wave, cx = sx * TX + lane;
        const int az = axis_gap(cz, zl, zh), ax = axis_gap(cx, xl, xh);
        const unsigned azx = (unsigned)(az * az) + (unsigned)(ax * ax);
        for (int yy = 0; yy < TY; ++yy) {
            const int cy = sy * TY + yy;
            const bool in = cz < d.D && cx < d.W && cy < d.H;
            const int v = in ? d2[((long)cz * d.H + cy) * d.W + cx] : 0;
            const int ay = axis_gap(cy, yl, yh);
            const bool hit = v > floor && azx + (unsigned)(ay * ay) < (unsigned)v;  // floor >= 0
            const unsigned long long hits = __ballot(hit);
            if (hits == 0) continue;  // the whole wave alike
            int base = 0;
            if (lane == 0) base = atomicAdd(&q_n, __popcll(hits));
            base = __shfl(base, 0);
            if (hit) {
                const int slot = base + __popcll(hits & ((1ull << lane) - 1));  // < kThQueue: q_n <= kThDrainAt before this tile
                q_d2[slot] = v;
                q_zy[slot] = cz << 16 | cy;
                q_x[slot] = cx;
            }
        }
        __syncthreads();
        const int n = q_n;
        __syncthreads();  // everybody has read q_n before anybody adds to it again
        if (n > kThDrainAt) {
            if (threadIdx.x == 0) q_n = 0;
            thickness_drain(n, best, q_d2, q_zy, q_x, z0, y0, x0, lane, wave);
            __syncthreads();
            floor = tile_floor();
        }
    };
    const int oz = z0 / TZ, oy = y0 / TY, ox = x0 / TX;
    visit(oz, oy, ox);  // the own tile first: it raises the floor most
    for (int sz = sz_lo; sz <= sz_hi; ++sz)
        for (int sy = sy_lo; sy <= sy_hi; ++sy)
            for (int sx = sx_lo; sx <= sx_hi; ++sx)
                if (sz != oz || sy != oy || sx != ox) visit(sz, sy, sx);
    thickness_drain(q_n, best, q_d2, q_zy, q_x, z0, y0, x0, lane, wave);  // q_n: stable since the last barrier
    __syncthreads();
    if (column)
        for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy)
            t2[((long)z * d.H + y0 + yy) * d.W + x] = (fg >> yy & 1) ? best[(wave * TY + yy) * kThRow + lane] : 0;
}

// ---- the per-instance table ----

__global__ __launch_bounds__(kCclThreads) void k_thickness_stats_init(long long* __restrict__ out, long cells) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < cells) out[i] = i % CVX_THICKNESS_COLS < 3 ? 0 : -1;  // -1 is also the largest uint64: the minimum is taken unsigned
}

struct ThAcc {
    long long n, sum_t2, sum_r;
    int lo, hi;
    __device__ void wave_combine() {
        n = wave_sum(n), sum_t2 = wave_sum(sum_t2), sum_r = wave_sum(sum_r);
        lo = wave_min(lo), hi = wave_max(hi);
    }
    __device__ void merge(const ThAcc& a) {
        n += a.n, sum_t2 += a.sum_t2, sum_r += a.sum_r;
        lo = min(lo, a.lo), hi = max(hi, a.hi);
    }
};
constexpr ThAcc kThEmpty{0, 0, 0, INT_MAX, -1};

// floor(sqrt(t << 16)) = floor(256 sqrt t), 0 < t < 2^31
__device__ __forceinline__ long long thickness_r_fx(int t) {
    const long long v = (long long)t << 16;
    long long r = (long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// acc goes to row id - 1; acc = empty
__device__ __forceinline__ void thickness_flush(long long* __restrict__ out, int id, ThAcc& acc) {
    if (acc.n) {
        long long* row = out + (long)(id - 1) * CVX_THICKNESS_COLS;
        auto* u = (unsigned long long*)row;
        atomicAdd(u + 0, (unsigned long long)acc.n);
        atomicAdd(u + 1, (unsigned long long)acc.sum_t2);
        atomicAdd(u + 2, (unsigned long long)acc.sum_r);
        if ((unsigned long long)acc.lo < *(volatile unsigned long long*)(u + 3)) atomicMin(u + 3, (unsigned long long)acc.lo);
        table_max(row + 4, acc.hi);
    }
    acc = kThEmpty;
}

__global__ __launch_bounds__(kCclThreads) void k_thickness_stats(const int* __restrict__ labels, const int* __restrict__ t2,
                                                                 long long* __restrict__ out, Dims d, int k) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + wave, x = x0 + lane;
    ThAcc acc = kThEmpty;
    int cur = 0;  // the id acc belongs to; 0: none yet
    if (z < d.D && x < d.W)
        for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) {
            const long v = ((long)z * d.H + y0 + yy) * d.W + x;
            const int id = labels[v];
            if (id < 1 || id > k) continue;
            const int t = t2[v];
            if (t <= 0 || t == CVX_EDT_NONE) continue;
            if (id != cur) {
                if (cur) thickness_flush(out, cur, acc);
                cur = id;
            }
            acc.n += 1;
            acc.sum_t2 += t;
            acc.sum_r += thickness_r_fx(t);
            acc.lo = min(acc.lo, t);
            acc.hi = max(acc.hi, t);
        }
    table_reduce(acc, cur, [&](int id, ThAcc& a) { thickness_flush(out, id, a); });
}

}  // namespace cvx

using namespace cvx;

namespace {

// what every entry refuses about the volume; n = the voxel count, tiles = its 4x8x64 tiles (<= n).  nullptr: fine
const char* thickness_extents(int D, int H, int W, long& n, long& tiles) {
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return why;
    tiles = tile_count(ccl_dims(D, H, W));
    return nullptr;
}

}  // namespace

extern "C" long cvx_local_thickness_workspace_bytes(int D, int H, int W) {
    long n = 0, tiles = 0;
    if (thickness_extents(D, H, W, n, tiles)) return -1;
    return (tiles + 1) * (long)sizeof(int);
}

extern "C" int cvx_local_thickness_squared(const int32_t* d2, int D, int H, int W, int32_t* t2, void* workspace, long workspace_bytes,
                                           hipStream_t st) {
    long n = 0, tiles = 0;
    if (const char* why = thickness_extents(D, H, W, n, tiles)) return cvx_fail("local_thickness_squared", why);
    if (n == 0) return 0;
    if (!d2 || !t2 || !workspace) return cvx_fail("local_thickness_squared", "null pointer");
    if (((uintptr_t)d2 | (uintptr_t)t2 | (uintptr_t)workspace) & 3) return cvx_fail("local_thickness_squared", "misaligned pointer");
    if (workspace_bytes < (tiles + 1) * (long)sizeof(int))
        return cvx_fail("local_thickness_squared", "workspace shorter than cvx_local_thickness_workspace_bytes");
    if (d2 == t2) return cvx_fail("local_thickness_squared", "d2 and t2 must be different arrays");
    int* tilemax = (int*)workspace;
    const Dims d = ccl_dims(D, H, W);
    CVX_HIP(hipMemsetAsync(tilemax + tiles, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_thickness_tilemax, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, d2, d, (int)tiles, tilemax);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_thickness_map, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, d2, tilemax, d, (int)tiles, t2);
    return cvx_check_launch();
}

extern "C" int cvx_instance_thickness_stats(const int32_t* labels, const int32_t* t2, int D, int H, int W, long k, int64_t* table,
                                            hipStream_t st) {
    long n = 0, tiles = 0;
    if (const char* why = thickness_extents(D, H, W, n, tiles)) return cvx_fail("instance_thickness_stats", why);
    if (k < 0) return cvx_fail("instance_thickness_stats", "k < 0");
    if (!rows_fit(k, CVX_THICKNESS_COLS)) return cvx_fail("instance_thickness_stats", "k rows do not fit in memory");
    if (k == 0) return 0;
    if (!table || (n > 0 && (!labels || !t2))) return cvx_fail("instance_thickness_stats", "null pointer");
    if (((uintptr_t)table & 7) || (((uintptr_t)labels | (uintptr_t)t2) & 3)) return cvx_fail("instance_thickness_stats", "misaligned pointer");
    const long cells = k * CVX_THICKNESS_COLS;
    if ((cells + kCclThreads - 1) / kCclThreads > INT_MAX) return cvx_fail("instance_thickness_stats", "k rows do not fit in one launch");
    hipLaunchKernelGGL(k_thickness_stats_init, dim3(blocks_of(cells)), dim3(kCclThreads), 0, st, (long long*)table, cells);
    if (const int rc = cvx_check_launch()) return rc;
    if (n == 0) return 0;
    const Dims d = ccl_dims(D, H, W);
    hipLaunchKernelGGL(k_thickness_stats, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, labels, t2, (long long*)table, d, clamp_int(k));
    return cvx_check_launch();
}
