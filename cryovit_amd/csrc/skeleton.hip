// Centreline skeletons of the instances of an int32 label volume (`--skeleton`): topology-preserving thinning in the order of
// the distance map, and the per-instance table of what remains.  The definition is in include/cryovit_hip.h; in short: a voxel is
// deleted when it is alive, its d2 is at most the level's, it is a (26,6) simple point of ITS OWN instance (everything that is
// not its id is outside) and it is no protected end (exactly one neighbour, d2 >= end_d2).  A cycle is eight passes, one per
// parity subfield ((z&1)<<2 | (y&1)<<1 | (x&1)); the caller repeats cycles until one deletes nothing, level by level.
//
// ONE PASS, IN PLACE, NO RACE.  Two voxels of one subfield differ by an even amount along every axis, so they are never
// 26-adjacent, and a decision reads the voxel and its 26 neighbours only: nothing a decision of this pass reads is written by
// this pass.  Every thread may therefore clear its own voxel in `alive` directly, and the pass equals deleting the same voxels
// one after another in any order.  Passes are separate launches on one stream.
//
// LAYOUT: DIRECT READS, NO TILE.  Only one voxel in eight can act in a pass, and of those only the alive ones at or below the
// level: a thin shell.  So a thread takes one voxel OF THE SUBFIELD (lanes along x: 64 lanes read 128 consecutive words, every
// other one used), reads its own id and d2 (a quarter of the rows of each volume are touched at all), and only a candidate reads
// its neighbours (the six by a face first, the other twenty unless all six are set), from global memory through the caches.
// A 4x8x64 tile with halo in LDS, as shape.hip has it, would load 3960 words and pass a barrier for 256 possible actors, most of
// them rejected by their own two words.  No LDS, no barrier.
//
// The table pass (k_skeleton_stats) looks at every voxel, so it does use the tile with halo of voxel_rows.h, and combines like
// shape.hip: a thread sums along y while the id stays the same, a wave whose threads end on one id sums over its lanes and
// lane 0 sends the nonzero columns; other threads send their own.  Integer atomic adds only: two calls give the same bits.
#include "entry_checks.h"
#include "skeleton_masks.h"

namespace cvx {

__global__ __launch_bounds__(kCclThreads) void k_skeleton_init(const int* __restrict__ labels, long n, int k, int* __restrict__ alive) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= n) return;
    const int l = labels[v];
    alive[v] = l >= 1 && l <= k ? l : 0;
}

// the voxels of subfield `sub`: (nz, ny, nx) of them per axis, thread t <-> (zi, yi, xi), xi fastest
struct SubGrid {
    int nz, ny, nx;
    int sz, sy, sx;
};

__global__ __launch_bounds__(kCclThreads) void k_skeleton_pass(int* alive, const int* __restrict__ d2, int D, int H, int W, int k, int level_d2,
                                                               int end_d2, SubGrid g, int* __restrict__ changed) {
    const long t = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (t >= (long)g.nz * g.ny * g.nx) return;
    const int x = 2 * (int)(t % g.nx) + g.sx, y = 2 * (int)(t / g.nx % g.ny) + g.sy, z = 2 * (int)(t / g.nx / g.ny) + g.sz;
    const long v = ((long)z * H + y) * W + x;
    const int id = alive[v];
    if (id < 1 || id > k) return;
    const int dist = d2[v];
    if (dist > level_d2 || dist == CVX_EDT_NONE) return;
    // the six face neighbours first: a voxel inside its instance (all six set) is rejected after 6 reads, not 26
    uint32_t m = 0;
#pragma unroll
    for (int part = 0; part < 2; ++part) {
#pragma unroll
        for (int b = 0; b < 27; ++b) {
            if (b == kSkCentre || (sk_kind(b) == 1) != (part == 0)) continue;
            const int dz = sk_dz(b), dy = sk_dy(b), dx = sk_dx(b);
            const bool in = (unsigned)(z + dz) < (unsigned)D && (unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W;
            if (in && alive[v + ((long)dz * H + dy) * W + dx] == id) m |= 1u << b;
        }
        if (part == 0 && m == kSkN6) return;  // no way out by a face: not simple
    }
    if (m == 0) return;                                         // nothing to stay connected to: not simple
    if ((m & (m - 1)) == 0 && dist >= end_d2) return;           // a protected end
    if (!sk_simple(m)) return;
    alive[v] = 0;
    *changed = 1;  // every writer stores the same value
}

// the later directions (bits 14..26) by kind
constexpr uint32_t kSkLater = ~((2u << kSkCentre) - 1u);
constexpr uint32_t kSkLaterFace = kSkN6 & kSkLater, kSkLaterEdge = kSkN18 & ~kSkN6 & kSkLater, kSkLaterCorner = kSkN26 & ~kSkN18 & kSkLater;

__global__ __launch_bounds__(kCclThreads) void k_skeleton_stats(const int* __restrict__ alive, const int* __restrict__ d2,
                                                                long long* __restrict__ out, Dims d, int k) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    __shared__ int ids[kHaloCells];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    tile_load_ids(alive, d, z0, y0, x0, k, ids);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long acc[CVX_SKELETON_COLS];
#pragma unroll
    for (int c = 0; c < CVX_SKELETON_COLS; ++c) acc[c] = 0;
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
        for (int b = 0; b < 27; ++b)
            if (b != kSkCentre && ids[c + (sk_dz(b) * kHaloY + sk_dy(b)) * kHaloX + sk_dx(b)] == id) m |= 1u << b;
        const int degree = __popc(m);
        const int dist = d2[((long)(z0 + wave) * d.H + y0 + yy) * d.W + x0 + lane];  // id != 0: inside the volume
        acc[0] += 1;
        acc[1] += degree == 1;
        acc[2] += degree >= 3;
        acc[3] += degree == 0;
        acc[4] += __popc(m & kSkLaterFace);  // a link is counted at its raster-first voxel
        acc[5] += __popc(m & kSkLaterEdge);
        acc[6] += __popc(m & kSkLaterCorner);
        acc[7] += dist == CVX_EDT_NONE ? 0 : dist;
    }
    // the wave: one id among the threads that hold one?  Then lane 0 sends the wave's sums; else every thread sends its own
    const int one = wave_single_id(cur);
    if (!one) {
        if (cur) table_flush(out, cur, acc);
        return;
    }
#pragma unroll
    for (int c = 0; c < CVX_SKELETON_COLS; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) table_flush(out, one, acc);
}

}  // namespace cvx

using namespace cvx;

namespace {

// what every entry refuses about the volume and its id count; n = the voxel count.  nullptr: fine
const char* skeleton_extents(int D, int H, int W, long k, long& n) {
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return why;
    return k < 0 ? "k < 0" : nullptr;
}

}  // namespace

extern "C" int cvx_skeleton_init(const int32_t* labels, int D, int H, int W, long k, int32_t* alive, hipStream_t st) {
    long n = 0;
    if (const char* why = skeleton_extents(D, H, W, k, n)) return cvx_fail("skeleton_init", why);
    if (n == 0) return 0;
    if (!labels || !alive) return cvx_fail("skeleton_init", "null pointer");
    if (((uintptr_t)labels | (uintptr_t)alive) & 3) return cvx_fail("skeleton_init", "misaligned pointer");
    hipLaunchKernelGGL(k_skeleton_init, dim3(blocks_of(n)), dim3(kCclThreads), 0, st, labels, n, clamp_int(k), alive);
    return cvx_check_launch();
}

extern "C" int cvx_skeleton_cycles(int32_t* alive, const int32_t* d2, int D, int H, int W, long k, int level_d2, int end_d2, int cycles,
                                   int32_t* changed, hipStream_t st) {
    long n = 0;
    if (const char* why = skeleton_extents(D, H, W, k, n)) return cvx_fail("skeleton_cycles", why);
    if (end_d2 < 1) return cvx_fail("skeleton_cycles", "end_d2 < 1");
    if (level_d2 < 0) return cvx_fail("skeleton_cycles", "level_d2 < 0");
    if (cycles < 1) return cvx_fail("skeleton_cycles", "cycles < 1");
    if (!changed || (n > 0 && (!alive || !d2))) return cvx_fail("skeleton_cycles", "null pointer");
    if (((uintptr_t)alive | (uintptr_t)d2 | (uintptr_t)changed) & 3) return cvx_fail("skeleton_cycles", "misaligned pointer");
    CVX_HIP(hipMemsetAsync(changed, 0, (size_t)cycles * sizeof(int), st));
    if (n == 0 || k == 0) return 0;
    for (int c = 0; c < cycles; ++c)
        for (int sub = 0; sub < 8; ++sub) {
            SubGrid g;
            g.sz = sub >> 2 & 1, g.sy = sub >> 1 & 1, g.sx = sub & 1;
            g.nz = (D - g.sz + 1) / 2, g.ny = (H - g.sy + 1) / 2, g.nx = (W - g.sx + 1) / 2;  // the coordinates of that parity below the extent
            const long count = (long)g.nz * g.ny * g.nx;
            if (count == 0) continue;
            hipLaunchKernelGGL(k_skeleton_pass, dim3(blocks_of(count)), dim3(kCclThreads), 0, st, alive, d2, D, H,
                               W, clamp_int(k), level_d2, end_d2, g, changed + c);
            const int rc = cvx_check_launch();
            if (rc) return rc;
        }
    return 0;
}

extern "C" int cvx_skeleton_stats(const int32_t* alive, const int32_t* d2, int D, int H, int W, long k, int64_t* table, hipStream_t st) {
    long n = 0;
    if (const char* why = skeleton_extents(D, H, W, k, n)) return cvx_fail("skeleton_stats", why);
    if (!rows_fit(k, CVX_SKELETON_COLS)) return cvx_fail("skeleton_stats", "k rows do not fit in memory");
    if (k == 0) return 0;
    if (!table || (n > 0 && (!alive || !d2))) return cvx_fail("skeleton_stats", "null pointer");
    if (((uintptr_t)table & 7) || (((uintptr_t)alive | (uintptr_t)d2) & 3)) return cvx_fail("skeleton_stats", "misaligned pointer");
    CVX_HIP(hipMemsetAsync(table, 0, (size_t)k * CVX_SKELETON_COLS * sizeof(int64_t), st));
    if (n == 0) return 0;
    const Dims d = ccl_dims(D, H, W);
    hipLaunchKernelGGL(k_skeleton_stats, dim3((unsigned)tile_count(d)), dim3(kCclThreads), 0, st, alive, d2, (long long*)table, d, clamp_int(k));
    return cvx_check_launch();
}
