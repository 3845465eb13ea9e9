// Scoring a predicted mask at its boundary (`cryovit evaluate --boundary`: HD95, surface distance, surface Dice): which z-slices
// of a sparse label volume are annotated, the surface voxels of a mask, and the histogram of a distance map sampled at surface
// voxels, from which the host takes percentiles, means and tolerance counts.  edt.hip makes the distance maps.  Integers only, no
// float atomics: two calls give the same bits.
//
// SLICE VALID.  k_slice_valid: one workgroup per z-slice ORs "a voxel is <= -1" over the slice (16 B per lane where the slice's
// bytes are 16-B aligned, bytes at its ragged ends) and its first thread stores valid[z]: plain stores, every entry written.
// SURFACE.  k_mask_surface: a workgroup owns a 4x8x64 tile (voxel_rows.h) and stages it with its one-voxel halo in LDS as bytes
// (0 / 1; a cell outside the volume or in a slice that is not valid is 0 = background), so the mask is read once per tile.  A
// voxel is surface iff it is set and one of its 4 in-plane (SLICES) or 6 face neighbours is 0.  With SLICES the planes above and
// below are not staged.  Every voxel of out is written.
// HISTOGRAM.  k_surface_hist: surfaces are sparse and most distances small.  A thread reads four 16-byte groups of surf (all four
// loads in flight together) and loads d2 only under a set byte; a workgroup whose 16384 voxels hold no surface voxel ends there.
// The bin of a voxel: bins for CVX_EDT_NONE (unmatched), bins - 1 for (uint32)d2 >= bins - 1 (overflow; takes a negative d2), else
// d2.  A thread combines the run of equal bins it meets (neighbouring surface voxels mostly share
// theirs) and sends a run to the workgroup's LDS histogram of the bins below kHistLds with one 32-bit LDS atomic, or, for a bin
// beyond it, with one 64-bit global atomic.  kHistLds = 4096 bins = 16 KB: eight 256-thread workgroups fit in a CU's 160 KB and
// fill its 32 wave slots, and d2 < 4096 covers every distance below 64 voxels.  A workgroup reads at most kHistPerGroup = 16384
// voxels, so a 32-bit LDS count cannot wrap.  At the end the workgroup adds its non-zero LDS bins to hist with 64-bit global
// atomics.  Integer adds commute: the histogram does not depend on scheduling.
#include "entry_checks.h"

namespace cvx {

constexpr int kHistLds = 4096;                                // bins of the per-workgroup LDS histogram
constexpr int kHistIters = 4;                                 // 16-byte groups per thread
constexpr long kHistPerGroup = 16L * kCclThreads * kHistIters;  // voxels per workgroup
static_assert(kHistPerGroup + 32 < (1L << 32), "a workgroup's voxels, ragged ends included, fit a 32-bit LDS count");
constexpr long kHistBinsMax = (1L << 24) + 1;
constexpr long kHistVoxelsMax = 1L << 40;                     // the grid of k_surface_hist stays below 2^31 workgroups

// ---- slice valid ----

__global__ __launch_bounds__(kCclThreads) void k_slice_valid(const int8_t* __restrict__ y, long slice, int* __restrict__ valid) {
    const int8_t* p = y + (long)blockIdx.x * slice;
    const long head = min(slice, (long)((16 - ((uintptr_t)p & 15)) & 15)), groups = (slice - head) / 16, tail = head + groups * 16;
    int bad = 0;
    for (long g = threadIdx.x; g < groups; g += kCclThreads) {
        const uint4 v = ((const uint4*)(p + head))[g];
        bad |= ((v.x | v.y | v.z | v.w) & 0x80808080u) != 0;  // int8 <= -1: the sign bit
    }
    if (threadIdx.x < head) bad |= p[threadIdx.x] < 0;
    if (tail + threadIdx.x < slice) bad |= p[tail + threadIdx.x] < 0;  // fewer than 16 left
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) valid[blockIdx.x] = !bad;
}

// ---- surface ----

constexpr int kSurfCells = kHaloZ * kHaloY * kHaloX;  // 3960 bytes

template <bool SLICES>
__global__ __launch_bounds__(kCclThreads) void k_mask_surface(const uint8_t* __restrict__ mask, const int* __restrict__ valid, Dims d,
                                                              uint8_t* __restrict__ out) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    __shared__ uint8_t cell[kSurfCells];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    constexpr int kFirst = SLICES ? kHaloY * kHaloX : 0, kLast = SLICES ? kSurfCells - kHaloY * kHaloX : kSurfCells;  // own planes only
    for (int c = kFirst + threadIdx.x; c < kLast; c += kCclThreads) {
        const int x = x0 - 1 + c % kHaloX, y = y0 - 1 + c / kHaloX % kHaloY, z = z0 - 1 + c / (kHaloX * kHaloY);
        bool in = (unsigned)x < (unsigned)d.W && (unsigned)y < (unsigned)d.H && (unsigned)z < (unsigned)d.D;
        if (SLICES && in && valid) in = valid[z] != 0;
        cell[c] = in && mask[((long)z * d.H + y) * d.W + x] != 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + wave, x = x0 + lane;
    if (z >= d.D || x >= d.W) return;
    for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) {
        const uint8_t* p = cell + halo_cell(wave, yy, lane);
        int inside = p[-1] & p[1] & p[-kHaloX] & p[kHaloX];
        if (!SLICES) inside &= p[-kHaloY * kHaloX] & p[kHaloY * kHaloX];
        out[((long)z * d.H + y0 + yy) * d.W + x] = p[0] & (inside ^ 1);
    }
}

// ---- histogram ----

struct HistRun {
    long bin;  // -1: none yet
    unsigned count;
};

__device__ __forceinline__ void hist_flush(unsigned* lds, unsigned long long* __restrict__ hist, const HistRun& r) {
    if (r.bin < 0) return;
    if (r.bin < kHistLds) atomicAdd(lds + r.bin, r.count);
    else atomicAdd(hist + r.bin, (unsigned long long)r.count);
}

__device__ __forceinline__ void hist_tally(unsigned* lds, unsigned long long* __restrict__ hist, HistRun& r, int d, long bins) {
    const long bin = d == CVX_EDT_NONE ? bins : (long)(unsigned)d >= bins - 1 ? bins - 1 : (long)d;
    if (bin != r.bin) {
        hist_flush(lds, hist, r);
        r = HistRun{bin, 0};
    }
    ++r.count;
}

// head: the voxels before the first 16-B aligned byte of surf, groups: the whole 16-byte groups after them
__global__ __launch_bounds__(kCclThreads) void k_surface_hist(const uint8_t* __restrict__ surf, const int* __restrict__ d2, long n, long head,
                                                              long groups, long bins, unsigned long long* __restrict__ hist) {
    __shared__ unsigned lds[kHistLds];
    const uint4* s16 = (const uint4*)(surf + head);
    const long g0 = (long)blockIdx.x * (kCclThreads * kHistIters) + threadIdx.x;
    uint4 v[kHistIters];  // all of the thread's surf loads are in flight together
    unsigned any = 0;
#pragma unroll
    for (int it = 0; it < kHistIters; ++it) {
        const long g = g0 + (long)it * kCclThreads;
        v[it] = g < groups ? s16[g] : uint4{0, 0, 0, 0};
        any |= v[it].x | v[it].y | v[it].z | v[it].w;
    }
    // most workgroups see no surface voxel: they are done, without touching LDS (workgroup 0 also owns the ragged ends)
    if (!__syncthreads_or(any != 0 || blockIdx.x == 0)) return;
    for (int b = threadIdx.x; b < kHistLds; b += kCclThreads) lds[b] = 0;
    __syncthreads();
    HistRun r{-1, 0};
#pragma unroll
    for (int it = 0; it < kHistIters; ++it) {
        if ((v[it].x | v[it].y | v[it].z | v[it].w) == 0) continue;
        const unsigned w[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        const int* q = d2 + head + (g0 + (long)it * kCclThreads) * 16;  // a set byte: the group lies below `groups`
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (w[i >> 2] >> (8 * (i & 3)) & 0xffu) hist_tally(lds, hist, r, q[i], bins);
    }
    if (blockIdx.x == 0) {  // the ragged ends: fewer than 16 voxels each
        const long tail = head + groups * 16;
        if (threadIdx.x < head && surf[threadIdx.x]) hist_tally(lds, hist, r, d2[threadIdx.x], bins);
        if (tail + threadIdx.x < n && surf[tail + threadIdx.x]) hist_tally(lds, hist, r, d2[tail + threadIdx.x], bins);
    }
    hist_flush(lds, hist, r);
    __syncthreads();
    for (int b = threadIdx.x; b < kHistLds && b <= bins; b += kCclThreads) {
        const unsigned c = lds[b];
        if (c) atomicAdd(hist + b, (unsigned long long)c);
    }
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_slice_valid(const int8_t* y, int D, int H, int W, int32_t* valid, hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("slice_valid", why);
    if (D == 0) return 0;
    if (!valid || (n > 0 && !y)) return cvx_fail("slice_valid", "null pointer");
    if ((uintptr_t)valid & 3) return cvx_fail("slice_valid", "valid must be 4-B aligned");
    hipLaunchKernelGGL(k_slice_valid, dim3((unsigned)D), dim3(kCclThreads), 0, st, y, (long)H * W, valid);  // an empty slice is valid
    return cvx_check_launch();
}

extern "C" int cvx_surface_mask(const uint8_t* mask, const int32_t* valid, int D, int H, int W, int slices, uint8_t* out, hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("mask_surface", why);
    if (slices != 0 && slices != 1) return cvx_fail("mask_surface", "slices must be 0 or 1");
    if (!slices && valid) return cvx_fail("mask_surface", "valid is for slices = 1: in 3-D every slice is scored");
    if ((uintptr_t)valid & 3) return cvx_fail("mask_surface", "valid must be 4-B aligned");
    if (n == 0) return 0;
    if (!mask || !out) return cvx_fail("mask_surface", "null pointer");
    if (mask == out) return cvx_fail("mask_surface", "mask and out must be different arrays");
    const Dims d = ccl_dims(D, H, W);
    const dim3 grid((unsigned)tile_count(d)), block(kCclThreads);
    if (slices) hipLaunchKernelGGL(k_mask_surface<true>, grid, block, 0, st, mask, valid, d, out);
    else hipLaunchKernelGGL(k_mask_surface<false>, grid, block, 0, st, mask, valid, d, out);
    return cvx_check_launch();
}

extern "C" int cvx_surface_distance_hist(const uint8_t* surf, const int32_t* d2, long n, long bins, int64_t* hist, hipStream_t st) {
    if (n < 0 || n > kHistVoxelsMax) return cvx_fail("surface_distance_hist", "n must lie in [0, 2^40]");
    if (bins < 2 || bins > kHistBinsMax) return cvx_fail("surface_distance_hist", "bins must lie in [2, 2^24 + 1]");
    if (!hist || (n > 0 && (!surf || !d2))) return cvx_fail("surface_distance_hist", "null pointer");
    if (((uintptr_t)hist & 7) || ((uintptr_t)d2 & 3)) return cvx_fail("surface_distance_hist", "misaligned pointer");
    CVX_HIP(hipMemsetAsync(hist, 0, (size_t)(bins + 1) * sizeof(int64_t), st));
    if (n == 0) return 0;
    const long head = n < 16 ? n : (long)((16 - ((uintptr_t)surf & 15)) & 15), groups = (n - head) / 16;
    const long per = (long)kCclThreads * kHistIters;
    const long blocks = groups ? (groups + per - 1) / per : 1;  // <= 2^40 / 65536
    hipLaunchKernelGGL(k_surface_hist, dim3((unsigned)blocks), dim3(kCclThreads), 0, st, surf, d2, n, head, groups, bins,
                       (unsigned long long*)hist);
    return cvx_check_launch();
}
