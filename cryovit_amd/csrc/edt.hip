// Exact squared Euclidean distance maps of a mask or an instance volume, and the per-instance reduction over (labels, d2) that
// `cryovit infer --morphology` and `cryovit instances --morphology / --distance-to` read: thickness, surface, deepest voxel,
// gap to another label.  Integers only, no atomics in the transform and no workspace: two calls give the same bits.
//
// The transform is separable (out[v] = min over sites s of dz^2 + dy^2 + dx^2), three passes over the int32 volume:
//   x pass   src -> out: per row, the squared distance to the nearest site of the row (kEdtNone when the row has none).  One
//            wave per row.  The wave's ballots are 64-voxel site bitmaps: a count of leading / trailing zeros finds the nearest
//            site inside a voxel's own bitmap, and a forward max-scan / backward min-scan over the bitmaps' last / first sites
//            (one lane per bitmap) finds it beyond.
//   y pass   in place, out[i] = min_j f[j] + (i - j)^2 along y (lines of H elements, stride W)
//   z pass   the same along z (lines of D elements, stride H*W); cvx_slices_edt_squared leaves it out: every z-slice on its own
// A min-plus workgroup owns a slab of 64 adjacent x (256-B row pieces: every access of either pass is a coalesced wave access)
// times the WHOLE line, so that nothing it overwrites is still needed by another workgroup.
//   RULE: a line of up to kLineMax = 512 elements (512 x 256 B = 128 KB of LDS) is staged in LDS once and every output is
//   computed from there.  A longer line is done in place from global memory in two sweeps over blocks of outputs: blocks in
//   descending order with the sources j <= i only, then in ascending order with j >= i only.  A block is computed, then
//   (barrier) written, so a sweep only ever reads elements it has not yet written.  The second sweep reads the first one's
//   results g1[j] = min_{k<=j} f[k] + (j-k)^2; every term it forms, f[k] + (j-k)^2 + (j-i)^2 with k <= j >= i, is at least
//   f[k] + (i-k)^2 (one of the two steps is at least as long as |i-k|), and the terms with j = k or j = i are exactly those,
//   so the minimum is the exact transform.
// A thread holds kIpt = 8 consecutive outputs of one x and updates all of them per read of f[j]; (i - j)^2 is the same for a
// whole wave (scalar).  f[j] == kEdtNone is skipped, so every sum formed is a true squared distance inside the volume, which
// the entry point has checked to be below INT32_MAX.  The walk goes outwards from the thread's outputs and stops once the
// squared step alone reaches the largest of the wave's current minima.  The site bitmaps and the walk are in edt_pieces.h, which
// nearest.hip shares.
#include "edt_pieces.h"
#include "entry_checks.h"

namespace cvx {

constexpr int kLineMax = 512;              // longest line staged in LDS

// ---- x pass ----

template <typename T, bool NONZERO>
__global__ __launch_bounds__(kRowThreads) void k_edt_rows(const T* __restrict__ src, int* __restrict__ out, long rows, int W, int nc) {
    extern __shared__ unsigned long long edt_row_lds[];
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (kRowThreads / 64) + wave_id();
    const bool live = row < rows;  // a wave past the last row walks the same loops (their barriers) and touches no memory
    const T* s = src + (live ? row : 0) * W;
    const RowSites sites = edt_row_sites(edt_row_lds, nc, [&](int x) { return live && x < W && (s[x] != 0) == NONZERO; });
    if (!live) return;
    int* o = out + row * W;
    for (int c = 0; c < nc; ++c) {
        const int x = c * 64 + lane;
        if (x >= W) break;
        int left, right;
        edt_row_sides(sites, c, lane, left, right);
        int d = INT_MAX;
        if (left >= 0) d = x - left;
        if (right != INT_MAX) d = min(d, right - x);
        o[x] = d == INT_MAX ? kEdtNone : d * d;  // d < W, and (W-1)^2 < INT32_MAX was checked
    }
}

// ---- y and z passes ----

__device__ __forceinline__ void edt_store(int* line, const LineGeom& g, int i0, const int (&best)[kIpt]) {
#pragma unroll
    for (int k = 0; k < kIpt; ++k)
        if (i0 + k < g.n) line[(long)(i0 + k) * g.stride] = best[k];
}

// lines of up to kLineMax elements: staged in LDS (g.n * kSlab ints), every wave then takes blocks of kIpt outputs
__global__ __launch_bounds__(kLineWavesMax * 64) void k_edt_lines_lds(int* vol, LineGeom g) {
    extern __shared__ int edt_line_lds[];
    const int lane = threadIdx.x & 63, wave = wave_id(), waves = blockDim.x >> 6;
    const int x = (int)(blockIdx.x % g.nslab) * kSlab + lane;
    const bool in = x < g.W;
    int* line = vol + (long)(blockIdx.x / g.nslab) * g.ostride + (in ? x : 0);
    for (int j = wave; j < g.n; j += waves) edt_line_lds[j * kSlab + lane] = in ? line[(long)j * g.stride] : kEdtNone;
    __syncthreads();
    const int* col = edt_line_lds + lane;
    for (int i0 = wave * kIpt; i0 < g.n; i0 += waves * kIpt) {
        int best[kIpt];
#pragma unroll
        for (int k = 0; k < kIpt; ++k) best[k] = kEdtNone;
        edt_minplus<EdtDistance, 0>([&](int j) { return col[j * kSlab]; }, in, i0, 0, g.n, best);
        if (in) edt_store(line, g, i0, best);
    }
}

// longer lines: two sweeps in place (the rule at the top of the file)
__global__ __launch_bounds__(kLineWavesMax * 64) void k_edt_lines_long(int* vol, LineGeom g) {
    const int lane = threadIdx.x & 63, wave = wave_id(), waves = blockDim.x >> 6;
    const int x = (int)(blockIdx.x % g.nslab) * kSlab + lane;
    const bool in = x < g.W;
    int* line = vol + (long)(blockIdx.x / g.nslab) * g.ostride + (in ? x : 0);
    auto f = [&](int j) { return in ? __hip_atomic_load(line + (long)j * g.stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : kEdtNone; };
    const int per_block = waves * kIpt, blocks = (g.n + per_block - 1) / per_block;
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int t = 0; t < blocks; ++t) {
            const int b = sweep == 0 ? blocks - 1 - t : t;
            const int i0 = b * per_block + wave * kIpt;
            int best[kIpt];
#pragma unroll
            for (int k = 0; k < kIpt; ++k) best[k] = kEdtNone;
            if (i0 < g.n) {
                if (sweep == 0) edt_minplus<EdtDistance, 1>(f, in, i0, 0, g.n, best);
                else edt_minplus<EdtDistance, 2>(f, in, i0, 0, g.n, best);
            }
            __syncthreads();  // every wave has read what this block overwrites
            if (in && i0 < g.n) edt_store(line, g, i0, best);
        }
        __syncthreads();  // the first sweep's results are what the second reads
    }
}

// ---- per-instance statistics over (labels, d2) ----

// table rows while the voxels are reduced: count, min d2, the key (d2 << 32 | INT32_MAX - index), unused
__global__ __launch_bounds__(kCclThreads) void k_dstat_init(long long* __restrict__ out, long k) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i >= k * CVX_DSTAT_COLS) return;
    const int c = (int)(i % CVX_DSTAT_COLS);
    out[i] = c == 1 ? LLONG_MAX : c == 2 ? -1 : 0;
}

struct DstatRun {
    int id;
    long long count, lo, key;
};

__device__ __forceinline__ void dstat_flush(long long* __restrict__ out, const DstatRun& r) {
    if (r.id == 0 || r.key < 0) return;
    long long* row = out + (long)(r.id - 1) * CVX_DSTAT_COLS;
    if (r.count) atomicAdd((unsigned long long*)row, (unsigned long long)r.count);
    // entries move one way only: a plain read that shows no change is possible spares the atomic
    if (r.lo < *(volatile long long*)(row + 1)) atomicMin(row + 1, r.lo);
    if (r.key > *(volatile long long*)(row + 2)) atomicMax(row + 2, r.key);
}

__global__ __launch_bounds__(kCclThreads) void k_dstat_reduce(const int* __restrict__ labels, const int* __restrict__ d2, long long* __restrict__ out,
                                                              long k, int thr, Dims dims, int segs) {
    long row;
    int x0, cnt;
    if (!row_piece(dims, segs, row, x0, cnt)) return;
    const long v0 = row * dims.W + x0;
    int id[RV], d[RV];
    row_load(labels + v0, cnt, id);
    row_load(d2 + v0, cnt, d);  // past the row's end id and d are 0: the id is looked at first, and 0 is nobody's
    DstatRun r{0, 0, 0, -1};
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        const int c = id[i] >= 1 && id[i] <= k ? id[i] : 0;  // ids past the table are nobody's
        if (c != r.id) {
            dstat_flush(out, r);
            r = DstatRun{c, 0, LLONG_MAX, -1};
        }
        if (c == 0 || d[i] == kEdtNone) continue;
        r.count += d[i] <= thr;
        r.lo = min(r.lo, (long long)d[i]);
        r.key = max(r.key, ((long long)d[i] << 32) | (long long)(INT_MAX - (int)(v0 + i)));  // equal d2: the smaller index wins
    }
    dstat_flush(out, r);
}

__global__ __launch_bounds__(kCclThreads) void k_dstat_finalize(long long* __restrict__ out, long k) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i >= k) return;
    long long* row = out + i * CVX_DSTAT_COLS;
    const long long key = row[2];
    if (key < 0) {  // no voxel of this id has a distance
        row[0] = 0;
        row[1] = row[2] = row[3] = -1;
        return;
    }
    row[2] = key >> 32;
    row[3] = INT_MAX - (key & 0xffffffffLL);
}

}  // namespace cvx

using namespace cvx;

namespace {

template <typename T>
int edt_launch_rows(const void* src, int sites, int* out, long rows, int W, hipStream_t st) {
    const int nc = (W + 63) / 64;
    const unsigned blocks = (unsigned)((rows + kRowThreads / 64 - 1) / (kRowThreads / 64));
    const size_t lds = edt_row_lds_bytes(nc);
    if (sites == CVX_EDT_SITES_NONZERO) hipLaunchKernelGGL((k_edt_rows<T, true>), dim3(blocks), dim3(kRowThreads), lds, st, (const T*)src, out, rows, W, nc);
    else hipLaunchKernelGGL((k_edt_rows<T, false>), dim3(blocks), dim3(kRowThreads), lds, st, (const T*)src, out, rows, W, nc);
    return cvx_check_launch();
}

int edt_launch_lines(int* vol, int n, long stride, long lines, long ostride, int W, hipStream_t st) {
    if (n <= 1) return 0;  // a line of one element is its own transform
    const LineGeom g{n, stride, ostride, W, (W + kSlab - 1) / kSlab};
    const int waves = min(kLineWavesMax, (n + kIpt - 1) / kIpt);
    const dim3 grid((unsigned)(lines * g.nslab));  // <= D*H*W
    if (n <= kLineMax) {
        const int lds = n * kSlab * (int)sizeof(int);
        CVX_HIP(hipFuncSetAttribute((const void*)k_edt_lines_lds, hipFuncAttributeMaxDynamicSharedMemorySize, kLineMax * kSlab * (int)sizeof(int)));
        hipLaunchKernelGGL(k_edt_lines_lds, grid, dim3(waves * 64), lds, st, vol, g);
    } else {
        hipLaunchKernelGGL(k_edt_lines_long, grid, dim3(waves * 64), 0, st, vol, g);
    }
    return cvx_check_launch();
}

}  // namespace

extern "C" int cvx_edt_squared(const void* src, int src_dtype, int sites, int D, int H, int W, int32_t* out, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("edt_squared", kExtentsRule);
    if (src_dtype != CVX_EDT_U8 && src_dtype != CVX_EDT_I32) return cvx_fail("edt_squared: src_dtype must be CVX_EDT_U8 or CVX_EDT_I32");
    if (sites != CVX_EDT_SITES_ZERO && sites != CVX_EDT_SITES_NONZERO) return cvx_fail("edt_squared: sites must be CVX_EDT_SITES_ZERO or CVX_EDT_SITES_NONZERO");
    if (n == 0) return 0;
    const long long far = (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1);
    if (far >= INT_MAX) return cvx_fail("edt_squared: the squared diagonal (D-1)^2 + (H-1)^2 + (W-1)^2 must be below INT32_MAX");
    if (!src || !out) return cvx_fail("edt_squared: null pointer");
    if (((uintptr_t)out & 3) || (src_dtype == CVX_EDT_I32 && ((uintptr_t)src & 3))) return cvx_fail("edt_squared: int32 volumes must be 4-B aligned");
    int rc = src_dtype == CVX_EDT_U8 ? edt_launch_rows<uint8_t>(src, sites, out, (long)D * H, W, st)
                                     : edt_launch_rows<int32_t>(src, sites, out, (long)D * H, W, st);
    if (rc) return rc;
    if ((rc = edt_launch_lines(out, H, W, D, (long)H * W, W, st))) return rc;  // y: one line per (z, x)
    return edt_launch_lines(out, D, (long)H * W, H, W, W, st);                  // z: one line per (y, x)
}

// every z-slice an image of its own: the x pass and the y pass of cvx_edt_squared, no z pass
extern "C" int cvx_slices_edt_squared(const void* src, int src_dtype, int sites, int D, int H, int W, int32_t* out, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("slices_edt_squared", kExtentsRule);
    if (src_dtype != CVX_EDT_U8 && src_dtype != CVX_EDT_I32) return cvx_fail("slices_edt_squared: src_dtype must be CVX_EDT_U8 or CVX_EDT_I32");
    if (sites != CVX_EDT_SITES_ZERO && sites != CVX_EDT_SITES_NONZERO)
        return cvx_fail("slices_edt_squared: sites must be CVX_EDT_SITES_ZERO or CVX_EDT_SITES_NONZERO");
    if (n == 0) return 0;
    const long long far = (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1);
    if (far >= INT_MAX) return cvx_fail("slices_edt_squared: the squared diagonal (H-1)^2 + (W-1)^2 must be below INT32_MAX");
    if (!src || !out) return cvx_fail("slices_edt_squared: null pointer");
    if (((uintptr_t)out & 3) || (src_dtype == CVX_EDT_I32 && ((uintptr_t)src & 3))) return cvx_fail("slices_edt_squared: int32 volumes must be 4-B aligned");
    const int rc = src_dtype == CVX_EDT_U8 ? edt_launch_rows<uint8_t>(src, sites, out, (long)D * H, W, st)
                                           : edt_launch_rows<int32_t>(src, sites, out, (long)D * H, W, st);
    if (rc) return rc;
    return edt_launch_lines(out, H, W, D, (long)H * W, W, st);  // y: one line per (z, x); a slice without a site stays kEdtNone
}

extern "C" int cvx_instance_distance_stats(const int32_t* labels, const int32_t* d2, int D, int H, int W, long k, int threshold_d2,
                                           int64_t* out, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("instance_distance_stats", kExtentsRule);
    if (k < 0) return cvx_fail("instance_distance_stats: k < 0");
    if (k == 0) return 0;
    if (!out || (n > 0 && (!labels || !d2))) return cvx_fail("instance_distance_stats: null pointer");
    if (((uintptr_t)out & 7) || (((uintptr_t)labels | (uintptr_t)d2) & 3)) return cvx_fail("instance_distance_stats: misaligned pointer");
    hipLaunchKernelGGL(k_dstat_init, dim3(blocks_of(k * CVX_DSTAT_COLS)), dim3(kCclThreads), 0, st, (long long*)out, k);
    int rc = cvx_check_launch();
    if (rc) return rc;
    if (n > 0) {
        const int segs = (W + RV - 1) / RV;
        hipLaunchKernelGGL(k_dstat_reduce, dim3(blocks_of((long)D * H * segs)), dim3(kCclThreads), 0, st, labels, d2, (long long*)out, k, threshold_d2,
                           ccl_dims(D, H, W), segs);
        if ((rc = cvx_check_launch())) return rc;
    }
    hipLaunchKernelGGL(k_dstat_finalize, dim3(blocks_of(k)), dim3(kCclThreads), 0, st, (long long*)out, k);
    return cvx_check_launch();
}
