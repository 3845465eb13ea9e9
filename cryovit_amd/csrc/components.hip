// 3D connected-component labelling of a predicted mask (`cryovit infer --instances`, `cryovit instances`): labels, count and a
// per-instance table (voxels, coordinate sums, bounding box) without the mask leaving HBM.
//
// Union-find on voxel indices.  parent[v] holds (index of v's parent) + 1 for a foreground voxel and 0 for background; a link
// always points from the larger index to the smaller, so the root of a component is its smallest linear voxel index whatever
// the order the links were made in -- the one scheduling-independent fact every later step builds on:
//   1. tile pass     a workgroup resolves a 4x8x64 tile in LDS (atomicMin links) and writes parent = tile root
//   2. border pass   voxels whose neighbour lies in another tile link the two roots in global memory (atomicMin)
//   3. flatten       every voxel is pointed at its root
//   4. (min_size)    per-root voxel counts, runs of one root along x combined per thread before the integer atomicAdd
//   5. compaction    roots (that survive min_size) flagged, block counts, one fixed-order scan of the block counts, ids 1..K
//                    in ascending root index = ascending smallest voxel index
//   6. relabel+table labels = id, and the table rows by integer atomic add / min / max (exact and commutative)
// Only the backward half of the neighbourhood (3 of 6, 13 of 26) is visited: the relation is symmetric.
// Every sum is an integer, so the labels and the table are bit-identical from run to run.
#include "entry_checks.h"

namespace cvx {

constexpr int kChunk = kCclThreads * RV;      // voxels per block in the compaction passes
constexpr int kScanThreads = 1024;
constexpr int kDead = INT_MIN;                // parent[] of a root that min_size removed

__device__ __forceinline__ int ld_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int ld_dev(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_dev(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// LDS union-find on tile-local indices: lab[i] = parent of i (i itself for a root)
__device__ __forceinline__ int lds_find(const int* lab, int v) {
    int p;
    while ((p = ld_lds(lab + v)) != v) v = p;
    return v;
}
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);  // a was a root when read; whoever got there first, a's set and b's set get joined
        if (old == a) return;
        a = old;  // a had been linked elsewhere meanwhile: join that parent with b as well
    }
}

// the same on global indices, parent[v] = parent index + 1.  Links only ever decrease, so a stale read still names an
// ancestor; the atomicMin returns the true value and decides.
__device__ __forceinline__ int dev_find(const int* parent, int v) {
    int p;
    while ((p = ld_dev(parent + v) - 1) != v) v = p;
    return v;
}
__device__ __forceinline__ void dev_union(int* parent, int a, int b) {
    for (;;) {
        a = dev_find(parent, a);
        b = dev_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b + 1);
        if (old == a + 1) return;
        a = old - 1;
    }
}

// is (dz, dy, dx) in the backward half of the CONN-neighbourhood?
template <int CONN>
__device__ __forceinline__ constexpr bool backward(int dz, int dy, int dx) {
    const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
    const int steps = (dz != 0) + (dy != 0) + (dx != 0);
    return before && (CONN == 26 || steps == 1);
}

// 1. tile pass: parent[v] = (smallest voxel index of v's component within its tile) + 1, 0 for background
template <int CONN>
__global__ __launch_bounds__(kCclThreads) void k_ccl_tile(const uint8_t* __restrict__ mask, int* __restrict__ parent, Dims d) {
    __shared__ int lab[kTileVox];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int li = threadIdx.x + k * kCclThreads;
        const int x = x0 + (li & (TX - 1)), y = y0 + (li / TX & (TY - 1)), z = z0 + li / (TX * TY);
        const bool in = x < d.W && y < d.H && z < d.D;
        lab[li] = in && mask[((long)z * d.H + y) * d.W + x] ? li : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int li = threadIdx.x + k * kCclThreads;
        if (ld_lds(lab + li) < 0) continue;
        const int lx = li & (TX - 1), ly = li / TX & (TY - 1), lz = li / (TX * TY);
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward<CONN>(dz, dy, dx)) continue;
                    const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
                    if ((unsigned)nx >= (unsigned)TX || (unsigned)ny >= (unsigned)TY || (unsigned)nz >= (unsigned)TZ) continue;
                    const int nli = (nz * TY + ny) * TX + nx;
                    if (ld_lds(lab + nli) >= 0) lds_union(lab, li, nli);
                }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int li = threadIdx.x + k * kCclThreads;
        const int x = x0 + (li & (TX - 1)), y = y0 + (li / TX & (TY - 1)), z = z0 + li / (TX * TY);
        if (x >= d.W || y >= d.H || z >= d.D) continue;
        int out = 0;
        if (lab[li] >= 0) {
            const int r = lds_find(lab, li);  // local order = global order within a tile, so this is the tile's smallest index
            const int rx = x0 + (r & (TX - 1)), ry = y0 + (r / TX & (TY - 1)), rz = z0 + r / (TX * TY);
            out = (int)(((long)rz * d.H + ry) * d.W + rx) + 1;
        }
        parent[((long)z * d.H + y) * d.W + x] = out;
    }
}

// 2. border pass: every backward neighbour that lies in another tile
template <int CONN>
__global__ __launch_bounds__(kCclThreads) void k_ccl_border(const uint8_t* __restrict__ mask, int* __restrict__ parent, Dims d) {
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int li = threadIdx.x + k * kCclThreads;
        const int lx = li & (TX - 1), ly = li / TX & (TY - 1), lz = li / (TX * TY);
        if (lx > 0 && lx < TX - 1 && ly > 0 && ly < TY - 1 && lz > 0) continue;  // all backward neighbours inside the tile
        const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
        if (x >= d.W || y >= d.H || z >= d.D) continue;
        const long v = ((long)z * d.H + y) * d.W + x;
        if (!mask[v]) continue;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward<CONN>(dz, dy, dx)) continue;
                    const int tnx = lx + dx, tny = ly + dy, tnz = lz + dz;
                    if ((unsigned)tnx < (unsigned)TX && (unsigned)tny < (unsigned)TY && (unsigned)tnz < (unsigned)TZ) continue;  // tile pass
                    const int nx = x + dx, ny = y + dy, nz = z + dz;
                    if ((unsigned)nx >= (unsigned)d.W || (unsigned)ny >= (unsigned)d.H || (unsigned)nz >= (unsigned)d.D) continue;
                    const long nv = ((long)nz * d.H + ny) * d.W + nx;
                    if (mask[nv]) dev_union(parent, (int)v, (int)nv);
                }
    }
}

// 3. flatten: parent[v] = root + 1.  Other lanes may walk through v meanwhile: they meet either its old parent or its root,
// both ancestors.
__global__ __launch_bounds__(kCclThreads) void k_ccl_flatten(int* __restrict__ parent, long n) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= n) return;
    const int p = ld_dev(parent + v);
    if (p == 0 || p == (int)v + 1) return;
    st_dev(parent + v, dev_find(parent, p - 1) + 1);
}

// 4. count[root] += voxels (count = the zeroed label volume, which nothing else uses yet); one add per run of a root along x
__global__ __launch_bounds__(kCclThreads) void k_ccl_sizes(const int* __restrict__ parent, int* __restrict__ count, Dims d, int segs) {
    int z, y, x0, cnt;
    if (!row_piece(d, segs, z, y, x0, cnt)) return;
    int p[RV];
    row_load(parent + ((long)z * d.H + y) * d.W + x0, cnt, p);
    int cur = 0, run = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        if (p[i] != cur) {
            if (cur) atomicAdd(&count[cur - 1], run);
            cur = p[i];
            run = 0;
        }
        ++run;
    }
    if (cur) atomicAdd(&count[cur - 1], run);
}

__device__ __forceinline__ bool is_kept_root(int p, long v, const int* __restrict__ count, int min_size) {
    return p == (int)v + 1 && (min_size <= 1 || count[v] >= min_size);
}

// 5a. partial[block] = kept roots among the block's kChunk voxels (thread t: voxels [t*RV, t*RV + RV) of the chunk)
__global__ __launch_bounds__(kCclThreads) void k_ccl_count_roots(const int* __restrict__ parent, const int* __restrict__ count,
                                                                 int min_size, long n, int* __restrict__ partial) {
    __shared__ int red[kCclThreads / 64];
    const long base = (long)blockIdx.x * kChunk + (long)threadIdx.x * RV;
    int c = 0;
    if (base < n) {
        const int cnt = (int)min((long)RV, n - base);
        int p[RV];
        row_load(parent + base, cnt, p);
#pragma unroll
        for (int i = 0; i < RV; ++i) c += i < cnt && is_kept_root(p[i], base + i, count, min_size);
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kCclThreads / 64; ++w) s += red[w];
        partial[blockIdx.x] = s;
    }
}

// 5b. partial[] -> its exclusive prefix sums, *k_out = the total: one workgroup walking the array in index order
__global__ __launch_bounds__(kScanThreads) void k_ccl_scan(int* __restrict__ partial, int nb, int* __restrict__ k_out) {
    __shared__ int wsum[kScanThreads / 64];
    const int wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nb; base += kScanThreads) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? partial[i] : 0;
        const int incl = wave_scan_incl(v);
        if ((threadIdx.x & 63) == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const int s = wsum[w];
            if (w < wave) woff += s;
            total += s;
        }
        if (i < nb) partial[i] = carry + woff + incl - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *k_out = carry;
}

// 5c. parent[root] = -id for the kept roots in index order, kDead for the others
__global__ __launch_bounds__(kCclThreads) void k_ccl_assign(int* __restrict__ parent, const int* __restrict__ count, int min_size, long n,
                                                            const int* __restrict__ partial) {
    __shared__ int wsum[kCclThreads / 64];
    const long base = (long)blockIdx.x * kChunk + (long)threadIdx.x * RV;
    const int cnt = base < n ? (int)min((long)RV, n - base) : 0;
    int p[RV];
    uint32_t kept = 0, root = 0;
    if (cnt) {
        row_load(parent + base, cnt, p);
#pragma unroll
        for (int i = 0; i < RV; ++i) {
            if (i < cnt && p[i] == (int)(base + i) + 1) {
                root |= 1u << i;
                if (is_kept_root(p[i], base + i, count, min_size)) kept |= 1u << i;
            }
        }
    }
    const int c = __popc(kept);
    const int incl = wave_scan_incl(c);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    int id = partial[blockIdx.x] + incl - c;  // kept roots before this thread's voxels
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) id += wsum[w];
    if (!root) return;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        if (!(root >> i & 1)) continue;
        parent[base + i] = kept >> i & 1 ? -(++id) : kDead;
    }
}

// 6. labels[v] = id of v's root (0: background or removed), and the table from runs of one id along x
__global__ __launch_bounds__(kCclThreads) void k_ccl_relabel(const int* __restrict__ parent, int* __restrict__ labels,
                                                             long long* __restrict__ table, long k, Dims d, int segs) {
    int z, y, x0, cnt;
    if (!row_piece(d, segs, z, y, x0, cnt)) return;
    const long v0 = ((long)z * d.H + y) * d.W + x0;
    int p[RV], id[RV];
    row_load(parent + v0, cnt, p);
    int last_p = 0, last_id = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        if (p[i] != last_p) {
            last_p = p[i];
            const int q = last_p > 0 ? parent[last_p - 1] : last_p;  // a root holds -id or kDead, everything else points at a root
            last_id = q == kDead || -(long)q > k ? 0 : -q;  // (an id past the caller's k would index past its table)
        }
        id[i] = last_id;
    }
    row_store(labels + v0, cnt, id);
    table_add_piece(table, id, z, y, x0, cnt);
}

}  // namespace cvx

using namespace cvx;

namespace {

struct CclLayout {
    long n, nb;              // voxels, compaction blocks
    long off_partial, off_parent, bytes;
};

// scratch: [0, 16) K (int32), then the block counts, then parent int32 [n]; every piece 16-B aligned
bool ccl_layout(int D, int H, int W, CclLayout& L) {
    if (extents_fault(D, H, W, kExtentAny, L.n)) return false;
    L.nb = (L.n + kChunk - 1) / kChunk;
    L.off_partial = 16;
    L.off_parent = L.off_partial + (L.nb * 4 + 15) / 16 * 16;
    L.bytes = L.off_parent + (L.n * 4 + 15) / 16 * 16;
    return true;
}

}  // namespace

extern "C" long cvx_components_scratch_bytes(int D, int H, int W) {
    CclLayout L;
    if (!ccl_layout(D, H, W, L)) return cvx_fail("components", kExtentsRule);
    return L.bytes;
}

extern "C" int cvx_components_label(const uint8_t* mask, int D, int H, int W, int connectivity, long min_size, int32_t* labels,
                                    void* scratch, long scratch_bytes, hipStream_t st) {
    CclLayout L;
    if (!ccl_layout(D, H, W, L)) return cvx_fail("components_label", kExtentsRule);
    if (connectivity != 6 && connectivity != 26) return cvx_fail("components_label: connectivity must be 6 or 26");
    if (min_size < 0) return cvx_fail("components_label: min_size < 0");
    if (!scratch || scratch_bytes < L.bytes) return cvx_fail("components_label: null or short scratch (cvx_components_scratch_bytes)");
    if (L.n > 0 && (!mask || !labels)) return cvx_fail("components_label: null pointer");
    if (((uintptr_t)scratch | (uintptr_t)labels) & 15) return cvx_fail("components_label: labels and scratch must be 16-B aligned");
    int* k_out = (int*)scratch;
    if (L.n == 0) {
        CVX_HIP(hipMemsetAsync(k_out, 0, sizeof(int), st));
        return 0;
    }
    int* partial = (int*)((char*)scratch + L.off_partial);
    int* parent = (int*)((char*)scratch + L.off_parent);
    const Dims d = ccl_dims(D, H, W);
    const int ms = clamp_int(min_size);
    const long tiles = tile_count(d);
    const unsigned nlin = blocks_of(L.n);
    const int segs = (W + RV - 1) / RV;
    const unsigned nrow = blocks_of((long)D * H * segs);
    int rc;
    if (connectivity == 26) hipLaunchKernelGGL(k_ccl_tile<26>, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, mask, parent, d);
    else hipLaunchKernelGGL(k_ccl_tile<6>, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, mask, parent, d);
    if ((rc = cvx_check_launch())) return rc;
    if (connectivity == 26) hipLaunchKernelGGL(k_ccl_border<26>, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, mask, parent, d);
    else hipLaunchKernelGGL(k_ccl_border<6>, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, mask, parent, d);
    if ((rc = cvx_check_launch())) return rc;
    hipLaunchKernelGGL(k_ccl_flatten, dim3(nlin), dim3(kCclThreads), 0, st, parent, L.n);
    if ((rc = cvx_check_launch())) return rc;
    if (ms > 1) {
        CVX_HIP(hipMemsetAsync(labels, 0, (size_t)L.n * sizeof(int), st));
        hipLaunchKernelGGL(k_ccl_sizes, dim3(nrow), dim3(kCclThreads), 0, st, parent, labels, d, segs);
        if ((rc = cvx_check_launch())) return rc;
    }
    hipLaunchKernelGGL(k_ccl_count_roots, dim3((unsigned)L.nb), dim3(kCclThreads), 0, st, parent, labels, ms, L.n, partial);
    if ((rc = cvx_check_launch())) return rc;
    hipLaunchKernelGGL(k_ccl_scan, dim3(1), dim3(kScanThreads), 0, st, partial, (int)L.nb, k_out);
    if ((rc = cvx_check_launch())) return rc;
    hipLaunchKernelGGL(k_ccl_assign, dim3((unsigned)L.nb), dim3(kCclThreads), 0, st, parent, labels, ms, L.n, partial);
    return cvx_check_launch();
}

extern "C" int cvx_components_table(int D, int H, int W, long k, int32_t* labels, int64_t* table, const void* scratch,
                                    long scratch_bytes, hipStream_t st) {
    CclLayout L;
    if (!ccl_layout(D, H, W, L)) return cvx_fail("components_table", kExtentsRule);
    if (k < 0 || k > L.n) return cvx_fail("components_table: k outside [0, D*H*W]");
    if (!scratch || scratch_bytes < L.bytes) return cvx_fail("components_table: null or short scratch (cvx_components_scratch_bytes)");
    if (L.n == 0) return 0;
    if (!labels || (k > 0 && !table)) return cvx_fail("components_table: null pointer");
    if (((uintptr_t)scratch | (uintptr_t)labels) & 15) return cvx_fail("components_table: labels and scratch must be 16-B aligned");
    if ((uintptr_t)table & 7) return cvx_fail("components_table: table must be 8-B aligned");
    if (k == 0) {  // nothing kept: no table to index
        CVX_HIP(hipMemsetAsync(labels, 0, (size_t)L.n * sizeof(int), st));
        return 0;
    }
    const int* parent = (const int*)((const char*)scratch + L.off_parent);
    const Dims d = ccl_dims(D, H, W);
    const int segs = (W + RV - 1) / RV;
    hipLaunchKernelGGL(k_table_init<CVX_COMPONENT_COLS>, dim3(blocks_of(k * CVX_COMPONENT_COLS)), dim3(kCclThreads), 0, st, (long long*)table, k, d);
    int rc = cvx_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_ccl_relabel, dim3(blocks_of((long)D * H * segs)), dim3(kCclThreads), 0, st, parent, labels, (long long*)table, k, d, segs);
    return cvx_check_launch();
}
