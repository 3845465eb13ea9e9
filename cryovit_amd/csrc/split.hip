// Splitting touching instances at their necks (`--split-radius`): the instances of an int32 label volume are eroded to cores
// (edt.hip + components.hip, called by the layer above), and this file grows the cores back inside their instances and numbers
// the pieces.
//
// Regrowth is a shortest-path assignment.  A step joins two neighbouring voxels (6 or 26) of the SAME non-zero input label; a
// foreground voxel goes to the seed with the smallest pair (steps to the seed, seed id).  With key = steps << 32 | seed id that is
// the unique fixpoint of
//     key[v] = min(key[v], min over allowed neighbours n of key[n] + (1 << 32)),   seeds start at (0, id), the rest at all-ones
// (unique: a key can only be lowered to the length of a real path to a real seed, and the least such pair propagates along a
// shortest path whatever the order of the updates).  So the update order is free:
//   k_split_round  a workgroup owns a 4x8x64 tile, loads keys and labels with a one-voxel halo into LDS, relaxes there until its
//                  tile is stable, stores the interior keys it lowered (one aligned 8-B store each: a neighbour's halo read is
//                  never torn, and a stale one is still a valid upper bound) and raises the round's flag.  It waits for no other
//                  workgroup.  The host launches rounds until one raises no flag: then every tile was stable against the halo
//                  everybody saw, which is the fixpoint.
// Renumbering follows components.hip: per seed the smallest voxel index (integer atomicMin per run of a row piece), ranked by the
// caller, then one pass writes labels = rank, the table rows (integer add / min / max) and the input id of every piece.
// Integers only; the result does not depend on scheduling.
#include "entry_checks.h"

namespace cvx {

typedef unsigned long long SplitKey;
constexpr SplitKey kKeyNone = ~0ull;
constexpr SplitKey kKeyStep = 1ull << 32;
constexpr int HZ = TZ + 2, HY = TY + 2, HX = TX + 2;  // tile with its halo
constexpr int kHaloVox = HZ * HY * HX;                // 3960 cells: 31 KB of keys + 15.5 KB of labels

__device__ __forceinline__ SplitKey ld_key_lds(const SplitKey* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_key_lds(SplitKey* p, SplitKey v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ SplitKey ld_key_dev(const SplitKey* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_key_dev(SplitKey* p, SplitKey v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// mask[v] = d2[v] > thr (and d2 is a distance at all): the voxels deeper than the radius inside the foreground
__global__ __launch_bounds__(kCclThreads) void k_split_core_mask(const int* __restrict__ d2, int thr, long n, uint8_t* __restrict__ mask) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= n) return;
    const int d = d2[v];
    mask[v] = d > thr && d != CVX_EDT_NONE;
}

// has_core[id] = 1 for every input instance that holds a core voxel (plain stores of the same value)
__global__ __launch_bounds__(kCclThreads) void k_split_flag(const int* __restrict__ labels, const int* __restrict__ cores, long n, long k,
                                                            int* __restrict__ has_core) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= n || cores[v] <= 0) return;
    const int id = labels[v];
    if (id >= 1 && id <= k) has_core[id] = 1;
}

// a core voxel is a seed voxel of its core; an instance without a core is its own seed, id m + (input id)
__global__ __launch_bounds__(kCclThreads) void k_split_init(const int* __restrict__ labels, const int* __restrict__ cores,
                                                            const int* __restrict__ has_core, long n, long k, long m, SplitKey* __restrict__ keys) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= n) return;
    const int id = labels[v];
    SplitKey key = kKeyNone;
    if (id >= 1 && id <= k) {
        const int c = cores ? cores[v] : 0;
        if (c >= 1 && c <= m) key = (SplitKey)c;
        else if (!has_core[id]) key = (SplitKey)(m + id);
    }
    keys[v] = key;
}

// is (dz, dy, dx) a step of the CONN-neighbourhood?
template <int CONN>
__device__ __forceinline__ constexpr bool is_step(int dz, int dy, int dx) {
    const int axes = (dz != 0) + (dy != 0) + (dx != 0);
    return axes != 0 && (CONN == 26 || axes == 1);
}

template <int CONN>
__global__ __launch_bounds__(kCclThreads) void k_split_round(const int* __restrict__ labels, SplitKey* __restrict__ keys, Dims d,
                                                             int* __restrict__ changed) {
    __shared__ SplitKey key[kHaloVox];
    __shared__ int lab[kHaloVox];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    // labels with the halo; a cell outside the volume is background
    int any = 0;
    for (int c = threadIdx.x; c < kHaloVox; c += kCclThreads) {
        const int x = x0 - 1 + c % HX, y = y0 - 1 + c / HX % HY, z = z0 - 1 + c / (HX * HY);
        const bool in = (unsigned)x < (unsigned)d.W && (unsigned)y < (unsigned)d.H && (unsigned)z < (unsigned)d.D;
        const int l = in ? labels[((long)z * d.H + y) * d.W + x] : 0;
        lab[c] = l;
        const bool interior = x >= x0 && x < x0 + TX && y >= y0 && y < y0 + TY && z >= z0 && z < z0 + TZ;
        any |= interior && l != 0;
    }
    if (!__syncthreads_or(any)) return;  // no foreground in the tile: nothing to assign
    for (int c = threadIdx.x; c < kHaloVox; c += kCclThreads) {
        const int x = x0 - 1 + c % HX, y = y0 - 1 + c / HX % HY, z = z0 - 1 + c / (HX * HY);
        key[c] = lab[c] ? ld_key_dev(keys + ((long)z * d.H + y) * d.W + x) : kKeyNone;  // lab != 0 only inside the volume
    }
    __syncthreads();
    // per own voxel: the steps that stay inside its instance, one bit per neighbour; none for a voxel that cannot be lowered
    // (background, or a seed voxel: no key is below (0, its own id) + a step)
    uint32_t allowed[kPerThread];
    int open = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int li = threadIdx.x + k * kCclThreads;
        const int c = ((li / (TX * TY) + 1) * HY + (li / TX & (TY - 1)) + 1) * HX + (li & (TX - 1)) + 1;
        const int l = lab[c];
        uint32_t m = 0;
        if (l != 0 && key[c] >= kKeyStep) {
            int bit = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!is_step<CONN>(dz, dy, dx)) continue;
                        if (lab[c + (dz * HY + dy) * HX + dx] == l) m |= 1u << bit;
                        ++bit;
                    }
        }
        allowed[k] = m;
        open |= m != 0;
    }
    if (!__syncthreads_or(open)) return;  // every voxel of the tile is a seed voxel or has no neighbour to step from
    // relax inside LDS until a sweep lowers nothing.  Other waves lower keys meanwhile; whatever a read returns is the length of
    // a real path, so the order only changes how many sweeps it takes.
    uint32_t lowered = 0;  // bit k: own voxel k ends below the key it was loaded with
    for (;;) {
        int moved = 0;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const uint32_t m = allowed[k];
            if (m == 0) continue;
            const int li = threadIdx.x + k * kCclThreads;
            const int c = ((li / (TX * TY) + 1) * HY + (li / TX & (TY - 1)) + 1) * HX + (li & (TX - 1)) + 1;
            const SplitKey mine = ld_key_lds(key + c);
            SplitKey best = mine;
            int bit = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!is_step<CONN>(dz, dy, dx)) continue;
                        if (m >> bit & 1) {
                            const SplitKey nk = ld_key_lds(key + c + (dz * HY + dy) * HX + dx);
                            if (nk != kKeyNone) best = min(best, nk + kKeyStep);  // steps < 2^31: no carry out of the key
                        }
                        ++bit;
                    }
            if (best < mine) {
                st_key_lds(key + c, best);
                lowered |= 1u << k;
                moved = 1;
            }
        }
        if (!__syncthreads_or(moved)) break;
    }
    // only this workgroup writes its interior, so a plain 8-B store of the lower key is enough
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (!(lowered >> k & 1)) continue;
        const int li = threadIdx.x + k * kCclThreads;
        const int lx = li & (TX - 1), ly = li / TX & (TY - 1), lz = li / (TX * TY);
        const int c = ((lz + 1) * HY + ly + 1) * HX + lx + 1;
        st_key_dev(keys + ((long)(z0 + lz) * d.H + y0 + ly) * d.W + x0 + lx, key[c]);  // lowered => foreground => inside the volume
    }
    if (__syncthreads_or(lowered != 0) && threadIdx.x == 0) *changed = 1;
}

// seed id of a key, 0 for anything that is no seed of 1..seeds (background, or a voxel no seed reached)
__device__ __forceinline__ int key_seed(SplitKey k, long seeds) {
    const unsigned s = (unsigned)(k & 0xffffffffu);
    return k != kKeyNone && s >= 1 && s <= seeds ? (int)s : 0;
}

// a row piece of keys -> the seed ids of its foreground voxels
__device__ __forceinline__ void seed_piece(const SplitKey* __restrict__ keys, const int* __restrict__ labels, long v0, int cnt, long seeds,
                                           int (&seed)[RV], int (&lab)[RV]) {
    row_load(labels + v0, cnt, lab);
#pragma unroll
    for (int i = 0; i < RV; ++i) seed[i] = i < cnt && lab[i] != 0 ? key_seed(keys[v0 + i], seeds) : 0;
}

__global__ __launch_bounds__(kCclThreads) void k_split_fill(int* __restrict__ p, long n, int value) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < n) p[i] = value;
}

// first[seed] = the smallest linear index of its voxels: the first voxel of every run along a row piece is a candidate
__global__ __launch_bounds__(kCclThreads) void k_split_first(const SplitKey* __restrict__ keys, const int* __restrict__ labels, long seeds,
                                                             int* __restrict__ first, Dims d, int segs) {
    int z, y, x0, cnt;
    if (!row_piece(d, segs, z, y, x0, cnt)) return;
    const long v0 = ((long)z * d.H + y) * d.W + x0;
    int seed[RV], lab[RV];
    seed_piece(keys, labels, v0, cnt, seeds, seed, lab);
    int cur = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        if (seed[i] == cur) continue;
        cur = seed[i];
        if (cur && (int)(v0 + i) < *(volatile int*)(first + cur)) atomicMin(first + cur, (int)(v0 + i));
    }
}

// labels_out = rank of the voxel's seed, the table rows of the pieces, and component[piece] = the input id it lies in (every
// run of a piece stores the same value)
__global__ __launch_bounds__(kCclThreads) void k_split_relabel(const SplitKey* __restrict__ keys, const int* __restrict__ labels,
                                                               const int* __restrict__ rank, long seeds, long kp, int* __restrict__ labels_out,
                                                               long long* __restrict__ table, long long* __restrict__ component, Dims d, int segs) {
    int z, y, x0, cnt;
    if (!row_piece(d, segs, z, y, x0, cnt)) return;
    const long v0 = ((long)z * d.H + y) * d.W + x0;
    int id[RV], lab[RV];
    seed_piece(keys, labels, v0, cnt, seeds, id, lab);
    int last_seed = 0, last_id = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        if (id[i] != last_seed) {
            last_seed = id[i];
            const int r = last_seed ? rank[last_seed] : 0;
            last_id = r >= 1 && r <= kp ? r : 0;  // (a rank past the caller's kp would index past its table)
            if (last_id) component[last_id - 1] = lab[i];
        }
        id[i] = last_id;
    }
    row_store(labels_out + v0, cnt, id);
    table_add_piece(table, id, z, y, x0, cnt);
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_split_core_mask(const int32_t* d2, int D, int H, int W, int threshold_d2, uint8_t* mask, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("split_core_mask", kExtentsRule);
    if (threshold_d2 < 0) return cvx_fail("split_core_mask: threshold_d2 < 0");
    if (n == 0) return 0;
    if (!d2 || !mask) return cvx_fail("split_core_mask: null pointer");
    if ((uintptr_t)d2 & 3) return cvx_fail("split_core_mask: d2 must be 4-B aligned");
    hipLaunchKernelGGL(k_split_core_mask, dim3(blocks_of(n)), dim3(kCclThreads), 0, st, d2, threshold_d2, n, mask);
    return cvx_check_launch();
}

extern "C" int cvx_split_init(const int32_t* labels, const int32_t* cores, int D, int H, int W, long k, long m, int32_t* has_core,
                              uint64_t* keys, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("split_init", kExtentsRule);
    if (k < 0 || m < 0 || k > n || m > n) return cvx_fail("split_init: k and m must lie in [0, D*H*W]");
    if (n == 0) return 0;
    if (!labels || !has_core || !keys || (m > 0 && !cores)) return cvx_fail("split_init: null pointer");
    if ((((uintptr_t)labels | (uintptr_t)cores | (uintptr_t)has_core) & 3) || ((uintptr_t)keys & 7))
        return cvx_fail("split_init: int32 volumes must be 4-B aligned, keys 8-B aligned");
    CVX_HIP(hipMemsetAsync(has_core, 0, (size_t)(k + 1) * sizeof(int), st));
    int rc;
    if (m > 0) {
        hipLaunchKernelGGL(k_split_flag, dim3(blocks_of(n)), dim3(kCclThreads), 0, st, labels, cores, n, k, has_core);
        if ((rc = cvx_check_launch())) return rc;
    }
    hipLaunchKernelGGL(k_split_init, dim3(blocks_of(n)), dim3(kCclThreads), 0, st, labels, m > 0 ? cores : nullptr, has_core, n, k, m,
                       (SplitKey*)keys);
    return cvx_check_launch();
}

extern "C" int cvx_split_rounds(const int32_t* labels, uint64_t* keys, int D, int H, int W, int connectivity, int rounds, int32_t* changed,
                                hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("split_rounds", kExtentsRule);
    if (connectivity != 6 && connectivity != 26) return cvx_fail("split_rounds: connectivity must be 6 or 26");
    if (rounds < 1) return cvx_fail("split_rounds: rounds < 1");
    if (!changed || (n > 0 && (!labels || !keys))) return cvx_fail("split_rounds: null pointer");
    if ((((uintptr_t)changed | (uintptr_t)labels) & 3) || ((uintptr_t)keys & 7))
        return cvx_fail("split_rounds: changed and labels must be 4-B aligned, keys 8-B aligned");
    CVX_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int), st));
    if (n == 0) return 0;
    const Dims d = ccl_dims(D, H, W);
    const long tiles = tile_count(d);
    for (int r = 0; r < rounds; ++r) {
        if (connectivity == 26) hipLaunchKernelGGL(k_split_round<26>, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, labels, (SplitKey*)keys, d, changed + r);
        else hipLaunchKernelGGL(k_split_round<6>, dim3((unsigned)tiles), dim3(kCclThreads), 0, st, labels, (SplitKey*)keys, d, changed + r);
        const int rc = cvx_check_launch();
        if (rc) return rc;
    }
    return 0;
}

extern "C" int cvx_split_first(const int32_t* labels, const uint64_t* keys, int D, int H, int W, long seeds, int32_t* first, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("split_first", kExtentsRule);
    if (seeds < 0 || seeds > 2 * n) return cvx_fail("split_first: seeds outside [0, 2*D*H*W]");
    if (!first || (n > 0 && (!labels || !keys))) return cvx_fail("split_first: null pointer");
    if ((((uintptr_t)first | (uintptr_t)labels) & 3) || ((uintptr_t)keys & 7))
        return cvx_fail("split_first: first and labels must be 4-B aligned, keys 8-B aligned");
    hipLaunchKernelGGL(k_split_fill, dim3(blocks_of(seeds + 1)), dim3(kCclThreads), 0, st, first, seeds + 1, INT_MAX);
    int rc = cvx_check_launch();
    if (rc || n == 0) return rc;
    const int segs = (W + RV - 1) / RV;
    hipLaunchKernelGGL(k_split_first, dim3(blocks_of((long)D * H * segs)), dim3(kCclThreads), 0, st, (const SplitKey*)keys, labels, seeds, first,
                       ccl_dims(D, H, W), segs);
    return cvx_check_launch();
}

extern "C" int cvx_split_relabel(const int32_t* labels, const uint64_t* keys, const int32_t* rank, int D, int H, int W, long seeds, long kp,
                                 int32_t* labels_out, int64_t* table, int64_t* component, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("split_relabel", kExtentsRule);
    if (seeds < 0 || seeds > 2 * n || kp < 0 || kp > seeds) return cvx_fail("split_relabel: need 0 <= kp <= seeds <= 2*D*H*W");
    if (n == 0) return 0;
    if (!labels || !keys || !rank || !labels_out || (kp > 0 && (!table || !component))) return cvx_fail("split_relabel: null pointer");
    if ((((uintptr_t)labels | (uintptr_t)rank | (uintptr_t)labels_out) & 3) || (((uintptr_t)keys | (uintptr_t)table | (uintptr_t)component) & 7))
        return cvx_fail("split_relabel: int32 arrays must be 4-B aligned, keys, table and component 8-B aligned");
    const Dims d = ccl_dims(D, H, W);
    int rc;
    if (kp > 0) {
        hipLaunchKernelGGL(k_table_init<CVX_COMPONENT_COLS>, dim3(blocks_of(kp * CVX_COMPONENT_COLS)), dim3(kCclThreads), 0, st, (long long*)table, kp, d);
        if ((rc = cvx_check_launch())) return rc;
    }
    const int segs = (W + RV - 1) / RV;
    hipLaunchKernelGGL(k_split_relabel, dim3(blocks_of((long)D * H * segs)), dim3(kCclThreads), 0, st, (const SplitKey*)keys, labels, rank, seeds, kp,
                       labels_out, (long long*)table, (long long*)component, d, segs);
    return cvx_check_launch();
}
