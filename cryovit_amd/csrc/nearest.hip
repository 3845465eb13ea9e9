// The labelled form of the distance map (a feature transform) and the pair table `cryovit instances --contacts-with` reads
// from it: for every voxel the squared distance to the nearest instance of a label volume AND that instance's id, then per pair
// (instance a of one label, nearest instance b of the other) the voxels of a within a radius of b, the narrowest gap and where
// it is.  Integers only; no atomics in the transform; integer atomic add / min only in the table.  Two calls give the same bits.
//
// WHY THE TRANSFORM IS EXACT AND INDEPENDENT OF LAUNCH ORDER.  Every voxel wants the lexicographic minimum over the sites s of
// the pair (|v - s|^2, id(s)): the nearest site, the smallest id among equals.  Pairs are held as one key d2 << 32 | id (d2 <
// 2^31 and id < 2^31, so keys are positive int64 and compare like the pairs).  Adding a constant to the d2 of every pair of a
// set keeps their order, hence  min_s (dz^2 + dy^2 + dx^2, id) = min_z' dz^2 + ( min_y' dy^2 + ( min_x' (dx^2, id) ) )  with
// lexicographic minima throughout: the same three passes as edt.hip, on keys.  Every pass takes a minimum over a set that does
// not depend on which thread forms it, so nothing depends on scheduling, and the d2 half is what edt.hip computes, bit for bit.
//   x pass   labels -> keys: the ballot-and-scan row pass of edt.hip (a site is a voxel with a value in 1..k) finds the nearest
//            site to the left and to the right; the id is the label there; at equal distance the smaller id wins.
//   y pass   keys in place, key[i] = min_j key[j] + ((i - j)^2 << 32) along y
//   z pass   the same along z, read from the keys and written as the two int32 planes d2 and nearest.  It is not in place.
// PRUNING.  The walk of edt.hip stops when the squared step ALONE reaches the widest minimum of the wave: no source further out
// can then lower a d2.  It can still EQUAL one (a source whose own d2 is 0, at step^2 == d2) and carry a smaller id, so here
// the walk goes on while step^2 <= the widest d2 and stops only when step^2 exceeds it: every key further out is then larger
// in its d2 half than every minimum held, and can neither lower one nor tie with it.
// SLAB RULE.  A key is 8 B, so a workgroup's slab of 64 adjacent x (512-B row pieces) stages lines of up to kKeyLineMax = 256
// elements (256 x 512 B = 128 KB of LDS, the budget of edt.hip's 512 x 256 B); a longer line takes the two-sweep path from
// global memory.  The two-sweep argument at the top of edt.hip carries over to keys unchanged: the first sweep leaves g1[j] =
// min_{k<=j} key[k] + (j-k)^2, every term the second forms has the id of its site k and a d2 at least that of the direct term
// key[k] + (i-k)^2, and the direct terms are among them (j = k or j = i), so the lexicographic minimum is the exact one.  The z
// pass overwrites nothing it reads, so above the limit it is a single sweep over all sources.
//
// THE PAIR TABLE is an open-addressed table in device memory, keyed a << 32 | b, filled in two sweeps over the voxels:
//   claim       a thread walks the slots from the key's hash with atomicMin(slot, key): an empty slot (INT64_MAX) or a larger key
//               gives way, and the thread carries the key it displaced onwards from the next slot.  Slots only ever decrease,
//               so every key ends in exactly one slot, on its own probe path, with no empty slot before it: a walk finds it.
//   accumulate  the walk finds the key's slot (plain reads: the claim kernel has ended); atomicAdd the count, atomicMin the
//               key gap_d2 << 32 | voxel index.
// Sums and minima do not depend on order, which slot a key sits in is not part of the result (the caller sorts the claimed
// keys), and a table that was too small says so in status[0] and is discarded: the rows depend on neither capacity nor
// scheduling.  As in k_dstat_reduce a thread merges runs of equal (a, b) along 16 voxels of a row before it touches the table.
#include "edt_pieces.h"
#include "entry_checks.h"
#include "pair_table.h"

namespace cvx {

constexpr nkey_t kNoneKey = (nkey_t)kEdtNone << 32;  // no site: d2 = CVX_EDT_NONE, id 0
constexpr int kKeyLineMax = 256;                     // longest line of keys staged in LDS

__device__ __forceinline__ int key_d2(nkey_t v) { return (int)(v >> 32); }

// ---- x pass ----

__global__ __launch_bounds__(kRowThreads) void k_near_rows(const int* __restrict__ labels, nkey_t* __restrict__ keys, long rows, int W, int nc, int k) {
    extern __shared__ unsigned long long near_row_lds[];
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (kRowThreads / 64) + wave_id();
    const bool live = row < rows;  // a wave past the last row walks the same loops (their barriers) and touches no memory
    const int* s = labels + (live ? row : 0) * W;
    const RowSites sites = edt_row_sites(near_row_lds, nc, [&](int x) { return live && x < W && s[x] >= 1 && s[x] <= k; });
    if (!live) return;
    nkey_t* o = keys + row * W;
    for (int c = 0; c < nc; ++c) {
        const int x = c * 64 + lane;
        if (x >= W) break;
        int left, right;
        edt_row_sides(sites, c, lane, left, right);  // positions of sites of this row: 0 <= left <= x <= right < W
        nkey_t key = kNoneKey;
        if (left >= 0) {
            const int d = x - left;
            key = ((nkey_t)(d * d) << 32) | s[left];  // d < W, and (W-1)^2 < INT32_MAX was checked
        }
        if (right != INT_MAX) {
            const int d = right - x;
            key = min(key, ((nkey_t)(d * d) << 32) | s[right]);  // equal distance: the smaller id
        }
        o[x] = key;
    }
}

// ---- y and z passes ----

// what edt_minplus walks over here: keys.  kTies: a key at the same distance can be smaller (the file header, PRUNING)
struct NearKey {
    typedef nkey_t T;
    static constexpr bool kTies = true;
    __device__ static T none() { return kNoneKey; }
    __device__ static bool is_none(T v) { return key_d2(v) == kEdtNone; }
    __device__ static T step(T v, int dd) { return v + ((nkey_t)dd << 32); }
    __device__ static int d2(T v) { return key_d2(v); }
};

// where a line's results go: back into the keys (y pass), or split into the two planes (z pass, LAST)
struct NearOut {
    nkey_t* keys;
    int* d2;
    int* nearest;
};

template <bool LAST>
__device__ __forceinline__ void near_store(const NearOut& out, long at, const LineGeom& g, int i0, const nkey_t (&best)[kIpt]) {
#pragma unroll
    for (int k = 0; k < kIpt; ++k) {
        if (i0 + k >= g.n) continue;
        const long v = at + (long)(i0 + k) * g.stride;
        if (LAST) {
            out.d2[v] = key_d2(best[k]);
            out.nearest[v] = (int)(best[k] & 0xffffffffLL);
        } else {
            out.keys[v] = best[k];
        }
    }
}

// lines of up to kKeyLineMax elements: staged in LDS (g.n * kSlab keys), every wave then takes blocks of kIpt outputs
template <bool LAST>
__global__ __launch_bounds__(kLineWavesMax * 64) void k_near_lines_lds(NearOut out, LineGeom g) {
    extern __shared__ nkey_t near_line_lds[];
    const int lane = threadIdx.x & 63, wave = wave_id(), waves = blockDim.x >> 6;
    const int x = (int)(blockIdx.x % g.nslab) * kSlab + lane;
    const bool in = x < g.W;
    const long at = (long)(blockIdx.x / g.nslab) * g.ostride + (in ? x : 0);
    for (int j = wave; j < g.n; j += waves) near_line_lds[j * kSlab + lane] = in ? out.keys[at + (long)j * g.stride] : kNoneKey;
    __syncthreads();
    const nkey_t* col = near_line_lds + lane;
    for (int i0 = wave * kIpt; i0 < g.n; i0 += waves * kIpt) {
        nkey_t best[kIpt];
#pragma unroll
        for (int k = 0; k < kIpt; ++k) best[k] = kNoneKey;
        edt_minplus<NearKey, 0>([&](int j) { return col[j * kSlab]; }, in, i0, 0, g.n, best);
        if (in) near_store<LAST>(out, at, g, i0, best);
    }
}

// longer lines.  In place (y pass): the two sweeps of k_edt_lines_long.  LAST (z pass): nothing read is written, one sweep.
template <bool LAST>
__global__ __launch_bounds__(kLineWavesMax * 64) void k_near_lines_long(NearOut out, LineGeom g) {
    const int lane = threadIdx.x & 63, wave = wave_id(), waves = blockDim.x >> 6;
    const int x = (int)(blockIdx.x % g.nslab) * kSlab + lane;
    const bool in = x < g.W;
    const long at = (long)(blockIdx.x / g.nslab) * g.ostride + (in ? x : 0);
    auto f = [&](int j) {
        return in ? __hip_atomic_load(out.keys + at + (long)j * g.stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : kNoneKey;
    };
    const int per_block = waves * kIpt, blocks = (g.n + per_block - 1) / per_block;
    if (LAST) {
        for (int i0 = wave * kIpt; i0 < g.n; i0 += per_block) {
            nkey_t best[kIpt];
#pragma unroll
            for (int k = 0; k < kIpt; ++k) best[k] = kNoneKey;
            edt_minplus<NearKey, 0>(f, in, i0, 0, g.n, best);
            if (in) near_store<true>(out, at, g, i0, best);
        }
        return;
    }
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int t = 0; t < blocks; ++t) {
            const int b = sweep == 0 ? blocks - 1 - t : t;
            const int i0 = b * per_block + wave * kIpt;
            nkey_t best[kIpt];
#pragma unroll
            for (int k = 0; k < kIpt; ++k) best[k] = kNoneKey;
            if (i0 < g.n) {
                if (sweep == 0) edt_minplus<NearKey, 1>(f, in, i0, 0, g.n, best);
                else edt_minplus<NearKey, 2>(f, in, i0, 0, g.n, best);
            }
            __syncthreads();  // every wave has read what this block overwrites
            if (in && i0 < g.n) near_store<false>(out, at, g, i0, best);
        }
        __syncthreads();  // the first sweep's results are what the second reads
    }
}

// ---- the pair table (pair_table.h) over the nearest-instance map ----

// PHASE 0: claim a slot for every pair; PHASE 1: accumulate into the claimed slots
template <int PHASE>
__global__ __launch_bounds__(kCclThreads) void k_pair_reduce(const int* __restrict__ labels_a, const int* __restrict__ nearest_b, const int* __restrict__ d2_b,
                                                              PairTable t, int ka, int thr, Dims dims, int segs) {
    long row;
    int x0, cnt;
    if (!row_piece(dims, segs, row, x0, cnt)) return;
    const long v0 = row * dims.W + x0;
    int a[RV], b[RV], d[RV];
    row_load(labels_a + v0, cnt, a);
    row_load(nearest_b + v0, cnt, b);
    row_load(d2_b + v0, cnt, d);  // past the row's end a, b and d are 0: a is looked at first, and 0 is nobody's
    auto flush = [&](nkey_t key, long long count, nkey_t lo) {
        if (key < 0) return;
        if (PHASE == 0) pair_claim(t, key);
        else pair_accumulate(t, key, count, lo);
    };
    nkey_t run = -1, lo = LLONG_MAX;  // -1: no pair
    long long count = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) {
        const bool hit = a[i] >= 1 && a[i] <= ka && b[i] != 0 && d[i] >= 0 && d[i] <= thr;
        const nkey_t key = hit ? ((nkey_t)a[i] << 32) | (unsigned)b[i] : -1;
        if (key != run) {
            flush(run, count, lo);
            run = key, count = 0, lo = LLONG_MAX;
        }
        if (!hit) continue;
        ++count;
        lo = min(lo, ((nkey_t)d[i] << 32) | (nkey_t)(v0 + i));  // equal d2: the smaller index wins
    }
    flush(run, count, lo);
}

}  // namespace cvx

using namespace cvx;

namespace {

template <bool LAST>
int near_launch_lines(const NearOut& out, int n, long stride, long lines, long ostride, int W, hipStream_t st) {
    const LineGeom g{n, stride, ostride, W, (W + kSlab - 1) / kSlab};
    const int waves = min(kLineWavesMax, (n + kIpt - 1) / kIpt);
    const dim3 grid((unsigned)(lines * g.nslab));  // <= D*H*W
    if (n <= kKeyLineMax) {
        const int lds = n * kSlab * (int)sizeof(nkey_t);
        CVX_HIP(hipFuncSetAttribute((const void*)k_near_lines_lds<LAST>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kKeyLineMax * kSlab * (int)sizeof(nkey_t)));
        hipLaunchKernelGGL(k_near_lines_lds<LAST>, grid, dim3(waves * 64), lds, st, out, g);
    } else {
        hipLaunchKernelGGL(k_near_lines_long<LAST>, grid, dim3(waves * 64), 0, st, out, g);
    }
    return cvx_check_launch();
}

}  // namespace

extern "C" long cvx_nearest_workspace_bytes(int D, int H, int W) {
    long n;
    return extents_fault(D, H, W, kExtentAny, n) ? -1 : n * (long)sizeof(nkey_t);
}

extern "C" int cvx_nearest_instance(const int32_t* labels, long k, int D, int H, int W, int32_t* d2_out, int32_t* nearest_out,
                                    void* workspace, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("nearest_instance", kExtentsRule);
    if (k < 0) return cvx_fail("nearest_instance: k < 0");
    if (n == 0) return 0;
    const long long far = (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1);
    if (far >= INT_MAX) return cvx_fail("nearest_instance: the squared diagonal (D-1)^2 + (H-1)^2 + (W-1)^2 must be below INT32_MAX");
    if (!labels || !d2_out || !nearest_out || !workspace) return cvx_fail("nearest_instance: null pointer");
    if ((((uintptr_t)labels | (uintptr_t)d2_out | (uintptr_t)nearest_out) & 3) || ((uintptr_t)workspace & 7))
        return cvx_fail("nearest_instance: int32 volumes must be 4-B aligned, the workspace 8-B aligned");
    const NearOut out{(nkey_t*)workspace, d2_out, nearest_out};
    const long rows = (long)D * H;
    const int nc = (W + 63) / 64;
    hipLaunchKernelGGL(k_near_rows, dim3((unsigned)((rows + kRowThreads / 64 - 1) / (kRowThreads / 64))), dim3(kRowThreads), edt_row_lds_bytes(nc), st, labels,
                       out.keys, rows, W, nc, clamp_int(k));
    int rc = cvx_check_launch();
    if (rc) return rc;
    if (H > 1 && (rc = near_launch_lines<false>(out, H, W, D, (long)H * W, W, st))) return rc;  // y: one line per (z, x)
    return near_launch_lines<true>(out, D, (long)H * W, H, W, W, st);  // z: one line per (y, x); also splits the keys when D == 1
}

extern "C" int cvx_instance_pair_contacts(const int32_t* labels_a, long ka, const int32_t* nearest_b, const int32_t* d2_b, int threshold_d2,
                                          int D, int H, int W, int64_t* table, long capacity, int64_t* status, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("instance_pair_contacts", kExtentsRule);
    if (ka < 0) return cvx_fail("instance_pair_contacts: ka < 0");
    PairTable t;
    if (!pair_table(table, capacity, status, t)) return cvx_fail("instance_pair_contacts: capacity must be a power of two in 1..2^31");
    if (!table || !status || (n > 0 && (!labels_a || !nearest_b || !d2_b))) return cvx_fail("instance_pair_contacts: null pointer");
    if ((((uintptr_t)table | (uintptr_t)status) & 7) || (((uintptr_t)labels_a | (uintptr_t)nearest_b | (uintptr_t)d2_b) & 3))
        return cvx_fail("instance_pair_contacts: misaligned pointer");
    hipLaunchKernelGGL(k_pair_init, dim3(blocks_of(capacity)), dim3(kCclThreads), 0, st, t);
    int rc = cvx_check_launch();
    if (rc || n == 0 || ka == 0) return rc;
    const int segs = (W + RV - 1) / RV;
    const dim3 grid(blocks_of((long)D * H * segs));
    const Dims d = ccl_dims(D, H, W);
    hipLaunchKernelGGL(k_pair_reduce<0>, grid, dim3(kCclThreads), 0, st, labels_a, nearest_b, d2_b, t, clamp_int(ka), threshold_d2, d, segs);
    if ((rc = cvx_check_launch())) return rc;
    hipLaunchKernelGGL(k_pair_reduce<1>, grid, dim3(kCclThreads), 0, st, labels_a, nearest_b, d2_b, t, clamp_int(ka), threshold_d2, d, segs);
    return cvx_check_launch();
}

extern "C" int cvx_instance_pair_rows(const int64_t* table, long capacity, const int64_t* order, long p, int64_t* rows, hipStream_t st) {
    PairTable t;
    if (!pair_table((int64_t*)table, capacity, nullptr, t)) return cvx_fail("instance_pair_rows: capacity must be a power of two in 1..2^31");
    if (p < 0 || p > capacity) return cvx_fail("instance_pair_rows: p must lie in 0..capacity");
    if (p == 0) return 0;
    if (!table || !order || !rows) return cvx_fail("instance_pair_rows: null pointer");
    if (((uintptr_t)table | (uintptr_t)order | (uintptr_t)rows) & 7) return cvx_fail("instance_pair_rows: misaligned pointer");
    hipLaunchKernelGGL(k_pair_rows, dim3(blocks_of(p)), dim3(kCclThreads), 0, st, t, (const long long*)order, p, (long long*)rows);
    return cvx_check_launch();
}
