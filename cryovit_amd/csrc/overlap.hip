// The contingency table between two instance volumes (`cryovit evaluate --instance-metrics`): per pair (a, b) the voxels v with
// a = labels_a[v] in 1..ka and b = labels_b[v] in 1..kb, and the smallest linear index of such a voxel.  The table is the pair
// table of pair_table.h, filled as nearest.hip fills it: a claim pass, then an accumulate pass.  Integers only: counts are sums
// and the index is a minimum, so the rows depend on neither scheduling, the size of the LDS table below, nor capacity.
//
// WHY NOT k_pair_reduce.  That pass goes from a thread's 16 voxels straight to 64-bit global atomics, which suits contacts: few
// voxels lie near another label.  Here nearly every foreground voxel hits and a segmentation has a few dozen instances, so the
// global atomics of a whole volume would land on a few dozen addresses.  Three reductions come before them:
//   thread     a thread walks kOvPieces row pieces of RV voxels (the same x, kCclThreads / segs rows apart: mostly the same
//              instance) and keeps ONE pending (key, count, lowest index).  Background does not end a run; a different key does, and
//              the run it ends goes to the workgroup's table.
//   wave       at the end, when every lane's pending key is the same, or none, one wave_sum, one minimum and one insert per wave.
//   workgroup  an open-addressed table of kOvSlots (key, count, lowest index) in LDS, filled with LDS integer atomics (compare-and-
//              swap on the key, add, min), at most kOvProbes slots tried per insert.  It is flushed once, one slot per thread, by
//              pair_claim / pair_accumulate.  A key that finds no slot among its kOvProbes goes straight to the global table.
// A workgroup covers kCclThreads * kOvPieces * RV = 32768 voxels, so a count and an index both fit 32 bits in LDS.
#include "entry_checks.h"
#include "pair_table.h"

namespace cvx {

constexpr int kOvPieces = 8;   // row pieces per thread
constexpr int kOvSlots = 256;  // LDS table: one slot per thread at the flush; 256 * 16 B = 4 KB
constexpr int kOvProbes = 8;   // slots tried before a key goes to the global table
constexpr unsigned kOvNoIndex = 0xffffffffu;  // no voxel index reaches it: D*H*W <= 2^31 - 2
static_assert(kOvSlots == kCclThreads, "the flush gives every thread one slot");
static_assert((long)kCclThreads * kOvPieces * RV < (1L << 31), "a workgroup's count fits the 32-bit LDS counter");

struct OvLds {
    nkey_t keys[kOvSlots];  // kPairEmpty or a << 32 | b
    unsigned count[kOvSlots];
    unsigned lo[kOvSlots];  // smallest linear voxel index
};

// into the workgroup's table; false: no slot among the key's kOvProbes (the caller goes to the global table)
template <int PHASE>
__device__ __forceinline__ bool ov_lds_add(OvLds& l, nkey_t key, unsigned count, unsigned lo) {
    unsigned s = (unsigned)(((unsigned long)key * 0x9E3779B97F4A7C15ul) >> 56) & (kOvSlots - 1);
    for (int probes = 0; probes < kOvProbes; ++probes, s = (s + 1) & (kOvSlots - 1)) {
        // a slot is written once: a plain read that shows a key is final, one that shows it empty is settled by the swap
        nkey_t seen = *(volatile nkey_t*)(l.keys + s);
        if (seen == kPairEmpty) seen = (nkey_t)atomicCAS((unsigned long long*)(l.keys + s), (unsigned long long)kPairEmpty, (unsigned long long)key);
        if (seen != kPairEmpty && seen != key) continue;
        if (PHASE == 1) {
            atomicAdd(l.count + s, count);
            atomicMin(l.lo + s, lo);
        }
        return true;
    }
    return false;
}

template <int PHASE>
__device__ __forceinline__ void ov_add(OvLds& l, const PairTable& t, nkey_t key, unsigned count, unsigned lo) {
    if (ov_lds_add<PHASE>(l, key, count, lo)) return;
    if (PHASE == 0) pair_claim(t, key);
    else pair_accumulate(t, key, (long long)count, (nkey_t)lo);
}

// the key, when every lane that holds one (cur >= 0) holds the same; else -1.  wave_single_id of voxel_rows.h on 64-bit keys
__device__ __forceinline__ nkey_t wave_single_key(nkey_t cur) {
    const unsigned long long has = __ballot(cur >= 0);
    const nkey_t first = has ? __shfl(cur, __ffsll((long long)has) - 1) : -1;
    return __all(cur < 0 || cur == first) ? first : -1;
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// PHASE 0: claim a slot for every pair; PHASE 1: accumulate into the claimed slots.  No thread leaves early: all meet at the
// barriers and the wave reductions.
template <int PHASE>
__global__ __launch_bounds__(kCclThreads) void k_overlap_reduce(const int* __restrict__ labels_a, const int* __restrict__ labels_b, PairTable t, int ka,
                                                                 int kb, int W, int segs, long pieces) {
    __shared__ OvLds l;
    l.keys[threadIdx.x] = kPairEmpty;
    l.count[threadIdx.x] = 0;
    l.lo[threadIdx.x] = kOvNoIndex;
    __syncthreads();
    nkey_t cur = -1;  // -1: no pair pending
    unsigned count = 0, lo = kOvNoIndex;
    const long p0 = (long)blockIdx.x * (kCclThreads * kOvPieces) + threadIdx.x;
    for (int it = 0; it < kOvPieces; ++it) {
        const long p = p0 + (long)it * kCclThreads;
        if (p >= pieces) break;  // the pieces of a thread ascend
        const long row = p / segs;
        const int x0 = (int)(p % segs) * RV, cnt = min(RV, W - x0);
        const long v0 = row * W + x0;  // v0 + cnt <= D*H*W
        int a[RV], b[RV];
        row_load(labels_a + v0, cnt, a);
        row_load(labels_b + v0, cnt, b);  // past the row's end a and b are 0, nobody's
#pragma unroll
        for (int i = 0; i < RV; ++i) {
            if (!(a[i] >= 1 && a[i] <= ka && b[i] >= 1 && b[i] <= kb)) continue;
            const nkey_t key = ((nkey_t)a[i] << 32) | (unsigned)b[i];
            if (key != cur) {
                if (cur >= 0) ov_add<PHASE>(l, t, cur, count, lo);
                cur = key, count = 0, lo = (unsigned)(v0 + i);  // indices ascend along a thread's walk: the first is the lowest
            }
            ++count;
        }
    }
    const nkey_t single = wave_single_key(cur);
    if (single >= 0) {
        const unsigned n = (unsigned)wave_sum((int)count), first = wave_min(lo);
        if ((threadIdx.x & 63) == 0) ov_add<PHASE>(l, t, single, n, first);
    } else if (cur >= 0) {
        ov_add<PHASE>(l, t, cur, count, lo);
    }
    __syncthreads();
    const nkey_t key = l.keys[threadIdx.x];
    if (key == kPairEmpty) return;
    if (PHASE == 0) pair_claim(t, key);
    else pair_accumulate(t, key, (long long)l.count[threadIdx.x], (nkey_t)l.lo[threadIdx.x]);
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_overlap_instances(const int32_t* labels_a, long ka, const int32_t* labels_b, long kb, int D, int H, int W, int64_t* table,
                                     long capacity, int64_t* status, hipStream_t st) {
    long n;
    if (extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("instance_overlaps", kExtentsRule);
    if (ka < 0 || kb < 0) return cvx_fail("instance_overlaps: ka < 0 or kb < 0");
    PairTable t;
    if (!pair_table(table, capacity, status, t)) return cvx_fail("instance_overlaps: capacity must be a power of two in 1..2^31");
    if (!table || !status || (n > 0 && (!labels_a || !labels_b))) return cvx_fail("instance_overlaps: null pointer");
    if ((((uintptr_t)table | (uintptr_t)status) & 7) || (((uintptr_t)labels_a | (uintptr_t)labels_b) & 3))
        return cvx_fail("instance_overlaps: misaligned pointer");
    hipLaunchKernelGGL(k_pair_init, dim3(blocks_of(capacity)), dim3(kCclThreads), 0, st, t);
    int rc = cvx_check_launch();
    if (rc || n == 0 || ka == 0 || kb == 0) return rc;
    const int segs = (W + RV - 1) / RV;
    const long pieces = (long)D * H * segs;  // <= D*H*W
    const long per_group = (long)kCclThreads * kOvPieces;
    const dim3 grid((unsigned)((pieces + per_group - 1) / per_group));
    hipLaunchKernelGGL(k_overlap_reduce<0>, grid, dim3(kCclThreads), 0, st, labels_a, labels_b, t, clamp_int(ka), clamp_int(kb), W, segs, pieces);
    if ((rc = cvx_check_launch())) return rc;
    hipLaunchKernelGGL(k_overlap_reduce<1>, grid, dim3(kCclThreads), 0, st, labels_a, labels_b, t, clamp_int(ka), clamp_int(kb), W, segs, pieces);
    return cvx_check_launch();
}
