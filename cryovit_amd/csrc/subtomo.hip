// Oriented subtomograms (`--extract`): a box of B^3 voxels around every particle, rotated by the particle's matrix and sampled
// trilinearly from the uint8 tomogram, the sums of the boxes and the density profile along the box z axis.  The definition (fixed
// point, the eight taps, the replicated border, the refusal of a matrix that is no rotation) is in include/cryovit_hip.h.
// Integers only; the extraction stores plainly, the sums are 64-bit integer atomics, so two calls give the same bits.
//
// EXTRACT.  k_subtomo_extract, one workgroup per (particle, 16x16x16 block of the box; ragged where 16 does not divide B).
//   1. the twelve table entries; a particle whose matrix fails the span test (below) gets zeros.
//   2. s16 is linear in the box offset, so its extremes over the block lie at the block's 8 corners: per source axis
//      lo = min floor(s16 / 2^16), hi = max floor(s16 / 2^16) + 1 (the upper tap), both clamped to the volume.  The brick
//      [lo_z..hi_z][lo_y..hi_y][lo_x..hi_x] of bytes goes to LDS, consecutive threads along source x.
//   3. a thread takes the box voxels (t_z, t_y, t_x) with t_y, t_x from its index and t_z = 0..15: the position relative to the
//      brick's unclamped origin fits 32 bits, the eight taps come from LDS at clamp(idx + d) - lo.
// THE SPAN TEST.  span_a = 15 (|m[a][0]| + |m[a][1]| + |m[a][2]|) bounds max s16 - min s16 over a block, so a block touches at
//   most ceil(span_a / 2^16) + 2 indices of axis a (the floors of two numbers `span` apart differ by at most ceil(span), plus the
//   upper tap).  A particle is refused when that exceeds the brick (30, 30, 32).  A rotation's rows have length 1, so the sum of
//   their absolute values is at most sqrt 3 and the need is 28.  The test depends on the matrix alone: not on the volume, the
//   centre, the block or the launch.  k_subtomo_refused counts the refused particles, one workgroup, a plain store.
// SUM.  k_subtomo_sum: one thread per box voxel and segment of kSumSeg particles; the running sum of a group stays in a register
//   and goes to the table by one 64-bit atomic add when the group changes and at the end: one per thread where all share a group.
// PROFILE.  k_subtomo_profile: one wave per (particle, z slab), lanes over the slab's B^2 voxels inside the disc, a wave sum.
#include "subtomo_stack.h"

namespace cvx {

constexpr int kSubBlock = 16;                           // box voxels per block and axis
constexpr int kBrickZ = 30, kBrickY = 30, kBrickX = 32;  // the LDS brick, 28 800 bytes
constexpr int kSumSeg = 32;                              // particles per thread of k_subtomo_sum
constexpr int kBoxMin = CVX_SUBTOMO_BOX_MIN, kBoxMax = CVX_SUBTOMO_BOX_MAX, kSubCols = CVX_SUBTOMO_COLS;

// does the matrix (table entries 3..11) pass the span test?
__device__ __forceinline__ bool subtomo_fits(const int* __restrict__ t) {
    const int brick[3] = {kBrickZ, kBrickY, kBrickX};
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        long long sum = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long m = t[3 + 3 * a + j];
            sum += m < 0 ? -m : m;
        }
        const long long need = (((kSubBlock - 1) * sum + 65535) >> 16) + 2;
        ok = ok && need <= brick[a];
    }
    return ok;
}

__global__ __launch_bounds__(kCclThreads) void k_subtomo_extract(const unsigned char* __restrict__ vol, int D, int H, int W,
                                                                 const int* __restrict__ table, int box, int nb, int* __restrict__ out) {
    __shared__ unsigned char brick[kBrickZ * kBrickY * kBrickX];
    const int b = blockIdx.x % (nb * nb * nb);
    const long p = blockIdx.x / (nb * nb * nb);
    const int* t = table + p * kSubCols;
    const int bo[3] = {b / (nb * nb) * kSubBlock, b / nb % nb * kSubBlock, b % nb * kSubBlock};  // the block's first box voxel
    int n[3];                                                                                    // its voxels per axis
#pragma unroll
    for (int j = 0; j < 3; ++j) n[j] = min(kSubBlock, box - bo[j]);
    const int tx = threadIdx.x % kSubBlock, ty = threadIdx.x / kSubBlock;
    const bool mine = ty < n[1] && tx < n[2];
    const long at = ((p * box + bo[0]) * box + bo[1] + ty) * box + bo[2] + tx;  // of this thread's first voxel; inside out iff mine
    if (!subtomo_fits(t)) {  // the whole workgroup alike
        for (int tz = 0; mine && tz < n[0]; ++tz) out[at + (long)tz * box * box] = 0;
        return;
    }
    const int ext[3] = {D, H, W};
    int m[3][3], lo[3], lo_c[3], e[3], rel0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        long long base = (long long)t[a] << 8;  // s16 of the block's first voxel
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m[a][j] = t[3 + 3 * a + j];
            base += (long long)m[a][j] * (bo[j] - box / 2);
        }
        long long s_min = base, s_max = base;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long step = (long long)m[a][j] * (n[j] - 1);
            s_min += step < 0 ? step : 0;
            s_max += step > 0 ? step : 0;
        }
        // after the span test |idx| < 2^24: |c| < 2^31 in Q8 and the offsets add less than 2^7 * 30
        lo[a] = (int)(s_min >> 16);
        const int hi = (int)(s_max >> 16) + 1;
        lo_c[a] = min(max(lo[a], 0), ext[a] - 1);
        e[a] = min(max(hi, 0), ext[a] - 1) - lo_c[a] + 1;  // <= hi - lo + 1 <= the need of the span test
        rel0[a] = (int)(base - ((long long)lo[a] << 16));  // 0 <= rel0 + the steps below < 32 * 2^16
    }
    // 2. the brick, rows along source x
    const int cells = e[0] * e[1] * e[2];
    for (int c = threadIdx.x; c < cells; c += kCclThreads) {
        const int x = c % e[2], y = c / e[2] % e[1], z = c / (e[2] * e[1]);
        brick[(z * kBrickY + y) * kBrickX + x] = vol[((long)(lo_c[0] + z) * H + lo_c[1] + y) * W + lo_c[2] + x];
    }
    __syncthreads();
    if (!mine) return;
    // 3. the taps
    int row[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) row[a] = rel0[a] + m[a][1] * ty + m[a][2] * tx;
    for (int tz = 0; tz < n[0]; ++tz) {
        int i0[3], i1[3], f[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int s = (row[a] + m[a][0] * tz) >> 9;  // lo << 16 is a multiple of 2^9: the floor is that of s16 >> 9
            const int idx = lo[a] + (s >> 7);
            f[a] = s & 127;
            i0[a] = min(max(idx, 0), ext[a] - 1) - lo_c[a];
            i1[a] = min(max(idx + 1, 0), ext[a] - 1) - lo_c[a];
        }
        const int z0 = i0[0] * kBrickY, z1 = i1[0] * kBrickY;
        auto line = [&](int zy) {  // along x
            const unsigned char* q = brick + zy * kBrickX;
            return q[i0[2]] * (128 - f[2]) + q[i1[2]] * f[2];
        };
        const int a0 = line(z0 + i0[1]) * (128 - f[1]) + line(z0 + i1[1]) * f[1];
        const int a1 = line(z1 + i0[1]) * (128 - f[1]) + line(z1 + i1[1]) * f[1];
        out[at + (long)tz * box * box] = a0 * (128 - f[0]) + a1 * f[0];
    }
}

// *status = the particles that fail the span test: one workgroup
__global__ __launch_bounds__(kCclThreads) void k_subtomo_refused(const int* __restrict__ table, long P, long long* __restrict__ status) {
    __shared__ long long part[kCclThreads / 64];
    long long mine = 0;
    for (long p = threadIdx.x; p < P; p += kCclThreads) mine += !subtomo_fits(table + p * kSubCols);
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long all = 0;
        for (int w = 0; w < kCclThreads / 64; ++w) all += part[w];
        *status = all;
    }
}

__global__ __launch_bounds__(kCclThreads) void k_subtomo_sum(const int* __restrict__ stack, long P, long vox, long vblocks,
                                                             const int* __restrict__ group, int G, long long* __restrict__ sums) {
    const long v = (blockIdx.x % vblocks) * kCclThreads + threadIdx.x;
    const long p0 = (blockIdx.x / vblocks) * kSumSeg, p1 = min(p0 + kSumSeg, P);
    if (v >= vox) return;
    int cur = -1;
    long long acc = 0;
    for (long p = p0; p < p1; ++p) {
        const int g = group[p];  // the same in every lane
        if (g < 0 || g >= G) continue;
        if (g != cur) {
            if (cur >= 0) atomicAdd((unsigned long long*)(sums + cur * vox + v), (unsigned long long)acc);
            cur = g;
            acc = 0;
        }
        acc += stack[p * vox + v];
    }
    if (cur >= 0) atomicAdd((unsigned long long*)(sums + cur * vox + v), (unsigned long long)acc);
}

// one wave per (particle, slab)
__global__ __launch_bounds__(kCclThreads) void k_subtomo_profile(const int* __restrict__ stack, long slabs, int box, long radius2,
                                                                 long long* __restrict__ profile) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * (kCclThreads / 64) + (threadIdx.x >> 6);
    if (s >= slabs) return;  // the whole wave alike
    const int* slab = stack + s * box * box;
    long long sum = 0;
    for (int c = lane; c < box * box; c += 64) {
        const int oy = c / box - box / 2, ox = c % box - box / 2;
        if ((long)(oy * oy + ox * ox) <= radius2) sum += slab[c];
    }
    sum = wave_sum(sum);
    if (lane == 0) profile[s] = sum;
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_subtomo_extract(const uint8_t* vol, int D, int H, int W, const int32_t* table, long P, int box, int32_t* out, int64_t* status,
                                   hipStream_t st) {
    long n = 0, vox = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("subtomo_extract", why);
    if (const char* why = stack_fault(P, box, vox)) return cvx_fail("subtomo_extract", why);
    if (P == 0 || n == 0) return 0;  // nothing to sample from, or nobody to sample for: out and status stay as they are
    if (!vol || !table || !out || !status) return cvx_fail("subtomo_extract", "null pointer");
    if ((((uintptr_t)table | (uintptr_t)out) & 3) || ((uintptr_t)status & 7)) return cvx_fail("subtomo_extract", "misaligned pointer");
    const int nb = (box + kSubBlock - 1) / kSubBlock;  // <= 8: P * nb^3 <= 2^29 blocks
    hipLaunchKernelGGL(k_subtomo_extract, dim3((unsigned)(P * nb * nb * nb)), dim3(kCclThreads), 0, st, vol, D, H, W, table, box, nb, out);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_subtomo_refused, dim3(1), dim3(kCclThreads), 0, st, table, P, (long long*)status);
    return cvx_check_launch();
}

extern "C" int cvx_subtomo_sum(const int32_t* stack, long P, int box, const int32_t* group, int G, int64_t* sums, hipStream_t st) {
    long vox = 0;
    if (const char* why = stack_fault(P, box, vox)) return cvx_fail("subtomo_sum", why);
    if (G < 1) return cvx_fail("subtomo_sum", "G < 1");
    if (P == 0) return 0;
    if (!stack || !group || !sums) return cvx_fail("subtomo_sum", "null pointer");
    if ((((uintptr_t)stack | (uintptr_t)group) & 3) || ((uintptr_t)sums & 7)) return cvx_fail("subtomo_sum", "misaligned pointer");
    const long vblocks = (vox + kCclThreads - 1) / kCclThreads, segments = (P + kSumSeg - 1) / kSumSeg;  // <= 2^13 * 2^15 blocks
    hipLaunchKernelGGL(k_subtomo_sum, dim3((unsigned)(vblocks * segments)), dim3(kCclThreads), 0, st, stack, P, vox, vblocks, group, G,
                       (long long*)sums);
    return cvx_check_launch();
}

extern "C" int cvx_subtomo_profile(const int32_t* stack, long P, int box, long radius2, int64_t* profile, hipStream_t st) {
    long vox = 0;
    if (const char* why = stack_fault(P, box, vox)) return cvx_fail("subtomo_profile", why);
    if (radius2 < 0) return cvx_fail("subtomo_profile", "radius2 < 0");
    if (P == 0) return 0;
    if (!stack || !profile) return cvx_fail("subtomo_profile", "null pointer");
    if (((uintptr_t)stack & 3) || ((uintptr_t)profile & 7)) return cvx_fail("subtomo_profile", "misaligned pointer");
    const long slabs = P * box;  // <= 2^27 waves
    hipLaunchKernelGGL(k_subtomo_profile, dim3(wave_blocks_of(slabs)), dim3(kCclThreads), 0, st, stack, slabs, box, radius2, (long long*)profile);
    return cvx_check_launch();
}
