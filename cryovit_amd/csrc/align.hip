// Alignment of oriented subtomograms about their axis (`--extract-align`): the boxes of cvx_subtomo_extract resampled on rings
// around the box z axis, and the circular correlation of every particle with a reference over the in-plane angle and the shift
// along the axis.  The definition (fixed point, the four taps, q, the ring weight) is in include/cryovit_hip.h.  Integers only;
// every table element is stored plainly by one thread, so two calls give the same bits.
//
// POLAR.  k_subtomo_polar, one workgroup per (particle, slab), threads over (ring, step).  Every index is clamped, so no trig
//   table makes an access leave the box.
// MOMENTS.  k_subtomo_moments, one wave per (particle, slab), lanes over (ring, step), a wave sum.
// CORRELATE.  k_subtomo_correlate<T>, one workgroup of four waves per particle; it makes all 2 S + 1 shifts, so that a q row read
//   from LDS meets 2 S + 1 reference rows.
//   1. per ring r and tile of kAlignRows q slabs: q = min(255, (polar + 2^20) >> 21) goes to LDS as 16-bit values, every row
//      twice in a row (the rotation needs no modulo) and in two copies, the second moved by one element: lane k reads its
//      window q[k .. k + T - 1] as T/2 aligned dwords from copy k & 1.  The second copy starts 16 dwords past a multiple of 32,
//      so the even and the odd lanes of a 32-lane half read disjoint banks.
//   2. a wave takes q rows of the tile; lane k (k and k + 64 are two waves' work at T = 128; at T = 32 the upper half wave
//      repeats the lower one and stores nothing) keeps the window in T/2 registers.  Per shift d the reference row z' = zq - d
//      comes through the scalar cache (its address is the same in every lane) and one 16-bit dot2 makes two MACs.
//      The partial over t of one (slab, ring) is an int32: T * 255 * 32768 <= 2^30.  It is folded into an int64 per shift
//      with the ring weight: (2 zh + 1) * rmax (rmax + 1) / 2 * 2^30 <= 127 * 2016 * 2^30 < 2^49.
//   3. the waves' int64 sums meet in LDS by 64-bit integer adds (any order, the same bits) and go out by plain vector stores.
#include "subtomo_stack.h"

namespace cvx {

constexpr int kAlignRows = 16;                               // q slabs per LDS tile
constexpr int kAlignCand = 2 * CVX_ALIGN_SHIFT_MAX + 1;      // shifts d = -S..S
constexpr long long kQHalf = 1ll << 20;

typedef short short2v __attribute__((ext_vector_type(2)));

// q of the definition; a polar value outside [0, 255 * 2^21] (none that cvx_align_polar writes) is brought into 0..255
__device__ __forceinline__ int polar_q(int v) {
    const long long q = ((long long)v + kQHalf) >> 21;
    return (int)(q < 0 ? 0 : q > 255 ? 255 : q);
}

__global__ __launch_bounds__(kCclThreads) void k_subtomo_polar(const int* __restrict__ stack, int box, const int* __restrict__ trig, int T,
                                                               int rmax, int* __restrict__ polar) {
    const long s = blockIdx.x;  // p * box + z
    const int* slab = stack + s * box * box;
    int* out = polar + s * rmax * T;
    const long long c7 = (long long)(box / 2) << 7;
    for (int e = threadIdx.x; e < rmax * T; e += kCclThreads) {
        const int r = e / T + 1, t = e % T;
        const long long py7 = c7 + (((long long)r * trig[2 * t]) >> 7), px7 = c7 + (((long long)r * trig[2 * t + 1]) >> 7);
        const long long iy = py7 >> 7, ix = px7 >> 7;
        const int fy = (int)(py7 & 127), fx = (int)(px7 & 127);
        const int y0 = (int)min(max(iy, 0ll), (long long)box - 1), y1 = (int)min(max(iy + 1, 0ll), (long long)box - 1);
        const int x0 = (int)min(max(ix, 0ll), (long long)box - 1), x1 = (int)min(max(ix + 1, 0ll), (long long)box - 1);
        const long long a = (long long)slab[y0 * box + x0] * (128 - fx) + (long long)slab[y0 * box + x1] * fx;
        const long long b = (long long)slab[y1 * box + x0] * (128 - fx) + (long long)slab[y1 * box + x1] * fx;
        out[e] = (int)((a * (128 - fy) + b * fy) >> 14);
    }
}

// one wave per (particle, slab)
__global__ __launch_bounds__(kCclThreads) void k_subtomo_moments(const int* __restrict__ polar, long slabs, int T, int rmax,
                                                                 long long* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * (kCclThreads / 64) + (threadIdx.x >> 6);
    if (s >= slabs) return;  // the whole wave alike
    const int* rows = polar + s * rmax * T;
    long long m1 = 0, m2 = 0;  // <= 2016 * 128 * 255^2 < 2^35
    for (int e = lane; e < rmax * T; e += 64) {
        const long long r = e / T + 1, q = polar_q(rows[e]);
        m1 += r * q;
        m2 += r * q * q;
    }
    m1 = wave_sum(m1);
    m2 = wave_sum(m2);
    if (lane == 0) {
        moments[2 * s] = m1;
        moments[2 * s + 1] = m2;
    }
}

template <int T>
__global__ __launch_bounds__(kCclThreads) void k_subtomo_correlate(const int* __restrict__ polar, int box, int rmax,
                                                                   const int* __restrict__ ref, int zh, int S,
                                                                   long long* __restrict__ corr) {
    constexpr int kParts = T > 64 ? T / 64 : 1;   // 64-lane parts of k
    constexpr int kWaves = kCclThreads / 64;
    constexpr int kCopy = T + 16;                 // dwords from copy 0 to copy 1 of a row
    constexpr int kRow = 2 * T + 32;              // dwords per LDS row
    static_assert(kWaves % kParts == 0 && T % 32 == 0, "a wave keeps one part of k");
    __shared__ unsigned tile[kAlignRows * kRow];
    __shared__ unsigned long long total[kAlignCand * T];
    const long p = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nd = 2 * S + 1, nq = 2 * zh + nd;  // the q slabs zq = 0..nq-1 are the slabs box/2 - zh - S + zq: inside the box
    const int k = T >= 64 ? (wave % kParts) * 64 + lane : lane & (T - 1);
    for (int i = threadIdx.x; i < nd * T; i += kCclThreads) total[i] = 0;
    long long acc[kAlignCand];
#pragma unroll
    for (int dd = 0; dd < kAlignCand; ++dd) acc[dd] = 0;
    for (int r = 1; r <= rmax; ++r) {
        for (int zq0 = 0; zq0 < nq; zq0 += kAlignRows) {
            const int rows = min(kAlignRows, nq - zq0);
            __syncthreads();  // the tile's readers are done
            unsigned short* t16 = (unsigned short*)tile;
            for (int e = threadIdx.x; e < rows * T; e += kCclThreads) {
                const int row = e / T, t = e % T;
                const long slab = p * box + box / 2 - zh - S + zq0 + row;
                const unsigned short q = (unsigned short)polar_q(polar[(slab * rmax + r - 1) * T + t]);
                unsigned short* c0 = t16 + row * (2 * kRow);
                unsigned short* c1 = c0 + 2 * kCopy;
                const int j = (t + T - 1) % T;  // copy 1 [j] = q[j + 1]
                c0[t] = q;
                c0[t + T] = q;
                c1[j] = q;
                c1[j + T] = q;
            }
            __syncthreads();
            for (int row = wave / kParts; row < rows; row += kWaves / kParts) {
                const unsigned* w = tile + row * kRow + (k & 1) * kCopy + (k >> 1);  // (k >> 1) + T/2 - 1 <= T - 1
                unsigned win[T / 2];
#pragma unroll
                for (int j = 0; j < T / 2; ++j) win[j] = w[j];
                const int zq = zq0 + row;
#pragma unroll
                for (int dd = 0; dd < kAlignCand; ++dd) {
                    const int zr = zq - dd;  // the reference slab that meets this q slab at the shift dd - S
                    if (dd < nd && zr >= 0 && zr <= 2 * zh) {  // the whole wave alike
                        const int* rr = ref + ((long)zr * rmax + r - 1) * (T / 2);
                        int part = 0;  // |part| <= T * 255 * 32768 <= 2^30
#pragma unroll
                        for (int j = 0; j < T / 2; ++j)
                            part = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, win[j]), __builtin_bit_cast(short2v, rr[j]), part, false);
                        acc[dd] += (long long)r * part;  // < 2^49 in all (above)
                    }
                }
            }
        }
    }
    __syncthreads();  // total is zero everywhere
    if (lane < T) {
#pragma unroll
        for (int dd = 0; dd < kAlignCand; ++dd)
            if (dd < nd) atomicAdd(&total[dd * T + k], (unsigned long long)acc[dd]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nd * T; i += kCclThreads) corr[p * nd * T + i] = (long long)total[i];
}

}  // namespace cvx

using namespace cvx;

namespace {

// what both entries refuse about T and rmax, after stack_fault
const char* polar_fault(int box, int T, int rmax) {
    if (T != 32 && T != 64 && T != 128) return "T must be 32, 64 or 128";
    if (rmax < 1 || rmax > box / 2 - 1) return "rmax must lie in [1, box/2 - 1]";
    return nullptr;
}

}  // namespace

extern "C" int cvx_align_polar(const int32_t* stack, long P, int box, const int32_t* trig, int T, int rmax, int32_t* polar, hipStream_t st) {
    long vox = 0;
    if (const char* why = stack_fault(P, box, vox)) return cvx_fail("align_polar", why);
    if (const char* why = polar_fault(box, T, rmax)) return cvx_fail("align_polar", why);
    if (P == 0) return 0;
    if (!stack || !trig || !polar) return cvx_fail("align_polar", "null pointer");
    if (((uintptr_t)stack | (uintptr_t)trig | (uintptr_t)polar) & 3) return cvx_fail("align_polar", "misaligned pointer");
    hipLaunchKernelGGL(k_subtomo_polar, dim3((unsigned)(P * box)), dim3(kCclThreads), 0, st, stack, box, trig, T, rmax, polar);  // <= 2^27 blocks
    return cvx_check_launch();
}

extern "C" int cvx_align_correlate(const int32_t* polar, long P, int box, int T, int rmax, const int16_t* ref, int zh, int shift, int64_t* corr,
                                     int64_t* moments, hipStream_t st) {
    long vox = 0;
    if (const char* why = stack_fault(P, box, vox)) return cvx_fail("align_correlate", why);
    if (const char* why = polar_fault(box, T, rmax)) return cvx_fail("align_correlate", why);
    if (zh < 0) return cvx_fail("align_correlate", "zh < 0");
    if (shift < 0 || shift > CVX_ALIGN_SHIFT_MAX) return cvx_fail("align_correlate", "shift must lie in [0, 8]");
    if (zh + shift > box / 2 - 1) return cvx_fail("align_correlate", "zh + shift must be <= box/2 - 1");
    if (P == 0) return 0;
    if (!polar || !ref || !corr || !moments) return cvx_fail("align_correlate", "null pointer");
    // ref is read two int16 at a time: a row holds an even number of them, so the table only has to start at a multiple of 4
    if ((((uintptr_t)polar | (uintptr_t)ref) & 3) || (((uintptr_t)corr | (uintptr_t)moments) & 7))
        return cvx_fail("align_correlate", "misaligned pointer");
    const long slabs = P * box;  // <= 2^27 waves
    hipLaunchKernelGGL(k_subtomo_moments, dim3(wave_blocks_of(slabs)), dim3(kCclThreads), 0, st, polar, slabs, T, rmax, (long long*)moments);
    if (const int rc = cvx_check_launch()) return rc;
    const int* ref2 = (const int*)ref;
    long long* out = (long long*)corr;
    if (T == 32)
        hipLaunchKernelGGL(k_subtomo_correlate<32>, dim3((unsigned)P), dim3(kCclThreads), 0, st, polar, box, rmax, ref2, zh, shift, out);
    else if (T == 64)
        hipLaunchKernelGGL(k_subtomo_correlate<64>, dim3((unsigned)P), dim3(kCclThreads), 0, st, polar, box, rmax, ref2, zh, shift, out);
    else
        hipLaunchKernelGGL(k_subtomo_correlate<128>, dim3((unsigned)P), dim3(kCclThreads), 0, st, polar, box, rmax, ref2, zh, shift, out);
    return cvx_check_launch();
}
