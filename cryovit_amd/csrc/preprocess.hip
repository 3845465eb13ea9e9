// Raw tomogram -> uint8 in [0, 255] (`cryovit preprocess`, `features --normalize`): box sums over kz x k x k blocks, per-slice
// moments, exact order statistics by radix select, and the quantising pass.  A volume is one of six element types (CVX_VOL_*: the
// four integer and the float32 types a reconstruction program writes, plus the int32 sums of the bin pass); every pass after the
// bin pass reads the type it is given, so an unbinned volume is never copied.  All indices are 64-bit.
//
// ACCESS.  Moments, select and quantise walk the volume in groups of 16 consecutive voxels, one group per lane and load: a full
// group whose first byte is 16-B aligned is read with 16-byte loads (1 / 2 / 4 of them for 1 / 2 / 4-byte elements, all in
// flight together), another group element by element (group_load; the row_load of voxel_rows.h for six types).  Neighbouring
// lanes own neighbouring groups.
// BIN.  k_volume_bin: one thread per output voxel adds its block z outer, y, x inner, left to right.  Integer sums are int32
// (8*8*8*65535 < 2^31: exact); a float32 sum starts from 0.0f and uses plain float adds in that order (nothing to contract, no
// reassociation), so a host loop in the same order gives the same bits.  No division: what follows is scale invariant.
// MOMENTS.  k_volume_moments: workgroup c of slice s owns the voxels [c * 4096, (c + 1) * 4096) of the slice, 16 per thread, and
// writes one partial {finite count, sum v, sum v^2}: plain stores, no atomics.  Integers: int64 / uint64 sums (|v| < 2^25, so
// v^2 < 2^50 and 4096 of them < 2^62).  float32: each thread adds its finite voxels in order in double (the chain,
// CVX_MOMENT_CHAIN = 16 adds; v * v is exact in double), then a fixed tree: six xor butterflies over the wave and
// (w0 + w1) + (w2 + w3) over the workgroup's four waves (CVX_MOMENT_TREE = 8 levels).  One rounding per operation: no FMA can form.
// SELECT.  k_volume_select_hist is one pass of a radix select on a 32-bit order-preserving key (integers: v - base, base = the
// least value the type and bin factor allow; float32: the sign-flip transform; NaN and +-Inf have no key): for each rank r a voxel
// votes iff (key & mask[r]) == prefix[r], for bin (key >> shift) & (2^width - 1), width <= 11.  A thread reads four groups (64
// voxels), combines the run of equal bins it meets and sends a run to the workgroup's LDS histogram with one 32-bit LDS atomic;
// the run a thread ends with is combined over the wave when every lane holds the same bin (tomogram intensities crowd a few
// buckets).  A workgroup reads 16384 voxels, so an LDS count cannot wrap; its nonzero bins go to table [slices][ranks][2048]
// by 64-bit integer atomics.  Integer adds commute: the table does not depend on scheduling.
// QUANTISE.  k_volume_quantize: q = floor((double(v) - lo) * scale + 0.5) with one rounding per double operation (no FMA), clamped to
// [0, 255] before the conversion; NaN (of v or of the product) -> 128, +Inf -> 255, -Inf -> 0; invert stores 255 - q.  Each lane
// stores one 16-byte group of out; the bytes before the first aligned byte of out and after the last whole group are written one
// by one by workgroup 0 (as k_surface_hist of boundary.hip reads its ragged ends).  The voxels below lo and above hi are counted
// per slice: per thread, then per wave when the wave lies in one slice, then one 64-bit integer atomic.
#include "entry_checks.h"

// the sums and the quantiser are specified operation by operation: no multiply-add may be contracted anywhere in this file
#pragma clang fp contract(off)

namespace cvx {

constexpr int kGroup = 16;                                        // voxels per lane and group
constexpr int kMomentGroup = kCclThreads * kGroup;                // voxels per moment partial
static_assert(kMomentGroup == CVX_MOMENT_GROUP && kGroup == CVX_MOMENT_CHAIN, "the header states the partial's shape");
static_assert(CVX_MOMENT_TREE == 6 + 2, "six butterflies over 64 lanes, two levels over four waves");
constexpr int kSelIters = 4;                                      // groups per thread
constexpr long kSelPerGroup = (long)kCclThreads * kGroup * kSelIters;  // voxels per workgroup: 16384 < 2^32
constexpr int kSelBins = CVX_SELECT_BINS;
constexpr int kSelRanks = CVX_SELECT_MAX_RANKS;

// one IEEE double operation each, rounded to nearest.  HIP's __dadd_rn / __dmul_rn / __dsub_rn are plain operators compiled under
// the contraction setting of their header, and hipcc fused them into v_fma_f64; these stand under this file's pragma
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double dsub(double a, double b) { return a - b; }
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }

template <class T> struct is_float_t { static constexpr bool value = false; };
template <> struct is_float_t<float> { static constexpr bool value = true; };

template <class T> __device__ __forceinline__ bool is_finite(T) { return true; }
template <> __device__ __forceinline__ bool is_finite<float>(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// v[0..cnt) = p[0..cnt), the rest 0: 16-B loads for a full, 16-B aligned group, element loads otherwise
template <class T>
__device__ __forceinline__ void group_load(const T* __restrict__ p, int cnt, T (&v)[kGroup]) {
    if (cnt == kGroup && ((uintptr_t)p & 15) == 0) {
        uint4 w[sizeof(T)];
#pragma unroll
        for (int q = 0; q < (int)sizeof(T); ++q) w[q] = ((const uint4*)p)[q];
        __builtin_memcpy(v, w, sizeof(w));
    } else {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) v[i] = i < cnt ? p[i] : T(0);
    }
}

// ---- bin ----

template <class T, class S>
__global__ __launch_bounds__(kCclThreads) void k_volume_bin(const T* __restrict__ src, long H, long W, int Ho, int Wo, int kz, int k,
                                                            S* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i >= n) return;
    const long x = i % Wo, y = i / Wo % Ho, z = i / Wo / Ho;
    const T* p = src + (z * kz * H + y * k) * W + x * k;  // the block lies inside the source: (z + 1) * kz <= D, and so on
    S s = 0;
    for (int dz = 0; dz < kz; ++dz)
        for (int dy = 0; dy < k; ++dy) {
            const T* r = p + (dz * H + dy) * W;
            for (int dx = 0; dx < k; ++dx) s += (S)r[dx];
        }
    out[i] = s;
}

// ---- moments ----

template <class T>
__global__ __launch_bounds__(kCclThreads) void k_volume_moments(const T* __restrict__ v, long len, long P, long long* __restrict__ partials) {
    const long s = blockIdx.x / P, c = blockIdx.x % P;
    const long e0 = c * kMomentGroup + (long)threadIdx.x * kGroup;
    const int cnt = (int)max(0L, min((long)kGroup, len - e0));
    T x[kGroup];
    group_load(v + s * len + e0, cnt, x);  // cnt == 0 reads nothing
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long* out = partials + (long)blockIdx.x * 3;
    if constexpr (is_float_t<T>::value) {
        __shared__ double wa[4], wb[4];
        __shared__ int wn[4];
        double a = 0.0, b = 0.0;
        int n = 0;
#pragma unroll
        for (int i = 0; i < kGroup; ++i)
            if (i < cnt && is_finite(x[i])) {
                const double d = (double)x[i];
                a = dadd(a, d);
                b = dadd(b, dmul(d, d));  // exact: 24 x 24 bits
                ++n;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // every lane adds the same pairs: a fixed tree
            a = dadd(a, __shfl_xor(a, o, 64));
            b = dadd(b, __shfl_xor(b, o, 64));
        }
        n = wave_sum(n);
        if (lane == 0) { wa[wave] = a; wb[wave] = b; wn[wave] = n; }
        __syncthreads();
        if (threadIdx.x == 0) {
            out[0] = (long long)wn[0] + wn[1] + wn[2] + wn[3];
            out[1] = __double_as_longlong(dadd(dadd(wa[0], wa[1]), dadd(wa[2], wa[3])));
            out[2] = __double_as_longlong(dadd(dadd(wb[0], wb[1]), dadd(wb[2], wb[3])));
        }
    } else {
        __shared__ long long wa[4], wb[4];
        long long a = 0, b = 0;  // b holds an unsigned sum: adds wrap the same way
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {  // the voxels past cnt are 0
            const long long d = (long long)x[i];
            a += d;
            b += d * d;
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) { wa[wave] = a; wb[wave] = b; }
        __syncthreads();
        if (threadIdx.x == 0) {
            out[0] = max(0L, min((long)kMomentGroup, len - c * kMomentGroup));
            out[1] = wa[0] + wa[1] + wa[2] + wa[3];
            out[2] = wb[0] + wb[1] + wb[2] + wb[3];
        }
    }
}

// ---- select ----

template <class T> __device__ __forceinline__ unsigned select_key(T v, long base) { return (unsigned)((long)v - base); }
template <> __device__ __forceinline__ unsigned select_key<float>(float v, long) {
    const unsigned u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

struct SelRun {
    int bin;  // -1: none yet
    unsigned count;
};

template <class T>
__global__ __launch_bounds__(kCclThreads) void k_volume_select_hist(const T* __restrict__ v, long len, long G, long base, int shift, int width,
                                                                    int R, const long long* __restrict__ prefix,
                                                                    unsigned long long* __restrict__ table) {
    __shared__ unsigned lds[kSelRanks * kSelBins];
    const long s = blockIdx.x / G, c = blockIdx.x % G;
    const T* p = v + s * len;
    T x[kSelIters][kGroup];
    int cnt[kSelIters];
#pragma unroll
    for (int it = 0; it < kSelIters; ++it) {  // all of the thread's loads are in flight together
        const long e0 = c * kSelPerGroup + ((long)it * kCclThreads + threadIdx.x) * kGroup;
        cnt[it] = (int)max(0L, min((long)kGroup, len - e0));
        if (cnt[it] > 0) group_load(p + e0, cnt[it], x[it]);
    }
    for (int b = threadIdx.x; b < R * kSelBins; b += kCclThreads) lds[b] = 0;
    unsigned pre[kSelRanks], msk[kSelRanks];
#pragma unroll
    for (int r = 0; r < kSelRanks; ++r) {
        pre[r] = r < R ? (unsigned)prefix[(s * R + r) * 2] : 1u;  // (key & 0) == 1 never holds
        msk[r] = r < R ? (unsigned)prefix[(s * R + r) * 2 + 1] : 0u;
    }
    __syncthreads();
    const unsigned field = (1u << width) - 1;
    SelRun run[kSelRanks] = {{-1, 0}, {-1, 0}};
#pragma unroll
    for (int it = 0; it < kSelIters; ++it)
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            if (i >= cnt[it] || !is_finite(x[it][i])) continue;
            const unsigned key = select_key(x[it][i], base);
            const int bin = (int)(key >> shift & field);
#pragma unroll
            for (int r = 0; r < kSelRanks; ++r) {
                if ((key & msk[r]) != pre[r]) continue;
                if (bin != run[r].bin) {
                    if (run[r].bin >= 0) atomicAdd(lds + r * kSelBins + run[r].bin, run[r].count);
                    run[r] = SelRun{bin, 0};
                }
                ++run[r].count;
            }
        }
#pragma unroll
    for (int r = 0; r < kSelRanks; ++r) {  // all 64 lanes are here
        const int single = wave_single_id(run[r].bin + 1);
        if (single) {
            const int total = wave_sum((int)run[r].count);  // <= 64 * 64
            if ((threadIdx.x & 63) == 0) atomicAdd(lds + r * kSelBins + single - 1, (unsigned)total);
        } else if (run[r].bin >= 0) {
            atomicAdd(lds + r * kSelBins + run[r].bin, run[r].count);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < R * kSelBins; b += kCclThreads) {
        const unsigned n = lds[b];
        if (n) atomicAdd(table + s * R * kSelBins + b, (unsigned long long)n);
    }
}

// ---- quantise ----

struct QuantState {
    long slice;  // -1: no voxel yet
    double lo, hi, scale;
    int below, above;
};

__device__ __forceinline__ void quant_flush(const QuantState& q, unsigned long long* __restrict__ clipped) {
    if (q.below) atomicAdd(clipped + q.slice * 2, (unsigned long long)q.below);
    if (q.above) atomicAdd(clipped + q.slice * 2 + 1, (unsigned long long)q.above);
}

// the state moves to `slice`: its counts go out and the slice's lo, hi, scale come in
__device__ __forceinline__ void quant_enter(QuantState& q, long slice, const double* __restrict__ params, int per_slice,
                                            unsigned long long* __restrict__ clipped) {
    if (q.slice >= 0) quant_flush(q, clipped);
    const double* t = params + (per_slice ? slice * 3 : 0);
    q = QuantState{slice, t[0], t[1], t[2], 0, 0};
}

template <class T>
__device__ __forceinline__ unsigned quant_one(QuantState& q, T v, int invert) {
    const double d = (double)v;
    q.below += d < q.lo;
    q.above += d > q.hi;
    double t = floor(dadd(dmul(dsub(d, q.lo), q.scale), 0.5));
    if (!is_finite(v)) t = d > 0.0 ? 255.0 : d < 0.0 ? 0.0 : t;  // +-Inf clamp whatever the scale; NaN stays NaN
    const unsigned r = t != t ? 128u : (unsigned)(int)fmin(fmax(t, 0.0), 255.0);
    return invert ? 255u - r : r;
}

// head: the voxels before the first 16-B aligned byte of out, groups: the whole 16-byte groups after them
template <class T>
__global__ __launch_bounds__(kCclThreads) void k_volume_quantize(const T* __restrict__ v, long n, long len, long head, long groups,
                                                                 const double* __restrict__ params, int per_slice, int invert,
                                                                 uint8_t* __restrict__ out, unsigned long long* __restrict__ clipped) {
    const long g = (long)blockIdx.x * kCclThreads + threadIdx.x;
    QuantState q{-1, 0.0, 0.0, 0.0, 0, 0};
    if (g < groups) {
        const long e0 = head + g * kGroup;
        T x[kGroup];
        group_load(v + e0, kGroup, x);
        long slice = e0 / len, left = len - e0 % len;  // voxels of `slice` from e0 on
        quant_enter(q, slice, params, per_slice, clipped);
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            if (left == 0) {
                left = len;
                quant_enter(q, ++slice, params, per_slice, clipped);
            }
            --left;
            w[i >> 2] |= quant_one(q, x[i], invert) << (8 * (i & 3));
        }
        *(uint4*)(out + e0) = uint4{w[0], w[1], w[2], w[3]};
    }
    if (blockIdx.x == 0) {  // the ragged ends: fewer than 16 voxels each
        const long tail = head + groups * kGroup;
        for (int side = 0; side < 2; ++side) {
            const long e = side ? tail + threadIdx.x : (long)threadIdx.x;
            if (side ? e >= n : e >= head) continue;
            if (e / len != q.slice) quant_enter(q, e / len, params, per_slice, clipped);
            out[e] = (uint8_t)quant_one(q, v[e], invert);
        }
    }
    const int single = wave_single_id((int)(q.slice + 1));  // slices < 2^31 - 1; all 64 lanes are here
    if (single) {
        const int below = wave_sum(q.below), above = wave_sum(q.above);
        if ((threadIdx.x & 63) == 0) quant_flush(QuantState{single - 1, 0.0, 0.0, 0.0, below, above}, clipped);
    } else if (q.slice >= 0) {
        quant_flush(q, clipped);
    }
}

// fn(T()) for the element type of a CVX_VOL_* value; false for another value
template <class F>
inline bool vol_dispatch(int dtype, F&& fn) {
    switch (dtype) {
        case CVX_VOL_I8: fn(int8_t()); return true;
        case CVX_VOL_U8: fn(uint8_t()); return true;
        case CVX_VOL_I16: fn(int16_t()); return true;
        case CVX_VOL_U16: fn(uint16_t()); return true;
        case CVX_VOL_I32: fn(int32_t()); return true;
        case CVX_VOL_F32: fn(float()); return true;
    }
    return false;
}

inline int vol_elem_bytes(int dtype) {
    return dtype == CVX_VOL_I8 || dtype == CVX_VOL_U8 ? 1 : dtype == CVX_VOL_I16 || dtype == CVX_VOL_U16 ? 2 : 4;
}
inline bool vol_dtype_ok(int dtype) { return dtype >= CVX_VOL_I8 && dtype <= CVX_VOL_F32; }

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_volume_bin(const void* src, int dtype, long D, long H, long W, int kz, int k, void* out, hipStream_t st) {
    if (!vol_dtype_ok(dtype) || dtype == CVX_VOL_I32) return cvx_fail("volume_bin", "dtype must be one of int8, uint8, int16, uint16, float32");
    if (kz < 1 || kz > CVX_BIN_MAX || k < 1 || k > CVX_BIN_MAX) return cvx_fail("volume_bin", "bin factors must lie in 1..8");
    if (D < 0 || H < 0 || W < 0) return cvx_fail("volume_bin", "negative extent");
    if (D / kz > INT_MAX || H / k > INT_MAX || W / k > INT_MAX) return cvx_fail("volume_bin", kExtentsRule);
    const int Do = (int)(D / kz), Ho = (int)(H / k), Wo = (int)(W / k);
    long n = 0;
    if (extents_fault(Do, Ho, Wo, kExtentAny, n)) return cvx_fail("volume_bin", kExtentsRule);  // of the binned volume
    if (n == 0) return 0;
    if (!src || !out) return cvx_fail("volume_bin", "null pointer");
    if (((uintptr_t)src & (vol_elem_bytes(dtype) - 1)) || ((uintptr_t)out & 3)) return cvx_fail("volume_bin", "misaligned pointer");
    if (src == out) return cvx_fail("volume_bin", "src and out must be different arrays");
    const dim3 grid(blocks_of(n)), block(kCclThreads);
    vol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (is_float_t<T>::value) hipLaunchKernelGGL((k_volume_bin<T, float>), grid, block, 0, st, (const T*)src, H, W, Ho, Wo, kz, k, (float*)out, n);
        else if constexpr (sizeof(T) < 4) hipLaunchKernelGGL((k_volume_bin<T, int>), grid, block, 0, st, (const T*)src, H, W, Ho, Wo, kz, k, (int*)out, n);
    });
    return cvx_check_launch();
}

extern "C" int cvx_volume_moments(const void* v, int dtype, int D, int H, int W, void* partials, hipStream_t st) {
    long n = 0;
    if (!vol_dtype_ok(dtype)) return cvx_fail("volume_moments", "unknown dtype");
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("volume_moments", why);
    if (D == 0) return 0;
    if (!partials || (n > 0 && !v)) return cvx_fail("volume_moments", "null pointer");
    if (((uintptr_t)v & (vol_elem_bytes(dtype) - 1)) || ((uintptr_t)partials & 7)) return cvx_fail("volume_moments", "misaligned pointer");
    const long len = (long)H * W, P = len ? (len + kMomentGroup - 1) / kMomentGroup : 1;  // D * P <= n / 4096 + D < 2^31
    vol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_volume_moments<T>, dim3((unsigned)(D * P)), dim3(kCclThreads), 0, st, (const T*)v, len, P, (long long*)partials);
    });
    return cvx_check_launch();
}

extern "C" int cvx_volume_select_hist(const void* v, int dtype, long slices, long len, long base, int shift, int width, int ranks,
                                      const int64_t* prefix, int64_t* table, hipStream_t st) {
    if (!vol_dtype_ok(dtype)) return cvx_fail("volume_select_hist", "unknown dtype");
    if (slices < 0 || len < 0 || (len && slices > CVX_COMPONENT_MAX_VOXELS / len) || slices > INT_MAX)
        return cvx_fail("volume_select_hist", "slices and len must be >= 0 with slices*len <= 2^31 - 2");
    if (ranks < 1 || ranks > kSelRanks) return cvx_fail("volume_select_hist", "ranks must be 1 or 2");
    if (width < 1 || width > 11 || shift < 0 || shift + width > 32) return cvx_fail("volume_select_hist", "the bit field must hold 1..11 bits inside the 32-bit key");
    if (slices == 0) return 0;
    if (!prefix || !table || (len > 0 && !v)) return cvx_fail("volume_select_hist", "null pointer");
    if (((uintptr_t)v & (vol_elem_bytes(dtype) - 1)) || ((uintptr_t)prefix & 7) || ((uintptr_t)table & 7)) return cvx_fail("volume_select_hist", "misaligned pointer");
    CVX_HIP(hipMemsetAsync(table, 0, (size_t)slices * ranks * kSelBins * sizeof(int64_t), st));
    if (len == 0) return 0;
    const long G = (len + kSelPerGroup - 1) / kSelPerGroup;  // slices * G <= n / 16384 + slices < 2^31
    vol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_volume_select_hist<T>, dim3((unsigned)(slices * G)), dim3(kCclThreads), 0, st, (const T*)v, len, G, base, shift, width,
                           ranks, (const long long*)prefix, (unsigned long long*)table);
    });
    return cvx_check_launch();
}

extern "C" int cvx_volume_quantize(const void* v, int dtype, int D, int H, int W, const double* params, int per_slice, int invert,
                                   uint8_t* out, int64_t* clipped, hipStream_t st) {
    long n = 0;
    if (!vol_dtype_ok(dtype)) return cvx_fail("volume_quantize", "unknown dtype");
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("volume_quantize", why);
    if ((per_slice != 0 && per_slice != 1) || (invert != 0 && invert != 1)) return cvx_fail("volume_quantize", "per_slice and invert must be 0 or 1");
    if (D == 0) return 0;
    if (!clipped || (n > 0 && (!v || !out || !params))) return cvx_fail("volume_quantize", "null pointer");
    if (((uintptr_t)v & (vol_elem_bytes(dtype) - 1)) || ((uintptr_t)params & 7) || ((uintptr_t)clipped & 7)) return cvx_fail("volume_quantize", "misaligned pointer");
    if (v == (const void*)out) return cvx_fail("volume_quantize", "v and out must be different arrays");
    CVX_HIP(hipMemsetAsync(clipped, 0, (size_t)D * 2 * sizeof(int64_t), st));
    if (n == 0) return 0;
    const long head = n < kGroup ? n : (long)((16 - ((uintptr_t)out & 15)) & 15), groups = (n - head) / kGroup;
    const unsigned blocks = groups ? blocks_of(groups) : 1;
    vol_dispatch(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_volume_quantize<T>, dim3(blocks), dim3(kCclThreads), 0, st, (const T*)v, n, (long)H * W, head, groups, params, per_slice,
                           invert, out, (unsigned long long*)clipped);
    });
    return cvx_check_launch();
}
