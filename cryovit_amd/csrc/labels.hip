// Label decode and evaluation counts of `cryovit evaluate` (run/eval_model.py:run_evaluation): the host-side
// utils._match_label_keys_to_data (np.unique + two np.where per label name) and the two metric passes (DiceMetric at p >= t,
// F1Metric at p > t) become one census kernel pair and one counting kernel, both reading the label volume in its file dtype.
// HBM-bound streaming kernels: 16-B loads, grid-stride, ragged tail on block 0.  Integer results only: min / max / the
// presence bitmap / the counts are combined with integer atomics (min, max, or, add), which are exact and commutative, so
// every call gives the same bits whatever the block order; no float atomics.
#include "voxel_rows.h"  // wave_sum
#include "host_util.h"

#include <limits.h>

namespace cvx {

constexpr int kLabelThreads = 256;
constexpr int kBitmapWords = CVX_LABEL_BITMAP_BITS / 32;

// label element -> int32 value; `bad` gets CVX_LABEL_NONINTEGER / CVX_LABEL_WIDE for float32 values that are not integers
// (NaN, inf, fractions) or lie outside int32.  Integer dtypes always fit.
template <typename T>
__device__ __forceinline__ int label_int(T v, uint32_t& bad) { return (int)v; }
template <>
__device__ __forceinline__ int label_int<float>(float v, uint32_t& bad) {
    if (!(v == truncf(v)) || isinf(v)) { bad |= CVX_LABEL_NONINTEGER; return 0; }
    if (v < -2147483648.0f || v >= 2147483648.0f) { bad |= CVX_LABEL_WIDE; return 0; }
    return (int)v;
}

// np.asarray(v).astype(np.int8): integers wrap to their low byte; float32 truncates toward zero (values outside int32 are
// clamped first: numpy leaves that case undefined)
template <typename T>
__device__ __forceinline__ int as_int8(T v) { return (int)(int8_t)v; }
template <>
__device__ __forceinline__ int as_int8<float>(float v) {
    return (int)(int8_t)(int)fminf(fmaxf(truncf(v), -2147483648.0f), 2147483520.0f);
}

template <typename T>
__device__ __forceinline__ bool label_eq(T v, int value) { return (int)v == value; }
template <>
__device__ __forceinline__ bool label_eq<float>(float v, int value) { return (double)v == (double)value; }

// one 16-byte vector of labels
template <typename T>
struct LabelVec {
    static constexpr int N = 16 / (int)sizeof(T);
    T v[N];
};

template <typename T>
__device__ __forceinline__ LabelVec<T> load_labels16(const T* p) {
    LabelVec<T> out;
    *(uint4*)out.v = *(const uint4*)p;
    return out;
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_or_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// census[0] = INT_MAX, census[1] = INT_MIN, flags and bitmap 0
__global__ __launch_bounds__(kLabelThreads) void k_label_census_init(int32_t* __restrict__ census) {
    for (int i = threadIdx.x; i < CVX_LABEL_CENSUS_WORDS; i += kLabelThreads)
        census[i] = i == 0 ? INT_MAX : i == 1 ? INT_MIN : 0;
}

// pass 1: min, max and the validity flags
template <typename T>
__global__ __launch_bounds__(kLabelThreads) void k_label_minmax(const T* __restrict__ labels, long n, int32_t* __restrict__ census) {
    constexpr int N = LabelVec<T>::N;
    __shared__ int red[3][kLabelThreads / 64];
    int lo = INT_MAX, hi = INT_MIN;
    uint32_t bad = 0;
    const long nvec = n / N;
    for (long i = (long)blockIdx.x * kLabelThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kLabelThreads) {
        const LabelVec<T> lv = load_labels16(labels + i * N);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int x = label_int(lv.v[e], bad);
            lo = min(lo, x);
            hi = max(hi, x);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * N)) {  // the last n % N elements
        const int x = label_int(labels[nvec * N + threadIdx.x], bad);
        lo = min(lo, x);
        hi = max(hi, x);
    }
    lo = wave_min_i(lo); hi = wave_max_i(hi); bad = wave_or_u(bad);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = lo; red[1][wave] = hi; red[2][wave] = (int)bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kLabelThreads / 64; ++w) { lo = min(lo, red[0][w]); hi = max(hi, red[1][w]); bad |= (uint32_t)red[2][w]; }
        if (lo <= hi) { atomicMin(&census[0], lo); atomicMax(&census[1], hi); }
        if (bad) atomicOr((uint32_t*)&census[2], bad);
    }
}

// pass 2: presence bitmap over [min, max] in LDS, then OR-ed into census[4..].  A lane ORs a bit only when its value changes
// from the previous element it saw: label maps are piecewise constant, so this removes almost all LDS atomics.
template <typename T>
__global__ __launch_bounds__(kLabelThreads) void k_label_bitmap(const T* __restrict__ labels, long n, int32_t* __restrict__ census) {
    constexpr int N = LabelVec<T>::N;
    __shared__ uint32_t bits[kBitmapWords];
    const int lo = census[0], hi = census[1];
    if (census[2] != 0 || lo > hi) return;  // invalid values, or no elements
    if ((long)hi - (long)lo >= CVX_LABEL_BITMAP_BITS) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr((uint32_t*)&census[2], (uint32_t)CVX_LABEL_WIDE);
        return;
    }
    const int words = (int)(((long)hi - (long)lo) >> 5) + 1;
    for (int w = threadIdx.x; w < words; w += kLabelThreads) bits[w] = 0u;
    __syncthreads();
    uint32_t unused = 0;
    int last = -1;
    const long nvec = n / N;
    for (long i = (long)blockIdx.x * kLabelThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kLabelThreads) {
        const LabelVec<T> lv = load_labels16(labels + i * N);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int k = label_int(lv.v[e], unused) - lo;
            if (k != last && (unsigned)k < (unsigned)(words * 32)) { atomicOr(&bits[k >> 5], 1u << (k & 31)); last = k; }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * N)) {
        const int k = label_int(labels[nvec * N + threadIdx.x], unused) - lo;
        if ((unsigned)k < (unsigned)(words * 32)) atomicOr(&bits[k >> 5], 1u << (k & 31));
    }
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += kLabelThreads)
        if (bits[w]) atomicOr((uint32_t*)&census[4 + w], bits[w]);
}

// decoded label of one voxel: the int8 array utils._match_label_keys_to_data ("match") or the single-key HDF branch's
// data.astype(np.int8) ("weight") would hold.  match: np.where((d != v) & (d != -1), 0, d), then np.where(== v, 1, .) ->
//   1 where d == v; -1 where d == -1; elsewhere 1 if v == 0 (the second where also catches the zeros the first one wrote) else 0
template <typename T, int MODE>
__device__ __forceinline__ int decode_label(T d, int value) {
    if (MODE == CVX_LABEL_MATCH) {
        if (label_eq(d, value)) return 1;
        if (label_eq(d, -1)) return -1;  // never true for unsigned dtypes, as numpy's `data != -1`
        return value == 0 ? 1 : 0;
    }
    return as_int8(d);
}

// counts[0..4] += sum y, sum [p >= t], sum y [p >= t], sum [p > t], sum y [p > t] over voxels with decoded y > -1;
// y_out (nullable) = the decoded int8 label of every voxel
template <typename T, int MODE>
__global__ __launch_bounds__(kLabelThreads) void k_label_metrics(const float* __restrict__ probs, const T* __restrict__ labels, long n,
                                                                int value, float thr, unsigned long long* __restrict__ counts,
                                                                int8_t* __restrict__ y_out) {
    constexpr int N = LabelVec<T>::N;
    __shared__ unsigned long long red[5][kLabelThreads / 64];
    unsigned long long acc[5] = {0, 0, 0, 0, 0};
    auto count = [&](int y, float p) {
        if (y > -1) {
            const unsigned ge = p >= thr, gt = p > thr;
            acc[0] += (unsigned)y;
            acc[1] += ge;
            acc[2] += (unsigned)y * ge;
            acc[3] += gt;
            acc[4] += (unsigned)y * gt;
        }
    };
    const long nvec = n / N;
    for (long i = (long)blockIdx.x * kLabelThreads + threadIdx.x; i < nvec; i += (long)gridDim.x * kLabelThreads) {
        const LabelVec<T> lv = load_labels16(labels + i * N);
        int8_t ys[N];
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const float4 p = *(const float4*)(probs + i * N + 4 * q);
            const float pv[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int y = decode_label<T, MODE>(lv.v[4 * q + e], value);
                ys[4 * q + e] = (int8_t)y;
                count(y, pv[e]);
            }
        }
        if (y_out) {
            if constexpr (N == 16) *(uint4*)(y_out + i * N) = *(const uint4*)ys;
            else if constexpr (N == 8) *(uint2*)(y_out + i * N) = *(const uint2*)ys;
            else *(uint32_t*)(y_out + i * N) = *(const uint32_t*)ys;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * N)) {
        const long j = nvec * N + threadIdx.x;
        const int y = decode_label<T, MODE>(labels[j], value);
        if (y_out) y_out[j] = (int8_t)y;
        count(y, probs[j]);
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long s = (unsigned long long)wave_sum((long long)acc[k]);  // two's complement: the same bits
        if ((threadIdx.x & 63) == 0) red[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned long long s = 0;
        for (int w = 0; w < kLabelThreads / 64; ++w) s += red[threadIdx.x][w];
        if (s) atomicAdd(&counts[threadIdx.x], s);
    }
}

}  // namespace cvx

using namespace cvx;

static int label_elem_bytes(int dtype) {
    switch (dtype) {
        case CVX_LABEL_I8: case CVX_LABEL_U8: return 1;
        case CVX_LABEL_I16: case CVX_LABEL_U16: return 2;
        case CVX_LABEL_I32: case CVX_LABEL_F32: return 4;
        default: return 0;
    }
}

// enough blocks to cover the volume with a few 16-B vectors per lane, at most 2048 (8 per CU)
static unsigned label_blocks(long n, int elem_bytes) {
    const long vec = n / (16 / elem_bytes) + 1;
    long b = (vec + 4L * kLabelThreads - 1) / (4L * kLabelThreads);
    if (b < 1) b = 1;
    return (unsigned)(b < 2048 ? b : 2048);
}

template <typename T>
static int census_launch(const void* labels, long n, int32_t* census, hipStream_t st) {
    const unsigned nblk = label_blocks(n, sizeof(T));
    hipLaunchKernelGGL(k_label_minmax<T>, dim3(nblk), dim3(kLabelThreads), 0, st, (const T*)labels, n, census);
    int rc = cvx_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_label_bitmap<T>, dim3(nblk), dim3(kLabelThreads), 0, st, (const T*)labels, n, census);
    return cvx_check_launch();
}

extern "C" int cvx_label_census(const void* labels, int dtype, long n, int32_t* census, hipStream_t st) {
    const int eb = label_elem_bytes(dtype);
    if (!eb) return cvx_fail("label_census: unknown label dtype");
    if (!census || (n > 0 && !labels)) return cvx_fail("label_census: null pointer");
    if (n < 0) return cvx_fail("label_census: n < 0");
    if ((uintptr_t)labels & 15) return cvx_fail("label_census: labels must be 16-B aligned");
    hipLaunchKernelGGL(k_label_census_init, dim3(1), dim3(kLabelThreads), 0, st, census);
    int rc = cvx_check_launch();
    if (rc || n == 0) return rc;
    switch (dtype) {
        case CVX_LABEL_I8: return census_launch<int8_t>(labels, n, census, st);
        case CVX_LABEL_U8: return census_launch<uint8_t>(labels, n, census, st);
        case CVX_LABEL_I16: return census_launch<int16_t>(labels, n, census, st);
        case CVX_LABEL_U16: return census_launch<uint16_t>(labels, n, census, st);
        case CVX_LABEL_I32: return census_launch<int32_t>(labels, n, census, st);
        default: return census_launch<float>(labels, n, census, st);
    }
}

template <typename T>
static int metrics_launch(const float* probs, const void* labels, long n, int mode, int value, float thr, uint64_t* counts,
                          int8_t* y_out, hipStream_t st) {
    const unsigned nblk = label_blocks(n, sizeof(T));
    auto* c = (unsigned long long*)counts;
    if (mode == CVX_LABEL_MATCH)
        hipLaunchKernelGGL((k_label_metrics<T, CVX_LABEL_MATCH>), dim3(nblk), dim3(kLabelThreads), 0, st, probs, (const T*)labels, n, value,
                           thr, c, y_out);
    else
        hipLaunchKernelGGL((k_label_metrics<T, CVX_LABEL_WEIGHT>), dim3(nblk), dim3(kLabelThreads), 0, st, probs, (const T*)labels, n, value,
                           thr, c, y_out);
    return cvx_check_launch();
}

extern "C" int cvx_label_metrics(const float* probs, const void* labels, int dtype, long n, int mode, int value, float thr,
                                 uint64_t* counts, int8_t* y_out, hipStream_t st) {
    const int eb = label_elem_bytes(dtype);
    if (!eb) return cvx_fail("label_metrics: unknown label dtype");
    if (mode != CVX_LABEL_MATCH && mode != CVX_LABEL_WEIGHT) return cvx_fail("label_metrics: unknown mode");
    if (!counts || (n > 0 && (!probs || !labels))) return cvx_fail("label_metrics: null pointer");
    if (n < 0) return cvx_fail("label_metrics: n < 0");
    if (((uintptr_t)probs | (uintptr_t)labels | (uintptr_t)y_out) & 15)
        return cvx_fail("label_metrics: probs, labels and y_out must be 16-B aligned");
    if (n == 0) return 0;
    switch (dtype) {
        case CVX_LABEL_I8: return metrics_launch<int8_t>(probs, labels, n, mode, value, thr, counts, y_out, st);
        case CVX_LABEL_U8: return metrics_launch<uint8_t>(probs, labels, n, mode, value, thr, counts, y_out, st);
        case CVX_LABEL_I16: return metrics_launch<int16_t>(probs, labels, n, mode, value, thr, counts, y_out, st);
        case CVX_LABEL_U16: return metrics_launch<uint16_t>(probs, labels, n, mode, value, thr, counts, y_out, st);
        case CVX_LABEL_I32: return metrics_launch<int32_t>(probs, labels, n, mode, value, thr, counts, y_out, st);
        default: return metrics_launch<float>(probs, labels, n, mode, value, thr, counts, y_out, st);
    }
}
