// Multi-label segmentation overlays (the frames of cryovit/visualization/segmentations.py:_process_file): every label volume
// times its colour, summed, clipped, laid over the grey data where a channel exceeds the threshold, and written next to the
// grey data as packed uint8 RGB.  One streaming pass: up to 9 volumes read once, 6 B per voxel written, no atomics, no LDS.
// Operation for operation numpy's arithmetic (float32 += float32 * float64 per label, float32 clip / compare / * 255,
// truncation), so the frames are bit-equal to the numpy form.
#include "common.h"
#include "../../include/cryovit_hip.h"
#include "host_util.h"

namespace cvx {

constexpr int kSegThreads = 256;
constexpr int SV = 16;  // voxels of one row per thread: 64 B of fp32 / 16 B of uint8 read, 48 B written per half

struct SegArgs {
    const void* lab[CVX_SEG_MAX_LABELS];
    double col[CVX_SEG_MAX_LABELS][3];
    int is_u8[CVX_SEG_MAX_LABELS];
    int n;
};

// v[0..cnt) = p[0..cnt): 16-B loads for a full, 16-B aligned group, element loads otherwise (row tails, rows that start
// off a 16-B boundary because W is not a multiple of 4 / 16)
__device__ __forceinline__ void seg_load(const float* __restrict__ p, int cnt, float (&v)[SV]) {
    if (cnt == SV && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < SV / 4; ++q) {
            const float4 f = ((const float4*)p)[q];
            v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < SV; ++i) v[i] = i < cnt ? p[i] : 0.f;
    }
}
__device__ __forceinline__ void seg_load(const uint8_t* __restrict__ p, int cnt, float (&v)[SV]) {
    if (cnt == SV && ((uintptr_t)p & 15) == 0) {
        const uint4 q = *(const uint4*)p;
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < SV; ++i) v[i] = (float)((wd[i >> 2] >> (8 * (i & 3))) & 0xff);
    } else {
#pragma unroll
        for (int i = 0; i < SV; ++i) v[i] = i < cnt ? (float)p[i] : 0.f;
    }
}

// nbytes (= 3 * voxels, <= 48) packed bytes w -> dst.  A full group goes out as 3 x 16 B when dst is 16-B aligned, else as
// up to 3 head bytes, 11 aligned dwords funnel-shifted out of w, and the remaining bytes; a row tail goes out bytewise.
__device__ __forceinline__ void seg_store(uint8_t* __restrict__ dst, const uint32_t (&w)[12], int nbytes) {
    if (nbytes == 3 * SV) {
        if (((uintptr_t)dst & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) ((u32x4*)dst)[q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
            return;
        }
        const int s = (int)((0 - (uintptr_t)dst) & 3);  // bytes up to the next dword boundary
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (b < s) dst[b] = (uint8_t)(w[0] >> (8 * b));
        uint32_t* q = (uint32_t*)(dst + s);
#pragma unroll
        for (int j = 0; j < 11; ++j) q[j] = (uint32_t)((((uint64_t)w[j + 1] << 32) | w[j]) >> (8 * s));
        const uint32_t t = w[11] >> (8 * s);  // bytes 44 + s .. 47
        if (s == 0) {
            q[11] = t;
        } else {
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b < 4 - s) dst[44 + s + b] = (uint8_t)(t >> (8 * b));
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < 3 * SV; ++b)
        if (b < nbytes) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
}

// one thread = SV consecutive voxels of one row -> 3 * SV bytes in the left (grey) and in the right (overlay) half of that
// output row.  out row = [2W][3] bytes.
__global__ __launch_bounds__(kSegThreads) void k_seg_overlay(const float* __restrict__ data, const SegArgs a, long rows, int W, int groups_row,
                                                             float thr, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * kSegThreads + threadIdx.x;
    if (t >= rows * groups_row) return;
    const long r = t / groups_row;
    const int x0 = (int)(t - r * groups_row) * SV;
    const int cnt = min(SV, W - x0);
    const long off = r * W + x0;
    float comb[SV][3];
#pragma unroll
    for (int i = 0; i < SV; ++i) comb[i][0] = comb[i][1] = comb[i][2] = 0.f;
    for (int l = 0; l < a.n; ++l) {
        float seg[SV];
        if (a.is_u8[l]) seg_load((const uint8_t*)a.lab[l] + off, cnt, seg);
        else seg_load((const float*)a.lab[l] + off, cnt, seg);
        const double c0 = a.col[l][0], c1 = a.col[l][1], c2 = a.col[l][2];
#pragma unroll
        for (int i = 0; i < SV; ++i) {
            const double s = (double)seg[i];
            comb[i][0] = (float)((double)comb[i][0] + s * c0);
            comb[i][1] = (float)((double)comb[i][1] + s * c1);
            comb[i][2] = (float)((double)comb[i][2] + s * c2);
        }
    }
    float g[SV];
    seg_load(data + off, cnt, g);
    uint32_t left[12], right[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) left[k] = right[k] = 0u;
#pragma unroll
    for (int i = 0; i < SV; ++i) {
        const float gi = fminf(fmaxf(g[i], 0.f), 1.f);
        const uint32_t gb = (uint32_t)(uint8_t)(int)(gi * 255.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float cc = fminf(fmaxf(comb[i][c], 0.f), 1.f);
            const uint32_t ob = cc > thr ? (uint32_t)(uint8_t)(int)(cc * 255.0f) : gb;
            const int k = 3 * i + c;
            left[k >> 2] |= gb << (8 * (k & 3));
            right[k >> 2] |= ob << (8 * (k & 3));
        }
    }
    uint8_t* row = out + r * (6L * W) + 3L * x0;
    seg_store(row, left, 3 * cnt);
    seg_store(row + 3L * W, right, 3 * cnt);
}

}  // namespace cvx

using namespace cvx;

extern "C" int cvx_seg_overlay(const float* data, const void* const* labels, const int* label_dtypes, const double* colours, int n,
                               int D, int H, int W, double threshold, uint8_t* out, hipStream_t st) {
    if (D <= 0 || H <= 0 || W <= 0) return cvx_fail("seg_overlay: D, H, W must be positive");
    if (n < 0 || n > CVX_SEG_MAX_LABELS) return cvx_fail("seg_overlay: 0 <= n <= CVX_SEG_MAX_LABELS label volumes");
    if (!data || !out || (n > 0 && (!labels || !label_dtypes || !colours))) return cvx_fail("seg_overlay: null pointer");
    if ((uintptr_t)data & 3) return cvx_fail("seg_overlay: data must be 4-byte aligned");
    SegArgs a = {};
    a.n = n;
    for (int l = 0; l < n; ++l) {
        if (label_dtypes[l] != CVX_SEG_F32 && label_dtypes[l] != CVX_SEG_U8) return cvx_fail("seg_overlay: label dtype must be CVX_SEG_F32 or CVX_SEG_U8");
        if (!labels[l]) return cvx_fail("seg_overlay: null label volume");
        a.is_u8[l] = label_dtypes[l] == CVX_SEG_U8;
        if (!a.is_u8[l] && ((uintptr_t)labels[l] & 3)) return cvx_fail("seg_overlay: fp32 label volumes must be 4-byte aligned");
        a.lab[l] = labels[l];
        for (int c = 0; c < 3; ++c) a.col[l][c] = colours[3 * l + c];
    }
    const long rows = (long)D * H;
    const int groups_row = (W + SV - 1) / SV;
    const long nblk = (rows * groups_row + kSegThreads - 1) / kSegThreads;
    if (nblk > 0x7fffffffL) return cvx_fail("seg_overlay: volume too large");
    hipLaunchKernelGGL(k_seg_overlay, dim3((unsigned)nblk), dim3(kSegThreads), 0, st, data, a, rows, W, groups_row, (float)threshold, out);
    return cvx_check_launch();
}
