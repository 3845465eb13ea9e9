// PCA colour maps of DINO patch features (the export of cryovit/visualization/dino_pca.py): moments of every tenth slice on
// the fp16 MFMA, projection onto three components, bicubic x2, matplotlib's HSV recolouring and the uint8 image canvas.
// Every result is bitwise reproducible: no atomics, split-K partials reduced in a fixed order.
#include "common.h"
#include "../../include/cryovit_hip.h"
#include "host_util.h"

namespace cvx {

constexpr int PCA_STEP = CVX_PCA_SLICE_STEP;
constexpr int GT = 128;                 // Gram output tile (GT x GT, 4 waves of 64 x 64)
constexpr int GRAM_TARGET_BLOCKS = 1024; // tiles x K splits aimed at (4 per CU on 256 CUs)
constexpr int MM_BLOCKS = 256;          // partial min / max blocks (data and colour channels)

struct GramPlan {
    int nt, ntiles, nsteps, splits, steps_per;
};
static GramPlan gram_plan(int C, int D, int hw) {
    GramPlan p;
    p.nt = (C + GT - 1) / GT;
    p.ntiles = p.nt * (p.nt + 1) / 2;
    const long K = (long)((D + PCA_STEP - 1) / PCA_STEP) * hw;
    p.nsteps = (int)((K + 31) / 32);
    int s = (GRAM_TARGET_BLOCKS + p.ntiles - 1) / p.ntiles;
    s = min(s, max(1, p.nsteps / 8));  // at least 8 K steps of 32 per block
    p.steps_per = (p.nsteps + s - 1) / s;
    p.splits = (p.nsteps + p.steps_per - 1) / p.steps_per;
    return p;
}

// 8 consecutive K of feature row `row` at flattened K index kk0 (kk = selected slice * hw + pixel); zero past K / C.
// ALIGNED (hw % 8 == 0): the 8 values never straddle a slice and sit 16-B aligned -> one 16-B load.
template <bool ALIGNED>
__device__ __forceinline__ bf16x8 gram_frag(const uint16_t* __restrict__ x, int row, int C, long row_stride, long kk0, long K, int hw) {
    if constexpr (ALIGNED) {
        uint4 v = {0u, 0u, 0u, 0u};
        if (row < C && kk0 < K) {
            const long j = kk0 / hw, p = kk0 - j * hw;
            v = *(const uint4*)(x + row * row_stride + j * PCA_STEP * hw + p);
        }
        return __builtin_bit_cast(bf16x8, v);
    } else {
        uint16_t e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long kk = kk0 + i;
            e[i] = 0;
            if (row < C && kk < K) {
                const long j = kk / hw, p = kk - j * hw;
                e[i] = x[row * row_stride + j * PCA_STEP * hw + p];
            }
        }
        uint4 v;
        v.x = e[0] | ((uint32_t)e[1] << 16); v.y = e[2] | ((uint32_t)e[3] << 16);
        v.z = e[4] | ((uint32_t)e[5] << 16); v.w = e[6] | ((uint32_t)e[7] << 16);
        return __builtin_bit_cast(bf16x8, v);
    }
}

// Upper-triangle GT x GT tile (blockIdx.x) of X X^T over one K split (blockIdx.y) -> fp32 partial [split][tile][col][row].
// Operands straight from the [C][D][hw] feature buffer (no LDS: each value feeds 4 MFMAs of its wave; the 2x2 waves of a
// block share rows through the L1), next K step loaded while the current one is multiplied.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_pca_gram(const uint16_t* __restrict__ x, int C, int D, int hw, long K, int nt,
                                                  int steps_per, int nsteps, float* __restrict__ part) {
    int t = blockIdx.x, tr = 0;
    while (t >= nt - tr) { t -= nt - tr; ++tr; }
    const int tc = tr + t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = tr * GT + (wave >> 1) * 64, c0 = tc * GT + (wave & 1) * 64;
    const long row_stride = (long)D * hw;
    const int s0 = blockIdx.y * steps_per, s1 = min(s0 + steps_per, nsteps);
    const int lr = lane & 15, lk = (lane >> 4) * 8;
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 ra[4], rb[4], na[4], nb[4];
    auto load = [&](int s, bf16x8 (&fa)[4], bf16x8 (&fb)[4]) {
        const long kk0 = (long)s * 32 + lk;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            fa[f] = gram_frag<ALIGNED>(x, r0 + f * 16 + lr, C, row_stride, kk0, K, hw);
            fb[f] = gram_frag<ALIGNED>(x, c0 + f * 16 + lr, C, row_stride, kk0, K, hw);
        }
    };
    if (s0 < s1) load(s0, ra, rb);
    for (int s = s0; s < s1; ++s) {
        if (s + 1 < s1) load(s + 1, na, nb);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = mfma16x16x32<true>(ra[a], rb[b], acc[a][b]);
#pragma unroll
        for (int f = 0; f < 4; ++f) { ra[f] = na[f]; rb[f] = nb[f]; }
    }
    // D layout of the 16x16 MFMA: lane -> column lane%16, rows 4*(lane/16) .. +3 (4 consecutive rows -> one 16-B store)
    float* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * GT * GT;
    const int rl0 = (wave >> 1) * 64, cl0 = (wave & 1) * 64;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int rl = rl0 + a * 16 + (lane >> 4) * 4, cl = cl0 + b * 16 + (lane & 15);
            *(f32x4*)(out + cl * GT + rl) = acc[a][b];
        }
}

// G[a][b] = G[b][a] = fp64 sum over the K splits in split order, from the a <= b entries only (exactly symmetric);
// block (tile, 256 consecutive partial entries)
__global__ __launch_bounds__(256) void k_pca_gram_reduce(const float* __restrict__ part, int C, int nt, int ntiles, int splits,
                                                         double* __restrict__ gram) {
    int t = blockIdx.x, tr = 0;
    while (t >= nt - tr) { t -= nt - tr; ++tr; }
    const int tc = tr + t;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int cl = e / GT, rl = e - cl * GT;
    const int a = tr * GT + rl, b = tc * GT + cl;
    if (a >= C || b >= C || a > b) return;
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)part[((long)k * ntiles + blockIdx.x) * GT * GT + e];
    gram[(long)a * C + b] = s;
    gram[(long)b * C + a] = s;
}

// s[c] = sum over the selected rows of channel c, fp64 (exact: fp16 values), fixed-order tree
__global__ __launch_bounds__(256) void k_pca_colsum(const uint16_t* __restrict__ x, int D, int hw, long K, double* __restrict__ sums) {
    __shared__ double red[256];
    const uint16_t* row = x + (long)blockIdx.x * D * hw;
    double s = 0.0;
    for (long kk = threadIdx.x; kk < K; kk += 256) {
        const long j = kk / hw, p = kk - j * hw;
        s += (double)h2f(row[j * PCA_STEP * hw + p]);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

// P[i][n] = sum_c V[i][c] (x[c][n] - mu[c]).  Block = 64 selected pixels (one per lane: each channel's read is coalesced) x
// PROJ_WAVES waves, wave k summing channels [k*C/PROJ_WAVES, (k+1)*C/PROJ_WAVES) in order; the wave partials are added in
// wave order (deterministic)
constexpr int PROJ_WAVES = 16;
__global__ __launch_bounds__(64 * PROJ_WAVES) void k_pca_project(const uint16_t* __restrict__ x, int C, int D, int hw, long K,
                                                                 const float* __restrict__ mean, const float* __restrict__ comps,
                                                                 float* __restrict__ proj) {
    __shared__ float red[PROJ_WAVES][3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = (long)blockIdx.x * 64 + lane;
    const int c0 = (int)((long)C * wave / PROJ_WAVES), c1 = (int)((long)C * (wave + 1) / PROJ_WAVES);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (n < K) {
        const long j = n / hw, p = n - j * hw;
        const uint16_t* px = x + j * PCA_STEP * hw + p;
        const long cs = (long)D * hw;
#pragma unroll 8
        for (int c = c0; c < c1; ++c) {
            const float d = h2f(px[c * cs]) - mean[c];
            a0 = fmaf(comps[c], d, a0);
            a1 = fmaf(comps[C + c], d, a1);
            a2 = fmaf(comps[2 * C + c], d, a2);
        }
    }
    red[wave][0][lane] = a0;
    red[wave][1][lane] = a1;
    red[wave][2][lane] = a2;
    __syncthreads();
    if (wave < 3 && n < K) {
        float s = red[0][wave][lane];
        for (int k = 1; k < PROJ_WAVES; ++k) s += red[k][wave][lane];
        proj[wave * K + n] = s;
    }
}

// U[i][j][Y][X] = torch bicubic x2 (align_corners=False, A = -0.75) of P[i][j][h][w]; per-block channel min / max partials
__global__ __launch_bounds__(256) void k_pca_upsample(const float* __restrict__ proj, int Dp, int h, int w, float* __restrict__ up,
                                                      float* __restrict__ mm_part) {
    __shared__ float red[4][6];
    const long total = (long)Dp * 4 * h * w;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        const int X = (int)(o % (2 * w));
        const long t1 = o / (2 * w);
        const int Y = (int)(t1 % (2 * h));
        const long j = t1 / (2 * h);
        // source coordinate 0.5 * (dst + 0.5) - 0.5: floor = dst/2 - (even), fraction 0.75 (even dst) / 0.25 (odd dst)
        const int iy = (Y >> 1) - 1 + (Y & 1), ix = (X >> 1) - 1 + (X & 1);
        float wy[4], wx[4];
        cubic_taps((Y & 1) ? 0.25f : 0.75f, wy);
        cubic_taps((X & 1) ? 0.25f : 0.75f, wx);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* src = proj + ((long)ch * Dp + j) * h * w;
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int yy = min(max(iy - 1 + a, 0), h - 1);
                float rowv = 0.f;
#pragma unroll
                for (int b = 0; b < 4; ++b) rowv += wx[b] * src[(long)yy * w + min(max(ix - 1 + b, 0), w - 1)];
                acc += wy[a] * rowv;
            }
            up[(long)ch * total + o] = acc;
            mn[ch] = fminf(mn[ch], acc);
            mx[ch] = fmaxf(mx[ch], acc);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a = -wave_max(-mn[ch]), b = wave_max(mx[ch]);
        if (lane == 0) { red[wave][ch] = a; red[wave][3 + ch] = b; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const bool is_min = threadIdx.x < 3;
        float v = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) v = is_min ? fminf(v, red[k][threadIdx.x]) : fmaxf(v, red[k][threadIdx.x]);
        mm_part[blockIdx.x * 8 + threadIdx.x] = v;
    }
}

// whole-volume min / max of the data (uint8 or fp32), per-block partials
template <bool U8>
__global__ __launch_bounds__(256) void k_pca_data_minmax(const void* __restrict__ data, long n, float* __restrict__ mm_part) {
    __shared__ float red[4][2];
    float mn = INFINITY, mx = -INFINITY;
    constexpr int E = U8 ? 16 : 4;  // elements per 16-B load
    const long nv = ((uintptr_t)data & 15) ? 0 : n / E;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        const uint4 q = ((const uint4*)data)[i];
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (U8) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float v = (float)((wd[k] >> (8 * b)) & 0xff);
                    mn = fminf(mn, v);
                    mx = fmaxf(mx, v);
                }
            } else {
                const float v = __uint_as_float(wd[k]);
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
        }
    }
    for (long i = nv * E + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {  // tail / unaligned
        const float v = U8 ? (float)((const uint8_t*)data)[i] : ((const float*)data)[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    if (lane == 0) { red[wave][0] = mn; red[wave][1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { mn = fminf(mn, red[k][0]); mx = fmaxf(mx, red[k][1]); }
        mm_part[blockIdx.x * 8 + 6] = mn;
        mm_part[blockIdx.x * 8 + 7] = mx;
    }
}

// mm[0..2] colour-channel minima, [3..5] maxima, [6] data min, [7] data max
// one wave per value; min / max are exact, so the result does not depend on the order
__global__ __launch_bounds__(512) void k_pca_minmax_finalize(const float* __restrict__ mm_part, int nblk, float* __restrict__ mm) {
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const bool is_min = q < 3 || q == 6;
    float v = is_min ? INFINITY : -INFINITY;
    for (int k = lane; k < nblk; k += 64) v = is_min ? fminf(v, mm_part[k * 8 + q]) : fmaxf(v, mm_part[k * 8 + q]);
    v = is_min ? -wave_max(-v) : wave_max(v);
    if (lane == 0) mm[q] = v;
}

// numpy float32 `%` 1.0: fmod, then + 1.0 when the remainder is negative (npy_divmodf)
__device__ __forceinline__ float np_mod1(float a) {
    float m = fmodf(a, 1.0f);
    if (m != 0.f) {
        if (m < 0.f) m = __fadd_rn(m, 1.0f);
    } else {
        m = 0.f;
    }
    return m;
}

// cryovit _color_features for one pixel, operation for operation as numpy / matplotlib 3.x evaluate it: min-max
// normalisation and rgb_to_hsv in float32 (blue over green over red on ties), s = 0.9, v = 0.75, hsv_to_rgb (its f, q, t
// in float64: float32 minus the int64 sector index promotes), 255 * rgb in float32, truncation to uint8.
__device__ void pca_colour(const float u[3], const float* __restrict__ mm, uint8_t rgb[3]) {
#pragma clang fp contract(off)
    float c[3];
    bool defined = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sub = u[k] - mm[k];
        const float top = mm[3 + k] - mm[k];  // max over the block of (u - min): rounding is monotonic
        c[k] = sub / top;
        // a channel that is constant over the block is 0 / 0 in numpy; its NaN goes through arr.max(-1) and ptp, `delta > 0` is
        // false and the hue stays 0.  fmaxf / fminf would drop the NaN and take a hue from the other two channels.
        defined = defined && top > 0.f && c[k] == c[k];
    }
    const float amax = fmaxf(fmaxf(c[0], c[1]), c[2]), amin = fminf(fminf(c[0], c[1]), c[2]);
    const float delta = amax - amin;
    float hue = 0.f;
    if (defined && delta > 0.f) {
        if (c[2] == amax) hue = 4.0f + (c[0] - c[1]) / delta;
        else if (c[1] == amax) hue = 2.0f + (c[2] - c[0]) / delta;
        else if (c[0] == amax) hue = (c[1] - c[2]) / delta;
    }
    hue = np_mod1(hue / 6.0f);
    const float s = 0.9f, v = 0.75f;
    const float h6 = hue * 6.0f;
    const long i = (long)h6;
    const double f = (double)h6 - (double)i;
    const float p = v * (1.0f - s);
    const float q = (float)((double)v * (1.0 - (double)s * f));
    const float t = (float)((double)v * (1.0 - (double)s * (1.0 - f)));
    float r, g, b;
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
    rgb[0] = (uint8_t)(int)(255.0f * r);
    rgb[1] = (uint8_t)(int)(255.0f * g);
    rgb[2] = (uint8_t)(int)(255.0f * b);
}

// grey value of one data voxel: (d - min) / (max - min) * 255, float64 for uint8 data (numpy promotes), float32 for fp32
template <bool U8>
__device__ __forceinline__ uint8_t pca_grey(const void* __restrict__ data, long off, const float* __restrict__ mm) {
#pragma clang fp contract(off)
    if constexpr (U8) {
        const uint8_t d = ((const uint8_t*)data)[off];
        const int lo = (int)mm[6], span = (int)mm[7] - lo;
        if (span == 0) return 0;
        const double g = (double)(uint8_t)(d - lo) / (double)span * 255.0;
        return (uint8_t)(int)g;
    } else {
        const float sub = ((const float*)data)[off] - mm[6];
        const float top = mm[7] - mm[6];
        const float g = top > 0.f ? sub / top * 255.0f : 0.f;  // a constant volume is 0 / 0 in numpy, which nan_to_num makes 0
        return g == g ? (uint8_t)(int)g : 0;                   // a NaN voxel likewise; never cast a NaN
    }
}

// canvas [Dp][16h][32w][3] uint8, one thread per 16 bytes of a row (a row is 96w bytes): the data slice idx = 10 j (flipped,
// grey, H x W at the origin), the colour map of slice j (flipped, each upsampled pixel as an 8x8 block) at column x_map
template <bool U8>
__global__ __launch_bounds__(256) void k_pca_canvas(const float* __restrict__ up, const void* __restrict__ data, const float* __restrict__ mm,
                                                    int Dp, int H, int W, int h, int w, int x_map, uint8_t* __restrict__ canvas) {
    const int CW = 32 * w, CH = 16 * h, chunks_row = 6 * w;
    const long total = (long)Dp * CH * chunks_row;
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int xc = (int)(o % chunks_row);
    const long t1 = o / chunks_row;
    const int y = (int)(t1 % CH);
    const int j = (int)(t1 / CH);
    const long plane = (long)4 * h * w, uD = (long)Dp * plane;
    uint8_t bytes[16];
    int last_x = -1;
    uint8_t px[3] = {0, 0, 0};
    for (int b = 0; b < 16; ++b) {
        const int byte = xc * 16 + b, x = byte / 3, ch = byte - x * 3;
        if (x != last_x) {
            last_x = x;
            px[0] = px[1] = px[2] = 0;
            if (x < W && y < H) {
                const uint8_t g = pca_grey<U8>(data, ((long)j * PCA_STEP * H + (H - 1 - y)) * W + x, mm);
                px[0] = px[1] = px[2] = g;
            } else if (x >= x_map && x - x_map < 16 * w && x < CW) {
                const int uy = (CH - 1 - y) >> 3, ux = (x - x_map) >> 3;
                const long ui = j * plane + (long)uy * 2 * w + ux;
                const float u[3] = {up[ui], up[uD + ui], up[2 * uD + ui]};
                pca_colour(u, mm, px);
            }
        }
        bytes[b] = px[ch];
    }
    u32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        v[k] = bytes[4 * k] | ((uint32_t)bytes[4 * k + 1] << 8) | ((uint32_t)bytes[4 * k + 2] << 16) | ((uint32_t)bytes[4 * k + 3] << 24);
    *(u32x4*)(canvas + ((long)j * CH + y) * (3L * CW) + (long)xc * 16) = v;
}

}  // namespace cvx

using namespace cvx;

static bool pca_dims_ok(int C, int D, int hw) { return C > 0 && D > 0 && hw > 0 && (long)C * D * hw < (1L << 40); }

extern "C" long cvx_pca_moments_scratch_bytes(int C, int D, int hw) {
    if (!pca_dims_ok(C, D, hw)) return cvx_fail("pca_moments_scratch_bytes: C, D, hw must be positive");
    const GramPlan p = gram_plan(C, D, hw);
    return (long)p.splits * p.ntiles * GT * GT * (long)sizeof(float);
}

extern "C" int cvx_pca_moments_f16(const void* feats, int C, int D, int hw, double* sums, double* gram, void* scratch,
                                   long scratch_bytes, hipStream_t st) {
    if (!pca_dims_ok(C, D, hw)) return cvx_fail("pca_moments: C, D, hw must be positive");
    if (!feats || !sums || !gram || !scratch) return cvx_fail("pca_moments: null pointer");
    const GramPlan p = gram_plan(C, D, hw);
    if (scratch_bytes < (long)p.splits * p.ntiles * GT * GT * (long)sizeof(float))
        return cvx_fail("pca_moments: scratch smaller than cvx_pca_moments_scratch_bytes()");
    const long K = (long)((D + PCA_STEP - 1) / PCA_STEP) * hw;
    const bool aligned = hw % 8 == 0 && ((uintptr_t)feats & 15) == 0;
    const dim3 grid(p.ntiles, p.splits);
    if (aligned)
        hipLaunchKernelGGL(k_pca_gram<true>, grid, dim3(256), 0, st, (const uint16_t*)feats, C, D, hw, K, p.nt, p.steps_per, p.nsteps,
                           (float*)scratch);
    else
        hipLaunchKernelGGL(k_pca_gram<false>, grid, dim3(256), 0, st, (const uint16_t*)feats, C, D, hw, K, p.nt, p.steps_per, p.nsteps,
                           (float*)scratch);
    if (int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_pca_gram_reduce, dim3(p.ntiles, GT * GT / 256), dim3(256), 0, st, (const float*)scratch, C, p.nt, p.ntiles, p.splits, gram);
    if (int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_pca_colsum, dim3(C), dim3(256), 0, st, (const uint16_t*)feats, D, hw, K, sums);
    return cvx_check_launch();
}

extern "C" int cvx_pca_project_f16(const void* feats, int C, int D, int hw, const float* mean, const float* comps, float* proj,
                                   hipStream_t st) {
    if (!pca_dims_ok(C, D, hw)) return cvx_fail("pca_project: C, D, hw must be positive");
    if (!feats || !mean || !comps || !proj) return cvx_fail("pca_project: null pointer");
    const long K = (long)((D + PCA_STEP - 1) / PCA_STEP) * hw;
    hipLaunchKernelGGL(k_pca_project, dim3((unsigned)((K + 63) / 64)), dim3(64 * PROJ_WAVES), 0, st, (const uint16_t*)feats, C, D, hw, K, mean,
                       comps, proj);
    return cvx_check_launch();
}

extern "C" long cvx_pca_colormap_scratch_bytes(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return cvx_fail("pca_colormap_scratch_bytes: D, H, W must be positive");
    const long Dp = (D + PCA_STEP - 1) / PCA_STEP, h = (H + 15) / 16, w = (W + 15) / 16;
    return (3 * Dp * 4 * h * w + 2L * MM_BLOCKS * 8 + 8) * (long)sizeof(float);
}

extern "C" int cvx_pca_colormap(const float* proj, const void* data, int is_u8, int D, int H, int W, int x_map, uint8_t* canvas,
                                void* scratch, long scratch_bytes, hipStream_t st) {
    if (D <= 0 || H <= 0 || W <= 0) return cvx_fail("pca_colormap: D, H, W must be positive");
    if (!proj || !data || !canvas || !scratch) return cvx_fail("pca_colormap: null pointer");
    const int Dp = (D + PCA_STEP - 1) / PCA_STEP, h = (H + 15) / 16, w = (W + 15) / 16;
    if (x_map < 0) return cvx_fail("pca_colormap: x_map must be >= 0");
    if (scratch_bytes < cvx_pca_colormap_scratch_bytes(D, H, W))
        return cvx_fail("pca_colormap: scratch smaller than cvx_pca_colormap_scratch_bytes()");
    if ((uintptr_t)canvas & 15) return cvx_fail("pca_colormap: canvas must be 16-byte aligned");
    float* up = (float*)scratch;
    float* mm_part = up + 3L * Dp * 4 * h * w;  // [MM_BLOCKS][8]: colour min/max in 0..5, data min/max in 6..7
    float* mm = mm_part + 2L * MM_BLOCKS * 8;
    hipLaunchKernelGGL(k_pca_upsample, dim3(MM_BLOCKS), dim3(256), 0, st, proj, Dp, h, w, up, mm_part);
    if (int rc = cvx_check_launch()) return rc;
    const long n = (long)D * H * W;
    if (is_u8)
        hipLaunchKernelGGL(k_pca_data_minmax<true>, dim3(MM_BLOCKS), dim3(256), 0, st, data, n, mm_part);
    else
        hipLaunchKernelGGL(k_pca_data_minmax<false>, dim3(MM_BLOCKS), dim3(256), 0, st, data, n, mm_part);
    if (int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_pca_minmax_finalize, dim3(1), dim3(512), 0, st, mm_part, MM_BLOCKS, mm);
    if (int rc = cvx_check_launch()) return rc;
    const long chunks = (long)Dp * 16 * h * 6 * w;
    const unsigned nblk = (unsigned)((chunks + 255) / 256);
    if (is_u8)
        hipLaunchKernelGGL(k_pca_canvas<true>, dim3(nblk), dim3(256), 0, st, up, data, mm, Dp, H, W, h, w, x_map, canvas);
    else
        hipLaunchKernelGGL(k_pca_canvas<false>, dim3(nblk), dim3(256), 0, st, up, data, mm, Dp, H, W, h, w, x_map, canvas);
    return cvx_check_launch();
}
