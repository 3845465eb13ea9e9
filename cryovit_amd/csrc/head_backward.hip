// Backward of the CryoVIT segmentation head: the arithmetic the forward kernels have no counterpart for.
//   cvx_conv_wgrad_f16          dW[o][tap*C + c] = sum_v dz[v][o] x[v + shift(tap)][c]  and  db[o] = sum_v dz[v][o]
//   cvx_gelu_f16                y = gelu(z): the training forward keeps z and y (the kernels run with act = 0)
//   cvx_gelu_backward_f16       dz = dy (Phi(z) + z phi(z)), optionally written in the (1,2,2)-unshuffled row layout
//   cvx_groupnorm_backward_f16  dx, dgamma, dbeta from the forward's group sums
//   cvx_conv3_out_backward      the 8 -> 1 output convolution: dy_mid, dW, db from the fp32 logit gradient
//   cvx_unscale_check_f32       g *= 1 / loss scale and one "all finite" flag for the whole flat gradient
// The data gradients of the 3x3x3 and the transposed convolutions run on cvx_conv3d_f16 / cvx_gemm_bf16 with repacked weights
// (engine/head_train.py).  No floating-point atomics anywhere: every reduction is block partials in a workspace followed by a
// fixed-order finalize, and the number of slabs is a function of the shape alone, so results are bit-reproducible.
#include "common.h"
#include "../../include/cryovit_hip.h"
#include "entry_checks.h"

using namespace cvx;

namespace {

constexpr int kWgChunk = 64;        // voxels (along W) staged per step: two MFMA K steps of 32
constexpr int kWgCols = 64;         // k columns (tap*C + c) per workgroup
constexpr int kWgLdsRow = 72;       // halfs per LDS tile row: 64 + 8 of padding (144 B: 16-B aligned rows that do not share banks)
constexpr int kWgTargetBlocks = 2048;
constexpr int kSumSlabsMax = 1024;  // of the column-sum, GroupNorm and output-layer reductions

struct WgShape {
    int C, cout, taps, dil, D, H, W;
    long KT;      // taps * C
    int wchunks;  // chunks per line
    long nch;     // chunks in the volume
    long cps;     // chunks per slab
    int slabs, oblocks, kblocks;  // workgroups: oblocks (16 * OTB outputs each) x kblocks (64 columns each) x slabs
};

inline int wg_otb(int cout) { return cout <= 16 ? 1 : cout <= 32 ? 2 : 4; }  // 16-row output tiles per workgroup

// the slab count depends on the shape only
bool wg_shape(int C, int cout, int taps, int dil, int D, int H, int W, WgShape& s) {
    s.C = C; s.cout = cout; s.taps = taps; s.dil = dil; s.D = D; s.H = H; s.W = W;
    s.KT = (long)taps * C;
    s.wchunks = (W + kWgChunk - 1) / kWgChunk;
    s.nch = (long)D * H * s.wchunks;
    s.oblocks = (cout + 16 * wg_otb(cout) - 1) / (16 * wg_otb(cout));
    s.kblocks = (int)((s.KT + kWgCols - 1) / kWgCols);
    const long units = (long)s.oblocks * s.kblocks;
    if (units > 0x7fffffffL) return false;
    long slabs = (kWgTargetBlocks + units - 1) / units;
    const long most = (s.nch + 3) / 4;  // at least four chunks per slab
    if (slabs > most) slabs = most;
    if (slabs < 1) slabs = 1;
    s.cps = (s.nch + slabs - 1) / slabs;
    if (s.cps < 1) s.cps = 1;
    s.slabs = (int)((s.nch + s.cps - 1) / s.cps);
    if (s.slabs < 1) s.slabs = 1;
    return s.slabs <= 65535;
}

// A GEMM whose K is the voxel index while both operands are stored voxel-major.  One workgroup per (16 * OTB outputs o) x (64
// columns k = tap*C + c) x (slab of 64-voxel chunks of a line).  Per chunk the 256 threads stage the dz tile [64 voxels][16 * OTB o]
// and the tap-shifted x tile [64 voxels][64 k] in LDS by channel-contiguous 8-B / 16-B loads (each 8-column piece of the x tile has
// its own tap, hence its own shift; every address comes from in-volume coordinates, everything outside the volume, past cout or
// past taps*C is staged as zeros, so padded taps add exact zeros), prefetching the next chunk into registers under the MFMAs.
// The MFMA wants 8 consecutive voxels of ONE column per lane: ds_read_b64_tr_b16 delivers that from the row-major tiles (a
// 16-lane group reads a 4-voxel x 16-column block, lane li the voxel li / 4, columns 4 (li % 4) .., and receives column li of the
// four voxels).  The waves split the workgroup's 16 x 16 tiles: OTB = 4: wave w owns output tile w and the four column tiles,
// OTB = 2: output tile w & 1 and two column tiles, OTB = 1: the one output tile and column tile w.  fp32 accumulation.
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef short v8s_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 wg_frag(const uint16_t* tile, int row0, int col0, int lane) {
    typedef __attribute__((address_space(3))) v4s_t* lds_v4;
    const int li = lane & 15, g = lane >> 4;
    const uint16_t* p = tile + (row0 + 8 * g + (li >> 2)) * kWgLdsRow + col0 + 4 * (li & 3);
    const v4s_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)p);
    const v4s_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * kWgLdsRow));
    return __builtin_bit_cast(bf16x8, v8s_t{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]});
}

template <int OTB>
__global__ __launch_bounds__(256) void k_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dz, float* __restrict__ part,
                                               WgShape s) {
    __shared__ __attribute__((aligned(16))) uint16_t sA[kWgChunk * kWgLdsRow];
    __shared__ __attribute__((aligned(16))) uint16_t sB[kWgChunk * kWgLdsRow];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ob = (int)(blockIdx.x % s.oblocks), kb = (int)(blockIdx.x / s.oblocks);
    const int o0 = ob * 16 * OTB;
    const long k0 = (long)kb * kWgCols;

    // loader roles.  x tile: the 16-B piece bp of rows br and br + 32; dz tile: OTB 8-B pieces (4 outputs each)
    const int bp = tid & 7, br = tid >> 3;
    const long bk = k0 + 8 * bp;
    const bool bk_ok = bk < s.KT;
    const int btap = bk_ok ? (int)(bk / s.C) : 0, bc = bk_ok ? (int)(bk % s.C) : 0;
    int dzo = 0, dyo = 0, dxo = 0;
    if (s.taps == 27) { dzo = (btap / 9 - 1) * s.dil; dyo = (btap / 3) % 3 - 1; dxo = btap % 3 - 1; }
    int arow[OTB], acol[OTB];
#pragma unroll
    for (int e = 0; e < OTB; ++e) {
        const int q = tid + 256 * e;
        arow[e] = q / (4 * OTB);
        acol[e] = 4 * (q % (4 * OTB));
    }

    uint2 ra[OTB];
    uint4 rb[2];
    auto fetch = [&](long ch) {
        const long line = ch / s.wchunks;
        const int xc = (int)(ch % s.wchunks) * kWgChunk;
        const int z = (int)(line / s.H), y = (int)(line % s.H);
#pragma unroll
        for (int e = 0; e < OTB; ++e) {
            const int xx = xc + arow[e], o = o0 + acol[e];
            ra[e] = (xx < s.W && o < s.cout) ? *(const uint2*)(dz + (line * s.W + xx) * (long)s.cout + o) : uint2{0u, 0u};
        }
        const int zz = z + dzo, yy = y + dyo;
        const bool ok = bk_ok && zz >= 0 && zz < s.D && yy >= 0 && yy < s.H;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int xj = xc + br + 32 * hh, xs = xj + dxo;
            rb[hh] = (ok && xj < s.W && xs >= 0 && xs < s.W) ? *(const uint4*)(x + (((long)zz * s.H + yy) * s.W + xs) * (long)s.C + bc)
                                                              : uint4{0u, 0u, 0u, 0u};
        }
    };

    const int ot = OTB == 4 ? wave : OTB == 2 ? (wave & 1) : 0;  // this wave's output tile and first column tile
    const int ct0 = OTB == 4 ? 0 : OTB == 2 ? 2 * (wave >> 1) : wave;
    f32x4 acc[OTB];
#pragma unroll
    for (int t = 0; t < OTB; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const long ch0 = (long)blockIdx.y * s.cps, ch1 = min(s.nch, ch0 + s.cps);
    if (ch0 < ch1) fetch(ch0);
    for (long ch = ch0; ch < ch1; ++ch) {
#pragma unroll
        for (int e = 0; e < OTB; ++e) *(uint2*)(sA + arow[e] * kWgLdsRow + acol[e]) = ra[e];
        *(uint4*)(sB + br * kWgLdsRow + 8 * bp) = rb[0];
        *(uint4*)(sB + (br + 32) * kWgLdsRow + 8 * bp) = rb[1];
        __syncthreads();
        if (ch + 1 < ch1) fetch(ch + 1);  // (in flight under the MFMAs)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 af = wg_frag(sA, 32 * ks, 16 * ot, lane);
#pragma unroll
            for (int t = 0; t < OTB; ++t) acc[t] = mfma16x16x32<true>(af, wg_frag(sB, 32 * ks, 16 * (ct0 + t), lane), acc[t]);
        }
        __syncthreads();  // every wave is done with the tiles before they are overwritten
    }
    float* dst = part + (long)blockIdx.y * s.cout * s.KT;
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < OTB; ++t) {
        const long kk = k0 + 16 * (ct0 + t) + i;  // this lane's column; its rows are the tile's g*4 + e
        if (kk >= s.KT) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int oo = o0 + 16 * ot + g * 4 + e;
            if (oo < s.cout) dst[(long)oo * s.KT + kk] = acc[t][e];
        }
    }
}

// out[i] = part[0][i] + part[1][i] + ... in slab order
__global__ __launch_bounds__(256) void k_slab_sum(const float* __restrict__ part, float* __restrict__ out, long n, int slabs) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = part[i];
    for (int sl = 1; sl < slabs; ++sl) acc += part[(long)sl * n + i];
    out[i] = acc;
}

// column sums of fp16 rows: block partials [slab][cols], then k_colsum_final in slab order (fp64, one rounding)
__global__ __launch_bounds__(256) void k_colsum_part(const uint16_t* __restrict__ a, long rows, int cols, long rows_per_slab,
                                                     float* __restrict__ part) {
    __shared__ float red[4][64];
    const int col = blockIdx.y * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.x * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
    float acc = 0.f;
    if (col < cols)
        for (long r = r0 + rl; r < r1; r += 4) acc += h2f(a[r * cols + col]);
    red[rl][threadIdx.x & 63] = acc;
    __syncthreads();
    if (rl == 0 && col < cols) part[(long)blockIdx.x * cols + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void k_colsum_final(const float* __restrict__ part, int slabs, int cols, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    double acc = 0.0;
    for (int sl = 0; sl < slabs; ++sl) acc += (double)part[(long)sl * cols + c];
    out[c] = (float)acc;
}

// ---- GELU forward (training keeps z and y) and backward ------------------------------------------------------------------------

__device__ __forceinline__ float gelu_grad(float z) {  // Phi(z) + z phi(z), exact-erf GELU; erfc keeps both tails accurate
    const float cdf = 0.5f * erfcf(-z * 0.70710678118654752440f);
    const float pdf = 0.39894228040143267794f * expf(-0.5f * z * z);
    return fmaf(z, pdf, cdf);
}

__global__ __launch_bounds__(256) void k_gelu(const uint16_t* __restrict__ z, uint16_t* __restrict__ y, long n) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (i0 + 8 <= n) {
        const uint4 u = *(const uint4*)(z + i0);
        uint4 o;
        o.x = pack2h(gelu_erf(hlo(u.x)), gelu_erf(hhi(u.x)));
        o.y = pack2h(gelu_erf(hlo(u.y)), gelu_erf(hhi(u.y)));
        o.z = pack2h(gelu_erf(hlo(u.z)), gelu_erf(hhi(u.z)));
        o.w = pack2h(gelu_erf(hlo(u.w)), gelu_erf(hhi(u.w)));
        *(uint4*)(y + i0) = o;
    } else {
        for (long i = i0; i < n; ++i) y[i] = f2h(gelu_erf(h2f(z[i])));
    }
}

__device__ __forceinline__ uint4 gelu_bwd8(const uint4& d, const uint4& u) {
    uint4 o;
    o.x = pack2h(hlo(d.x) * gelu_grad(hlo(u.x)), hhi(d.x) * gelu_grad(hhi(u.x)));
    o.y = pack2h(hlo(d.y) * gelu_grad(hlo(u.y)), hhi(d.y) * gelu_grad(hhi(u.y)));
    o.z = pack2h(hlo(d.z) * gelu_grad(hlo(u.z)), hhi(d.z) * gelu_grad(hhi(u.z)));
    o.w = pack2h(hlo(d.w) * gelu_grad(hlo(u.w)), hhi(d.w) * gelu_grad(hhi(u.w)));
    return o;
}

// elementwise; 8 elements per thread (the buffers are 16-B aligned, checked by the entry), a scalar tail
__global__ __launch_bounds__(256) void k_gelu_bwd(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ z, uint16_t* __restrict__ dz,
                                                  long n) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (i0 + 8 <= n) {
        *(uint4*)(dz + i0) = gelu_bwd8(*(const uint4*)(dy + i0), *(const uint4*)(z + i0));
    } else {
        for (long i = i0; i < n; ++i) dz[i] = f2h(h2f(dy[i]) * gelu_grad(h2f(z[i])));
    }
}

// dy, z: [D][2H][2W][c3]  ->  dz rows [D*H*W][4*c3], column (i*2 + j)*c3 + o of row (z, y, x) = the voxel (z, 2y+i, 2x+j): the
// inverse of the transposed convolution's pixel shuffle.  One thread per 8 output columns.
__global__ __launch_bounds__(256) void k_gelu_bwd_unshuffle(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ z,
                                                            uint16_t* __restrict__ dz, long nv, int H, int W, int c3) {
    const int c8 = c3 >> 3;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nv * 4 * c8) return;
    const int oc = (int)(t % c8), ij = (int)((t / c8) % 4);
    const long v = t / (4 * c8);
    const int xx = (int)(v % W), yy = (int)((v / W) % H);
    const long zz = v / ((long)W * H);
    const long src = (((zz * 2 * H + 2 * yy + (ij >> 1)) * 2 * W) + 2 * xx + (ij & 1)) * (long)c3 + oc * 8;
    *(uint4*)(dz + v * 4 * c3 + ij * c3 + oc * 8) = gelu_bwd8(*(const uint4*)(dy + src), *(const uint4*)(z + src));
}

// ---- GroupNorm backward --------------------------------------------------------------------------------------------------------

// mean and rstd of the 8 channels a thread owns, from the forward's published fp32 group sums with its fp64 arithmetic (norm.hip:322-329)
__device__ __forceinline__ void gn_moments8(const float* stats, int c0, int C, int G, long nvox, float eps, float* mean, float* rstd) {
    const int cpg = C / G;
    const double cnt = (double)nvox * cpg;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int gidx = (c0 + e) / cpg;
        const double m = (double)stats[gidx] / cnt;
        double var = (double)stats[G + gidx] / cnt - m * m;
        var = var < 0.0 ? 0.0 : var;
        mean[e] = (float)m;
        rstd[e] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// per slab and channel: sum dn | sum dn xhat   (thread layout of k_gn_stats: lane-private sums -> LDS -> summed in thread order)
__global__ __launch_bounds__(256) void k_gnb_part(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dn, const float* __restrict__ stats,
                                                  float* __restrict__ part, long nvox, int C, int G, float eps, long vox_per_block) {
    __shared__ float red[256][17];
    const int tid = threadIdx.x;
    const int cpt = C >> 3;
    const int cidx = tid % cpt, vstride = 256 / cpt;
    const int vsub = tid / cpt < vstride ? tid / cpt : -1;
    float mean[8], rstd[8], s[8], q[8];
    gn_moments8(stats, cidx * 8, C, G, nvox, eps, mean, rstd);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
    const long v0 = (long)blockIdx.x * vox_per_block, v1 = min(nvox, v0 + vox_per_block);
    for (long v = vsub < 0 ? v1 : v0 + vsub; v < v1; v += vstride) {
        const uint4 ux = *(const uint4*)(x + v * C + cidx * 8), ud = *(const uint4*)(dn + v * C + cidx * 8);
        const uint32_t wx[4] = {ux.x, ux.y, ux.z, ux.w}, wd[4] = {ud.x, ud.y, ud.z, ud.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d0 = hlo(wd[e]), d1 = hhi(wd[e]);
            s[2 * e] += d0; q[2 * e] += d0 * ((hlo(wx[e]) - mean[2 * e]) * rstd[2 * e]);
            s[2 * e + 1] += d1; q[2 * e + 1] += d1 * ((hhi(wx[e]) - mean[2 * e + 1]) * rstd[2 * e + 1]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[tid][e] = s[e]; red[tid][8 + e] = q[e]; }
    __syncthreads();
    for (int k = tid; k < 2 * C; k += 256) {
        const int c = k < C ? k : k - C, col = (c & 7) + (k < C ? 0 : 8);
        float acc = 0.f;
        for (int vs = 0; vs < vstride; ++vs) acc += red[vs * cpt + (c >> 3)][col];
        part[(long)blockIdx.x * 2 * C + k] = acc;
    }
}

// one wave per group: dgamma, dbeta of its channels (slabs added in order, fp64) and the group means m1 = mean(gamma dn),
// m2 = mean(gamma dn xhat) -> gm[g], gm[G + g]
__global__ __launch_bounds__(64) void k_gnb_final(const float* __restrict__ part, int slabs, const float* __restrict__ gamma, float* __restrict__ dgamma,
                                                  float* __restrict__ dbeta, float* __restrict__ gm, long nvox, int C, int G) {
    const int g = blockIdx.x, lane = threadIdx.x, cpg = C / G;
    double a1 = 0.0, a2 = 0.0;
    for (int e = lane; e < cpg; e += 64) {
        const int c = g * cpg + e;
        double sb = 0.0, sg = 0.0;
        for (int sl = 0; sl < slabs; ++sl) {
            sb += (double)part[(long)sl * 2 * C + c];
            sg += (double)part[(long)sl * 2 * C + C + c];
        }
        dbeta[c] = (float)sb;
        dgamma[c] = (float)sg;
        a1 += (double)gamma[c] * sb;
        a2 += (double)gamma[c] * sg;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a1 += __shfl_xor(a1, o, 64); a2 += __shfl_xor(a2, o, 64); }
    if (lane == 0) {
        const double cnt = (double)nvox * cpg;
        gm[g] = (float)(a1 / cnt);
        gm[G + g] = (float)(a2 / cnt);
    }
}

// dx = rstd (gamma dn - m1 - xhat m2), fp32 math, one fp16 rounding
__global__ __launch_bounds__(256) void k_gnb_apply(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dn, const float* __restrict__ gamma,
                                                   const float* __restrict__ stats, const float* __restrict__ gm, uint16_t* __restrict__ dx,
                                                   long nvox, int C, int G, float eps, long vox_per_block) {
    const int tid = threadIdx.x;
    const int cpt = C >> 3;
    const int cidx = tid % cpt, vsub = tid / cpt, vstride = 256 / cpt;
    if (vsub >= vstride) return;
    float mean[8], rstd[8], gw[8], m1[8], m2[8];
    gn_moments8(stats, cidx * 8, C, G, nvox, eps, mean, rstd);
    const int cpg = C / G;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = cidx * 8 + e;
        gw[e] = gamma[c];
        m1[e] = gm[c / cpg];
        m2[e] = gm[G + c / cpg];
    }
    auto one = [&](float xv, float dv, int e) {
        const float xh = (xv - mean[e]) * rstd[e];
        return rstd[e] * (gw[e] * dv - m1[e] - xh * m2[e]);
    };
    const long v0 = (long)blockIdx.x * vox_per_block, v1 = min(nvox, v0 + vox_per_block);
    for (long v = v0 + vsub; v < v1; v += vstride) {
        const uint4 ux = *(const uint4*)(x + v * C + cidx * 8), ud = *(const uint4*)(dn + v * C + cidx * 8);
        uint4 o;
        o.x = pack2h(one(hlo(ux.x), hlo(ud.x), 0), one(hhi(ux.x), hhi(ud.x), 1));
        o.y = pack2h(one(hlo(ux.y), hlo(ud.y), 2), one(hhi(ux.y), hhi(ud.y), 3));
        o.z = pack2h(one(hlo(ux.z), hlo(ud.z), 4), one(hhi(ux.z), hhi(ud.z), 5));
        o.w = pack2h(one(hlo(ux.w), hlo(ud.w), 6), one(hhi(ux.w), hhi(ud.w), 7));
        *(uint4*)(dx + v * C + cidx * 8) = o;
    }
}

// ---- the output layer (8 -> 1, 3x3x3, fp32 weights) ----------------------------------------------------------------------------

// dy_mid[v][c] = sum_tap dlogit[v - tap] w[tap][c]: one thread per voxel, one 16-B store
__global__ __launch_bounds__(256) void k_out_bwd_data(const float* __restrict__ dlogit, const float* __restrict__ w, uint16_t* __restrict__ dy,
                                                      int D, int H, int W) {
    __shared__ float ws[216];
    if (threadIdx.x < 216) ws[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= (long)D * H * W) return;
    const int xx = (int)(v % W), yy = (int)((v / W) % H), zz = (int)(v / ((long)W * H));
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < 27; ++tap) {
        const int sz = zz - (tap / 9 - 1), sy = yy - ((tap / 3) % 3 - 1), sx = xx - (tap % 3 - 1);
        if (sz < 0 || sz >= D || sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
        const float gl = dlogit[((long)sz * H + sy) * W + sx];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = fmaf(gl, ws[tap * 8 + c], acc[c]);
    }
    uint4 o;
    o.x = pack2h(acc[0], acc[1]); o.y = pack2h(acc[2], acc[3]); o.z = pack2h(acc[4], acc[5]); o.w = pack2h(acc[6], acc[7]);
    *(uint4*)(dy + v * 8) = o;
}

// part[slab][tap*8 + c] = sum over the slab's voxels of dlogit[v] y_mid[v + tap][c]; part[slab][216] = sum dlogit.  A thread's
// sums go through a fixed xor tree inside its wave, the four waves are added in order.
__global__ __launch_bounds__(256) void k_out_bwd_weight(const float* __restrict__ dlogit, const uint16_t* __restrict__ ymid, float* __restrict__ part,
                                                        int D, int H, int W, long vox_per_block) {
    __shared__ float wred[4][8];
    const long nv = (long)D * H * W;
    const long v0 = (long)blockIdx.x * vox_per_block, v1 = min(nv, v0 + vox_per_block);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int tap = 0; tap <= 27; ++tap) {
        const int oz = tap / 9 - 1, oy = (tap / 3) % 3 - 1, ox = tap % 3 - 1;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (long v = v0 + threadIdx.x; v < v1; v += 256) {
            const float gl = dlogit[v];
            if (tap == 27) { acc[0] += gl; continue; }
            const int xx = (int)(v % W) + ox, yy = (int)((v / W) % H) + oy, zz = (int)(v / ((long)W * H)) + oz;
            if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const uint4 u = *(const uint4*)(ymid + (((long)zz * H + yy) * W + xx) * 8);
            acc[0] = fmaf(gl, hlo(u.x), acc[0]); acc[1] = fmaf(gl, hhi(u.x), acc[1]);
            acc[2] = fmaf(gl, hlo(u.y), acc[2]); acc[3] = fmaf(gl, hhi(u.y), acc[3]);
            acc[4] = fmaf(gl, hlo(u.z), acc[4]); acc[5] = fmaf(gl, hhi(u.z), acc[5]);
            acc[6] = fmaf(gl, hlo(u.w), acc[6]); acc[7] = fmaf(gl, hhi(u.w), acc[7]);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c) wred[wave][c] = acc[c];
        }
        __syncthreads();
        const int nc = tap == 27 ? 1 : 8;
        if (threadIdx.x < nc) part[(long)blockIdx.x * 217 + tap * 8 + threadIdx.x] =
            ((wred[0][threadIdx.x] + wred[1][threadIdx.x]) + wred[2][threadIdx.x]) + wred[3][threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_out_bwd_final(const float* __restrict__ part, int slabs, float* __restrict__ dw, float* __restrict__ db) {
    const int k = threadIdx.x;
    if (k >= 217) return;
    double acc = 0.0;
    for (int sl = 0; sl < slabs; ++sl) acc += (double)part[(long)sl * 217 + k];
    if (k < 216) dw[k] = (float)acc; else db[0] = (float)acc;
}

// ---- loss scaling ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_unscale_check(float* __restrict__ g, long n, float inv, int* __restrict__ flag) {
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = g[i] * inv;
        g[i] = v;
        bad |= !(fabsf(v) <= 3.402823466e38f);  // inf or nan
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);  // (an integer flag: the result has no order)
}

int sum_slabs(long items, long per_slab_min) {
    long s = (items + per_slab_min - 1) / per_slab_min;
    return (int)(s < 1 ? 1 : s > kSumSlabsMax ? kSumSlabsMax : s);
}

bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" long cvx_conv_wgrad_workspace_bytes(int C, int cout, int taps, int dil, int D, int H, int W) {
    long n = 0;
    if (C < 8 || C % 8 || cout < 4 || cout % 4 || (taps != 1 && taps != 27) || dil < 1) return cvx_fail("conv_wgrad_workspace_bytes", "C % 8, cout % 4, taps 1 or 27, dil >= 1");
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("conv_wgrad_workspace_bytes", why);
    WgShape s;
    if (!wg_shape(C, cout, taps, dil, D, H, W, s)) return cvx_fail("conv_wgrad_workspace_bytes", "too many voxel slabs");
    const long colslabs = sum_slabs(n, 1024);
    return (long)sizeof(float) * ((s.slabs > 1 ? (long)s.slabs * cout * s.KT : 0) + colslabs * cout);
}

extern "C" int cvx_conv_wgrad_f16(const void* x, const void* dz, int C, int cout, int taps, int dil, int D, int H, int W, float* dW, float* db,
                                  void* workspace, long workspace_bytes, hipStream_t st) {
    const char* const entry = "conv_wgrad_f16";
    long n = 0;
    if (C < 8 || C % 8 || cout < 4 || cout % 4) return cvx_fail(entry, "C must be a multiple of 8 and cout a multiple of 4");
    if ((taps != 1 && taps != 27) || dil < 1) return cvx_fail(entry, "taps must be 1 or 27 and dil >= 1");
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail(entry, why);
    if (!x || !dz || !dW || !workspace) return cvx_fail(entry, "null pointer");
    if (misaligned16(workspace) || misaligned16(x) || misaligned16(dz)) return cvx_fail(entry, "x, dz and workspace must be 16-B aligned");
    WgShape s;
    if (!wg_shape(C, cout, taps, dil, D, H, W, s)) return cvx_fail(entry, "too many voxel slabs");
    const long need = cvx_conv_wgrad_workspace_bytes(C, cout, taps, dil, D, H, W);
    if (need < 0 || workspace_bytes < need) return cvx_fail(entry, "workspace smaller than cvx_conv_wgrad_workspace_bytes");
    const long nout = (long)cout * s.KT;
    if (n == 0) {
        CVX_HIP(hipMemsetAsync(dW, 0, nout * sizeof(float), st));
        if (db) CVX_HIP(hipMemsetAsync(db, 0, cout * sizeof(float), st));
        return CVX_OK;
    }
    float* part = (float*)workspace;
    float* colpart = part + (s.slabs > 1 ? (long)s.slabs * nout : 0);
    const dim3 grid((unsigned)((long)s.oblocks * s.kblocks), (unsigned)s.slabs);
    float* tiles = s.slabs > 1 ? part : dW;
    switch (wg_otb(cout)) {
        case 1: hipLaunchKernelGGL(k_wgrad<1>, grid, dim3(256), 0, st, (const uint16_t*)x, (const uint16_t*)dz, tiles, s); break;
        case 2: hipLaunchKernelGGL(k_wgrad<2>, grid, dim3(256), 0, st, (const uint16_t*)x, (const uint16_t*)dz, tiles, s); break;
        default: hipLaunchKernelGGL(k_wgrad<4>, grid, dim3(256), 0, st, (const uint16_t*)x, (const uint16_t*)dz, tiles, s); break;
    }
    if (s.slabs > 1) hipLaunchKernelGGL(k_slab_sum, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, part, dW, nout, s.slabs);
    if (db) {
        const int cs = sum_slabs(n, 1024);
        const long rps = (n + cs - 1) / cs;
        hipLaunchKernelGGL(k_colsum_part, dim3(cs, (cout + 63) / 64), dim3(256), 0, st, (const uint16_t*)dz, n, cout, rps, colpart);
        hipLaunchKernelGGL(k_colsum_final, dim3((cout + 255) / 256), dim3(256), 0, st, colpart, cs, cout, db);
    }
    return cvx_check_launch();
}

extern "C" int cvx_gelu_f16(const void* z, void* y, long n, hipStream_t st) {
    const char* const entry = "gelu_f16";
    if (n < 0) return cvx_fail(entry, "n < 0");
    if (n == 0) return CVX_OK;
    if (!z || !y) return cvx_fail(entry, "null pointer");
    if (misaligned16(z) || misaligned16(y)) return cvx_fail(entry, "buffers must be 16-B aligned");
    hipLaunchKernelGGL(k_gelu, dim3(blocks_of((n + 7) / 8)), dim3(256), 0, st, (const uint16_t*)z, (uint16_t*)y, n);
    return cvx_check_launch();
}

extern "C" int cvx_gelu_backward_f16(const void* dy, const void* z, void* dz, long n, int unshuffle, int D, int H, int W, int c3, hipStream_t st) {
    const char* const entry = "gelu_backward_f16";
    if (!dy || !z || !dz) return cvx_fail(entry, "null pointer");
    if (misaligned16(dy) || misaligned16(z) || misaligned16(dz)) return cvx_fail(entry, "buffers must be 16-B aligned");
    if (!unshuffle) {
        if (n < 0) return cvx_fail(entry, "n < 0");
        if (n == 0) return CVX_OK;
        hipLaunchKernelGGL(k_gelu_bwd, dim3(blocks_of((n + 7) / 8)), dim3(256), 0, st, (const uint16_t*)dy, (const uint16_t*)z, (uint16_t*)dz, n);
        return cvx_check_launch();
    }
    long nv = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, nv)) return cvx_fail(entry, why);
    if (c3 < 8 || c3 % 8) return cvx_fail(entry, "c3 must be a multiple of 8");
    if (nv > (LONG_MAX / 4) / c3 || n != nv * 4 * c3) return cvx_fail(entry, "n must be D*H*W*4*c3 (the coarse extents are given)");
    if (nv == 0) return CVX_OK;
    const long threads = nv * 4 * (c3 / 8);
    if ((threads + 255) / 256 > 0x7fffffffL) return cvx_fail(entry, "volume too large");
    hipLaunchKernelGGL(k_gelu_bwd_unshuffle, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const uint16_t*)dy, (const uint16_t*)z,
                       (uint16_t*)dz, nv, H, W, c3);
    return cvx_check_launch();
}

extern "C" long cvx_groupnorm_backward_workspace_floats(int C, int G) {
    if (C < 8 || C % 8 || C > 2048 || G < 1 || G > CVX_GN_MAX_GROUPS || C % G) return cvx_fail("groupnorm_backward_workspace_floats", "C % 8, C <= 2048, C % G");
    return (long)kSumSlabsMax * 2 * C + 2 * G;
}

extern "C" int cvx_groupnorm_backward_f16(const void* x, const void* dn, const float* gamma, const float* stats, void* dx, float* dgamma,
                                          float* dbeta, float* workspace, long workspace_floats, long nvox, int C, int G, float eps, hipStream_t st) {
    const char* const entry = "groupnorm_backward_f16";
    if (C < 8 || C % 8 || C > 2048 || G < 1 || G > CVX_GN_MAX_GROUPS || C % G) return cvx_fail(entry, "C must be a multiple of 8 (<= 2048) and of G (<= 512)");
    if (nvox < 1 || nvox > CVX_COMPONENT_MAX_VOXELS) return cvx_fail(entry, "nvox must be in 1 .. 2^31 - 2");
    if (!x || !dn || !gamma || !stats || !dx || !dgamma || !dbeta || !workspace) return cvx_fail(entry, "null pointer");
    if (misaligned16(x) || misaligned16(dn) || misaligned16(dx)) return cvx_fail(entry, "x, dn and dx must be 16-B aligned");
    if (workspace_floats < cvx_groupnorm_backward_workspace_floats(C, G)) return cvx_fail(entry, "workspace smaller than cvx_groupnorm_backward_workspace_floats");
    const int vstride = 256 / (C >> 3);
    const int slabs = sum_slabs(nvox, (long)vstride * 16);
    const long vpb = (nvox + slabs - 1) / slabs;
    float* gm = workspace + (long)kSumSlabsMax * 2 * C;
    hipLaunchKernelGGL(k_gnb_part, dim3(slabs), dim3(256), 0, st, (const uint16_t*)x, (const uint16_t*)dn, stats, workspace, nvox, C, G, eps, vpb);
    hipLaunchKernelGGL(k_gnb_final, dim3(G), dim3(64), 0, st, workspace, slabs, gamma, dgamma, dbeta, gm, nvox, C, G);
    const long ablocks = (nvox + (long)vstride * 16 - 1) / ((long)vstride * 16);
    const long nb = ablocks > 65536 ? 65536 : ablocks;
    hipLaunchKernelGGL(k_gnb_apply, dim3((unsigned)nb), dim3(256), 0, st, (const uint16_t*)x, (const uint16_t*)dn, gamma, stats, gm, (uint16_t*)dx,
                       nvox, C, G, eps, (nvox + nb - 1) / nb);
    return cvx_check_launch();
}

extern "C" long cvx_conv3_out_backward_workspace_floats(void) { return (long)kSumSlabsMax * 217; }

extern "C" int cvx_conv3_out_backward(const float* dlogit, const void* y_mid, const float* w, void* dy_mid, float* dW, float* db, float* workspace,
                                      long workspace_floats, int D, int H, int W, hipStream_t st) {
    const char* const entry = "conv3_out_backward";
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail(entry, why);
    if (n == 0) return cvx_fail(entry, "empty volume");
    if (!dlogit || !y_mid || !w || !dy_mid || !dW || !db || !workspace) return cvx_fail(entry, "null pointer");
    if (misaligned16(y_mid) || misaligned16(dy_mid)) return cvx_fail(entry, "y_mid and dy_mid must be 16-B aligned");
    if (workspace_floats < cvx_conv3_out_backward_workspace_floats()) return cvx_fail(entry, "workspace smaller than cvx_conv3_out_backward_workspace_floats");
    hipLaunchKernelGGL(k_out_bwd_data, dim3(blocks_of(n)), dim3(256), 0, st, dlogit, w, (uint16_t*)dy_mid, D, H, W);
    const int slabs = sum_slabs(n, 2048);
    hipLaunchKernelGGL(k_out_bwd_weight, dim3(slabs), dim3(256), 0, st, dlogit, (const uint16_t*)y_mid, workspace, D, H, W, (n + slabs - 1) / slabs);
    hipLaunchKernelGGL(k_out_bwd_final, dim3(1), dim3(256), 0, st, workspace, slabs, dW, db);
    return cvx_check_launch();
}

extern "C" int cvx_unscale_check_f32(float* g, long n, float inv_scale, int* flag, hipStream_t st) {
    const char* const entry = "unscale_check_f32";
    if (n < 0) return cvx_fail(entry, "n < 0");
    if (!flag || (n > 0 && !g)) return cvx_fail(entry, "null pointer");
    CVX_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (n == 0) return CVX_OK;
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_unscale_check, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, g, n, inv_scale, flag);
    return cvx_check_launch();
}
