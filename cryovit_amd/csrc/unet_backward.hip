// Backward of the UNet3D baseline: the arithmetic UNet3D has and the CryoVIT head (head_backward.hip) does not.
//   cvx_instnorm_gelu_backward_f16  InstanceNorm (GroupNorm with G = C) + GELU backward in two passes over dy and z: dz, dgamma, dbeta
//   cvx_space_to_depth_f16          [D][H][W][C] -> [D/2 * H/2 * W/2][8C], column ((iz*2 + iy)*2 + ix)*C + c
//   cvx_pointwise_out_backward      the 1x1x1 output layer: dy, dW, db from the fp32 logit gradient
//   cvx_concat_backward_f16         splits the gradient of torch.cat: d_up = dcat[:, :C_up], d_skip = dcat[:, C_up:] + d_pool
// The weight gradients (cvx_conv_wgrad_f16) and the data gradients (cvx_conv3d_f16, cvx_gemm_bf16 on repacked weights) are the
// head's.  No floating-point atomics: every reduction is block partials in a workspace followed by a fixed-order finalize, and the
// number of slabs is a function of the shape alone, so results are bit-reproducible.
#include "common.h"
#include "../../include/cryovit_hip.h"
#include "entry_checks.h"

using namespace cvx;

namespace {

constexpr int kSlabsMax = 1024;  // of the norm and output-layer reductions

int sum_slabs(long items, long per_slab_min) {
    long s = (items + per_slab_min - 1) / per_slab_min;
    return (int)(s < 1 ? 1 : s > kSlabsMax ? kSlabsMax : s);
}

bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

__device__ __forceinline__ float gelu_grad(float n) {  // Phi(n) + n phi(n), exact-erf GELU; erfc keeps both tails accurate
    const float cdf = 0.5f * erfcf(-n * 0.70710678118654752440f);
    const float pdf = 0.39894228040143267794f * expf(-0.5f * n * n);
    return fmaf(n, pdf, cdf);
}

__device__ __forceinline__ void unpack8(const uint4& u, float* f) {
    f[0] = hlo(u.x); f[1] = hhi(u.x); f[2] = hlo(u.y); f[3] = hhi(u.y);
    f[4] = hlo(u.z); f[5] = hhi(u.z); f[6] = hlo(u.w); f[7] = hhi(u.w);
}

__device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 o;
    o.x = pack2h(f[0], f[1]); o.y = pack2h(f[2], f[3]); o.z = pack2h(f[4], f[5]); o.w = pack2h(f[6], f[7]);
    return o;
}

// ---- InstanceNorm + GELU backward ------------------------------------------------------------------------------------------------

// mean, rstd, gamma, beta of the 8 channels a thread owns, from the forward's published fp32 sums with its fp64 arithmetic (norm.hip)
struct In8 {
    float mean[8], rstd[8], gw[8], gb[8];
};

__device__ __forceinline__ void in_moments8(const float* stats, const float* gamma, const float* beta, int c0, int C, long nvox, float eps,
                                            In8& m) {
    const double cnt = (double)nvox;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double mu = (double)stats[c0 + e] / cnt;
        double var = (double)stats[C + c0 + e] / cnt - mu * mu;
        var = var < 0.0 ? 0.0 : var;
        m.mean[e] = (float)mu;
        m.rstd[e] = (float)(1.0 / sqrt(var + (double)eps));
        m.gw[e] = gamma[c0 + e];
        m.gb[e] = beta[c0 + e];
    }
}

// pass 1.  Per slab and channel: sum dn | sum dn xhat with dn = dy GELU'(gamma xhat + beta).  The thread layout is k_gn_stats': thread
// (cidx, vsub) owns the 16-B piece cidx of the voxels vsub, vsub + vstride, ..; lane-private sums -> LDS -> summed in thread order.
__global__ __launch_bounds__(256) void k_ingb_part(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ z, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ stats, float* __restrict__ part,
                                                   long nvox, int C, float eps, long vox_per_block) {
    __shared__ float red[256][17];
    const int tid = threadIdx.x;
    const int cpt = C >> 3;
    const int cidx = tid % cpt, vstride = 256 / cpt;
    const int vsub = tid / cpt < vstride ? tid / cpt : -1;
    In8 m;
    in_moments8(stats, gamma, beta, cidx * 8, C, nvox, eps, m);
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
    const long v0 = (long)blockIdx.x * vox_per_block, v1 = min(nvox, v0 + vox_per_block);
    for (long v = vsub < 0 ? v1 : v0 + vsub; v < v1; v += vstride) {
        float fz[8], fd[8];
        unpack8(*(const uint4*)(z + v * C + cidx * 8), fz);
        unpack8(*(const uint4*)(dy + v * C + cidx * 8), fd);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (fz[e] - m.mean[e]) * m.rstd[e];
            const float dn = fd[e] * gelu_grad(fmaf(m.gw[e], xh, m.gb[e]));
            s[e] += dn;
            q[e] += dn * xh;
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

// one wave per channel: the slabs in lane order, then a fixed xor tree, all in fp64 (the arithmetic of k_gnb_final with one channel per
// group): dbeta, dgamma and the means m1 = mean(gamma dn), m2 = mean(gamma dn xhat) -> cm[c], cm[C + c]
__global__ __launch_bounds__(256) void k_ingb_final(const float* __restrict__ part, int slabs, const float* __restrict__ gamma,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ cm, long nvox, int C) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;  // (a whole wave)
    double sb = 0.0, sg = 0.0;
    for (int sl = lane; sl < slabs; sl += 64) {
        sb += (double)part[(long)sl * 2 * C + c];
        sg += (double)part[(long)sl * 2 * C + C + c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sb += __shfl_xor(sb, o, 64); sg += __shfl_xor(sg, o, 64); }
    if (lane == 0) {
        dbeta[c] = (float)sb;
        dgamma[c] = (float)sg;
        cm[c] = (float)((double)gamma[c] * sb / (double)nvox);
        cm[C + c] = (float)((double)gamma[c] * sg / (double)nvox);
    }
}

// pass 2.  dz = rstd (gamma dn - m1 - xhat m2) with dn recomputed from dy and z: fp32 math, one fp16 rounding
__global__ __launch_bounds__(256) void k_ingb_apply(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ z, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ stats, const float* __restrict__ cm,
                                                    uint16_t* __restrict__ dz, long nvox, int C, float eps, long vox_per_block) {
    const int tid = threadIdx.x;
    const int cpt = C >> 3;
    const int cidx = tid % cpt, vsub = tid / cpt, vstride = 256 / cpt;
    if (vsub >= vstride) return;
    In8 m;
    in_moments8(stats, gamma, beta, cidx * 8, C, nvox, eps, m);
    float m1[8], m2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { m1[e] = cm[cidx * 8 + e]; m2[e] = cm[C + cidx * 8 + e]; }
    const long v0 = (long)blockIdx.x * vox_per_block, v1 = min(nvox, v0 + vox_per_block);
    for (long v = v0 + vsub; v < v1; v += vstride) {
        float fz[8], fd[8], o[8];
        unpack8(*(const uint4*)(z + v * C + cidx * 8), fz);
        unpack8(*(const uint4*)(dy + v * C + cidx * 8), fd);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (fz[e] - m.mean[e]) * m.rstd[e];
            const float dn = fd[e] * gelu_grad(fmaf(m.gw[e], xh, m.gb[e]));
            o[e] = m.rstd[e] * (m.gw[e] * dn - m1[e] - xh * m2[e]);
        }
        *(uint4*)(dz + v * C + cidx * 8) = pack8(o);
    }
}

// ---- space to depth ----------------------------------------------------------------------------------------------------------------

// one thread per 16-B piece of the output: consecutive threads write consecutive pieces of a row and read runs of 2C halfs (the two
// ix of one (iz, iy)).  D, H, W: the COARSE extents
__global__ __launch_bounds__(256) void k_space_to_depth(const uint16_t* __restrict__ x, uint16_t* __restrict__ out, long pieces, int H, int W, int C) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pieces) return;
    const int c8 = C >> 3;
    const int oc = (int)(t % c8), k = (int)((t / c8) % 8);
    const long v = t / (8 * c8);
    const int xx = (int)(v % W), yy = (int)((v / W) % H);
    const long zz = v / ((long)W * H);
    const long src = ((zz * 2 + (k >> 2)) * 2 * H + 2 * yy + ((k >> 1) & 1)) * 2 * W + 2 * xx + (k & 1);
    *(uint4*)(out + t * 8) = *(const uint4*)(x + src * C + oc * 8);
}

// ---- the output layer (C -> 1, 1x1x1, fp32 weights) -------------------------------------------------------------------------------

// dy[v][c] = dlogit[v] w[c] and, in the same pass over y, part[slab][c] = sum_v dlogit[v] y[v][c], part[slab][C] = sum_v dlogit[v]
// (thread layout of k_ingb_part; the threads of piece 0 carry the dlogit sum)
__global__ __launch_bounds__(256) void k_pw_out_bwd(const float* __restrict__ dlogit, const uint16_t* __restrict__ y, const float* __restrict__ w,
                                                    uint16_t* __restrict__ dy, float* __restrict__ part, long nvox, int C, long vox_per_block) {
    __shared__ float red[256][9];
    const int tid = threadIdx.x;
    const int cpt = C >> 3;  // 1, 2, 4 or 8: divides 256
    const int cidx = tid % cpt, vsub = tid / cpt, vstride = 256 / cpt;
    float wv[8], acc[8], sd = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { wv[e] = w[cidx * 8 + e]; acc[e] = 0.f; }
    const long v0 = (long)blockIdx.x * vox_per_block, v1 = min(nvox, v0 + vox_per_block);
    for (long v = v0 + vsub; v < v1; v += vstride) {
        const float gl = dlogit[v];
        float fy[8], o[8];
        unpack8(*(const uint4*)(y + v * C + cidx * 8), fy);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[e] = fmaf(gl, fy[e], acc[e]);
            o[e] = gl * wv[e];
        }
        sd += gl;
        *(uint4*)(dy + v * C + cidx * 8) = pack8(o);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid][e] = acc[e];
    red[tid][8] = sd;
    __syncthreads();
    for (int k = tid; k <= C; k += 256) {
        const int piece = k < C ? k >> 3 : 0, col = k < C ? (k & 7) : 8;
        float a = 0.f;
        for (int vs = 0; vs < vstride; ++vs) a += red[vs * cpt + piece][col];
        part[(long)blockIdx.x * (C + 1) + k] = a;
    }
}

__global__ __launch_bounds__(128) void k_pw_out_final(const float* __restrict__ part, int slabs, int C, float* __restrict__ dw, float* __restrict__ db) {
    const int k = threadIdx.x;
    if (k > C) return;
    double acc = 0.0;
    for (int sl = 0; sl < slabs; ++sl) acc += (double)part[(long)sl * (C + 1) + k];
    if (k < C) dw[k] = (float)acc; else db[0] = (float)acc;
}

// ---- concat backward ---------------------------------------------------------------------------------------------------------------

// one thread per 16-B piece of a dcat row: the first cup columns are copied, the others added to d_pool in fp32 and rounded once.
// dup or dskip may be null: the backward needs the up half at once and the skip half only when d_pool exists
__global__ __launch_bounds__(256) void k_concat_bwd(const uint16_t* __restrict__ dcat, const uint16_t* __restrict__ dpool, uint16_t* __restrict__ dup,
                                                    uint16_t* __restrict__ dskip, long pieces, int cup, int cskip) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pieces) return;
    const int p8 = (cup + cskip) >> 3, u8 = cup >> 3;
    const long v = t / p8;
    const int pc = (int)(t % p8);
    if (pc < u8 ? !dup : !dskip) return;  // (this half is not asked for: its piece is not even read)
    const uint4 u = *(const uint4*)(dcat + t * 8);
    if (pc < u8) {
        *(uint4*)(dup + v * cup + pc * 8) = u;
        return;
    }
    const long o = v * cskip + (long)(pc - u8) * 8;
    float a[8], b[8];
    unpack8(u, a);
    unpack8(*(const uint4*)(dpool + o), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += b[e];
    *(uint4*)(dskip + o) = pack8(a);
}

bool norm_shape_ok(int C) { return C >= 8 && C % 8 == 0 && C <= CVX_GN_MAX_GROUPS; }
bool out_channels_ok(int C) { return C == 8 || C == 16 || C == 32 || C == 64; }

}  // namespace

extern "C" long cvx_instnorm_gelu_backward_workspace_floats(int C) {
    if (!norm_shape_ok(C)) return cvx_fail("instnorm_gelu_backward_workspace_floats", "C must be a multiple of 8, at most CVX_GN_MAX_GROUPS");
    return (long)kSlabsMax * 2 * C + 2 * C;
}

extern "C" int cvx_instnorm_gelu_backward_f16(const void* dy, const void* z, const float* gamma, const float* beta, const float* stats, void* dz,
                                              float* dgamma, float* dbeta, float* workspace, long workspace_floats, long nvox, int C, float eps,
                                              hipStream_t st) {
    const char* const entry = "instnorm_gelu_backward_f16";
    if (!norm_shape_ok(C)) return cvx_fail(entry, "C must be a multiple of 8, at most CVX_GN_MAX_GROUPS");
    if (nvox < 2 || nvox > CVX_COMPONENT_MAX_VOXELS) return cvx_fail(entry, "nvox must be in 2 .. 2^31 - 2");
    if (!dy || !z || !gamma || !beta || !stats || !dz || !dgamma || !dbeta || !workspace) return cvx_fail(entry, "null pointer");
    if (misaligned16(dy) || misaligned16(z) || misaligned16(dz)) return cvx_fail(entry, "dy, z and dz must be 16-B aligned");
    if (workspace_floats < cvx_instnorm_gelu_backward_workspace_floats(C)) return cvx_fail(entry, "workspace smaller than cvx_instnorm_gelu_backward_workspace_floats");
    const int vstride = 256 / (C >> 3);
    const int slabs = sum_slabs(nvox, (long)vstride * 4);
    const long vpb = (nvox + slabs - 1) / slabs;
    float* cm = workspace + (long)kSlabsMax * 2 * C;
    hipLaunchKernelGGL(k_ingb_part, dim3(slabs), dim3(256), 0, st, (const uint16_t*)dy, (const uint16_t*)z, gamma, beta, stats, workspace, nvox, C,
                       eps, vpb);
    hipLaunchKernelGGL(k_ingb_final, dim3((C + 3) / 4), dim3(256), 0, st, workspace, slabs, gamma, dgamma, dbeta, cm, nvox, C);
    const long ablocks = (nvox + (long)vstride * 4 - 1) / ((long)vstride * 4);
    const long nb = ablocks > 65536 ? 65536 : ablocks;
    hipLaunchKernelGGL(k_ingb_apply, dim3((unsigned)nb), dim3(256), 0, st, (const uint16_t*)dy, (const uint16_t*)z, gamma, beta, stats, cm,
                       (uint16_t*)dz, nvox, C, eps, (nvox + nb - 1) / nb);
    return cvx_check_launch();
}

extern "C" int cvx_space_to_depth_f16(const void* x, void* out, int D, int H, int W, int C, hipStream_t st) {
    const char* const entry = "space_to_depth_f16";
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail(entry, why);
    if ((D | H | W) & 1) return cvx_fail(entry, "D, H and W must be even");
    if (C < 8 || C % 8) return cvx_fail(entry, "C must be a multiple of 8");
    if (n > LONG_MAX / C) return cvx_fail(entry, "volume too large");
    if (n == 0) return CVX_OK;
    if (!x || !out) return cvx_fail(entry, "null pointer");
    if (misaligned16(x) || misaligned16(out)) return cvx_fail(entry, "buffers must be 16-B aligned");
    const long pieces = n * (C / 8);
    if ((pieces + 255) / 256 > 0x7fffffffL) return cvx_fail(entry, "volume too large");
    hipLaunchKernelGGL(k_space_to_depth, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, (const uint16_t*)x, (uint16_t*)out, pieces, H / 2,
                       W / 2, C);
    return cvx_check_launch();
}

extern "C" long cvx_pointwise_out_backward_workspace_floats(int C) {
    if (!out_channels_ok(C)) return cvx_fail("pointwise_out_backward_workspace_floats", "C must be 8, 16, 32 or 64");
    return (long)kSlabsMax * (C + 1);
}

extern "C" int cvx_pointwise_out_backward(const float* dlogit, const void* y, const float* w, void* dy, float* dW, float* db, float* workspace,
                                          long workspace_floats, long nvox, int C, hipStream_t st) {
    const char* const entry = "pointwise_out_backward";
    if (!out_channels_ok(C)) return cvx_fail(entry, "C must be 8, 16, 32 or 64");
    if (nvox < 1 || nvox > CVX_COMPONENT_MAX_VOXELS) return cvx_fail(entry, "nvox must be in 1 .. 2^31 - 2");
    if (!dlogit || !y || !w || !dy || !dW || !db || !workspace) return cvx_fail(entry, "null pointer");
    if (misaligned16(y) || misaligned16(dy)) return cvx_fail(entry, "y and dy must be 16-B aligned");
    if (workspace_floats < cvx_pointwise_out_backward_workspace_floats(C)) return cvx_fail(entry, "workspace smaller than cvx_pointwise_out_backward_workspace_floats");
    const int vstride = 256 / (C >> 3);
    const int slabs = sum_slabs(nvox, (long)vstride * 4);
    hipLaunchKernelGGL(k_pw_out_bwd, dim3(slabs), dim3(256), 0, st, dlogit, (const uint16_t*)y, w, (uint16_t*)dy, workspace, nvox, C,
                       (nvox + slabs - 1) / slabs);
    hipLaunchKernelGGL(k_pw_out_final, dim3(1), dim3(128), 0, st, workspace, slabs, C, dW, db);
    return cvx_check_launch();
}

extern "C" int cvx_concat_backward_f16(const void* dcat, const void* d_pool, void* d_up, void* d_skip, long nvox, int c_up, int c_skip, hipStream_t st) {
    const char* const entry = "concat_backward_f16";
    if (c_up < 8 || c_up % 8 || c_skip < 8 || c_skip % 8 || c_up > 4096 || c_skip > 4096) return cvx_fail(entry, "c_up and c_skip must be multiples of 8, at most 4096");
    if (nvox < 0 || nvox > CVX_COMPONENT_MAX_VOXELS) return cvx_fail(entry, "nvox must be in 0 .. 2^31 - 2");
    if (nvox == 0) return CVX_OK;
    if (!dcat || (!d_up && !d_skip) || (d_skip && !d_pool)) return cvx_fail(entry, "null pointer");
    if (misaligned16(dcat) || misaligned16(d_pool) || misaligned16(d_up) || misaligned16(d_skip)) return cvx_fail(entry, "buffers must be 16-B aligned");
    const long pieces = nvox * ((c_up + c_skip) / 8);
    if ((pieces + 255) / 256 > 0x7fffffffL) return cvx_fail(entry, "volume too large");
    hipLaunchKernelGGL(k_concat_bwd, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, (const uint16_t*)dcat, (const uint16_t*)d_pool,
                       (uint16_t*)d_up, (uint16_t*)d_skip, pieces, c_up, c_skip);
    return cvx_check_launch();
}
