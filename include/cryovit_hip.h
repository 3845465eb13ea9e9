/* cryovit_hip.h -- C ABI of libcryovit_hip.so (gfx950 / MI355X).
 *
 * The reference (VivianDLi/CryoVIT) is pure Python and has NO FFI boundary of its own: its plug-in
 * surface is Hydra `_target_` instantiation plus two duck-typed Python protocols.  This
 * header is therefore the boundary a maintainer would bind with ctypes to replace the third-party
 * arithmetic the reference delegates to torch / xformers / the dinov2 hub model:
 *
 *   cvx_preprocess_patches + cvx_vit_encode
 *                     replace   model.forward_features(vec)["x_norm_patchtokens"] + reshape/permute/half
 *                               src/cryovit/run/dino_features.py:53-61  and the CPU bicubic resize of
 *                               src/cryovit/datasets/vit_dataset.py:117-123 (fused into the first kernel)
 *   cvx_head_forward (= cvx_gemm_bf16 with fp16 operands, cvx_groupnorm_f16, cvx_conv3d_f16, cvx_conv3_out_fused)
 *                     replaces  CryoVIT.forward_volume + sigmoid          src/cryovit/models/cryovit.py:36-49
 *                               and the masked Dice reductions            src/cryovit/models/base_model.py:99-110,
 *                                                                         src/cryovit/models/metrics.py:30-43
 *
 * Conventions: every function returns 0 on success and a negative code on failure
 * (cvx_last_error() gives the message, thread-local); all pointers named *_dev / in descriptors are DEVICE
 * pointers owned by the caller; nothing allocates, frees or synchronises inside a call (graph-capturable);
 * every launch goes to the caller's hipStream_t.  One handle per stream / GPU; handles are not thread-safe.
 * The op-level entry points (cvx_gemm_bf16 ... cvx_dice_sums) are the kernels the two high-level calls are
 * built from; they are exported so the parity tests can check each kernel against the CPU oracle.
 */
#ifndef CRYOVIT_HIP_H
#define CRYOVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t; /* same as <hip/hip_runtime_api.h> */

#define CVX_OK 0
#define CVX_ERR_ARG (-1)
#define CVX_ERR_HIP (-2)

const char* cvx_last_error(void);
int cvx_version(void);
/* name of the device the library would launch on ("gfx950...") or "" when no HIP device is visible */
int cvx_device_arch(char* buf, int buflen);
/* Process-global tuning switches for in-process A/B measurements (tools/, tests): every default is the shipped, measured-best setting and
 * no product path sets one.  Returns non-zero (cvx_last_error) for an unknown name or a value the library was not built with (the product
 * library holds the shipped kernel variants only; the rejected ones live in the -DCVX_ABLATION build).  Names: use_gemm256, gemm256_variant,
 * gemm_stagger, gemm_tail_split, tile_group_l,
 * attn_variant, attn_xcd_remap, attn_mfma_prio, attn_half_tile, win_attn_prefetch, win_attn_x32, conv_halo, conv_wide, convt_small
 * -- each is described where it is defined (csrc/gemm.hip, attention.hip, hiera.hip) and in DESIGN.md s.4 / s.8. */
int cvx_set_option(const char* name, int value);
/* diagnostic: per-wave cycle sums {load, load-barrier, mma, mma-barrier} x 8 waves written by the per-phase stamped build of the
 * one-shot 256-tile (gemm256_variant 20; 21, the coarse stamps, writes {prologue, K loop, epilogue, total} there) */
int cvx_debug_read_gemm256(unsigned long long* out32);
/* diagnostic: cycle stamps of the persistent tile kernel (variant 29, -DCVX_ABLATION builds only; zeros otherwise):
 * [wave group 2][tile 8][6] = K-loop start, K-loop end, epilogue start, epilogue end, next tile released, first K tile done */
int cvx_debug_read_gemm256p(unsigned long long* out96);

/* ---------------------------------------------------------------------------------------------------
 * Dense GEMM  C[M,N] = A[M,K] * W[N,K]^T, bf16 operands (K contiguous, leading dims in elements),
 * fp32 accumulation on v_mfma_f32_16x16x32_bf16, fused epilogue.  A must be allocated (not necessarily
 * valid) up to a multiple of 256 rows; W / bias / gamma are packed to n_pad (multiple of 16; 128 for
 * SWIGLU / VT) rows and k_pad (multiple of 64) columns.  Replaces torch.nn.Linear / Conv2d(14,14) /
 * Conv3d(k=1) / ConvTranspose3d calls made by the hub ViT and by cryovit/models/cryovit.py:18-34,74-77.
 * ------------------------------------------------------------------------------------------------- */
enum cvx_epilogue {
    CVX_EPI_BF16 = 0,      /* out bf16 [M][ldc]       = acc + bias                                   */
    CVX_EPI_BF16_GELU = 1, /* out bf16 [M][ldc]       = gelu_erf(acc + bias)                         */
    CVX_EPI_SWIGLU = 2,    /* out bf16 [M][ldc], N/2 cols = silu(a) * b   (W rows interleaved by 8)  */
    CVX_EPI_RESID = 3,     /* out fp32 [M][ldc]      += gamma * (acc + bias)     (LayerScale+residual)*/
    CVX_EPI_PATCH = 4,     /* out fp32 token stream: row slice*ntp+tok0+p = acc + bias + pos[1+p]     */
    CVX_EPI_VT = 5,        /* out bf16 V^T [slice][head][64][kp] = acc + bias   (for cvx_attention)   */
    CVX_EPI_CONVT = 6,     /* out bf16 [D][2H][2W][cout] pixel-shuffle of N = 4*cout, optional GELU   */
    CVX_EPI_F32 = 7,       /* out fp32 [M][ldc]       = gamma * (acc + bias)   (written, not accumulated)  */
    CVX_EPI_RESID_HL = 8   /* the residual stream as a bf16 PAIR: x = hi + lo (out = hi, out2 = lo, both bf16 [M][ldc]);
                              x += gamma * (acc + bias); hi = bf16(x), lo = bf16(x - hi); stat_part[n / 64][m] = (sum, sum of
                              squares) of the new x over 64-column slots (N a multiple of 64, N <= n_pad).  hi is the next GEMM's A
                              operand: see ln_rowstat                                                            */
};

enum { CVX_DTYPE_BF16 = 0, CVX_DTYPE_F16 = 1 };

typedef struct cvx_gemm_desc {
    int epilogue;
    const void* a; long lda;   /* bf16 [M_alloc][lda]  */
    const void* w; long ldw;   /* bf16 [n_pad][ldw]    */
    long m, n, n_pad, k_pad;   /* valid rows / cols; padded N, K */
    void* out; long ldc;
    const float* bias;         /* [n_pad] */
    const float* gamma;        /* RESID: [n_pad] */
    const float* pos; long ldpos; /* PATCH: fp32 [1+npatch][ldpos] */
    int npatch, ntp, tok0;     /* PATCH: patches per slice, padded tokens per slice, first patch token */
    int heads, kp;             /* VT: heads, padded key count (multiple of 64) */
    int H, W, cout, act;       /* CONVT: input plane size, C_out, act (0 none / 1 GELU) */
    int dtype;                 /* CVX_DTYPE_BF16 (0, default): bf16 operands / 16-bit outputs; CVX_DTYPE_F16: fp16 operands
                                  and outputs (BF16, BF16_GELU and CONVT epilogues only: the segmentation head) */
    int convt_up_z;            /* CONVT: 0 = kernel/stride (1,2,2), N = 4*C_out (the head); 1 = (2,2,2), N = 8*C_out with
                                  n = ((iz*2+i)*2+j)*C_out + o, output [2D][2H][2W][C_out] (UNet3D upconv, unet3d.py:166-170) */
    /* LayerNorm folded into the GEMM (BF16, BF16_GELU, SWIGLU, VT; bf16 operands): A = bf16(x) un-normalised (the hi array), W
     * packed as bf16(W * ln_gamma), bias = fp32 [2][n_pad]: b' = b + W ln_beta, then cs[n] = sum_k W'[n][k];
     * ln_rowstat = fp32 [M][2] = (rstd, -mean * rstd) per row (cvx_rowstat_finalize / cvx_split_stream).  The epilogue then
     * starts from  rstd * acc + (-mean * rstd) * cs[n] + b'[n]  instead of acc + bias[n].  NULL: plain epilogue.  Non-NULL with
     * fp16 operands or another epilogue: the call fails. */
    const float* ln_rowstat;
    /* RESID_HL: lo array, fp32 partial row sums [n / 64][stat_rows][2], stat_rows >= M rounded up to 256.  Slots < n / 64 of rows
     * < M are written and nothing else: no slot of a padded column (n .. n_pad), no row >= M */
    void* out2; float* stat_part; long stat_rows;
} cvx_gemm_desc;

int cvx_gemm_bf16(const cvx_gemm_desc* d, hipStream_t stream);

/* Measurement hook: while set, every cvx_gemm_bf16 launch with this epilogue (also inside cvx_vit_encode) is bracketed by
 * hipEventRecord(start[i]) / hipEventRecord(stop[i]) on the launch stream, i = 0 .. capacity-1.  NULL arrays disable it. */
int cvx_set_gemm_event_hook(int epilogue, void** start_events, void** stop_events, int capacity);
int cvx_get_gemm_event_count(void);

/* Dilated 3x3x3 "same" convolution, dilation (dil,1,1), channels-last FP16 volume in[D][H][W][C] ->
 * out[D][H][W][cout] fp16 = act(conv + bias), as an implicit GEMM (K = tap*C + c) on v_mfma_f32_16x16x32_f16 (the head
 * stores fp16: the reference runs it under fp16 autocast, and fp16 storage keeps the logits within 1e-2 of the fp32 CPU
 * path where bf16 storage costs 0.2 -- DESIGN.md s.2).  w is fp16 [n_pad][k_pad] with
 * k = ((kz*3+ky)*3+kx)*C + c.  zero_page: >= 16 zero bytes on the device (source of padded taps).
 * Replaces nn.Conv3d(c1,c2,3,padding="same",dilation=(d,1,1)) -- cryovit/models/cryovit.py:70-73,30-33. */
typedef struct cvx_conv3d_desc {
    const void* in; const void* w; const float* bias; const void* zero_page; void* out;
    int C, D, H, W, dil, cout, n_pad, k_pad, act;
} cvx_conv3d_desc;
int cvx_conv3d_f16(const cvx_conv3d_desc* d, hipStream_t stream);

/* nn.Conv3d(C, cout, 2, stride=2) (UNet3D's pooling convolution, models/unet3d.py:127-131) on the same descriptor: in fp16
 * [D][H][W][C] (D, H, W even, C a power of two >= 8) -> out fp16 [D/2][H/2][W/2][cout] = act(conv + bias); w fp16 [n_pad][8*C]
 * with k = ((iz*2+iy)*2+ix)*C + c; dil is ignored. */
int cvx_conv2s2_f16(const cvx_conv3d_desc* d, hipStream_t stream);

/* UNet3D helpers (csrc/unet.hip).  cvx_concat_channels_f16: out[v][0..Ca) = a[v][:], out[v][Ca..Ca+Cb) = b[v][:] (torch.cat along
 * channels, unet3d.py:64; Ca, Cb multiples of 8).  cvx_pointwise_out_f16: the 1x1x1 output layer + clip + sigmoid
 * (unet3d.py:45,69-71,96): logits / probs fp32 [nvox] (either nullable) from in fp16 [nvox][C], w fp32 [C], C <= 64, a multiple of 8. */
int cvx_concat_channels_f16(const void* a, int Ca, const void* b, int Cb, void* out, long nvox, hipStream_t stream);
int cvx_pointwise_out_f16(const void* in, const float* w, float bias, float* logits, float* probs, long nvox, int C, hipStream_t stream);

/* LayerNorm over the last dim of an fp32 token stream -> bf16 (GEMM operand).  eps inside the sqrt.
 * x fp32 [rows][ldx], out bf16 [rows][ldo].  Replaces nn.LayerNorm(C, eps=1e-6) in the hub ViT blocks. */
int cvx_layernorm_bf16(const float* x, long ldx, const float* w, const float* b, void* out, long ldo, long rows,
                       int C, float eps, hipStream_t stream);

/* Multi-head attention, head_dim 64, no mask/dropout:  O = softmax(Q K^T) V  per (slice, head).
 *   qk   bf16 [slices*ntp (+64 rows slack)][ldqk] : columns [0,C) = Q pre-scaled by head_dim^-0.5 * log2(e)
 *                                                  (scores in log2 units: the kernel uses exp2),
 *                                                  [C,2C) = K, head h at columns h*64..h*64+63
 *   vt   bf16 [slices][heads][64][kp]  (kp = ntok rounded up to 64; columns >= ntok must be finite)
 *   out  bf16 [slices*ntp][ldo], head h at columns h*64...
 * ntok = valid tokens per slice (keys >= ntok are masked), ntp = padded tokens per slice (multiple of 8).
 * Replaces xformers.memory_efficient_attention inside the hub model (run/dino_features.py:58). */
int cvx_attention_bf16(const void* qk, long ldqk, const void* vt, void* out, long ldo, int slices, int heads,
                       int ntok, int ntp, int kp, hipStream_t stream);

/* The same attention reading V ROW-MAJOR from the buffer that holds Q and K: qkv bf16 [slices*ntp (+64 rows slack)][ld], columns
 * [0,C) = Q (log2 units), [C,2C) = K, [2C,3C) = V, C = heads*64 -- the output of ONE qkv GEMM with the plain row-major epilogue
 * (no V^T GEMM launch, no vt buffer).  ld % 64 == 0.  The kernel transposes V fragments on the LDS read (ds_read_b64_tr_b16). */
int cvx_attention_qkv_bf16(const void* qkv, long ld, void* out, long ldo, int slices, int heads, int ntok, int ntp,
                           hipStream_t stream);

/* Pre-processing fused with im2col: raw slices [b][H][W] (u8 -> /255, or f32), edge-pad to x16, bicubic
 * x14/16 (A = -0.75, align_corners = False, clamped taps), cut into 14x14 patches of ONE channel (the 3
 * input channels are identical copies -- vit_dataset.py:117-118 -- so the patch-embed weight is summed over
 * channels at pack time): out bf16 [b*hp*wp][k_pad], k = py*14+px, zero padded to k_pad.
 * Replaces VITDataset._dino_transform (vit_dataset.py:90-123) + the unfold inside Conv2d(3,C,14,14). */
int cvx_preprocess_patches(const void* slices, int is_u8, int b, int H, int W, void* out, int k_pad,
                           hipStream_t stream);

/* cls / register / padding rows of the token stream: x[s*ntp + 0] = cls + pos[0]; rows 1..n_reg = registers;
 * rows ntok..ntp-1 = 0.  (patch rows are written by CVX_EPI_PATCH.) */
int cvx_init_tokens(float* x, long ldx, const float* cls_pos0, const float* reg, int n_reg, int slices, int ntok,
                    int ntp, int C, hipStream_t stream);

/* Final LayerNorm + drop cls/registers + layout transform (run/dino_features.py:58-61):
 *   feats_f16  (nullable) fp16 [C][d_total][hp][wp], slices written at depth d0..d0+slices-1
 *   feats_cl   (nullable) fp16 [slices][hp][wp][C]   channels-last copy for the segmentation head (same rounding as feats_f16)
 *   tokens_f32 (nullable) fp32 [slices][hp*wp][C]    "x_norm_patchtokens" of the encoder protocol */
int cvx_final_norm_features(const float* x, long ldx, const float* w, const float* b, float eps, int slices,
                            int ntp, int tok0, int hp, int wp, int C, void* feats_f16, long d_total, long d0,
                            void* feats_cl, float* tokens_f32, hipStream_t stream);

/* The ViT path keeps its residual stream as a PAIR of bf16 arrays, x = hi + lo (hi = bf16(x) doubles as the A operand of the
 * next GEMM, which applies the LayerNorm in its epilogue: cvx_gemm_desc.ln_rowstat; lo = bf16(x - hi)).
 * cvx_final_norm_features_hl: cvx_final_norm_features reading that pair (ld in elements of either array).
 * cvx_split_stream: fp32 rows -> (hi, lo) and rowstat[row] = (rstd, -mean * rstd) of nn.LayerNorm(C, eps) over the row: the
 *   hand-over from the patch-embedding GEMM (fp32) to the first block.
 * cvx_rowstat_finalize: the partial row sums a CVX_EPI_RESID_HL GEMM left in stat_part[nslot = C / 64][part_rows][2] ->
 *   rowstat[rows][2] for the next GEMM. */
int cvx_final_norm_features_hl(const void* xh, const void* xl, long ld, const float* w, const float* b, float eps, int slices,
                               int ntp, int tok0, int hp, int wp, int C, void* feats_f16, long d_total, long d0,
                               void* feats_cl, float* tokens_f32, hipStream_t stream);
int cvx_split_stream(const float* x, long ldx, void* xh, void* xl, long ld, float* rowstat, long rows, int C, float eps,
                     hipStream_t stream);
int cvx_rowstat_finalize(const float* part, int nslot, long part_rows, float* rowstat, long rows, int C, float eps,
                         hipStream_t stream);
/* (hi, lo) -> fp32 rows, x = hi + lo (exact): the hand-over from a folded stretch of a stream to kernels that take fp32. */
int cvx_merge_stream(const void* xh, const void* xl, long ld, float* x, long ldx, long rows, int C, hipStream_t stream);

/* im2col of already-resized 3-channel images x fp32 [b][3][Hi][Wi] (Hi, Wi multiples of 14) for the
 * encoder-protocol entry point forward_features(x) (run/dino_features.py:58): out bf16 [b*hp*wp][k_pad],
 * k = c*196 + py*14 + px (the flattening of Conv2d(3,C,14,14).weight), zero padded to k_pad >= 588. */
int cvx_im2col_patches(const float* x, int b, int Hi, int Wi, void* out, int k_pad, hipStream_t stream);

/* fp16 [C][D][h][w] (the HDF5 `dino_features` layout) -> fp16 channels-last [D][h][w][C] (a transpose: exact) */
int cvx_features_to_channels_last(const void* feats_f16, void* out_cl, int C, long nvox, hipStream_t stream);

/* GroupNorm over a channels-last fp16 volume x[nvox][C], G groups (<= 512), biased variance, eps inside sqrt
 * (nn.GroupNorm(G, C, eps=1e-3) -- cryovit.py:69).  Three launches: per-block partial sums, fixed-order reduction (no
 * atomics: results are bitwise reproducible) that also leaves the per-channel affine coefficients, apply -> fp16 out.
 * stats: fp32 scratch of 2*G*(1 + CVX_GN_BLOCKS) floats (stats[0..2G) = sum | sum of squares per group after the call;
 * block partials and the 2*C coefficients behind them). */
#define CVX_GN_BLOCKS 1024
#define CVX_GN_MAX_GROUPS 512
int cvx_groupnorm_f16(const void* x, const float* w, const float* b, void* out, float* stats, long nvox, int C,
                       int G, float eps, hipStream_t stream);
/* The same with an activation fused into the apply pass (act: 0 none, 1 exact GELU).  G = C is
 * nn.InstanceNorm3d(C, eps, affine=True) of the UNet3D baseline (models/unet3d.py:19-25,127-140). */
int cvx_groupnorm_act_f16(const void* x, const float* w, const float* b, void* out, float* stats, long nvox, int C,
                           int G, float eps, int act, hipStream_t stream);
/* The same writing into a column block of a WIDER channels-last buffer: out points at the block's first column, rows are ldo
 * elements apart (ldo >= C, a multiple of 8); out2_dense (nullable) receives a second, dense [nvox][C] copy.  torch.cat along the
 * channels of a UNet3D synthesis block (models/unet3d.py:64) then costs no pass of its own: both of its inputs are outputs of this op. */
int cvx_groupnorm_act_strided_f16(const void* x, const float* w, const float* b, void* out, long ldo, void* out2_dense, float* stats,
                                   long nvox, int C, int G, float eps, int act, hipStream_t stream);

/* Last layer of the head at full resolution, channels-last fp16 in[D][H][W][8]:
 *   conv3x3x3(8->1, w fp32 [27][8] tap-major) + bias, clip(+-5) -> logits fp32 (nullable), sigmoid -> probs fp32
 *   (nullable), and masked Dice partial sums (labels int8 nullable; dice must be zeroed by the caller):
 *   dice[0] += sum(y*p_hat), dice[1] += sum(y), dice[2] += sum(p_hat) over labels > -1, p_hat = (p >= mask_threshold): the
 *   threshold of DiceMetric (configs/model/metrics/dice_metric.yaml: 0.5) and of the uint8 mask are ONE parameter.
 * Replaces output_layer.2 + clip + sigmoid (cryovit.py:33,39,49) and the reductions of
 * base_model.py:99-110 / metrics.py:36-41.  (output_layer.0 + GELU runs through cvx_conv3d_f16.)
 * scratch: >= 3*CVX_DICE_BLOCKS floats (per-block partial sums, reduced in a fixed order: reproducible).
 * mask (nullable): uint8 [D][H][W] = (p >= mask_threshold), the binary segmentation PredictionWriter stores
 * (src/cryovit/models/callbacks.py:100-102), written here so that only 1 byte per voxel leaves the GPU. */
#define CVX_DICE_BLOCKS 4096
int cvx_conv3_out_fused(const void* in, const float* w, float bias, float* logits, float* probs, const int8_t* labels,
                        float* dice, float* scratch, uint8_t* mask, float mask_threshold, int D, int H, int W,
                        hipStream_t stream);

/* Masked Dice partial sums over existing predictions (same definition as above, threshold thr): dice[k] += the three counts.
 * The counts are accumulated as integers (per block) and added in fp64 in a fixed order, then rounded ONCE to fp32: exact and
 * bitwise reproducible also beyond 2^24 voxels.  scratch: >= 3*CVX_DICE_BLOCKS floats. */
int cvx_dice_sums(const float* probs, const int8_t* labels, float* dice, float* scratch, long n, float thr, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training-side pieces of the head (csrc/train.hip).
 *
 * cvx_dice_loss_forward -- replaces DiceLoss.forward (/root/reference/src/cryovit/models/losses.py:17-32) applied to the
 *   masked predictions of BaseModel._masked_predict (models/base_model.py:91-112): over the n voxels with label > -1,
 *   out4 = { I = sum y p, Sy = sum y, Sp = sum p, loss = 1 - 2 I / (Sy + Sp + 1e-3) }.  probs fp32 (16-B aligned), labels int8
 *   in {-1, 0, 1}; scratch: >= 3*CVX_DICE_BLOCKS floats.  Block partials + fixed-order finalize: bitwise reproducible.
 * cvx_dice_loss_backward -- what autograd derives for that expression: grad[i] = grad_out * (-2 y_i / den + 2 I / den^2) for
 *   label > -1, 0 elsewhere (den = Sy + Sp + 1e-3; sums4 = the forward's out4, on the device).  through_sigmoid = 1 continues
 *   through p = sigmoid(clip(logit, -5, 5)) (models/cryovit.py:39,49): * p (1 - p), and 0 where |logits[i]| >= 5 (logits
 *   nullable: the clipped logits the forward stored).
 * cvx_adamw_step -- one torch.optim.AdamW step (the optimizer of BaseModel.configure_optimizers, models/base_model.py:57-63)
 *   over flat fp32 arrays (16-B aligned), in place, same order of operations as torch's single-tensor path:
 *   p *= 1 - lr wd; m += (1 - b1)(g - m); v = b2 v + (1 - b2) g^2; p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
 * --------------------------------------------------------------------------------------------------- */
int cvx_dice_loss_forward(const float* probs, const int8_t* labels, long n, float* scratch, float* out4, hipStream_t stream);
int cvx_dice_loss_backward(const float* probs, const float* logits, const int8_t* labels, long n, const float* sums4, float grad_out,
                           int through_sigmoid, float* grad, hipStream_t stream);
int cvx_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int step, hipStream_t stream);
/* cvx_focal_loss_forward / _backward -- FocalLoss.forward (/root/reference/src/cryovit/models/losses.py:35-64), i.e.
 * torchvision.ops.sigmoid_focal_loss(y_pred, y_true, alpha = (n - sum y) / n, gamma, reduction = "mean") over the voxels with
 * label > -1 (x: the model output the reference passes as the loss's "logits"; labels int8).  out4 = {count, sum y, alpha, loss};
 * scratch >= 3*CVX_DICE_BLOCKS floats.  backward: grad[i] = grad_out / count * d loss_i / d x_i, alpha treated as a constant
 * (weight.item()), 0 where the label is -1. */
int cvx_focal_loss_forward(const float* x, const int8_t* labels, long n, float gamma, float* scratch, float* out4, hipStream_t stream);
int cvx_focal_loss_backward(const float* x, const int8_t* labels, long n, float gamma, const float* stats4, float grad_out, float* grad,
                            hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Backward of the segmentation head (csrc/head_backward.hip).  All volumes are channels-last fp16 unless said
 * otherwise; no floating-point atomics: block partials in a caller-provided workspace, then a fixed-order finalize, with a slab
 * count that depends on the shape only, so every result is bitwise reproducible.
 *
 * cvx_conv_wgrad_f16 -- weight and bias gradient of a 3x3x3 "same" convolution with dilation (dil, 1, 1) (taps = 27) or of a
 *   per-voxel linear map (taps = 1: the 1x1x1 projection, and the (1,2,2) transposed convolution on its unshuffled rows):
 *   dW[o][tap*C + c] = sum_v dz[v][o] x[v + shift(tap)][c]  (fp32 [cout][taps*C], the forward's k order; padded taps add exact
 *   zeros),  db[o] = sum_v dz[v][o]  (fp32 [cout], nullable).  x [D][H][W][C], dz [D][H][W][cout]; C % 8 == 0, cout % 4 == 0.
 *   workspace: cvx_conv_wgrad_workspace_bytes(...) bytes, 16-B aligned.
 * cvx_gelu_f16 -- y = gelu(z), the exact-erf form of the forward epilogues, one fp16 rounding; n elements, 16-B aligned buffers.
 * cvx_gelu_backward_f16 -- dz = dy (Phi(z) + z phi(z)), fp32 math, one fp16 rounding.  unshuffle = 0: elementwise over n.
 *   unshuffle = 1: dy and z are [D][2H][2W][c3], dz is [D*H*W][4*c3] with column (i*2 + j)*c3 + o of row (z, y, x) taken from voxel
 *   (z, 2y + i, 2x + j) -- the inverse of the transposed convolution's pixel shuffle; n = D*H*W*4*c3, c3 % 8 == 0.
 * cvx_groupnorm_backward_f16 -- x: the GroupNorm input, dn: the gradient of its output, stats: the forward's stats buffer
 *   (sum | sum of squares per group).  dgamma_c = sum_v dn xhat, dbeta_c = sum_v dn (fp32), dx = rstd (gamma dn - m1 - xhat m2)
 *   (fp16) with m1, m2 the group means of gamma dn and gamma dn xhat; fp32 partials, fp64 finalize.
 *   workspace: cvx_groupnorm_backward_workspace_floats(C, G) floats.
 * cvx_conv3_out_backward -- the 8 -> 1 output convolution (fp32 weights w [27][8]) from the fp32 logit gradient [D][H][W]:
 *   dy_mid[v][c] = sum_tap dlogit[v - tap] w[tap][c] (fp16), dW[tap][c] = sum_v dlogit[v] y_mid[v + tap][c] (fp32 [27][8]),
 *   db = sum_v dlogit[v].  workspace: cvx_conv3_out_backward_workspace_floats() floats.
 * cvx_unscale_check_f32 -- g[i] *= inv_scale in place; *flag (device int) = 1 if any product is not finite, else 0.
 * --------------------------------------------------------------------------------------------------- */
long cvx_conv_wgrad_workspace_bytes(int C, int cout, int taps, int dil, int D, int H, int W);
int cvx_conv_wgrad_f16(const void* x, const void* dz, int C, int cout, int taps, int dil, int D, int H, int W, float* dW, float* db,
                       void* workspace, long workspace_bytes, hipStream_t stream);
int cvx_gelu_f16(const void* z, void* y, long n, hipStream_t stream);
int cvx_gelu_backward_f16(const void* dy, const void* z, void* dz, long n, int unshuffle, int D, int H, int W, int c3, hipStream_t stream);
long cvx_groupnorm_backward_workspace_floats(int C, int G);
int cvx_groupnorm_backward_f16(const void* x, const void* dn, const float* gamma, const float* stats, void* dx, float* dgamma, float* dbeta,
                               float* workspace, long workspace_floats, long nvox, int C, int G, float eps, hipStream_t stream);
long cvx_conv3_out_backward_workspace_floats(void);
int cvx_conv3_out_backward(const float* dlogit, const void* y_mid, const float* w, void* dy_mid, float* dW, float* db, float* workspace,
                           long workspace_floats, int D, int H, int W, hipStream_t stream);
int cvx_unscale_check_f32(float* g, long n, float inv_scale, int* flag, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Backward of the UNet3D baseline (csrc/unet_backward.hip): what UNet3D has and the head does not.  Channels-last
 * fp16 volumes, 16-B aligned; the same reduction rule as above (fp32 block partials, fp64 fixed-order finalize, bitwise reproducible).
 *
 * cvx_instnorm_gelu_backward_f16 -- backward of cvx_groupnorm_act_f16(G = C, act = 1) from the layer's input z [nvox][C], the gradient
 *   dy of its output and the forward's stats buffer (sum | sum of squares per channel).  Recomputed in fp32: xhat = (z - mean) rstd,
 *   n = gamma xhat + beta, dn = dy (Phi(n) + n phi(n)).  dbeta_c = sum_v dn, dgamma_c = sum_v dn xhat (fp32),
 *   dz = rstd (gamma dn - mean_v(gamma dn) - xhat mean_v(gamma dn xhat)) (one fp16 rounding).  Two passes over dy and z.
 *   C % 8 == 0, C <= CVX_GN_MAX_GROUPS, nvox >= 2; workspace: cvx_instnorm_gelu_backward_workspace_floats(C) floats.
 * cvx_space_to_depth_f16 -- x [D][H][W][C] (even extents) -> out [D/2 * H/2 * W/2][8C], column ((iz*2 + iy)*2 + ix)*C + c of row
 *   (z, y, x) taken from voxel (2z + iz, 2y + iy, 2x + ix): the row layout of the stride-2 pooling convolution and of the
 *   transposed convolution's GEMM.  C % 8 == 0.
 * cvx_pointwise_out_backward -- the 1x1x1 output layer (fp32 weights w [C], C in {8, 16, 32, 64}) from the fp32 logit gradient
 *   [nvox] and the layer's input y: dy[v][c] = dlogit[v] w[c] (fp16), dW[c] = sum_v dlogit[v] y[v][c], db = sum_v dlogit[v] (fp32).
 *   workspace: cvx_pointwise_out_backward_workspace_floats(C) floats.
 * cvx_concat_backward_f16 -- dcat [nvox][c_up + c_skip] is split: d_up[v][c] = dcat[v][c] (dense [nvox][c_up]) and
 *   d_skip[v][c] = dcat[v][c_up + c] + d_pool[v][c], summed in fp32 and rounded once.  c_up % 8 == 0, c_skip % 8 == 0.  One of d_up and
 *   d_skip may be null (d_pool too when d_skip is): that half is neither read nor written -- the up half is needed before the
 *   pooling branch's gradient exists.
 * --------------------------------------------------------------------------------------------------- */
long cvx_instnorm_gelu_backward_workspace_floats(int C);
int cvx_instnorm_gelu_backward_f16(const void* dy, const void* z, const float* gamma, const float* beta, const float* stats, void* dz,
                                   float* dgamma, float* dbeta, float* workspace, long workspace_floats, long nvox, int C, float eps,
                                   hipStream_t stream);
int cvx_space_to_depth_f16(const void* x, void* out, int D, int H, int W, int C, hipStream_t stream);
long cvx_pointwise_out_backward_workspace_floats(int C);
int cvx_pointwise_out_backward(const float* dlogit, const void* y, const float* w, void* dy, float* dW, float* db, float* workspace,
                               long workspace_floats, long nvox, int C, hipStream_t stream);
int cvx_concat_backward_f16(const void* dcat, const void* d_pool, void* d_up, void* d_skip, long nvox, int c_up, int c_skip,
                            hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Alternate encoder: SAM2.1 Hiera image encoder + FPN neck (BASELINE configs[4]).  These entry points, together with
 * cvx_gemm_bf16 (qkv / proj / MLP / patch-embed / lateral convs) and cvx_layernorm_bf16, replace
 * `self.model.image_encoder(flat_data)` and the resize in front of it -- SAM2.forward_features,
 * src/cryovit/models/sam2.py:190-209 -- whose outputs _sam_features stores as float16
 * (src/cryovit/run/dino_features.py:67-106).  Token rows are channels-last: row = (slice * G + y) * G + x.
 * ------------------------------------------------------------------------------------------------- */

/* Resize to S x S (bilinear, align_corners = False: the in-plane part of the reference's trilinear F.interpolate,
 * sam2.py:196-203; identity when H == W == S) and gather the 7x7 / stride 4 / pad 3 patches of the patch-embedding
 * conv as a bf16 GEMM operand out[slices*(S/4)^2][ldo], column c*49 + ky*7 + kx (zero outside the image).
 * mode 0: src uint8 [D][H][W] scaled by 1/255 and replicated to 3 channels (vit_dataset.py:86-88,136-137);
 * mode 1: float [D][H][W] replicated; mode 2: float [D][3][H][W]. */
int cvx_sam_patches(const void* src, int mode, int slices, int H, int W, int S, void* out, long ldo, hipStream_t stream);

/* Multi-head attention inside windows of a token grid (Hiera's MultiScaleAttention after window_partition):
 * keys/values k, v: bf16 rows on a grid x grid token grid (leading dimension ldkv, head h at column h*head_dim),
 * windows of window x window tokens (window == grid: global attention); queries q on a q_grid x q_grid grid with
 * q_window x q_window windows -- the same grid, or the 2x2-pooled one of a stage transition.  out rows follow the query
 * grid.  softmax(q k^T / sqrt(head_dim)) v per (slice, window, head).  window^2 % 16 == 0, head_dim % 4 == 0, <= 96. */
int cvx_window_attention_bf16(const void* q, long ldq, const void* k, const void* v, long ldkv, void* out, long ldo,
                              int slices, int heads, int head_dim, int grid, int window, int q_grid, int q_window,
                              hipStream_t stream);

/* 2x2 max pool over the token grid (Hiera's do_pool): rows on grid x grid -> rows on grid/2 x grid/2, C channels;
 * fp32 (is_bf16 = 0: the residual shortcut) or bf16 (the queries). */
int cvx_pool2x2(const void* in, long ldi, void* out, long ldo, int slices, int grid, int C, int is_bf16, hipStream_t stream);

/* fp32 rows -> bf16 rows (residual stream -> GEMM operand of the FPN lateral convs). */
int cvx_cast_bf16(const float* in, long ldi, void* out, long ldo, long rows, int C, hipStream_t stream);

/* One FPN level: out_f16[slice][c][y][x] = lateral[(slice*grid + y)*grid + x][c] (+ coarse[(slice*grid/2 + y/2)*grid/2
 * + x/2][c] when coarse != NULL: the nearest-upsampled top-down term), fp32 in, float16 out. */
int cvx_fpn_level_out(const float* lateral, const float* coarse, int slices, int C, int grid, void* out_f16,
                      hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The whole DINOv2-with-registers encoder for one slice batch as ONE call: token init + patch-embed
 * GEMM, `depth` x { LN, QK GEMM, V^T GEMM, attention, proj GEMM (LayerScale+residual), LN, FFN-in GEMM (SwiGLU gate or
 * GELU), FFN-out GEMM (LayerScale+residual) }, final LN + feature layouts.  Replaces the hub model's forward_features
 * (run/dino_features.py:58).  All pointers are device buffers owned by the caller; weights are packed as documented for
 * cvx_gemm_bf16 (Q rows pre-scaled by log2(e)/8; W12 interleaved in blocks of 8 for the SwiGLU variant).
 * ------------------------------------------------------------------------------------------------- */
typedef struct cvx_vit_layer {
    const float *ln1_w, *ln1_b;
    const void* qk_w; const float* qk_b;      /* bf16 [rup(2C,128)][C], fp32 [rup(2C,128)] */
    const void* v_w; const float* v_b;        /* bf16 [rup(C,128)][C] */
    const void* proj_w; const float *proj_b, *ls1;
    const float *ln2_w, *ln2_b;
    const void* ffn1_w; const float* ffn1_b;  /* SwiGLU: bf16 [2*hid_pad][C] interleaved; MLP: bf16 [hid_pad][C] */
    const void* ffn2_w; const float *ffn2_b, *ls2; /* bf16 [rup(C,128)][hid_pad] */
} cvx_vit_layer;

typedef struct cvx_vit_desc {
    int dim, depth, heads, n_reg, ffn_swiglu, hid_pad;
    float ln_eps;
    int qkv_merged;                /* 1 (with ln_fold): ONE qkv GEMM per block -- layers[i].qk_w / qk_b hold all 3C rows (q | k | v), v_w / v_b
                                      are not read, ws.qk is [rows][3C] and ws.vt is not used; attention through cvx_attention_qkv_bf16 */
    int ln_fold;                   /* 1 (the product path): LayerNorms folded into the qk / v / ffn1 GEMMs and the residual stream
                                      kept as a bf16 (hi, lo) pair.  The layers then carry qk_w / v_w / ffn1_w = bf16(W * ln_gamma)
                                      and qk_b / v_b / ffn1_b = fp32 [2][n_pad] (b' | column sums, see cvx_gemm_desc.ln_rowstat);
                                      ln1_* / ln2_* are not read.  0: separate cvx_layernorm_bf16 passes over an fp32 stream */
    const float* pe_b;             /* fp32 [rup(C,128)] patch-embed bias */
    const float* reg;              /* fp32 [n_reg][C] register tokens */
    const float *norm_w, *norm_b;  /* final LayerNorm */
    const cvx_vit_layer* layers;   /* HOST array of `depth` entries (device pointers inside) */
} cvx_vit_desc;

typedef struct cvx_vit_ws {        /* device workspaces, rows = rup(b*ntp,256)+256 (ntp = tokens per slice rounded up to 8) */
    void* x;    /* fp32 [rows][C]: the residual stream (ln_fold = 0); ln_fold = 1: staging of the embedded tokens only, dead
                   after the split -- it may alias `hid` when hid_pad >= 2 C */
    void* xn;   /* bf16 [rows][C]  LayerNorm output (ln_fold = 0 only; may be NULL otherwise) */
    void* qk;   /* bf16 [rows][2C]       */
    void* vt;   /* bf16 [b][heads][64][kp], zero-initialised once (kp = tokens rounded up to 64) */
    void* ao;   /* bf16 [rows][C], zero-initialised once */
    void* hid;  /* bf16 [rows][hid_pad]  */
    /* ln_fold = 1: */
    void* xh;   /* bf16 [rows][C]  hi half of the residual stream = A operand of the qk / v / ffn1 GEMMs */
    void* xl;   /* bf16 [rows][C]  lo half */
    float* stat_part; /* fp32 [C / 64][rows][2] partial row sums */
    float* rowstat;   /* fp32 [rows][2] (rstd, -mean * rstd) */
} cvx_vit_ws;

/* patches: bf16 [rup(b*hp*wp,256)+256][patches_ld] from cvx_preprocess_patches (patches_ld = 256, pe_w = channel-summed
 * kernel [rup(C,128)][256]) or cvx_im2col_patches (patches_ld = 640, pe_w [rup(C,128)][640]); pos fp32 [1+hp*wp][C]
 * (interpolated position table), cls_pos0 fp32 [C] = cls_token + pos[0].  Outputs as in cvx_final_norm_features. */
int cvx_vit_encode(const cvx_vit_desc* vit, const cvx_vit_ws* ws, int b, int hp, int wp, const void* patches, long patches_ld,
                   const void* pe_w, const float* pos, const float* cls_pos0, void* feats_f16, long d_total, long d0,
                   void* feats_cl, float* tokens_f32, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The whole CryoVIT segmentation head as ONE call: Conv3d(c_in -> c0, k=1) + GELU, n_blocks x SynthesisBlock { GroupNorm(eps
 * 1e-3), dilated Conv3d + GELU, dilated Conv3d + GELU, ConvTranspose3d (1,2,2) + GELU }, Conv3d(8,8,3) + GELU, Conv3d(8,1,3),
 * clip(+-5), sigmoid, masked Dice sums and the thresholded uint8 segmentation.  Replaces CryoVIT.forward_volume / forward
 * (src/cryovit/models/cryovit.py:36-49), the reductions of base_model.py:99-110 / metrics.py:36-41 and PredictionWriter's
 * threshold (callbacks.py:100-102).  Weights packed as documented for cvx_gemm_bf16 / cvx_conv3d_f16, in FP16.
 * ------------------------------------------------------------------------------------------------- */
typedef struct cvx_head_block {
    int c1, c2, c3, d1, d2, groups;           /* SynthesisBlock(c1, c2, c3, d1, d2); groups = max(8, c1/8) */
    const float *gn_w, *gn_b;                 /* fp32 [c1] */
    const void* conv1_w; const float* conv1_b; int conv1_npad, conv1_kpad;   /* fp16 [npad][rup(27*c1,64)] */
    const void* conv2_w; const float* conv2_b; int conv2_npad, conv2_kpad;   /* fp16 [npad][rup(27*c2,64)] */
    const void* convt_w; const float* convt_b; int convt_npad, convt_kpad;   /* fp16 [npad(4*c3)][rup(c2,64)], row (i*2+j)*c3 + o */
} cvx_head_block;

typedef struct cvx_head_desc {
    int c_in, c0, c_tail, n_blocks;           /* c_tail must be 8 */
    const void* proj_w; const float* proj_b; int proj_npad, proj_kpad;
    const cvx_head_block* blocks;             /* HOST array of n_blocks entries (device pointers inside) */
    const void* out0_w; const float* out0_b; int out0_npad, out0_kpad;        /* Conv3d(8,8,3) */
    const float* out2_w; float out2_b;        /* Conv3d(8,1,3): fp32 [27][8] tap-major, scalar bias */
    const void* zero_page;                    /* >= 256 zero bytes */
} cvx_head_desc;

#define CVX_HEAD_MAX_BLOCKS 8
typedef struct cvx_head_ws {                  /* device workspaces, fp16 channels-last, rows = rup(voxels,256)+256 (+2048 elements) */
    void* act0;                               /* [D*h*w rows][c0] */
    void* gn[CVX_HEAD_MAX_BLOCKS];            /* block i input resolution rows x c1 */
    void* t1[CVX_HEAD_MAX_BLOCKS];            /* rows x c2 */
    void* t2[CVX_HEAD_MAX_BLOCKS];            /* rows x c2 */
    void* up[CVX_HEAD_MAX_BLOCKS];            /* 4*rows x c3 */
    void* mid;                                /* full-resolution rows x 8 */
    float* gn_stats;                          /* fp32 [2*G_max*(1+CVX_GN_BLOCKS)], G_max = 128 */
    float* dice_scratch;                      /* fp32 [3*CVX_DICE_BLOCKS] (only read when labels != NULL) */
} cvx_head_ws;

/* feats_cl: FP16 channels-last features [D*h*w (+pad rows)][c_in] (cvx_vit_encode's feats_cl or
 * cvx_features_to_channels_last).  Outputs at 2^n_blocks x the in-plane resolution, all nullable: logits / probs fp32,
 * dice fp32[3] (+=, needs labels int8), mask uint8 (probs >= mask_threshold). */
int cvx_head_forward(const cvx_head_desc* head, const cvx_head_ws* ws, const void* feats_cl, int D, int h, int w, float* logits,
                     float* probs, const int8_t* labels, float* dice, uint8_t* mask, float mask_threshold, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * PCA colour maps of DINO features (export_features=True / `cryovit features --visualize`; the reference's
 * cryovit/visualization/dino_pca.py with PCA-3 in place of PCA(1024) + UMAP).  feats: fp16 [C][D][hw] (the
 * features as the encoder writes them, hw = h*w); only slices 0, 10, 20, ... (D' = ceil(D / 10), N' = D'*hw rows) are read.
 * Everything is deterministic: fixed-order reductions, no atomics.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_PCA_SLICE_STEP 10

/* bytes of device scratch cvx_pca_moments_f16 needs (fp32 split-K partials of the Gram tiles); < 0 on bad sizes */
long cvx_pca_moments_scratch_bytes(int C, int D, int hw);
/* sums fp64 [C] = column sums over the N' selected rows; gram fp64 [C][C] = X X^T over them (fp16 MFMA, fp32 split
 * partials summed in fp64 in split order, exactly symmetric).  No centring: the caller forms (G - s s^T / N') / (N' - 1). */
int cvx_pca_moments_f16(const void* feats, int C, int D, int hw, double* sums, double* gram, void* scratch, long scratch_bytes,
                        hipStream_t stream);
/* proj fp32 [3][N'] = comps (fp32 [3][C]) . (x - mean (fp32 [C])) for every selected row, row index = slice' * hw + pixel */
int cvx_pca_project_f16(const void* feats, int C, int D, int hw, const float* mean, const float* comps, float* proj,
                        hipStream_t stream);
/* bytes of device scratch cvx_pca_colormap needs: fp32 [3][D'][2h][2w] upsampled maps + min / max partials */
long cvx_pca_colormap_scratch_bytes(int D, int H, int W);
/* canvas uint8 [D'][16h][2*16w][3] (h = ceil(H/16), w = ceil(W/16); 16-byte aligned), one RGB image per selected slice:
 * black, the data slice 10*j' (data uint8 when is_u8 else fp32 [D][H][W], min-max normalised over the whole volume, truncated,
 * flipped vertically, grey) at the origin, and at column x_map the colour map of proj (fp32 [3][D'][h][w] from
 * cvx_pca_project_f16): bicubic x2 (A = -0.75), per-channel min-max over all D' slices, matplotlib rgb_to_hsv, s = 0.9,
 * v = 0.75, hsv_to_rgb, (uint8)(255 * rgb), each pixel an 8x8 block, flipped vertically (x_map = W as the reference
 * pastes it; anything past the canvas edge is dropped). */
int cvx_pca_colormap(const float* proj, const void* data, int is_u8, int D, int H, int W, int x_map, uint8_t* canvas, void* scratch,
                     long scratch_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Label decode and evaluation counts (`cryovit evaluate`, run/eval_model.py:run_evaluation).  labels: the label volume as read
 * from its file, one of the CVX_LABEL_* dtypes, n elements; labels / probs / y_out 16-byte aligned.  Integer results only,
 * combined with integer atomics (exact and order-independent: two calls give the same bits).
 * ------------------------------------------------------------------------------------------------- */
#define CVX_LABEL_I8 0
#define CVX_LABEL_U8 1
#define CVX_LABEL_I16 2
#define CVX_LABEL_U16 3
#define CVX_LABEL_I32 4
#define CVX_LABEL_F32 5
#define CVX_LABEL_BITMAP_BITS 65536                            /* widest value range the census resolves */
#define CVX_LABEL_CENSUS_WORDS (4 + CVX_LABEL_BITMAP_BITS / 32)
#define CVX_LABEL_NONINTEGER 1                                 /* census flag: a float32 value is NaN, inf or not an integer */
#define CVX_LABEL_WIDE 2                                       /* census flag: max - min >= CVX_LABEL_BITMAP_BITS (or outside int32) */
#define CVX_LABEL_MATCH 0  /* y = 1 where lab == value, -1 (ignored) where lab == -1, else (value == 0 ? 1 : 0): _match_label_keys_to_data */
#define CVX_LABEL_WEIGHT 1 /* y = int8(lab), ignored where y <= -1: the single-key HDF branch of load_labels */

/* census int32 [CVX_LABEL_CENSUS_WORDS] (written whole): [0] min, [1] max, [2] flags, [3] 0, then a bitmap of
 * CVX_LABEL_BITMAP_BITS bits, word 4 + k/32 bit k%32 set iff the value min + k occurs.  The bitmap is left empty when a flag is
 * set.  n == 0 gives min = INT_MAX > max = INT_MIN. */
int cvx_label_census(const void* labels, int dtype, long n, int32_t* census, hipStream_t stream);
/* counts uint64 [5] (+=) over the voxels with y > -1 (y decoded as `mode` says with `value`): sum y, sum [p >= thr],
 * sum y [p >= thr], sum [p > thr], sum y [p > thr]; probs fp32 [n].  y_out (nullable) int8 [n] = y of every voxel. */
int cvx_label_metrics(const float* probs, const void* labels, int dtype, long n, int mode, int value, float thr, uint64_t* counts,
                      int8_t* y_out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Multi-label segmentation overlays (`python -m cryovit_amd.training.visualize_results --exp_type segmentations`; the
 * reference's cryovit/visualization/segmentations.py).  One streaming pass, no atomics: two calls give the same bits.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_SEG_MAX_LABELS 8
#define CVX_SEG_F32 0 /* label volume of fp32 probabilities */
#define CVX_SEG_U8 1  /* label volume of uint8 masks */

/* out uint8 [D][H][2W][3] (any alignment): left half the grey data, right half the overlay.  data fp32 [D][H][W]; labels /
 * label_dtypes / colours are HOST arrays of n (0 <= n <= CVX_SEG_MAX_LABELS) device pointers to [D][H][W] volumes, their
 * CVX_SEG_* dtypes and n x 3 RGB doubles.  Per voxel and channel c, as numpy evaluates it: comb = 0 (fp32); for each label in
 * order comb = (float)((double)comb + (double)seg * colour[c]); comb = clip(comb, 0, 1); g = clip(data, 0, 1); right =
 * comb > (float)threshold ? comb : g (per channel); left = g; bytes = (uint8)(x * 255.0f), truncated.  Inputs must be finite. */
int cvx_seg_overlay(const float* data, const void* const* labels, const int* label_dtypes, const double* colours, int n, int D,
                    int H, int W, double threshold, uint8_t* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Connected instances of a predicted mask (`cryovit infer --instances`, `cryovit instances`).  mask uint8 [D][H][W], nonzero =
 * foreground.  Two foreground voxels belong to one component iff a chain of foreground voxels joins them, each step a
 * neighbour under the connectivity: 6 (faces) or 26 (faces, edges, corners); no wrap-around.  Background is 0; components are
 * numbered 1..K in ascending order of their smallest linear voxel index (z*H + y)*W + x, the order of a C-order raster scan.
 * Components with fewer than min_size voxels become background and the others are numbered 1..K in the same order (min_size 0
 * and 1 remove nothing).  Integers only (integer atomic add / min / max): two calls give the same bits.
 * Two calls, because the table has K rows and K is known only after the first:
 *   cvx_components_label   writes the int32 K to the first 4 bytes of scratch; labels is used as workspace
 *   (the caller reads K once and allocates table int64 [K][CVX_COMPONENT_COLS])
 *   cvx_components_table   writes labels int32 [D][H][W] and the table, from the same scratch, on the same stream
 * A table row: voxels, sum_z, sum_y, sum_x, z0, z1, y0, y1, x0, x1 (bounding box inclusive).  An empty volume and an all-zero
 * mask give K = 0.  Refused with an error: D*H*W > CVX_COMPONENT_MAX_VOXELS, negative extents, another connectivity, null
 * pointers, scratch shorter than cvx_components_scratch_bytes.  labels and scratch 16-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_COMPONENT_COLS 10
#define CVX_COMPONENT_MAX_VOXELS 2147483646L /* 2^31 - 2: voxel index + 1 is held in an int32 */

/* bytes of device scratch for one volume; < 0 on bad extents */
long cvx_components_scratch_bytes(int D, int H, int W);
int cvx_components_label(const uint8_t* mask, int D, int H, int W, int connectivity, long min_size, int32_t* labels, void* scratch,
                         long scratch_bytes, hipStream_t stream);
/* k: the K that cvx_components_label left in scratch (ids past k are written as background rather than past the table) */
int cvx_components_table(int D, int H, int W, long k, int32_t* labels, int64_t* table, const void* scratch, long scratch_bytes,
                         hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Exact squared Euclidean distance maps (`--morphology`, `cryovit instances --distance-to`).  src [D][H][W] is uint8 (a mask)
 * or int32 (an instance volume); the sites are its zero voxels (CVX_EDT_SITES_ZERO: the depth inside the foreground, the
 * convention of scipy.ndimage.distance_transform_edt) or its nonzero voxels (CVX_EDT_SITES_NONZERO: the distance to the
 * foreground).  out int32 [D][H][W]: out[v] = min over the site voxels s INSIDE the volume of |v - s|^2, in voxels, exact; 0 on
 * a site; CVX_EDT_NONE everywhere when the volume holds no site.  Voxels outside the volume are never sites.  Integers only,
 * no atomics, no workspace.  Refused with an error before any launch: null pointers, negative extents, D*H*W >
 * CVX_COMPONENT_MAX_VOXELS, (D-1)^2 + (H-1)^2 + (W-1)^2 >= INT32_MAX, another dtype or sites value.  An empty volume succeeds.
 *
 * cvx_instance_distance_stats: labels int32 [D][H][W] with ids 0..k, d2 as written by cvx_edt_squared, out int64
 * [k][CVX_DSTAT_COLS] (initialised by the call).  Row id - 1, over the voxels of that id with d2 != CVX_EDT_NONE: the number with
 * d2 <= threshold_d2, min d2, max d2, and the smallest linear index (z*H + y)*W + x of a voxel that attains the max.  An id
 * without such a voxel gets 0, -1, -1, -1; ids outside 1..k are ignored; k == 0 succeeds.  64-bit integer atomic add / min /
 * max only (the argmax rides in one packed key), so the table does not depend on scheduling.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_EDT_U8 0
#define CVX_EDT_I32 1
#define CVX_EDT_SITES_ZERO 0
#define CVX_EDT_SITES_NONZERO 1
#define CVX_EDT_NONE 2147483647 /* INT32_MAX */
#define CVX_DSTAT_COLS 4

int cvx_edt_squared(const void* src, int src_dtype, int sites, int D, int H, int W, int32_t* out, hipStream_t stream);
int cvx_instance_distance_stats(const int32_t* labels, const int32_t* d2, int D, int H, int W, long k, int threshold_d2,
                                int64_t* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Nearest-instance maps and pairwise contacts between the instances of two labels (`cryovit instances --contacts-with`).
 *
 * cvx_nearest_instance: labels int32 [D][H][W]; a voxel is a site iff its value lies in 1..k (other values are nobody's, as
 * in cvx_instance_distance_stats).  d2_out int32 [D][H][W] = min over the sites s of |v - s|^2: bit for bit what
 * cvx_edt_squared(CVX_EDT_SITES_NONZERO) gives when every nonzero value lies in 1..k.  nearest_out int32 [D][H][W] = the
 * smallest id among the sites that attain it; on a site its own id.  Without a site: CVX_EDT_NONE and 0 everywhere.
 * workspace: cvx_nearest_workspace_bytes(D, H, W) = 8 * D*H*W bytes, 8-byte aligned: the keys d2 << 32 | id between the passes;
 * its contents after the call mean nothing.  Integers only, no atomics.  Refused with an error before any launch: what
 * cvx_edt_squared refuses (null pointers, negative extents, D*H*W > CVX_COMPONENT_MAX_VOXELS, the squared diagonal >= INT32_MAX)
 * and k < 0.  An empty volume succeeds.
 *
 * cvx_instance_pair_contacts: over the voxels v with a = labels_a[v] in 1..ka, b = nearest_b[v] != 0 and 0 <= d2_b[v] <=
 * threshold_d2 (nearest_b, d2_b as cvx_nearest_instance wrote them for the other label), every pair (a, b) accumulates
 * contact_voxels = their number, gap_d2 = the smallest d2_b among them and `at` = the smallest linear index of a voxel that
 * attains it.  The pairs land in an open-addressed table of `capacity` slots (a power of two in 1..CVX_PAIR_MAX_CAPACITY):
 * table int64 [3][capacity] = per slot the key a << 32 | b (INT64_MAX: empty), the count, and gap_d2 << 32 | at; status int64
 * [2] = {1 if some pair found no slot (the table is then void: repeat with a larger one), P = the claimed slots}.  Both are
 * initialised by the call and stay on the device.  Integer atomic add / min / max only; no part of a table that did not
 * overflow, other than which slot a pair sits in, depends on capacity or scheduling.
 * cvx_instance_pair_rows: rows int64 [p][CVX_PAIR_COLS] = a, b, contact_voxels, gap_d2, at of the slots order[0..p): the
 * caller sorts the table's keys ascending (empty slots sort last) and passes the first P slot indices, which gives the rows in
 * (a, b) order.  An index that names no claimed slot gives -1, -1, 0, -1, -1.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_PAIR_COLS 5
#define CVX_PAIR_MAX_CAPACITY 2147483648L /* 2^31: more slots than voxels */

long cvx_nearest_workspace_bytes(int D, int H, int W); /* < 0 on bad extents */
int cvx_nearest_instance(const int32_t* labels, long k, int D, int H, int W, int32_t* d2_out, int32_t* nearest_out, void* workspace,
                         hipStream_t stream);
int cvx_instance_pair_contacts(const int32_t* labels_a, long ka, const int32_t* nearest_b, const int32_t* d2_b, int threshold_d2,
                               int D, int H, int W, int64_t* table, long capacity, int64_t* status, hipStream_t stream);
int cvx_instance_pair_rows(const int64_t* table, long capacity, const int64_t* order, long p, int64_t* rows, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The contingency table between two instance volumes (`cryovit evaluate --instance-metrics`).
 *
 * cvx_overlap_instances: over the voxels v with a = labels_a[v] in 1..ka and b = labels_b[v] in 1..kb (other values are
 * nobody's), every pair (a, b) accumulates its number of voxels and the smallest linear index of one.  Table, status, capacity,
 * overflow and refusals are those of cvx_instance_pair_contacts (kb < 0 is refused as ka < 0 is); the third word of a slot holds
 * the index (a gap_d2 of 0), so cvx_instance_pair_rows reads the rows out as a, b, voxels, 0, at.  Counts are reduced per
 * thread, per wave and per workgroup (a small table in LDS) before they reach the table; integer atomics only, and no part of
 * a table that did not overflow, other than which slot a pair sits in, depends on capacity or scheduling.
 * ------------------------------------------------------------------------------------------------- */
int cvx_overlap_instances(const int32_t* labels_a, long ka, const int32_t* labels_b, long kb, int D, int H, int W, int64_t* table,
                          long capacity, int64_t* status, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Per-instance shape (`infer --instances --shape`, `cryovit instances --shape`): the integer sums from which the surface area
 * (discrete Crofton estimate), the Euler number and the principal axes of every instance follow.
 *
 * labels int32 [D][H][W]; voxel v belongs to instance i iff labels[v] == i with i in 1..k; ids outside 1..k belong to nobody, as
 * in cvx_instance_distance_stats.  For a given i everything that is not i counts as outside: background, other ids (split pieces
 * touch each other) and positions beyond the volume.  out int64 [k][CVX_SHAPE_COLS], initialised by the call.  Row i - 1:
 *    0       voxels n
 *    1..3    sum of z, y, x over the voxels
 *    4..9    sum of zz, yy, xx, zy, zx, yx
 *   10       Euler number of the instance under `connectivity` (6 or 26)
 *   11..23   N[0..12], the crossing counts N_d = #{v in i : v + d not in i} over the 13 directions d = (dz, dy, dx) that are
 *            lexicographically greater than (0,0,0), in lexicographic order: (0,0,1), (0,1,-1), (0,1,0), (0,1,1), (1,-1,-1), ...,
 *            (1,1,1).  The opposite direction gives the same number and is not stored.
 *
 * The Euler number is a sum over the voxels of i of a function of the 26 "same id" bits of the voxel's neighbourhood:
 *   connectivity 6    chi = #voxels - #face-adjacent pairs + #full 2x2 squares - #full 2x2x2 cubes: the cubical complex on the
 *                     voxel centres, which has the homotopy type of the 6-connected instance.  Every such cell is counted at its
 *                     raster-first voxel, which sees the rest of it at offsets >= 0.
 *   connectivity 26   chi = #lattice corners - #lattice edges + #lattice faces - #voxels of the union of the closed unit cubes
 *                     of i (cubes that share a face, an edge or a corner are joined: 26-connectivity).  A cell counts when any
 *                     voxel around it (8 around a corner, 4 around an edge, 2 at a face) belongs to i, and it is counted at the
 *                     raster-first voxel OF i among those, so that a foreign voxel in front does not lose it.
 *
 * Integers only (64-bit integer atomic adds): two calls give the same bits.  Every sum fits in int64: extents are at most 32768
 * and n <= D*H*W <= CVX_COMPONENT_MAX_VOXELS < 2^31, so a first moment is below 2^31 * 2^15 = 2^46, a second moment below 2^31 *
 * 2^30 = 2^61, a crossing count at most n, and the Euler number, to which a voxel adds between -13 and +13, below 2^35 in magnitude.
 * Refused with an error before any launch: null pointers, negative extents, an extent above 32768, D*H*W >
 * CVX_COMPONENT_MAX_VOXELS, k < 0, a connectivity other than 6 or 26, misaligned arrays (labels: 4 bytes, out: 8 bytes).  k == 0
 * and an empty volume succeed.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_SHAPE_COLS 24
int cvx_instance_shape_stats(const int32_t* labels, int D, int H, int W, long k, int connectivity, int64_t* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Touching instances split at their necks (`infer --instances --split-radius`, `cryovit instances --split-radius`).  labels
 * int32 [D][H][W] with ids 0..k as cvx_components_table writes them (two ids never share a face).  The caller erodes: d2 =
 * cvx_edt_squared(labels, CVX_EDT_I32, CVX_EDT_SITES_ZERO), cvx_split_core_mask marks d2 > threshold_d2 (= floor(radius^2)) with
 * d2 != CVX_EDT_NONE, and cvx_components_label / _table number that mask's components 1..m: the cores.  A threshold of 0 erodes
 * nothing: the caller then passes no cores (m = 0), and every instance is its own seed.  A volume without background has d2 =
 * CVX_EDT_NONE everywhere, hence no core either: the split is the identity.
 *   cvx_split_init     keys uint64 [D][H][W] = steps << 32 | seed id: a voxel of core c starts at (0, c); every voxel of an
 *                      instance i that holds no core voxel at (0, m + i); all else at all-ones.  has_core int32 [k + 1] is
 *                      workspace (cores may be null when m = 0).
 *   cvx_split_rounds   `rounds` launches of the regrowth kernel: a step joins two neighbours (connectivity 6 or 26) that carry
 *                      the SAME non-zero label, and every round lowers keys towards the fixpoint key[v] = min over such
 *                      neighbours n of key[n] + (1 << 32), i.e. the pair (fewest steps to a seed, smallest seed id among those).
 *                      changed int32 [rounds] is cleared by the call; round r sets changed[r] = 1 iff it lowered a key.  A round
 *                      that lowered nothing proves the fixpoint (and so does every round after it); the caller launches until
 *                      it sees one.  No workgroup waits for another; keys only ever decrease, each written by one aligned 8-byte
 *                      store.
 *   cvx_split_first    first int32 [seeds + 1] (seeds = m + k): per seed id the smallest linear index of a voxel whose key
 *                      names it, INT32_MAX for a seed that owns none (and in entry 0).  The caller ranks these: rank int32
 *                      [seeds + 1], 1..kp for the kp seeds that own a voxel in ascending order of `first`, anything else for
 *                      the rest.
 *   cvx_split_relabel  labels_out int32 [D][H][W] = rank of the voxel's seed (0 for background), table int64
 *                      [kp][CVX_COMPONENT_COLS] with the columns of cvx_components_table, component int64 [kp] = the input id
 *                      each piece lies in.  Ranks outside 1..kp are written as background rather than past the table.
 * Every piece is connected and lies inside one input instance.  Integers only (integer atomic add / min / max, plain stores of
 * equal values): two calls give the same bits.  Refused with an error before any launch: null pointers, negative extents, D*H*W >
 * CVX_COMPONENT_MAX_VOXELS, another connectivity, k, m, seeds or kp out of range, misaligned arrays (int32: 4 bytes; keys, table,
 * component: 8 bytes).  An empty volume succeeds.
 * ------------------------------------------------------------------------------------------------- */
int cvx_split_core_mask(const int32_t* d2, int D, int H, int W, int threshold_d2, uint8_t* mask, hipStream_t stream);
int cvx_split_init(const int32_t* labels, const int32_t* cores, int D, int H, int W, long k, long m, int32_t* has_core,
                   uint64_t* keys, hipStream_t stream);
int cvx_split_rounds(const int32_t* labels, uint64_t* keys, int D, int H, int W, int connectivity, int rounds, int32_t* changed,
                     hipStream_t stream);
int cvx_split_first(const int32_t* labels, const uint64_t* keys, int D, int H, int W, long seeds, int32_t* first,
                    hipStream_t stream);
int cvx_split_relabel(const int32_t* labels, const uint64_t* keys, const int32_t* rank, int D, int H, int W, long seeds, long kp,
                      int32_t* labels_out, int64_t* table, int64_t* component, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Centreline skeletons of instances (`infer --instances --skeleton`, `cryovit instances --skeleton`): topology-preserving
 * thinning in the order of a priority volume, and the per-instance table of the result.  Integers only, bit-reproducible.
 *
 * labels int32 [D][H][W]; ids outside 1..k and positions outside the volume are nobody's; for an instance everything that is
 * not its own id is outside.  d2 int32 [D][H][W] is the priority (in the product cvx_edt_squared(labels, CVX_EDT_I32,
 * CVX_EDT_SITES_ZERO)); it must not overlap alive.  For an alive voxel v with id i, its mask m has bit (dz+1)*9 + (dy+1)*3 +
 * (dx+1) set for each of the 26 neighbours that is alive with id i (the bit order of cvx_instance_shape_stats).
 *   simple          (a) the set bits of m are non-empty and form one 26-connected set, and (b) the unset positions of v's
 *                   18-neighbourhood that are face neighbours of v are non-empty and lie in one set connected through face steps
 *                   within the unset 18-neighbourhood positions: the classical (26,6) simple point.
 *   protected end   m has exactly one set bit and d2[v] >= end_d2.
 *   candidate       alive, d2[v] <= level_d2 and d2[v] != CVX_EDT_NONE.
 *   cycle           for subfield s = 0..7 in order: every candidate with ((z&1)<<2 | (y&1)<<1 | (x&1)) == s that is simple and no
 *                   protected end is deleted, all of them at once (one launch).  Two voxels of one subfield are never
 *                   26-adjacent and a decision reads the 26 neighbours only, so the launch updates alive in place and equals
 *                   deleting the same voxels one after another; a cycle after one that deleted nothing deletes nothing.
 * The caller finds Lmax, the smallest L with L*L >= the largest d2 != CVX_EDT_NONE over the alive voxels, and for L = 1..Lmax
 * repeats cycles with level_d2 = L*L until one deletes nothing.  What remains has, per id, the 26-components, handles and
 * cavities of the instance.
 *   cvx_skeleton_init    alive = labels with ids outside 1..k set to 0.
 *   cvx_skeleton_cycles  `cycles` cycles (8 launches each).  changed int32 [cycles] is cleared by the call; cycle c sets
 *                        changed[c] non-zero iff it deleted a voxel.
 *   cvx_skeleton_stats   table int64 [k][CVX_SKELETON_COLS], initialised by the call.  Row id - 1 over the alive voxels of that
 *                        id: 0 voxels; 1 voxels with exactly one alive same-id neighbour (of 26); 2 with three or more; 3 with
 *                        none; 4, 5, 6 links by a face, an edge, a corner step (a link is an unordered pair of 26-adjacent alive
 *                        voxels of the id, counted at its raster-first voxel: over the 13 directions after (0,0,0)); 7 the sum
 *                        of d2 over the voxels, CVX_EDT_NONE entries adding 0.  A count is at most 13 * D*H*W < 2^35 and the
 *                        sum of d2 below 2^31 * 2^31.
 * Refused with an error before any launch: null pointers, negative extents, an extent above 32768, D*H*W >
 * CVX_COMPONENT_MAX_VOXELS, k < 0, misaligned arrays (int32: 4 bytes, table: 8 bytes); by cvx_skeleton_cycles also end_d2 < 1,
 * level_d2 < 0 and cycles < 1.  k == 0 and an empty volume succeed.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_SKELETON_COLS 8
int cvx_skeleton_init(const int32_t* labels, int D, int H, int W, long k, int32_t* alive, hipStream_t stream);
int cvx_skeleton_cycles(int32_t* alive, const int32_t* d2, int D, int H, int W, long k, int level_d2, int end_d2, int cycles,
                        int32_t* changed, hipStream_t stream);
int cvx_skeleton_stats(const int32_t* alive, const int32_t* d2, int D, int H, int W, long k, int64_t* table, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Local thickness (`infer --instances --thickness`, `cryovit instances --thickness`): at every voxel the largest ball that fits
 * inside the structure and holds the voxel (Hildebrand & Ruegsegger), as its squared radius, and the per-instance table over it.
 * Integers only, bit-reproducible.
 *
 * d2 int32 [D][H][W], non-negative (in the product cvx_edt_squared(labels, CVX_EDT_I32, CVX_EDT_SITES_ZERO), but any values
 * are taken as they are).  t2 int32 [D][H][W], another array than d2:
 *   t2[p] = 0                                                             where d2[p] == 0,
 *   t2[p] = max { d2[c] : d2[c] > 0 and |p - c|^2 < d2[c] } over all voxels c of the volume   elsewhere.
 * The ball is open and c = p qualifies, so t2 >= d2.  Balls are clipped by the volume; its border is no site.  If any d2 is
 * CVX_EDT_NONE every nonzero voxel gets CVX_EDT_NONE.  Ids play no part: after a split, pieces that share a face are measured
 * as their union.
 *   cvx_local_thickness_workspace_bytes  4 bytes per 4x8x64 tile of the volume plus 4; < 0 on bad extents.
 *   cvx_local_thickness_squared          workspace: that many bytes, 4-byte aligned; its contents after the call mean nothing.
 *   cvx_instance_thickness_stats         table int64 [k][CVX_THICKNESS_COLS], initialised by the call.  Row id - 1 over the voxels
 *                                        with that id in 1..k whose t2 is neither 0 nor CVX_EDT_NONE: 0 voxels; 1 the sum of t2;
 *                                        2 the sum of r_fx = floor(sqrt(t2 * 2^16)), the exact integer root; 3 min t2; 4 max t2.
 *                                        An id without such a voxel: 0, 0, 0, -1, -1.  Sums stay below 2^31 * 2^31.
 * Refused with an error before any launch: negative extents, an extent above 32768, D*H*W > CVX_COMPONENT_MAX_VOXELS, k < 0,
 * null pointers, misaligned arrays (int32: 4 bytes, table: 8 bytes), a workspace shorter than
 * cvx_local_thickness_workspace_bytes, d2 == t2.  k == 0 and an empty volume succeed.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_THICKNESS_COLS 5
long cvx_local_thickness_workspace_bytes(int D, int H, int W);
int cvx_local_thickness_squared(const int32_t* d2, int D, int H, int W, int32_t* t2, void* workspace, long workspace_bytes,
                                hipStream_t stream);
int cvx_instance_thickness_stats(const int32_t* labels, const int32_t* t2, int D, int H, int W, long k, int64_t* table,
                                 hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Surface mesh (`infer --instances --mesh`, `cryovit instances --mesh`): one watertight, consistently oriented, indexed triangle
 * mesh of the mask labels > 0, by marching tetrahedra on the Kuhn decomposition; per-instance triangles, area and volume; integer
 * Taubin smoothing.  Integers only, bit-reproducible.
 *
 * Lattice.  The volume is treated as surrounded by one layer of background, so every surface closes (unlike cvx_edt_squared, where
 *   the border is no site).  A cell is the cube between 8 neighbouring voxel centres of the padded lattice: (D+1)(H+1)(W+1) cells,
 *   raster order z, y, x.  Each cell is cut into the 6 Kuhn tetrahedra: the paths from its corner (0,0,0) to (1,1,1) that add the
 *   three unit steps in the axis orders (z,y,x), (z,x,y), (y,z,x), (y,x,z), (x,z,y), (x,y,z) = tet 0..5.  Neighbouring cells agree on
 *   their common face, so there is no ambiguous case.  The connectivity this implies is 14 for foreground and background alike: the
 *   6 face neighbours, the face diagonals (0,1,1), (1,0,1), (1,1,0) and the body diagonal (1,1,1), each with its opposite.
 * Vertices.  One at the midpoint of every lattice edge of the decomposition whose ends differ in labels > 0; the edge types of a
 *   lower end are 0..6 = the offsets z, y, x, zy, zx, yx, zyx.  int32 [V][3] in z, y, x order, in units of 1/256 voxel: (a + b) * 128
 *   for the ends a, b in unpadded voxel coordinates (so -128 occurs).  Ordered by (raster index of the lower end, edge type).
 * Triangles.  int32 [T][3], ordered by (cell, tet, triangle 0 / 1).  A tet with 1 or 3 foreground corners gives one triangle: the
 *   edges from the single corner to the others (or from the others to it) in the order of the path.  A tet with foreground corners
 *   a < b and background corners c < d (positions along the path) gives the quad (ac, ad, bd, bc) as (ac, ad, bd) and (ac, bd, bc).
 *   Where the normal (p1 - p0) x (p2 - p0) of a triangle so listed does not point from foreground to background, p1 and p2 are
 *   exchanged.  ids int32 [T]: the label of the tet's first foreground corner along the path; ids otherwise play no part, so
 *   instances that share a face are meshed as their union and the plane between them carries no triangle.
 *
 *   cvx_mesh_workspace_bytes   8 bytes per 64 cells of a cell row (two int32 per row segment: 0.125 bytes per voxel) + 16; < 0 on
 *                              bad extents.
 *   cvx_mesh_count             totals int64 [2] in device memory = V, T; the workspace (16-byte aligned) keeps what cvx_mesh_emit needs.
 *   cvx_mesh_emit              the same labels and workspace, after cvx_mesh_count on the same stream; vertices [V][3], triangles [T][3],
 *                              ids [T] of exactly the counted sizes (with other V, T nothing is written).
 *   cvx_mesh_stats             table int64 [k][CVX_MESH_COLS], initialised by the call, row id - 1 over the triangles with that id in
 *                              1..k, of whatever vertex array is passed (coordinates within +-2^24): 0 triangles; 1 the sum of
 *                              floor(sqrt(|n|^2)), n = (p1 - p0) x (p2 - p0) (area = c1 / 2 / 65536 voxel^2); 2 the sum of
 *                              det(p0, p1, p2) modulo 2^64 (volume = c2 / 6 / 256^3 voxel^3, meaningful for an instance whose shell its
 *                              own triangles close).  A triangle with an index outside [0, V) is ignored.
 *   cvx_mesh_smooth_step       moved = x + floor((S - n x) c / (n 65536)) per vertex and axis in int64, S and n the sum and count of
 *                              the b of every directed edge a -> b (a triangle (a, b, c) gives a -> b, b -> c, c -> a; on a closed
 *                              oriented manifold that is every neighbour once); c = factor * 65536, |c| <= CVX_MESH_FACTOR_MAX; a
 *                              vertex without a neighbour stays; moved may be vertices.  Workspace: cvx_mesh_smooth_workspace_bytes
 *                              (32 bytes per vertex), 8-byte aligned.
 * Refused with an error before any launch: negative extents, an extent above 32768, D*H*W > CVX_COMPONENT_MAX_VOXELS, k < 0,
 * V or T negative or >= 2^31, null pointers, misaligned arrays, a short workspace.  An empty volume (V = T = 0) and k == 0 succeed.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_MESH_COLS 3
#define CVX_MESH_FACTOR_MAX 131072
long cvx_mesh_workspace_bytes(int D, int H, int W);
int cvx_mesh_count(const int32_t* labels, int D, int H, int W, void* workspace, long workspace_bytes, int64_t* totals, hipStream_t stream);
int cvx_mesh_emit(const int32_t* labels, int D, int H, int W, const void* workspace, long workspace_bytes, long V, long T,
                  int32_t* vertices, int32_t* triangles, int32_t* ids, hipStream_t stream);
int cvx_mesh_stats(const int32_t* vertices, const int32_t* triangles, const int32_t* ids, long V, long T, long k, int64_t* table,
                   hipStream_t stream);
long cvx_mesh_smooth_workspace_bytes(long V);
int cvx_mesh_smooth_step(const int32_t* vertices, int32_t* moved, const int32_t* triangles, long V, long T, int c, void* workspace,
                         long workspace_bytes, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Cleaning a predicted mask before it is labelled (`--close-radius`, `--fill-holes`, `--open-radius` of `infer --instances` and
 * `cryovit instances`).  Integers only, bit-reproducible.
 *
 * Fill holes.  A background voxel of mask uint8 [D][H][W] is filled unless it is connected to the border through background
 * voxels under the background connectivity 6 or 26.  The border is the six faces of the volume; with slices = 1 every z-slice is
 * an image of its own, the border its four edges, and the connectivity 4 (for 6) or 8 (for 26) within the slice.  The flood runs
 * on bits: WW = ceil(W / 64) uint64 words per row, [D][H][WW], bit i of word w = voxel x = 64 w + i; bits past W are 0.
 *   cvx_mask_flood_pack    open = (mask == 0); reach = the open bits of the border.
 *   cvx_mask_flood_rounds  `rounds` launches of the flood kernel: every round sets bits of reach towards the fixpoint reach = open
 *                          and (on the border or next to a reach voxel).  changed int32 [rounds] is cleared by the call; round r
 *                          sets changed[r] = 1 iff it set a bit.  A round that set none proves the fixpoint; the caller launches
 *                          until it sees one.  No workgroup waits for another; bits are only ever set, each word written by one
 *                          aligned 8-byte store, so the fixpoint does not depend on scheduling (the number of rounds does).
 *   cvx_mask_flood_unpack  out uint8 [D][H][W] = 1 where the voxel is not in reach (foreground or filled), 0 where it is.
 * Ball steps.  cvx_mask_threshold: out uint8 [D][H][W] = d2 <= threshold_d2 (CVX_MASK_LE: with d2 = cvx_edt_squared(...,
 *   CVX_EDT_SITES_NONZERO) the dilation by the ball |v|^2 <= threshold_d2) or d2 > threshold_d2 (CVX_MASK_GT: with
 *   CVX_EDT_SITES_ZERO the erosion; CVX_EDT_NONE is above every threshold), where d2 int32 [D+2 pad][H+2 pad][W+2 pad] is read at
 *   (z + pad, y + pad, x + pad): the crop of a map that was computed on a padded copy.
 * Added voxels.  cvx_mask_added_voxels: out int64 [k], initialised by the call; out[id - 1] = the voxels with labels == id (int32
 *   [D][H][W], ids 1..k, others ignored) where before (uint8 [D][H][W], the mask as predicted) is 0.
 * Refused with an error before any launch: negative extents, D*H*W (for cvx_mask_threshold also the padded extents' product) >
 * CVX_COMPONENT_MAX_VOXELS, null pointers, misaligned arrays (words and out of added_voxels: 8 bytes, int32: 4 bytes), open ==
 * reach, slices other than 0 / 1, a background other than 6 / 26, rounds < 1, pad outside [0, 32768], another mode, a threshold
 * outside [0, 2^31 - 2], k < 0.  An empty volume and k == 0 succeed and launch nothing.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_MASK_LE 0
#define CVX_MASK_GT 1
int cvx_mask_flood_pack(const uint8_t* mask, int D, int H, int W, int slices, uint64_t* open, uint64_t* reach, hipStream_t stream);
int cvx_mask_flood_rounds(const uint64_t* open, uint64_t* reach, int D, int H, int W, int background, int slices, int rounds,
                          int32_t* changed, hipStream_t stream);
int cvx_mask_flood_unpack(const uint64_t* reach, int D, int H, int W, uint8_t* out, hipStream_t stream);
int cvx_mask_threshold(const int32_t* d2, int D, int H, int W, int pad, int mode, int threshold_d2, uint8_t* out, hipStream_t stream);
int cvx_mask_added_voxels(const int32_t* labels, const uint8_t* before, int D, int H, int W, long k, int64_t* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Scoring a prediction at its boundary (`cryovit evaluate --boundary`: HD95, surface distance, surface Dice).  Integers only, no
 * float atomics, bit-reproducible.
 *
 * cvx_slices_edt_squared: the contract of cvx_edt_squared with every z-slice an image of its own: out[z][y][x] = min over the
 *   sites s of slice z of (y - sy)^2 + (x - sx)^2; a slice without a site is CVX_EDT_NONE throughout, whatever its neighbours
 *   hold.  Refused like cvx_edt_squared, the diagonal rule being (H-1)^2 + (W-1)^2 < INT32_MAX.
 * cvx_slice_valid: y int8 [D][H][W], a decoded label volume in which a value <= -1 means "not annotated"; valid int32 [D],
 *   every entry written by plain stores: valid[z] = 1 iff no voxel of slice z has y <= -1 (an empty slice is valid).
 * cvx_surface_mask: mask uint8 [D][H][W] (nonzero = foreground); out uint8 [D][H][W], every voxel written: 1 iff the voxel is
 *   foreground and one of its face neighbours is background or outside the volume (MedPy's surface, m & ~erosion(m, cross,
 *   border_value = 0)).  slices = 1: the 4 neighbours within the z-slice, and valid (int32 [D], nullable = every slice) zeroes the
 *   slices with valid[z] == 0.  slices = 0: the 6 neighbours in 3-D; a non-null valid is refused.  out must not be mask.
 * cvx_surface_distance_hist: surf uint8 [n], d2 int32 [n] (a distance map as cvx_edt_squared writes it), hist int64 [bins + 1],
 *   initialised by the call.  Every voxel with surf != 0 adds 1 to one entry: hist[bins] when d2 == CVX_EDT_NONE (unmatched: there
 *   was nothing to measure against); else hist[bins - 1] when (uint32)d2 >= bins - 1 (overflow, which also takes a negative d2);
 *   else hist[d2].  32-bit LDS and 64-bit global integer adds only, so the histogram does not depend on scheduling.
 * Refused with an error before any launch: negative extents, D*H*W > CVX_COMPONENT_MAX_VOXELS, null pointers, misaligned arrays
 * (int32: 4 bytes, hist: 8 bytes), slices other than 0 / 1, valid with slices = 0, mask == out, n outside [0, 2^40], bins outside
 * [2, 2^24 + 1].  An empty volume succeeds and launches nothing; n == 0 succeeds and leaves hist zero.
 * ------------------------------------------------------------------------------------------------- */
int cvx_slices_edt_squared(const void* src, int src_dtype, int sites, int D, int H, int W, int32_t* out, hipStream_t stream);
int cvx_slice_valid(const int8_t* y, int D, int H, int W, int32_t* valid, hipStream_t stream);
int cvx_surface_mask(const uint8_t* mask, const int32_t* valid, int D, int H, int W, int slices, uint8_t* out, hipStream_t stream);
int cvx_surface_distance_hist(const uint8_t* surf, const int32_t* d2, long n, long bins, int64_t* hist, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Membrane curvature (`infer --instances --curvature`, `cryovit instances --curvature`): the mean curvature H of the surface of
 * labels > 0 by the ball-volume integral invariant, and the per-instance table over it.  The fraction of a ball of radius r,
 * centred on the surface, that lies inside the object is 1/2 - (3/16) r H (exact for a sphere).  Integers only, no float atomics,
 * bit-reproducible.
 *
 * labels int32 [D][H][W], F = labels > 0 (ids play no part in the map: pieces that share a face are scored as their union);
 * radius r, CVX_CURVATURE_RADIUS_MIN <= r <= CVX_CURVATURE_RADIUS_MAX.  B = {o in Z^3 : |o|^2 <= r^2}, N = |B|,
 * n(v) = #{o in B : v + o in F}.
 *   Surface voxel  p in F with at least one face neighbour that is inside the volume and not in F; Q(p) = those neighbours, m = |Q(p)|.
 *   Scored voxel   a surface voxel with r + 1 <= index <= extent - r - 2 on every axis: no ball at p or at a q of Q(p) is clipped.
 *                  A volume with an extent below 2 r + 3 has none.
 *   h[p]           floor(32768 (m N - m n(p) - S) / (3 r m N)), S = the sum of n(q) over Q(p), in int64 and rounded towards minus
 *                  infinity: H in units of 1/4096 per voxel, |h| <= 5462.  Positive = convex (a ball), negative = concave (a cavity
 *                  wall).  Pairing p with its outside neighbours cancels the half-voxel offset of the ball's centre: on an
 *                  axis-aligned face n(p) + n(q) = N and h = 0.  Every other voxel of h is CVX_CURV_NONE.
 *   cvx_curvature_workspace_bytes  8 bytes per 64 voxels of a row (the foreground as bits); < 0 on bad extents.
 *   cvx_curvature_map              h int32 [D][H][W], every voxel written; workspace: that many bytes, 8-byte aligned; its contents
 *                                  after the call mean nothing.
 *   cvx_curvature_stats            table int64 [k][CVX_CURVATURE_COLS], initialised by the call.  Row id - 1 over the voxels with
 *                                  that id in 1..k: 0 scored voxels (h != CVX_CURV_NONE); 1 the sum of h; 2 the sum of h^2; 3 min h;
 *                                  4 max h (both 0 without a scored voxel); 5 scored voxels with h > 0; 6 surface voxels (of
 *                                  labels > 0, as above) whose h is CVX_CURV_NONE.
 * Refused with an error before any launch: negative extents, an extent above 32768, D*H*W > CVX_COMPONENT_MAX_VOXELS, a radius
 * outside [2, 16], k < 0, k rows that cannot be addressed, null pointers, misaligned arrays (int32: 4 bytes, workspace and table:
 * 8 bytes), a workspace shorter than cvx_curvature_workspace_bytes, labels == h.  k == 0 and an empty volume succeed and launch
 * nothing; a volume too small for a scored voxel gets CVX_CURV_NONE throughout.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_CURVATURE_COLS 7
#define CVX_CURVATURE_RADIUS_MIN 2
#define CVX_CURVATURE_RADIUS_MAX 16
#define CVX_CURV_NONE INT32_MIN
long cvx_curvature_workspace_bytes(int D, int H, int W);
int cvx_curvature_map(const int32_t* labels, int D, int H, int W, int radius, int32_t* h, void* workspace, long workspace_bytes,
                      hipStream_t stream);
int cvx_curvature_stats(const int32_t* labels, const int32_t* h, int D, int H, int W, long k, int64_t* table, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Membrane picking (`infer --instances --pick`, `cryovit instances --pick`): evenly spaced surface voxels of every instance, each
 * with the moment of the ball that gives the membrane normal: the particle positions of subtomogram averaging.  Integers only, no
 * atomics, bit-reproducible.
 *
 * labels int32 [D][H][W], F = labels > 0, instances 1..k.  Normal radius r, CVX_PICK_RADIUS_MIN <= r <= CVX_PICK_RADIUS_MAX;
 * spacing s, CVX_PICK_SPACING_MIN <= s <= CVX_PICK_SPACING_MAX (voxels); seed, any uint32.
 *   Candidate   a voxel p with 1 <= labels[p] <= k that is a surface voxel of F (the curvature section's surface: a face neighbour
 *               inside the volume and not in F) and has r <= index <= extent - 1 - r on every axis, so the ball at p is not
 *               clipped.  Ids play no part in what is surface: a face shared by two pieces is no surface.  A volume with an extent
 *               below 2 r + 1 has no candidate.
 *   Key         key(p) = (fmix32(i XOR seed) << 32) | i, i the linear voxel index (< 2^31 by CVX_COMPONENT_MAX_VOXELS), fmix32
 *               murmur3's finaliser: h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16, all mod 2^32.  Keys
 *               are distinct, so they order the candidates totally.
 *   Picks       two candidates conflict when they carry the same id and the squared distance of their voxel centres is < s*s.  The
 *               picks are the lexicographically first maximal independent set: go through the candidates by increasing key and take
 *               one unless it conflicts with one already taken.  Within an id no two picks are closer than s, and every candidate
 *               lies closer than s to a pick of its id.
 *   Normal      at a pick p, M(p) = the sum over o in B(r) of o * [p + o in F], three int32 (z, y, x), |M| < 2^19, B the curvature
 *               section's ball; n(p) = #{o in B(r) : p + o in F}.  The outward unit normal is -M / |M| (the host computes it in
 *               float64); M == 0 marks the pick as unoriented (a one-voxel sheet: its two sides are indistinguishable).
 *   Pick table  int32 [P][CVX_PICK_COLS] in raster order of the voxel index, each row z, y, x, id, Mz, My, Mx, n.
 * The selection runs as synchronous rounds over a state of two bitmaps, uint64 [2][D][H][WW], WW = ceil(W / 64), bit i of word w of a
 * row = voxel x = 64 w + i: [0] undecided (the candidates at the start), [1] picked (empty at the start).  In one round an undecided
 * p is rejected when a picked voxel conflicts with it, picked when no undecided conflicting voxel has a smaller key, and waits
 * otherwise; the fixpoint is the set of picks above, and a round after it changes nothing.
 *   cvx_pick_workspace_bytes  the bytes B of one bitmap, 8 per 64 voxels of a row; < 0 on bad extents.  fg holds B bytes, a state
 *                             2 B; every entry takes B as workspace_bytes and refuses a smaller one.
 *   cvx_pick_pack             fg = F as bits; state = (candidates, none picked).
 *   cvx_pick_rounds           `rounds` rounds; round j = 0, 1, ... reads state_a when j is even and state_b when odd, and writes the
 *                             whole of the other (only state_a need be initialised).  changed int32 [rounds], zeroed by the call:
 *                             changed[j] = 1 iff round j rejected or picked a voxel.  After a round with changed[j] == 0 both states
 *                             hold the fixpoint.
 *   cvx_pick_count            row_first int32 [D*H] = the number of picked voxels in the rows before each row; total = P.
 *   cvx_pick_emit             the pick table of `state` from fg and row_first; P as cvx_pick_count gave it (with a larger P the
 *                             rows past the count are zero, with a smaller one the picks past it are left out).
 * Refused with an error before any launch: negative extents, an extent above 32768, D*H*W > CVX_COMPONENT_MAX_VOXELS, r or s
 * outside [2, 16], k < 0, rounds < 1, P outside [0, D*H*W], null pointers, misaligned arrays (int32: 4 bytes, bitmaps and total: 8
 * bytes), a workspace_bytes below cvx_pick_workspace_bytes, fg inside state, state_a and state_b that overlap.  k == 0, an empty
 * volume and P == 0 succeed and launch nothing (cvx_pick_rounds and cvx_pick_count still zero changed and total).
 * ------------------------------------------------------------------------------------------------- */
#define CVX_PICK_COLS 8
#define CVX_PICK_RADIUS_MIN 2
#define CVX_PICK_RADIUS_MAX 16
#define CVX_PICK_SPACING_MIN 2
#define CVX_PICK_SPACING_MAX 16
long cvx_pick_workspace_bytes(int D, int H, int W);
int cvx_pick_pack(const int32_t* labels, int D, int H, int W, long k, int radius, uint64_t* fg, uint64_t* state, long workspace_bytes,
                  hipStream_t stream);
int cvx_pick_rounds(const int32_t* labels, int D, int H, int W, long k, int spacing, uint32_t seed, int rounds, uint64_t* state_a,
                    uint64_t* state_b, long workspace_bytes, int32_t* changed, hipStream_t stream);
int cvx_pick_count(const uint64_t* state, int D, int H, int W, long workspace_bytes, int32_t* row_first, int64_t* total, hipStream_t stream);
int cvx_pick_emit(const int32_t* labels, const uint64_t* fg, const uint64_t* state, const int32_t* row_first, int D, int H, int W, int radius,
                  long workspace_bytes, long P, int32_t* table, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Filament tracing (`infer --instances --trace`, `cryovit instances --trace`): the skeleton of every instance as a graph of branches,
 * every voxel with its branch, its rank along it and the steps up to it: lengths per filament, junctions, and where to cut
 * segments for helical averaging.  Integers only, no float atomics, bit-reproducible.
 *
 * sk int32 [D][H][W] (in the product the volume of the skeleton section; any volume is traced exactly), ids outside 1..k count as 0.
 *   Neighbours   two voxels that are 26-adjacent and carry the same id; deg(v) = the number of neighbours of v.
 *   Path voxel   deg == 2.  Node voxel: any other nonzero voxel (end: deg 1, junction voxel: deg >= 3, point: deg 0).
 *   Chain        a maximal connected set of path voxels; each has at most two path neighbours, so it is open or a closed ring.  An
 *                open chain has two extremal path voxels (a chain of one voxel: the same twice) and its two terminal node voxels
 *                are their non-path neighbours.  The head is the extremal path voxel with the smaller raster index (of a
 *                one-voxel chain the start node is the neighbour with the smaller index); the branch runs from the start node, the
 *                terminal next to the head, through the ranks 1..n to the end node.
 *   Ring         a chain in which every voxel has two path neighbours.  m = its voxel with the smallest raster index has rank 1, the
 *                neighbour of m with the smaller index rank 2, and so on to rank L; start node = end node = m, and the step
 *                counts include the step that closes the ring.
 *   Link         an end voxel whose only neighbour is a node voxel; no path voxels; between two ends counted once, from the end
 *                with the smaller index.  The start is that key end voxel, the end its neighbour.
 *   Junction voxels belong to no branch; points are no branches.  The key voxel of a branch is the head of a chain, m of a ring, the
 *   key end of a link; branches are numbered 1..B in raster order of their key voxels.
 *   Steps        a step between neighbours is a face, an edge or a corner step.  A voxel's (f, e, c) count the steps from the start
 *                node to it, a branch's also the step into the end node.
 *   Voxel table  int32 [N][CVX_TRACE_VOXEL_COLS] in raster order of the N nonzero voxels: z, y, x, id, degree, branch, rank, f, e,
 *                c, d2, ring.  branch, rank and the counts are 0 on node voxels; d2 is the caller's distance map at the voxel (0
 *                without one, and where it holds CVX_EDT_NONE); ring is 1 on ring voxels.
 *   Branch table int64 [B][CVX_TRACE_BRANCH_COLS]: id, kind (0 end-end, 1 end-junction, 2 junction-junction, 3 ring), path_voxels,
 *                f, e, c, start_index, end_index (linear voxel indices), start_degree, end_degree, sum_d2, min_d2, max_d2 (over the
 *                path voxels; 0 without any), head_index, last_index (-1 for a link), chord2 (the squared distance of the start
 *                and end node voxels).
 * A voxel's slot is its row in the voxel table.  The ranking runs by pointer doubling over direction states: state 2 v + j = at
 * path voxel v, travelling to its neighbour j (0: the one with the smaller index).  A state holds CVX_TRACE_STATE_BYTES bytes.
 *   cvx_trace_workspace_bytes  the bytes of one bitmap, 8 per 64 voxels of a row; < 0 on bad extents.  bits holds two of them.
 *   cvx_trace_count            bits = (nonzero voxels, path voxels) as bits; row_first int32 [2][D*H]: [0] the voxels in the rows
 *                              before each row, [1] the same of the path voxels; totals int64 [2] = N, Np, zeroed by the call.
 *   cvx_trace_emit             z, y, x, id, degree, d2 of every voxel (the other columns 0) and nbrs int32 [N][2], the slots of the
 *                              neighbours of an end or path voxel in raster order (-1: none; both -1 on other voxels).  d2 may
 *                              be null.  With an N above the count the rows past it are zero, with a smaller one voxels are left out.
 *   cvx_trace_rank             writes the states of the path voxels to state_a and runs `rounds` doubling rounds, round j = 0, 1, ...
 *                              from state_a to state_b when j is even and back when odd: the result is in state_a after an even
 *                              number of rounds, in state_b after an odd one.  ceil(log2(max(Np, 2))) rounds bring every chain
 *                              state to its end of the chain.  cut int32 [N] (nullable): a state stops before voxel cut[v].
 *   cvx_trace_rings            cut[v] = the smallest slot of the ring v lies on, -1 elsewhere, from the states of a rank without
 *                              cut; any int32 [1], zeroed by the call, = 1 iff there is a ring.  With rings, rank again with cut.
 *   cvx_trace_keys             rank, f, e, c and ring of every path voxel; keys int32 [N] = the key voxels before each voxel;
 *                              total = B, zeroed by the call.  state (of the last rank) may be null when Np == 0, cut when
 *                              there is no ring.
 *   cvx_trace_branches         the branch column of the voxel table and the branch table; first = keys of cvx_trace_keys, B its
 *                              total (with a larger B the rows past the count are zero, with a smaller one branches are left out).
 * Refused with an error before any launch: negative extents, an extent above 32768, D*H*W > CVX_COMPONENT_MAX_VOXELS, k < 0, N
 * outside [0, D*H*W] (without extents: [0, CVX_COMPONENT_MAX_VOXELS]), B outside [0, N], rounds outside [0, 32], null pointers,
 * misaligned arrays (int32 and states: 4 bytes, bitmaps, totals and branches: 8 bytes), a workspace_bytes below
 * cvx_trace_workspace_bytes, states that overlap, a cut without a state.  k == 0, an empty volume and N == 0 succeed and launch
 * nothing (cvx_trace_count, cvx_trace_rings and cvx_trace_keys still zero totals, any and total).
 * ------------------------------------------------------------------------------------------------- */
#define CVX_TRACE_VOXEL_COLS 12
#define CVX_TRACE_BRANCH_COLS 16
#define CVX_TRACE_STATE_BYTES 20
long cvx_trace_workspace_bytes(int D, int H, int W);
int cvx_trace_count(const int32_t* sk, int D, int H, int W, long k, uint64_t* bits, long workspace_bytes, int32_t* row_first,
                    int64_t* totals, hipStream_t stream);
int cvx_trace_emit(const int32_t* sk, const int32_t* d2, const uint64_t* bits, const int32_t* row_first, int D, int H, int W, long k,
                   long workspace_bytes, long N, int32_t* voxels, int32_t* nbrs, hipStream_t stream);
int cvx_trace_rank(const int32_t* voxels, const int32_t* nbrs, const int32_t* cut, long N, int rounds, void* state_a, void* state_b,
                   hipStream_t stream);
int cvx_trace_rings(const int32_t* voxels, const void* state, long N, int32_t* cut, int32_t* any, hipStream_t stream);
int cvx_trace_keys(int32_t* voxels, const int32_t* nbrs, const void* state, const int32_t* cut, long N, int32_t* keys, int64_t* total,
                   hipStream_t stream);
int cvx_trace_branches(int32_t* voxels, const int32_t* nbrs, const void* state, const int32_t* cut, const int32_t* first, int D, int H,
                       int W, long N, long B, int64_t* branches, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Oriented subtomograms (`infer --instances --extract picks|filaments`, `cryovit instances --extract`): a box of B^3 voxels around
 * every particle, rotated so that the box axes are the columns of the particle's matrix, sampled trilinearly from the tomogram; the
 * sums of the boxes (the average) and the density profile along the box z axis.  Fixed point throughout, integers only: the result
 * does not depend on the launch shape or on any order, and two calls give the same bits.
 *
 * vol uint8 [D][H][W].  table int32 [P][CVX_SUBTOMO_COLS]: cz, cy, cx, the centre in 1/256 voxel (Q8), then m[a][j], a, j = 0..2
 * row by row, in 1/65536 (Q16): a is the source axis z, y, x, j the box axis z, y, x.  box = B, even, 8 <= B <= 128.
 *   Sampling   the box voxel (i_z, i_y, i_x) has the offset o = i - B/2.  Per source axis a, in 64 bits:
 *                s16 = (c[a] << 8) + m[a][0] o_z + m[a][1] o_y + m[a][2] o_x;  s = s16 >> 9 (arithmetic: the floor, 7 fraction bits);
 *                idx = s >> 7;  f = s & 127.
 *              q = the sum over the 8 taps d in {0, 1}^3 of w_z w_y w_x vol[clamp(idx + d)], w = f for d = 1 and 128 - f for d = 0,
 *              every index clamped to [0, extent - 1] (the border is replicated).  q is an int32 in units of 2^-21 grey level,
 *              at most 255 * 2^21; the float image is float32(q) * 2^-21.
 *   Refusal    need_a = ((15 (|m[a][0]| + |m[a][1]| + |m[a][2]|) + 65535) >> 16) + 2 bounds the source indices of axis a that a
 *              16^3 block of the box touches.  A particle with need_z > 30, need_y > 30 or need_x > 32 (no rotation: the rows of one
 *              have length 1 and need at most 28) is written as zeros and counted in *status.  The table may hold anything: no
 *              access leaves the volume, the table or out.
 *   cvx_subtomo_extract  out int32 [P][B][B][B] = q, every element written; *status int64 = the refused particles of this call.
 *   cvx_subtomo_sum      sums int64 [G][B^3] += the boxes of the particles p with group[p] == g, element by element; particles with
 *                        a group outside 0..G-1 (-1: left out) are skipped.  The caller zeroes sums once; the chunks of a long
 *                        particle list accumulate.  64-bit integer atomics.
 *   cvx_subtomo_profile  profile int64 [P][B]: entry (p, i_z) = the sum of stack[p][i_z][i_y][i_x] over o_y^2 + o_x^2 <= radius2;
 *                        the number of voxels of the disc is the host's to derive.  Every entry written.
 * Refused with an error before any launch: negative extents, D*H*W > CVX_COMPONENT_MAX_VOXELS, P < 0 or above
 * CVX_SUBTOMO_MAX_PARTICLES (cut a longer list into chunks), a box that is odd or outside [8, 128], G < 1, radius2 < 0, null pointers,
 * misaligned arrays (int32: 4 bytes, int64: 8 bytes).  P == 0, and for cvx_subtomo_extract an empty volume, succeed and touch
 * nothing, *status included.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_SUBTOMO_COLS 12
#define CVX_SUBTOMO_BOX_MIN 8
#define CVX_SUBTOMO_BOX_MAX 128
#define CVX_SUBTOMO_MAX_PARTICLES (1 << 20)
int cvx_subtomo_extract(const uint8_t* vol, int D, int H, int W, const int32_t* table, long P, int box, int32_t* out, int64_t* status,
                        hipStream_t stream);
int cvx_subtomo_sum(const int32_t* stack, long P, int box, const int32_t* group, int G, int64_t* sums, hipStream_t stream);
int cvx_subtomo_profile(const int32_t* stack, long P, int box, long radius2, int64_t* profile, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Alignment of oriented subtomograms about their axis (`--extract-align`): every box on rings around its z axis, and the circular
 * correlation of every particle with a reference table over the in-plane angle (T steps of 360/T degrees) and the shift along the
 * axis (-S..S voxels).  Integers only; the result does not depend on the launch shape or on any order; two calls give the same bits.
 * The scores, the choice of the best candidate and the refinement of the frames are the host's (analysis/alignment.py).
 *
 * cvx_align_polar: stack int32 [P][B][B][B], the output of cvx_subtomo_extract (2^-21 grey level).  trig int32 [T][2] =
 *   (rint(sin(2 pi t / T) * 2^14), rint(cos(2 pi t / T) * 2^14)), made by the host.  polar int32 [P][B][rmax][T], every element
 *   written.  Per slab z, ring r = 1..rmax and step t, in 64 bits:
 *     py7 = ((B/2) << 7) + ((r * sin_t) >> 7);  px7 = ((B/2) << 7) + ((r * cos_t) >> 7)   (arithmetic shifts: floors);
 *     i = p7 >> 7;  f = p7 & 127;  the taps i and i + 1 are clamped to [0, B - 1] per axis;
 *     polar = (the sum over the four taps of w_y w_x stack[p][z][y][x], w = f for the upper tap and 128 - f for the lower) >> 14.
 *   The weights add up to 2^14: polar is at most 255 * 2^21 and has the unit of the stack.  With the trig table above and
 *   rmax <= B/2 - 1 only an upper tap of weight 0 is clamped; with any other table the clamps keep every access inside the box.
 * cvx_align_correlate: polar as above; ref int16 [2 zh + 1][rmax][T] (1/64 grey level, the host's to make).
 *     q = min(255, (polar + 2^20) >> 21)   (a polar value outside [0, 255 * 2^21], which cvx_align_polar never writes, gives 0 or 255);
 *     corr[p][d + S][k] = sum_{z' = -zh..zh} sum_{r = 1..rmax} r * sum_{t = 0..T-1} q[p][B/2 + z' + d][r][(t + k) mod T] * ref[z' + zh][r][t]
 *   for d = -S..S, k = 0..T-1: corr int64 [P][2 S + 1][T];
 *     moments[p][z][0] = sum_r r sum_t q[p][z][r][t],  moments[p][z][1] = sum_r r sum_t q[p][z][r][t]^2
 *   for every slab z = 0..B-1: moments int64 [P][B][2].  Every element of both tables is written, by plain stores.
 *   Bounds: a sum over t of one (slab, ring) is below T * 255 * 32768 <= 2^30 and is kept in 32 bits; with the ring weights and
 *   the slabs |corr| <= 127 * 2016 * 2^30 < 2^49 (B = 128, T = 128, rmax = 63, zh = 63); a moment is below 2016 * 128 * 255^2 < 2^35.
 * Refused with an error before any launch, in this order: P < 0, a box that is odd or outside [8, 128], P above
 * CVX_SUBTOMO_MAX_PARTICLES, T other than 32, 64, 128, rmax outside [1, B/2 - 1], zh < 0, shift outside [0, CVX_ALIGN_SHIFT_MAX],
 * zh + shift > B/2 - 1 (a scored slab would leave the box), then (P > 0) null pointers and misaligned arrays (int32 and ref: 4
 * bytes, ref is read two elements at a time; int64: 8 bytes).  P == 0 succeeds and touches nothing.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_ALIGN_SHIFT_MAX 8
int cvx_align_polar(const int32_t* stack, long P, int box, const int32_t* trig, int T, int rmax, int32_t* polar, hipStream_t stream);
int cvx_align_correlate(const int32_t* polar, long P, int box, int T, int rmax, const int16_t* ref, int zh, int shift, int64_t* corr,
                          int64_t* moments, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Raw tomogram -> uint8 in [0, 255] (`cryovit preprocess`, `features --normalize`): bin, moments, order statistics, quantise.
 * A volume is [D][H][W] of one of the CVX_VOL_* element types; CVX_VOL_I32 is what the bin pass makes of an integer source.
 * Everything but the two float32 moment sums is exact and bit-reproducible; those two are reproducible and bounded (below).
 *
 * cvx_volume_bin: src [D][H][W] (int8 / uint8 / int16 / uint16 / float32; D*H*W may exceed 2^31), out [D/kz][H/k][W/k]: the
 *   sum of every kz x k x k block, 1 <= kz, k <= CVX_BIN_MAX; trailing voxels that fill no block are dropped.  Integer sources:
 *   out int32, exact.  float32: out float32 = (((0.0f + v0) + v1) + ...) over the block z outer, y, x inner, one rounding per add.
 *   No division by the block size.  Every voxel of out is written.
 * cvx_volume_moments: partials [D][P][3] of 8-byte words, P = max(1, ceil(H*W / CVX_MOMENT_GROUP)); partial (z, c) covers the
 *   voxels [c * CVX_MOMENT_GROUP, (c + 1) * CVX_MOMENT_GROUP) of slice z: word 0 int64 the finite voxels, word 1 their sum, word 2
 *   the sum of their squares.  Integer types: int64 and uint64, exact.  float32: doubles; a thread adds CVX_MOMENT_CHAIN consecutive
 *   voxels in order, a fixed tree of CVX_MOMENT_TREE levels adds the threads; squares are exact.  NaN and +-Inf are left out and
 *   not counted.  Plain stores, every word written; the caller adds the partials.
 * cvx_volume_select_hist: one pass of an exact radix select over v [slices][len].  key(v) is 32 bits and order preserving:
 *   (uint32)(v - base) for the integer types (base <= every v, v - base < 2^32), for float32 the bits with the sign bit set when
 *   it was clear and all bits flipped when it was set (base unused); NaN and +-Inf are left out.  prefix int64 [slices][ranks][2]
 *   = (value, mask); table int64 [slices][ranks][CVX_SELECT_BINS], zeroed by the call: entry [s][r][b] counts the voxels of
 *   slice s with (key & mask) == value and ((key >> shift) & (2^width - 1)) == b.  1 <= width <= 11, shift + width <= 32,
 *   1 <= ranks <= CVX_SELECT_MAX_RANKS, slices * len <= CVX_COMPONENT_MAX_VOXELS.  64-bit integer atomics.
 * cvx_volume_quantize: params double [D][3] (per_slice = 1) or [1][3] = (lo, hi, scale); out uint8 [D][H][W], every voxel
 *   written: q = floor((double(v) - lo) * scale + 0.5), each operation rounded once (no fused multiply-add), clamped to [0, 255];
 *   128 for a NaN voxel or a NaN product, 255 / 0 for +Inf / -Inf; invert = 1 stores 255 - q.  clipped int64 [D][2], zeroed by the
 *   call: the voxels of slice z with double(v) < lo and with double(v) > hi.
 * Refused with an error before any launch: another dtype (cvx_volume_bin: CVX_VOL_I32 as well), negative extents, a (binned)
 * volume with D*H*W > CVX_COMPONENT_MAX_VOXELS, bin factors outside 1..CVX_BIN_MAX, a bit field or rank count out of range, flags
 * other than 0 / 1, null pointers, misaligned arrays (elements: their size; partials, prefix, table, params, clipped: 8 bytes),
 * src == out.  An empty volume succeeds.
 * ------------------------------------------------------------------------------------------------- */
#define CVX_VOL_I8 0
#define CVX_VOL_U8 1
#define CVX_VOL_I16 2
#define CVX_VOL_U16 3
#define CVX_VOL_I32 4
#define CVX_VOL_F32 5
#define CVX_BIN_MAX 8
#define CVX_MOMENT_GROUP 4096
#define CVX_MOMENT_CHAIN 16
#define CVX_MOMENT_TREE 8
#define CVX_SELECT_BINS 2048
#define CVX_SELECT_MAX_RANKS 2
int cvx_volume_bin(const void* src, int dtype, long D, long H, long W, int kz, int k, void* out, hipStream_t stream);
int cvx_volume_moments(const void* v, int dtype, int D, int H, int W, void* partials, hipStream_t stream);
int cvx_volume_select_hist(const void* v, int dtype, long slices, long len, long base, int shift, int width, int ranks,
                           const int64_t* prefix, int64_t* table, hipStream_t stream);
int cvx_volume_quantize(const void* v, int dtype, int D, int H, int W, const double* params, int per_slice, int invert, uint8_t* out,
                        int64_t* clipped, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRYOVIT_HIP_H */
