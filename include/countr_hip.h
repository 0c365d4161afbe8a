/*
 * countr_hip.h -- C ABI of libcountr_hip.so: the MI355X (gfx950) kernels behind the CounTR
 * SupervisedMAE hot path (reference: /root/reference/models_mae_cross.py:136-207 and
 * models_crossvit.py:46-156).  The reference has no FFI of its own (it is pure PyTorch); each
 * entry point below replaces the torch.nn call sites cited next to it.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch types.  All pointers are DEVICE pointers to
 *     caller-owned, 16-byte aligned buffers unless noted.  `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success, <0 on error; countr_last_error() returns the message
 *     (thread-local).  Nothing throws across the ABI.
 *   - no hipMalloc/hipFree/synchronisation inside any call: every call only enqueues kernels on
 *     `stream`, so whole steps are hipGraph-capturable.  Workspaces are caller-allocated.
 *   - dtype codes: COUNTR_F32 = 0 (fp32 storage, exact-f32 MFMA 16x16x4), COUNTR_BF16 = 1 (bf16
 *     storage, MFMA 16x16x32 bf16 with fp32 accumulate).  Statistics, softmax, loss, gradients of
 *     parameters and optimizer state are always fp32.
 *   - activations are token-major [rows, features] (== torch [B, N, C] flattened) and images /
 *     feature maps are NHWC.
 */
#ifndef COUNTR_HIP_H
#define COUNTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_F32 0
#define COUNTR_BF16 1

/* operand addressing modes of the generic MFMA GEMM */
#define COUNTR_OP_ROW 0    /* elem(r,k) = p[r*ld + k]            (K contiguous)                    */
#define COUNTR_OP_COL 1    /* elem(r,k) = p[k*ld + r]            (K strided, rows contiguous)      */
#define COUNTR_OP_IM2ROW 2 /* r = pixel (b,y,x), k = tap*C + c : 3x3 pad-1 gather of NHWC p         */
#define COUNTR_OP_IM2COL 3 /* r = tap*C + c, k = pixel (b,y,x) : same gather, K = pixels (wgrad)    */

#define COUNTR_ACT_NONE 0
#define COUNTR_ACT_GELU 1 /* exact erf GELU, nn.GELU default (models_crossvit.py:49,63) */
#define COUNTR_ACT_GELU_BWD 2 /* out = acc * GELU'(C2): autograd of the line above fused into the fc2 dgrad GEMM; C2 is an
                                 INPUT here (the saved pre-activation, same layout and dtype as C) */

/* -------- library management -------- */
int countr_init(int device);            /* selects device, checks it is gfx950-class, allocates the library's ONE per-device
                                           constant (a vector of zeros that bias-less GEMM / convolution launches read); 0 = ok.
                                           REQUIRED once per device and PER LIBRARY before any launch: libcountr_hip.so (bf16) and
                                           libcountr_hip_f16.so (fp16) are separate images with separate state.  Idempotent and
                                           thread-safe.  A bias-less countr_gemm / countr_conv launch on a device without it fails
                                           with a negative code and a message naming countr_init (it does not allocate lazily:
                                           no allocation inside a launch) */
#define COUNTR_ABI_VERSION 9
int countr_version(void);               /* COUNTR_ABI_VERSION (9: countr_gemm_args grew at its end (gn_rows) + countr_groupnorm_relu_fwd_rows -- rebuild callers; 8: countr_transpose16 added, no layout change; 7: countr_masked_mse_amp / countr_patch_mse_amp / countr_adamw_step_amp added, no layout change; 6: countr_softmax_fwd_ld added, no layout change; 5: countr_step_prologue added, no layout change; countr_gemm_args grew at its end -- round 3: ln_* fields, rowsum_slabs; round 4: prefetch hint (3) -- so a caller built against an older version must be rebuilt; 4: countr_gemm_group / countr_gemm_group_tiles added, no layout change) */
const char* countr_last_error(void);    /* thread-local message of the last failing call        */

/*
 * Generic tiled MFMA GEMM:  C[m,n] = epilogue( alpha * sum_k A(m,k) * B(n,k) )
 *   epilogue(v) = act(v + bias[n]) + resid[(m % res_mod) , n]      (each part optional)
 *   C2 (optional) receives v + bias[n] before the activation (saved for GELU backward).
 * A is the M-side operand, B the N-side operand, each in one of the COUNTR_OP_* modes.
 * Batched when nbatch > 1: z = b0*nb1 + b1 adds b0*s?0 + b1*s?1 (in elements) to A, B, C.
 * Split-K when partial != NULL (nbatch must be 1): block z of max(splitk,1) handles a K range and stores
 * raw fp32 sums to partial[z][M][N]; finish with countr_splitk_reduce.
 * Replaces: torch addmm/bmm behind nn.Linear (models_crossvit.py:62,65,84,92,115-127;
 * models_mae_cross.py:152), q@k^T / attn@v (models_crossvit.py:87,91,121,125), the PatchEmbed conv
 * (timm PatchEmbed, models_mae_cross.py:138) and the 3x3 convs (models_mae_cross.py:47-100) as
 * implicit GEMMs, plus their autograd backward formulas.
 */
typedef struct countr_gemm_args {
  const void* A;
  const void* B;
  void* C;
  void* C2;           /* optional second output (pre-activation), same type/ld as C           */
  const float* bias;  /* optional [N] fp32                                                    */
  const float* resid; /* optional fp32 [*, ldres]; may alias C when C is fp32                 */
  float* partial;     /* split-K workspace, fp32 [splitk][M][N]                               */
  int64_t lda, ldb, ldc, ldres;
  int64_t sA0, sA1, sB0, sB1, sC0, sC1;
  int32_t M, N, K;
  int32_t res_mod;  /* 0 = residual row is m                                                  */
  int32_t act;      /* COUNTR_ACT_*                                                           */
  int32_t out_bf16; /* 1: C/C2 stored as bf16, 0: fp32                                        */
  int32_t nbatch, nb1;
  int32_t splitk;
  int32_t H, W, Cin; /* conv geometry for IM2ROW / IM2COL                                     */
  float alpha;
  float* rowsum_partial; /* optional (bf16 split-K only): fp32 [max(splitk,1)][M] receives sum_k A(m,k) per
                            K split -- the bias gradient of a wgrad GEMM, fused as one extra MFMA per tile    */
  /* LayerNorm folded into the surrounding nn.Linear layers (frozen encoder, bf16, (ROW, ROW), N % 128 == 0, K % 64 == 0 -- K % 128 == 0
   * for a consumer, whose row partials are read 16 bytes at a time; timm Block:
   * x = x + proj(attn(norm1(x))); x = x + fc2(gelu(fc1(norm2(x)))) -- models_mae_cross.py:144-146).
   * Producer (fp32 output with residual): ln_xcopy receives a bf16 copy of C, ln_stats_out[m][N/64][2] the {sum, sum of squares} of
   * every 64-column block of the fp32 output row.  Consumer (bf16 output): A is that copy, B = gamma o W, bias = b + W beta,
   * ln_stats the producer's partials (ln_nblk = K / 64 blocks per row), ln_colsum[n] = sum_k B[n][k]; the epilogue applies
   * rstd_m (acc - mean_m ln_colsum[n]) + bias[n] with mean / rstd over the K features of row m (biased variance, ln_eps). */
  void* ln_xcopy;
  float* ln_stats_out;
  const float* ln_stats;
  const float* ln_colsum;
  int32_t ln_nblk;
  float ln_eps;
  int32_t rowsum_slabs; /* slabs the caller sized rowsum_partial for: 0 = max(splitk,1) (the layout above); otherwise it must be
                           countr_gemm_rowsum_slabs() of this launch (the lean convolution weight gradient deals the bias-gradient
                           work over more waves and writes [rowsum_slabs][M]; the sum over ALL slabs is the bias gradient)        */
  /* Cache warm-up hint (ABI 3): a read-only range -- normally the B operand of the NEXT launch on the stream -- that spare workgroups
   * of this launch read once and discard (16-byte aligned pointer and size).  Honoured by the bf16 (ROW, ROW) kernels: the CUs a grid of
   * fewer than 256 tiles leaves idle (up to 64 workgroups, a multiple of 8), or 32 extra workgroups in front of a bigger grid.  Never changes a result.  Why: the frozen encoder's weight panels
   * (blocks.i.attn / mlp, models_mae_cross.py:32-34,141-145) are cold in every step -- ~5 GB stream through the 256-MB memory-side cache
   * between two uses -- and a single-round GEMM that walks a cold [N][K] panel k-slab by k-slab pays the HBM latency on every k-tile
   * (fc2: 38.7 us in the step, 28.7 us with the panel resident: tools/bench_chain.py). */
  const void* prefetch;
  int64_t prefetch_bytes;
  /* GroupNorm statistics from the convolution's epilogue (ABI 9; bf16 (IM2ROW, ROW) launches on the lean kernels -- maps of more than
   * 256 output tiles --, N % 32 == 0): gn_rows[m][N / 32][2] receives {sum, sum of squares} of every 32-channel block of output row m,
   * taken from the ROUNDED 16-bit values the launch stores (what a separate statistics pass over C would read).  The density head's
   * Conv2d -> GroupNorm(8, 256) pairs (models_mae_cross.py:80-100): countr_groupnorm_relu_fwd_rows then reads 64 bytes per pixel
   * instead of the 512-byte pixel itself.  A launch that would run on a kernel without this epilogue fails instead of leaving the
   * buffer unwritten. */
  float* gn_rows;
} countr_gemm_args;

int countr_gemm(const countr_gemm_args* a, int dtype, int modeA, int modeB, void* stream);

/* 1 when countr_gemm on these arguments runs on a kernel whose epilogue writes a->gn_rows (ABI 9), else 0 -- shape, alignment and the
 * environment's kernel selectors decide; a caller asks before it replaces its statistics pass by countr_groupnorm_relu_fwd_rows. */
int countr_gemm_gn_rows(const countr_gemm_args* a, int dtype, int modeA, int modeB);

/* Number of [M]-slabs the launch described by a (rowsum_slabs ignored) writes to rowsum_partial.  Depends on the shape and on the
 * environment switches only; callers size rowsum_partial with it and pass the value back in a->rowsum_slabs. */
int countr_gemm_rowsum_slabs(const countr_gemm_args* a, int dtype, int modeA, int modeB);

/* Output tiles (= workgroups per split-K slab) the launch described by a would run with (pointers, splitk and partial may still be
 * unset): a split-K caller picks splitk ~ CUs / tiles.  128 x 128 tiles everywhere except the lean convolution weight gradient on
 * maps with Cin % 256 == 0 (128 x 256). */
int countr_gemm_tiles(const countr_gemm_args* a, int dtype, int modeA, int modeB);

/* n (1..10) independent launches of one (dtype, modeA, modeB) kind, with the results of n countr_gemm calls bit for bit, in ONE kernel
 * launch where a grouped form exists: bf16 (COL, COL) split-K launches, i.e. the weight gradients dW = dy^T x of a transformer block's
 * nn.Linear layers (autograd of Mlp / Attention / CrossAttention, models_crossvit.py:46-128; timm Block, models_mae_cross.py:32-34).
 * Why: those are 16-72 output tiles each -- alone each needs 3-16 split-K slabs to fill 256 CUs (fp32 partials written, then summed
 * again); together they fill the chip with one or two.  Otherwise the launches run one after the other.
 * countr_gemm_group_tiles: output tiles per split-K slab of that ONE launch (the caller picks a common splitk ~ CUs / tiles), or 0 when
 * the launches would run separately (then countr_gemm_tiles applies per launch). */
int countr_gemm_group(const countr_gemm_args* items, int n, int dtype, int modeA, int modeB, void* stream);
int countr_gemm_group_tiles(const countr_gemm_args* items, int n, int dtype, int modeA, int modeB);

/* out[M,N] (+)= sum_z partial[z][M][N]; optional permute for conv weights:
 * perm_taps > 0: partial is [Cout][taps][Cin] (OHWI) and out is torch OIHW [Cout][Cin][taps].
 * rowsum_partial/rowsum_out (optional): also reduces the fused bias-gradient partials [splitk][M] -> [M]. */
int countr_splitk_reduce(const float* partial, float* out, int splitk, int M, int N, int perm_taps,
                         int accumulate, const float* rowsum_partial, float* rowsum_out, void* stream);

/* Finisher of a split-K GEMM whose result is an ACTIVATION (forward / dgrad with few tiles and a long K, e.g. the 24x24 and 8x8
 * convolutions: Conv2d forward models_mae_cross.py:47-100 and its input gradient): out[M][N] (fp32 or bf16, dense) =
 * sum_z partial[z][M][N] (+ bias[n]).  N % 4 == 0. */
int countr_splitk_finish(const float* partial, void* out, const float* bias, int splitk, int M, int N, int out_bf16,
                         void* stream);

/* Many deferred slab reductions in ONE launch (the wgrad / bias-gradient / LayerNorm dgamma-dbeta finishers of a backward phase;
 * replaces the per-parameter accumulation of autograd's AccumulateGrad nodes, util/misc.py:266-280 loss_scaler -> backward()).
 * table: device int64 [n][8] rows {partial (const float*), out (float*), nslabs | accumulate << 32 | wide << 33, slab stride
 * (floats), count, N, perm_taps, first block}: out[perm(i)] (+)= sum_z partial[z*stride + i], i < count; entry e owns the
 * 256-thread blocks [first_block(e), first_block(e+1)), total_blocks in all: ceil(count / 256) blocks per entry, or
 * ceil(count / 16) for a "wide" entry (many slabs: 16 columns x 16 slab groups per block, no permutation).  The rows are
 * followed (at table + 8 n) by an int32 array [total_blocks] giving the entry of every block.
 * perm as in countr_splitk_reduce (taps > 0). */
int countr_reduce_table(const long long* table, int n, int total_blocks, void* stream);


/* -------- LayerNorm (nn.LayerNorm eps=1e-6: models_mae_cross.py:146,182; models_crossvit.py:153-155;
 * timm Block.norm1/norm2).  x is the fp32 residual stream [rows, D]; y is fp32 or bf16.
 * mean/rstd (fp32 [rows]) are optional outputs kept for the backward. */
int countr_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, float* mean,
                         float* rstd, int rows, int D, float eps, int out_bf16, void* stream);
/* dx (+)= LN backward of dy; dgamma[D], dbeta[D] fp32 (may be NULL).  dx_bf16 (optional) receives a bf16 copy of the
 * updated dx (the operand of the next backward GEMM), saving a separate cast pass.
 * workspace: fp32 [countr_layernorm_bwd_nblocks()][2][D]. */
int countr_layernorm_bwd_nblocks(void);
int countr_layernorm_bwd(const void* dy, const float* x, const float* gamma, const float* mean,
                         const float* rstd, float* dx, float* dgamma, float* dbeta, float* workspace,
                         int rows, int D, int dy_bf16, int accumulate_dx, int accumulate_dgb, void* dx_bf16,
                         void* stream);
int countr_colsum_partials(const float* partial, float* out, int nparts, int C, int accumulate, void* stream);

/* -------- GroupNorm(8, 256) + ReLU on NHWC maps (decode_head*: models_mae_cross.py:80-100).
 * With w1 != NULL the 1x1 conv 256->1 of decode_head3 (:99) is fused: out1[b,p] = sum_c y*w1[c] + b1 and
 * y may be NULL.  stats: fp32 [B][G][2] (mean, rstd) output.  workspace: fp32 >= B*nsplit*3*256 + 64 + 16*B (forward),
 * + B*3*256 (backward: behind the split partials its finalize pass leaves the per-image sums [B][3][256] = {sum g, sum g*xhat,
 * sum d1*y} at float offset countr_groupnorm_bwd_image_sums_offset(B, HW), for callers that finish dbeta / dgamma / dw1 themselves). */
int countr_groupnorm_nsplit(int HW);
long long countr_groupnorm_bwd_image_sums_offset(int B, int HW);
int countr_groupnorm_relu_fwd(const void* x, const float* gamma, const float* beta, void* y, const float* w1,
                              const float* b1, float* out1, float* stats, float* workspace, int B, int HW,
                              int C, int G, float eps, int dtype, void* stream);
/* The same, with the statistics pass reading rows [B*HW][8][2] -- the {sum, sum of squares} per 32-channel group that the convolution
 * which produced x left through countr_gemm_args.gn_rows (ABI 9; 16-bit maps, G == 8) -- instead of the map: Conv2d -> GroupNorm of
 * decode_head1..3 on the big maps (models_mae_cross.py:86-100). */
int countr_groupnorm_relu_fwd_rows(const void* x, const float* rows, const float* gamma, const float* beta, void* y,
                                   const float* w1, const float* b1, float* out1, float* stats, float* workspace, int B,
                                   int HW, int C, int G, float eps, int dtype, void* stream);
/* dy (same dtype as x) is the gradient of y, or pass dy = NULL with d1 [B,HW] fp32 + w1 for the fused head.
 * dgamma/dbeta/dw1 [256], db1 [1] fp32 (each optional). */
int countr_groupnorm_relu_bwd(const void* x, const void* dy, const float* d1, const float* w1,
                              const float* stats, const float* gamma, const float* beta, void* dx,
                              float* dgamma, float* dbeta, float* dw1, float* db1, float* workspace, int B,
                              int HW, int C, int G, int dtype, int accumulate, void* stream);

/* -------- InstanceNorm2d(affine=False) + ReLU + MaxPool2d(2) | AdaptiveAvgPool2d(1) on NHWC
 * (decoder_proj1-4: models_mae_cross.py:47-71).  stats: fp32 [S][C][2]. */
/* workspace (optional, fp32 [countr_instnorm_workspace_floats(S, C)]): lets the wide first layers (few (sample, 64-channel)
 * blocks) run as two pixel-band kernels with Chan-combined statistics; NULL = single-kernel path. */
int countr_instnorm_workspace_floats(int S, int C);
/* xhat_out (optional; may be x itself = in place): the forward also stores the NORMALISED activation (x - mean) * rstd, rounded to the
 * dtype, and computes the pooled output from those rounded values; the backward is then given that buffer as x with x_is_xhat = 1.
 * What it is for: in bf16 an x-hat recomputed from a rounded x is off by (|mean| / sigma + |x-hat|) * 2^-9 relative, which the two
 * reductions of the InstanceNorm backward amplify (exemplar-CNN weight gradients: cosine 0.96 against fp32); a stored x-hat is good
 * to |x-hat| * 2^-9.
 * x_f32 = 1: the map x is fp32 although y / xhat_out have `dtype` (a convolution that writes its output -- bias included -- in fp32:
 * a bf16 map is rounded at 2^-9 of its VALUE, which for a channel whose mean is several sigma moves pixels across the ReLU boundary of
 * x-hat and costs the backward ~2 % in cosine per layer; the normalised activation does not have that problem). */
int countr_instnorm_relu_pool_fwd(const void* x, void* y, float* stats, int S, int H, int W, int C,
                                  int avgpool, float eps, int dtype, float* workspace, void* xhat_out, int x_f32, void* stream);
int countr_instnorm_relu_pool_bwd(const void* x, const void* dyp, const float* stats, void* dx, int S, int H,
                                  int W, int C, int avgpool, int dtype, float* workspace, int x_is_xhat, void* stream);

/* -------- fused self-attention forward (Attention.forward, models_crossvit.py:82-94 == timm Attention):
 * out = softmax(q k^T * scale) v on a packed bf16 qkv [B, N, 3, H, dh] (dh = 32 or 64) -> bf16 [B, N, H*dh].
 * lse: optional fp32 [B, H, N] log-sum-exp of the scaled scores.
 * scale <= 0 (dh = 64, N % 64 == 0 only): the caller has already multiplied q by dh^-0.5 * log2(e) -- e.g. by packing the
 * frozen encoder's q projection rows and bias pre-scaled, as engine.py does -- so the scores leave the matrix core in the exp2
 * domain and the kernel spends no VALU instruction on the scale / max subtraction. */
int countr_attn_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, int dh, float scale, void* stream);

/* Backward of countr_attn_fwd (autograd of models_crossvit.py:84-91), two fused passes, no P materialised, no atomics.
 * out/lse: the forward's outputs; dout bf16 [B, N, H*dh]; delta: fp32 [B, H, N] (must be non-NULL; not touched since both passes of the one launch compute it); dqkv bf16 [B, N, 3, H, dh]. */
int countr_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                    int B, int N, int H, int dh, float scale, void* stream);

/* -------- softmax rows for the unfused attention path (models_crossvit.py:87-88) */
int countr_softmax_fwd(const float* s, void* p, int64_t rows, int n, int out_bf16, void* stream);
/* The same with a row pitch ld >= n (ABI 6): columns n .. ld - 1 of p are written as zeros.  For token counts that are not a multiple of
 * the GEMM's 16-byte chunk (mae_vit_huge_patch14, models_mae_cross.py:235-239: 27 x 27 = 729 tokens): the score / probability
 * matrices are padded, nothing else is. */
int countr_softmax_fwd_ld(const float* s, void* p, int64_t rows, int n, int ld, int out_bf16, void* stream);
int countr_softmax_bwd(const void* p, const float* dp, void* ds, int64_t rows, int n, float scale, int dtype,
                       void* stream);

/* -------- cross attention against S <= 8 exemplar tokens (CrossAttention.forward,
 * models_crossvit.py:111-128; D = 512, 16 heads of 32).  q/out [B*N, D]; k, v [B*S, ldkv]. */
int countr_xattn_fwd(const void* q, const void* k, const void* v, void* out, int B, int N, int S, int D,
                     int heads, int ldkv, float scale, int dtype, void* stream);
int64_t countr_xattn_bwd_workspace_floats(int B, int N, int S, int D);
/* dk / dv: fp32 [B*S, D]; dk_bf16 / dv_bf16 (optional): bf16 copies of the same sums -- the operands of the wk / wv backward GEMMs */
int countr_xattn_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, float* dk,
                     float* dv, float* workspace, int B, int N, int S, int D, int heads, int ldkv, float scale,
                     int dtype, void* dk_bf16, void* dv_bf16, void* stream);

/* -------- data movement / elementwise */
/* timm PatchEmbed gather (models_mae_cross.py:138): img fp32 NCHW -> patches [B*gh*gw, 3*p*p], k=(c,py,px) */
int countr_im2patch(const float* img, void* out, int B, int H, int W, int patch, int dtype, void* stream);
/* decoder_proj1 conv 3->64 (models_mae_cross.py:48): in fp32 NCHW [S,3,H,W], w fp32 OIHW, out NHWC */
int countr_conv3x3_c3_fwd(const float* in, const float* w, const float* bias, void* out, int S, int H, int W,
                          int dtype, void* stream);
int countr_conv3x3_c3_wgrad_nblocks(void);
/* workspace: fp32 [nblocks][64*28] */
int countr_conv3x3_c3_wgrad(const float* in, const void* dy, float* dw, float* db, float* workspace, int S,
                            int H, int W, int dtype, int accumulate, void* stream);
/* F.interpolate(x2, bilinear, align_corners=False) on NHWC (models_mae_cross.py:189-196); C==1 or C%8==0 */
int countr_upsample2x_fwd(const void* in, void* out, int B, int H, int W, int C, int dtype, void* stream);
int countr_upsample2x_bwd(const void* dout, void* din, int B, int H, int W, int C, int dtype, void* stream);
int countr_gelu_bwd(const void* dh, const void* pre, void* dpre, int64_t n, int dtype, void* stream);
/* bias gradient: out[N] (+)= column sums of x [M,N]; workspace fp32 [countr_colsum_nparts()][N] */
int countr_colsum_nparts(void);
int countr_colsum(const void* x, float* out, float* workspace, int M, int N, int dtype, int accumulate,
                  void* stream);
/* weight shadows: mode 0 cast, 1 OIHW->OHWI, 2 conv-dgrad form Wd[ci][tap'][co] = W[co][ci][T-1-tap'] */
/* up to 8 device-to-device copies in one launch (src / dst / bytes are HOST arrays; 16-byte aligned pointers and sizes): the
 * per-iteration staging of a batch -- `samples.to(device)`, `boxes.to(device)`, `gt_density.to(device)` and the fresh loss mask of
 * FSC_finetune_cross.py:270-296 -- into the static input buffers of a plan.  src[i] == NULL zero-fills dst[i] (the gradients DDP's
 * find_unused_parameters=True, FSC_finetune_cross.py:230, contributes for parameters a rank did not use in an iteration). */
int countr_copy_multi(int n, const void* const* src, void* const* dst, const int64_t* bytes, void* stream);
/* Step prologue (ABI 5): what an optimisation step takes from the host per iteration -- the batch hand-over (samples / gt_density /
 * boxes .to(device): FSC_finetune_cross.py:273-275), the Bernoulli loss mask drawn per iteration (:290-292: np.random.binomial(1, 0.8,
 * [384, 384])) and the iteration's AdamW scalars (lr of lr_sched.adjust_learning_rate :271, bias corrections) -- as ONE launch with
 * FROZEN arguments, so that it can be the first node of the step's captured hipGraph and nothing is launched between two replays.
 * ring: `slots` records of countr_step_prologue_record_bytes() (= 256) bytes in memory the device can read and the host can write
 * (pinned host memory); counter: device int64[34] (16-byte aligned), zero-initialised by the caller, owned by the library afterwards:
 * counter[0] = executions so far, [2..33] = device copy of the current record.  Execution k (eager or replayed) reads record k % slots
 * -- a one-block kernel fetches it from the host and increments counter[0], a wide kernel does the work -- so the host counts
 * executions and fills record k before execution k, not before execution k - slots has finished.  Record layout (little endian): u64 src[6], u64 dst[6], i64 n16[6]
 * (16-byte units; src 0 = zero fill), i32 first[6] (first of the countr_step_prologue_copy_blocks() copy blocks dealt to entry i,
 * ascending, first[0] = 0), i32 n (0..6 copies), i32 draw_mask, u32 key[2], u32 ctr[2], f32 hyper[8], u32 mask_thr, 28 bytes pad.
 * hyper_dev: device fp32[8] <- hyper.  mask (NULL: none), mask_n % 4 == 0: with draw_mask, element 4g + j = (word j of
 * Philox4x32-10(counter = (g, 0, ctr[0], ctr[1]), key) < mask_thr) ? 1 : 0 -- Bernoulli(mask_thr / 2^32), reproducible from (key, ctr). */
int countr_step_prologue_record_bytes(void);
int countr_step_prologue_copy_blocks(void);
int countr_step_prologue(const void* ring, int slots, int64_t* counter, float* hyper_dev, float* mask, int mask_n, void* stream);
int countr_cast_permute(const float* src, void* dst, int64_t n, int mode, int Co, int Ci, int taps, int dtype,
                        void* stream);

/* -------- loss + optimizer (FSC_finetune_cross.py:290-303, :235) */
/* sums (fp32 [1+2B]) = {loss, pred counts[B], gt counts[B]}; dpred optional (= dloss/dpred * grad_scale);
 * workspace: fp32 [countr_masked_mse_workspace_floats(B)].  Deterministic two-stage reduction. */
/* both permuted shadows (OHWI and dgrad form, see countr_cast_permute modes 1 and 2) of up to 32 weights in ONE launch;
 * the arrays are HOST arrays of n device pointers / shapes (the optimiser step refreshes all shadows at once).  wf[i] may be NULL
 * (only wd is written); with taps = 1 a weight is an nn.Linear matrix [co][ci] and wd its TRANSPOSE [ci][co] -- the K-contiguous
 * B operand that turns the input gradient dx = dy W (autograd of models_crossvit.py:62-65, 84-92, 115-127) into a (ROW, ROW) GEMM. */
int countr_conv_shadows(int n, const float* const* src, void* const* wf, void* const* wd, const int* co, const int* ci,
                        const int* taps, int dtype, void* stream);
/* ABI 8: dst[i][c][r] = src[i][r][c] for up to 96 matrices of 16-bit elements (rows, cols multiples of 64; 16-byte aligned) in ONE launch:
 * the W^T shadows (see countr_conv_shadows, taps = 1) taken from the 16-bit shadow W that countr_adamw_step has just written instead of
 * from the fp32 master -- same bits, half the bytes read.  Host arrays of n device pointers / shapes. */
int countr_transpose16(int n, const void* const* src, void* const* dst, const int* rows, const int* cols, void* stream);
int countr_masked_mse_workspace_floats(int B);
int countr_masked_mse(const float* pred, const float* gt, const float* mask, float* dpred, float* sums,
                      float* workspace, int B, int HW, float grad_scale, void* stream);
/* fused AdamW over flat fp32 buffers (torch.optim.AdamW at FSC_finetune_cross.py:235); up to 16 [start,end) ranges each with
 * its weight decay, its bias-correction counter group (groups[i] in {0,1,2}, NULL = all 0: torch keeps a step counter per
 * parameter, util/misc.py:266-280 steps only parameters that have a gradient) and a zero-gradient flag (zero_grad[i] != 0: the
 * range is stepped with g = 0, which is what torch 1.13's zero_grad() -- zero tensors, not None -- makes of a parameter that is
 * unused in this iteration but had a gradient before).  hyper_dev (optional, device fp32[8] = {lr, bc1[0], bc2[0], grad_scale,
 * bc1[1], bc2[1], bc1[2], bc2[2]}, bc = 1 - beta^t of the group) overrides the scalars so a captured graph can be replayed with
 * new values; without it every group uses `step`.  shadow_bf16 (optional) receives bf16(p).  gnorm_ws (optional,
 * countr_adamw_gnorm_floats() floats): gnorm_ws[0] = L2 norm of the (scaled) gradients of the stepped ranges
 * (get_grad_norm_, util/misc.py:289-301). */
/* Dynamic loss scaling of the fp16 mode (ABI 7) = torch.cuda.amp.GradScaler as the reference uses it (util/misc.py:260-286: scale the
 * loss, unscale_, skip the optimizer step on a non-finite gradient, update()), on the device so that a captured step needs no host
 * decision.  amp: device fp32[8] owned by the caller = {scale (GradScaler's initial 65536), steps since the last change, found_inf,
 * skipped steps so far, growth interval (GradScaler's 2000), reserved x 3}.
 *   countr_masked_mse_amp / countr_patch_mse_amp: the loss gradient is multiplied by grad_scale * amp[0];
 *   countr_adamw_step_amp: amp[2] <- any non-finite gradient in the ranges it reads (after an all-reduce every rank sees the same);
 *     if set: parameters, moments and shadows are left untouched, gnorm_ws[0] = inf, scale *= 0.5, amp[3] += 1; otherwise the gradients
 *     are divided by amp[0] on the fly, and after `interval` updates without a skip scale *= 2.  amp == NULL: countr_adamw_step. */
int countr_masked_mse_amp(const float* pred, const float* gt, const float* mask, float* dpred, float* sums,
                          float* workspace, int B, int HW, float grad_scale, const float* amp, void* stream);
int countr_patch_mse_amp(const float* pred, const float* imgs, void* dpred, float* loss, float* workspace, int B, int H, int W,
                         int patch, int norm_pix, float grad_scale, int dpred_dtype, const float* amp, void* stream);
int countr_adamw_step_amp(float* p, const float* g, float* m, float* v, void* shadow_bf16, int nranges,
                          const int64_t* starts, const int64_t* ends, const float* wds, const int* groups,
                          const int* zero_grad, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                          const float* hyper_dev, float* gnorm_ws, float* amp, void* stream);
int countr_adamw_gnorm_floats(void);
int countr_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, int nranges,
                      const int64_t* starts, const int64_t* ends, const float* wds, const int* groups, const int* zero_grad,
                      float lr, float beta1, float beta2, float eps, int step, float grad_scale, const float* hyper_dev,
                      float* gnorm_ws, void* stream);

/* ---- MAE pretraining (reference models_mae_noct.py) ----
 * row gather: dst[r,:] = (idx[r] >= 0 ? src[idx[r],:] : default_row[:]) + add[r % add_mod,:]; idx may be NULL (identity),
 * default_row/add may be NULL, add_mod <= 0 means add[r,:].  cols % 4 == 0; src/dst dtype codes independent.  Covers
 * random_masking's gather of kept tokens (:125-126), the unshuffle with mask tokens + decoder_pos_embed (:166-172) and
 * the backward of both. */
/* index buffers of random_masking (:119-132) from ids_shuffle [B][N] int64 (argsort of the noise): ids_restore [B][N] int64 (its
 * inverse permutation), keep_pos / keep_src [B*K] int32 (kept token = position s, row s + b N of the patch matrix), restore_src
 * [B*N] int32 (row of the kept-token matrix, or -1 = mask token), mask_src [B*(N-K)] int32 (rows of the masked tokens; may be NULL
 * when K == N), mask [B*N] fp32 (1 = masked). */
int countr_mae_indices(const long long* ids_shuffle, long long* ids_restore, int* keep_pos, int* keep_src, int* restore_src,
                       int* mask_src, float* mask, int B, int N, int K, void* stream);
int countr_gather_rows(const void* src, const int* idx, void* dst, const float* default_row, const float* add, int add_mod,
                       int rows, int cols, int src_dtype, int dst_dtype, void* stream);
/* forward_loss (:181-198): target = patchify(imgs) in (py,px,c) order (:84-96), optional norm_pix (unbiased var, eps 1e-6),
 * loss[0] = mean over ALL patches of the per-patch mean squared error; dpred (optional, dtype dpred_dtype) =
 * grad_scale * dloss/dpred.  pred fp32 [B*L, 3*patch^2]; imgs fp32 NCHW; workspace fp32[countr_patch_mse_workspace_floats].
 * Deterministic two-stage reduction (no atomics). */
int countr_patch_mse_workspace_floats(int B, int H, int W, int patch);
int countr_patch_mse(const float* pred, const float* imgs, void* dpred, float* loss, float* workspace, int B, int H, int W,
                     int patch, int norm_pix, float grad_scale, int dpred_dtype, void* stream);

/* ---- sliding-window test path (FSC_test_cross(few-shot).py:326-349, demo_zero.py:49-72): images of height H = 384 are covered by
 * 384-px windows (stride 128, the last snapped to w - 384), every window is one forward, densities are stitched column by column --
 * a column a previous window already covered becomes old / 2 + new / 2, in window order.
 * countr_window_gather: window j (0 <= j < nw <= 64) = columns [starts[j], starts[j] + 384) of the fp32 image frames[j] [3, H, widths[j]]
 *   (frames / widths / starts: HOST arrays, read at call time) -> wins fp32 [nw, 3, H, 384], normally the engine's input batch.
 * countr_window_blend: outs fp32 [n * nwin, H, 384] (image-major: the nwin windows of image 0, then of image 1, ...) of n images of ONE
 *   width W with the window starts starts[nwin] (HOST array, increasing, <= 16) -> dm fp32 [n, H, W]; sums (optional) fp32 [n] = sum
 *   of each stitched map (the predicted count x 60), deterministic two-pass sum through workspace fp32 [n * countr_window_blend_blocks(H, W)].
 * Both equal the reference's tensor slicing / blending bit for bit (x / 2 is exact in fp32). */
#define COUNTR_WINDOW_MAX_STARTS 16 /* window starts of a countr_window_blend call */
int countr_window_gather(const void* const* frames, const int* widths, const int* starts, int nw, int H, float* wins, void* stream);
int countr_window_blend(const float* outs, int n, int nwin, const int* starts, int H, int W, float* dm, float* sums, float* workspace, void* stream);
int countr_window_blend_blocks(int H, int W);

/* ---- the front of the inference path: raw 8-bit RGB frames and pixel boxes -> the tensors the window path above consumes (additive
 * exports, no layout change: the ABI version stays 9).
 * countr_pil_bilinear_tables (HOST only, touches no GPU): the tap tables of Pillow's 8-bit BILINEAR resample of one axis from in_size to
 *   out_size pixels -- what transforms.Resize does to a PIL image (demo_zero.py:23-38, demo.py:42-49).  Returns the tap stride ksize
 *   (= 2 ceil(max(in / out, 1)) + 1) and, unless both pointers are NULL (a query), fills bounds int32 [out_size][2] = {first source
 *   index, tap count} and weights int32 [out_size][ksize] (fixed point, 2^22 = 1.0; entries behind the tap count are 0).  Output pixel =
 *   clamp((2^21 + sum_j src[first + j] * weights[j]) >> 22, 0, 255); Pillow runs the horizontal pass first, into 8 bits, then the vertical.
 * countr_frame_resize_u8: n (1..16) frames of ONE size, uint8 [H, W, 3] interleaved on the device (frames / outs: HOST arrays of n
 *   device pointers, read at call time) -> outs[i] fp32 planar [3, out_h, out_w] = ToTensor(resize(frame)): float(u8) / 255 as a
 *   correctly rounded division, equal to PIL + ToTensor bit for bit.  hbounds / hweights (W -> out_w) and vbounds / vweights
 *   (H -> out_h) are DEVICE copies of the tables above, owned by the caller; tmp: device uint8 [n, H, out_w, 3], the intermediate of
 *   the horizontal pass, caller-owned.  Two launches on `stream` for all n frames.  16-byte loads / stores when the frame and output
 *   pointers are 16-byte aligned and out_w % 4 == 0, element-wise otherwise.  Fails (no launch) when the taps of one output pixel do
 *   not fit the 16-KB row staging (in / out above ~2700 in width).
 * countr_crop_resize_f32: n (1..16) rectangles rects[n][4] = {y1, x1, y2, x2} (HOST array, corners INCLUSIVE, >= 0; clipped to the
 *   image as img[:, y1:y2 + 1, x1:x2 + 1] clips) of the fp32 planar image img [3, h, w] -> out fp32 [n, 3, oh, ow], bilinear,
 *   align_corners=False, no antialias -- F.interpolate(crop, size=(oh, ow), mode="bilinear") with torch's fp32 source coordinates:
 *   the 64 x 64 exemplar crops (demo.py:60-68) and the 3x3 crop-and-upscale for tiny exemplars (:84-99).  A rectangle that is empty
 *   after clipping is an error, not a launch. */
#define COUNTR_FRAMES_MAX 16 /* frames of a countr_frame_resize_u8 call, rectangles of a countr_crop_resize_f32 call */
int countr_pil_bilinear_tables(int in_size, int out_size, int* bounds, int* weights);
int countr_frame_resize_u8(const void* const* frames, void* const* outs, int n, int H, int W, int out_h, int out_w,
                           const int* hbounds, const int* hweights, const int* vbounds, const int* vweights, void* tmp, void* stream);
int countr_crop_resize_f32(const float* img, int h, int w, const int* rects, int n, int oh, int ow, float* out, void* stream);

/* ---- train-time augmentation of the finetuning loader on the device (csrc/augment.hip; additive exports, the ABI version stays 9).
 * The oracle of every call is the named host function of countr_amd/data/fsc147.py (transform_train_aug and its parts).  All images are
 * fp32 planar [3, h, w] on the device; `imgs` is a HOST array of n (1..COUNTR_AUG_MAX_IMAGES) descriptors read at call time, one per
 * image of the batch, sizes free per image; every call is a fixed number of launches on `stream` whatever n is, and allocates nothing.
 * 16-byte accesses where a buffer is 16-byte aligned and h * w (jitter) / w (blur) is a multiple of 4, element-wise otherwise.
 * Each call reads only the descriptor fields named for it. */
#define COUNTR_AUG_MAX_IMAGES 32
typedef struct countr_aug_image {
  const float* src;      /* the clean resized frame (countr_frame_resize_u8): input of the jitter, source of the exemplars */
  float* jit;            /* output of countr_aug_jitter, input of countr_aug_blur */
  float* blr;            /* output of countr_aug_blur (a buffer of its own) */
  const float* noise;    /* noise_mode 2: an explicit noise image [3, h, w], added as it is (already scaled by 0.1) */
  const float* win;      /* input of countr_aug_window, [3, win_h, win_w] */
  uint64_t counter;      /* noise_mode 1: this image's noise counter */
  double brightness, contrast, saturation, hue;   /* color_jitter's factors (hue: the shift); rounded to fp32 as torch rounds a Python float */
  double affine[6];      /* win_mode 1: output pixel (y, x) of the warp samples (row, col) = (affine[2] + y affine[0] + x affine[1],
                            affine[5] + y affine[3] + x affine[4]) -- matrix rows and offset as warp_affine hands them to scipy */
  float kx[7], ky[9];    /* normalised blur weights along x and y (gaussian_blur's k1d) */
  int h, w;              /* size of src / jit / blr */
  int win_h, win_w;      /* size of win */
  int nops, order[4];    /* the first nops (0..4) entries of order run: 0 brightness, 1 contrast, 2 saturation, 3 hue, each at most once */
  int noise_mode;        /* 0 none, 1 generator, 2 explicit */
  int win_mode;          /* 0 copy, 1 affine warp (bilinear, zero outside) */
  int flip;              /* != 0: the window is cut from the horizontally flipped image */
  int start_h, start_w;  /* first row / column of the 384 x 384 window */
  int rects[12];         /* three exemplar rectangles {y1, x1, y2, x2} of src, corners inclusive (countr_crop_resize_f32's convention) */
  int cell_off, cell_cnt;/* this image's range of the cell list of countr_aug_density */
} countr_aug_image;
/* The normal stream.  Element e of stream (seed, counter): g = e / 4, j = e % 4, (r0, r1, r2, r3) = Philox4x32-10(counter = (g, 1,
 * counter lo, counter hi), key = (seed lo, seed hi)) -- counter word 1 is 1 where the loss mask of countr_step_prologue uses 0, so the
 * two stay disjoint under one seed.  Box-Muller in fp32 on (a, b) = (r0, r1) for j = 0, 1 and (r2, r3) for j = 2, 3:
 * u1 = ((a >> 9) + 1) 2^-23 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1) (both exact), rad = sqrtf(-2 logf(u1)),
 * z = rad * cos(2 pi u2) for even j, rad * sin(2 pi u2) for odd j (sincospif(2 u2)).
 * countr_aug_normal: out[e] = scale * z[e] for e < n.  An image's noise is 0.1f * z[e], e its index in the flattened [3, h, w]. */
int countr_aug_normal(float* out, int64_t n, float scale, uint64_t seed, uint64_t counter, void* stream);
/* countr_aug_jitter: jit <- color_jitter(clamp(src + noise, 0, 1), order[:nops], ...) (noise_mode 0: no noise, no clamp).  _blend clamps
 * after every op; the contrast op blends with the mean of _gray over the whole image at that point of the chain: launch 1 runs the noise
 * and the ops in front of it and leaves 128 partial sums per image in `partials` (fp32 [countr_aug_partials_floats(n)]), launch 2 adds
 * them in one fixed order and runs the rest in place (skipped when no image has a contrast op).  Bit-reproducible. */
int countr_aug_partials_floats(int n);
int countr_aug_jitter(const countr_aug_image* imgs, int n, uint64_t seed, float* partials, void* stream);
/* countr_aug_blur: blr <- gaussian_blur(jit, (7, 9), sigma) with the caller's weights: 7 taps along x, then 9 along y, reflect padding
 * that does not repeat the edge pixel.  One launch. */
int countr_aug_blur(const countr_aug_image* imgs, int n, void* stream);
/* countr_aug_window: out [n, 3, 384, 384] (16-byte aligned) <- rows start_h.., columns start_w.. of win (win_mode 0), or of
 * warp_affine(win) = scipy.ndimage.affine_transform(order=1, mode="constant", cval=0) (win_mode 1), flipped left-right first when flip
 * is set.  The source coordinate is computed in double as scipy does; a coordinate strictly outside [0, size - 1] on either axis
 * gives 0.  The window must lie inside win_h x win_w.  One launch; the full warp is never stored. */
int countr_aug_window(const countr_aug_image* imgs, int n, float* out, void* stream);
/* countr_aug_density: out [n, 384, 384] (16-byte aligned) <- 60 * scipy.ndimage.gaussian_filter(dot map, sigma=(1, 1)) where the dot
 * map of image i is 1 at the cells cells[cell_off .. cell_off + cell_cnt) and 0 elsewhere; a cell is (row << 16) | col, row and col
 * < 384 (others are ignored), duplicates allowed.  cells: DEVICE int32 [ncells].  Radius 4, weights exp(-x^2 / 2) normalised in
 * double, mode "reflect" (the edge sample repeats), axis 0 into an fp32 intermediate, then axis 1.  One launch. */
int countr_aug_density(const countr_aug_image* imgs, int n, const int* cells, int ncells, float* out, void* stream);
/* countr_aug_exemplars: out [n, 3, 3, 64, 64] (16-byte aligned) <- the three rectangles of every src, each resized as
 * countr_crop_resize_f32 resizes it (same formula; fp contraction off here, on there), in one launch for the batch. */
int countr_aug_exemplars(const countr_aug_image* imgs, int n, float* out, void* stream);

/* ---- the mosaic branch of that augmentation on the device (csrc/mosaic.hip; an additive export with a descriptor of its own:
 * countr_aug_image keeps its layout and the ABI version stays 9).  The oracle is fsc147.mosaic() with _blend_pair: piece k is the
 * length x length crop at (start_h, start_w) of a clean resized frame, resized to resize_l x resize_l, resize_l = 192 + 2 bl, as
 * F.interpolate(mode="bilinear", align_corners=False) resizes it (countr_crop_resize_f32's formula, contraction off).  Pieces 0 / 1 are joined along
 * the rows into the left half and 2 / 3 into the right half, the two halves along the columns: the 192-line cores are put side by side,
 * then line 192 + i takes weight (i + bl) / (2 bl) and the first piece's line resize_l - 1 - bl + i the weight (bl - i) / (2 bl), line
 * 191 - i mixes with the second piece's line bl - i in the same way, i < bl (index_select's own lines: the asymmetry is the
 * reference's); each join ends with a clamp to [0, 1].  Products and sums are rounded one by one, as torch rounds them. */
typedef struct countr_mosaic_piece {
  const float* src;      /* a clean resized frame, fp32 planar [3, h, w] on the device (countr_frame_resize_u8) */
  int h, w;              /* its size */
  int start_h, start_w;  /* first row / column of the crop */
  int length;            /* the crop's edge, 1..min(h, w); start + length lies inside the frame */
} countr_mosaic_piece;
typedef struct countr_mosaic_image {
  countr_mosaic_piece piece[4];   /* quadrants 0 top left, 1 bottom left, 2 top right, 3 bottom right; pieces may share a frame */
  int bl;                /* half width of the cross-fade, 10..20 */
  int row;               /* the row of `out` this image is written to, 0..out_rows - 1 */
} countr_mosaic_image;
/* countr_aug_mosaic: out[imgs[i].row] [3, 384, 384] <- the mosaic of imgs[i], i < n (1..COUNTR_AUG_MAX_IMAGES; a HOST array read at call
 * time).  out: the batch tensor [out_rows, 3, 384, 384], 16-byte aligned; rows no descriptor names are left as they are.  One launch on
 * `stream`, nothing allocated; the resized pieces and the halves are never stored: a pixel evaluates the one, two or four piece samples
 * it depends on.  Bit-reproducible.  Every argument is checked before anything touches the GPU. */
int countr_aug_mosaic(const countr_mosaic_image* imgs, int n, float* out, int out_rows, void* stream);

/* ---- the pretraining loader's transform on the device (csrc/pretrain_aug.hip; additive exports, the ABI version stays 9).  The oracle
 * is fsc147.transform_pretrain: Pillow BILINEAR resize of the frame to multiples of 16 (H16 = 16 (H / 16), W16 likewise), crop, Pillow
 * BICUBIC resize of the crop to 384 x 384, horizontal flip, ToTensor -- reproduced bit for bit.
 * countr_pil_tables (HOST only, touches no GPU): countr_pil_bilinear_tables for both filters, same query form and layout.  filter 0 is
 *   BILINEAR (equal to countr_pil_bilinear_tables), filter 1 is BICUBIC: a = -0.5, support 2 max(in / out, 1), tap stride
 *   2 ceil(support) + 1, negative weights rounded as int(-0.5 + w 2^22).  The sum of a pixel can be negative: shift arithmetically, then
 *   clamp. */
int countr_pil_tables(int filter, int in_size, int out_size, int* bounds, int* weights);
#define COUNTR_PRETRAIN_MAX_IMAGES 16
typedef struct countr_pretrain_image {
  const void* frame;     /* the decoded frame, uint8 [H, W, 3] interleaved on the device (16-byte loads when 16-byte aligned) */
  int H, W;              /* its size, each >= 16 */
  int i, j, ch, cw;      /* the crop: first row, first column, height, width, in the coordinates of the H16 x W16 frame */
  int flip;              /* != 0: the output is mirrored left-right */
  int row;               /* the row of the batch tensor this sample is written to */
} countr_pretrain_image;
/* All three take a HOST array of n (1..COUNTR_PRETRAIN_MAX_IMAGES) descriptors read at call time, sizes free per sample, and check every
 * argument before anything touches the GPU.
 * countr_pretrain_aug_layout (HOST only): sizes[0] = the group's tap stride (the largest ksize of its 4 n axes), sizes[1] = ints of the
 *   table workspace, sizes[2] = bytes of the image workspace, sizes[3 + 4 s + a] = first int of the table of sample s, axis a (0: W -> W16
 *   and 1: H -> H16, bilinear; 2: cw -> 384 and 3: ch -> 384, bicubic) in the table workspace: bounds int32 [out][2], then weights int32
 *   [out][stride], as countr_pil_tables lays them out but with the group's stride (zeros behind an axis' own ksize).  sizes holds
 *   3 + 4 n entries.
 * countr_pretrain_aug_tables: fills the table workspace (DEVICE int32 [sizes[1]]) in one launch, one thread per (sample, axis, output
 *   index), in fp64 with Pillow's operation order and without fused multiply-adds: equal to countr_pil_tables bit for bit.
 * countr_pretrain_aug: out[imgs[s].row] [3, 384, 384] <- the transform of sample s; out is the batch tensor [out_rows, 3, 384, 384], fp32,
 *   16-byte aligned; workspace: DEVICE bytes [sizes[2]], 16-byte aligned.  Four launches on `stream` whatever n and the sizes are: the
 *   stage-1 horizontal and vertical pass (each into 8 bits; a pass whose sizes are equal is skipped and its successor reads its input),
 *   the bicubic horizontal pass over the crop rectangle (taps relative to the crop: the filter clamps at the crop's edges), the bicubic
 *   vertical pass + flip + float(u8) / 255 with a 16-byte store per plane.  int32 accumulators as Pillow's.  Table entries are clamped
 *   to the rectangle they index, so a wrong table cannot read outside a frame.  Nothing is allocated. */
int countr_pretrain_aug_layout(const countr_pretrain_image* imgs, int n, int64_t* sizes);
int countr_pretrain_aug_tables(const countr_pretrain_image* imgs, int n, int* tables, void* stream);
int countr_pretrain_aug(const countr_pretrain_image* imgs, int n, const int* tables, void* workspace, float* out, int out_rows, void* stream);

/* ---- the CARPK scripts' own preparation and count rule (csrc/carpk.hip; additive exports, the ABI version stays 9).
 * countr_carpk_prep_u8: n (1..16) uint8 [H, W, 3] frames on the device (frames: HOST array of n device pointers; shapes: HOST int
 *   [n][2] = {H, W}, free per frame) -> img fp32 [n, 3, out_h, out_cols] = F.interpolate(frame / 255, (out_h, out_w), bilinear,
 *   align_corners=False)[..., :out_cols], what torchvision 0.14.1's Resize does to a TENSOR (FSC_test_CARPK.py:154, :191: no antialias,
 *   not Pillow's resample), 1 <= out_cols <= out_w: only the columns that are kept are computed (FSC_finetune_CARPK.py:225-226 crops
 *   the left 384 after the resize); and the nrects (0..32) rectangles rects[nrects][5] = {frame, y1, x1, y2, x2} (HOST array, corners
 *   INCLUSIVE and >= 0, in pixels of the ORIGINAL frame; clipped as frame[y1:y2 + 1, x1:x2 + 1] clips; empty after clipping = error)
 *   -> ex fp32 [nrects, 3, 64, 64], the same interpolation of the rectangle / 255 (:166-171).  Source coordinates as torch computes
 *   them: scale = in / out in fp32, src = scale * (dst + 0.5) - 0.5 clamped at 0.  ONE launch; 16-byte stores when out_cols % 4 == 0 and
 *   img / ex are 16-byte aligned, one pixel per thread otherwise (out_w = 683).  ex may be NULL when nrects == 0.
 * countr_carpk_count: the count rule of FSC_test_CARPK.py:220-243 on n (1..16) stitched maps fp32 [n, H, W] with two rectangles per map,
 *   rects[n][2][4] = (a, b, c, d) (HOST array, >= 0) -> out fp32 [n][4] = {pred, total, n_over, e_cnt}:
 *     cell = sum of a 16 x 16 block / 60 over floor(H / 16) x floor(W / 16) blocks (trailing rows / columns dropped, as the stride-16
 *     convolution drops them); total = sum of the cells; n_over = cells > 1.224;
 *     e_cnt = (sum over both rectangles of sum(map[a : a + c + 1, b : b + d + 1]) / 60) / 2, slices clipped to the map, empty = 0 (which
 *     rectangles the script's line :238 really cuts is the caller's business: countr_amd/data/carpk.py::script_rects); pred = total - n_over + (e_cnt <= 0.5 ? 2 : 0).
 *   Two launches (partials, fold) through workspace fp32 [n * countr_carpk_count_blocks(H, W) * 4]; every sum has a fixed order, no
 *   atomics: two runs give the same bits. */
#define COUNTR_CARPK_MAX_FRAMES 16 /* frames / maps of a call; countr_carpk_prep_u8 takes two rectangles per frame */
int countr_carpk_prep_u8(const void* const* frames, const int* shapes, int n, const int* rects, int nrects, int out_h, int out_w,
                         int out_cols, float* img, float* ex, void* stream);
int countr_carpk_count_blocks(int H, int W);
int countr_carpk_count(const float* maps, int n, int H, int W, const int* rects, float* out, float* workspace, void* stream);

/* ---- the evaluation report of FSC_test_cross(few-shot).py:379-425 (csrc/report.hip; additive exports, the ABI version stays 9).
 * countr_report_panels: the `full_*.png` picture of n (1..COUNTR_REPORT_MAX_IMAGES) images of one height h, widths free per image, in ONE
 *   launch: image i's panel uint8 [h, P w, 3] (HWC, what PIL encodes) at out + imgs[i].out_off, P = imgs[i].layout.  Per pixel, in fp32,
 *   every product and sum rounded on its own, in the script's operation order (s = the sample's channel, p = pred, g = gt):
 *     pred_img = (p, p, 0), gt_img = (g, 0, 0), fp = pred_img where gt_img - pred_img < -0.01, else 0
 *     tp_img  = s 0.6 + (pred_img - fp)[[1, 0, 2]]                (not clamped)
 *     mix2    = s 0.6 + |clamp01(pred_img) - clamp01(gt_img)|
 *     sam_box = clamp01(s + box + labels)                          (box, labels: 0..255 as the script adds them, NOT scaled)
 *     den_pr  = clamp01(s 0.6 + text + pred_img)
 *   layout 3 (gt_cnt != 0): [mix2 | sam_box | tp_img]; layout 2 (gt_cnt == 0): [sam_box without labels | den_pr].
 *   Every value is quantised as torchvision's save_image does: x 255 + 0.5, clamped to [0, 255], truncated.
 *   box: 255 on the outline of every rectangle of the image (cv2.rectangle, thickness 1: y in {y1, y2}, x1 <= x <= x2 or x in {x1, x2},
 *   y1 <= y <= y2, clipped to the image; corners in either order), rectangles rects[rect_off .. rect_off + rect_cnt) of the blob.
 *   pred: the stitched map, or (grid != 0) the nine maps of the 3 x 3 path tiled row-major in list order and resized [3 h, 3 w] -> [h, w]
 *   with bilinear, align_corners=False, no antialias: the source coordinate is 3 d + 1 with weight 1 on one tap, so
 *   pred[y, x] = maps[3 (Y / h) + X / w][Y % h, X % w] at Y = 3 y + 1, X = 3 x + 1, exactly.
 *   labels / text: a uint8 [ph, pw, 3] raster of the blob whose top-left pixel lies at (px, py) of the image; it may hang over any edge
 *   (only the pixels inside the image are read), pw = 0: none.  layout 3 reads `labels`, layout 2 reads `text`.
 *   blob: ONE device buffer the caller uploads per group: int32 rectangles {y1, x1, y2, x2} at byte rects_off, patch rasters at their
 *   `off`.  imgs is a HOST array read at call time; every offset is checked against blob_bytes / out_bytes, panels must not overlap, and
 *   nothing is launched when a check fails.  16-byte loads and 4-byte stores when w % 4 == 0 and the image's buffers are aligned, one pixel
 *   at a time otherwise.  Nothing is allocated.
 * countr_report_quantize: the `boxes_*.png` picture of n (1..16) exemplar sets: strips[i].ex fp32 [S, 3, eh, ew] -> uint8 [GH, GW, 3] at
 *   out + strips[i].out_off = save_image's grid (torchvision make_grid: 8 per row, padding 2, pad value 0; S = 1 is the exemplar itself,
 *   no padding), quantised as above.  countr_report_strip_shape gives {GH, GW}.  ONE launch. */
#define COUNTR_REPORT_MAX_IMAGES 16
typedef struct countr_report_patch {
  int64_t off;           /* first byte of the raster in the blob */
  int px, py, pw, ph;    /* position of its top-left pixel in the image, and its size (pw = 0 or ph = 0: no raster) */
} countr_report_patch;
typedef struct countr_report_image {
  const float* sam;      /* the sample, fp32 [3, h, w] */
  const float* maps[9];  /* maps[0]: the stitched map fp32 [h, w]; grid != 0: the nine maps of the 3 x 3 path */
  const float* gt;       /* the ground-truth map, fp32 [h, w] */
  int64_t out_off;       /* first byte of the panel in out */
  int w, layout, grid;   /* width, 3 or 2 panels, 3 x 3 path */
  int rect_off, rect_cnt;
  countr_report_patch labels, text;
} countr_report_image;
typedef struct countr_report_strip {
  const float* ex;       /* fp32 [S, 3, eh, ew] */
  int64_t out_off;
  int S;
} countr_report_strip;
int countr_report_panels(const countr_report_image* imgs, int n, int h, const void* blob, int64_t blob_bytes, int64_t rects_off,
                         int nrects, void* out, int64_t out_bytes, void* stream);
int countr_report_strip_shape(int S, int eh, int ew, int* shape);
int countr_report_quantize(const countr_report_strip* strips, int n, int eh, int ew, void* out, int64_t out_bytes, void* stream);

/* ---- object locations from density maps (csrc/peaks.hip; additive exports, the ABI version stays 9).
 * countr_density_peaks: the peaks of n (1..16) maps, maps[i].map fp32 [h, w] on the device, contiguous, any h, w >= 1 with h w <= 2^28,
 *   sizes free per map, no alignment requirement beyond the float's (16-byte loads in the maximum pass when a map's base is 16-byte
 *   aligned, element loads otherwise).  maps is a HOST array read at call time.  radius is 1..8, cap 1..8192, threshold >= 0 and
 *   0 <= rel_threshold <= 1; anything else is an error and nothing is launched.
 *   The rule, which is the specification:
 *     Let m be the maximum of the map.  A NaN never wins.
 *     Let idx(p) = y*w + x.
 *     Let win(p) be the (2r+1)^2 window around p, clipped to the map.
 *     Pixel p with value v is a peak iff all three hold:
 *       v > threshold
 *       v >= rel_threshold * m, where the product is one fp32 multiply
 *       for every q != p in win(p): v > d(q), or v == d(q) and idx(p) < idx(q)
 *     Consequences: a plateau yields exactly one peak, its first pixel in raster order, unless something higher is in reach; an all-zero
 *     map yields none; a NaN is never a peak (and neither is a pixel with a NaN inside its window).
 *   Per peak, with w(q) = max(d(q), 0) over win(p), accumulated in fp32 (64 lanes, then a fixed butterfly):
 *     score = v, mass = sum(w) / 60, cy = y + sum(w (qy - y)) / sum(w), cx likewise (offsets relative to the peak: magnitudes <= 8).
 *   Output: totals[i] = the true number of peaks of map i, even beyond cap; recs[i][k][6] = {y, x, score, cy, cx, mass} (fp32) for
 *   k < min(totals[i], cap): when totals[i] > cap the kept peaks are the first cap in raster order; the kept peaks are ordered by
 *   (score descending, idx ascending).  Entries behind the kept ones are left untouched.
 *   Four launches whatever n is (block maxima; tile detection with an r-wide halo in LDS, one 64-bit ballot mask per 64-pixel row segment;
 *   popcount scan + raster-order records; rank by counting).  No atomic decides an order or a sum: two runs give the same bytes.
 *   Nothing is allocated and the host never waits: all scratch lives in workspace (8-byte aligned, >= countr_peaks_workspace(n, max_h,
 *   max_w, cap) bytes for maps no taller than max_h and no wider than max_w; HOST only, < 0 on bad arguments). */
#define COUNTR_PEAKS_MAX_MAPS 16
#define COUNTR_PEAKS_MAX_RADIUS 8
#define COUNTR_PEAKS_MAX_POINTS 8192 /* the largest cap */
typedef struct countr_peak_map {
  const float* map;      /* fp32 [h, w], contiguous */
  int h, w;
} countr_peak_map;
int countr_peaks_workspace(int n, int max_h, int max_w, int cap);
int countr_density_peaks(const countr_peak_map* maps, int n, int radius, float threshold, float rel_threshold, int cap, int* totals,
                         float* recs, void* workspace, void* stream);

/* ---- predicted points against annotated dots (csrc/match.hip; additive exports, the ABI version stays 9).
 * countr_match_points: the one-to-one matching of n (1..16) sets.  sets is a HOST array read at call time; set s holds pred fp32 [P, 2]
 *   and gt fp32 [G, 2] on the device, both as (x, y) pairs, 8-byte aligned, P and G 0..8192 each (a pointer may be null when its count
 *   is 0), max_dist finite and > 0, and offset >= 0, the first element of the set's slice in match / match_d2.  Anything else is an
 *   error and nothing is launched.
 *   The rule, which is the specification:
 *     d2(i, j) = fl(fl(dx*dx) + fl(dy*dy)) with dx = fl(px_i - gx_j), dy = fl(py_i - gy_j): fp32, nothing contracted.
 *     Pair (i, j) is eligible iff d2(i, j) <= fl(max_dist * max_dist) (one fp32 multiply).  A point with a non-finite coordinate
 *     therefore has no eligible pair.
 *     The eligible pairs are totally ordered by the key (d2, i, j).
 *     The matching is the greedy one: go through the pairs in ascending key order and match (i, j) when both are still free.
 *   Two properties follow.  (1) The matching is the fixed point of rounds in which every pair that is the smallest remaining key of both
 *   its pred and its gt is matched -- this is how the kernel computes it, exactly.  (2) The matching under a smaller max_dist is the
 *   subset of this one whose d2 is within the smaller bound, so one call at the largest distance gives the matches of every smaller one.
 *   Letting each pred propose to its best gt and each gt take its best proposer is NOT this rule: a gt's best is taken over all its
 *   remaining eligible pairs.
 *   Output: match[offset + i] = the gt index of pred i or -1, match_d2[offset + i] = the pair's d2 or +inf, for i < P; counts[s] = the
 *   number of matched pairs of set s.  Entries outside the slices are left untouched.
 *   Two launches whatever the sets hold (every point's best partner over all CUs; then a block per set that runs the rounds until one
 *   matches nothing -- no round count is assumed).  Minima, atomic AND on bit masks and one integer atomic add: nothing depends on an
 *   order, two runs give the same bytes.  Nothing is allocated and the host never waits: all scratch lives in workspace (16-byte
 *   aligned, >= countr_match_workspace(n, max_p, max_g) bytes for sets of at most max_p preds and max_g gts; HOST only, < 0 on bad
 *   arguments). */
#define COUNTR_MATCH_MAX_SETS 16
#define COUNTR_MATCH_MAX_POINTS 8192 /* of P and of G */
typedef struct countr_match_set {
  const float* pred;     /* fp32 [P, 2] as (x, y) */
  const float* gt;       /* fp32 [G, 2] as (x, y) */
  int P, G;
  float max_dist;
  int offset;            /* of the set's slice in match / match_d2, in elements */
} countr_match_set;
int countr_match_workspace(int n, int max_p, int max_g);
int countr_match_points(const countr_match_set* sets, int n, int* match, float* match_d2, int* counts, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_H */
