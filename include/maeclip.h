/* libmaeclip -- C-ABI of the MI355X (gfx950) kernels behind the mae_clip hot path.
 *
 * The reference (ykojima4020/mae_clip) has no FFI: its boundary is the PyTorch
 * nn.Module API of modules.ImageEncoder / TextEncoder / ProjectionHead
 * (modules.py:8-76) and CLIP.CLIPModel (CLIP.py:9-52), which calls into
 * timm / HF transformers / torch ops. Each entry point below replaces the op
 * those modules dispatch (cited per function); the Python package
 * mae_clip_amd binds them with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is device memory unless noted;
 *     bf16 tensors are uint16 bit patterns; strides are in elements.
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream).
 *   - no entry point allocates, frees or synchronises (graph-capture safe);
 *     workspaces are provided by the caller.
 *   - return 0 on success, <0 on error; maeclip_last_error() gives the
 *     message (thread-local).
 */
#ifndef MAECLIP_H
#define MAECLIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAECLIP_ABI_VERSION 14
#ifndef MAECLIP_F32
#define MAECLIP_F32 0
#define MAECLIP_BF16 1
#endif
#define MAECLIP_FP8_E4M3 2   /* OCP float8 e4m3fn (gfx950), max 448 */
#define MAECLIP_FP8_E5M2 3   /* OCP float8 e5m2, max 57344 */

int32_t maeclip_abi_version(void);
const char* maeclip_last_error(void);
/* number of gfx950 devices visible (0 when no GPU); does not create a context */
int32_t maeclip_device_count(void);

/* Plan options (A/B and test knobs of the kernels' launch planning). The
 * library reads every MAECLIP_<name> environment variable ONCE, at the first
 * call of any entry point below, into this table; launches read the table,
 * never the environment. maeclip_set_option overrides one entry (value -1 =
 * the built-in default). Defaults are the measured-fastest plans; no option
 * changes results beyond the bf16 rounding of a different tile / split.
 *   GEMM_BM          force a tile height of plain GEMMs (256 / 192 / 128; 0 auto)
 *   GEMM_SK          1: the cost model may pick the aligned split plan (0 off)
 *   GEMM_SPLIT       force a split of S slices (192-row tiles) where it fits
 *   GEMM_SPLIT_D     slice 0's lead in K-tiles per other slice (default 4)
 *   GEMM_SPLIT_MINK  the cost model's split only at K >= this (default 0)
 *   GEMM_BM128       1: 128-row tiles enter the cost model (default 0)
 *   GEMM_GRID        cap of the persistent GEMM grid (diagnostic; 0 = #CUs)
 *   WG_SK            0: grouped weight gradients use uniform split-K slices
 *                    instead of the stream-K remainder (default 1)
 *   ATTN_TWO         bf16 attention backward layout: 0 four images, 1 two, 3
 *                    two at 3 workgroups / CU (hd 32); -1 by occupancy
 *   ATTN_ROWS        1: fp32 attention on the streaming rows path
 *   ATTN_DIAG        diagonal backward (hd 32 on, hd 64 at npad >= 192); 0 / 1
 *   ATTN_BW16        16-wave backward beyond MAXW tiles (default hd 32); 0 / 1
 *   ATTN_FW16        16-wave forward when LDS leaves one workgroup (default 1)
 *   ATTN_STREAM      bf16 streamed attention kernels (LDS footprint independent
 *                    of n): -1 where the resident images do not fit, 1 at
 *                    every n, 0 never (such shapes are rejected) */
enum {
  MAECLIP_OPT_GEMM_BM = 0,
  MAECLIP_OPT_GEMM_SK = 1,
  MAECLIP_OPT_GEMM_SPLIT = 2,
  MAECLIP_OPT_GEMM_SPLIT_D = 3,
  MAECLIP_OPT_GEMM_SPLIT_MINK = 4,
  MAECLIP_OPT_GEMM_BM128 = 5,
  MAECLIP_OPT_GEMM_GRID = 6,
  MAECLIP_OPT_WG_SK = 7,
  MAECLIP_OPT_ATTN_TWO = 8,
  MAECLIP_OPT_ATTN_ROWS = 9,
  MAECLIP_OPT_ATTN_DIAG = 10,
  MAECLIP_OPT_ATTN_BW16 = 11,
  MAECLIP_OPT_ATTN_FW16 = 12,
  MAECLIP_OPT_ATTN_STREAM = 13,
  MAECLIP_OPT_COUNT = 14
};
/* returns the previous value, or INT32_MIN for an unknown key */
int32_t maeclip_set_option(int32_t key, int32_t value);
/* current value (-1: default), INT32_MIN for an unknown key */
int32_t maeclip_get_option(int32_t key);

/* ------------------------------------------------------------------ GEMM
 * Replaces torch.nn.functional.linear (cuBLAS) for every nn.Linear on the
 * hot path (timm Block qkv/proj/fc1/fc2, PatchEmbed conv-as-GEMM,
 * modules.py:64-66 ProjectionHead, DistilBERT q/k/v/out/lin1/lin2, HF ViTMAE
 * decoder_embed/decoder_pred) in forward, dgrad and wgrad form, and the
 * N x N x P products of the CLIP loss (CLIP.py:34-38).
 *   C[z][m][n] = alpha * sum_k A(m,k) B(k,n) (+bias[n]) (epilogue) (+beta*C)
 * layouts: 0 = K-contiguous (A[m*lda+k], B[n*ldb+k]); 1 = row-contiguous
 * (A[k*lda+m], B[k*ldb+n]).
 * epilogue: 0 none; 1 GELU (aux_out <- pre-activation, C <- gelu(pre));
 *           2 residual (C(f32) <- resid + acc (+bias)); 3 dGELU (C <- acc *
 *           gelu'(aux) (+ resid if resid != NULL)); 4 GELU' (C <- gelu(pre),
 *           aux_out <- gelu'(pre): the backward then needs no transcendental);
 *           5 mul-aux (C <- acc * aux (+ resid if resid != NULL)).
 *           For 1 and 4 aux_out may be NULL (forward-only callers). Any
 *           other epilogue value is rejected.
 *           aux / aux_out have the operand dtype on the fp32 path, bf16 on the
 *           bf16 path.
 * batch > 1: A, B and C of batch z start z * strideA / strideB / strideC
 *   elements after the pointers (a stride of 0 shares the operand). aux,
 *   aux_out and resid have no stride of their own: batch z reads / writes them
 *   z * strideC elements after their pointers, rows ldaux / ldr apart, so a
 *   batched epilogue lays them out like C (ldaux = ldr = ldc). bias is shared
 *   by the batch; colsum_partial takes maeclip_gemm_colsum_rows(M) rows per
 *   batch.
 * colsum_partial (optional, f32 [batch*maeclip_gemm_colsum_rows(M)][N]):
 *   per-block column sums of the final C, reduce with maeclip_colsum_reduce.
 * splitk > 1 (epilogue 0, no colsum): K is cut into splitk slices whose fp32
 *   partial tiles go to workspace [batch][splitk][M][N]; a second launch sums
 *   them in fixed order (+bias, +beta*C) -> deterministic. Use
 *   maeclip_gemm_splitk(M,N,K) for the slice count. */
typedef struct {
  const void* A;
  const void* B;
  void* C;
  int64_t M, N, K;
  int64_t lda, ldb, ldc;
  int64_t batch, strideA, strideB, strideC;
  int32_t dtype;     /* MAECLIP_F32 = 0 / MAECLIP_BF16 = 1 (A, B, aux) */
  int32_t out_dtype; /* C */
  int32_t a_layout, b_layout;
  int32_t epilogue;
  float alpha, beta;
  const float* bias;
  const void* aux;
  void* aux_out;
  int64_t ldaux;
  const float* resid;
  int64_t ldr;
  float* colsum_partial;
  int32_t splitk;
  float* workspace;
  /* optional fp8-blocks copy of the output (bf16 C only, N % 128 == 0): q8
   * [M, ldq8] bytes of format q8_fmt and e8m0 block scales q8_scale
   * (maeclip_fp8b_scale_bytes(M, N) bytes), the quantisation of the bf16 C as
   * stored (bit-identical to maeclip_quant_blocks_fp8 of C): the next fp8
   * GEMM's A operand without a separate pass */
  void* q8;
  int64_t ldq8;
  uint8_t* q8_scale;
  int32_t q8_fmt;
} maeclip_gemm_args;
int32_t maeclip_gemm(const maeclip_gemm_args* args, void* stream);
/* fp8 GEMM (C4 path; replaces the nn.Linear matmuls of the timm / ViTMAE
 * blocks, modules.py:17-19, when precision = "fp8"). A [M, lda] and B [N, ldb]
 * are OCP fp8 bytes, both KC (K contiguous, K % 128 == 0, lda, ldb % 16 == 0);
 * args->dtype is A's format (MAECLIP_FP8_E4M3 / _E5M2), B is e4m3. The
 * block-scaled 16x16x128 MFMA accumulates in fp32 and the epilogue applies
 * scale_a[m] * scale_b[n] * alpha before bias / epilogue (args->epilogue as
 * maeclip_gemm; no split-K, beta must be 0). M, N >= 256, N % 8 == 0. */
int32_t maeclip_gemm_fp8(const maeclip_gemm_args* args, const float* scale_a, const float* scale_b, void* stream);
/* fp8 BLOCKS (the MX layout of the block-scaled MFMA): a row of K elements is
 * cut into K / 32 blocks, each quantised with its own power-of-two scale
 * 2^(e - 127), e an e8m0 byte: e = the smallest exponent with amax(block) /
 * 2^(e - 127) <= FMT_MAX, q = rne(x * 2^(127 - e)); x ~= q * 2^(e - 127). A
 * producer that owns only part of a row (a GEMM epilogue tile, an attention
 * head) can quantise it without the whole-row amax a per-row scale needs.
 * Scale bytes are laid out for the GEMM's reads (K % 128 == 0):
 *   byte (r, b) at (((r / 64) * (K / 128) + b / 4) * 256 + (b % 4) * 64 +
 *                   (r % 16) * 4 + (r / 16) % 4)
 * maeclip_fp8b_scale_bytes(rows, K) = ceil(rows / 64) * 64 * K / 32. */
int64_t maeclip_fp8b_scale_bytes(int64_t rows, int64_t K);
/* x (bf16 / f32 [rows, ld]) -> fp8 blocks q [rows, ldq] + scales (cols % 128 == 0) */
int32_t maeclip_quant_blocks_fp8(const void* x, int32_t x_dtype, int64_t rows, int64_t cols, int64_t ld, void* q,
                                 int64_t ldq, uint8_t* scales, int32_t fmt, void* stream);
/* fp8 GEMM with an fp8-blocks A operand: as maeclip_gemm_fp8, the A block
 * scales (e8m0, the layout above, K = args->K) applied by the MFMA itself,
 * B (e4m3) scaled per column by scale_b in the epilogue. */
int32_t maeclip_gemm_fp8_blocks(const maeclip_gemm_args* args, const uint8_t* scale_a, const float* scale_b,
                                void* stream);
/* Row-wise fp8 quantisation: q[r, :] = rne(x[r, :] / s[r]), s[r] = amax(x[r, :]) /
 * FMT_MAX (1 when the row is zero). x bf16 or f32 [rows, ld]; q [rows, ldq]
 * bytes; fmt MAECLIP_FP8_E4M3 (activations, weights) or _E5M2 (gradients). */
int32_t maeclip_quant_rows_fp8(const void* x, int32_t x_dtype, int64_t rows, int64_t cols, int64_t ld, void* q,
                               int64_t ldq, float* scales, int32_t fmt, void* stream);
/* W^T quantisation (e4m3) from the fp32 master W [rows, ld]: qt [cols, ldq]
 * (ldq % 16 == 0), one scale per column of W (per row of W^T). */
/* Every fp8 stack weight of a step at once (two launches): for each entry,
 * q = rows of W quantised per output channel (scales sq [rows]) and qt = W^T
 * quantised per input channel (scales sqt [cols], rows of ldqt bytes), from
 * the fp32 master W [rows, ld], cols <= 4096 (the first launch keeps a row in
 * registers: it quantises the rows and takes the column maxima from that one
 * read; the second reads W again for W^T). The host array is filled in by
 * maeclip_quant_weights_fp8_prepare (prefix sums; returns the workspace
 * bytes); dev is its device copy. */
typedef struct {
  const float* w;
  void* q;
  float* sq;
  void* qt;
  float* sqt;
  int32_t rows, cols, ld, ldqt;
  int64_t row_begin, unit_begin, part_begin;
} maeclip_fp8w_entry;
int64_t maeclip_quant_weights_fp8_prepare(maeclip_fp8w_entry* host, int32_t n);
int32_t maeclip_quant_weights_fp8(const maeclip_fp8w_entry* dev, const maeclip_fp8w_entry* host, int32_t n,
                                  float* workspace, int64_t ws_bytes, void* stream);
int64_t maeclip_quant_cols_fp8_workspace(int64_t rows, int64_t cols);
int32_t maeclip_quant_cols_fp8(const float* w, int64_t rows, int64_t cols, int64_t ld, void* qt, int64_t ldq,
                               float* scales, float* workspace, int64_t ws_bytes, void* stream);
int64_t maeclip_gemm_colsum_rows(int64_t M);
/* scratch bytes maeclip_gemm may use for *args when args->splitk <= 1 (pass
 * them as args->workspace; a NULL workspace is always valid, just slower) */
int64_t maeclip_gemm_workspace(const maeclip_gemm_args* args);
/* which kernel family maeclip_gemm runs *args on: 0 = v1 (128x128 MFMA tiles:
 * fp32 parity mode, odd K), 1 = the small fp32 kernel, 2 = v2 (LDS-DMA tiles),
 * 4 = v4 (256-wide ping-pong tiles). The arguments are checked as maeclip_gemm
 * checks them (-1 and a message if they fail; 0 for an empty output, which
 * launches nothing); nothing is launched and no device is needed. MAECLIP_GEMM_VARIANT (1..7 a v2 tile, 8 = v4 then v2,
 * 99 = v1) moves the answer as it moves the launch. */
int32_t maeclip_gemm_impl(const maeclip_gemm_args* args);
/* maeclip_gemm_impl plus, for a v4 call, its launch plan on `ncu` compute units
 * (ncu <= 0: the current device's, the only case that needs a device):
 * out = {tile height 256 / 192 / 128, in-launch split S (0: none), K-tiles of
 * slice 0, grid x, y, z, dynamic LDS bytes, persistent (1: one block per CU
 * loops over the tiles)}, zeros on the other routes; *workspace_bytes (may be
 * NULL): maeclip_gemm_workspace of the call for ncu compute units (the v4
 * split plan's scratch were a workspace offered, or the small path's K-slice
 * partials). The plan options
 * (maeclip_set_option) move the answer as they move the launch. Launches
 * nothing. maeclip_gemm_fp8_plan: the same for maeclip_gemm_fp8 (blocks = 0) /
 * maeclip_gemm_fp8_blocks (blocks != 0) after their argument checks; returns
 * 4 or -1. */
int32_t maeclip_gemm_plan(const maeclip_gemm_args* args, int32_t ncu, int32_t out[8], int64_t* workspace_bytes);
int32_t maeclip_gemm_fp8_plan(const maeclip_gemm_args* args, int32_t blocks, int32_t ncu, int32_t out[8],
                              int64_t* workspace_bytes);
int32_t maeclip_gemm_splitk(int64_t M, int64_t N, int64_t K);

/* Grouped weight gradients. Replaces the weight-gradient half of autograd's
 * nn.Linear backward (torch.nn.functional.linear's backward, reached from
 * loss.backward() at main.py:58) for all Linears of a transformer stack at
 * once (timm Block qkv/proj/fc1/fc2, HF ViTMAE decoder layers):
 *   dw_p[n][k] = sum_m dy_p[m*ldy + n] * x_p[m*ldx + k]  (+ beta * dw_p[n][k])
 * for p < nprob, m < M (tokens, shared by every problem). dw is fp32 dense
 * [N][K]; dy/x have `dtype`. bf16 problems with M % 64 == 0 and N, K >= 256
 * share one persistent launch per 48 problems (split-K slabs, S <= 4, only when
 * they cut the waves of output tiles by >= 15%); others run one maeclip_gemm
 * each.
 * Deterministic (fixed summation order). workspace: >= the bytes
 * maeclip_wgrad_grouped_workspace() returns (0 is common), 16-B aligned. */
typedef struct {
  const void* dy;
  const void* x;
  float* dw;
  int64_t N, K, ldy, ldx;
} maeclip_wgrad_problem;
int64_t maeclip_wgrad_grouped_workspace(const maeclip_wgrad_problem* probs, int32_t nprob, int64_t M,
                                        int32_t dtype);
int32_t maeclip_wgrad_grouped(const maeclip_wgrad_problem* probs, int32_t nprob, int64_t M, int32_t dtype,
                              float beta, void* workspace, int64_t ws_bytes, void* stream);
/* The launch plan of the first chunk (at most 48 problems) of such a call on
 * `ncu` compute units (ncu <= 0: the current device's), without a launch:
 * returns 1 and out = {output tiles T, uniform split-K slices S (1: none),
 * stream-K remainder K-tiles per block skw (0: none), whole tiles Tdp and
 * K-tiles per tile NT (both 0 without a remainder), blocks of the main launch,
 * reduce launch (0 none, 1 split-K slabs, 2 stream-K remainder), its grid x, y,
 * workspace bytes}; 0 when the list runs as one maeclip_gemm per problem; -1
 * for a bad list. */
int32_t maeclip_wgrad_grouped_plan(const maeclip_wgrad_problem* probs, int32_t nprob, int64_t M, int32_t dtype,
                                   int32_t ncu, int64_t out[10]);

/* ------------------------------------------------------------- attention
 * Replaces F.scaled_dot_product_attention in timm Attention / HF ViTMAE
 * decoder layers and DistilBERT attention with key-padding mask
 * (modeling_distilbert.py:125-145). qkv: [B*n, ld_qkv] token rows with q at
 * column h*hd, k at H*hd + h*hd, v at 2*H*hd + h*hd. o: [B*n, ld_o].
 * lse: [B, H, n] f32, log2-domain row log-sum-exp of scale*q.k (bwd input).
 * key_mask (optional, f32 [B, n]): 0 = padding key, in the forward and in the
 * backward (masked keys take P = 0: their dK / dV rows are zero). A sample
 * whose mask has no valid key is out of scope (DistilBERT's CLS is always
 * valid). dropout_p > 0 drops probabilities with the counter-based keep mask
 * of (seed, *step_ptr, b*H + h, q, k), scaled by 1/(1-p); the backward redraws
 * the same mask from the same seed / step value (ABI 12), so pass the
 * forward's: dV = (M.P/(1-p))^T dO, dS = P.(M/(1-p).(dO V^T) - rowsum(dO.O)).
 * The backward takes key_mask and dropout in bf16 and fp32 at head_dim 64 and
 * n <= 256 (the two-phase MFMA kernel's own instantiations; deterministic, no
 * atomics; the v-bias partial then comes from the dV it computes). Past that
 * the fp32 streamed "rows" path takes the mask (no dropout) and everything
 * else is rejected. fp32 forward / backward at any n: past the LDS images
 * (n ~ 540 at hd 32) 64-row blocks are streamed (no dropout there).
 * bf16 at any n: the resident kernels hold a head's whole K / V (backward:
 * Q / dO too) in LDS, up to n = 576 at hd 64 and n = 1216 (forward) / 1152
 * (backward) at hd 32; past that the streamed kernels take the call (option
 * ATTN_STREAM; forward and backward decide independently, lse and o are the
 * same convention): 64-row blocks through a two-slot LDS ring, the backward
 * as a dQ and a dK / dV launch plus a column-sum launch for colsum_partial,
 * deterministic, nothing allocated. They take neither key_mask nor dropout
 * (rejected with -1 before any launch), and q8 by the standalone pass.
 * bwd: dout [B*n, ld_o], dqkv [B*n, ld_dqkv]; colsum_partial optional
 * [B, 3*H*hd] per-sample column sums of dqkv (qkv bias gradient). */
typedef struct {
  const void* qkv;
  void* o;
  float* lse;
  const void* dout;
  void* dqkv;
  const float* key_mask;
  float* colsum_partial;
  int64_t ld_qkv, ld_o, ld_dqkv;
  int32_t B, n, H, head_dim, dtype;
  float scale, dropout_p;
  uint64_t seed;
  /* optional device step counter: dropout seed = seed + (*step_ptr) * MAECLIP_STEP_MULT
   * (so a captured HIP graph draws fresh masks every replay) */
  const int64_t* step_ptr;
  /* optional fp8-blocks copy of the main output (maeclip_fp8b_scale_bytes
   * layout; o [B*n, H*head_dim] for the forward, dqkv [B*n, 3*H*head_dim] for
   * the backward, whose row length must be a multiple of 128): the bytes of
   * maeclip_quant_blocks_fp8 of the bf16 output as stored. Written by the
   * bf16 MFMA kernels' own stores; the other variants (fp32, the diagonal and
   * row-streaming backward, the bf16 streamed kernels) run the standalone pass after the kernel. */
  void* q8;
  int64_t ldq8;
  uint8_t* q8_scale;
  int32_t q8_fmt;
} maeclip_attn_args;
int32_t maeclip_attn_fwd(const maeclip_attn_args* args, void* stream);
int32_t maeclip_attn_bwd(const maeclip_attn_args* args, void* stream);
/* The kernel maeclip_attn_fwd (bwd = 0) / maeclip_attn_bwd (bwd != 0) runs *args
 * on, after their argument checks and under the options set (-1 and the message
 * for a call they reject); nothing is launched and no device is needed:
 *   0 resident forward, 1 resident forward with 16 waves, 2 backward with four
 *   LDS images (fp32: the two-phase backward), 3 backward with two images, 4 two
 *   images at 3 workgroups per CU, 5 backward with key_mask / dropout, 6 diagonal
 *   backward, 7 16-wave backward, 8 fp32 rows, 9 streamed, 10 backward 2, 3 or 4
 *   by occupancy (bf16 with ATTN_TWO unset: the one choice that asks the device,
 *   made at the launch). */
int32_t maeclip_attn_impl(const maeclip_attn_args* args, int32_t bwd);

/* ------------------------------------------------------------- LayerNorm
 * Replaces nn.LayerNorm (timm norm1/norm2/fc_norm, modules.py:67, DistilBERT
 * LayerNorms, decoder_norm). fwd: x' = dropout(x; in_dropout_p) + res;
 * y = LN(x') (* out dropout); y2 optional bf16 copy; xsum_out optional x'. */
typedef struct {
  const void* x;
  int32_t x_dtype;
  const float* res;
  int64_t ldres;
  float in_dropout_p;
  const float* gamma;
  const float* beta;
  void* y;
  int32_t y_dtype;
  void* y2;
  int64_t ldy2;
  float* xsum_out;
  int64_t ldxs;
  float* mean;
  float* rstd;
  float out_dropout_p;
  uint64_t seed_in, seed_out;
  const int64_t* step_ptr; /* optional: both seeds + (*step_ptr) * MAECLIP_STEP_MULT */
  int64_t M, D, ldx, ldy;
  float eps;
  /* optional fp8 copy of y for an fp8 GEMM (C4): q8 [M, ldq8] quantised per
   * row exactly as maeclip_quant_rows_fp8 would quantise the stored y (format
   * q8_fmt, scales q8_scale [M]) -- the quantisation pass fused into the LN */
  void* q8;
  int64_t ldq8;
  float* q8_scale;
  int32_t q8_fmt;
} maeclip_ln_fwd_args;
int32_t maeclip_ln_fwd(const maeclip_ln_fwd_args* args, void* stream);

/* bwd: dx(f32) = LN'(dy) + dres; dx_bf optional bf16 copy; partials
 * [maeclip_ln_bwd_partial_rows(M, D)][D] of dgamma, dbeta, colsum(dx) (ABI 10: the
 * count depends on D -- up to 1024 workgroups at D <= 512, 512 above).
 * dres_pool (instead of dres, optional): the residual gradient is the
 * backward of timm's global_pool="avg" over pool_n tokens per sample, read
 * from dres_pool [M / pool_n][D]: row r gets dres_pool[r / pool_n] / (pool_n - 1)
 * for r % pool_n != 0 and 0 for the prefix (cls) token -- the pool backward
 * fused into the LN backward, no [M, D] residual tensor in HBM. */
typedef struct {
  const void* dy;
  int32_t dy_dtype;
  const void* x;
  int32_t x_dtype;
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* dres;
  float* dx;
  void* dx_bf;
  int64_t lddx_bf;
  float* dgamma_partial;
  float* dbeta_partial;
  float* dx_colsum_partial;
  int64_t M, D, ldx, lddy, lddx;
  const float* dres_pool;
  int64_t pool_n;
  /* optional fp8 copy of dx_bf (required with it) for an fp8 dgrad GEMM, as
   * maeclip_quant_rows_fp8 of dx_bf with format q8_fmt (fused) */
  void* q8;
  int64_t ldq8;
  float* q8_scale;
  int32_t q8_fmt;
} maeclip_ln_bwd_args;
int32_t maeclip_ln_bwd(const maeclip_ln_bwd_args* args, void* stream);
int32_t maeclip_ln_bwd_partial_rows(int64_t M, int64_t D);

/* ------------------------------------------------------------ reductions */
/* out[n] (+)= scale * sum_p partial[p*N + n]  (fixed order -> deterministic);
 * two passes when maeclip_colsum_scratch(P, N) > 0: scratch holds that many
 * floats (N > 1, P > 64: [ceil(P/64)][N]; N == 1, P > 4096: ceil(P/4096)),
 * may be NULL otherwise. */
int32_t maeclip_colsum_reduce(const float* partial, int64_t P, int64_t N, float* out, int32_t accumulate, float scale,
                              float* scratch, void* stream);
int64_t maeclip_colsum_scratch(int64_t P, int64_t N);
/* many independent column reductions in one launch (bias / LN-parameter
 * gradients of a whole transformer stack): out[n] (+)= scale * sum_p partial[p][n];
 * block_start = prefix sum of ceil(N/64) over the entries. */
typedef struct {
  const float* partial;
  float* out;
  int64_t P, N;
  float scale;
  int32_t accumulate;
  int64_t block_start;
} maeclip_colsum_entry;
int32_t maeclip_colsum_multi(const maeclip_colsum_entry* dev_entries, const maeclip_colsum_entry* host_entries,
                             int32_t ne, void* stream);
/* partial column sums of a [M, D] row matrix (dtype f32/bf16, row stride ld)
 * into partial [maeclip_rows_colsum_partial_rows(M)][D]; optional bf16 copy
 * out_bf16 [M, D]. */
int32_t maeclip_rows_colsum(const void* x, int32_t dtype, int64_t M, int64_t D, int64_t ld, void* out_bf16,
                            float* partial, void* stream);
/* the same with the fp8 rows of the bf16 copy (per-row scales, bit-identical
 * to maeclip_quant_rows_fp8 of out_bf16; the fp8 stack's top operand) */
int32_t maeclip_rows_colsum_q8(const void* x, int32_t dtype, int64_t M, int64_t D, int64_t ld, void* out_bf16,
                               float* partial, void* q8, int64_t ldq8, float* q8_scale, int32_t q8_fmt, void* stream);
int32_t maeclip_rows_colsum_partial_rows(int64_t M);
/* timm global_pool="avg": out[b] = mean_{t>=1} x[b,t,:] ; bwd scatters 1/(n-1) */
int32_t maeclip_pool_fwd(const float* x, int32_t B, int32_t n, int32_t D, float* out, void* stream);
int32_t maeclip_pool_bwd(const float* dout, int32_t B, int32_t n, int32_t D, float* dx, int32_t accumulate, void* stream);
/* nn.Dropout with the library's counter-based mask (same as LN in_dropout) */
int32_t maeclip_dropout(const float* x, float* y, int64_t M, int32_t D, int64_t ld, float p, uint64_t seed,
                        const int64_t* step_ptr, void* stream);
/* DistilBERT Embeddings word+position gather (modeling_distilbert.py:92-117);
 * mask_in (optional, int64 [B*T], the tokenizer's attention_mask) -> mask_out
 * (f32 [B*T], the attention kernels' key mask) in the same launch */
int32_t maeclip_embed_fwd(const int64_t* ids, const float* word, const float* pos, int32_t B, int32_t T, int32_t D,
                          int64_t V, float* out, const int64_t* mask_in, float* mask_out, void* stream);
/* its backward (ABI 12): dx f32 [B*T, D] -> dense dword [V, D] and dpos [P, D]
 * (P >= T). Rows no token maps to are zero, position rows >= T are zero, and
 * row padding_idx (-1: none; HF builds nn.Embedding(vocab, dim, padding_idx =
 * pad_token_id = 0)) stays zero. Tokens of one id are added in ascending
 * token order in fp32 by one workgroup and the row is written once: no
 * atomics, bitwise reproducible. No workspace, allocation or synchronisation
 * (capture-safe). ids are clamped to [0, V) as in the forward. */
int32_t maeclip_embed_bwd(const float* dx, const int64_t* ids, int32_t B, int32_t T, int32_t D, int64_t V, int64_t P,
                          int64_t padding_idx, float* dword, float* dpos, void* stream);

/* ---------------------------------------------------------- multi-tensor */
typedef struct {
  void* p0; /* param (f32) / cast source */
  void* p1; /* grad (f32) */
  void* p2; /* exp_avg */
  void* p3; /* exp_avg_sq */
  void* p4; /* bf16 shadow / cast destination (optional for adamw) */
  int64_t n;
  int64_t chunk_start; /* prefix sum of ceil(n / maeclip_mt_chunk()) */
} maeclip_mt_entry;
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  float step_size; /* lr / (1 - beta1^t) */
  float bc2_sqrt;  /* sqrt(1 - beta2^t) */
  float grad_scale;
  /* optional device step count t (>= 1): when set, step_size and bc2_sqrt are
   * recomputed in the kernel from lr, beta1, beta2 and *step_ptr */
  const int64_t* step_ptr;
  /* ABI 13, both optional (NULL: the by-value fields above, bit for bit).
   * lr_ptr: device learning rate, read in place of lr; decay = 1 - lr * wd and
   * step_size = lr / (1 - beta1^t) are derived in the kernel in fp32 exactly as
   * from the by-value lr, so it needs step_ptr. grad_scale_ptr: device factor
   * the gradient is multiplied by in place of grad_scale (the clip coefficient
   * of maeclip_clip_coef); the gradient tensor itself is not written. */
  const float* lr_ptr;
  const float* grad_scale_ptr;
} maeclip_adamw_hparams;
int64_t maeclip_mt_chunk(void);
/* dev_entries: device copy of host_entries (host pointer used for the grid size).
 * cast_multi: p4[i] = bf16(p0[i]) (RNE, NaN stays NaN), i < n, per entry. No
 * alignment contract beyond the element types' own (4 B for p0, 2 B for p4):
 * an entry whose p0 is 16-B aligned, whose p4 is 8-B aligned and whose n is a
 * multiple of 4 is converted with 16-B loads and 8-B stores, any other entry
 * element by element, with the same result. maeclip_adamw_multi makes the same
 * per-entry choice (p0..p3 16-B aligned, p4 8-B aligned, n % 4 == 0). */
int32_t maeclip_cast_multi(const maeclip_mt_entry* dev_entries, const maeclip_mt_entry* host_entries, int32_t ne,
                           void* stream);
/* flat conversion dst[i] = scale * src[i], dtypes MAECLIP_F32 / MAECLIP_BF16
 * (RNE): the bf16 gradient all-reduce buckets of data parallelism */
int32_t maeclip_cast_flat(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, float scale,
                          void* stream);
/* torch.optim.AdamW step (main.py:101-103,59) fused over all parameters */
int32_t maeclip_adamw_multi(const maeclip_mt_entry* dev_entries, const maeclip_mt_entry* host_entries, int32_t ne,
                            const maeclip_adamw_hparams* hp, void* stream);
/* global-norm gradient clipping (ABI 13), deterministic: no atomics, every sum
 * in a fixed order.
 * sumsq_multi: sum of squares of the f32 tensors p1 of an AdamW plan (the other
 * pointers are not read). Workgroup b of the plan (one per maeclip_mt_chunk()
 * elements, as in maeclip_adamw_multi) writes partials[partial_offset + b]; the
 * caller sizes partials for partial_offset + the plan's block count, so several
 * plans fill disjoint ranges of one buffer.
 * clip_coef: one workgroup sums n_partials values in double and writes
 * norm_out[0] = sqrt(sum) and coef_out[0] = min(1, max_norm / (norm + 1e-6)),
 * torch.nn.utils.clip_grad_norm_'s factor (NaN for a NaN norm, 0 for inf). */
int32_t maeclip_sumsq_multi(const maeclip_mt_entry* dev_entries, const maeclip_mt_entry* host_entries, int32_t ne,
                            float* partials, int64_t partial_offset, void* stream);
int32_t maeclip_clip_coef(const float* partials, int64_t n_partials, float max_norm, float* norm_out, float* coef_out,
                          void* stream);
/* dst[i] = host_values[i], i < n <= 32 (device f32). The values are copied into
 * the launch's kernel arguments, so host_values may be reused at once and any
 * number of such launches may be queued (the per-group learning rates). */
int32_t maeclip_store_f32(float* dst, const float* host_values, int32_t n, void* stream);

/* ------------------------------------------------------------------- MAE */
/* HF ViTMAE random_masking (modeling_vit_mae.py:297-327) with counter-based
 * noise: ids int32 [B, L]; mask f32 [B, L] (1 = removed); noise optional. */
typedef struct {
  int32_t* ids_shuffle;
  int32_t* ids_restore;
  float* mask;
  float* noise;
  int32_t B, L, len_keep;
  uint64_t seed, step, sample_offset;
  const int64_t* step_ptr; /* optional: step used = step + *step_ptr */
} maeclip_mask_args;
int32_t maeclip_mask_ids(const maeclip_mask_args* args, void* stream);

/* visible-patch rows for the patch-embed GEMM (timm PatchEmbed Conv2d(k=s=p)
 * as GEMM): out[(b*keep+j), c*p*p+ky*p+kx] = img[b,c,py*p+ky,px*p+kx] for
 * patch l = ids_shuffle[b,j] (identity if NULL); columns >= C*p*p zeroed.
 * Image source: fp32 NCHW img, or -- when img_u8 is set (img ignored) -- the
 * decoded uint8 RGB HWC pixels [B][S][S][C] (C = 3) with albumentations
 * Normalize(u8_mean, u8_std, u8_max_pixel) (dataset.py:49) and the HWC->CHW
 * permute (dataset.py:34) applied in the gather: the fp32 image is never
 * materialised (same floats as maeclip_image_normalize_u8 + the fp32 gather). */
typedef struct {
  const float* img;
  const int32_t* ids_shuffle;
  void* out;
  int64_t ld_out;
  int32_t B, C, S, p, keep, dtype;
  const uint8_t* img_u8;
  float u8_mean[3], u8_std[3], u8_max_pixel;
} maeclip_patch_args;
int32_t maeclip_patch_gather(const maeclip_patch_args* args, void* stream);

/* Input pipeline. Replaces dataset.py:44-58 on the host: albumentations
 * Normalize(mean, std, max_pixel_value) of the decoded RGB uint8 HWC image
 * (dataset.py:49) and permute(2, 0, 1).float() (dataset.py:34), for a batch:
 * src uint8 [B][H][W][3] dense -> dst fp32 [B][3][H][W] dense,
 * dst = (float(src) - mean*max_pixel) * (1 / (std*max_pixel)) in fp32. */
typedef struct {
  const uint8_t* src;
  float* dst;
  int64_t B, H, W;
  float mean[3], std[3];
  float max_pixel;
} maeclip_image_u8_args;
int32_t maeclip_image_normalize_u8(const maeclip_image_u8_args* args, void* stream);
/* The whole get_transforms() pipeline of dataset.py:44-58 + the permute of
 * :34 in one pass, for decoded RGB uint8 HWC images of ANY sizes: A.Resize(S,
 * S) (cv2.resize INTER_LINEAR: OpenCV's fixed-point uint8 algorithm, equal
 * size = copy, exact 2x = INTER_AREA) then A.Normalize as above, into dst fp32
 * [B][3][S][S]. images: DEVICE array of B descriptors (src rows of row_stride
 * bytes, 3 interleaved channels). */
typedef struct {
  const uint8_t* src;
  int32_t H, W;
  int64_t row_stride;
} maeclip_image_src;
typedef struct {
  const maeclip_image_src* images;
  float* dst;
  int64_t B, S;
  float mean[3], std[3];
  float max_pixel;
} maeclip_preprocess_args;
int32_t maeclip_image_preprocess_u8(const maeclip_preprocess_args* args, void* stream);

/* Training augmentation on the device: A.RandomResizedCrop(S, S, scale, ratio,
 * INTER_LINEAR) -> A.HorizontalFlip(p) -> (A.Normalize + permute), drawn from
 * the device step so that a replayed graph sees new pixels every step.
 *
 * maeclip_crop_params draws one box per sample: boxes int32 [B][5] = (x0, y0,
 * w, h, flip). Source sizes (H, W) of sample b: images[b].H / .W when `images`
 * is set, else sizes[2b], sizes[2b + 1] (clamped to [1, H] x [1, W]) when
 * `sizes` is set, else H x W for every sample. All arithmetic is double, in
 * exactly this order (input.hip mc_crop_draw; no fused multiply-add):
 *   step_seed = seed + (*step_ptr) * MAECLIP_STEP_MULT      (seed if NULL)
 *   u(k, f)   = (mc_hash4(step_seed, sample_offset + b, k, f) >> 8) * 2^-24
 *   lr0 = log(ratio[0]), lr1 = log(ratio[1])
 *   for attempt k = 0 .. 9:
 *     area = (H * W) * (scale[0] + u(k, 0) * (scale[1] - scale[0]))
 *     ar   = exp(lr0 + u(k, 1) * (lr1 - lr0))
 *     w = rint(sqrt(area * ar)), h = rint(sqrt(area / ar))   (ties to even)
 *     if 0 < w <= W and 0 < h <= H:
 *       y0 = floor(u(k, 2) * (H - h + 1)), x0 = floor(u(k, 3) * (W - w + 1)); stop
 *   after ten failures (get_params' centre crop), with in = W / H:
 *     in < ratio[0]: w = W, h = clamp(rint(W / ratio[0]), 1, H)
 *     in > ratio[1]: h = H, w = clamp(rint(H * ratio[1]), 1, W)
 *     else         : w = W, h = H
 *     y0 = (H - h) / 2, x0 = (W - w) / 2                     (integer division)
 *   flip = u(10, 4) < flip_p
 * maeclip_crop_params_host evaluates the same function on the CPU: every
 * pointer (images, sizes, step_ptr, boxes) is a HOST pointer, only H / W of a
 * descriptor are read, and nothing touches a device. exp / log may differ in
 * the last bit between the two, which can only matter where sqrt(...) lies
 * within ~1e-13 of a half-integer. */
typedef struct {
  const maeclip_image_src* images; /* optional: per-sample sizes from descriptors */
  const int32_t* sizes;            /* optional int32 [B][2] = (h, w); needs H, W > 0 */
  int32_t H, W;                    /* size of every sample / of a padded slot */
  int32_t* boxes;
  int32_t B;
  float scale[2], ratio[2], flip_p;
  uint64_t seed, sample_offset;
  const int64_t* step_ptr;
} maeclip_crop_params_args;
int32_t maeclip_crop_params(const maeclip_crop_params_args* args, void* stream);
int32_t maeclip_crop_params_host(const maeclip_crop_params_args* args);

/* crop -> resize -> flip -> store for a batch, boxes read from device memory
 * (maeclip_crop_params' or the caller's). Source: EITHER `images` (device
 * descriptor array, any sizes, row-strided) OR `batch`, a dense padded uint8
 * [B][Hmax][Wmax][3] with optional device `sizes` int32 [B][2] = valid (h, w)
 * of each slot (clamped to the slot). Every box is clamped into its image
 * (x0 in [0, W-1], w in [1, W-x0], likewise y), then the w x h crop is resized
 * to S x S exactly as maeclip_image_preprocess_u8 resizes a whole image
 * (copy at S x S, INTER_AREA at 2S x 2S, fixed-point INTER_LINEAR otherwise)
 * and mirrored when flip != 0: out[.., x] = resized[.., S-1-x]. Destinations
 * (at least one): dst_f32 fp32 [B][3][S][S], normalised as
 * maeclip_image_normalize_u8 does; dst_u8 uint8 [B][S][S][3]. */
typedef struct {
  const maeclip_image_src* images;
  const uint8_t* batch;
  const int32_t* sizes;
  int32_t Hmax, Wmax;
  const int32_t* boxes;
  float* dst_f32;
  uint8_t* dst_u8;
  int64_t B, S;
  float mean[3], std[3];
  float max_pixel;
} maeclip_augment_args;
int32_t maeclip_image_augment_u8(const maeclip_augment_args* args, void* stream);

/* Mixup / CutMix on the device (mix.hip): timm's Mixup with correct_lam=True,
 * no cutmix_minmax, partner of sample b = B - 1 - b (x.flip(0)), drawn from the
 * device step like the crop above, so a replayed graph mixes anew every step.
 *
 * One record per sample; as int32 [B][8] it reads (kind, partner, x0, y0, x1,
 * y1, bits of lam_pixel, bits of lam_target). kind: MAECLIP_MIX_NONE / _MIXUP /
 * _CUTMIX. The box is [x0, x1) x [y0, y1) in pixels. lam_pixel weighs the own
 * pixels of a mixup (1 otherwise); lam_target is the own label's weight.
 *
 * maeclip_mix_params draws the records. mode MAECLIP_MIX_BATCH: one draw for
 * the whole call, key = MAECLIP_MIX_BATCH_KEY whatever sample_offset is, so
 * every data-parallel rank draws the same mix; mode MAECLIP_MIX_ELEM: one draw
 * per sample, key = sample_offset + b. All arithmetic is double, in exactly
 * this order (mix.hip mc_mix_draw; no fused multiply-add); the fields start at
 * 16, the crop draw uses 0 .. 4, so at equal seeds the two are independent:
 *   step_seed = seed + (*step_ptr) * MAECLIP_STEP_MULT      (seed if NULL)
 *   u(k, f)  = (mc_hash4(step_seed, key, k, f) >> 8) * 2^-24           in [0, 1)
 *   uo(k, f) = ((mc_hash4(step_seed, key, k, f) >> 8) + 1) * 2^-24     in (0, 1]
 *   record = (NONE, B-1-b, 0, 0, 0, 0, 1, 1)
 *   if not u(0, 16) < prob: done
 *   both alphas > 0: cutmix = u(0, 17) < switch_prob, alpha = its alpha
 *   one alpha > 0  : that one (u(0, 17) is not looked at); none: done
 *   lam ~ Beta(alpha, alpha):
 *     alpha == 1: lam = u(0, 18)
 *     else      : X = gamma(alpha, 0), Y = gamma(alpha, 1), lam = X / (X + Y)
 *   gamma(a, g), Marsaglia-Tsang with Box-Muller normals, attempt t = 0 .. 15
 *   at k = 16 g + t:
 *     a' = a < 1 ? a + 1 : a;  d = a' - 1/3;  c = 1 / sqrt(9 d)   (1/3 = 1.0 / 3.0)
 *     x = sqrt(-2 log(uo(k, 18))) * cos(6.283185307179586 * u(k, 19))
 *     t1 = 1 + c x;  if t1 <= 0: next attempt
 *     v = t1 t1 t1 = (t1 * t1) * t1
 *     if log(uo(k, 20)) < 0.5 x x + d - d v + d log(v), evaluated
 *        (((0.5 * x) * x + d) - d * v) + d * log(v): G = d v, stop
 *     after 16 rejections: G = d (v = 1). An attempt is rejected with
 *     probability < 0.05 for every a' >= 1, so this happens with probability
 *     < 0.05^16 ~ 1.5e-21 per variate.
 *     a < 1: G = G * exp(log(uo(16 g, 21)) / a)                     (the boost)
 *   mixup : kind MIXUP, lam_pixel = lam_target = (float)lam
 *   cutmix: r = sqrt(1 - lam), ch = (int)(H r), cw = (int)(W r)     (truncation)
 *           cy = (int)floor(u(0, 22) H), cx = (int)floor(u(0, 23) W)
 *           y0 = clip(cy - ch / 2, 0, H), y1 = clip(cy + ch / 2, 0, H), x0 / x1
 *           likewise with cw, W (integer division; timm's rand_bbox)
 *           kind CUTMIX, lam_pixel = 1,
 *           lam_target = (float)(1 - (double)((x1 - x0) (y1 - y0)) / (double)(H W))
 * Every loop above has a fixed bound, and 0 < X, Y < inf, so 0 <= lam <= 1.
 * maeclip_mix_params_host evaluates the same function on the CPU: params and
 * step_ptr are HOST pointers and nothing touches a device. log / exp / cos may
 * differ in the last bit between the two: lam agrees to a few ulp, and a box
 * can differ only where H r or W r lies within ~1e-13 of an integer.
 * 0 <= B, 1 <= H, W <= 32768, alphas finite and >= 0, prob and switch_prob in [0, 1]. */
#define MAECLIP_MIX_NONE 0
#define MAECLIP_MIX_MIXUP 1
#define MAECLIP_MIX_CUTMIX 2
#define MAECLIP_MIX_BATCH 0
#define MAECLIP_MIX_ELEM 1
#define MAECLIP_MIX_BATCH_KEY 0x4d49584261746368ull /* "MIXBatch" */
typedef struct {
  int32_t kind, partner;
  int32_t x0, y0, x1, y1;
  float lam_pixel, lam_target;
} maeclip_mix_record;
typedef struct {
  maeclip_mix_record* params;
  int32_t B, H, W;
  float mixup_alpha, cutmix_alpha, prob, switch_prob;
  int32_t mode;
  uint64_t seed, sample_offset;
  const int64_t* step_ptr;
} maeclip_mix_params_args;
int32_t maeclip_mix_params(const maeclip_mix_params_args* args, void* stream);
int32_t maeclip_mix_params_host(const maeclip_mix_params_args* args);

/* dst = the batch mixed by `params` (device memory; maeclip_mix_params' or the
 * caller's own), out of place: dst overlapping src is an argument error.
 * dtype MAECLIP_MIX_U8: uint8 [B][S][S][3]; MAECLIP_MIX_F32: fp32 [B][3][S][S]
 * -- the two forms maeclip_image_augment_u8 emits. Per element, a = the own
 * sample's, p = the partner's (partner clamped to [0, B - 1]) at the same place:
 *   kind NONE (and any kind not listed): a
 *   kind CUTMIX: p where x0 <= x < x1 and y0 <= y < y1, a elsewhere, the box
 *     clamped into [0, S] first (x1 <= x0 or y1 <= y0: empty); exact copies
 *   kind MIXUP: v = fl32(fl32(lam a) + fl32(fl32(1 - lam) p)), lam = lam_pixel,
 *     no fused multiply-add; fp32 stores v, uint8 stores rintf(v) (ties to
 *     even; timm's FastCollateMixup), clamped to [0, 255] (a NaN gives 0)
 * 16-byte loads and stores when src and dst are 16-byte aligned and a sample's
 * extent in bytes is a multiple of 16 (S = 224: both dtypes); otherwise one
 * element per access, the same bits. One launch, nothing allocated, no
 * atomics: 2 reads + 1 write per element at most (a CUTMIX / NONE piece that
 * lies wholly on one side reads one source only). 1 <= S <= 8192; fp32
 * pointers 4-byte aligned. */
#define MAECLIP_MIX_U8 0
#define MAECLIP_MIX_F32 1
typedef struct {
  const void* src;
  void* dst;
  const maeclip_mix_record* params;
  int64_t B, S;
  int32_t dtype;
} maeclip_mix_images_args;
int32_t maeclip_mix_images(const maeclip_mix_images_args* args, void* stream);

/* The class-probability targets of the mix: targets fp32 [B][ld_t], ld_t >= C,
 *   t_bj = [j == y_b] lam_t + [j == y_p] fl32(1 - lam_t),   j < C
 * with y = labels (int32: label_dtype 0, int64: 1), p = the record's partner
 * (clamped to [0, B - 1]) and lam_t its lam_target; y_b == y_p gives exactly 1
 * at that column. Columns C .. ld_t - 1 get zeros. A label outside [0, C)
 * contributes nothing (as maeclip_xent_fwd treats one). Every thread computes
 * its own columns: no zero-then-scatter, no barrier, no atomics, one launch.
 * No label smoothing is applied here: maeclip_xent_fwd's eps is linear,
 * t' = (1 - eps) t + eps / C, and it applies it to soft targets as well, so
 * label_smoothing = eps there on these targets IS timm's mixup_target(eps) +
 * SoftTargetCrossEntropy: (1 - eps) (lam 1[y_a] + (1 - lam) 1[y_p]) + eps / C =
 * lam (on 1[y_a] + off) + (1 - lam) (on 1[y_p] + off), off = eps / C, on = 1 - eps. */
typedef struct {
  const void* labels;
  int32_t label_dtype;
  const maeclip_mix_record* params;
  float* targets;
  int64_t ld_t;
  int64_t B, C;
} maeclip_mix_targets_args;
int32_t maeclip_mix_targets(const maeclip_mix_targets_args* args, void* stream);

/* Stochastic depth (timm DropPath(p, scale_by_keep=True)) on a residual branch
 * of the pre-LN blocks (droppath.hip): x <- x + s_b branch(x), one s per sample
 * b and branch key k, drawn from the device step like the crop and mix draws,
 * so a replayed graph draws new masks every step and a resumed run continues
 * the sequence:
 *   step_seed = seed + (*step_ptr) * MAECLIP_STEP_MULT         (seed if NULL)
 *   u(b, k)   = (mc_hash4(step_seed, sample_offset + b, k, MAECLIP_DROPPATH_FIELD) >> 8) * 2^-24
 *               (a 24-bit integer times 2^-24: exact in fp32)
 *   keep(b,k) = u(b, k) >= p                                   (fp32 compare)
 *   s(b, k)   = keep ? 1.0f / (1.0f - p) : 0.0f                (one IEEE fp32 division, on the host)
 * k = 2 * block + branch, block the index in the WHOLE encoder, branch 0 =
 * attention, 1 = MLP. The field is 32; the crop draw uses 0 .. 4 and the mix
 * draw 16 .. 23, so at equal seeds the three are independent. sample_offset =
 * the index of the call's first sample in the global batch (rank * B + the
 * micro-batch's first sample), so ranks and micro-batches draw what one
 * whole-batch launch would. Nothing is stored: each kernel re-forms s for the
 * rows it owns (row r belongs to sample r / n).
 *
 * maeclip_droppath_fwd: out[r, :] = fl32(resid[r, :] + fl32(s branch[r, :])), fp32
 * [M][D] with row strides ld_*; two roundings, no fused multiply-add, so torch's
 * resid + s * branch is bit-exact. out == branch (same stride) is allowed: in
 * place; any other overlap of out with branch or resid is an argument error.
 * Rows of a dropped sample copy resid and do not read branch.
 * maeclip_droppath_bwd: gs[r, :] = fl32(s g[r, :]) stored in gs_dtype (MAECLIP_F32:
 * the product; MAECLIP_BF16: rounded to nearest even), g fp32; gs may not
 * overlap g. partial f32 [maeclip_droppath_partial_rows(M)][D] (dense) gets the
 * column sums of the fp32 products of each group of 64 consecutive rows, summed
 * in a fixed order without atomics: reduce with maeclip_colsum_reduce (the
 * branch's bias gradient). Groups depend on the row index alone, so launches on
 * row ranges that start at multiples of 64 fill the same partial rows one
 * whole launch would. Rows of a dropped sample write zeros and do not read g.
 * Both: one launch, 16-byte accesses (8-byte for bf16 gs): D % 4 == 0, strides
 * multiples of 4, fp32 pointers 16-byte and bf16 gs 8-byte aligned; 0 <= p < 1,
 * n >= 1, M % n == 0, k >= 0; maeclip_droppath_bwd D <= 2048.
 * maeclip_droppath_scales_host evaluates s on the CPU (nothing touches a
 * device): scales [nk][B] for keys[0 .. nk), host_step a HOST pointer or NULL. */
#define MAECLIP_DROPPATH_FIELD 32
typedef struct {
  const float* resid; /* fwd */
  int64_t ld_resid;
  const float* branch; /* fwd */
  int64_t ld_branch;
  float* out; /* fwd */
  int64_t ld_out;
  const float* g; /* bwd */
  int64_t ld_g;
  void* gs; /* bwd */
  int64_t ld_gs;
  int32_t gs_dtype;
  float* partial; /* bwd */
  int64_t M, D, n;
  float p;
  int32_t k;
  uint64_t seed, sample_offset;
  const int64_t* step_ptr;
} maeclip_droppath_args;
int32_t maeclip_droppath_fwd(const maeclip_droppath_args* args, void* stream);
int32_t maeclip_droppath_bwd(const maeclip_droppath_args* args, void* stream);
int64_t maeclip_droppath_partial_rows(int64_t M);
int32_t maeclip_droppath_scales_host(float* scales, int64_t B, const int32_t* keys, int32_t nk, float p, uint64_t seed,
                                     uint64_t sample_offset, const int64_t* host_step);

/* Retrieval (inference.py:40-45). l2_normalize replaces F.normalize(x, p=2,
 * dim=-1): y = x / max(||x||_2, eps), fp32 [M][P] rows (strides ldx / ldy).
 * topk_rows replaces torch.topk(dot_similarity, k) row-wise: s fp32 [Q][N]
 * (row stride lds) -> vals [Q][k] descending, idx [Q][k] (int64), ties broken
 * by the lower index; 1 <= k <= min(N, 1024). The similarity itself is an
 * fp32 maeclip_gemm (text_n @ image_n^T). */
int32_t maeclip_l2_normalize(const float* x, float* y, int64_t M, int64_t P, int64_t ldx, int64_t ldy, float eps,
                             void* stream);
int32_t maeclip_topk_rows(const float* s, int64_t Q, int64_t N, int64_t lds, int32_t k, float* vals, int64_t* idx,
                          void* stream);

/* Retrieval evaluation: similarity and top-k in one streamed pass, the [Q][N]
 * similarity matrix never written. maeclip_sim_topk: q fp32 [Q][P] (row stride
 * ldq), g fp32 [N][P] (row stride ldg), used as given (normalise first with
 * maeclip_l2_normalize; inputs are assumed finite). For every query row the k
 * largest s_ij = sum_p q_ip g_jp over j < N: vals fp32 [Q][k] descending, idx
 * int64 [Q][k], ties broken by the lower index (the order of
 * maeclip_topk_rows). The products are exact f32 fma chains in a fixed order,
 * so the result is deterministic and does not depend on the split count.
 * Limits: 1 <= k <= min(N, 64); P % 16 == 0, 16 <= P <= 512; Q >= 0 (0 is a
 * no-op); 1 <= N < 2^31 - 256; ldq, ldg >= P. Larger k: maeclip_gemm +
 * maeclip_topk_rows.
 * splits: over how many workgroups per 64-row query block the gallery is
 * divided (0 = automatic: enough to fill the chip when Q is small; > 0 =
 * forced, clamped to the number of 16-row gallery tiles). With more than one
 * split the partial lists go through ws (maeclip_sim_topk_workspace bytes,
 * 8-byte aligned) and a second launch merges them.
 * q_label int64 [Q] and g_label int64 [N], both or neither, with first_hit
 * int32 [Q]: first_hit[q] = the smallest t < k with g_label[idx[q][t]] ==
 * q_label[q], or k when there is none (recall@K = mean(first_hit < K) for any
 * K <= k).
 * maeclip_sim_topk_splits (host only): the split count a launch will use, < 0
 * on bad arguments. maeclip_sim_topk_workspace (host only): bytes of ws, 0
 * with one split. No allocation, no synchronisation, no atomics. */
int32_t maeclip_sim_topk_splits(int64_t Q, int64_t N, int64_t P, int32_t k, int32_t splits);
int64_t maeclip_sim_topk_workspace(int64_t Q, int64_t N, int64_t P, int32_t k, int32_t splits);
int32_t maeclip_sim_topk(const float* q, const float* g, int64_t Q, int64_t N, int64_t P, int64_t ldq, int64_t ldg,
                         int32_t k, int32_t splits, float* vals, int64_t* idx, const int64_t* q_label,
                         const int64_t* g_label, int32_t* first_hit, void* ws, int64_t ws_bytes, void* stream);

/* timm _pos_embed on the visible tokens: x[b,0] = cls + pos[0];
 * x[b,1+j] = y[b*keep+j] + pos[1+ids_shuffle[b,j]]; bwd: dy rows, dpos, dcls. */
typedef struct {
  const void* y;
  int64_t ldy;
  const int32_t* ids_shuffle;
  const int32_t* ids_restore;
  const float* pos;
  const float* cls;
  float* x;
  const float* dx;
  void* dy;
  float* dpos;
  float* dcls;
  int32_t B, L, keep, D, dtype;
} maeclip_tokens_args;
int32_t maeclip_tokens_fwd(const maeclip_tokens_args* args, void* stream);
int32_t maeclip_tokens_bwd(const maeclip_tokens_args* args, void* stream);

/* HF ViTMAEDecoder mask-token append + unshuffle + pos (modeling_vit_mae.py:548-566).
 * fwd: y f32 [B, 1+keep, ldy] -> out f32 [B, 1+L, D]. bwd (reads ids_restore):
 * dout f32 -> dy (dtype) [B, 1+keep, ldy]; dmask_partial / colsum_partial f32
 * [maeclip_unshuffle_bwd_partial_rows(B), D] (column-reduce them: mask_token
 * and decoder_embed bias gradients). D % 4 == 0, D <= 1024. */
typedef struct {
  const float* y;
  int64_t ldy;
  const int32_t* ids_shuffle;
  const int32_t* ids_restore;
  const float* mask_token;
  const float* pos;
  float* out;
  const float* dout;
  void* dy;
  float* dmask_partial;
  float* colsum_partial;
  int32_t B, L, keep, D, dtype;
} maeclip_unshuffle_args;
int32_t maeclip_unshuffle_fwd(const maeclip_unshuffle_args* args, void* stream);
int32_t maeclip_unshuffle_bwd(const maeclip_unshuffle_args* args, void* stream);
int32_t maeclip_unshuffle_bwd_partial_rows(int32_t B);

/* MAE reconstruction loss (modeling_vit_mae.py:706-745 patchify, :852-859).
 * pred: decoder output rows [B, 1+L, ldp] (row 0 = cls, ignored); targets are
 * patchified from img on the fly (only for masked patches) -- fp32 NCHW img,
 * or the uint8 HWC pixels img_u8 normalised in-kernel exactly as in
 * maeclip_patch_args (u8_mean / u8_std / u8_max_pixel). fwd: row_loss [B*L]
 * = mask * mean_k diff^2 (sum / mask_count outside). bwd: dpred [B, 1+L, lddp]
 * = grad_out[0] * loss_scale * 2 diff mask / (P * mask_count) (columns
 * [P, lddp) zeroed); colsum_partial [maeclip_mae_loss_bwd_partial_rows(B, L)][P]
 * optional. P = C*p*p <= 1024, P % 4 == 0. */
typedef struct {
  const void* pred;
  int64_t ldp;
  const float* img;
  const float* mask;
  float* row_loss;
  void* dpred;
  int64_t lddp;
  const float* grad_out;
  float* colsum_partial;
  float loss_scale, mask_count;
  int32_t B, C, S, p, L, norm_pix, dtype;
  const uint8_t* img_u8;
  float u8_mean[3], u8_std[3], u8_max_pixel;
} maeclip_mae_loss_args;
int32_t maeclip_mae_loss_fwd(const maeclip_mae_loss_args* args, void* stream);
int32_t maeclip_mae_loss_bwd(const maeclip_mae_loss_args* args, void* stream);
int32_t maeclip_mae_loss_bwd_partial_rows(int32_t B, int32_t L);

/* ------------------------------------------------------------- CLIP loss
 * CLIPModel.forward loss (CLIP.py:34-43) + cross_entropy (CLIP.py:46-52), fp32,
 * fused and deterministic, three launches at every N: the all-pairs products
 * once on the exact-f32 MFMA (S, L, L^T kept in the workspace, online row-LSE
 * partials), one statistics pass over the stored rows (row / column LSE, the
 * column sums of the soft targets, per-row losses and the loss), and the
 * gradient rows of the requested slice (no reduction launch). Above N = 2048
 * the statistics pass stages the column statistics per 2048-column chunk.
 * Any N >= 1; P in {64, 128, 256, 512}. I, T: [N, P] (row strides ld_I/ld_T, 0 = P, 16-B aligned rows).
 * loss: device scalar. row_loss_out (optional, [N]): rl_i with loss = sum rl_i.
 * dI, dT optional: d loss / d I, T for the rows [grad_row0, grad_row0 +
 * grad_rows) only (grad_rows 0 = to the end), stored from row 0 of dI / dT --
 * under data parallelism each rank asks for its own slice of the gathered batch.
 * workspace: >= maeclip_clip_loss_workspace(N, P, number of gradient rows).
 * Learnable temperature (ABI 14), both optional (NULL: the by-value field, bit
 * for bit). log_temperature: device f32 theta = ln tau; every kernel of the call
 * then uses tau = expf(*log_temperature) and ignores `temperature`, so a
 * captured graph follows the value in device memory. d_log_temperature: device
 * f32 output, d loss / d theta = sum_ij (dS_ij S_ij - dL_ij L_ij) over the rows
 * i in [grad_row0, grad_row0 + grad_rows) (the slices of disjoint row ranges
 * add up to the whole derivative); needs log_temperature, dI and dT. One more
 * launch (a one-workgroup fixed-order sum), deterministic like the rest. */
typedef struct {
  const float* I;
  const float* T;
  int64_t ld_I, ld_T;
  int64_t N, P;
  float temperature;
  float* loss;
  float* row_loss_out;
  float* dI;
  float* dT;
  int64_t ld_dI, ld_dT;
  int64_t grad_row0, grad_rows;
  void* workspace;
  size_t ws_bytes;
  const float* log_temperature;
  float* d_log_temperature;
} maeclip_clip_args;
size_t maeclip_clip_loss_workspace(int64_t N, int64_t P, int64_t grad_rows);
int32_t maeclip_clip_loss(const maeclip_clip_args* args, void* stream);

/* ---------------------------------------------- InfoNCE and SigLIP losses
 * The hard-target contrastive losses, fp32, fused and deterministic, with no
 * N x N matrix in memory (the gradient pass recomputes its logit tiles with
 * the fma chain of the statistics pass). l_ij = (I_i . T_j) / tau + b, tau as
 * in maeclip_clip_loss (the by-value field, or expf(*log_temperature)).
 * kind 0, InfoNCE (b = 0):
 *   loss = (1/2N) sum_i [lse_j(l_ij) + lse_j(l_ji) - 2 l_ii]
 *   launches: statistics, combine, gradient (if asked), reduce.
 * kind 1, SigLIP (z_ij = 2 delta_ij - 1, b = *logit_bias or 0):
 *   loss = -(1/N) sum_ij log sigma(z_ij l_ij)
 *   launches: products-and-gradient, reduce.
 * The embeddings are used as given (normalise first with maeclip_l2_normalize).
 * I, T, P, strides, loss, row_loss_out (per-row terms, their sum is the loss),
 * dI, dT and the gradient rows: as in maeclip_clip_args; the loss is always
 * that of all N rows. 1 <= N <= 262144.
 * d_log_temperature = -sum dl_ij (l_ij - b) and d_logit_bias = sum dl_ij, both
 * over the image rows i of the gradient slice and all j (slices of disjoint row
 * ranges add up to the whole derivative); both need dI and dT,
 * d_log_temperature needs log_temperature. logit_bias / d_logit_bias: kind 1.
 * workspace: >= maeclip_contrastive_workspace(N, P, number of gradient rows,
 * kind) bytes, 16-B aligned: O(N). */
typedef struct {
  const float* I;
  const float* T;
  int64_t ld_I, ld_T;
  int64_t N, P;
  int32_t kind;
  float temperature;
  const float* log_temperature;
  const float* logit_bias;
  float* loss;
  float* row_loss_out;
  float* dI;
  float* dT;
  int64_t ld_dI, ld_dT;
  int64_t grad_row0, grad_rows;
  float* d_log_temperature;
  float* d_logit_bias;
  void* workspace;
  size_t ws_bytes;
} maeclip_contrastive_args;
size_t maeclip_contrastive_workspace(int64_t N, int64_t P, int64_t grad_rows, int32_t kind); /* host only */
int32_t maeclip_contrastive_loss(const maeclip_contrastive_args* args, void* stream);
/* backward of maeclip_l2_normalize: dx = (g - y (y . g)) / ||x|| where ||x|| >
 * eps, g / eps elsewhere; one wave per row, fp32, fixed summation order. */
int32_t maeclip_l2_normalize_bwd(const float* x, const float* g, float* dx, int64_t M, int64_t P, int64_t ldx,
                                 int64_t ldg, int64_t lddx, float eps, void* stream);

/* ------------------------------------------------- softmax cross-entropy
 * torch.nn.functional.cross_entropy(reduction="mean") with label_smoothing over
 * class logits [M, C], fp32, class-index or class-probability targets, fused
 * and deterministic (fixed-order sums, no atomics; xent.hip). Per row i, row
 * stride ld >= C; columns >= C are never read:
 *   m = max_j x_j, lse = m + log sum_j exp(x_j - m), p_j = exp(x_j - lse)
 *   hard (soft_targets = 0): t_j = (1 - eps) [j == labels[i]] + eps / C
 *   soft (soft_targets = 1): t_j = (1 - eps) targets[i, j] + eps / C (row
 *     stride ld_t >= C; the rows need not sum to 1)
 *   r_i  = (sum_j t_j) lse - sum_j t_j x_j
 *   loss = s sum_i r_i, s = loss_scale / M (loss_scale: 1, or 1 / world under
 *     data parallelism)
 *   dlogits_ij = g s ((sum_j t_j) p_ij - t_ij), g = *grad_output (NULL: 1)
 *   rank_i = #{ j : x_j > x_y, or x_j == x_y and j < y }, y = labels[i]: top-k is
 *     a hit iff rank < k, ties broken by index.
 * Exactly one of labels and targets defines the loss: soft_targets = 0 takes
 * labels and no targets, soft_targets = 1 takes targets; labels may then still
 * be given, and only rank uses them. labels: int32 (label_dtype 0) or int64 (1).
 * A hard label outside [0, C) is defined behaviour: the row's loss term is 0,
 * its gradient row is zero and its rank is C. The divisor stays M -- unlike
 * torch's ignore_index, which divides by the number of rows kept.
 * 1 <= M < 2^31, 1 <= C < 2^31 (C = 1: loss 0, gradient 0), 0 <= eps < 1.
 * Alignment: every float / int32 pointer 4 bytes, int64 labels 8 bytes, the
 * workspace 16 bytes. The 16-byte loads and stores are used when the base of
 * logits (and of targets, and in the backward of dlogits) is 16-byte aligned
 * and its row stride is a multiple of 4; otherwise 4-byte accesses, same bits.
 * maeclip_xent_fwd writes loss [1], lse [M], and when not NULL row_loss [M] (the
 * terms s r_i, whose sum is the loss), lse_lo [M] and rank [M] (needs labels).
 * lse_lo is the rounding error of lse = fl(m + log sum exp): the backward takes
 * x - lse as (x - lse) - lse_lo, which keeps p exact to fp32 at |x| ~ 1e4 (NULL
 * in the backward: 0). Launches: the row pass, then a one-workgroup reduce in
 * double. workspace: >= maeclip_xent_workspace(M) bytes.
 * maeclip_xent_bwd reads logits, lse (, lse_lo) and the targets and writes
 * dlogits [M, ld_d], ld_d >= C, in one launch; columns C .. ld_d - 1 get exact
 * zeros. dlogits == logits (with ld_d == ld) is allowed: every element is read
 * by the thread that overwrites it, before it is overwritten. loss, row_loss,
 * rank and the workspace are not used. */
typedef struct {
  const float* logits;
  int64_t ld;
  const void* labels;
  int32_t label_dtype;
  int32_t soft_targets;
  const float* targets;
  int64_t ld_t;
  int64_t M, C;
  float label_smoothing;
  float loss_scale;
  float* loss;
  float* row_loss;
  float* lse;
  float* lse_lo;
  int32_t* rank;
  float* dlogits;
  int64_t ld_d;
  void* workspace;
  size_t ws_bytes;
} maeclip_xent_args;
size_t maeclip_xent_workspace(int64_t M); /* host only */
int32_t maeclip_xent_fwd(const maeclip_xent_args* args, void* stream);
int32_t maeclip_xent_bwd(const maeclip_xent_args* args, const float* grad_output, void* stream);

/* ------------------------------------------------------------ step state
 * Device-resident step counters (model RNG step, optimizer step t) so that a
 * whole training step can be captured once in a HIP graph and replayed. */
#define MAECLIP_STEP_MULT 0x9E3779B97F4A7C15ull
int32_t maeclip_counter_add(int64_t* counter, int64_t delta, void* stream);
/* snap[0] = counter[0]; counter[0] += delta -- the step a forward used, kept for
 * its backward (dropout masks re-drawn there) without a separate copy */
int32_t maeclip_counter_add_snap(int64_t* counter, int64_t delta, int64_t* snap, void* stream);
/* loss combination on device scalars (CLIP.py total loss + MAE term):
 * out[0] = a[0] + w * b[0] */
int32_t maeclip_scalar_axpy(const float* a, const float* b, float w, float* out, void* stream);
/* Pinned, device-mapped host memory (hipHostMalloc mapped) for values the host
 * reads every step without a copy launch: *host_ptr for the CPU, *dev_ptr for
 * kernels (e.g. maeclip_copy_f32's dst). The reference reads its loss every
 * step (main.py:64 loss.item()); a kernel inside the captured step writes it
 * here instead of a device-to-host copy. */
int32_t maeclip_host_mapped_alloc(int64_t bytes, void** host_ptr, void** dev_ptr);
int32_t maeclip_host_mapped_free(void* host_ptr);
/* dst[0..n) = src[0..n) (f32, small n; dst may be device-mapped host memory) */
int32_t maeclip_copy_f32(const float* src, float* dst, int64_t n, void* stream);
/* dst[(counter[0] & 1) n + i] = src[i]: the step's loss into one of two host
 * slots picked by the device step counter, so the host can read step k's value
 * while step k + 1 (writing the other slot) is already running */
int32_t maeclip_copy_f32_slot(const float* src, float* dst, int64_t n, const int64_t* counter, void* stream);
/* dst_i[k] = w * s[0] * src_i[k] (src_i NULL: w * s[0]) for two dense f32
 * arrays in one launch (n_i = 0: unused); src_i == dst_i allowed. The
 * backward of a loss that scales stored gradients by the incoming grad_output
 * (a device scalar) without a host sync. */
int32_t maeclip_scale_by_scalar2(const float* src0, float* dst0, int64_t n0, const float* src1, float* dst1, int64_t n1,
                                 const float* s, float w, void* stream);
/* stream-ordered device timestamp (REALTIME counter, maeclip_wallclock_khz ticks/ms) */
int32_t maeclip_timestamp(int64_t* dst, void* stream);
int64_t maeclip_wallclock_khz(void);
/* stream-ordered host->device copy (pinned src), capturable into a HIP graph */
int32_t maeclip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAECLIP_H */
