/* maskunet_hip.h -- C ABI of libmaskunet_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the MaskAttn-UNet forward/backward hot path.  The reference
 * (Belis0811/MaskUnet) has no FFI of its own: its hot path is a chain of torch aten ops invoked from
 * nn.Module.forward (code/ade20k/ade_semantic.py:152-314) and their autograd backward (:400).  Each
 * entry point below replaces one such op group; the reference line it stands for is cited.  The
 * Python binding that a maintainer would add is the ctypes table in maskunet_amd/_lib.py (shown in
 * INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory
 *     (outputs and workspaces included), nothing is allocated or freed inside, no host sync;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it (capturable);
 *   - activations are NHWC rows: a tensor [B,H,W,C] is M = B*H*W rows of C elements with row
 *     stride `ld` (elements); internal channel counts are multiples of 32 (callers zero-pad);
 *   - dtype: MU_F32 (0) = fp32 storage + exact-fp32 MFMA, MU_F16 (1) = fp16 storage + fp32 accumulate, MU_F32X (2) = fp32 storage +
 *     split-bf16 matrix products (matrix entry points only, see below);
 *     per-channel parameters, statistics and all parameter gradients are always fp32;
 *   - return value: 0 on success, <0 on error (MU_ERR_*); no exceptions cross the boundary.
 */
#ifndef MASKUNET_HIP_H
#define MASKUNET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MU_OK 0
#define MU_ERR_ARG (-1)       /* null pointer / non-positive size / unknown enum            */
#define MU_ERR_SHAPE (-2)     /* shape not supported by the kernels (alignment, channel set) */
#define MU_ERR_LAUNCH (-3)    /* HIP launch failure                                           */
#define MU_ERR_WORKSPACE (-4) /* workspace smaller than mu_*_workspace_bytes()                */

#define MU_F32 0
#define MU_F16 1
/* fp32 storage, matrix products on the 16-bit matrix cores with (hi, lo) splits of the fp32 operands, fp32 accumulate (~1e-5 relative per
 * product or better; torch's float32_matmul_precision "high").  Accepted by the matrix entry points (mu_conv_fwd, mu_conv_fwd_fused,
 * mu_conv1x1_fwd_add, mu_conv_wgrad, mu_attn_*); every other entry point takes MU_F32 for the same tensors.
 * With MU_F32X the MATRIX OPERANDS of those entry points are passed ENCODED (same size, same strides; the split then costs one pass per
 * tensor instead of VALU work per fragment per wave):
 *   - 1x1 layers / Linear (taps = 1) -- x and w of the convolutions, x and dy of the weight gradient: every aligned 16-byte chunk of four
 *     fp32 values re-written as [4 x bf16 hi | 4 x bf16 lo] by mu_split_encode; three bf16 MFMAs per product;
 *   - 3x3 layers (taps = 9; round 6) -- x and w of mu_conv_fwd / mu_conv_fwd_stats / mu_conv_fwd_fused: every aligned 16-byte chunk
 *     re-written as [4 x fp16 hi | 4 x fp16 lo] by mu_split_encode_h4 (|value| < 65504; 22 mantissa bits down to an absolute floor of
 *     2^-25), the weights under a static shift of 2^6 that the epilogues undo (mu_prep_weight / mu_prep_weights_multi with MU_F32X
 *     write every layer's layouts in the right encoding); three fp16 MFMAs per product.  Their BACKWARD has its own entry points:
 *     mu_conv_dgrad_h / mu_conv_wgrad_h take dy as ONE power-of-two-scaled fp16 operand (mu_bn_act_bwd_h, mu_bn_pair_bwd_h or
 *     mu_dy_encode_h) against the fp16 pair of the partner: two MFMAs per product.  mu_conv_wgrad with taps = 9 and MU_F32X serves
 *     only the <= 3-channel first layer (a plain-FMA kernel on plain fp32 operands);
 *   - qkv of the attention sweeps (mu_attn_*): every aligned 32-byte group of eight fp32 values re-written as
 *     [8 x fp16 hi | 8 x fp16 lo] by mu_split_encode_h (|value| < 65504; the softmax probabilities and dS then enter the matrix core as
 *     single fp16 operands: two MFMAs per P V / dS K / dS^T Q / P^T dO product, three for Q K^T and dO V^T).
 * Outputs, biases, residual / addend tensors, x / oattn / grad_out / dY of the attention block are plain fp32.  Producers that write an encoded form directly and save the encoding pass: mu_bn_act_fwd with MU_F32X writes
 * y in the 3x3 operand encoding (for a y that only feeds a 3x3 convolution), mu_bn_act_bwd_h / mu_bn_pair_bwd_h write dx as the scaled fp16
 * dy of the 3x3 convolution in front of the BatchNorm; their inputs, dres and all statistics stay plain fp32. */
#define MU_F32X 2

#define MU_ACT_NONE 0
#define MU_ACT_GELU 1 /* exact erf GELU, ade_semantic.py:201,208 */
#define MU_ACT_RELU 2 /* ade_semantic.py:286                      */

/* library / build identification ("gfx950"); host pointer to a static string */
const char* mu_version_host(void);

/* ---- layout -------------------------------------------------------------------------------- */
/* dst[b][c][r] = (dst_dtype) src[b][r][c], b < batch, r < R, c < C.  Replaces x.view(B,C,HW).permute
 * (ade_semantic.py:168), the `.view(B,C,H,W)` re-interpretation of [B,N,C] (:190) and the
 * NCHW<->NHWC conversions at the module boundary. */
int mu_transpose(const void* src, int src_dtype, long src_ld, void* dst, int dst_dtype, long dst_ld, int batch, int R, int C,
                 void* stream);
/* as mu_transpose, and additionally dst[b][c][r] = 0 for R <= r < R_pad <= dst_ld (the zero channel padding of the NHWC
 * layout). */
int mu_transpose_pad(const void* src, int src_dtype, long src_ld, void* dst, int dst_dtype, long dst_ld, int batch, int R, int C,
                     int R_pad, void* stream);
/* fp32x operand encoding (see MU_F32X): n_elems fp32 values (a multiple of 4, 16-byte aligned, contiguous rows) -> the chunk-encoded
 * operand; dst may be src (in place). */
int mu_split_encode(const void* src, void* dst, long n_elems, void* stream);
/* fp32x 3x3-CONVOLUTION operand encoding (see MU_F32X): n_elems fp32 values (a multiple of 4, 16-byte aligned, contiguous rows) ->
 * [4 fp16 hi | 4 fp16 lo] per chunk of four, hi = fp16(x), lo = fp16(x - hi); dst may be src (in place).  The input of a 3x3 layer
 * (nn.Conv2d k = 3 in ConvBlock, ade_semantic.py:199,202) that no producer wrote encoded. */
int mu_split_encode_h4(const void* src, void* dst, long n_elems, void* stream);
/* mu_split_encode_h4 with a second output: dst16 = the fp16 rounding of the values (n_elems halves: the hi halves as plain rows) -- the
 * saved-input form of the one-term weight gradient mu_conv_wgrad_h1.  Out of place. */
int mu_split_encode_h4x(const void* src, void* dst, void* dst16, long n_elems, void* stream);
/* A plain fp32 gradient (n_elems values, a multiple of 4) -> ONE power-of-two-scaled fp16 operand dy_h (n_elems halves; must not alias
 * dy) + dy_scale = {S, 1 / S} on the device (S max|dy| in [2^13, 2^14); no host sync): the dy form of mu_conv_dgrad_h / mu_conv_wgrad_h
 * for a 3x3 layer whose dy does not come out of mu_bn_act_bwd_h (a conv without a BatchNorm behind it, city_instance.py:243). */
long mu_dy_encode_h_workspace_bytes(void);
int mu_dy_encode_h(const void* dy, void* dy_h, float* dy_scale, long n_elems, void* workspace, long ws_bytes, void* stream);
/* fp32x ATTENTION operand encoding (see MU_F32X): n_elems fp32 values (a multiple of 8, 32-byte aligned) -> [8 fp16 hi | 8 fp16 lo] per
 * group of eight, hi = fp16(x), lo = fp16(x - hi); dst may be src (in place).  qkv of mu_attn_fwd / mu_attn_bwd* with MU_F32X. */
int mu_split_encode_h(const void* src, void* dst, long n_elems, void* stream);
/* y[M][Cout] = x[M][Cin] w^T + bias with y written DIRECTLY in the attention operand encoding (the mu_split_encode_h form): the q/k/v
 * projection nn.Linear(C, C) x 3 (ade_semantic.py:170-172) of the MU_F32X attention block as one 1x1 layer, without the separate
 * encoding pass over qkv.  x, w chunk-encoded MU_F32X operands (mu_split_encode), bias fp32 or NULL; Cin % 32 == 0, Cout % 64 == 0. */
int mu_conv1x1_fwd_enc_h(const void* x, const void* w, const float* bias, void* y, long M, int Cin, int Cout, long x_ld, long y_ld,
                         void* stream);
/* elementwise dtype conversion of n elements */
int mu_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream);
/* OIHW fp32 parameter -> tap-major compute layout [taps][rows_pad][cols_pad].
 * mode 0: forward weights (rows=O, cols=I); mode 1: data-gradient weights (taps flipped, rows=I, cols=O);
 * mode 2: both in one launch, dst = the mode-0 block followed by the mode-1 block [taps][cols_pad][rows_pad].
 * dtype MU_F32X: fp32-sized blocks in their operand encodings (see MU_F32X) -- taps = 1: both blocks bf16 chunk-encoded; taps = 9: the
 * forward block fp16 chunk-encoded (x 2^6), the data-gradient block as "HL" rows for mu_conv_dgrad_h: each row (tap, in) of the padded
 * output-channel count n becomes [n fp16 lo | n fp16 hi] of 2^6 w (the same bytes).  MU_F32X needs rows_pad % 4 == 0 and
 * cols_pad % 4 == 0, and with taps = 9 and mode != 0 that n <= 8192: MU_ERR_SHAPE otherwise, before anything is written to dst. */
int mu_prep_weight(const float* w_oihw, void* dst, int dtype, int O, int I, int taps, int rows_pad, int cols_pad, int mode,
                   void* stream);

/* mu_prep_weight for MANY layers in one launch (a training forward re-lays every conv weight of the model: nn.Conv2d keeps OIHW fp32
 * masters, ade_semantic.py:199,202,284).  jobs = DEVICE array of njobs x 10 int64:
 *   { address of the OIHW fp32 weight, dst offset in elements from dst_base, first_tile, O, I, taps, rows_pad, cols_pad, mode, 0 }
 * a layer occupies the 32 x 32 tiles [first_tile, first_tile + rows_pad/32 * cols_pad/32) of the launch (rows = O, cols = I, both padded
 * to multiples of 32; mode 0, 1 or 2 as above with rows/cols always meaning out/in); ntiles = the sum over layers.  njobs <= 128.
 * Same values, bit for bit, as njobs mu_prep_weight calls. */
int mu_prep_weights_multi(const void* jobs, int njobs, long ntiles, void* dst_base, int dtype, void* stream);

/* The q/k/v projection of one attention block -- three nn.Linear(C, C) with bias (ade_semantic.py:157-159,170-172) -- as ONE [3C, C]
 * 1x1 layer: dst = the forward block [3C][C] followed by the data-gradient block [C][3C] (mu_prep_weight mode 2 of the concatenated
 * weight), bias[3C] = the concatenated fp32 biases.  C % 32 == 0. */
int mu_prep_qkv(const float* wq, const float* wk, const float* wv, const float* bq, const float* bk, const float* bv, void* dst,
                float* bias, int dtype, int C, void* stream);

/* ---- convolution / linear (MFMA implicit GEMM) --------------------------------------------- */
/* y[p][co] = bias[co] + sum_{tap,ci} x[p+shift(tap)][ci] * w[tap][co][ci]; taps = 9 (3x3, pad 1) or 1.
 * Replaces nn.Conv2d in ConvBlock (ade_semantic.py:199,202), the 1x1 heads (:284, city_instance.py:243-249)
 * and nn.Linear query/key/value (:170-172, as one [3C,C] weight).  Called with mode-1 weights it is the
 * data-gradient of the same layer. */
int mu_conv_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int taps, long x_ld,
                long y_ld, int dtype, void* stream);
/* y = conv1x1(x, w) + addend over M rows (addend has y's row stride): the two gradients of Mask2FormerAttention's input -- the
 * data-gradient of the q/k/v projection and the residual branch of `attention_output += x` (ade_semantic.py:187) -- joined in the
 * projection's epilogue.  Only where mu_conv1x1_add_supported(...) == 1; MU_ERR_SHAPE otherwise (callers then use mu_conv_fwd + mu_add). */
int mu_conv1x1_add_supported(int Cin, int Cout, int dtype);
int mu_conv1x1_fwd_add(const void* x, const void* w, const void* addend, void* y, long M, int Cin, int Cout, long x_ld, long y_ld, int dtype,
                       void* stream);
/* Inference epilogue: y = act(conv(x, w) * scale[co] + shift[co] + res) with per-channel fp32 scale / shift (either may be NULL = 1 / 0),
 * res (may be NULL) a tensor with y's shape and row stride, act = MU_ACT_*.  One launch for Conv2d -> BatchNorm2d(eval) [-> BatchNorm2d(eval)]
 * [-> + x] -> GELU / ReLU of ConvBlock and the heads (ade_semantic.py:199-208, 283-287; validation loop :443-471) with (scale, shift)
 * from mu_bn_eval_fold; every shape mu_conv_fwd accepts. */
int mu_conv_fwd_fused(const void* x, const void* w, const float* scale, const float* shift, const void* res, int act, void* y, int B, int H,
                      int W, int Cin, int Cout, int taps, long x_ld, long y_ld, int dtype, void* stream);
/* mu_conv_fwd that also leaves per-tile BatchNorm statistics of its (rounded) output: stat_part[rows][Cout][2] floats =
 * (sum, sum of squares) per output channel, rows = mu_conv_stats_rows(...) (0 = this shape has no statistics epilogue;
 * stat_part must then be NULL).  Feeds mu_bn_train_stats_rows and saves the separate statistics sweep of
 * conv -> BatchNorm2d (ade_semantic.py:199-200, 202-204). */
int mu_conv_stats_rows(int B, int H, int W, int Cin, int Cout, int taps, int dtype);
int mu_conv_fwd_stats(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int taps,
                      long x_ld, long y_ld, int dtype, float* stat_part, void* stream);
/* Which kernel serves a shape -- host-only queries that never touch the device.  Each returns a small stable plan id (> 0; 0 = the
 * arguments are not served) read from the same selection function the entry point's launch switches on:
 *   mu_conv_fwd_plan        mu_conv_fwd (with_stats = 0) / mu_conv_fwd_stats with a statistics buffer (with_stats = 1);
 *   mu_conv_fwd_fused_plan  mu_conv_fwd_fused;
 *   mu_conv_dgrad_h_plan    mu_conv_dgrad_h (Cin = channels of dy, Cout = channels of dx, as in that entry);
 *   mu_conv_wgrad_plan      mu_conv_wgrad (pair = 0), mu_conv_wgrad_h1 (dtype MU_F16, pair = 0), mu_conv_wgrad_h (dtype MU_F16, pair = 1);
 *   mu_conv_wgrad_bias_plan mu_conv_wgrad_bias.
 * mu_conv_plan_name(op, id): the kernel's name, op = 0 forward, 1 fused, 2 dgrad_h, 3 wgrad; ids run from 1 to mu_conv_plan_count(op) - 1;
 * NULL for an id outside that range. */
int mu_conv_fwd_plan(int B, int H, int W, int Cin, int Cout, int taps, int dtype, int with_stats);
int mu_conv_fwd_fused_plan(int B, int H, int W, int Cin, int Cout, int taps, int dtype);
int mu_conv_dgrad_h_plan(int B, int H, int W, int Cin, int Cout);
int mu_conv_wgrad_plan(int B, int H, int W, int Cin, int Cout, int taps, int cin_valid, int dtype, int pair);
int mu_conv_wgrad_bias_plan(int B, int H, int W, int Cin, int Cout, int taps, int cin_valid, int dtype);
int mu_conv_plan_count(int op);
const char* mu_conv_plan_name(int op, int id);
/* fp32x 3x3 layers, two-term data gradient (round 6; autograd of nn.Conv2d k = 3, ade_semantic.py:199,202,400): dx[p][ci] =
 * (1 / S) sum_{tap,co} dy_h[p - shift(tap)][co] * w[co][ci][tap] with dy_h = fp16(S dy) ONE scaled fp16 operand (rows of Cin halves,
 * stride dy_ld halves; Cin = the layer's OUTPUT channels) and w_hl the HL data-gradient block of mu_prep_weight(MU_F32X, taps 9);
 * dx plain fp32 rows of Cout floats (the layer's INPUT channels, stride dx_ld floats); dy_scale = {S, 1 / S} on the device. */
int mu_conv_dgrad_h(const void* dy_h, const void* w_hl, const float* dy_scale, void* dx, int B, int H, int W, int Cin, int Cout, long dy_ld,
                    long dx_ld, void* stream);
/* fp32x 3x3 layers, two-term weight gradient: dw_oihw as mu_conv_wgrad from x = the layer's input in the 3x3 operand encoding
 * (mu_split_encode_h4 form, Cin channels, stride x_ld floats) and dy_h / dy_scale as above (Cout halves per row, stride dy_ld halves).
 * cin_valid > 3 (the first layer keeps mu_conv_wgrad on plain operands). */
long mu_conv_wgrad_h_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int mu_conv_wgrad_h(const void* x, const void* dy_h, const float* dy_scale, float* dw_oihw, int B, int H, int W, int Cin, int Cout,
                    int cin_valid, int cout_valid, long x_ld, long dy_ld, void* workspace, long ws_bytes, void* stream);
/* ... and its ONE-term form: x_h = the fp16 rounding of the input (rows of Cin halves, stride x_ld halves: the second output of
 * mu_bn_act_fwd_enc / mu_split_encode_h4x).  One MFMA per product on the fp16 kernels; dW sums over every pixel of the batch and the
 * roundings of x are random-signed: the sum carries ~2^-12 of the root-sum-square of its terms (no change of any gradient metric in the
 * oracle sizing).  Workspace: mu_conv_wgrad_workspace_bytes(B, H, W, Cin, Cout, 9). */
int mu_conv_wgrad_h1(const void* x_h, const void* dy_h, const float* dy_scale, float* dw_oihw, int B, int H, int W, int Cin, int Cout,
                     int cin_valid, int cout_valid, long x_ld, long dy_ld, void* workspace, long ws_bytes, void* stream);
/* dw_oihw[o][i][tap] = sum_p dy[p][o] * x[p+shift(tap)][i] for o < cout_valid, i < cin_valid (fp32, OIHW). */
long mu_conv_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int taps);
int mu_conv_wgrad(const void* x, const void* dy, float* dw_oihw, int B, int H, int W, int Cin, int Cout, int taps, int cin_valid,
                  int cout_valid, long x_ld, long dy_ld, void* workspace, long ws_bytes, int dtype, void* stream);
/* mu_conv_wgrad that also returns the bias gradient db[cout_valid] = sum over pixels of dy (nn.Linear query/key/value biases
 * :170-172, final_layer / head Conv2d biases :284) from the same sweep: the dy tiles are multiplied with one more column of ones.
 * Only where mu_conv_wgrad_bias_supported(...) == 1 (fp16 1x1 layers served by the wide tiles); MU_ERR_SHAPE otherwise --
 * callers then use mu_conv_wgrad + mu_colsum.  Same workspace size. */
int mu_conv_wgrad_bias_supported(int Cin, int Cout, int taps, int dtype);
int mu_conv_wgrad_bias(const void* x, const void* dy, float* dw_oihw, float* db, int B, int H, int W, int Cin, int Cout, int taps,
                       int cin_valid, int cout_valid, long x_ld, long dy_ld, void* workspace, long ws_bytes, int dtype, void* stream);
/* out[c] = sum_r x[r][c]  (bias gradients); dtype MU_F32X: x is chunk-encoded (mu_split_encode form) */
long mu_colsum_workspace_bytes(int C);
int mu_colsum(const void* x, long M, int C, long ld, float* out, void* workspace, long ws_bytes, int dtype, void* stream);

/* ---- BatchNorm2d (+activation, +residual) --------------------------------------------------- */
/* nn.BatchNorm2d training statistics (ade_semantic.py:200,204,219,240,285): biased batch variance ->
 * mean/rstd; running stats updated with the unbiased variance and `momentum` for c < c_valid
 * (running_* may be NULL); *num_batches_tracked (int64 on the device, may be NULL) is incremented. */
long mu_bn_workspace_bytes(int C);
int mu_bn_train_stats(const void* x, long M, int C, long ld, float* mean, float* rstd, float* running_mean, float* running_var,
                      long* num_batches_tracked, int c_valid, float momentum, float eps, void* workspace, long ws_bytes, int dtype,
                      void* stream);
/* the same from the rows written by mu_conv_fwd_stats (M = pixels per channel behind those rows) */
int mu_bn_train_stats_rows(const float* stat_part, int rows, long M, int C, float* mean, float* rstd, float* running_mean,
                           float* running_var, long* num_batches_tracked, int c_valid, float momentum, float eps, void* workspace,
                           long ws_bytes, void* stream);
/* eval mode: mean/rstd from the running statistics */
int mu_bn_eval_stats(const float* running_mean, const float* running_var, float eps, float* mean, float* rstd, int C, int c_valid,
                     void* stream);
/* eval mode, folded: the affine map of one BatchNorm2d with running statistics, or of two applied back to back (DownSample / UpSample
 * tails, :218-219, 239-240), behind a conv with optional bias: scale[c], shift[c] for mu_conv_fwd_fused; entries c >= c_valid are (0, 0).
 * gamma / beta / conv_bias and the whole second layer may be NULL. */
int mu_bn_eval_fold(const float* running_mean1, const float* running_var1, const float* gamma1, const float* beta1, float eps1,
                    const float* running_mean2, const float* running_var2, const float* gamma2, const float* beta2, float eps2,
                    const float* conv_bias, float* scale, float* shift, int C, int c_valid, void* stream);
/* y = act( res + (x-mean)*rstd*gamma + beta ); res may be NULL.  ConvBlock's BN+GELU (:200-201), BN (+x, GELU)
 * (:204,208) and final_layer's BN+ReLU (:285-286). */
int mu_bn_act_fwd(const void* x, const void* res, void* y, long M, int C, long ld, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, int act, int dtype, void* stream);
/* fp32x: mu_bn_act_fwd(MU_F32X) -- y written in the 3x3 operand encoding -- with a second output y16 = the fp16 rounding of y as plain rows
 * of C halves (row stride C; contiguous input rows): the form of y the backward of the convolution behind keeps (mu_conv_wgrad_h1). */
int mu_bn_act_fwd_enc(const void* x, const void* res, void* y_enc, void* y16, long M, int C, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int act, void* stream);
/* backward of mu_bn_act_fwd: dx (wrt x), dres (wrt res, iff res given), dgamma, dbeta.  training=1 uses the
 * batch-statistics formula, 0 treats mean/rstd as constants. */
int mu_bn_act_bwd(const void* x, const void* res, const void* grad_out, void* dx, void* dres, long M, int C, long ld,
                  const float* mean, const float* rstd, const float* gamma, const float* beta, int act, int training, float* dgamma,
                  float* dbeta, void* workspace, long ws_bytes, int dtype, void* stream);
/* BatchNorm pair: DownSample / UpSample apply nn.BatchNorm2d directly to the output of ConvBlock's last nn.BatchNorm2d
 * (ade_semantic.py:216-219, 237-240; maxpool_conv[2..3], conv[1..2]).  In training mode the second layer's batch statistics
 * follow from the first's (mean = beta1, biased var = gamma1^2 * var1/(var1+eps1)), so the pair is one normalisation of the conv
 * output: mu_bn_pair_compose turns (rstd1, gamma1, beta1, gamma2) into gamma_eff for mu_bn_act_fwd(.., gamma_eff, beta2), updates the
 * second layer's running statistics / step counter, and leaves the per-channel factors of the backward:
 * mu_bn_act_bwd_scaled(.., gamma_eff, .., xhat_scale) returns dx, dbeta = dbeta2 and dgamma = A;
 * dgamma2 = dgamma2_coef * A, dgamma1 = dgamma1_coef * A, dbeta1 = 0.  All vectors have C (padded) entries. */
int mu_bn_pair_compose(const float* rstd1, const float* gamma1, const float* beta1, const float* gamma2, int C, int c_valid, long M,
                       float eps1, float eps2, float momentum2, float* running_mean2, float* running_var2,
                       long* num_batches_tracked2, float* gamma_eff, float* xhat_scale, float* dgamma2_coef, float* dgamma1_coef,
                       void* stream);
/* mu_bn_act_bwd with the xhat term of the batch-statistics formula scaled per channel (xhat_scale NULL = mu_bn_act_bwd) */
int mu_bn_act_bwd_scaled(const void* x, const void* res, const void* grad_out, void* dx, void* dres, long M, int C, long ld,
                         const float* mean, const float* rstd, const float* gamma, const float* beta, int act, int training,
                         float* dgamma, float* dbeta, const float* xhat_scale, void* workspace, long ws_bytes, int dtype, void* stream);

/* The pair's whole backward in one call (training mode, no residual, no activation): mu_bn_act_bwd_scaled(.., gamma_eff, beta2, ..,
 * xhat_scale) plus the three parameter gradients that follow from A, written by the same finalize kernel:
 * pair_grads[0][c] = dgamma2_coef[c] * A[c] (dgamma2), pair_grads[1][c] = dgamma1_coef[c] * A[c] (dgamma1), pair_grads[2][c] = 0 (dbeta1);
 * dbeta2 as mu_bn_act_bwd's dbeta.  pair_grads: 3 * C floats. */
int mu_bn_pair_bwd(const void* x, const void* grad_out, void* dx, long M, int C, long ld, const float* mean, const float* rstd,
                   const float* gamma_eff, const float* beta2, const float* xhat_scale, const float* dgamma2_coef,
                   const float* dgamma1_coef, float* pair_grads, float* dbeta2, void* workspace, long ws_bytes, int dtype, void* stream);

/* fp32x (round 6): mu_bn_act_bwd / mu_bn_pair_bwd on fp32 storage (contiguous rows, ld = C) with dx written as ONE power-of-two-scaled
 * fp16 operand -- dx of a BatchNorm is the dy of the 3x3 convolution in front of it and of nothing else (ConvBlock wiring,
 * ade_semantic.py:199-204).  dx_h: M rows of C halves (row stride C); dy_scale = {S, 1 / S}, two floats written on the device from
 * maxima the statistics sweep collects (|S dx| < 2^14; no host sync), handed to mu_conv_dgrad_h / mu_conv_wgrad_h.  dres (residual
 * form) stays plain fp32.  The BatchNorm's own parameter gradients are computed from the fp32 operands as always. */
int mu_bn_act_bwd_h(const void* x, const void* res, const void* grad_out, void* dx_h, void* dres, long M, int C, const float* mean,
                    const float* rstd, const float* gamma, const float* beta, int act, int training, float* dgamma, float* dbeta,
                    float* dy_scale, void* workspace, long ws_bytes, void* stream);
int mu_bn_pair_bwd_h(const void* x, const void* grad_out, void* dx_h, long M, int C, const float* mean, const float* rstd,
                     const float* gamma_eff, const float* beta2, const float* xhat_scale, const float* dgamma2_coef,
                     const float* dgamma1_coef, float* pair_grads, float* dbeta2, float* dy_scale, void* workspace, long ws_bytes,
                     void* stream);

/* ---- per-sample LayerNorm with full-shape affine: nn.LayerNorm([64,128,128]) (:281,311) ------ */
long mu_ln_sample_workspace_bytes(int B);
int mu_ln_sample_fwd(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd, int B, long L, float eps,
                     void* workspace, long ws_bytes, int dtype, void* stream);
int mu_ln_sample_bwd(const void* x, const void* dy, const float* w, const float* mean, const float* rstd, void* dx, float* dw,
                     float* db, int B, long L, void* workspace, long ws_bytes, int dtype, void* stream);

/* ---- pooling / resampling -------------------------------------------------------------------- */
/* nn.MaxPool2d(2) (:216); backward recomputes the arg-max (first maximum in scan order).  NaN as in aten: the scan over
 * (0,0), (0,1), (1,0), (1,1) updates on `t > m || isnan(t)`, so a window that holds a NaN pools to NaN and its gradient goes to the
 * last NaN of the window.  Odd H / W floor; the uncovered last row / column gets a zero gradient (plus dx_add). */
int mu_maxpool2_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
int mu_maxpool2_bwd(const void* x, const void* dy, void* dx, int B, int H, int W, int C, int dtype, void* stream);
/* mu_maxpool2_bwd with gradient joins that autograd would otherwise run as separate elementwise kernels: dy2 (may be NULL, pooled
 * resolution) is a second gradient of the pooled tensor -- the residual branch of the ConvBlock behind the pool, F.gelu(x + block(x))
 * (:208, 216-217) -- and dx_add (may be NULL, input resolution) a gradient the pool's input received from its other consumer, the skip
 * connection into UpSample (:253, 303-309):  dx = scatter(dy + dy2) + dx_add. */
int mu_maxpool2_bwd_acc(const void* x, const void* dy, const void* dy2, const void* dx_add, void* dx, int B, int H, int W, int C, int dtype,
                        void* stream);
/* y = cat([skip, bilinear_x2(x, align_corners=True)], channel)  (:235,250-253); x [B,h,w,Cx], skip [B,2h,2w,Cs] */
int mu_upcat_fwd(const void* x, const void* skip, void* y, int B, int h, int w, int Cx, int Cs, int dtype, void* stream);
int mu_upcat_bwd(const void* dy, void* dx, void* dskip, int B, int h, int w, int Cx, int Cs, int dtype, void* stream);
/* mu_upcat_bwd of (dy + dy2): dy2 (may be NULL) is the residual-branch gradient of the ConvBlock behind the concat (:208, 237-238) */
int mu_upcat_bwd_acc(const void* dy, const void* dy2, void* dx, void* dskip, int B, int h, int w, int Cx, int Cs, int dtype, void* stream);
/* the same for channel counts that are not multiples of the 32-channel padding (stand-alone UpSample, :231-256): x holds
 * Cx_valid of Cx_ld stored channels, skip Cs_valid of Cs_ld; y rows are [skip valid | up valid | zeros] with Ct_ld stored channels.
 * The backward writes exact zeros into the padded channels of dx / dskip. */
int mu_upcat_compact_fwd(const void* x, const void* skip, void* y, int B, int h, int w, int Cx_ld, int Cx_valid, int Cs_ld, int Cs_valid,
                         int Ct_ld, int dtype, void* stream);
int mu_upcat_compact_bwd(const void* dy, void* dx, void* dskip, int B, int h, int w, int Cx_ld, int Cx_valid, int Cs_ld, int Cs_valid,
                         int Ct_ld, int dtype, void* stream);
/* nn.Dropout (:273,304,307): y = x*keep/(1-p); keep from `mask` (uint8, may be NULL) or the (seed,index) generator.
 * The backward is the same call on the gradient with the same seed/mask. mask_out (may be NULL) receives keep. */
int mu_dropout(const void* x, void* y, long n, float p, unsigned long long seed, const unsigned char* mask, unsigned char* mask_out,
               int dtype, void* stream);
/* the same with a device-resident step counter mixed into the seed (seed_step[0], read by the kernel): a training step captured in
 * a HIP graph bakes `seed` into the launch, the counter -- bumped inside the graph -- gives every replay its own mask, and the
 * backward launch of the same replay regenerates the same one.  seed_step NULL = mu_dropout. */
int mu_dropout_step(const void* x, void* y, long n, float p, unsigned long long seed, const unsigned long long* seed_step,
                    const unsigned char* mask, unsigned char* mask_out, int dtype, void* stream);

/* out = a + b over n elements (joins the residual and projection gradients of the attention block, :187) */
int mu_add(const void* a, const void* b, void* out, long n, int dtype, void* stream);

/* ---- masked attention (flash-style) ---------------------------------------------------------- */
/* The key mask of Mask2FormerAttention (`torch.randint(0, 2, (B,H,W))` -> {0,-inf} per KEY, ade_semantic.py:177-183) as the index list
 * the kernels below iterate over: kidx[b] = the visible keys in ascending order followed by the masked keys in ascending order (a whole
 * permutation of 0..N-1 == torch.argsort(keep, descending=True, stable=True): the MU_ATTN_KIDX_PERMUTATION form), kcnt[b] = visible
 * keys.  keep: [B][N], 1-byte or 8-byte integers (keep_elem_bytes), non-zero = visible; keep8 (may be NULL) receives the {0,1} bytes. */
int mu_compact_keys(const void* keep, int keep_elem_bytes, int B, int N, int* kidx, int* kcnt, unsigned char* keep8, void* stream);
/* Mask2FormerAttention core (ade_semantic.py:174-188) on projected qkv [B,N,3C]:
 *   out = LayerNorm_C( softmax_keys( q k^T / sqrt(C) + keymask ) v + x ), token-major [B,N,C].
 * The {0,-inf} key mask is given as the compacted list of kept keys: kidx[b][0..kcnt[b]) (int32, row
 * stride nkmax).  Also returns what the backward needs: oattn (PV/l, pre-residual), lse2 (log2-domain
 * log-sum-exp of the scaled scores), LayerNorm mean/rstd per token.  C in {32,64,128,256}.
 * An image without a visible key (kcnt[b] == 0) yields NaN in out / oattn and, in the backward, NaN dY and NaN dQ / dK / dV rows --
 * what the reference's softmax over -inf only produces (:183-185).  fp16: the sweep first runs without per-tile running-max tracking and verifies the row sums; a score
 * that exceeds the first 64 kept keys' maximum by more than 16 (log2 units) makes the block repeat its sweep with exact tracking. */
int mu_attn_fwd(const void* qkv, const void* x, const int* kidx, const int* kcnt, const float* gamma, const float* beta, void* out,
                void* oattn, float* lse2, float* ln_mean, float* ln_rstd, int B, int N, int C, int nkmax, float eps, int dtype,
                void* stream);
/* backward: grad_out [B,N,C] (wrt `out`) -> dY (grad wrt the pre-LayerNorm sum, i.e. the residual branch),
 * dqkv [B,N,3C] (masked keys get exact zeros), dgamma, dbeta.  delta [B,N] is scratch output.  workspace: 16-byte aligned,
 * mu_attn_bwd_workspace_bytes(B, N, C) bytes (the same size for every dtype).
 * Refusal order of the attention entry points: a null pointer, a non-positive B / N / nkmax or c_valid outside 1..C is MU_ERR_ARG; then
 * (backward) ws_bytes below the query is MU_ERR_WORKSPACE; then an unknown dtype is MU_ERR_ARG; then (backward) N % 4 != 0, or a C
 * outside {32,64,128,256}, is MU_ERR_SHAPE.  A refused call enqueues nothing: no kernel and no memset, every buffer is left as it was. */
long mu_attn_bwd_workspace_bytes(int B, int N, int C);
int mu_attn_bwd(const void* qkv, const void* x, const void* oattn, const void* grad_out, const int* kidx, const int* kcnt,
                const float* lse2, const float* ln_mean, const float* ln_rstd, const float* gamma, void* dY, float* delta, void* dqkv,
                float* dgamma, float* dbeta, int B, int N, int C, int nkmax, void* workspace, long ws_bytes, int dtype, void* stream);
/* the same, one phase group at a time (bit mask): 1 = zero dqkv + LayerNorm backward / delta / dgamma,dbeta,
 * 2 = dQ sweep, 4 = dK/dV sweep.  Phases 2 and 4 need phase 1's dY, delta and workspace contents.
 * 8 (MU_ATTN_KIDX_PERMUTATION, OR-ed into every call of one backward) = a promise about kidx: nkmax == N and every row is a whole
 * permutation of 0..N-1 with the masked keys listed after the kept ones (what a stable descending argsort of the keep mask
 * gives).  The dK/dV sweep then writes the masked keys' zero rows itself and phase 1 skips the memset of the whole dqkv buffer. */
#define MU_ATTN_KIDX_PERMUTATION 8
/* 16 (MU_ATTN_DQKV_ENCODED, OR-ed into every call of one backward; MU_F32X only, ignored otherwise): dqkv is written CHUNK-ENCODED
 * ([4 bf16 hi | 4 bf16 lo] per 16 bytes, the mu_split_encode form) -- the operand form mu_conv_fwd / mu_conv1x1_fwd_add / mu_conv_wgrad
 * take for the q/k/v projection's data- and weight-gradient, and mu_colsum(MU_F32X) for its bias gradient. */
#define MU_ATTN_DQKV_ENCODED 16
int mu_attn_bwd_phases(const void* qkv, const void* x, const void* oattn, const void* grad_out, const int* kidx, const int* kcnt,
                       const float* lse2, const float* ln_mean, const float* ln_rstd, const float* gamma, void* dY, float* delta,
                       void* dqkv, float* dgamma, float* dbeta, int B, int N, int C, int nkmax, void* workspace, long ws_bytes,
                       int dtype, int phases, void* stream);
/* Channel counts that are not one of the kernels' widths (32, 64, 128, 256) -- `Mask2FormerAttention(channels, size)` accepts any
 * (ade_semantic.py:153-161) -- run zero-padded: C = the padded width every tensor here is stored with (qkv, x, out, ... and gamma /
 * beta, all zero in the pad channels: zero-padded projection weights give zero Q/K/V pads), c_valid = the true channel count.  The
 * scores are scaled by 1/sqrt(c_valid), the LayerNorm spans the first c_valid channels, pad channels of every output are zero.
 * c_valid == C is exactly mu_attn_fwd / mu_attn_bwd_phases. */
int mu_attn_fwd_padded(const void* qkv, const void* x, const int* kidx, const int* kcnt, const float* gamma, const float* beta, void* out,
                       void* oattn, float* lse2, float* ln_mean, float* ln_rstd, int B, int N, int C, int c_valid, int nkmax, float eps,
                       int dtype, void* stream);
int mu_attn_bwd_phases_padded(const void* qkv, const void* x, const void* oattn, const void* grad_out, const int* kidx, const int* kcnt,
                              const float* lse2, const float* ln_mean, const float* ln_rstd, const float* gamma, void* dY, float* delta,
                              void* dqkv, float* dgamma, float* dbeta, int B, int N, int C, int c_valid, int nkmax, void* workspace,
                              long ws_bytes, int dtype, int phases, void* stream);
/* ---- generic path for channel counts above the sweeps' widths (C > 256) ------------------------------------------
 * `Mask2FormerAttention(channels, size)` accepts any `channels` (ade_semantic.py:153-161); the model uses 64 / 128 / 256.  For wider
 * blocks the products of one image run as GEMMs on mu_conv_fwd / mu_conv_wgrad (taps = 1) over the KEPT key rows -- S = Q Kg^T,
 * O = P Vg, dP = dO Vg^T, dQ = dS Kg, dKg = dS^T Q, dVg = P^T dO, an N x Nk score tile per image does exist on this path -- and the
 * row kernels below sit in between (maskunet_amd/ops.py `_WideMaskAttention`).  dtype MU_F16 or MU_F32 (MU_F32X is taken as MU_F32:
 * plain, un-encoded fp32 tensors); cnt = a device pointer to ONE int (kcnt + b), idx = kidx + b * nkmax.
 *   mu_gather_rows : dst[j][0..C) = j < *cnt ? src[idx[j]][0..C) : 0 for j < rows_out (src rows src_ld elements apart, dst dense)
 *   mu_scatter_rows: dst[idx[j]][0..C) = (T) src[j][0..C) for j < *cnt (fp32 src dense, dst rows dst_ld apart; other rows untouched);
 *                    *cnt == 0: all dst_rows rows NaN (the reference's dK / dV of an image without a visible key)
 *   mu_softmax_rows: S[r][j] <- softmax_j(scale * S[r][j]) over j < *cnt, 0 for *cnt <= j < ld (:174-184; no visible key: NaN rows,
 *                    as the reference's softmax of an all -inf row)
 *   mu_attn_wide_ds: dP[r][j] <- P[r][j] * (dP[r][j] - sum_k P[r][k] dP[r][k] / sum_k P[r][k]) * scale for j < *cnt, 0 behind (softmax
 *                    backward; the division by the stored row's own sum, 1 to rounding, keeps dS right where one key dominates)
 *   mu_ln_rows_fwd : out = LayerNorm over the first c_valid of C stored channels of (o + x), * gamma + beta (:187-188); mean / rstd
 *                    [rows] saved for the backward; pad channels 0
 *   mu_ln_rows_bwd : dY = d(o + x) of the above; g_xhat = grad_out * xhat (its column sums are dgamma, those of grad_out dbeta:
 *                    mu_colsum) */
int mu_gather_rows(const void* src, long src_ld, const int* idx, const int* cnt, void* dst, int rows_out, int C, int dtype, void* stream);
int mu_scatter_rows(const float* src, const int* idx, const int* cnt, void* dst, long dst_ld, int dst_rows, int C, int dtype, void* stream);
int mu_softmax_rows(void* S, int N, int ld, const int* cnt, float scale, int dtype, void* stream);
int mu_attn_wide_ds(const void* P, void* dP, int N, int ld, const int* cnt, float scale, int dtype, void* stream);
int mu_ln_rows_fwd(const void* o, const void* x, const float* gamma, const float* beta, void* out, float* mean, float* rstd, long rows,
                   int C, int c_valid, float eps, int dtype, void* stream);
int mu_ln_rows_bwd(const void* grad_out, const void* o, const void* x, const float* mean, const float* rstd, const float* gamma, void* dY,
                   void* g_xhat, long rows, int C, int c_valid, int dtype, void* stream);

/* ---- "next" rows: the steps either side of the path ------------------------------ */
/* f1: nn.CrossEntropyLoss (ade_semantic.py:377,399; ignore_index: city_semantic.py:341) on NHWC logits [M, Cp] (C valid
 * channels): mean loss over counted pixels -> loss[0], count[0]; lse[M] is saved for the backward. */
long mu_ce_workspace_bytes(void);
int mu_ce_fwd(const void* logits, const long* labels, long M, int Cp, int C, long ignore_index, float* lse, float* loss, float* count,
              void* workspace, long ws_bytes, int dtype, void* stream);
/* dlogits = (softmax - onehot) * grad_out[0] * grad_scale / count[0]; zeros for ignored pixels and padded channels */
int mu_ce_bwd(const void* logits, const long* labels, const float* lse, const float* count, const float* grad_out, float grad_scale,
              long M, int Cp, int C, long ignore_index, void* dlogits, int dtype, void* stream);
/* f1 on the module's own output: the same loss on NCHW logits [B, C, HW] (fp32 or fp16) exactly as the reference calls it,
 * criterion(outputs, labels) (ade_semantic.py:399; city_semantic.py:341,362); labels [B, HW]; lse [B*HW]; workspace as mu_ce_fwd */
int mu_ce_nchw_fwd(const void* logits, const long* labels, int B, int C, long HW, long ignore_index, float* lse, float* loss,
                   float* count, void* workspace, long ws_bytes, int dtype, void* stream);
int mu_ce_nchw_bwd(const void* logits, const long* labels, const float* lse, const float* count, const float* grad_out,
                   float grad_scale, int B, int C, long HW, long ignore_index, void* dlogits, int dtype, void* stream);
/* f3: mean_iou (ade_semantic.py:128-146) without host syncs.  Element (pixel r, class c) is read at
 * logits[(r / inner) * outer_stride + c * c_stride + (r % inner) * p_stride]; counts is scratch [3*C] uint32; out[0] = mean IoU. */
int mu_mean_iou(const void* logits, const long* labels, long M, int C, long inner, long outer_stride, long c_stride, long p_stride,
                float smooth, unsigned int* counts, float* out, int dtype, void* stream);
/* f1b: InstanceContrastiveLoss (ade_panoptic.py:390-418, city_instance.py:279-307) on the device, no host round trips.
 * feat: fp32 NCHW [B,C,H,W]; mask: int64 [B,H,W] instance ids in [0, id_cap) (others ignored); ignore_label < 0: none;
 * u[k] in [0,1): the k-th instance (ids ascending) that reaches the reference's torch.randint draw takes negative pixel
 * floor(u[k] * n_neg); at most max_inst instances.  loss[0] = mean triplet margin loss (0 without instances).  The backward
 * re-uses the workspace of the forward and writes d loss / d feat * grad_out[0] (dfeat is zero-filled first). */
long mu_inst_triplet_workspace_bytes(int id_cap, int max_inst);
int mu_inst_triplet_fwd(const float* feat, const long* mask, int B, int C, int H, int W, int ignore_label, float margin,
                        const float* u, int id_cap, int max_inst, void* workspace, long ws_bytes, float* loss, void* stream);
int mu_inst_triplet_bwd(const float* feat, int B, int C, int H, int W, const void* workspace, int id_cap, int max_inst,
                        const float* grad_out, float* dfeat, void* stream);
/* Refusal order of the post-processing entry points (mu_instances, mu_dbscan_instances, mu_instance_pairs, mu_instance_match,
 * mu_coco_match, mu_id_instances, mu_rle_encode / _decode, mu_coco_masks, mu_panoptic, mu_sem_eval, mu_sem_eval_native): a null pointer,
 * a non-positive or otherwise invalid scalar, an unknown dtype / kind is MU_ERR_ARG; then a shape outside the limits of the entry's
 * mu_*_supported is MU_ERR_SHAPE (the two match entries then check their thresholds / area ranges: MU_ERR_ARG; mu_sem_eval_native then
 * its block count: MU_ERR_SHAPE); then ws_bytes below the entry's mu_*_workspace_bytes is MU_ERR_WORKSPACE (mu_sem_eval then checks its
 * block count: MU_ERR_SHAPE); then a kernel that needs more dynamic LDS than the default limit is granted it, once per process and
 * kernel: a failure is MU_ERR_LAUNCH; only then the first kernel or memset.  A refused call enqueues nothing, every buffer is left as it
 * was.  mu_pil_resize_u8_nhwc keeps its own convention (below): MU_ERR_ARG for its limits and for a short workspace, -1 from its size
 * query.  The size query of an entry and the carve of its workspace are one walk over one layout type in the entry's source file. */
/* f5: instance post-processing of the instance / panoptic scripts on the device (no host round trip of the [B,c,H,W] output).
 * mu_argmax_prob: probs = softmax(outputs / 0.5, dim=1); preds = argmax(probs, 1) (ade_instance.py:408-411, ade_panoptic.py:529-532)
 * in one read of the logits, addressed as in mu_mean_iou.  cls[r] = first arg-max over the C channels (taken on the logits: softmax is
 * monotone), prob[r] = 1 / sum_c exp((x_c - x_max) * inv_temperature) = the soft-max probability of that class; prob may be null.
 * The logits must be finite. */
int mu_argmax_prob(const void* logits, long M, int C, long inner, long outer_stride, long c_stride, long p_stride,
                   float inv_temperature, int* cls, float* prob_or_null, int dtype, void* stream);
/* get_instances_from_mask (ade_instance.py:367-397: per class cv2.connectedComponents, 8-connected; per component bbox and mean
 * probability), its sorted(..., key=score, reverse=True) (ade_instance.py:417-419) and generate_instance_mask (ade_panoptic.py:36-47).
 * cls: int32 [B,H,W], values <= 0 are background; prob: fp32 [B,H,W] or null (score 1.0, the ground-truth case).
 * ids [B,H,W]: 0 = background, else 1..count[b] in raster order of each instance's first pixel (always complete, also past max_inst);
 * count [B]: the true number of instances; rows k < min(count, max_inst) of
 *   table [B,max_inst,8] = class, area, x_min, y_min, x_max, y_max, first_pixel (y*W+x), class_rank (1-based among the instances of
 *                          the same class in id order: the value generate_instance_mask writes),
 *   score [B,max_inst]   = mean of prob over the instance (fixed-point sums: bit-identical from run to run),
 *   order [B,max_inst]   = ids by descending score, ties by ascending id;
 * the remaining rows are zero.  H*W <= 65536 and 1 <= max_inst <= 4096, else MU_ERR_SHAPE (mu_instances_supported: host only). */
long mu_instances_workspace_bytes(int B, int H, int W, int max_inst);
int mu_instances_supported(int H, int W, int max_inst);
int mu_instances(const int* cls, const float* prob_or_null, int B, int H, int W, int max_inst, int* ids, int* table, float* score,
                 int* count, int* order, void* workspace, long ws_bytes, void* stream);
/* Instances of the 3-head model from its embedding head: get_instances_from_embeddings + get_instance_annotations
 * (city_instance.py:405-449), i.e. per image and per class 1 <= c < num_classes (ascending; every other value is background)
 * sklearn's DBSCAN(eps, min_samples) over the embeddings of the class's pixels, restated:
 *   points     the pixels of class c in raster order, D coordinates each;
 *   neighbours i ~ j iff sum_k (double(a_k) - double(b_k))^2 <= double(eps)^2, decided in fp64 for fp32 and fp16 input alike (i ~ i);
 *   core       at least min_samples neighbours, itself included;
 *   clusters   connected components of the core points under ~, ordered by their lowest core point (not their lowest pixel);
 *   border     a non-core point with a core neighbour joins the first such cluster that has one; other non-core points are noise (id 0);
 *   ids        1..count per image over (class ascending, cluster order).
 * cls: int32 [B,H,W].  emb element (pixel r of B*H*W, channel k) at emb[(r / inner) * outer_stride + k * c_stride + (r % inner) * p_stride]
 * (the addressing of mu_argmax_prob: NCHW, or the NHWC rows of a module output), dtype MU_F32 / MU_F16, values finite.
 * ids / table / score / count / order as for mu_instances (also past max_inst); every score is 1.0, so order is ascending id;
 * first_pixel is the instance's lowest pixel, which may be a border pixel.  Bit-identical from run to run.
 * H*W <= 65536, 1 <= D <= 64, 1 <= num_classes <= 1024, 1 <= max_inst <= 4096, min_samples >= 1, eps > 0, else MU_ERR_SHAPE
 * (mu_dbscan_supported and mu_dbscan_workspace_bytes: host only; the latter is 0 for unsupported shapes). */
long mu_dbscan_workspace_bytes(int B, int H, int W, int num_classes, int max_inst);
int mu_dbscan_supported(int H, int W, int D, int num_classes, int max_inst);
int mu_dbscan_instances(const int* cls, const void* emb, int B, int H, int W, int D, long inner, long outer_stride, long c_stride,
                        long p_stride, int dtype, int num_classes, float eps, int min_samples, int max_inst, int* ids, int* table,
                        float* score, int* count, int* order, void* workspace, long ws_bytes, void* stream);
/* Ground-truth instances from an id map the dataset supplies: get_instance_annotations(gt_inst, gt_sem) (city_instance.py:431-449,
 * called at :472-474) on Cityscapes instanceIds, on panopticapi's rgb2id of a COCO panoptic PNG (coco_panoptic.py:70-85) or on the ids
 * of mu_coco_masks.  id_map [B,H,W]: MU_IDMAP_I32 int32, MU_IDMAP_I64 int64, or MU_IDMAP_RGB8 uint8 [B,H,W,3] in RGB order with
 * v = R + 256 * G + 65536 * B formed in the kernel.  sem: int32 [B,H,W].
 *   dropped    a pixel with v != 0 whose class is outside [0, class_cap) (bit 0 of invalid[b]) or whose int64 v does not fit int32
 *              (bit 1) counts as v = 0 below; invalid [B] is written for every image, 0 when clean;
 *   numbering  the distinct non-zero values in ascending SIGNED order (np.unique) are v_1 < ... < v_count; instance k is the set of
 *              pixels that hold v_k (it need not be connected);
 *   ids / count / table / score / order as for mu_instances (ids and count complete past max_inst; score 1.0 and order 1..K over the
 *              K = min(count, max_inst) rows, zero after), with
 *              class       = (c_((n-1)/2) + c_(n/2)) / 2 over the instance's n semantic values in ascending order, integer division:
 *                            int(np.median(..)), possibly a class that no pixel of the instance has,
 *              first_pixel = the instance's lowest raster index;
 *   values [B,max_inst]: v_k in row k - 1 for k <= K, 0 after.
 * Stream-ordered, nothing read back, integer atomics only: bit-identical from run to run; every output byte is written.
 * H*W <= 65536, 1 <= max_inst <= 4096, 1 <= class_cap <= 1024, else MU_ERR_SHAPE; an unknown id_kind is MU_ERR_ARG
 * (mu_id_instances_supported and mu_id_instances_workspace_bytes: host only; the latter is 0 for unsupported shapes). */
#define MU_IDMAP_I32 0
#define MU_IDMAP_I64 1
#define MU_IDMAP_RGB8 2
int mu_id_instances_supported(int H, int W, int max_inst, int class_cap);
long mu_id_instances_workspace_bytes(int B, int H, int W, int max_inst, int class_cap);
int mu_id_instances(const void* id_map, int id_kind, const int* sem, int B, int H, int W, int max_inst, int class_cap, int* ids,
                    int* table, float* score, int* count, int* order, int* values, int* invalid, void* workspace, long ws_bytes,
                    void* stream);
/* Panoptic segments (the stage save_predictions / evaluate_panoptic leave open, coco_panoptic.py:388-439): the semantic map and the
 * instances of mu_instances / mu_dbscan_instances / mu_id_instances merged into COCO panoptic segments.  The rule restates
 * panopticapi's published format (id2rgb, segments_info, one segment per stuff class) and the usual semantic + instance merge.
 * cls int32 [B,H,W]; ids int32 [B,H,W], table int32 [B,max_inst,8], score fp32 [B,max_inst], count int32 [B] as those entry points
 * write them; kind int32 [num_classes]: 0 void, 1 stuff, 2 thing; category int32 [num_classes]: label -> dataset category id.
 * For a pixel with k = ids, c = cls:
 *   thing      1 <= k <= min(count, max_inst) and kind[table[k-1].class] == 2 (a class outside [0, num_classes) is void): the pixel
 *              belongs to thing candidate k, kept iff table[k-1].area >= thing_area_limit and score[k-1] >= score_threshold (fp32);
 *              the pixels of a candidate that is not kept are VOID, they do not become stuff.  max_inst < k <= count: void, and bit 2
 *              of invalid[b].  k <= 0, k > count, or an instance whose class is not a thing: no instance;
 *   stuff      otherwise, 0 <= c < num_classes and kind[c] == 1: a stuff candidate of class c; the class is kept iff the image has at
 *              least max(stuff_area_limit, 1) such pixels, and all of them form ONE segment, connected or not;
 *   void       everything else.
 *   numbering  the kept segments that hold a pixel are 1..n by their first pixel in raster order; seg_count[b] = n, also past max_seg.
 * seg int32 [B,H,W]: the segment number, 0 = void, complete also past max_seg.  seg_cls int32 [B,H,W]: the segment's class
 * (table[k-1].class of a thing, c of stuff), 0 on void.  Per segment, rows [B,max_seg], zero past min(n, max_seg):
 *   seg_table  int32 x 8, the columns of mu_instances over the segment's pixels; class_rank = the 1-based rank among the kept segments of
 *              the class in segment order (always 1 for stuff);
 *   seg_score  fp32: score[k-1] of a thing, 1.0 of stuff;   seg_order: segments by descending score, ties by ascending number;
 *   seg_source the instance id k of a thing, 0 of stuff;
 *   seg_values the COCO segment id category[class] * label_divisor + (thing ? class_rank : 0), or 0 where that id is <= 0, >= 2^24, or
 *              a thing's class_rank >= label_divisor (ids would collide or not fit a PNG): bit 0 of invalid[b].
 * id_map int32 [B,H,W]: seg_values of the pixel's segment; 0 on void, on a segment past max_seg and on one of bit 0.  rgb uint8
 * [B,H,W,3]: panopticapi's id2rgb of id_map, R = v & 255, G = (v >> 8) & 255, B = v >> 16, stored R,G,B, or B,G,R with bgr = 1.
 * invalid int32 [B]: bit 0 and bit 2 above, bit 1: n > max_seg (rows past max_seg are dropped).
 * One launch, one workgroup per image, stream-ordered, nothing read back, integer atomics only: bit-identical from run to run; every
 * output byte is written.  H*W <= 65536, 1 <= max_inst <= 4096, 1 <= max_seg <= 4096, 1 <= num_classes <= 1024, label_divisor >= 1,
 * both area limits >= 0, else MU_ERR_SHAPE; bgr other than 0 / 1 is MU_ERR_ARG (mu_panoptic_supported and
 * mu_panoptic_workspace_bytes: host only; the latter is 0 for unsupported shapes). */
int mu_panoptic_supported(int H, int W, int max_inst, int num_classes, int max_seg, int label_divisor, int stuff_area_limit,
                          int thing_area_limit);
long mu_panoptic_workspace_bytes(int B, int H, int W, int max_inst, int num_classes, int max_seg);
int mu_panoptic(const int* cls, const int* ids, const int* table, const float* score, const int* count, const int* kind,
                const int* category, int B, int H, int W, int max_inst, int num_classes, int label_divisor, int stuff_area_limit,
                int thing_area_limit, float score_threshold, int max_seg, int bgr, int* seg, int* seg_cls, int* seg_table,
                float* seg_score, int* seg_count, int* seg_order, int* seg_source, int* seg_values, int* id_map, unsigned char* rgb,
                int* invalid, void* workspace, long ws_bytes, void* stream);
/* Semantic evaluation of one validation batch in ONE read of the logits: what the validation loops take from `outputs` --
 * criterion(outputs, labels) (ade_semantic.py:454; ignore_index = 255: city_semantic.py:341), mean_iou(outputs, labels, c_out)
 * (city_panoptic.py:225-236, ade_semantic.py:128-146), compute_iou_for_image per image (city_panoptic.py:212-222) and
 * softmax(outputs / 0.5) + argmax (ade_instance.py:408-411) -- and the confusion matrix their sklearn precision / recall / F1 are
 * functions of.  Element (pixel r of M = B * HW, class c) at logits[(r / inner) * outer_stride + c * c_stride + (r % inner) * p_stride],
 * exactly as mu_mean_iou / mu_argmax_prob; the image of r is r / HW; labels int64 [M]; the logits must be finite.
 *   pred[r]    the first maximum over the C real channels (torch.argmax); padded channels are never read into the maximum;
 *   void       row r is void if labels[r] == ignore_index or labels[r] lies outside [0, C);
 *   img_counts int32 [B,3,C], overwritten: per image I_c = #(pred == c and label == c), P_c = #(pred == c), L_c = #(label == c).
 *              P counts every pixel, void ones too; I and L only non-void ones -- what mean_iou and compute_iou_for_image count (a
 *              label of 255 equals no class, but the prediction at that pixel still enters the union);
 *   confusion  int64 [C+1,C], ADDED TO (the caller zeroes it once and accumulates a validation set): row = the label, or C for void;
 *              column = pred.  Column sums are sum_b P_c, the sum of row c is sum_b L_c, the diagonal is sum_b I_c;
 *   img_loss   fp64 [B,2], overwritten: {sum over the non-void rows of image b of lse_r - x[r, label_r], the number of such rows}; lse
 *              in fp32 as mu_ce_fwd; the sums in a fixed order (per-block fp64 partials in the workspace, then an ordered finalize);
 *   cls int32 [M], prob fp32 [M], each may be null: pred, and 1 / sum_c exp((x_c - x_max) * inv_temperature) as mu_argmax_prob.
 * Integer atomics only: every output is bit-identical from run to run.  The (C+1) x C counters are privatised in LDS per workgroup
 * for C <= MU_SEM_EVAL_LDS_MAX_C and flushed with 64-bit atomics; above it every pixel adds to the global matrix.
 * Null required pointers, B < 1, HW < 1, HW >= 2^31, inner < 1, a dtype other than MU_F32 / MU_F16 or inv_temperature <= 0:
 * MU_ERR_ARG; C outside [1, 4096]: MU_ERR_SHAPE (mu_sem_eval_supported); a short workspace: MU_ERR_WORKSPACE; all before the first
 * launch.  mu_sem_eval_supported and mu_sem_eval_workspace_bytes are host only; the latter is 0 for unsupported shapes. */
#define MU_SEM_EVAL_LDS_MAX_C 192
int mu_sem_eval_supported(int C);
long mu_sem_eval_workspace_bytes(int B, long HW, int C);
int mu_sem_eval(const void* logits, const long* labels, int B, long HW, int C, long inner, long outer_stride, long c_stride,
                long p_stride, long ignore_index, float inv_temperature, int* img_counts, double* img_loss, long* confusion,
                int* cls_or_null, float* prob_or_null, void* workspace, long ws_bytes, int dtype, void* stream);
/* Semantic evaluation at the labels' OWN resolution: what ADE20K, Cityscapes and COCO define as mIoU.  The logits of image b are upsampled
 * bilinearly to the size of that image's label map, the first arg-max is taken there and counted against the labels, in one kernel that
 * never writes the upsampled logits.  This text is the specification.
 * logits: B images of h x w pixels and C real classes, element (pixel r of M = B * h * w, class c) at
 * logits[(r / inner) * outer_stride + c * c_stride + (r % inner) * p_stride] exactly as mu_sem_eval (NCHW, or the channel-padded NHWC rows
 * of a module output); MU_F32 or MU_F16; the values must be finite.  Labels: a ragged uint8 batch as mu_pil_resize_u8_nhwc takes one --
 * image b is the H_b * W_b bytes at labels + offsets[b], (H_b, W_b) = sizes[b][0..1]; offsets int64 [B+1] in bytes and sizes int32 [B][2]
 * are DEVICE arrays, image starts need no alignment, and the host passes only the bounds max_h, max_w.  ignore_index: any value outside
 * [0, 255] means "none".
 * Rule per image b and output pixel (Y, X); every fp32 operation is rounded on its own (NO fused multiply-add), fp16 logits are widened
 * exactly to fp32:
 *   sy = fp32(h) / fp32(H_b)                      (IEEE division; sx likewise from w, W_b)
 *   fy = max(sy * (fp32(Y) + 0.5f) - 0.5f, 0.0f)
 *   y0 = min((int)fy, h - 1);  y1 = y0 + (y0 < h - 1);  ly1 = fy - fp32(y0);  ly0 = 1.0f - ly1        (x0, x1, lx0, lx1 likewise)
 *   v_c  = ly0 * (lx0 * x[c,y0,x0] + lx1 * x[c,y0,x1]) + ly1 * (lx0 * x[c,y1,x0] + lx1 * x[c,y1,x1])
 *   pred = the first c in ascending order with the largest v_c      (strict > replaces; padded channels are never read)
 * This is the formula of torch's upsample_bilinear2d(align_corners=False).  It agrees with torch bit for bit where the arithmetic is
 * exact, and only to within rounding elsewhere (tests/test_native_eval_host.py holds both comparisons).
 *   void       a pixel is void if its label equals ignore_index or is >= C;
 *   REFUSED    image b is refused, exactly as in mu_pil_resize_u8_nhwc, if H_b or W_b lies outside [1, max_h] / [1, max_w], if
 *              offsets[b] < 0 or if offsets[b+1] - offsets[b] < H_b * W_b: valid[b] = 0, nothing of it is read, it adds nothing to
 *              confusion, its img_counts are zero and its class-map bytes are not written;
 *   img_counts int32 [B][3][C], overwritten: I_c, P_c, L_c with the meaning of mu_sem_eval (P counts every pixel, I and L only the
 *              non-void ones);
 *   confusion  int64 [C+1][C], ADDED TO: row = the label, or C for void; column = pred;
 *   valid      uint8 [B];
 *   classes_or_null  uint8, laid out like labels with the same offsets: pred at native resolution (what a labelIds PNG submission is made
 *              from).  Bytes between two images (offsets that leave gaps) are never written.
 * Integer atomics only: every output is bit-identical from run to run.  Two launches (image descriptors into the workspace, then one
 * workgroup per MU_SEM_NATIVE_TILE_H x MU_SEM_NATIVE_TILE_W tile of the bounds), stream-ordered, no host synchronisation, capturable.  A
 * workgroup stages the source window of its tile in LDS as fp32 where C * (window pixels | 1) * 4 <= min(MU_SEM_NATIVE_WINDOW_BYTES,
 * C * (h * w | 1) * 4) =: S and reads the same taps from global memory otherwise; it keeps the (C+1) x C counters in LDS where
 * (3 * C + ceil((C + 1) * C / 2)) * 4 + S <= MU_SEM_NATIVE_LDS_BYTES and adds one 64-bit global atomic per pixel otherwise.  Every path gives
 * the same results.
 * Limits: B >= 1, 1 <= C <= 256 (labels and the class map are bytes), h, w >= 1, h * w <= 65536 (mu_sem_eval_native_supported, else
 * MU_ERR_SHAPE), 1 <= max_h, max_w <= 16384.  A null pointer (classes_or_null apart), a workspace that is not 8-byte aligned, a scalar
 * outside the limits, inner < 1 or a dtype other than MU_F32 / MU_F16: MU_ERR_ARG; a grid beyond 2^31 - 1 tiles: MU_ERR_SHAPE; a short
 * workspace: MU_ERR_WORKSPACE; all before the first launch.  mu_sem_eval_native_supported and mu_sem_eval_native_workspace_bytes are host
 * only; the latter is 0 for unsupported arguments. */
#define MU_SEM_NATIVE_TILE_H 16
#define MU_SEM_NATIVE_TILE_W 64
#define MU_SEM_NATIVE_WINDOW_BYTES 65536
#define MU_SEM_NATIVE_LDS_BYTES 159744
int mu_sem_eval_native_supported(int C, int h, int w);
long mu_sem_eval_native_workspace_bytes(int B, int C, int h, int w, int max_h, int max_w);
int mu_sem_eval_native(const void* logits, int B, int C, int h, int w, long inner, long outer_stride, long c_stride, long p_stride,
                       const unsigned char* labels, const long* offsets, const int* sizes, int max_h, int max_w, long ignore_index,
                       int* img_counts, long* confusion, unsigned char* valid, unsigned char* classes_or_null, void* workspace,
                       long ws_bytes, int dtype, void* stream);
/* Instance matching: what evaluate_instances / evaluate_panoptic_metrics (ade_panoptic.py:520-586, city_instance.py:451-500) hand to
 * pycocotools and panopticapi, restated from the published algorithms (COCOeval.evaluateImg, maskUtils.iou, panopticapi's
 * pq_compute_single_core) on id maps; no RLE.  Not pinned to those packages.
 * mu_instance_pairs: pred_ids, gt_ids int32 [B,H,W] (the `ids` of mu_instances / mu_dbscan_instances, or any id maps: regions need not
 * be connected); ids outside 1..max_inst_* count as 0.  pairs int32 [B,H*W,3]: every (p, g, intersection) with p >= 1, g >= 0 (g = 0:
 * the pixels of p on no ground truth) and intersection > 0, sorted by (p, g); n_pairs [B] rows are used, the rest is zero.  H*W rows can
 * never overflow.  Integer arithmetic only: bit-identical from run to run. */
int mu_instance_pairs_supported(int H, int W, int max_inst_pred, int max_inst_gt);
long mu_instance_pairs_workspace_bytes(int B, int H, int W, int max_inst_pred, int max_inst_gt);
int mu_instance_pairs(const int* pred_ids, const int* gt_ids, int B, int H, int W, int max_inst_pred, int max_inst_gt, int* pairs,
                      int* n_pairs, void* workspace, long ws_bytes, void* stream);
/* mu_instance_match: pred_table / pred_score / pred_order / pred_count and gt_table / gt_count as mu_instances writes them
 * ([B,max_inst,8], [B,max_inst], [B]).  Row k < K of the outputs is the detection pred_order[b][k] (K <= max_inst_pred: the reference's
 * [:max_queries]).  It is evaluated iff its id is in 1..min(count, max_inst_pred), its class in 1..num_classes-1 and fewer than max_dets
 * earlier rows of the image have that class; a ground truth takes part iff its id is in 1..min(count, max_inst_gt) and its class in
 * 1..num_classes-1, every other ground-truth pixel is void.  thr: T thresholds in (0, 1], fp64, on the HOST (copied into the launch).
 *   det_valid, det_class int32 [B,K], det_score fp32 [B,K];  gt_per_class int32 [B,num_classes];
 *   det_gt int32 [B,T,K], det_iou fp64 [B,T,K]: COCO's greedy matching per (image, class, threshold): for each detection in order, of the
 *     ground truths of its class not yet matched at this threshold the one with the largest iou >= min(t, 1 - 1e-10), the later
 *     (higher id) of equal ones; iou = double(i) / double(a_p + a_g - i), one correctly rounded division.  0 = no match;
 *   pq_gt int32, pq_iou fp64, pq_fp int32 [B,K]: the ground truth of the same class with double(i) / double(a_p + a_g - i - v_p) > 0.5,
 *     v_p = the detection's overlap with void (at most one exists); pq_fp = 1 for an unmatched detection unless v_p / a_p > 0.5;
 *   overflow int32 [B]: a count exceeds its max_inst, the results of that image are unspecified.
 * Rows that are not evaluated are zero; every output byte is written.  H*W <= 65536, 1 <= max_inst_* <= 4096, 1 <= num_classes <= 1024,
 * 1 <= K <= max_inst_pred, max_dets >= 1, 1 <= T <= 32, else MU_ERR_SHAPE.  The *_supported / *_workspace_bytes queries are host only. */
int mu_instance_match_supported(int H, int W, int max_inst_pred, int max_inst_gt, int num_classes, int K, int max_dets, int T);
long mu_instance_match_workspace_bytes(int B, int K);
int mu_instance_match(const int* pairs, const int* n_pairs, const int* pred_table, const float* pred_score, const int* pred_order,
                      const int* pred_count, const int* gt_table, const int* gt_count, int B, int H, int W, int max_inst_pred,
                      int max_inst_gt, int num_classes, int K, int max_dets, const double* thr, int T, int* det_valid, int* det_class,
                      float* det_score, int* det_gt, double* det_iou, int* gt_per_class, int* pq_gt, double* pq_iou, int* pq_fp,
                      int* overflow, void* workspace, long ws_bytes, void* stream);
/* mu_coco_match: COCOeval.evaluateImg in full and panopticapi's crowd rules over the pair table of mu_instance_pairs: what
 * `coco_eval.evaluate()` does per image before accumulate() / summarize() (coco_instance.py:361-367, ade_instance.py:441-447).  Inputs,
 * rows that take part, K and max_dets as mu_instance_match (max_dets = the largest of the maxDets ladder), and
 *   gt_crowd int32 [B,max_inst_gt] or NULL (all 0): row g-1 != 0 = ground truth g is iscrowd;
 *   gt_area fp64 [B,max_inst_gt] or NULL (the pixel area of the table): the area of the RANGE test only, never of an IoU;
 *   area_rng fp64 [A][2] on the HOST, lo <= hi, both ends inclusive; thr as mu_instance_match.
 * Per (image, class, range a, threshold t): gtIg[g] = crowd || area < lo || area > hi; the ground truths are visited non-ignored first,
 * ascending id in each group; for each detection in order: iou = min(t, 1 - 1e-10), m = none; for each g: skip if matched at (a, t) and
 * not crowd; stop if m is non-ignored and g ignored; skip if iou(d, g) < iou; else iou = iou(d, g), m = g (of equal IoUs the later
 * wins).  iou = double(i) / double(a_p + a_g - i), against a crowd ground truth double(i) / double(a_p).
 *   det_valid, det_class, det_rank int32 [B,K] (rank among the evaluated rows of the class in the image, from 0), det_score fp32 [B,K];
 *   det_gt int32, det_iou fp64, det_ignore uint8 [B,A,T,K]: det_ignore = gtIg[m], or for an unmatched detection a_p < lo || a_p > hi;
 *   gt_counted int32 [B,A,num_classes]: the non-ignored ground truths (npig);
 *   pq_gt_per_class int32 [B,num_classes], pq_gt, pq_iou, pq_fp [B,K]: as mu_instance_match, but a crowd ground truth is neither a
 *     candidate nor counted, and pq_fp = 0 if (v_p + i_crowd) / a_p > 0.5, i_crowd = the overlap with the crowd ground truth of the
 *     detection's class that has the highest id;  overflow int32 [B].
 * Rows that are not evaluated are zero; every output byte is written.  Limits of mu_instance_match and 1 <= A <= 4, else MU_ERR_SHAPE;
 * a threshold outside (0, 1], lo > hi or a NaN in thr / area_rng: MU_ERR_ARG, before any launch. */
int mu_coco_match_supported(int H, int W, int max_inst_pred, int max_inst_gt, int num_classes, int K, int max_dets, int T, int A);
long mu_coco_match_workspace_bytes(int B, int K);
int mu_coco_match(const int* pairs, const int* n_pairs, const int* pred_table, const float* pred_score, const int* pred_order,
                  const int* pred_count, const int* gt_table, const int* gt_count, const int* gt_crowd_or_null,
                  const double* gt_area_or_null, int B, int H, int W, int max_inst_pred, int max_inst_gt, int num_classes, int K,
                  int max_dets, const double* thr, int T, const double* area_rng, int A, int* det_valid, int* det_class, int* det_rank,
                  float* det_score, int* det_gt, double* det_iou, unsigned char* det_ignore, int* gt_counted, int* pq_gt_per_class,
                  int* pq_gt, double* pq_iou, int* pq_fp, int* overflow, void* workspace, long ws_bytes, void* stream);
/* COCO run-length masks: what mask_to_rle / maskUtils.encode make of every prediction (city_instance.py:399-403, coco_instance.py:351,397)
 * and annToMask (coco_instance.py:63) reads, restated from the published maskApi.c (rleEncode, rleDecode, rleToString, rleArea).
 * Format.  A mask [H,W] is read COLUMN-major: position j = x * H + y, N = H * W.  counts = the lengths of alternating runs, starting with
 * a run of zeros (which may be 0 long): with the boundaries b_0 < .. < b_{m-1} (m even; the positions where the value changes, N included
 * if the mask ends in a one) counts = [b_0, b_1 - b_0, ..], closed by N - b_{m-1} iff b_{m-1} < N; an empty mask is [N].  area = the sum
 * of the odd-indexed counts.  String: count i contributes x = counts[i], for i > 2 x = counts[i] - counts[i-2], as the characters
 * 48 + (c | 0x20 if more), c = x & 0x1f, x >>= 5 (arithmetic), more = (c & 0x10) ? x != -1 : x != 0, until more is false.
 * mu_rle_encode: ids int32 [B,H,W] (any id map: it partitions the image, so all rows of an image are encoded in one pass over it);
 * sel int32 [B,K]: row k encodes the mask ids == sel[b][k]; 0 or an id outside 1..max_id gives an EMPTY row (no counts, no characters,
 * area 0), an id that does not occur gives [N].  The non-zero ids of a row of sel are distinct (of equal ones the first row gets the mask,
 * the others [N]).  With L = 2 * H * W + K:
 *   offsets int32 [B,K+1], counts int32 [B,L]: row k's counts are counts[b][offsets[b][k] .. offsets[b][k+1]);
 *   area int32 [B,K];  str_offsets int32 [B,K+1], str_bytes uint8 [B,4*L] (4-byte aligned): row k's string likewise.  Every byte past the
 *   used part is 0.
 * L counts and 4 * L characters always suffice: at most two events per boundary, one closing count per row, |x| <= 65536 is 4 characters.
 * H*W <= 65536, 1 <= K <= 4096, 1 <= max_id <= 65536, else MU_ERR_SHAPE.  Stream-ordered, no host synchronisation, integer arithmetic
 * only: bit-identical from run to run.  The *_supported / *_workspace_bytes queries are host only (0 bytes for unsupported shapes).
 * mu_rle_decode: offsets int32 [B,K+1] and counts int32 [B,counts_per_image] as above (counts_per_image = L for the output of
 * mu_rle_encode; annotation files may hold more) -> ids int32 [B,H,W]: the largest k + 1 over the valid rows k whose mask covers the
 * pixel, else 0 (overlapping rows are legal); valid int32 [B,K] = 1 iff the row's offsets lie in order inside the image's counts, no
 * count is negative and they sum to exactly H*W.  An invalid or empty row paints nothing.  Parsing strings is host work. */
int mu_rle_encode_supported(int H, int W, int K, int max_id);
long mu_rle_encode_workspace_bytes(int B, int H, int W, int K, int max_id);
int mu_rle_encode(const int* ids, const int* sel, int B, int H, int W, int K, int max_id, int* offsets, int* counts, int* area,
                  int* str_offsets, unsigned char* str_bytes, void* workspace, long ws_bytes, void* stream);
int mu_rle_decode_supported(int H, int W, int K);
int mu_rle_decode(const int* offsets, const int* counts, int B, int H, int W, int K, long counts_per_image, int* ids, int* valid,
                  void* stream);
/* COCO annotations to masks and training targets: what coco_instance.py:52-83, 331-338 do on the host -- annToMask of every annotation
 * (rleFrPoly per polygon, their union; crowd annotations carry an RLE), cv2.resize(.., INTER_NEAREST) of every mask, torch.sum over them --
 * from the PARSED segmentation fields.  Restated from the published maskApi.c / coco.py, not pinned to pycocotools; this text is the
 * specification.  Masks are read column-major: position p = x * h + y, N = h * w.
 * Polygon (k >= 1 points xy[2j], xy[2j+1], fp64) -> toggle positions (rleFrPoly):
 *   1. X[j] = (int)(5.0 * xy[2j] + .5), Y[j] likewise (C truncation toward zero); X[k] = X[0], Y[k] = Y[0].
 *   2. Edge j = 0..k-1: xs, xe, ys, ye = X[j], X[j+1], Y[j], Y[j+1]; dx = |xe - xs|, dy = |ys - ye|;
 *      flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye); if flip, the two ends are swapped.
 *   3. dx >= dy: s = (double)(ye - ys) / dx; for d = 0..dx: t = flip ? dx - d : d, u = t + xs, v = (int)((ys + s * t) + .5).
 *      Otherwise: s = (double)(xe - xs) / dy; for d = 0..dy: t = flip ? dy - d : d, v = t + ys, u = (int)((xs + s * t) + .5).
 *      So the points run from the edge's original start to its original end; a degenerate edge (dx = dy = 0) emits (xs, ys).  Every
 *      fp64 operation is rounded on its own, in the order written: NO fused multiply-add.
 *   4. Over the concatenated points, every i >= 1 with u[i] != u[i-1] (no wrap-around from the last point to the first; the predecessor
 *      of an edge's first point is the previous edge's last emitted point, by that edge's own formula):
 *      xd = (double)(u[i] < u[i-1] ? u[i] : u[i] - 1); xd = (xd + .5) / 5.0 - .5; skipped if floor(xd) != xd, xd < 0 or xd > w - 1;
 *      yd = (double)(v[i] < v[i-1] ? v[i] : v[i-1]); yd = (yd + .5) / 5.0 - .5, clamped to [0, h], then ceil;
 *      the toggle is a = (int)xd * h + (int)yd.
 *   5. Position p < N of the polygon's mask is set iff an odd number of toggles is <= p (equal to maskApi's sort, difference and merge
 *      of zero-length runs).
 * Annotation a = the polygons ann_poly_offsets[a] .. ann_poly_offsets[a+1] (polygon q = the points poly_offsets[q] .. poly_offsets[q+1]
 * of xy; a polygon without points adds nothing), OR-ed, or -- where its range of rle_counts, ann_rle_offsets[a] .. ann_rle_offsets[a+1],
 * is not empty -- one RLE at the image's size, whose toggles are the prefix sums of its counts without the last.  The annotations
 * img_ann_offsets[b] .. img_ann_offsets[b+1] belong to image b of size (h, w) = sizes[b][0..1] (int32 [B,2], on the device like every
 * array here): the images of one call have sizes of their own.  A row is INVALID (valid = 0, area = 0, paints nothing) if a coordinate
 * is not finite or |5 x + .5| >= 2^24; a polygon has more than max_points upsampled points (sum of max(dx, dy) + 1 over its edges); a
 * count is negative or the counts do not sum to h * w; h < 1, w < 1 or h * w > 2^19; it has polygons and counts; or its offsets are out
 * of order or out of range.
 * Outputs at (Ho, Wo), sampled as mu_resize_nearest_u8 does (sx[j] = min(floor(j * (1.0 / (Wo / (double)w))), w - 1), rows likewise;
 * out[i][j] = mask[sy[i]][sx[j]]):
 *   cover int64 [B,Ho,Wo]   how many valid annotations of the image cover the pixel (the reference's combined_mask, as the loss takes it);
 *   ids   int32 [B,Ho,Wo]   the largest (row within the image + 1) among them, else 0: the rule of mu_rle_decode;
 *   masks uint8 [A,Ho,Wo]   per annotation (may be NULL);  area int32 [A]: the set bits at the ORIGINAL size (rleArea);  valid int32 [A].
 * Every output byte is written (cover and ids are zeroed here).  Ho * Wo <= 65536 and 1 <= max_points <= 2^21, else MU_ERR_SHAPE
 * (mu_coco_masks_supported: host only).  B >= 1; A = 0 is legal (xy / rle_counts may be NULL where n_points / n_counts is 0, area / valid
 * where A is 0).  One workgroup per annotation with both bitmaps in LDS: mu_coco_masks_workspace_bytes is 0 today and `workspace` may be
 * NULL; the arguments are there so that a build with the union bitmap in global memory keeps this ABI.  Stream-ordered, no host
 * synchronisation, integer atomics only: bit-identical from run to run. */
int mu_coco_masks_supported(int Ho, int Wo, int max_points);
long mu_coco_masks_workspace_bytes(int B, int A, int Ho, int Wo);
int mu_coco_masks(const double* xy, const int* poly_offsets, const int* ann_poly_offsets, const int* rle_counts, const int* ann_rle_offsets,
                  const int* img_ann_offsets, const int* sizes, int B, int A, int P, long n_points, long n_counts, int Ho, int Wo,
                  int max_points, long* cover, int* ids, unsigned char* masks_or_null, int* area, int* valid, void* workspace,
                  long ws_bytes, void* stream);
/* f4: uint8 HWC image bytes [npix, C] -> [0,1] floats in the NHWC compute layout [npix, Cp] (ToTensor, ade_semantic.py:85) */
int mu_u8_to_nhwc(const unsigned char* src, void* dst, long npix, int C, int Cp, int dtype, void* stream);
/* f4, resize half: the sample preparation of the reference datasets on the device.  src: decoded image bytes [B][Hs][Ws][C] (C <= 4, as
 * cv2.imread leaves them) of any size -> cv2.resize(.., (Wd, Hd), interpolation=cv2.INTER_LINEAR) (ade_semantic.py:72; OpenCV 4.10's
 * 8-bit fixed-point algorithm incl. its 2x2 INTER_AREA shortcut, restated: cv2 is not vendored by the reference), channels 0 and 2
 * swapped when swap_rb != 0 (cv2.COLOR_BGR2RGB, :65), then ToTensor (:85): dst [B][Hd][Wd][Cp] = byte / 255 in the NHWC compute layout,
 * zero channel padding.  u8_out (may be NULL) receives the resized bytes [B][Hd][Wd][C] themselves. */
int mu_resize_u8_nhwc(const unsigned char* src, int B, int Hs, int Ws, int C, int swap_rb, void* dst, unsigned char* u8_out, int Hd, int Wd,
                      int Cp, int dtype, void* stream);
/* the label map: uint8 [B][Hs][Ws] -> int64 [B][Hd][Wd] = torch.from_numpy(cv2.resize(mask, (Wd, Hd), interpolation=cv2.INTER_NEAREST)).long()
 * (:73,78): source index min(floor(d * scale), n - 1) */
int mu_resize_nearest_u8(const unsigned char* src, int B, int Hs, int Ws, long* dst, int Hd, int Wd, void* stream);
/* f4, the Pillow half: a RAGGED batch of decoded image bytes -> the network input by Pillow's ANTIALIASED bilinear resample, i.e.
 * T.ToPILImage() -> T.Resize((Hd, Wd)) -> T.ToTensor() (coco_instance.py:43-47,68) = Image.resize((Wd, Hd), Image.BILINEAR).  Restated from
 * Pillow's Resample.c and pinned to the bytes of Pillow 12.2.0 (tests/golden/pil/); this text is the specification.
 * Coefficients of one axis, n_in -> n_out, in fp64 with every operation rounded on its own (NO fused multiply-add), in this order:
 *   scale = n_in / n_out;  fs = max(scale, 1.0);  support = fs;  ss = 1.0 / fs;  ksize = 2 * ceil(support) + 1
 *   output index xx:  center = (xx + 0.5) * scale
 *                     xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), n_in);  n = xmax - xmin
 *                     w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|) for x < n;  ww = w[0] + w[1] + .. in ascending x;
 *                     w[x] /= ww if ww != 0;  k[x] = (int)(0.5 + w[x] * 2^22)              ((int) = C truncation; every argument is >= 0)
 * One pass: out = clamp((2^21 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255) in int32 (no overflow within the limits below).
 * Two passes: horizontal, then vertical, the intermediate ROUNDED TO uint8 (an axis that keeps its size has k = {2^22, 0}: the identity,
 * as Pillow skipping that pass).  Channels are independent; C is 1 or 3 (Pillow resizes RGBA premultiplied: refused).  Then ToTensor:
 * dst [B][Hd][Wd][Cp] = float(byte) / 255.0f by IEEE division, rounded to nearest even for fp16 storage, padding channels zero -- the rule
 * of mu_u8_to_nhwc.  swap_rb != 0 swaps channels 0 and 2 (cv2.imread bytes).  u8_out (may be NULL) receives the bytes [B][Hd][Wd][C].
 * Image b is the h * w * C bytes at src + offsets[b], (h, w) = sizes[b][0..1]; offsets int64 [B+1] in bytes and sizes int32 [B][2] are
 * DEVICE arrays, image starts need no alignment, and the host passes only the bounds max_h, max_w.  An image is REFUSED (valid[b] = 0, all
 * of its outputs zero, nothing of it read) if h or w lies outside [1, max_h] / [1, max_w]; if h > 100 * w and Hd < h (Pillow 12 resizes
 * those vertically first; h == 100 * w is inside); or if offsets[b] < 0 or offsets[b+1] - offsets[b] < h * w * C.  valid is uint8 [B].
 * Limits: B >= 1, 1 <= max_h, max_w <= 16384, Hd * Wd <= 65536, C in {1, 3}, Cp % 32 == 0, Cp >= C, dtype MU_F32 or MU_F16.  A null
 * pointer (u8_out apart), a scalar outside the limits or a workspace shorter than mu_pil_resize_workspace_bytes (host only; -1 for
 * arguments outside the limits) returns MU_ERR_ARG without touching the GPU.  Every output byte is written on every call.  Two launches
 * (coefficient tables into the workspace, then the resample), stream-ordered, no atomics, no host synchronisation: bit-identical from run
 * to run and capturable in a graph. */
long mu_pil_resize_workspace_bytes(int B, int max_h, int max_w, int Hd, int Wd);
int mu_pil_resize_u8_nhwc(const unsigned char* src, const long* offsets, const int* sizes, int B, int C, int max_h, int max_w, int swap_rb,
                          void* dst, unsigned char* u8_out, unsigned char* valid, int Hd, int Wd, int Cp, int dtype, void* workspace,
                          long workspace_bytes, void* stream);
/* f4, the cv2 half for RAGGED batches: the sample preparation of the loaders that read with OpenCV, whose images and maps have sizes of
 * their own (ade_semantic.py:65-78, ade_panoptic.py:89, city_semantic.py:84-88, city_instance.py:81-106, city_panoptic.py:97-115,
 * coco_semantic.py:70-84, coco_panoptic.py:70-95).  The three entry points below take a ragged batch exactly as mu_pil_resize_u8_nhwc
 * does: ONE flat device buffer, offsets int64 [B+1] in BYTES and sizes int32 [B][2] = (h, w) as DEVICE arrays, and from the host only the
 * bounds max_h, max_w.  The resize rules are those of mu_resize_u8_nhwc / mu_resize_nearest_u8 (one piece of code, csrc/cv2_rule.h), with
 * the scales derived on the device per image as scale = 1.0 / ((double)Wd / (double)w), two separately rounded fp64 operations, rows
 * likewise: exact against the restated OpenCV 4.10 rule (oracle/cv2_resize_oracle.py), NOT pinned to bytes of a real cv2 build.
 * Common to the three: image b is the bytes [offsets[b], offsets[b+1]) of the buffer and is REFUSED (valid[b] = 0, valid is uint8 [B],
 * none of its bytes read) if h or w lies outside [1, max_h] / [1, max_w], if offsets[b] < 0 or is not a multiple of the element size, or
 * if offsets[b+1] - offsets[b] < h * w * (bytes per pixel); a refused image does not affect its neighbours.  Every output element is
 * written on every call.  One launch each, stream-ordered, no atomics, no workspace, no host synchronisation: bit-identical from run to
 * run and capturable in a graph.  Limits (mu_cv2_ragged_supported, host only: MU_OK or MU_ERR_SHAPE): B >= 1, 1 <= max_h, max_w, Hd, Wd <= 16384,
 * B * ceil(Hd * Wd / 256) < 2^31.  Refusal order as for the post-processing entry points: a null pointer (optional ones apart), B < 1 or
 * an unknown dtype / kind or otherwise invalid scalar is MU_ERR_ARG; then a shape outside the limits is MU_ERR_SHAPE; a refused call
 * enqueues nothing. */
int mu_cv2_ragged_supported(int B, int max_h, int max_w, int Hd, int Wd);
/* Images: for every valid image the bytes (u8_out [B][Hd][Wd][C], may be NULL) and dst [B][Hd][Wd][Cp] are exactly what
 * mu_resize_u8_nhwc(image alone as [1,h,w,C], .., Hd, Wd, Cp, dtype) produces -- the 11-bit fixed-point INTER_LINEAR with the left / right
 * tap collapse and clamped rows, the `& 0xFF` narrowing, the INTER_AREA shortcut where w == 2 * Wd && h == 2 * Hd (decided per image),
 * swap_rb != 0 swapping channels 0 and 2 of a 3-channel image, dst = byte / 255 by IEEE division rounded to the storage type, padding
 * channels +0.  All outputs of a refused image are +0.  C in {1, 3}, Cp % 8 == 0, Cp >= C (else MU_ERR_SHAPE); dtype MU_F32 or MU_F16. */
int mu_cv2_resize_ragged_u8_nhwc(const unsigned char* src, const long* offsets, const int* sizes, int B, int C, int max_h, int max_w,
                                 int swap_rb, void* dst, unsigned char* u8_out, unsigned char* valid, int Hd, int Wd, int Cp, int dtype,
                                 void* stream);
/* Id maps: dst int64 [B][Hd][Wd] = torch.from_numpy(cv2.resize(map, (Wd, Hd), interpolation=cv2.INTER_NEAREST)).long() with the
 * Cityscapes clean-ups folded in.  kind names the element of the map: MU_MAP_U8 (IMREAD_GRAYSCALE label maps), MU_MAP_U16 (instanceIds
 * PNGs under IMREAD_UNCHANGED), MU_MAP_I32 (signed; the maps the COCO loaders build), MU_MAP_RGB8 (three bytes per pixel, value =
 * byte0 + 256 * byte1 + 65536 * byte2: rgb2id of an RGB image) and MU_MAP_BGR8 (the same with bytes 0 and 2 exchanged: rgb2id of
 * cv2.imread bytes -- the channel swap is a fifth kind, not a flag).  U16 / I32 elements are little-endian, and src and every
 * offsets[b] must be multiples of the element size (2 / 4; a misaligned src is MU_ERR_ARG, a misaligned offset refuses that image).
 *   v = map[min(floor(i * ify), h - 1)][min(floor(j * ifx), w - 1)]           ifx, ify as in mu_resize_nearest_u8
 *   divisor > 1:    v = floor(v / divisor)     (Python's //: -1 // 1000 = -1; it commutes with the nearest resize, so this is
 *                                               `instance_mask // 1000` before cv2.resize, city_instance.py:85)
 *   n_classes > 0:  v = fill unless 0 <= v < n_classes     (np.where((m >= 0) & (m < 19), m, 255), city_semantic.py:84;
 *                                                           mask[mask >= n] = 255, city_instance.py:106)
 * Every element of a refused image equals fill.  divisor >= 1 and n_classes >= 0, else MU_ERR_ARG. */
#define MU_MAP_U8 0
#define MU_MAP_U16 1
#define MU_MAP_I32 2
#define MU_MAP_RGB8 3
#define MU_MAP_BGR8 4
int mu_cv2_nearest_ragged(const void* src, const long* offsets, const int* sizes, int kind, int B, int max_h, int max_w, int divisor,
                          int n_classes, long fill, long* dst, unsigned char* valid, int Hd, int Wd, void* stream);
/* The COCO panoptic target (coco_panoptic.py:70-95; its semantic half is coco_semantic.py:70-86): png is a ragged batch of 3-byte
 * pixels; id = rgb2id of the nearest-sampled pixel (byte0 + 256 * byte1 + 65536 * byte2; swap_rb != 0 exchanges bytes 0 and 2:
 * cv2.imread bytes).  The segments of image b are rows img_seg_offsets[b] .. img_seg_offsets[b+1] (int32 [B+1]) of seg_ids / seg_labels
 * (int32 [S] each), their ids STRICTLY ASCENDING: the packer keeps the last-listed entry of a duplicated id, as the reference's loop
 * over segments_info does, and sorts.  If id is among the image's seg_ids: semantic = its label, instance = id; otherwise both are 0,
 * the reference's zero-initialised maps (an id-0 pixel is 0 / 0 unless id 0 is listed).  Outputs int64 [B][Hd][Wd] each.  An image is
 * REFUSED also if its table is not strictly ascending, has more than MU_PANOPTIC_SEG_MAX rows (the table is held in LDS: 8 KiB of a
 * workgroup's default 64 KiB, no grant needed), or its table offsets are out of order or outside [0, S]; then semantic = fill and
 * instance = 0.  S = 0 is legal (seg_ids / seg_labels may then be NULL); S < 0 is MU_ERR_ARG. */
#define MU_PANOPTIC_SEG_MAX 1024
int mu_panoptic_targets(const unsigned char* png, const long* offsets, const int* sizes, const int* seg_ids, const int* seg_labels,
                        const int* img_seg_offsets, int B, int S, int max_h, int max_w, int swap_rb, long fill, long* semantic,
                        long* instance, unsigned char* valid, int Hd, int Wd, void* stream);
/* f2: optim.AdamW step (ade_semantic.py:379,401) for every parameter in one launch.  table: device array of `ntensors` entries
 * {float* p; const float* g; float* m; float* v; long n; long step;} (48 bytes; g may be NULL = no gradient this step; step = that
 * tensor's own count of attempted updates including this one, torch keeps one counter per parameter); block_tensor/block_chunk:
 * per-block (tensor index, chunk index) with chunks of mu_adamw_chunk() elements.  Gradients are multiplied by grad_scale_inv, or by
 * 1 / *grad_scale when grad_scale (a DEVICE float, torch.cuda.amp.GradScaler's scale) is given.
 * Overflow protocol, all on the device (no host sync): found_inf (device float, may be NULL) != 0 makes the launch update NOTHING;
 * with check_finite == 1 the entry point first sets *found_inf itself (0, then 1 if any gradient element is inf / NaN); check_finite == 2
 * only ORs this table's gradients into *found_inf and updates nothing (several parameter groups: check all, then update all);
 * skipped (device int[ntensors], may be NULL) counts the skipped steps per tensor and is subtracted from `step` in the bias
 * corrections, so a skipped step leaves parameters, moments AND the effective step count untouched. */
int mu_adamw_chunk(void);
int mu_adamw_multi(const void* table, const int* block_tensor, const int* block_chunk, int nblocks, int ntensors, float lr, float beta1,
                   float beta2, float eps, float weight_decay, float grad_scale_inv, const float* grad_scale, float* found_inf,
                   int check_finite, int* skipped, void* stream);

/* ---- measurement aid (bench.py; not on the model's path) ------------------------------------- */
/* Clock / matrix-rate probe: one launch of `nblk` 256-thread blocks, every wave issuing iters * 16 register-only
 * v_mfma_f32_16x16x32_f16 on random operands, stamped once around the loop.  stamps [nblk][2] uint64 = {d s_memtime (shader
 * cycles), d s_memrealtime (100 MHz ticks)} -> clock the chip holds under a dense fp16 MFMA load = 100 MHz * [0]/[1]
 * (MI355X_MICROARCH.md "DVFS give-back" item 6).  sink: nblk * 256 floats of scratch.  The reference has no counterpart: it is what
 * makes two bench lines from two boxes of a pool comparable. */
int mu_clock_probe(void* stamps, void* sink, int nblk, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MASKUNET_HIP_H */
