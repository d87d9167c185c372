/*
 * sedcrnn.h — flat C ABI of libsedcrnn.so (hand-written HIP for gfx950 / MI355X).
 *
 * This is the drop-in boundary of the SEDnet hot path.  The
 * reference (noamzilo/sed-crnn) has no FFI of its own for this path: it reaches
 * native code only through torch.nn modules, so each entry point below cites the
 * reference call site whose ATen kernel it replaces (paths are relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; all tensors are fp32 device memory unless noted;
 *   - the CALLER owns every buffer (inputs, outputs, workspace); the library never
 *     allocates or frees device memory and keeps no pointer past return;
 *   - every launch is asynchronous on the hipStream_t passed as `stream`
 *     (void*; NULL = the default stream); no entry synchronises the device and the entries are
 *     re-entrant (no mutable process state) — with TWO exceptions: the measurement-only
 *     sed_prof_* group at the end of this header, which is off by default, and a per-thread,
 *     per-device cache of hipEvent_t host objects (at most 15 per calling thread and device,
 *     timing disabled) that sed_net_backward creates on its first call WITH an aux_stream to order
 *     the two streams; they hold no device memory, are never shared between threads, and live
 *     until the process exits (a caller that passes aux_stream = NULL never creates them);
 *   - return value: 0 = ok, <0 = argument / shape error, >0 = hipError_t.  The message
 *     of the last failure on the calling thread is sed_last_error_string().
 *
 * Activation layout inside the conv stack is channels-last: act[b][t][f][c]
 * ("(seq, mel, chan)"), c contiguous.  The network input keeps the reference layout
 * x[b][cin][f][t] (sed.py:105) and the GRU input keeps the reference feature order
 * feat = c*F + f (sed.py:108-110), so reference state_dicts load unchanged.
 */
#ifndef SEDCRNN_H
#define SEDCRNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SED_MAX_CONV 4
#define SED_MAX_GRU 4
#define SED_MAX_DENSE 4

/* ───────────── library ───────────── */
int sed_version(void);                       /* 10000*major + 100*minor + patch */
const char* sed_last_error_string(void);     /* thread-local, never NULL */

/* ───────────── conv 3x3, stride 1, zero pad 1 (sed.py:88,107; crnn_lightning.py:47) ─────────────
 * w_oihw is the reference/PyTorch weight [Cout][Cin][3][3] (kh over mel, kw over time).
 * sed_conv3x3_pack_weights lays it out for the kernels:
 *   wp_fwd  [9][Cout][Cin]  tap-major, ci contiguous           (forward)
 *   wp_dgrad[9][Cin][Cout]  taps flipped, ci/co swapped        (data gradient = conv of dy)
 * either output pointer may be NULL. */
int sed_conv3x3_pack_weights(const float* w_oihw, float* wp_fwd, float* wp_dgrad,
                             int Cout, int Cin, void* stream);

/* Number of per-block partial rows sed_conv3x3_fwd writes into `stat_partials`
 * ([rows][2][Cout]: sum and sum of squares of the outputs, pre-BN, bias included). */
int sed_conv3x3_stat_rows(int B, int Cin, int F, int T, int Cout, int x_is_nchw);

/* How a shape would run, read from the plan the launches read (host only, works without a GPU).  which = 0: the plan of
 * sed_conv3x3_fwd_ex and of the data gradients; which = 1: the plan of sed_conv3x3_bn_relu_pool_eval (x_is_nchw must be 0).
 * out[8] = {kind (0 small-channel kernel, 1 MFMA kernel, -1 none; the rest is 0 then), TT, FT (time rows x mel columns of a
 * block tile), nft (mel tiles), nct (32-wide output-channel tiles per workgroup; 0 on the small path), tblocks (= ceil(T/TT)),
 * rows (statistic partial rows = B * tblocks * nft; the tile (b, tb, fi) writes row (b * tblocks + tb) * nft + fi),
 * xcd_order (1: the MFMA kernel walks its tiles in the XCD-aware order, i.e. B % 8 == 0)}. */
int sed_conv3x3_plan(int B, int Cin, int F, int T, int Cout, int x_is_nchw, int which, int* out);

/* y[b][t][f][co] = bias[co] + sum_{kh,kw,ci} w[co][ci][kh][kw] x[.. f+kh-1, t+kw-1 ..]
 * x_is_nchw=1: x is the network input [B][Cin][F][T]; 0: x is channels-last [B][T][F][Cin].
 * wp = wp_fwd from sed_conv3x3_pack_weights ([9][Cout][Cin]).
 * bias may be NULL; stat_partials may be NULL (no statistics). */
int sed_conv3x3_fwd(const float* x, int x_is_nchw, const float* wp, const float* bias,
                    float* y, float* stat_partials,
                    int B, int Cin, int F, int T, int Cout, void* stream);

/* EXPERIMENT, explicit opt-in (never the default, never what bench.py reports as `value`): `mode` 1 runs the MFMA path
 * (Cin%32 == 0, Cout%32 == 0) on a 3-term bf16 split — x*w ~ x_hi*w_hi + x_hi*w_lo + x_lo*w_hi with fp32 accumulation on
 * v_mfma_f32_32x32x16_bf16: 5.3x the matrix rate of the exact-fp32 MFMA at a relative error of ~4e-6 on a K = 1152 sum
 * (exact fp32: 3e-7).  mode 0 = the exact fp32 kernels (identical to the entries above).  Weights for mode m must be
 * packed with sed_conv3x3_pack_weights_ex(..., m); shapes outside the MFMA path fall back to mode 0 in both entries. */
int sed_conv3x3_pack_weights_ex(const float* w_oihw, float* wp_fwd, float* wp_dgrad, int Cout, int Cin, int mode, void* stream);
int sed_conv3x3_fwd_ex(const float* x, int x_is_nchw, const float* wp, const float* bias, float* y, float* stat_partials,
                       int B, int Cin, int F, int T, int Cout, int mode, void* stream);

/* Weight gradient (aten::convolution_backward, reached from loss.backward() sed.py:137).
 * dw_oihw[co][ci][kh][kw] = sum_pos x[pos+tap][ci] * dy[pos][co].  dy is channels-last.
 * workspace: sed_conv3x3_wgrad_workspace_bytes(). Deterministic (fixed-order slab reduce). */
size_t sed_conv3x3_wgrad_workspace_bytes(int B, int Cin, int F, int T, int Cout);
int sed_conv3x3_wgrad(const float* x, int x_is_nchw, const float* dy, float* dw_oihw,
                      void* workspace, int B, int Cin, int F, int T, int Cout, void* stream);

/* mode 1 (EXPERIMENT, as sed_conv3x3_fwd_ex): the MFMA path on the 3-term bf16 split; other shapes run mode 0.
 * mode | SED_WGRAD_ZERO_ROW_CLEAN: the exact-fp32 MFMA kernel reads out-of-image rows from a zero-filled row at the START of
 * the workspace (sed_conv3x3_wgrad_zero_row_bytes(), 0 for shapes that have none), which the entry clears with a memset on
 * `stream` in every call — unless this flag says the caller keeps those bytes zero (nothing ever writes them): a plan that
 * calls the entry every step clears them once, off its critical chain, and saves the memset node in front of each launch.
 * mode | SED_WGRAD_DIRECT: mel extents that cut into 40- or 32-column tiles run the position-contiguous kernel in the Winograd
 * domain by default (F(2x2,3x3): 16 products per 2x2 tile and channel pair instead of 36, dW = G^T dU G applied by the slab
 * reduction; exact-fp32 MFMA arithmetic, see wino.hip); this flag keeps the direct 36-product form (A/B measurements, tests). */
#define SED_WGRAD_ZERO_ROW_CLEAN 0x100
#define SED_WGRAD_DIRECT 0x200
size_t sed_conv3x3_wgrad_zero_row_bytes(int B, int Cin, int F, int T, int Cout);
int sed_conv3x3_wgrad_ex(const float* x, int x_is_nchw, const float* dy, float* dw_oihw,
                         void* workspace, int B, int Cin, int F, int T, int Cout, int mode, void* stream);

/* Inference (run_epoch with optim=None, sed.py:128-141; `model.eval()`): conv3x3 + BatchNorm2d on RUNNING statistics + ReLU +
 * MaxPool2d((1,2)) (sed.py:107) in ONE launch.  BatchNorm is a per-channel affine map there, so it is folded on the way in:
 * sed_conv3x3_pack_weights_bn_folded writes the MFMA fragments of w * scale[co] and bias_folded = bias * scale + shift with
 * scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale; the kernel's epilogue applies ReLU and the time
 * pool to its accumulators and writes only the pooled tensor [B][T/2][F][Cout] (channels-last; a ragged last frame is dropped
 * like nn.MaxPool2d does): in + 0.5 out bytes instead of in + 2.5 out.  x [B][T][F][Cin] channels-last.
 * _supported: the 128-wide exact-fp32 MFMA tile with an even number of time rows (Cin % 32 == 0, Cout % 128 == 0, mel widths
 * whose tile is <= 32 columns: 40 -> 20, 64 -> 32, ...); otherwise use sed_conv3x3_fwd_ex + sed_bn_relu_pool_drop_fwd. */
int sed_conv3x3_bn_relu_pool_eval_supported(int B, int Cin, int F, int T, int Cout);
int sed_conv3x3_pack_weights_bn_folded(const float* w, const float* bias, const float* gamma, const float* beta,
                                       const float* running_mean, const float* running_var, float eps,
                                       float* wf, float* bias_folded, int Cout, int Cin, void* stream);
int sed_conv3x3_bn_relu_pool_eval(const float* x, const float* wp_folded, const float* bias_folded, float* pooled,
                                  int B, int Cin, int F, int T, int Cout, void* stream);
/* bf16 inference (opt-in: sed_net_cfg.conv_mode = 2) — the same block as sed_conv3x3_bn_relu_pool_eval on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Rounded to bf16 (nearest even): the folded weights w * scale[co] (formed in
 * fp32, then rounded; bias_folded stays fp32), the input x (x_is_bf16 = 0: fp32 x rounded while staged; 1: x is bf16 already) and
 * the output after bias + ReLU + pool in fp32.  x [B][T][F][Cin] channels-last -> pooled bf16 [B][T/2][F][Cout] (floor pooling).
 * wf_bf16: 9*Cout*Cin bf16 from sed_conv3x3_bf16_pack_weights_bn_folded (Cout % 32, Cin % 16 == 0).
 * _supported: Cin % 32 == 0, Cout % 64 == 0, T >= 2, any mel width (direct form, tiles of <= 32 mel columns). */
int sed_conv3x3_bf16_eval_supported(int B, int Cin, int F, int T, int Cout);
int sed_conv3x3_bf16_pack_weights_bn_folded(const float* w, const float* bias, const float* gamma, const float* beta,
                                            const float* running_mean, const float* running_var, float eps,
                                            void* wf_bf16, float* bias_folded, int Cout, int Cin, void* stream);
int sed_conv3x3_bf16_bn_relu_pool_eval(const void* x, int x_is_bf16, const void* wf_bf16, const float* bias_folded,
                                       void* pooled_bf16, int B, int Cin, int F, int T, int Cout, void* stream);
/* Data gradient of conv block l (the convolution of dy with wp_dgrad) FUSED with the reduction pass of the BatchNorm / ReLU /
 * max-pool / dropout backward of block l-1 (sed_bn_relu_pool_drop_bwd_reduce below), for the exact-fp32 MFMA shapes:
 * dy [B][T][F][C] -> dx [B][T][F][Cin] = gradient of block l-1's pooled output, and partials [rows][2][Cin] = per-workgroup
 * (sum g, sum g*xhat) of block l-1 — the input of sed_bn_bwd_finalize — formed in the epilogue from block l-1's own forward
 * OUTPUT `pooled` [B][T][F][Cin] (channels-last): it is > 0 exactly where the gradient passes (element kept by the dropout AND
 * ReLU gate open), g = dx / (1-p) there, and the normalised activation at the arg-max is (pooled (1-p) - beta) / gamma.
 * That recovery divides a rounding error of eps |z| by gamma, so with a stored conv output below (conv_out_below != NULL) the
 * channels with |gamma| < |beta| / 64 (and gamma == 0) contribute 0 to sum g*xhat here and MUST be finalised with
 * sed_bn_bwd_finalize_small_gamma, which recomputes exactly those channels from the conv output; sum g is exact for every
 * channel.  conv_out_below [B][Ty][Fy][Cin] is only tested for NULL here, mean / rstd are unused (kept for the signature) (pool_f, pool_t: block l-1's
 * pool, Ty / pool_t == T, Fy / pool_f == F); conv_out_below may be NULL for a block that stores none (the recomputed first
 * block: sed_conv1_bwd_apply_wgrad then supplies dgamma of those channels).  rows = sed_conv3x3_dgrad_bnred_rows(); 0 = shape not supported (use
 * sed_conv3x3_fwd_ex + sed_bn_relu_pool_drop_bwd_reduce).  Replaces a 1.5x re-read of block l-1's conv output. */
int sed_conv3x3_dgrad_bnred_rows(int B, int C, int F, int T, int Cin);
int sed_conv3x3_dgrad_bnred(const float* dy, const float* wp_dgrad, float* dx, float* partials, const float* pooled,
                            const float* gamma, const float* beta, const float* conv_out_below, const float* mean,
                            const float* rstd, float drop_p, int pool_f, int pool_t, int Fy, int Ty,
                            int B, int C, int F, int T, int Cin, void* stream);
/* ---- Winograd F(2x2, 3x3) form of the 128-input-channel convolutions (wino.hip; reference sed.py:88,107, the same nn.Conv2d) ----
 * Exact-fp32 MFMA arithmetic on 16 transformed products per 2x2 output tile instead of 36 (2.25x fewer MFMAs); the transforms'
 * coefficients are 0, +-1 and 1/2, the result differs from the direct kernels' by a few ulp of the accumulated magnitude.
 * Shapes: Cin == 128, Cout % 64 == 0, F and T even, a tile-row patch that fits the LDS, a sequence (T x F x Cin floats) below
 * 2 GiB; sed_conv3x3_wino_rows() = the number of
 * statistic / partial rows ([rows][2][Cout], as sed_conv3x3_fwd) or 0 when the shape is not taken.
 * pack_weights: w [Cout][Cin][3][3] -> uf (forward) and ud (data gradient: flipped taps, channel roles swapped), each
 * sed_conv3x3_wino_packed_floats() floats (16 Cin Cout transformed weights in MFMA fragment order + a zero tail, part of the layout: the
 * kernel's zero padding came from it until the patch DMA's range check took that over); either may be NULL.
 * wino_fwd = sed_conv3x3_fwd on channels-last x; wino_dgrad_bnred = sed_conv3x3_dgrad_bnred (same arguments and outputs). */
int sed_conv3x3_wino_rows(int B, int Cin, int F, int T, int Cout);
/* measurement only (tools/wino_probe.py): buf = 5 device uint64 — prologue / main loop / epilogue ticks of the 100 MHz clock summed
 * over the workgroups of every following Winograd forward / data-gradient launch, the workgroup count, and (wino_dgrad_bnred[_rg]
 * only) the part of the epilogue in front of its exchange barrier; NULL switches it off. */
int sed_conv3x3_wino_phase_ticks(unsigned long long* buf);
size_t sed_conv3x3_wino_packed_floats(int Cout, int Cin);
int sed_conv3x3_wino_pack_weights(const float* w_oihw, float* uf, float* ud, int Cout, int Cin, void* stream);
int sed_conv3x3_wino_fwd(const float* x, const float* uf, const float* bias, float* y, float* stat_partials,
                         int B, int Cin, int F, int T, int Cout, void* stream);
int sed_conv3x3_wino_dgrad_bnred(const float* dy, const float* ud, float* dx, float* partials, const float* pooled,
                                 const float* gamma, const float* beta, const float* conv_out_below, const float* mean,
                                 const float* rstd, float drop_p, int pool_f, int pool_t, int Fy, int Ty,
                                 int B, int C, int F, int T, int Cin, void* stream);
/* inference (= sed_conv3x3_pack_weights_bn_folded + sed_conv3x3_bn_relu_pool_eval): BatchNorm on running statistics folded into the
 * transformed weights and the bias, ReLU + (1,2) time pool in the epilogue (the two time rows of a 2x2 tile are a pooling pair):
 * pooled [B][T/2][F][Cout]; shapes as sed_conv3x3_wino_rows() > 0. */
int sed_conv3x3_wino_pack_weights_bn_folded(const float* w_oihw, const float* bias, const float* gamma, const float* beta,
                                            const float* running_mean, const float* running_var, float eps,
                                            float* uf, float* bias_folded, int Cout, int Cin, void* stream);
int sed_conv3x3_wino_bn_relu_pool_eval(const float* x, const float* uf_folded, const float* bias_folded, float* pooled,
                                       int B, int Cin, int F, int T, int Cout, void* stream);
/* = sed_conv3x3_dgrad_bnred_rg (the first block's weight-gradient sums from the same epilogue); rows = sed_conv3x3_wino_rg_rows().
 * dx may be NULL here: the data gradient itself is then not written (the training plan does so when the first block takes
 * everything it needs from partials and rg_partials: a tensor of the size of the pooled output that nobody would read);
 * partials and rg_partials are the same bit for bit with and without dx. */
int sed_conv3x3_wino_rg_rows(int B, int C, int F, int T, int Cin, int Cin1);
int sed_conv3x3_wino_dgrad_bnred_rg(const float* dy, const float* ud, float* dx, float* partials, const float* pooled,
                                    const float* gamma, const float* beta, const float* mean, const float* rstd, float drop_p,
                                    const float* x1, int Cin1, const unsigned char* argmax_bits, float* rg_partials,
                                    int B, int C, int F, int T, int Cin, void* stream);
/* The same launch when the block below is the recomputed first block with Cin1 = 1 or 2 input channels and pool (1,2)
 * (sed.py:86-92, ch = 1 or 2): the epilogue also forms that block's weight-gradient sums — rg_partials [rows][Cin][1 + 9 Cin1]
 * = (sum g, R_k) per channel and workgroup, R_{(3kh+kw) Cin1 + ci} = sum g~ x[ci][f+kh-1][2t'+sel+kw-1] with sel the arg-max
 * bit — from the network input x1 [B][Cin1][F][2T] and
 * the arg-max bits of sed_conv1_bn_relu_pool_drop_fwd, for sed_conv1_bwd_wgrad_assemble.  Replaces the pass of
 * sed_conv1_bwd_wgrad over dx, the pooled tensor and the bits.  rows = sed_conv3x3_dgrad_bnred_rg_rows(); 0 = not supported. */
int sed_conv3x3_dgrad_bnred_rg_rows(int B, int C, int F, int T, int Cin, int Cin1);
int sed_conv3x3_dgrad_bnred_rg(const float* dy, const float* wp_dgrad, float* dx, float* partials, const float* pooled,
                               const float* gamma, const float* beta, const float* mean, const float* rstd, float drop_p,
                               const float* x1, int Cin1, const unsigned char* argmax_bits, float* rg_partials,
                               int B, int C, int F, int T, int Cin, void* stream);

/* ───────────── BatchNorm2d + ReLU + MaxPool2d + Dropout (sed.py:89-92,107; crnn_lightning.py:48-52) ─────────────
 * Training statistics: reduce the conv partials in a fixed order (double accumulation),
 * write mean/rstd and the fused scale/shift (scale = gamma*rstd, shift = beta - mean*scale),
 * update running_mean / running_var (momentum, unbiased var) like nn.BatchNorm2d.
 * count = B*T*F elements per channel. */
int sed_bn_finalize_train(const float* stat_partials, int rows, int C, double count,
                          const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps,
                          float* mean, float* rstd, float* scale, float* shift, void* stream);
/* The same in two steps, for synchronised BatchNorm across ranks: sums[2C] = (sum x, sum x^2) of this rank's partials;
 * the host all-reduces (SUM) the 2C floats; finalize_from_sums then uses the GLOBAL element count. */
int sed_bn_stat_sums(const float* stat_partials, int rows, int C, float* sums, void* stream);
int sed_bn_finalize_from_sums(const float* sums, int C, double count, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps,
                              float* mean, float* rstd, float* scale, float* shift, void* stream);
/* Eval: scale/shift from the running statistics. */
int sed_bn_finalize_eval(const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, int C,
                         float* scale, float* shift, void* stream);

/* out = dropout(maxpool_{pool_f x pool_t}(relu(scale*y + shift))).
 * y [B][T][F][C] channels-last.  out_tcf=0: out [B][T/pt][F/pf][C];
 * out_tcf=1: out [B][T/pt][C][F/pf]  (the GRU feature order c*F'+f, sed.py:108-110).
 * T/pt and F/pf are floor divisions like nn.MaxPool2d's (sed.py:90): a ragged tail is dropped by the pool; it still
 * counts in the batch statistics and, in the backward, receives the statistics terms of the gradient.
 * drop_p=0 or training=0 disables dropout; the keep mask is a counter-based hash of
 * (seed, logical element index) so the backward pass regenerates it. */
int sed_bn_relu_pool_drop_fwd(const float* y, const float* scale, const float* shift, float* out,
                              int B, int T, int F, int C, int pool_f, int pool_t, int out_tcf,
                              float drop_p, uint64_t seed, const uint64_t* seed_dev, void* stream);
/* seed_dev (here and below; may be NULL): device pointer to a per-step salt added to `seed`, so that a captured
 * hipGraph of the step draws fresh masks on every replay (see sed_step_advance). */

/* Backward of the block above (training statistics).  Two passes:
 *  reduce: partials [rows][2][C] of  sum g  and  sum g*xhat  where g is dout routed through
 *          dropout, max-pool arg-max (first maximum wins) and ReLU;
 *  apply : dy = scale*(g - sum_g/N - xhat*sum_gx/N); also dgamma = sum_gx, dbeta = sum_g and
 *          the conv-bias gradient partials sum dy.  Fixed-order reductions. */
/* The routing DECISIONS of the block, as the forward and backward kernels make them (z = y*scale + shift, first maximum of a
 * window wins like max_pool2d, ReLU gate = max > 0; sed.py:107 `pool(torch.relu(bn(conv(x))))`): route [B][T/pt][F/pf][C], one
 * byte per pooled element, 0 = gate closed, 1 + w = window element w = df*pool_t + dt.  Inspection / parity tests: an oracle that
 * routes its gradient with these decisions differs from the kernels by rounding only.  pool_f*pool_t <= 254. */
int sed_bn_relu_pool_route(const float* y, const float* scale, const float* shift, unsigned char* route,
                           int B, int T, int F, int C, int pool_f, int pool_t, void* stream);
int sed_bn_bwd_rows(int B, int T, int pool_t);   /* partial rows written by the two passes below */
int sed_bn_relu_pool_drop_bwd_reduce(const float* y, const float* dout, const float* scale,
                                     const float* shift, const float* mean, const float* rstd,
                                     float* partials, int B, int T, int F, int C, int pool_f,
                                     int pool_t, int out_tcf, float drop_p, uint64_t seed, const uint64_t* seed_dev, void* stream);
int sed_bn_bwd_finalize(const float* partials, int rows, int C, float* sum_g, float* sum_gx,
                        float* dgamma, float* dbeta, void* stream);
/* sed_bn_bwd_finalize for partial rows that come out of sed_conv3x3_dgrad_bnred with a stored conv output below: channels
 * with |gamma| < |beta| / 64 (incl. gamma == 0 with beta > 0) were left out of sum g*xhat there (xhat = (z - beta)/gamma loses
 * eps |beta/gamma|) and are recomputed here from the block's conv output y [B][T][F][C]: g = dpooled/(1-p) where pooled > 0
 * (dpooled, pooled [B][T/pool_t][F/pool_f][C] channels-last), the window searched as the forward searches it (z = fma(y, scale,
 * shift), first maximum; sed.py:107 `pool(relu(bn(.)))`), xhat = (y_max - mean) rstd.  Same launch shape as
 * sed_bn_bwd_finalize; the recomputation is a cold path of the workgroups that own such a channel. */
int sed_bn_bwd_finalize_small_gamma(const float* partials, int rows, int C, float* sum_g, float* sum_gx,
                                    float* dgamma, float* dbeta, const float* dpooled, const float* pooled,
                                    const float* y, const float* gamma, const float* beta, const float* mean,
                                    const float* rstd, const float* scale, const float* shift,
                                    int B, int T, int F, int pool_f, int pool_t, float drop_p, void* stream);
/* The reduce pass of the block that feeds the GRU (out_tcf layout [B][T/pt][C][F/pf]) formed from that block's own pooled
 * OUTPUT and its gradient instead of the conv output: the same partial rows (sed_bn_bwd_rows) for sed_bn_bwd_finalize.
 * pooled > 0 exactly where the gradient passes, and the BatchNorm output at the arg-max is pooled*(1-p), so
 * xhat = (pooled*(1-p) - beta)/gamma; `y` (the conv output), scale and shift are read only for channels with
 * |gamma| < |beta| / 64 (incl. gamma == 0 with beta > 0), whose xhat is taken at the window's arg-max of the conv output.
 * _supported: out_tcf, F/pool_f a multiple of 4 and C*F/pool_f <= 16384; otherwise use sed_bn_relu_pool_drop_bwd_reduce. */
int sed_bn_bwd_reduce_pooled_supported(int F, int C, int pool_f, int pool_t, int out_tcf);
int sed_bn_bwd_reduce_pooled(const float* pooled, const float* dout, const float* gamma, const float* beta,
                             const float* y, const float* mean, const float* rstd, const float* scale, const float* shift,
                             float* partials, int B, int T, int F, int C, int pool_f, int pool_t, int out_tcf, float drop_p, void* stream);
int sed_bn_relu_pool_drop_bwd_apply(const float* y, const float* dout, const float* scale,
                                    const float* shift, const float* mean, const float* rstd,
                                    const float* sum_g, const float* sum_gx, float* dy,
                                    float* dbias_partials, int B, int T, int F, int C, int pool_f,
                                    int pool_t, int out_tcf, float drop_p, uint64_t seed, const uint64_t* seed_dev, void* stream);
/* out[c] = sum_r partials[r][c] in row order (double accumulation). */
int sed_reduce_rows(const float* partials, int rows, int C, int row_stride, float* out, void* stream);

/* ───────────── fused first conv block (conv recomputed, never stored; Cin <= 2) ─────────────
 * The first block of the stack (sed.py:86-92,106-107, ch = 1) expands a few MB of input into the largest tensor of
 * the step.  These four entries replace sed_conv3x3_fwd + the bn_* entries + sed_conv3x3_wgrad for block 1 and
 * recompute conv(x) on the fly, so that tensor never exists in HBM.  x [B][Cin][F][T] (network input layout),
 * wp = [9][C][Cin] from sed_conv3x3_pack_weights, pooled output / dout channels-last [B][T/pt][F/pf][C].
 * rows = sed_conv1_fused_rows(B,T) partial rows for bwd_reduce ([rows][2][C]); the statistics are one row. */
int sed_conv1_fused_supported(int Cin, int F, int T, int C, int pool_f, int pool_t);   /* 1 = shapes accepted */
int sed_conv1_fused_rows(int B, int T);
/* Statistics WITHOUT recomputing the convolution: sum y and sum y^2 of every output channel follow from the first and
 * second moments of the 9*Cin shifted inputs (one pass over x, fp64 quadratic form per channel).  Writes ONE partial
 * row [1][2][C]; workspace >= sed_conv1_stats_workspace_bytes().  With 1 or 2 input channels T may be any positive number
 * of time rows (this pass has a ragged last tile; the multiple of 4 of sed_conv1_fused_supported belongs to the other passes). */
size_t sed_conv1_stats_workspace_bytes(int B, int Cin, int T);
/* moments (may be NULL): device array of sed_conv1_moments_doubles(Cin) doubles that receives the input moments themselves
 * ([9*Cin] first moments, then the upper triangle of the second moments row by row) for sed_conv1_bwd_wgrad. */
size_t sed_conv1_moments_doubles(int Cin);
int sed_conv1_stats(const float* x, const float* wp, const float* bias, float* stat_partials, void* workspace,
                    int B, int Cin, int F, int T, int C, double* moments, void* stream);
/* argmax_bits (may be NULL; (1,2) pool only): one byte per output channel quad, [B][T/2][F][C/4], bit k = the second time row of
 * the window holds the maximum of channel 4q+k (the first maximum wins a tie): what sed_conv1_bwd_wgrad routes the gradient by. */
int sed_conv1_bn_relu_pool_drop_fwd(const float* x, const float* wp, const float* bias, const float* scale,
                                    const float* shift, float* out, int B, int Cin, int F, int T, int C,
                                    int pool_f, int pool_t, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                                    unsigned char* argmax_bits, void* stream);
/* sed_bn_relu_pool_route for the recomputed first block (the decisions of its passes; same shapes as the forward entry). */
int sed_conv1_route(const float* x, const float* wp, const float* bias, const float* scale, const float* shift,
                    unsigned char* route, int B, int Cin, int F, int T, int C, int pool_f, int pool_t, void* stream);
int sed_conv1_bwd_reduce(const float* x, const float* wp, const float* bias, const float* dout,
                         const float* scale, const float* shift, const float* mean, const float* rstd,
                         float* partials, int B, int Cin, int F, int T, int C, int pool_f, int pool_t,
                         float drop_p, uint64_t seed, const uint64_t* seed_dev, void* stream);
size_t sed_conv1_bwd_apply_workspace_bytes(int B, int Cin, int T, int C);
/* dy is formed on the fly: writes dw_oihw [C][Cin][3][3] and the conv-bias gradient only.
 * gamma / beta / dgamma (all three or none; may be NULL): when given, dgamma[c] is overwritten by this pass's own sum g*xhat
 * for every channel with gamma[c] == 0 and beta[c] > 0 — the one case in which the reduction fused into the data gradient
 * above (sed_conv3x3_dgrad_bnred) cannot form it, because this block stores no conv output. */
int sed_conv1_bwd_apply_wgrad(const float* x, const float* wp, const float* bias, const float* dout,
                              const float* scale, const float* shift, const float* mean, const float* rstd,
                              const float* sum_g, const float* sum_gx, float* dw_oihw, float* dbias,
                              void* workspace, int B, int Cin, int F, int T, int C, int pool_f, int pool_t,
                              float drop_p, uint64_t seed, const uint64_t* seed_dev,
                              const float* gamma, const float* beta, float* dgamma, void* stream);

/* Backward of the recomputed first block WITHOUT recomputing it ((1,2) pool; replaces sed_conv1_bwd_apply_wgrad where
 * sed_conv1_rgrad_supported() and the BatchNorm-backward sums are already known, e.g. from sed_conv3x3_dgrad_bnred):
 *   dW_k = scale [ R_k - (sum_g/N) S1_k - (sum_gx/N) rstd ( b S1_k + sum_k' w_k' G_kk' - mean S1_k ) ],   N = B*T*F,
 * with S1 / G the input moments of sed_conv1_stats and R_k = sum over pooled elements of g * x[arg-max position + tap k], the
 * only sum this pass forms: g = dout / (1-p) where `pooled` (the block's forward output) is > 0, the arg-max row from
 * `argmax_bits`.  No convolution, dropout hash or BatchNorm arithmetic is redone.  Also writes the conv-bias gradient and, given
 * gamma / beta / dgamma, dgamma of channels with gamma == 0 and beta > 0 (see sed_conv1_bwd_apply_wgrad).
 * workspace >= sed_conv1_bwd_wgrad_workspace_bytes(). */
int sed_conv1_rgrad_supported(int Cin, int F, int T, int C, int pool_f, int pool_t);
size_t sed_conv1_bwd_wgrad_workspace_bytes(int B, int Cin, int T, int C);
int sed_conv1_bwd_wgrad(const float* x, const float* dout, const float* pooled, const unsigned char* argmax_bits,
                        const double* moments, const float* wp, const float* bias, const float* mean, const float* rstd,
                        const float* scale, const float* sum_g, const float* sum_gx, float* dw_oihw, float* dbias,
                        void* workspace, int B, int Cin, int F, int T, int C, float drop_p,
                        const float* gamma, const float* beta, float* dgamma, void* stream);
/* its assembling half alone, from partials [rows][C][1 + 9 Cin] formed elsewhere (sed_conv3x3_dgrad_bnred_rg).
 * sum_gx may be NULL (both entries): sum g*xhat is then formed from the block's own sums — rstd (b sum g + sum_k w_k R_k - mean
 * sum g), exact for every gamma, where the value recovered from the pooled output, (z - beta)/gamma, loses eps |beta/gamma| — and
 * also written to dgamma; with sum_gx given (a recomputing reduce pass, or sums all-reduced for synchronised BatchNorm) it is
 * used as is and only gamma == 0 channels take the own value for dgamma. */
int sed_conv1_bwd_wgrad_assemble(const float* partials, int rows, const double* moments, const float* wp, const float* bias,
                                 const float* mean, const float* rstd, const float* scale, const float* sum_g,
                                 const float* sum_gx, float* dw_oihw, float* dbias, int B, int Cin, int F, int T, int C,
                                 const float* gamma, const float* beta, float* dgamma, void* stream);

/* ───────────── dense GEMM on fp32 MFMA (aten::mm/addmm under nn.GRU / nn.Linear, sed.py:101-103) ─────────────
 * C[i][j] = sum_k A(i,k) * B(k,j) (+ bias[j]) (+ beta*C[i][j]), C row-major with leading dim ldc.
 * A(i,k) = A[i*a_si + k*a_sk], B(k,j) = B[k*b_sk + j*b_sj]; for each operand one of the
 * two strides must be 1.  Exact fp32 (v_mfma_f32_32x32x2_f32: one fixed order of summation whatever the tile or layout). */
int sed_gemm_f32(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj,
                 float* C, long ldc, const float* bias, float beta, int M, int N, int K, void* stream);
/* Same product (optional bias, beta = 0) with a scratch buffer: small-output / long-K shapes (the GRU weight
 * gradients, M*N small, K = B*T'; the input projection of a small batch, M = B*T' small, K = C*F') would leave most
 * CUs without a tile, so they are split along K into fixed slices that are summed in slice order (deterministic; the
 * bias is added by the summing pass).  workspace >= sed_gemm_f32_workspace_bytes(M,N,K) (0 = the shape is not split). */
size_t sed_gemm_f32_workspace_bytes(int M, int N, int K);   /* covers sed_gemm_f32_ws and sed_gemm_f32_wgrad */
int sed_gemm_f32_ws(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj,
                    float* C, long ldc, const float* bias, int M, int N, int K, void* workspace, void* stream);

/* bf16 form (the input projection of GRU layer 0 in the bf16 inference plan): C[i][j] = sum_k A[i][k] B[j][k] + bias[j], A bf16
 * [M][K] and B bf16 [N][K] row-major, C fp32 with leading dim ldc, bias fp32 (may be NULL), K % 32 == 0.  fp32 accumulation on
 * v_mfma_f32_32x32x16_bf16, no split of K: every element sums its k-tiles in one fixed order whatever M (a batch equals its
 * chunks bit for bit). */
int sed_gemm_bf16_nt(const void* A, const void* B, const float* bias, float* C, long ldc, int M, int N, int K, void* stream);

/* Weight-gradient form (dW = dY^T X under loss.backward(), sed.py:137): the same product, beta = 0, no bias, whose K axis is
 * the batch x time axis.  Besides the small-output split above it may be cut into two K-slices when its best tiling
 * gives at most one tile per CU (two co-resident workgroups per CU instead of one).  Deterministic for given (M,N,K). */
int sed_gemm_f32_wgrad(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj,
                       float* C, long ldc, int M, int N, int K, void* workspace, void* stream);
/* Which plan a call of the three entries above runs (host only, the launches read the same rule).  policy 0: sed_gemm_f32,
 * 1: sed_gemm_f32_ws, 2: sed_gemm_f32_wgrad (the latter two given a workspace).  *bm x *bn = the block tile; *splits = number of
 * K-slices (1: not split); *k_len = k extent of a slice (K when not split; the last slice may be shorter). */
int sed_gemm_f32_plan(int M, int N, int K, int policy, int* bm, int* bn, int* splits, int* k_len);

/* Small dense layer y = act(x W^T + b) for the time-distributed head (sed.py:103,112;
 * crnn_lightning.py:63-64,72-73). x [M][K], W [N][K], y [M][N]; relu=1 applies ReLU. */
int sed_linear_fwd(const float* x, const float* W, const float* b, float* y,
                   int M, int K, int N, int relu, void* stream);
/* dy is modified in place when relu=1 (masked by y>0).  dx may be NULL.
 * workspace: sed_linear_bwd_workspace_bytes(). */
size_t sed_linear_bwd_workspace_bytes(int M, int K, int N);
int sed_linear_bwd(const float* x, const float* W, const float* y, float* dy, float* dx,
                   float* dW, float* db, void* workspace, int M, int K, int N, int relu, void* stream);

/* ───────────── bidirectional GRU layer recurrence (nn.GRU, sed.py:101-102,111) ─────────────
 * PyTorch gate convention (r,z,n): n = tanh(gi_n + r*(W_hn h + b_hn)), h' = (1-z)*n + z*h, h0 = 0.
 * gi   [B][T][2][3H]  input projections x W_ih^T + b_ih of both directions (dir 1 = reverse);
 * whh  2 pointers to weight_hh [3H][H]; bhh 2 pointers to bias_hh [3H];
 * out  [B][T][2H]  (forward | reverse), exactly nn.GRU's batch_first output;
 * saved[B][T][2][5][H] = r, z, n, (W_hn h + b_hn), h_prev  (training only, may be NULL). */
size_t sed_gru_seq_workspace_bytes(int H);          /* scratch for the transposed W_hh */
int sed_gru_seq_fwd(const float* gi, const float* const* whh, const float* const* bhh,
                    float* out, float* saved, void* workspace, int B, int T, int H, void* stream);
/* dout [B][T][2H] -> dgi [B][T][2][3H] (grad of gi) and dgh [B][T][2][3H] (grad of W_hh h + b_hh).
 * dbih / dbhh (2 pointers each, or both NULL): bias gradients summed in-kernel (no re-read of dgi/dgh);
 * workspace >= sed_gru_seq_bwd_workspace_bytes(B, H) when they are requested. */
size_t sed_gru_seq_bwd_workspace_bytes(int B, int H);
int sed_gru_seq_bwd(const float* dout, const float* saved, const float* const* whh,
                    float* dgi, float* dgh, float* const* dbih, float* const* dbhh, void* workspace,
                    int B, int T, int H, void* stream);
/* Which kernel variant a (B, H) call of the two functions above runs (host only, the launches read the same rule):
 * *bt = batch rows per workgroup (1, 2 or 4); *hreg = weights of a gate row held in registers (H: the whole row, 0: none,
 * the row is streamed from L2 every step); *hlds = weights of a row held in LDS (> 0 only for the H = 256 hybrid, where
 * *hreg is the forward kernel's share and the remaining H - hreg - hlds are streamed). */
int sed_gru_seq_variant(int B, int H, int* bt, int* hreg, int* hlds);

/* ───────────── loss heads (sed.py:136,160; crnn_lightning.py:27-35) ─────────────
 * kind 0: BCEWithLogits mean; kind 1: focal (alpha, gamma, log(pt+1e-12)); reduction_mean=0 -> sum.
 * loss (1 float), dlogits (may be NULL) = d loss / d logits, probs (may be NULL) = sigmoid(logits). */
int sed_loss_fwd_bwd(const float* logits, const float* targets, int n, int kind, float alpha,
                     float gamma, int reduction_mean, float* loss, float* dlogits, float* probs,
                     void* stream);
int sed_sigmoid(const float* x, float* y, int n, void* stream);
int sed_scale(float* x, long n, float alpha, void* stream);        /* x *= alpha */

/* ───────────── optimiser (torch.optim.Adam sed.py:159; crnn_lightning.py:195-197; clip train_lightning.py:50) ─────────────
 * sq-norm: norm_out[0] = ||g||_2, norm_out[1] = clip coefficient min(1, max_norm/(norm+1e-6))
 * (1 when max_norm <= 0).  workspace >= sed_sqnorm_workspace_bytes(n). Deterministic. */
size_t sed_sqnorm_workspace_bytes(long n);
int sed_grad_norm_clip_coef(const float* g, long n, float max_norm, float* norm_out,
                            void* workspace, void* stream);
/* Adam with coupled L2 weight decay on a flat arena; grads are multiplied by *grad_scale
 * (device pointer, may be NULL = 1) first.  step >= 1. */
int sed_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* grad_scale,
                  const uint64_t* step_state, void* stream);
/* step_state (may be NULL): device pointer to {dropout salt, optimiser step}; when given, the step count is read from
 * step_state[1] on the device instead of `step`.  sed_step_advance increments both words (one tiny launch per fit
 * step): with it the whole fit step is a replayable hipGraph. */
int sed_step_advance(uint64_t* step_state, void* stream);

/* ───────────── log-mel front end (feature.py:55-59 via librosa.stft / filters.mel) ─────────────
 * pcm [n_samples] mono f32 -> out [n_frames][n_mels] = log(mel @ |STFT|^2), n_frames = 1 + n_samples/hop; frames are
 * centred (librosa center=True): frame f covers samples [f*hop - n_fft/2, f*hop + n_fft/2), padded per pad_mode
 * (0 = zeros, librosa >= 0.10 "constant"; 1 = numpy "reflect", older librosa).  n_fft must be 2048.
 * The constant tables travel as ONE blob that the kernel keeps in LDS.  It is built on the HOST (no GPU call) from
 * host arrays: window [n_fft] and melfb [n_mels][n_fft/2+1] (both computed in double by the caller, librosa's Hann /
 * Slaney bank in sed_crnn_amd/feature.py); the builder adds the FFT twiddles and turns the filterbank into its sparse
 * band-major form (any bank whose non-zeros fit the plan: <= 8192 of them, n_mels <= 128).
 *   sed_logmel_tables_bytes  -> size of the blob for this bank (0 = cannot be planned);
 *   sed_logmel_build_tables  -> fills tables_host; the caller copies it to the device once.
 * sed_logmel: `tables` must be a blob written by sed_logmel_build_tables for this n_mels (the library cannot read device
 * memory to check it; only its size is validated); mu/inv_sigma (device, may both be NULL) fuse feature.py:127-129's
 * StandardScaler: (x-mu)*inv_sigma. */
size_t sed_logmel_tables_bytes(const float* melfb_host, int n_fft, int n_mels);
int sed_logmel_build_tables(const float* window_host, const float* melfb_host, int n_fft, int n_mels,
                            void* tables_host, size_t tables_bytes);
int sed_logmel(const float* pcm, long n_samples, const void* tables, size_t tables_bytes,
               const float* mu, const float* inv_sigma, float* out,
               int n_fft, int hop, int n_mels, int pad_mode, void* stream);
/* sed_logmel_batch: R mono clips packed in ONE pcm buffer [pcm_len] -> out [sum_r (1 + n_r/hop)][n_mels], the clips' frames
 * back to back in clip order, in one launch.  clips_host [R][2] = {first sample, n_r >= 1} (HOST array, validated: every
 * clip inside the buffer) is uploaded into `workspace` (>= sed_logmel_batch_workspace_bytes(R), device) on the stream; out_rows
 * must equal the frame total (< 2^31).  Each clip is framed and padded (pad_mode) at its own ends exactly like sed_logmel on
 * that clip alone: the result is bit for bit that of R sed_logmel calls.  A clip whose first sample is not 8-byte aligned
 * takes the guarded load path (same values). */
size_t sed_logmel_batch_workspace_bytes(int R);
int sed_logmel_batch(const float* pcm, long pcm_len, const long* clips_host, int R, const void* tables, size_t tables_bytes,
                     const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop, int n_mels,
                     int pad_mode, void* workspace, size_t workspace_bytes, void* stream);
/* sed_logmel_multi: R recordings of `channels` planar channels each, all R*channels clips packed in ONE pcm buffer
 * -> out [sum_r (1 + n_r/hop)][channels*n_mels], the [N, C*F] layout the nets read: clip (r, c) = entry r*channels + c of
 * clips_host [R*channels][2] = {first sample, n >= 1} writes the rows of recording r, columns [c*n_mels, (c+1)*n_mels).  The
 * channels of a recording must have equal length (validated on the host, with every clip's bounds; the message names the
 * recording); out_rows must equal the frame total.  mu/inv_sigma (may both be NULL) have channels*n_mels entries, column
 * c*n_mels + m for channel c, band m; they are kept in LDS, so the waves per workgroup are chosen with their real size and a
 * scaler beside which not even 2 waves fit is refused.  Every channel's columns are bit for bit sed_logmel on that channel with
 * its slice of the scaler; channels = 1 is bit for bit sed_logmel_batch.  1 <= channels <= 64. */
size_t sed_logmel_multi_workspace_bytes(int R, int channels);
int sed_logmel_multi(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                     size_t tables_bytes, const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop,
                     int n_mels, int pad_mode, void* workspace, size_t workspace_bytes, void* stream);
/* sed_logmel_gcc: the arguments of sed_logmel_multi plus n_lags -> out [rows][channels*n_mels + P*n_lags], P =
 * channels*(channels-1)/2.  Columns [c*n_mels, (c+1)*n_mels) are bit for bit what sed_logmel_multi writes for channel c (it is
 * that launch, with this row stride).  Columns [channels*n_mels + p*n_lags, .. + n_lags) hold the GCC-PHAT of microphone pair p
 * = (i, j), i < j in lexicographic order, of the same frame: with X_c the 2048-point spectrum of the windowed frame of channel c,
 * G = X_i conj X_j, Pk = G / |G| (0 where |G|^2 < 1e-30 in fp32: digital silence gives zeros, never NaN),
 * cc[tau] = (1/2048) (Pk[0] + (-1)^tau Pk[1024] + 2 sum_{k=1..1023} Re(Pk[k] e^{+2 pi i k tau / 2048})) for tau = -n_lags/2 ..
 * n_lags/2 - 1, in column tau + n_lags/2; values lie in [-1, 1]; channel j = channel i delayed by d samples peaks at tau = -d.
 * mu/inv_sigma (may both be NULL) are as wide as a row; the GCC columns become (cc - mu)*inv_sigma.  2 <= channels <= 8, n_lags
 * even and <= 128 (the feature path uses n_lags = n_mels).  Every value is summed in one fixed order that depends on the
 * frame's samples alone.  Where |G|^2 overflows fp32 (samples of ~1e6 and more) the bin is written as 0 — G / sqrt(inf) for a
 * finite G — never as inf * 0 = NaN.  workspace: 8-byte aligned, >= sed_logmel_gcc_workspace_bytes(R, channels) (0 = bad sizes). */
size_t sed_logmel_gcc_workspace_bytes(int R, int channels);
int sed_logmel_gcc(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                   size_t tables_bytes, const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop,
                   int n_mels, int n_lags, int pad_mode, void* workspace, size_t workspace_bytes, void* stream);
/* sed_event_tdoa: for each of E detected events and each microphone pair p = (i, j), i < j in lexicographic order, the
 * time difference of arrival in samples and how coherent it is, from the GCC-PHAT of the event's frames accumulated in the
 * frequency domain.  The recordings are given as for sed_logmel_gcc (planar channels, equal lengths; clips_host is a HOST table
 * that is validated before anything is enqueued).  ev_rec / ev_onset / ev_offset / ev_peak_frame: DEVICE int32 [E], in output
 * frames of time_factor feature frames, offset exclusive (what the decoders write); ev_rec may be NULL when R == 1.  With n_feat =
 * 1 + n/hop feature frames in the event's recording, a = onset*time_factor and b = min(offset*time_factor, n_feat), the event is
 * located on the frames [f0, f1): [a, b) when b - a <= max_frames, else the max_frames frames f0 = clamp(peak_frame*time_factor +
 * time_factor/2 - max_frames/2, a, b - max_frames); the single frame a when b <= a.  With Pk_f the whitened cross spectrum of
 * frame f as sed_logmel_gcc defines it, S = sum_f Pk_f and acc[tau] = (1/2048) (S[0] + (-1)^tau S[1024] + 2 sum_{k=1..1023}
 * Re(S[k] e^{+2 pi i k tau / 2048})), |tau| <= max_lag + 1: t* is the first maximum of acc over |tau| <= max_lag in ascending
 * order, lag = t* + 0.5 (l - r) / (l - 2m + r) with (l, m, r) = acc[t*-1 .. t*+1] where that denominator is < 0, else t*;
 * strength = m / (f1 - f0) in [-1, 1].  Channel j = channel i delayed by d samples gives lag = -d.  Digital silence gives acc = 0,
 * lag = 0, strength = 0, never NaN.  lag_out / strength_out: device float [E][P]; frames_out: device int32 [E] = f1 - f0; acc_out
 * (may be NULL): device float [E][P][2 max_lag + 3], acc[tau] at tau + max_lag + 1.  The event entries are checked on the device:
 * an event whose rec is outside [0, R) or whose onset is negative or beyond its recording's last frame gets 0 frames, lag 0 and
 * strength 0, and reads no memory.  Every output is summed in one fixed order that depends on the event's own samples and frame
 * range alone (frames in ascending order within chunks of 32 counted from f0, the chunks in ascending order): not on the other
 * events, the clip's place in the buffer or the workspace size.  workspace: 16-byte aligned;
 * sed_event_tdoa_workspace_bytes(R, channels, E, longest recording in samples, hop, max_frames) holds all E events at once (0 =
 * bad sizes); with less — at least the size for E = 1 — the event table is processed in slices, with the same bits.  The host
 * reads nothing back.  2 <= channels <= 8, 1 <= max_lag <= 127, max_frames >= 1, the 2048-point tables of sed_logmel_build_tables;
 * E = 0 launches nothing. */
size_t sed_event_tdoa_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames);
int sed_event_tdoa(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                   size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                   long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames, float* lag_out, float* strength_out,
                   int* frames_out, float* acc_out, void* workspace, size_t workspace_bytes, void* stream);
/* Live feeds: every planar lane of a stream keeps its last cap samples in a ring, ring [lanes][cap] float, sample i
 * of the lane (counted from the start of the feed) at ring[lane*cap + i % cap].
 * sed_stream_ring_write scatters a round's new samples into the rings in one launch.  table_host: HOST long [lanes][3] = {first
 * sample in src, count, absolute index of the first sample}, validated before anything is enqueued: 0 <= count <= cap (so no
 * entry is written twice), the source range inside src [src_len], cap a multiple of 4 (the lanes stay 16-byte aligned),
 * lanes * cap <= ring_len.  All counts 0: nothing is launched.  workspace: >= sed_stream_ring_write_workspace_bytes(lanes)
 * (0 = lanes outside 1..65535).  The host reads nothing back.
 * sed_event_tdoa_ring is sed_event_tdoa with recording r = feed r, its channels the rings (r*channels + ch) of cap >= 2048
 * samples, and n_host: HOST long [R], the samples feed r has received so far.  Absolute sample i reads ring[.. + i % cap] when
 * max(0, n - cap) <= i < n and 0 otherwise (constant padding).  The event's frames [f0, f1) are sed_event_tdoa's with n_feat =
 * 1 + n/hop; the event gets 0 frames, lag 0 and strength 0, and reads nothing, when in addition
 *   offset*time_factor + lat_frames - f0 > history_frames   (the stream's rule: it depends on the event and the settings alone), or
 *   max(0, f0*hop - 1024) < n - cap                         (its first sample has left the ring).
 * Everything else — the sums and their order, lag, strength, acc, the slicing by workspace size — is sed_event_tdoa's: an event
 * whose samples are all in the ring gets the bits sed_event_tdoa gives on the linear recording x[0, n), wherever the ring wraps.
 * ring: 16-byte aligned, R * channels * cap <= ring_len.  workspace: 16-byte aligned, sed_event_tdoa_ring_workspace_bytes(R,
 * channels, E, cap, hop, max_frames) for all E events at once (0 = bad sizes), at least that of E = 1.  E = 0 launches nothing. */
size_t sed_stream_ring_write_workspace_bytes(int lanes);
int sed_stream_ring_write(float* ring, long ring_len, int lanes, long cap, const float* src, long src_len, const long* table_host,
                          void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_tdoa_ring_workspace_bytes(int R, int channels, long E, long cap, int hop, int max_frames);
int sed_event_tdoa_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const void* tables,
                        size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                        long E, int time_factor, int hop, int max_lag, int max_frames, int lat_frames, int history_frames,
                        float* lag_out, float* strength_out, int* frames_out, float* acc_out, void* workspace,
                        size_t workspace_bytes, void* stream);
/* sed_event_doa: sed_event_tdoa, and for every event one direction out of a grid of D, by steered response power
 * (SRP-PHAT) for a known array.  Every argument it shares with sed_event_tdoa means what it means there, and lag_out,
 * strength_out, frames_out and acc_out receive the bits that call writes.  With S the accumulated whitened cross spectrum of
 * the event and pair p that acc is made from, Q = oversample in {1, 2, 4, 8, 16} and F = Q max_lag:
 *   fine_p[j] = (1/2048) (S[0] + Re S[1024] cos(pi j / Q) + 2 sum_{k=1..1023} Re(S[k] e^{+2 pi i k j / (2048 Q)})),  |j| <= F:
 * the band-limited correlation at the lag j / Q samples (at Q = 1, acc[j] bit for bit);
 *   srp[d] = sum_p fine_p[steer_lags[d][p]], fp32 adds in ascending p; dir = the first maximum of srp in ascending d; power =
 * srp[dir] / (P (f1 - f0)) in [-1, 1].  An event without frames and digital silence (every srp value 0) give dir = -1 and
 * power = 0; no NaN is written to either.  steer_lags: DEVICE int32 [D][P], the fine lag Q sr (r_j - r_i) . u_d / c of direction
 * d and pair p rounded to an integer (a value outside [-F, F] is read as the nearer end); trig: DEVICE float [512 Q + 1][2],
 * (cos, sin)(2 pi k / (2048 Q)) (float64 values rounded once), 8-byte aligned; dir_out: device int32 [E]; power_out: device
 * float [E]; srp_out (may be NULL): device float [E][D].  1 <= D <= 16384.  One more launch per slice of the event table; the
 * workspace is sed_event_tdoa's (sed_event_doa_workspace_bytes returns the same size) and the slicing changes no bit.  Every
 * output depends on the event's own samples, its frame range and these settings alone.  The host reads nothing back; every
 * argument is checked before anything is enqueued.
 * sed_event_doa_ring is the same on the rings of live feeds: sed_event_tdoa_ring's arguments, rules and bits. */
size_t sed_event_doa_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames);
int sed_event_doa(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                  size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                  long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames, float* lag_out, float* strength_out,
                  int* frames_out, float* acc_out, const int* steer_lags, int D, int Q, const float* trig, int* dir_out,
                  float* power_out, float* srp_out, void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_doa_ring_workspace_bytes(int R, int channels, long E, long cap, int hop, int max_frames);
int sed_event_doa_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const void* tables,
                       size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                       long E, int time_factor, int hop, int max_lag, int max_frames, int lat_frames, int history_frames,
                       float* lag_out, float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D, int Q,
                       const float* trig, int* dir_out, float* power_out, float* srp_out, void* workspace, size_t workspace_bytes,
                       void* stream);
/* sed_event_doa_track: sed_event_doa, and a direction per BLOCK of block_chunks = W chunks of 32 located frames, for
 * a source that moves while it sounds.  Every argument it shares with sed_event_doa means what it means there, and lag_out,
 * strength_out, frames_out, acc_out, dir_out, power_out and srp_out receive the bits that call writes.  An event located on nf
 * frames has nch = ceil(nf / 32) chunks, T0 = ceil(nch / W) and nl = nf - 32 W (T0 - 1); T = T0 - 1 where T0 > 1 and nl < 16 W (the
 * short tail joins the block before it), else T0; nf = 0 gives T = 0.  Block b covers the chunks [b W, (b + 1) W), the last block
 * up to nch, and its map m_b [D] is srp of sed_event_doa with S summed over the block's chunks alone (the first chunk starts the
 * sum, the others are added in ascending order: a block of all the event's chunks is the event's srp bit for bit).  With
 * Tm = ceil(ceil(max_frames / 32) / W) <= 256: trk_len_out: device int32 [E], T; trk_raw_out: device int32 [E][Tm], the first
 * maximum of m_b in ascending d, -1 for a silent block; trk_power_out: device float [E][Tm], m_b[raw] / (P n_b) with n_b the
 * block's frames, 0 where raw is -1; trk_map_out (may be NULL): device float [E][Tm][D]; rows b >= T are -1 / 0.
 * nbr_off / nbr_idx: DEVICE int32 [D + 1] / [nbr_off[D]], row d of a neighbour table lists the directions the path may come to d
 * from (localize.track_neighbours); both NULL: no smoothing, trk_dir_out: device int32 [E][Tm] is a copy of trk_raw_out.  With a
 * table, s_0 = m_0, s_b[d] = m_b[d] + max_j s_{b-1}[nbr_idx[nbr_off[d] + j]] (the first maximum in ascending j, one fp32 add per
 * cell; an index outside [0, D) is read as the nearer end), the path ends at the first maximum of s_{T-1} in ascending d and
 * trk_dir_out[e][b] is its direction in block b, -1 where trk_raw_out[e][b] is -1.  1 <= W <= 64.  The workspace is
 * sed_event_tdoa's followed, with a table (smooth != 0), by [Tw][D] floats and [Tw][D] 16-bit words per event, Tw =
 * ceil(chunk slots per event / W): sed_event_doa_track_workspace_bytes; a smaller one that takes one event (E = 1) is walked in
 * slices and changes no bit (0: the sizes are refused).  One launch more per slice than sed_event_tdoa, two with a table; the
 * host reads nothing back; every argument is checked before anything is enqueued.
 * sed_event_doa_track_ring is the same on the rings of live feeds: sed_event_doa_ring's arguments, rules and bits. */
size_t sed_event_doa_track_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames, int D,
                                           int block_chunks, int smooth);
int sed_event_doa_track(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                        size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                        long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames, float* lag_out,
                        float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D, int Q, const float* trig,
                        int* dir_out, float* power_out, float* srp_out, int block_chunks, const int* nbr_off, const int* nbr_idx,
                        int* trk_len_out, int* trk_raw_out, int* trk_dir_out, float* trk_power_out, float* trk_map_out,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_doa_track_ring_workspace_bytes(int R, int channels, long E, long cap, int hop, int max_frames, int D,
                                                int block_chunks, int smooth);
int sed_event_doa_track_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const void* tables,
                             size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                             const int* ev_peak_frame, long E, int time_factor, int hop, int max_lag, int max_frames, int lat_frames,
                             int history_frames, float* lag_out, float* strength_out, int* frames_out, float* acc_out,
                             const int* steer_lags, int D, int Q, const float* trig, int* dir_out, float* power_out, float* srp_out,
                             int block_chunks, const int* nbr_off, const int* nbr_idx, int* trk_len_out, int* trk_raw_out,
                             int* trk_dir_out, float* trk_power_out, float* trk_map_out, void* workspace, size_t workspace_bytes,
                             void* stream);
/* sed_event_contrast_frames / sed_event_doa_contrast / sed_event_doa_track_contrast: contrast SRP-PHAT, for an event
 * that sounds over a louder source of another class.  sed_event_doa gives such an event the louder source's direction; here the
 * share of that source is estimated from frames before the onset in which the event's own class is silent, and removed from the
 * event's accumulated cross spectrum before the map is steered: S'[k] = S[k] - w Sb[k], w = (float)((double)weight nf / nb), one
 * fmaf per component, with S the sum over the event's nf located frames and Sb the sum over its nb background frames, each of
 * them loaded, transformed and whitened exactly as the located frame of that index is, added in chunks of 32 consecutive list
 * entries and the chunk partials in ascending order.
 * The rule is integer and reads the event table and the settings alone.  ev_cls: device int32 [E], the class of every row,
 * counted in n_classes in [1, 32].  With H = time_factor hop and L_r = n_r / H + 1: mask[r][t] has bit cls of every row of the
 * table with 0 <= cls < n_classes, onset >= 0 and a recording in range, for onset <= t < min(offset, L_r), located or not.  An
 * event with frames (frames_out > 0) and a class in range has the candidates q = 0 .. search - 1: feature frame
 * g = onset time_factor - guard - 1 - q, which exists when g >= 0 and is eligible when bit cls of mask[r][t] is clear for
 * t = max(g hop - 1024, 0) / H .. min(ceil((g hop + 1024) / H), L_r) - 1.  The first `frames` eligible candidates in ascending q
 * are its background frames; bg_frames_out: device int32 [E], their number nb, 0 where fewer than min_frames were found;
 * bg_sel_out: device int32 [E][frames], their q in summation order (descending q, ascending time), -1 behind them.
 * 1 <= frames <= 256, frames <= search <= 4096, 0 <= guard <= 64, 1 <= min_frames <= frames, weight finite in (0, 4].
 * sed_event_contrast_frames does the activity and the selection alone and reads no sample.  sed_event_doa_contrast takes the
 * arguments of sed_event_doa with ev_cls behind ev_rec, the six settings behind max_frames and the two outputs behind srp_out:
 * lag_out, strength_out, frames_out and acc_out come from S and keep the bits of sed_event_doa; dir_out, power_out = srp[dir] /
 * (P nf) and srp_out come from S'; an event with nb = 0 gets the bits of sed_event_doa throughout.  sed_event_doa_track_contrast
 * is sed_event_doa_track in the same way: every block's map is made from S_b - w_b Sb with the event's one Sb and
 * w_b = (float)((double)weight n_b / nb), and trk_raw, trk_power, trk_map and the path come from those maps.
 * mask_frames: sum_r L_r.  The workspace is the recording table, the mask (built once per call from the whole table, whatever
 * the slicing) and, per event, the chunk slots of sed_event_tdoa and ceil(frames / 32) more (then the track's tail); the
 * _workspace_bytes functions return 0 for sizes that are refused; a smaller workspace that takes one event is walked in slices
 * and changes no bit.  Every output depends on the event's own samples, those of its background frames, the table and the
 * settings alone.  Everything that can be checked on the host is checked before anything is enqueued; the messages begin
 * "contrast_frames:" / "doa_contrast:" / "doa_track_contrast:"; E = 0 launches nothing.  There are no ring forms. */
size_t sed_event_contrast_frames_workspace_bytes(int R, int channels, long mask_frames, int frames);
int sed_event_contrast_frames(long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_cls,
                              const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, long E, int time_factor, int hop,
                              int max_frames, int n_classes, int frames, int search, int guard, int min_frames, int* bg_frames_out,
                              int* bg_sel_out, void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_doa_contrast_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames,
                                              long mask_frames, int frames);
int sed_event_doa_contrast(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                           size_t tables_bytes, const int* ev_rec, const int* ev_cls, const int* ev_onset, const int* ev_offset,
                           const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames,
                           int n_classes, int frames, int search, int guard, int min_frames, double weight, float* lag_out,
                           float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D, int Q,
                           const float* trig, int* dir_out, float* power_out, float* srp_out, int* bg_frames_out, int* bg_sel_out,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_doa_track_contrast_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames, int D,
                                                    int block_chunks, int smooth, long mask_frames, int frames);
int sed_event_doa_track_contrast(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                                 size_t tables_bytes, const int* ev_rec, const int* ev_cls, const int* ev_onset, const int* ev_offset,
                                 const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames,
                                 int n_classes, int frames, int search, int guard, int min_frames, double weight, float* lag_out,
                                 float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D, int Q,
                                 const float* trig, int* dir_out, float* power_out, float* srp_out, int block_chunks,
                                 const int* nbr_off, const int* nbr_idx, int* trk_len_out, int* trk_raw_out, int* trk_dir_out,
                                 float* trk_power_out, float* trk_map_out, int* bg_frames_out, int* bg_sel_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* sed_event_beam_spans / sed_event_beamform: the audio of every located event, with the array pointed at it by a
 * steered delay-and-sum beam.  The event columns, clips_host, R, channels, time_factor, hop and max_frames are sed_event_doa's;
 * ev_dir and ev_loc_frames are the dir_out and frames_out it wrote.  An event is extracted iff 0 <= dir < D; its samples are
 * [s0, s1) = [f0 hop, min((f0 + loc_frames) hop, n)) with f0 the first frame sed_event_tdoa locates it on (loc_frames is read
 * as at most that range).
 *   sed_event_beam_spans: len_out int32 [E] = max(0, s1 - s0) (0: not extracted), start_out int64 [E] = the exclusive prefix sum
 * of len_out in event order, total_out int64 [1] = its sum; one launch, nothing else is read.  max_frames * hop <= 2^31 - 1.
 *   sed_event_beamform: audio [audio_total] (the caller reads total_out, 8 bytes, to size it), event e at
 * [audio_start[e], + audio_len[e]).  delays: DEVICE int32 [D][C], M[d][c] = round(Q sr (r_c - rbar) . u_d / c), the delay of
 * channel c for direction d in 1/Q samples; taps: DEVICE float [Q][2H], row p evaluates a channel at m + p/Q:
 * x(m + p/Q) = sum_k taps[p][k] x[m + k - H + 1]; Q = oversample in {1, 2, 4, .., 64}, H = half_width in 1..32.  With
 * q = -M[dir][c], i = floor(q / Q), p = q - Q i, output sample j of the event (n = s0 + j):
 *   a_c = sum_{k=0}^{2H-1} taps[p][k] x_c[n + i + k - H + 1]   (an fp32 fma chain from 0 in ascending k)
 *   y   = (((0 + a_0) + a_1) + ... + a_{C-1}) * float32(1 / C)
 * and samples outside [0, n) of the recording read as 0.  Every value depends on the event's own samples, its frames and these
 * tables alone.  audio_len / audio_start must be what sed_event_beam_spans wrote for the same events: an event whose entries
 * disagree with its own span, or leave [0, audio_total), is skipped.  pcm must be 16-byte aligned.  workspace: at least
 * sed_event_beam_workspace_bytes(R, channels), 16-byte aligned (the recording table; each call uploads its own).  Every argument
 * is checked before anything is enqueued; E = 0 or audio_total = 0 launches nothing.
 * The _ring forms read the rings of live feeds as sed_event_tdoa_ring does (ring, ring_len, cap, n_host [R] = samples received):
 * sample s of feed r, channel c at ring[(r C + c) cap + s % cap]; samples before max(0, n - cap) read as 0 (no event that
 * sed_event_doa_ring located reaches them).  An extracted event gets, bit for bit, what the linear call gives on the feed's
 * samples [0, n).  workspace: sed_event_beam_ring_workspace_bytes(R). */
size_t sed_event_beam_workspace_bytes(int R, int channels);
size_t sed_event_beam_ring_workspace_bytes(int R);
int sed_event_beam_spans(long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_onset,
                         const int* ev_offset, const int* ev_peak_frame, const int* ev_dir, const int* ev_loc_frames, long E,
                         int time_factor, int hop, int max_frames, int D, int* len_out, long* start_out, long* total_out,
                         void* workspace, size_t workspace_bytes, void* stream);
int sed_event_beam_spans_ring(const long* n_host, int R, int channels, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                              const int* ev_peak_frame, const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop,
                              int max_frames, int D, int* len_out, long* start_out, long* total_out, void* workspace,
                              size_t workspace_bytes, void* stream);
int sed_event_beamform(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                       const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                       const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const int* delays, int D, int Q,
                       int H, const float* taps, const int* audio_len, const long* audio_start, float* audio, long audio_total,
                       void* workspace, size_t workspace_bytes, void* stream);
int sed_event_beamform_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const int* ev_rec,
                            const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                            const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const int* delays, int D,
                            int Q, int H, const float* taps, const int* audio_len, const long* audio_start, float* audio,
                            long audio_total, void* workspace, size_t workspace_bytes, void* stream);
/* sed_event_mvdr: the audio of every located event through an adaptive (MVDR) beam.  The arguments are
 * sed_event_beamform's with, in place of the delays and the filter, tau: DEVICE float64 [D][C], the delay of channel c for
 * direction d in samples (sr (r_c - rbar) . u_d / c, not rounded); loading in [1e-6, 1e6]; tables: a blob of
 * sed_logmel_build_tables made with the window w[m] = sqrt(0.5 - 0.5 cos(2 pi m / 2048)), of which the header, the window and the
 * twiddles are read.  The events, their samples [s0, s1) and audio_len / audio_start are sed_event_beam_spans'.  The transform grid
 * is the event's own: N = 2048, B = 1024, len = s1 - s0, J = ceil(len / B); frame j = 0..J holds x_c[s0 + (j - 1) B + m] with every
 * sample outside [s0, s1) read as 0.  Per bin k = 0..1024, with X_j the C spectra of frame j:
 *   R = sum_j X_j X_j^H                                   (fp32, ascending j)
 *   d_c = exp(+2 pi i k tau[dir][c] / 2048),  v = (R + loading trace(R) / C I)^-1 d,  w = v / (d^H v)   (float64; stored as fp32)
 *   trace(R) not > 0: w = d / C
 *   Y_j = sum_c conj(w_c) X_{c,j}                         (ascending c; the imaginary parts of Y[0] and Y[1024] are dropped)
 * and with v_j the inverse real FFT of Y_j, output sample i = j B + m < len is w[m + B] v_j[m + B] + w[m] v_{j+1}[m].  An event's
 * audio depends on its own samples, tau[dir] and loading alone.  workspace: 16-byte aligned, at least
 * sed_event_mvdr_workspace_bytes(R, channels, max_frames, hop) — the recording table and ONE event's covariance partials and
 * weights; with more, as many events as fit (at most 65535) go through the three launches at a time, which changes no bit.
 * Every argument is checked before anything is enqueued; E = 0 or audio_total = 0 launches nothing; an event whose audio_len /
 * audio_start disagree with its own span, or leave [0, audio_total), is skipped. */
size_t sed_event_mvdr_workspace_bytes(int R, int channels, int max_frames, int hop);
int sed_event_mvdr(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_onset,
                   const int* ev_offset, const int* ev_peak_frame, const int* ev_dir, const int* ev_loc_frames, long E,
                   int time_factor, int hop, int max_frames, const double* tau, int D, double loading, const void* tables,
                   size_t tables_bytes, const int* audio_len, const long* audio_start, float* audio, long audio_total,
                   void* workspace, size_t workspace_bytes, void* stream);
/* sed_event_mvdr_ring: sed_event_mvdr on the PCM rings of live feeds, as sed_event_beamform_ring relates to
 * sed_event_beamform: recording r is a feed that has received n_host[r] samples, its channel ch the ring of cap samples at
 * (r*C + ch)*cap, sample i at i % cap while max(0, n - cap) <= i < n (sed_stream_ring_write); cap >= 2048, cap % 4 == 0,
 * R*C*cap <= ring_len.  The spans are sed_event_beam_spans_ring's.  A sample outside what the ring still holds reads as 0.  An
 * extracted event's audio is, bit for bit, what sed_event_mvdr gives on the feed's samples [0, n) laid out linearly, wherever
 * the ring wraps.  workspace: at least sed_event_mvdr_ring_workspace_bytes(R, channels, max_frames, hop) — the table of the
 * sample counts and one event's partials and weights. */
size_t sed_event_mvdr_ring_workspace_bytes(int R, int channels, int max_frames, int hop);
int sed_event_mvdr_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const int* ev_rec,
                        const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                        const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                        double loading, const void* tables, size_t tables_bytes, const int* audio_len, const long* audio_start,
                        float* audio, long audio_total, void* workspace, size_t workspace_bytes, void* stream);

/* sed_event_mvdr_noise / sed_event_mvdr_noise_ring: sed_event_mvdr / sed_event_mvdr_ring with the covariance taken from
 * before the onset.  noise_blocks = Kn in [0, 256], noise_guard = G in [0, 64], in blocks of B = 1024 samples.  An extracted event
 * [s0, s1) with s0 >= (G + Kn + 1) B gets its weights from Rn[k] = sum_q X_q X_q^H over the Kn frames q = 0..Kn-1 of 2048 samples
 * that start at s0 - (G + Kn + 1 - q) B of its RECORDING (they cover [s0 - (G + Kn + 1) B, s0 - G B); fp32, ascending q, chunks
 * of 32 frames added in ascending order), by sed_event_mvdr's formula with Rn in place of R; the frames that are combined and
 * the output are unchanged.  Every other extracted event gets sed_event_mvdr's audio, bit for bit.  noise_frames_out: DEVICE int32
 * [E], Kn for an event that used the noise covariance, 0 for every other one; it is written when something is launched (E = 0
 * or audio_total = 0 launches nothing: no event is extracted).  Kn = 0 is sed_event_mvdr with noise_frames_out zeroed.  On a ring
 * a noise sample the ring no longer holds reads as 0.  With Kn > 0 a recording (a feed) has fewer than 2^42 samples.  An event's audio is a function of those samples and [s0, s1) of its own
 * recording, tau[dir] and the settings alone.  workspace: at least sed_event_mvdr_noise_workspace_bytes(R, channels, max_frames,
 * hop, noise_blocks) (0: refused sizes) — per event max(the chunks of the own frames, ceil(Kn / 32)) chunk slots.  Every argument
 * is checked on the host before anything is enqueued; messages begin with "mvdr_noise:" / "mvdr_noise_ring:". */
size_t sed_event_mvdr_noise_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks);
int sed_event_mvdr_noise(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                         const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                         const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                         double loading, int noise_blocks, int noise_guard, const void* tables, size_t tables_bytes,
                         const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_mvdr_noise_ring_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks);
int sed_event_mvdr_noise_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const int* ev_rec,
                              const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                              const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                              double loading, int noise_blocks, int noise_guard, const void* tables, size_t tables_bytes,
                              const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* sed_event_quiet_frames / sed_event_mvdr_quiet: the noise covariance of sed_event_mvdr_noise from the frames where the
 * event's class is silent.  Settings: Kn = noise_blocks in [1, 256], G = noise_guard in [0, 64], S = noise_search in [Kn, 1024],
 * M = noise_min in [1, Kn], n_classes in [1, 32], exclude_any 0 or 1; B = 1024, H = time_factor * hop.  All of the rule is integer:
 *   mask[r][t], t < L_r = n_r / H + 1, has bit k set when some row of the WHOLE table — located or not — has rec = r, cls = k and
 *     onset <= t < offset (both clamped to [0, L_r]); a row with rec outside [0, R), cls outside [0, n_classes) or onset < 0 marks nothing;
 *   candidate q = 0..S-1 of an extracted event [s0, s1) is the 2048 samples from s0 - (G + 2 + q) B; it exists when that is >= 0 and
 *     is eligible when mask[r][t] & excl == 0 for every t = max(lo, 0) / H .. ceil(hi / H) - 1 of [lo, hi) = [s0 - (2 G + 2 + q) B,
 *     s0 - q B); excl = 1 << cls, or all bits with exclude_any;
 *   the first Kn eligible candidates in ascending q are selected, n_e of them; an extracted event with cls in [0, n_classes) and
 *     n_e >= M gets its weights from Rn = sum X X^H over them in ascending time (descending q; fp32, chunks of 32 frames added in
 *     ascending order; a sample outside the recording reads as 0), by sed_event_mvdr's formula with Rn in place of R.  Every other
 *     extracted event gets sed_event_mvdr's audio, bit for bit; an event whose Kn nearest candidates are eligible and whose
 *     s0 >= (G + Kn + 1) B gets sed_event_mvdr_noise's, bit for bit.
 * ev_cls: DEVICE int32 [E].  noise_frames_out: DEVICE int32 [E], n_e where the noise covariance is used, else 0; noise_sel_out: DEVICE
 * int32 [E][Kn], the used q in summation order, -1 behind them (a row of -1 where it is unused).  Both are written for every row when
 * something is launched (sed_event_quiet_frames: E > 0; sed_event_mvdr_quiet: E > 0 and audio_total > 0).  sed_event_quiet_frames is
 * the activity and the selection alone and reads no sample; sed_event_mvdr_quiet takes sed_event_mvdr_noise's arguments and these.
 * workspace: at least sed_event_quiet_frames_workspace_bytes(R, channels, mask_frames, noise_blocks) /
 * sed_event_mvdr_quiet_workspace_bytes(R, channels, max_frames, hop, noise_blocks, mask_frames) with mask_frames = sum_r L_r (0:
 * refused sizes) — the recording table, the mask and, for the beam, one event's partials and weights; the mask is made once from
 * the whole table, whatever the slicing.  Every argument is checked on the host before anything is enqueued; messages begin with
 * "quiet_frames:" / "mvdr_quiet:".  There is no ring form. */
size_t sed_event_quiet_frames_workspace_bytes(int R, int channels, long mask_frames, int noise_blocks);
int sed_event_quiet_frames(long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_cls,
                           const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                           const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, int D, int n_classes,
                           int noise_blocks, int noise_guard, int noise_search, int noise_min, int exclude_any, int* noise_frames_out,
                           int* noise_sel_out, void* workspace, size_t workspace_bytes, void* stream);
size_t sed_event_mvdr_quiet_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, long mask_frames);
int sed_event_mvdr_quiet(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                         const int* ev_cls, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                         const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                         double loading, int noise_blocks, int noise_guard, int n_classes, int noise_search, int noise_min,
                         int exclude_any, const void* tables, size_t tables_bytes, const int* audio_len, const long* audio_start,
                         float* audio, long audio_total, int* noise_frames_out, int* noise_sel_out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* sed_event_mvdr_track / sed_event_mvdr_track_ring / sed_event_mvdr_quiet_track: sed_event_mvdr_noise /
 * sed_event_mvdr_noise_ring / sed_event_mvdr_quiet with the beam steered along every event's direction track, as
 * sed_event_doa_track(_ring) wrote it: block_chunks = W in [1, 64], track_slots = Tm in [1, 256] (the columns of trk_dir), trk_len
 * DEVICE int32 [E], trk_dir DEVICE int32 [E][Tm].  The samples, the spans, the covariance (noise_blocks = 0: the own frames; Kn >= 1:
 * the frames before the onset, or the quiet selection), the transform grid, the inverse transform and the overlap-add are the
 * untracked entry's.  The rule is integer: with T = trk_len[e] clamped to [0, Tm], frame j = 0..J of an event is combined with
 *   b_j = min((j * 1024 / hop) / (32 W), T - 1),   d_j = trk_dir[e][b_j] where T > 0 and 0 <= trk_dir[e][b_j] < D, else ev_dir[e]
 *   w_b = (R + lambda I)^-1 d_b / (d_b^H (R + lambda I)^-1 d_b)     float64, ONE Cholesky factor per (event, bin), a pair of
 *                                                                   solves per block b < max(T, 1); trace(R) not > 0: d_b / C; fp32
 *   Y_j = sum_c conj(w_{b_j,c}) X_{c,j}                              ascending c
 * (the centre of frame j is sample j * 1024 of the event, which lies in located frame j * 1024 / hop).  A silent block (-1), a row
 * outside [0, D) and an event without a track (T = 0) are steered at ev_dir and never index tau.  A track whose every used row
 * equals ev_dir gives the untracked entry's audio, bit for bit.  noise_frames_out (and noise_sel_out) as in the untracked entry.
 * workspace: at least sed_event_mvdr_track_workspace_bytes(R, channels, max_frames, hop, noise_blocks, track_slots) (..._track_ring_...;
 * sed_event_mvdr_quiet_track_workspace_bytes(R, channels, max_frames, hop, noise_blocks, mask_frames, track_slots); 0: refused sizes)
 * — per event the chunk slots of the untracked entry and C rows of weights for each of Tm blocks.  Every argument is checked on the
 * host before anything is enqueued; messages begin with "mvdr_track:" / "mvdr_track_ring:" / "mvdr_quiet_track:".  E = 0 or
 * audio_total = 0 launches nothing. */
size_t sed_event_mvdr_track_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, int track_slots);
int sed_event_mvdr_track(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                         const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                         const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                         double loading, int noise_blocks, int noise_guard, const void* tables, size_t tables_bytes,
                         const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                         int block_chunks, int track_slots, const int* trk_len, const int* trk_dir, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t sed_event_mvdr_track_ring_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, int track_slots);
int sed_event_mvdr_track_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const int* ev_rec,
                              const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                              const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                              double loading, int noise_blocks, int noise_guard, const void* tables, size_t tables_bytes,
                              const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                              int block_chunks, int track_slots, const int* trk_len, const int* trk_dir, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t sed_event_mvdr_quiet_track_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, long mask_frames,
                                                  int track_slots);
int sed_event_mvdr_quiet_track(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                               const int* ev_cls, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                               const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames,
                               const double* tau, int D, double loading, int noise_blocks, int noise_guard, int n_classes,
                               int noise_search, int noise_min, int exclude_any, const void* tables, size_t tables_bytes,
                               const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                               int* noise_sel_out, int block_chunks, int track_slots, const int* trk_len, const int* trk_dir,
                               void* workspace, size_t workspace_bytes, void* stream);

/* sed_pcen: per-channel energy normalisation, IN PLACE, of the columns [col0, col0 + W) of x [rows][stride], which
 * hold log-mel values (natural log, as sed_logmel* write them without a scaler); the other columns are not touched.  Every column
 * of a recording is one chain: E[t] = scale * exp(x[t]); M[t] = (1 - smooth_b) M[t-1] + smooth_b E[t] with M[0] = E[0] (librosa's
 * lfilter_zi start); pcen[t] = (E[t] (eps + M[t])^-gain + bias)^power - bias^power; with a scaler (mu / inv_sigma: both NULL, or
 * both W wide, entry c for column col0 + c) the value written is (pcen - mu) * inv_sigma.  x = -inf (E = 0) gives pcen = 0, never NaN.
 * recs_host [R][3] = {first row, n rows, absolute index of the first frame}: a HOST table, validated on the host before anything
 * is enqueued; the recordings lie inside the matrix, are disjoint and in increasing order; n rows may be 0 (nothing is read or
 * written for it).  state: a device buffer of R*W chains x 2 floats (recording r, column c at 2 (r W + c)), or NULL when every
 * recording starts at frame 0.  It is read for a recording whose absolute index is > 0, IGNORED for index 0 (a feed that restarts
 * needs no reset call) and written back after the call, so that the next call continues with index + n rows.  The fp32
 * operations behind M[t] depend on the absolute frame t and on the data only (blocks of 64 frames aligned to t; pcen.hip): a
 * recording processed in pieces of any sizes gives bit for bit the rows of one call.  smooth_b in (0, 1] (the powers of
 * 1 - smooth_b that the kernels use are taken in double here); gain > 0, bias >= 0, power > 0, eps > 0, scale > 0.  workspace:
 * 8-byte aligned, >= sed_pcen_workspace_bytes(rows, R, W) (0 = bad sizes: rows < 2^31, R <= 2^24, 1 <= W <= 65536).  Three plain
 * launches; no workgroup waits on another. */
size_t sed_pcen_workspace_bytes(long rows, int R, int W);
int sed_pcen(float* x, long rows, int stride, int col0, int W, const long* recs_host, int R, float* state, double smooth_b,
             float gain, float bias, float power, float eps, float scale, const float* mu, const float* inv_sigma,
             void* workspace, size_t workspace_bytes, void* stream);

/* ───────────── audio at any sample rate: rational-ratio polyphase resampler, format conversion and downmix ─────────────
 * What the reference does with `ffmpeg -ac 1 -ar 44100` before feature.py:55.  L/M = sr_out/sr_in reduced; taps [L][2 half]
 * (device float32, built by the caller in double: sed_crnn_amd/resample.py) weight, for output m of a clip (ABSOLUTE index,
 * 64-bit), u = m M, i_c = u div L, p = u mod L:  y[m] = sum_k taps[p][k] x[i_c - half + 1 + k], x = 0 where the clip has
 * nothing.  The sum is taken in fp32 in one fixed order that depends on (p, k) only, so a clip resampled in pieces (a stream)
 * equals the clip resampled whole bit for bit.
 * x: x_frames sample frames of `channels` interleaved samples, format 0 = float32, 1 = int16 (scaled by 1/32768); a frame
 * becomes (sum_c x_c) * (1/channels), summed in channel order, while it is loaded.  rows_host [R][9] (HOST array, validated,
 * then uploaded into `workspace` >= sed_resample_workspace_bytes(R) on the stream) = {first frame in x, n frames, absolute
 * index of that first frame, absolute index of the first output, n outputs, first output sample in out (a multiple of 4:
 * sed_logmel_batch's aligned clip starts; rows in increasing order), hist offset, n_hist, carry_dst}: hist[hist offset, +n_hist)
 * holds the mono float32 samples that precede the frames (the carry of a stream; n_hist = 0 for a whole clip at base 0) and,
 * unless carry_dst = -1, the last 2 half samples of (history | frames) are written to hist[carry_dst, +2 half) for the next
 * call (zeros before the clip's sample 0; the two ranges must not overlap).  A row may have 0 outputs (only its carry moves).
 * Limits: L (2 half + 1) <= 26 624 floats (the padded table stays in LDS) and a tile of 1024 outputs reads at most 8192
 * samples (M/L below about 7.5); sed_resample_check_table runs every host check of sed_resample and makes no GPU call. */
size_t sed_resample_workspace_bytes(int R);
int sed_resample_check_table(const long* rows_host, int R, long x_frames, long hist_len, long out_len, int L, int M, int half);
int sed_resample(const void* x, long x_frames, int format, int channels, float* hist, long hist_len, const float* taps,
                 long taps_len, int L, int M, int half, const long* rows_host, int R, float* out, long out_len, void* workspace,
                 size_t workspace_bytes, void* stream);
/* sed_resample_select: sed_resample whose rows may KEEP a channel instead of downmixing.  rows_host [R][10]: the
 * nine columns above and `channel`: -1 = the downmix of sed_resample; c in [0, channels) = the row reads only channel c of the
 * interleaved frames, as the converted sample itself (int16 * 1/32768; no multiplication by 1/channels), so that the row equals
 * sed_resample on the de-interleaved channel bit for bit, at any tile boundary, with history and carry and at any absolute
 * base.  History and carry stay mono float32 and belong to the row: a live feed has one per (feed, channel).  Several rows may
 * read the same frames (one row per channel of a clip).  sed_resample is this entry with every channel -1.  The workspace
 * (sed_resample_select_workspace_bytes(R)) also holds the R channels; sed_resample_select_check_table is the validator without
 * a GPU call: every check of sed_resample_check_table, and a channel outside [-1, channels) is refused. */
size_t sed_resample_select_workspace_bytes(int R);
int sed_resample_select_check_table(const long* rows_host, int R, int channels, long x_frames, long hist_len, long out_len, int L,
                                    int M, int half);
int sed_resample_select(const void* x, long x_frames, int format, int channels, float* hist, long hist_len, const float* taps,
                        long taps_len, int L, int M, int half, const long* rows_host, int R, float* out, long out_len,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ───────────── GPU-resident minibatch assembly (sed.py:64-79; decorte_datamodule.py:39-49,77-111; utils.py:15-41) ─────────────
 * mel [N][C*F] (a whole fold, device-resident; channel c = columns [c*F,(c+1)*F)), lab [N][K].
 * starts [B] window starts (clamped to [0, N-L] like the reference's fallback); tmask/fmask [B][n_masks] SpecAugment
 * offsets (-1 = skip; zeroes time_w frames / freq_w mel bins, all channels) or NULL with n_masks = 0.
 * x [B][C][F][L] (the network input layout), y [B][L/pool][K] = max over each group of `pool` frames. */
int sed_window_batch(const float* mel, const float* lab, long N, int C, int F, int K, const int* starts,
                     const int* tmask, const int* fmask, int n_masks, int time_w, int freq_w,
                     float* x, float* y, int B, int L, int pool, void* stream);
/* utils.split_in_seqs + split_multi_channels in one pass: feat [N][C*F] -> out [N/S][C][F][S] (time_last=1, network
 * input) or [N/S][C][S][F] (time_last=0, the utils.py layout); the N %% S remainder is dropped. */
int sed_pack_sequences(const float* feat, long N, int C, int F, int S, int time_last, float* out, void* stream);
/* StandardScaler.fit (feature.py:127-128): per-column mean and population sigma with sklearn's rules — float64
 * accumulation, centred two-pass variance, and scale 1 for a column whose variance is within that algorithm's rounding
 * bound (sklearn's _is_constant_feature: var <= N*eps*var + (N*mean*eps)^2).  x [N][F] f32, any F (256-column chunks); mean / stdv are
 * FLOAT64 device arrays [F], like sklearn's mean_ / scale_ (a float32 mean would already cost 5 % of a sigma on a column
 * whose mean is 1e6 sigmas). */
size_t sed_col_mean_std_workspace_bytes(int F);
int sed_col_mean_std(const float* x, long N, int F, double* mean, double* stdv, void* workspace, void* stream);
/* StandardScaler.transform (feature.py:128-129): out = f32(f32(x - mean[col]) / stdv[col]) (sklearn's two in-place
 * float32 roundings); mean / stdv float64 [F]; out may alias x. */
int sed_col_standardize(const float* x, long N, int F, const double* mean, const double* stdv, float* out, void* stream);

/* Segment-based metric counts (metrics.py:20-68) and the 2x2 confusion counts (crnn_lightning.py:112-119) of thresholded
 * predictions on the device: pred/lab [rows][K] (windows concatenated, K <= 32; labels are 0/1), 1-second blocks of
 * `block` rows.  counts17 (uint64, device):
 * [0..5] frame-wise TP,Nref,Nsys,S,D,I; [6..8] TP,Nref,Nsys over ceil(rows/block) blocks (F1 keeps the partial block);
 * [9..12] S,D,I,Nref over floor(rows/block) blocks (ER drops it); [13..16] element-wise tn,fp,fn,tp with the
 * reference's uint8 truncation of the label (label in [0,1) counts as 0, [1,2) as 1).  Integer arithmetic: exact. */
#define SED_SEGMENT_COUNTS 17
int sed_segment_counts(const float* pred, const float* lab, long rows, int K, int block, float threshold,
                       unsigned long long* counts17, void* stream);

/* ───────────── whole-recording event detection (sed_crnn_amd/detect.py) ─────────────
 * The eval forward runs on windows of a recording; these two entries turn its window logits into events.  Frames here are
 * OUTPUT frames (tf = product of the time pools input frames each).  Window w covers output frames
 * [start(w), start(w) + win_out) with start(w) = min(w * hop_out, last_start_out): the regular grid plus, where the last regular
 * window stops short, one extra window aligned to the end (last_start_out + win_out == n_out).
 * sed_detect_stitch: logits [n_win][win_out][K] -> probs [n_out][K] = sigmoid, then combined over the covering windows
 * (combine 0 = mean, 1 = max) in increasing window order (bitwise deterministic, no atomics); `trim` drops that many outermost
 * frames of each window on the sides that do not touch the recording's ends (refused if it would leave a frame uncovered). */
int sed_detect_stitch(const float* logits, long n_win, int win_out, int K, int hop_out, long last_start_out, long n_out,
                      int combine, int trim, float* probs, void* stream);
/* sed_detect_events: probs [n_out][K] (K <= 32), per class: median filter of odd width `median` (1 = off, <= 31; edges
 * 'nearest'), runs of p' > lo kept when max p' > hi (hi >= lo), kept runs merged across gaps of <= min_gap frames, events
 * shorter than min_len frames dropped.  Event e: cls, onset (inclusive), offset (exclusive), peak = max of the UNFILTERED track
 * over the event, peak_frame = its first arg-max; sorted by (class, onset).  *count (device int) = the true number of events;
 * at most max_events are written (0: count only, the outputs may then be NULL), so a host can grow its buffers and rerun.
 * workspace >= sed_detect_workspace_bytes(n_out, K, max_events) (0 = bad sizes). */
size_t sed_detect_workspace_bytes(long n_out, int K, int max_events);
int sed_detect_events(const float* probs, long n_out, int K, int median, float lo, float hi, int min_gap, int min_len,
                      int max_events, void* workspace, size_t workspace_bytes, int* cls, int* onset, int* offset,
                      float* peak, int* peak_frame, int* count, void* stream);
/* Batches of R recordings packed back to back (the tracks of recording r are rows [off_r, off_r + n_out_r) of probs).
 * Recording tables are HOST arrays, validated and then uploaded into `workspace` on the stream (a bad table is an error,
 * never a read out of bounds).  workspace >= sed_detect_batch_workspace_bytes(n_total, K, R, max_events) for both entries
 * (n_total = sum of n_out_r < 2^31, n_total * K < 2^31; 0 = bad sizes).
 * sed_detect_stitch_batch: recs_host [R][6] = {first logit (float index into logits [logits_len]), n_win, win_out, hop_out,
 * last_start_out, n_out} per recording, logit extents n_win*win_out*K inside the buffer and not overlapping (any order);
 * every grid checked like sed_detect_stitch's.  probs [n_total][K]: each recording's rows equal sed_detect_stitch of its logits.
 * sed_detect_events_batch: n_out_host [R]; the decoder of sed_detect_events per recording (the median clamps, runs, gaps and
 * events stop at each recording's ends; onset / offset / peak_frame are local to the recording), events sorted by
 * (recording, class, onset) with rec = the recording.  event_off [R+1] (device ints): recording r's events are
 * [event_off[r], event_off[r+1]); event_off[R] = the true total.  At most max_events are written (0: counts only). */
size_t sed_detect_batch_workspace_bytes(long n_total, int K, int R, int max_events);
int sed_detect_stitch_batch(const float* logits, long logits_len, const long* recs_host, int R, int K, int combine, int trim,
                            float* probs, long n_total, void* workspace, size_t workspace_bytes, void* stream);
int sed_detect_events_batch(const float* probs, const long* n_out_host, int R, int K, int median, float lo, float hi, int min_gap,
                            int min_len, int max_events, void* workspace, size_t workspace_bytes, int* rec, int* cls, int* onset,
                            int* offset, float* peak, int* peak_frame, int* event_off, void* stream);

/* ───────────── decoder sweep (sed_crnn_amd/tune.py) ─────────────
 * Scores the events of sed_detect_events_batch against reference events for G decoder settings at once, without writing an
 * event and without a read back.  probs [n_total][K] and n_out_host [R] as in sed_detect_events_batch.  settings_host [G]: the
 * five decoder values of each setting, checked like that entry's (median odd 1..31, hi >= lo, min_gap >= 0, min_len >= 1).
 * Reference events (DEVICE arrays, validated by the caller): ref_off [R*K + 1] is a CSR over (recording, class); within one
 * (recording, class) the events [ref_onset, ref_offset) are sorted, pairwise disjoint and inside [0, n_out_r]; all four arrays
 * non-NULL even when there is no event.  Matching per (recording, class): the system events in order, each taken by the first
 * unmatched reference event j with |onset - ref_onset[j]| <= collar (0..31 output frames) and, when ref_tol[j] >= 0,
 * |offset - ref_offset[j]| <= ref_tol[j].  Segments: blocks of `block` (>= 1) output frames from each recording's frame 0, the
 * partial last block kept; a block is active on a side when an event of that side covers one of its frames.
 * counts [G][K][6] (device, int64, cleared by the call) = ev_tp, n_sys, n_ref, seg_tp, seg_sys, seg_ref summed over recordings:
 * integer arithmetic, exact and repeatable.  One bit track is packed per distinct (median, threshold value) among the settings'
 * lo and hi; workspace >= sed_tune_workspace_bytes(n_total, K, R, n_tracks, G) with n_tracks that number (0 = bad sizes;
 * G in 1..2^20, n_tracks in 1..2G).  G = 0 is a no-op that returns 0 once the recording table has been checked. */
typedef struct sed_tune_setting { int median; float lo, hi; int min_gap, min_len; } sed_tune_setting;
size_t sed_tune_workspace_bytes(long n_total, int K, int R, int n_tracks, int G);
int sed_tune_sweep(const float* probs, const long* n_out_host, int R, int K, const sed_tune_setting* settings_host, int G,
                   const int* ref_off, const int* ref_onset, const int* ref_offset, const int* ref_tol, int collar, int block,
                   void* workspace, size_t workspace_bytes, long* counts, void* stream);

/* ───────────── PSDS: intersection criteria over a grid of settings (sed_crnn_amd/tune.py) ─────────────
 * The integer side of the polyphonic sound detection score: for G decoder settings at once, the events of
 * sed_detect_events_batch are judged against reference events by how much of them intersects the reference, without writing an
 * event and without a read back.  probs, n_out_host, settings_host and the reference arrays are those of sed_tune_sweep, with
 * the same checks and limits.  Criteria in thousandths (dtc_milli, gtc_milli in 1..1000; cttc_milli in 1..1000, or 0 for no
 * cross triggers); |x ∩ G_c| = the frames of x covered by reference events of class c; every comparison is a 64-bit integer
 * one.  Per (setting, recording, class k), with D the system events: d in D is relevant iff 1000 |d ∩ G_k| >= dtc_milli |d|; a
 * reference event t of class k is a true positive iff 1000 (sum over relevant d of |d ∩ t|) >= gtc_milli |t|; every other d is
 * a false positive of class k and, when cttc_milli > 0, a cross trigger (k -> c) for every class c != k with
 * 1000 |d ∩ G_c| >= cttc_milli |d|.  counts [G][K][4] (device, int64, cleared by the call) = tp, n_ref, n_sys, fp summed over
 * recordings; ct [G][K][K] (device, int64; row k, column c = cross triggers of detections of class k on the reference of class
 * c, the diagonal 0) is cleared and written only when cttc_milli > 0 and may be NULL otherwise.  The workspace is
 * sed_tune_sweep's with a per-frame prefix: >= sed_psds_workspace_bytes(n_total, K, R, n_tracks, G) (0 = bad sizes).  G = 0 is a
 * no-op that returns 0 once the recording table has been checked. */
size_t sed_psds_workspace_bytes(long n_total, int K, int R, int n_tracks, int G);
int sed_psds_sweep(const float* probs, const long* n_out_host, int R, int K, const sed_tune_setting* settings_host, int G,
                   const int* ref_off, const int* ref_onset, const int* ref_offset, int dtc_milli, int gtc_milli, int cttc_milli,
                   void* workspace, size_t workspace_bytes, long* counts, long* ct, void* stream);

/* ───────────── live streams (sed_crnn_amd/stream.py) ─────────────
 * S feeds keep their state on the device between calls, in ONE caller-owned buffer of sed_stream_state_bytes(...) bytes (0 = bad
 * sizes: S in 1..65535, K in 1..32, 1 <= hop_out <= win_out, median odd 1..31, max_new_windows in 1..1024; the size depends on
 * these arguments only): per stream a ring of window logits (window w in slot w mod WR, WR = 2 ceil(win_out / hop_out) +
 * max_new_windows + 2), a ring of track rows (frame j in row j mod TR, TR = median - 1 + win_out + (max_new_windows + 1) hop_out + 2)
 * and, per class, the decoder's state (open run, pending event, gap peak, decided frames).  Frames are OUTPUT frames from the
 * start of the stream.  sed_stream_init clears every stream, sed_stream_reset the listed ones (streams_host NULL = all).
 * sed_stream_step advances all streams: table_host [S][8] = {n_new windows, first logit (float index into logits
 * [logits_len]), index of the first new window, n_out before, n_out now, end (0 / 1), output frames
 * per new window (win_out; n_out for the single window of a stream that ends below win_out), first row in probs}.  The table is
 * validated on the host against the window grid (regular window w is complete iff w hop_out + win_out <= n_out; at the end the
 * offline grid's last window must arrive), then uploaded.  Track frame j is final iff j < n_out - win_out (all of them at the
 * end) and is stitched by the device function of sed_detect_stitch; filtered frame g is decided once track frame g + median/2 is
 * final (the 'nearest' clamp at the right edge applies at the end only).  A pending event [a, b) is emitted in the first step in
 * which more than b + min_gap frames are decided and no run that began at or before b + min_gap is still open; at the end
 * everything left is emitted and the stream restarts at frame 0.  Events: ev_stream, cls, onset, offset (exclusive), peak (max of
 * the unfiltered track over the event, kept as a running value), peak_frame, sorted by (stream, class, onset); event_off [S+1]
 * (device ints), event_off[S] = the true total, at most max_events are written (the state advances either way: size the outputs
 * to sum_s K ((decided frames of s in this step) / 2 + 2)).  probs (may be NULL) receives the newly final track rows.
 * max_new_decided >= every stream's newly decided frames; workspace >= sed_stream_step_workspace_bytes(S, K, max_new_decided).
 * sed_stream_append: per stream, [buf[src, +n_keep) | fresh[new, +n_new)] goes to work[work, ...) (work may be NULL) and its
 * last n_tail floats to buf[dst, ...): table_host [S][7] = {src, n_keep, new, n_new, work, dst, n_tail}; stream s owns
 * buf[s stride, (s+1) stride), src and dst must not overlap.  The PCM carry and the feature rows of the streams move with it. */
size_t sed_stream_state_bytes(int S, int K, int win_out, int hop_out, int median, int max_new_windows);
int sed_stream_init(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median, int max_new_windows,
                    void* stream);
int sed_stream_reset(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median, int max_new_windows,
                     const int* streams_host, int n_streams, void* stream);
size_t sed_stream_step_workspace_bytes(int S, int K, int max_new_decided);
int sed_stream_step(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median, int max_new_windows,
                    int combine, int trim, float lo, float hi, int min_gap, int min_len, const float* logits, long logits_len,
                    const long* table_host, int max_new_decided, float* probs, long probs_rows, int max_events, int* ev_stream,
                    int* cls, int* onset, int* offset, float* peak, int* peak_frame, int* event_off, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t sed_stream_append_workspace_bytes(int S);
int sed_stream_append(float* buf, long buf_len, long stride, const float* fresh, long fresh_len, float* work, long work_len,
                      const long* table_host, int S, void* workspace, size_t workspace_bytes, void* stream);

/* ───────────── class-wise decoder settings ─────────────
 * The three decoding entries with one row of decoder values PER CLASS: classes_host [K] (a HOST array, K <= 32) takes the place
 * of the scalar entries' median, lo, hi, min_gap, min_len; class k is decoded with row k — its own median width, thresholds, gap
 * merge and minimum length — and peaks still read the unfiltered track.  Every row is checked like the scalar values and a
 * refusal names the class ("...: class 3: need hi >= lo ..."); nothing is launched on a refusal.  The rows travel to the
 * kernels by value: workspaces, state, tables and outputs are exactly those of the scalar entries, with the same size functions.
 * Class k's events are bit for bit the class-k events of the scalar entry run with row k.
 * sed_stream_step_classwise: `median` (here and in sed_stream_state_bytes / sed_stream_init / sed_stream_reset) must be the
 * WIDEST median of the K classes.  There is one frontier per feed: filtered frame g of every class is decided once track frame
 * g + median/2 is final; a pending event [a, b) of class k is emitted in the first step in which more than b + min_gap_k frames
 * are decided and no run of class k that began at or before b + min_gap_k is still open. */
typedef sed_tune_setting sed_decoder_setting;
int sed_detect_events_classwise(const float* probs, long n_out, int K, const sed_decoder_setting* classes_host, int max_events,
                                void* workspace, size_t workspace_bytes, int* cls, int* onset, int* offset, float* peak,
                                int* peak_frame, int* count, void* stream);
int sed_detect_events_batch_classwise(const float* probs, const long* n_out_host, int R, int K,
                                      const sed_decoder_setting* classes_host, int max_events, void* workspace, size_t workspace_bytes,
                                      int* rec, int* cls, int* onset, int* offset, float* peak, int* peak_frame, int* event_off,
                                      void* stream);
int sed_stream_step_classwise(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median, int max_new_windows,
                              int combine, int trim, const sed_decoder_setting* classes_host, const float* logits, long logits_len,
                              const long* table_host, int max_new_decided, float* probs, long probs_rows, int max_events,
                              int* ev_stream, int* cls, int* onset, int* offset, float* peak, int* peak_frame, int* event_off,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ───────────── whole-network plan (TimePooledCRNN.forward sed.py:105-112 / crnn_lightning.py:66-73) ───────────── */
typedef struct sed_net_cfg {
    int B, Cin, F, T;                 /* input x [B][Cin][F][T] */
    int n_conv;
    int C[SED_MAX_CONV];              /* conv channels */
    int pool_f[SED_MAX_CONV], pool_t[SED_MAX_CONV];
    float drop_p[SED_MAX_CONV];       /* dropout after block i (0 = none) */
    int n_gru;
    int H[SED_MAX_GRU];               /* hidden size per direction of each stacked BiGRU layer */
    int n_dense;
    int D[SED_MAX_DENSE];             /* dense sizes; ReLU between layers, last = classes (logits) */
    float bn_eps, bn_momentum;
    int conv_mode;                    /* 0 = exact fp32 (default); 1 = EXPERIMENT: conv forward, data gradient and weight gradient of the
                                         MFMA blocks on the 3-term bf16 split (sed_conv3x3_fwd_ex / sed_conv3x3_wgrad_ex);
                                         2 = bf16 INFERENCE plan (training = 0 only, sed_net_forward only): the supported conv blocks
                                         at the top of the stack and the GRU layer-0 input projection on bf16 operands
                                         (sed_net_inference_plan says which), everything else as mode 0 */
    int flags;                        /* 0 (default) | SED_NET_* below: measurement / test switches of the backward schedule */
} sed_net_cfg;
/* The last backward phase runs the first block's passes (auxiliary stream) BESIDE the deferred MFMA weight gradients (main
 * stream); the persistent MFMA kernel must hold its CUs before the passes move in.  That order is a DEPENDENCY: the kernel's
 * workgroups announce themselves on a counter in the workspace and a one-wave gate at the head of the auxiliary chain waits
 * for them.  SED_NET_AUX_FIRST (tests): the host enqueues the auxiliary chain before the main-stream kernel — the adversarial
 * order, which must give the same gradients at the same speed.  SED_NET_NO_GATE (A/B measurements): no gate. */
#define SED_NET_AUX_FIRST 0x1
#define SED_NET_NO_GATE 0x2
#define SED_NET_DIRECT_CONV 0x4     /* the 128-channel blocks on the direct 3x3 kernels instead of the Winograd form (A/B measurements, tests) */

typedef struct sed_net_params {      /* pointers in the reference's own layouts */
    float* conv_w[SED_MAX_CONV];      /* [C][Cin][3][3] */
    float* conv_b[SED_MAX_CONV];
    float* bn_g[SED_MAX_CONV];
    float* bn_b[SED_MAX_CONV];
    float* bn_rm[SED_MAX_CONV];       /* running stats (params struct only; unused in grads) */
    float* bn_rv[SED_MAX_CONV];
    float* gru_wih[SED_MAX_GRU][2];   /* [3H][in]  (dir 1 = *_reverse) */
    float* gru_whh[SED_MAX_GRU][2];   /* [3H][H] */
    float* gru_bih[SED_MAX_GRU][2];
    float* gru_bhh[SED_MAX_GRU][2];
    float* dense_w[SED_MAX_DENSE];    /* [out][in] */
    float* dense_b[SED_MAX_DENSE];
} sed_net_params;

/* Output time steps / features of the conv stack for cfg (T', F'); returns <0 on a bad cfg. */
int sed_net_out_shape(const sed_net_cfg* cfg, int* Tp, int* Fp);
size_t sed_net_workspace_bytes(const sed_net_cfg* cfg, int training);
/* logits [B][T'][D_last].  training=1: batch statistics, dropout, activations kept in `workspace`
 * for sed_net_backward; running stats updated in place. */
int sed_net_forward(const sed_net_cfg* cfg, const sed_net_params* p, const float* x, float* logits,
                    void* workspace, int training, uint64_t seed, const uint64_t* seed_dev, void* stream);
/* Gradients of every parameter into `g` (same layouts as `p`; written, not accumulated).
 * Stages let the host overlap the gradient all-reduce with the rest of backward:
 *   stage 0 = dense head + GRU stack, stage s>=1 = conv block l = n_conv - s.  Run stages
 *   [stage_begin, stage_end) in increasing order; (0, n_conv+1) = everything.
 * The critical chain of the conv backward is dgrad(top) -> BN(top-1) -> ... -> dgrad(1) -> BN(0); the weight gradients
 * hang off it and are deferred to the stage of block 1, where all of them run back to back.  Hence the gradients of
 * stage 0 are complete on `stream` when stage 0 returns, and those of conv block l when stage
 * sed_net_backward_ready_stage(cfg, l) returns (block 0: the last stage; every other block: the stage of block 1).
 * aux_stream (NULL or == stream: serial): a second hipStream_t for the HBM-bound BatchNorm/ReLU/pool backward passes
 * that have MFMA-bound work to hide behind: BN(top) beside the GRU weight-gradient GEMM (issued by stage 0), BN(0) (for
 * a fused first block: all of block 0) beside the conv weight gradients (issued by the stage of block 1); it also takes
 * the weight gradients that have a latency- or HBM-bound pass of the data-gradient chain to run beside: the small GRU
 * weight-gradient GEMMs of the layers above the first (beside the recurrences) and the top conv block's weight gradient
 * (beside the BatchNorm backward of the block below it).  hipEvents
 * order the two streams and every auxiliary launch is joined back into `stream` before the last stage returns.
 * Stages must therefore be run in order with the same aux_stream for the whole backward. */
int sed_net_backward(const sed_net_cfg* cfg, const sed_net_params* p, const sed_net_params* g,
                     const float* x, const float* dlogits, void* workspace, uint64_t seed, const uint64_t* seed_dev,
                     int stage_begin, int stage_end, void* stream, void* aux_stream);
/* Stage of sed_net_backward after which every gradient of conv block `block` is complete (<0: bad arguments). */
int sed_net_backward_ready_stage(const sed_net_cfg* cfg, int block);

/* Phased execution, for synchronised BatchNorm in data-parallel training: the per-block statistics
 * are the only cross-sample coupling besides the loss mean, so the plan can stop at them.
 *   forward phases : 2l   = conv block l + its statistic sums (training),
 *                    2l+1 = finalise with count*count_scale, normalise/ReLU/pool/dropout,
 *                    2*n_conv = GRU stack + dense head.
 *   backward phases: 0    = dense head + GRU stack,
 *                    2k+1 = BatchNorm-backward sums (sum g, sum g*xhat) of block l = n_conv-1-k,
 *                    2k+2 = rest of block l (apply, weight/bias/data gradients); its gradients are then complete.
 * Between phase 2l and 2l+1 (forward) / 2k+1 and 2k+2 (backward) the host all-reduces (SUM) the workspace region
 * sed_net_sync_region() names; count_scale = number of ranks (1 = unsynchronised).  Single stream, no overlap. */
int sed_net_sync_region(const sed_net_cfg* cfg, int backward, int block, size_t* offset_bytes, size_t* n_floats);
int sed_net_forward_phases(const sed_net_cfg* cfg, const sed_net_params* p, const float* x, float* logits,
                           void* workspace, int training, uint64_t seed, int phase_begin, int phase_end,
                           float count_scale, void* stream);
int sed_net_backward_phases(const sed_net_cfg* cfg, const sed_net_params* p, const sed_net_params* g,
                            const float* x, const float* dlogits, void* workspace, uint64_t seed,
                            int phase_begin, int phase_end, float count_scale, void* stream);

/* Where an intermediate of the plan lives inside `workspace` (offsets are a pure function of cfg and `training`), for hosts
 * that read activations and for parity tests of intermediates.  name / index:
 *   "conv_out"[l] conv output of block l, channels-last [B][T_l][F_l][C] (absent for a recomputed first block);
 *   "pooled"[l] block output [B][T_l/pt][F_l/pf][C] (last block: [B][T'][C][F'], the GRU feature order, except in the eval
 *   plans whose last block pools in its conv epilogue: channels-last there); a bf16 block of the bf16 inference plan
 *   (sed_net_inference_plan) stores bf16 elements and n_floats counts ELEMENTS;
 *   "mean" / "rstd" / "scale" / "shift"[l] the batch statistics and fused BatchNorm coefficients of block l ([C]);
 *   "gi"[i] / "gru_out"[i] input projections [M][2][3H] and outputs [M][2H] of GRU layer i;
 *   training only: "dconv"[l] gradient of block l's conv output, "dgru_out"[i], "grad_act"[0] the buffer that carries the
 *   gradient of the pooled output being back-propagated (reused from block to block; when the first block's sums come out of
 *   the Winograd data gradient of block 1, the gradient of block 0's pooled output is never written: after a backward the
 *   buffer then holds the gradient of block 1's pooled output), "bn_sums_bwd"[0] (sum g, sum g*xhat),
 *   "wgrad_zero_row"[0|1] the zero-filled rows at the head of the weight-gradient scratch of the main / auxiliary stream
 *   (SED_WGRAD_ZERO_ROW_CLEAN: sed_net_backward re-clears them in every call that holds stage 0).
 * <0: unknown name / index for this plan. */
int sed_net_workspace_region(const sed_net_cfg* cfg, int training, const char* name, int index,
                             size_t* offset_bytes, size_t* n_floats);

/* The ReLU-gate / arg-max decisions (codes of sed_bn_relu_pool_route) of conv block `block` in the last TRAINING forward that
 * ran on `workspace` with input `x`; route: caller-owned [B][T_l/pt][F_l/pf][C] bytes.  Dispatches to sed_bn_relu_pool_route
 * (stored conv output) or sed_conv1_route (recomputed first block: it re-reads p->conv_b, so call this before the optimiser
 * moves the parameters).  For the parity tests of the gradient routing of
 * `loss.backward()` (sed.py:137): see oracle/crnn_ref.py forward_routed. */
/* What the eval plan of cfg runs in bf16 (conv_mode 2; zeros otherwise): conv_bf16[n_conv] per conv block (weights, input and
 * pooled output bf16 — its "pooled" region then holds bf16 elements), *proj_bf16 for the GRU layer-0 input projection. */
int sed_net_inference_plan(const sed_net_cfg* cfg, int* conv_bf16, int* proj_bf16);

int sed_net_routing(const sed_net_cfg* cfg, const sed_net_params* p, const float* x, const void* workspace, int block,
                    unsigned char* route, void* stream);

/* ───────────── in-library kernel timers — MEASUREMENT ONLY, off by default ─────────────
 * The one exception to the conventions at the top of this header: this group keeps process-wide mutable state (the
 * enabled mask and the recorded event pairs, guarded by a mutex) and sed_prof_read SYNCHRONISES (hipEventSynchronize
 * on every recorded pair).  Nothing in the product path enables it; bench.py does, for the `roofline` object.
 * When a tag's bit is set in `tag_mask`, every launch of that kernel family is bracketed by a pair of
 * hipEvents on the launch stream and tagged with its algorithmic work (FLOPs for the MFMA kernels,
 * bytes for the streaming ones).  sed_prof_read waits for the recorded events and returns the totals
 * since the last sed_prof_enable.  With the mask at 0 (the default) every entry is exactly as documented above:
 * no event is recorded and no state is touched. */
enum sed_kernel_tag {
    SED_K_CONV_MFMA_FWD = 0,   /* units: FLOPs */
    SED_K_CONV_SMALL_FWD,      /* units: bytes */
    SED_K_CONV_MFMA_WGRAD,     /* units: FLOPs */
    SED_K_CONV_SMALL_WGRAD,    /* units: bytes */
    SED_K_BN_FWD,              /* units: bytes */
    SED_K_BN_BWD_REDUCE,       /* units: bytes */
    SED_K_BN_BWD_APPLY,        /* units: bytes */
    SED_K_GEMM,                /* units: FLOPs */
    SED_K_GRU_FWD,             /* units: FLOPs */
    SED_K_GRU_BWD,             /* units: FLOPs */
    SED_K_ADAM,                /* units: bytes */
    SED_K_LOGMEL,              /* units: bytes (hop*4 read + n_mels*4 written per frame) */
    SED_K_CONV_MFMA_DGRAD,     /* units: FLOPs — sed_conv3x3_dgrad_bnred (the forward kernel with the BatchNorm-backward epilogue) */
    SED_K_COUNT
};
int sed_prof_enable(unsigned tag_mask);
int sed_prof_read(int tag, double* total_ms, long* launches, double* total_units);
const char* sed_prof_tag_name(int tag);
int sed_prof_tag_count(void);                /* = SED_K_COUNT of the loaded library */

#ifdef __cplusplus
}
#endif
#endif /* SEDCRNN_H */
