/* smplsim_mlp.h — C ABI of the policy-inference kernels of libsmplsim_hip.so (the sampler's caller side).
 *
 * The reference's sampler evaluates its Gaussian policy once per env step on the CPU worker that owns the env
 * (PolicyGaussian.select_action -> MLP.forward, smpl_sim/learning/policy_gaussian.py:14-41, mlp.py:36-60, with the
 * observation normalised by RunningNorm, running_norm.py:5-42).  With thousands of envs per GPU that forward pass is
 * GEMM-shaped (4096 x 289 -> 2048 -> 1536 -> 1024 -> 1024 -> 512 -> 512 -> 69: 59 GFLOP per env step) and sits in the
 * sampling loop next to ss_step, so it runs on the matrix cores: bf16 operands, fp32 accumulation
 * (v_mfma_f32_32x32x16_bf16), bias + activation fused into the GEMM's epilogue, activations kept in bf16 between layers.
 * The PPO update's products, loss heads, optimiser step (ss_adam_step) and RunningNorm update follow below; the chain rule between them stays with the caller.
 *
 * Conventions as in smplsim_hip.h: device pointers, int status + ss_last_error(), work enqueued on the caller's stream.
 */
#ifndef SMPLSIM_MLP_H
#define SMPLSIM_MLP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SS_ACT_NONE = 0, SS_ACT_SILU = 1, SS_ACT_TANH = 2, SS_ACT_RELU = 3 };   /* mlp.py:13-21 (the ones the reference's cfgs use) */

/* y = act(x W^T + b): x [M, K] bf16 row-major (K a multiple of 32, zero padded), W [N, K] bf16 row-major (torch.nn.Linear's
 * layout), b [N] f32 or NULL, y [M, ldy] bf16 (y_is_f32 = 0) or f32; columns >= N of y are not written. */
int ss_linear_bf16(const void *x, const void *w, const float *bias, void *y, int32_t M, int32_t N, int32_t K, int32_t ldy,
                   int32_t activation, int32_t y_is_f32, void *stream);

/* The product of the PPO update's forward and backward passes (round 6; the reference's update, agents/agent_ppo.py:20-83, runs them through
 * autograd): the same K-contiguous y = x W^T on the matrix cores, K a multiple of 64, with what a training step needs of it
 *   bf16 form (y_is_f32_accumulate = 0):  v = x W^T + bias;  v *= mul (if given: [M, ldy] bf16, the stored activation derivative of the layer
 *       below: dZ = (dZ' W) * act'(z));  y [M, ldy] = act(v);  yt [N, ldyt] = y^T (every product of the backward pass contracts over what is a row
 *       here: written transposed, dW = dZ^T h and dX = dZ W are this same kernel again);  dact [M, ldy] = act'(v).  Any of y / yt / dact may be
 *       NULL (mul and dact need y).
 *   accumulating fp32 form (y_is_f32_accumulate = 1):  y [M, ldy] fp32 += x W^T (+ bias), the contraction split over several workgroups whose
 *       partial sums meet in y by hardware atomics — for products with few outputs and a deep K (the weight gradients: K = the batch).
 *       The caller zeroes y.  This form has no deterministic twin: its result depends on the order in which the workgroups' atomics arrive; the update
 *       no longer calls it (weight gradients go through ss_wgrad_bf16, which has one: ss_wgrad_bf16_det). */
int ss_linear_bf16_train(const void *x, const void *w, const float *bias, const void *mul, void *y, void *yt, void *dact, int32_t M, int32_t N,
                         int32_t K, int32_t ldy, int32_t ldyt, int32_t activation, int32_t y_is_f32_accumulate, void *stream);

/* Observation -> first layer input: y = clamp(obs, clip_lo, clip_hi) (AgentPPO's clip_obs), then, when *norm_n > 0,
 * clamp((y - mean) / (std + 1e-8), -norm_clip, norm_clip) (RunningNorm.forward in eval mode), rounded to bf16 into
 * out [M, kpad] with the columns >= dim zeroed.  norm_* may be NULL (no normalisation). */
int ss_obs_to_bf16(const float *obs, int32_t M, int32_t dim, int32_t obs_stride, const float *norm_mean, const float *norm_std,
                   const int64_t *norm_n, float clip_lo, float clip_hi, float norm_clip, void *out, int32_t kpad, void *stream);

/* dZ of the layer below in one launch (the `grad_input = dZ @ W` of torch.nn.Linear's backward followed by the activation's backward, agents/agent_ppo.py:20-83):
 *   y = (x W^T) * mul   [M, ldy] bf16        x = dZ [M, K], w = W^T [N, K] (both K-contiguous), mul = act'(z_below) [M, ldy] bf16
 *   colsum[j] += sum_m of the fp32 result    [N] fp32: the bias gradient of the layer below (the caller zeroes it; partial sums by fp32 atomics)
 * Served by the 256 x 256 kernel only: M >= 2048, N >= 256, K a multiple of 128 (SS_ERR_INVALID otherwise: use ss_linear_bf16_train and sum the columns yourself). */
int ss_linear_bf16_dx(const void *x, const void *w, const void *mul, void *y, float *colsum, int32_t M, int32_t N, int32_t K, int32_t ldy, void *stream);

/* ss_linear_bf16_dx with reproducible column sums: same contract and shape limits (colsum += ; y is bit-identical to ss_linear_bf16_dx's), and the result is a
 * function of the arguments and the input bytes alone — not of the order in which workgroups run, nor of what the workspace held before.
 *   workspace  caller-owned, 16-byte aligned, at least ss_linear_bf16_dx_det_workspace(M, N, K) = 2 * ceil(M / 256) * N * 4 bytes.  After the call it holds
 *              P = 2 * ceil(M / 256) rows of N floats, dense: row p, column j is the fp32 sum of the result's column j over the rows [128 p, min(128 p + 128, M))
 *              (zero for a p whose rows all lie beyond M), formed inside one wavefront in an order fixed by the kernel.
 *   order      colsum[j] += (((P_0[j] + P_1[j]) + P_2[j]) + ... + P_{P-1}[j]): the sum over the partial rows first, ascending, in fp32, starting from
 *              row 0; then one addition to colsum[j].  Two launches on `stream` (the product, the reduce); the workspace may be reused by the next call on
 *              the same stream.
 * SS_ERR_INVALID (nothing launched) for a null, misaligned or too-small workspace.  The query returns a negative value for shapes ss_linear_bf16_dx rejects. */
int ss_linear_bf16_dx_det(const void *x, const void *w, const void *mul, void *y, float *colsum, int32_t M, int32_t N, int32_t K, int32_t ldy, void *workspace,
                          int64_t workspace_bytes, void *stream);
int64_t ss_linear_bf16_dx_det_workspace(int32_t M, int32_t N, int32_t K);

/* Weight gradient of a linear layer from the two tensors as autograd holds them (replaces `grad_W = dZ^T @ h` of torch.nn.Linear's backward inside the
 * reference's update_policy / update_value, agents/agent_ppo.py:20-83):
 *   dw[i, j] += sum_m dz[m, i] * h[m, j]      dz [Mb, ldz] bf16 (columns 0 .. n_out - 1 used), h [Mb, ldh] bf16 (columns 0 .. n_in - 1), dw [n_out, ldw] fp32
 * Both operands are read untransposed (contraction over their ROWS); the caller zeroes dw; partial sums of a K split meet by fp32 atomics.
 * Mb a multiple of 128 (pad rows zero), n_out, n_in, ldz, ldh multiples of 8, dz and h 16-byte aligned, ldw >= n_in. */
int ss_wgrad_bf16(const void *dz, const void *h, float *dw, int32_t Mb, int32_t n_out, int32_t n_in, int32_t ldz, int32_t ldh, int32_t ldw, void *stream);

/* ss_wgrad_bf16 with a reproducible result: same contract (dw += , the same alignment and size rules), and dw is a function of the arguments and the input
 * bytes alone.  The batch is cut into the same S shares of `kper` K tiles (64 rows each) as ss_wgrad_bf16 cuts it (S = ksplit of ss_debug_last_gemm:
 * min(256 / output tiles of 256 x 256, Mb / 512) shares, at least 1, rounded so that every share holds an even number of K tiles; no share is empty).
 *   workspace  caller-owned, 16-byte aligned, at least ss_wgrad_bf16_det_workspace(Mb, n_out, n_in) = S * n_out * n_in * 4 bytes.  After the call partial s lies
 *              dense at workspace + s * n_out * n_in floats, row-major [n_out, n_in]: the product over the rows [s * kper * 64, min((s + 1) * kper * 64, Mb))
 *              of dz and h, written by plain stores (no atomics; dw is not read by the product).
 *   order      dw[i, j] += (((p_0[i, j] + p_1[i, j]) + p_2[i, j]) + ... + p_{S-1}[i, j]): the sum over the shares first, ascending, in fp32, starting from
 *              p_0; then one addition to dw[i, j].  The padding of dw (columns n_in .. ldw - 1) is not touched.  Two launches on `stream`; the workspace may be
 *              reused by the next call on the same stream.
 * SS_ERR_INVALID (nothing launched) for a null, misaligned or too-small workspace.  The query returns a negative value for invalid arguments. */
int ss_wgrad_bf16_det(const void *dz, const void *h, float *dw, int32_t Mb, int32_t n_out, int32_t n_in, int32_t ldz, int32_t ldh, int32_t ldw, void *workspace,
                      int64_t workspace_bytes, void *stream);
int64_t ss_wgrad_bf16_det_workspace(int32_t Mb, int32_t n_out, int32_t n_in);

/* The Gaussian head of the sampler in one launch (PolicyGaussian.select_action, policy_gaussian.py:25-41 -> DiagGaussian.sample;
 * Agent.preprocess_actions with clip_actions, agents/agent.py:153-161; normal_log_density of get_log_prob): per row
 *   action = mean + exp(log_std) * noise          [M, dim], row stride lda (the rollout's action row: the UNCLIPPED draw is what is stored)
 *   action_env = clamp(action, clip_lo, clip_hi)  [M, dim], row stride lde, or NULL (what the env is stepped with)
 *   logp = sum_j -noise^2 / 2 - log sqrt(2 pi) - log_std_j   [M] or NULL (the behaviour policy's log-density of the draw)
 * mean, noise [M, dim] dense f32; log_std [dim].  The caller draws the noise (its generator, its stream order). */
int ss_gaussian_sample(const float *mean, const float *noise, const float *log_std, int32_t M, int32_t dim, float *action, int32_t lda,
                       float *action_env, int32_t lde, float clip_lo, float clip_hi, float *logp, void *stream);

/* The PPO update's loss heads (the step between the networks' forward passes and their backward products; they replace ~15 elementwise and reduction launches
 * forward and as many through autograd in the reference's update_policy / update_value, agents/agent_ppo.py:20-83).  For a caller without autograd they give the
 * head's dZ that ss_wgrad_bf16 / ss_linear_bf16_dx start from.
 *
 * Both heads are reproducible and have no second variant: every output is a function of the arguments and the input bytes alone — not of the order in which
 * workgroups run, nor of what the workspace held before.  No atomics.  Every per-element and per-row value is formed in fp64 from the fp32 inputs and rounded to
 * fp32 once, when it is stored; every sum is an fp64 sum in the order stated below, rounded to fp32 once at the end.  Two launches each on `stream` (the head, the
 * reduce); the workspace is caller-owned, 16-byte aligned, and may be reused by the next call on the same stream.  SS_ERR_INVALID, nothing launched: a null required
 * pointer, M < 1, a row stride below the row's width, a null, misaligned or too-small workspace, a bf16 gradient whose ldd is not a multiple of 8 or whose base is
 * not 16-byte aligned (what ss_wgrad_bf16 asks of its operands).  The workspace queries return a negative value (and set ss_last_error) for invalid shapes.
 *
 * ss_ppo_policy_head: the clipped surrogate of AgentPPO.ppo_loss over PolicyGaussian.get_log_prob.  mean [M, ldm], actions [M, lda] f32; log_std [dim], adv [M],
 * old_logp [M] f32; 1 <= dim <= 256 (a wavefront keeps a row's columns in registers, four trips of 64), clip_eps in (0, 1).  Per row i, with lo = 1 - clip_eps and
 * hi = 1 + clip_eps, both formed in fp64 from the float argument (for clip_eps = 0.2f: 0.799999997 and 1.200000003, where an fp32 evaluation clamps at
 * float(0.8) = 0.80000001 and float(1.2); clip_frac's "r_i outside [lo, hi]" is |r_i - 1| > clip_eps with that clip_eps):
 *   z_ij   = (a_ij - mean_ij) * exp(-log_std_j)
 *   logp_i = sum_j (-z_ij^2 / 2 - log_std_j - log sqrt(2 pi))
 *   r_i    = exp(logp_i - old_logp_i);  s1 = r_i A_i;  s2 = clamp(r_i, lo, hi) A_i   (a NaN stays a NaN through the clamp and the minimum, as in torch)
 *   g_i    = -(1 / M) r_i (s1 <= s2 ? A_i : 0)                     (dloss / dlogp_i: what autograd gives for -minimum(s1, s2).mean(), ties and a ratio on a bound included)
 * outputs
 *   logp     [M] f32 or NULL
 *   dmean    [M, ldd] f32 (dmean_is_bf16 = 0) or bf16 (the round-to-nearest-even of the f32 value):  g_i z_ij exp(-log_std_j).  Rows >= M and columns >= dim are not written.
 *   dlog_std [dim] f32 or NULL, overwritten:  sum_i g_i (z_ij^2 - 1)
 *   stats    [4] f32, overwritten:  loss = -(1 / M) sum_i min(s1, s2);  clip_frac = (1 / M) #{i: r_i < lo or r_i > hi};  approx_kl = (1 / M) sum_i (old_logp_i - logp_i);
 *            mean_ratio = (1 / M) sum_i r_i
 * A NaN in one row's mean gives a NaN loss and NaN in that row of dmean (and in dlog_std); the other rows of dmean are not affected.
 *   workspace  at least ss_ppo_policy_head_workspace(M, dim) = ceil(M / 128) * (4 + dim) * 8 bytes.  After the call it holds P = ceil(M / 128) rows of 4 + dim doubles, dense:
 *              row p is the sum over the rows [128 p, min(128 p + 128, M)) of  min(s1, s2) | (r_i outside [lo, hi]) | old_logp_i - logp_i | r_i | g_i (z_ij^2 - 1), j = 0 .. dim - 1.
 *   order      a row's logp: lane l of the row's wavefront adds its columns l, l + 64, ... ascending, then the 64 lanes meet by the xor butterfly (distances 32, 16, 8, 4, 2, 1).
 *              A partial row: wavefront w of workgroup p adds its rows 128 p + 32 w .. 128 p + 32 w + 31 ascending, then ((w_0 + w_1) + w_2) + w_3.
 *              The reduce: (((P_0 + P_1) + P_2) + ... + P_{P-1}) per column, ascending from row 0; the first four columns divided by M (the first negated) are stats. */
int ss_ppo_policy_head(const float *mean, int32_t ldm, const float *actions, int32_t lda, const float *log_std, const float *adv, const float *old_logp, int32_t M,
                       int32_t dim, float clip_eps, float *logp, void *dmean, int32_t ldd, int32_t dmean_is_bf16, float *dlog_std, float *stats, void *workspace,
                       int64_t workspace_bytes, void *stream);
int64_t ss_ppo_policy_head_workspace(int32_t M, int32_t dim);

/* ss_value_head: the critic's loss of AgentPPO.update_value.  pred, target [M] f32 (dense).
 *   dpred [M, ldd] f32 or bf16 (dpred_is_bf16; one column, ldd >= 1):  2 (pred_i - target_i) / M          loss [1] f32, overwritten:  (1 / M) sum_i (pred_i - target_i)^2
 * A NaN in pred gives a NaN loss and a NaN in that row of dpred only.
 *   workspace  at least ss_value_head_workspace(M) = ceil(M / 1024) * 8 bytes: P = ceil(M / 1024) doubles, partial p the sum of the squares over the rows [1024 p, min(1024 p + 1024, M)).
 *   order      thread t of workgroup p adds its rows 1024 p + t + 256 k, k = 0 .. 3 ascending; a wavefront's 64 lanes meet by the xor butterfly (32 .. 1); the
 *              four wavefronts ((w_0 + w_1) + w_2) + w_3; the reduce adds the partials ascending from p = 0, then divides by M. */
int ss_value_head(const float *pred, const float *target, int32_t M, void *dpred, int32_t ldd, int32_t dpred_is_bf16, float *loss, void *workspace,
                  int64_t workspace_bytes, void *stream);
int64_t ss_value_head_workspace(int32_t M);

/* ss_adam_step: the optimiser step of the update for all tensors of a network in one call — the global gradient norm, clip_grad_norm_'s coefficient, Adam, and the
 * bf16 images of the new weights that the next network pass reads (W for the forward products, W^T for ss_linear_bf16_dx).  It is torch.optim.Adam with
 * amsgrad = False, maximize = False (the reference's optimiser, agents/agent_ppo.py:85-88) preceded by torch.nn.utils.clip_grad_norm_(..., error_if_nonfinite = False)
 * (policy_grad_clip, agent_humanoid.py:110-111).  Reproducible like the loss heads: no atomics, every output a function of the arguments and the input bytes alone;
 * every value is formed in fp64 from the fp32 inputs and rounded to fp32 once, when it is stored:
 *   S      = sum over all tensors and elements of g^2            (fixed order, below)
 *   norm   = sqrt(S);  c = min(1, max_grad_norm / (norm + 1e-6))   (clip_grad_norm_'s coefficient; 1 when clipping is off)
 *   g'     = c g + weight_decay p
 *   m'     = beta1 m + (1 - beta1) g'
 *   v'     = beta2 v + (1 - beta2) g'^2
 *   p'     = p - (lr / (1 - beta1^step)) m' / (sqrt(v') / sqrt(1 - beta2^step) + eps)
 * A NaN or Inf anywhere in the gradients gives a non-finite norm, and through c it reaches every parameter of the call (as in torch; with clipping off only the
 * elements it touches).
 *   tensors   a HOST array of `count` descriptors, 1 <= count <= 32 (SS_ERR_INVALID beyond); it is copied into the kernel arguments and may be freed on return.
 *             p, m, v   fp32 [rows, cols] dense: parameter, exp_avg, exp_avg_sq; overwritten with p', m', v'.
 *             g         fp32 [rows, cols], row stride ldg >= cols, unit column stride; not modified.
 *             w_bf16    [rows, ld_w] bf16 or NULL: the round-to-nearest-even bf16 of the STORED fp32 p' (a NaN as 0x7FC0).  ld_w >= cols, a multiple of 8, the base
 *                       16-byte aligned; columns >= cols are not written (the owner zeroes them once).
 *             wt_bf16   [cols, ld_wt] bf16 or NULL: the same values transposed.  ld_wt >= rows, a multiple of 8, the base 16-byte aligned; elements outside
 *                       [cols, rows] are not written.
 *   step      >= 1, the number of this step (kept on the host, as torch.optim.Adam does by default); betas in [0, 1), eps >= 0.
 *   max_grad_norm   <= 0 or +inf: no clipping (the norm is still formed and reported).     grad_norm  [1] f32 on the device or NULL: float(norm).
 *   workspace caller-owned, 16-byte aligned, at least ss_adam_step_workspace(tensors, count) = (T + 1) * 8 bytes, T the number of tiles of the call: every tensor is cut
 *             into tiles of 64 rows x 64 columns, numbered in descriptor order and row-major within a tensor.  After the call workspace[tile] is the tile's fp64 sum of
 *             squares and workspace[T] is S.
 *   order     a tile: thread t of its 256-thread workgroup owns the rows (t >> 4) + 16 k, k = 0 .. 3, and in each the columns 4 (t & 15) .. 4 (t & 15) + 3; it adds its
 *             squares with k ascending, the columns ascending within a row; a wavefront's 64 lanes meet by the xor butterfly (32, 16, ..., 1); the four wavefronts
 *             ((w0 + w1) + w2) + w3.  S: the tiles' partials ascending from tile 0, by one wavefront.
 * Three launches on `stream` (partials, reduce, step), no host synchronisation, nothing read back.  Whole tiles of a tensor with cols a multiple of 4 (p, m, v 16-byte
 * aligned) are updated by 16-byte accesses and their part of wt_bf16 is written as 16-byte row segments through an LDS transpose; edge tiles and other tensors go
 * element by element.  SS_ERR_INVALID, nothing launched: the checks of the heads' style (null required pointers, rows / cols < 1, strides below the width, the
 * images' alignment, count, step, betas, eps, the workspace).  The query returns a negative value (and sets ss_last_error) for invalid descriptors. */
typedef struct ss_adam_tensor {
  float *p, *m, *v;
  const float *g;
  void *w_bf16, *wt_bf16;
  int32_t rows, cols, ldg, ld_w, ld_wt;
} ss_adam_tensor;
int ss_adam_step(const ss_adam_tensor *tensors, int32_t count, int32_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                 double max_grad_norm, float *grad_norm, void *workspace, int64_t workspace_bytes, void *stream);
int64_t ss_adam_step_workspace(const ss_adam_tensor *tensors, int32_t count);

/* ss_running_norm_update: RunningNorm.update of the policy's observation normalisation on the device (learning/networks.py; the reference's running_norm.py:22-29,
 * which the update runs in train mode once per optimisation iteration): the biased column statistics bm, bv of x [M, dim] (fp32, row stride ldx >= dim, any
 * 4-byte-aligned base) merged into the running statistics, in place:
 *   w = n / (n + M);   var' = w var + (1 - w) bv + w (1 - w) (bm - mean)^2;   mean' = w mean + (1 - w) bm;   std' = sqrt(var');   n' = n + M
 * mean, var, std [dim] f32 and n [1] int64, all on the device.  The normalised bf16 operand of the network is ss_obs_to_bf16 called after this with the same pointers.
 * Reproducible like the loss heads and ss_adam_step: no atomics, every output a function of the arguments and the input bytes alone — not of the order in which
 * workgroups run, nor of what the workspace held before.  Every value is formed in fp64 from the fp32 inputs and rounded to fp32 once, when it is stored; std' is the
 * fp32 rounding of the fp64 square root of the STORED fp32 var' (so a checkpoint's std stays var.sqrt() to 1 ulp).  Two launches on `stream` (partials, merge), no
 * host synchronisation, nothing read back; the workspace is caller-owned, 16-byte aligned, and may be reused by the next call on the same stream.
 * A NaN in column c makes mean'[c], var'[c] and std'[c] NaN and changes no other column; var' is never negative; a constant column gives bv = 0 and bm = the constant
 * exactly (from n = 0: var' = 0, mean' = the constant).
 *   workspace  at least ss_running_norm_workspace(M, dim) = ceil(M / SS_NORM_BLOCK_ROWS) * dim * 16 bytes.  After the call it holds, for row block b and column c, two
 *              doubles at workspace[(b * dim + c) * 2]: the mean of column c over the rows [256 b, min(256 b + 256, M)) and the sum of the squared deviations from that
 *              mean (M2), never negative.
 *   order      a block: workgroup (b, g) owns the columns 64 g .. 64 g + 63, one per lane; lane l of wavefront w adds d = x - K and d * d over the rows
 *              256 b + 64 w .. 256 b + 64 w + 63 (those below M) of column 64 g + l in ascending order, K being the block's first row in that column; the four
 *              wavefronts meet as ((w_0 + w_1) + w_2) + w_3 = S1, S2; mean = K + S1 / rows, M2 = S2 - S1 * S1 / rows (a negative result stored as 0).
 *              the merge: one workgroup, thread t owns the columns t, t + 256, ...; the blocks are folded ascending from block 0 by the pairwise formula, with
 *              n_a the rows folded so far and n_b those of the next block: f = n_b / (n_a + n_b); delta = mean_b - mean_a; mean_a += delta * f;
 *              M2_a += M2_b + delta * delta * (n_a * f).  Then bm = mean_a, bv = M2_a / M and the formulas above with w = (double)n / (double)(n + M) and 1 - w
 *              formed from that w.  Every thread reads n before a barrier; thread 0 stores n' after it.
 * SS_ERR_INVALID, nothing launched: a null required pointer, M < 1 or dim < 1, ldx < dim, a null, misaligned or too-small workspace, more than 2^24 workgroups
 * (ceil(M / 256) * ceil(dim / 64): beyond any device's memory).  The query returns a negative value (and sets ss_last_error) for M < 1 or dim < 1. */
#define SS_NORM_BLOCK_ROWS 256
int64_t ss_running_norm_workspace(int32_t M, int32_t dim);
int ss_running_norm_update(const float *x, int32_t M, int32_t dim, int32_t ldx, float *mean, float *var, float *std, int64_t *n, void *workspace,
                           int64_t workspace_bytes, void *stream);

/* ss_gather_rows: the shuffle of a mini-batch epoch of the update (the reference's agents/agent_ppo.py:26-46: states[perm].clone(), ... for seven tensors, then a
 * slice per mini-batch) — the rows perm[i] of up to 8 tensors copied into a blocked layout by ONE launch, so that every block of every tensor is a view the network
 * passes take as it is (learning/minibatch.py).
 *   result    for i in [0, rows) and every tensor: dst row (i / block_rows) * dst_block_stride + i % block_rows, columns [0, cols), equals src row perm[i], byte for
 *             byte.  No value is interpreted: NaN payloads and bf16 bit patterns survive.
 *   untouched everything else in dst: the columns >= cols, the dst_block_stride - block_rows rows between two blocks, the rows after the last block (the owner
 *             zeroes them once: the pad rows of a bf16 operand).
 *   perm      [rows] int64 on the device.  An entry outside [0, src_rows) skips row i in every tensor: its dst row keeps what it held and no other row is affected;
 *             the kernel compares the entry with the range before it forms an address from it.  Entries may repeat.
 *   tensors   a HOST array of `count` descriptors, 1 <= count <= 8; it is copied into the kernel arguments and may be freed on return.
 *             src   [src_rows, ld_src] elements of elem_bytes bytes (2 or 4), unit column stride; not modified.
 *             dst   blocked as above, row stride ld_dst elements; ld_src, ld_dst >= cols, in elements; dst_block_stride >= block_rows, in dst rows.
 *   overlap   the bytes a call reads ([src, src + ((src_rows - 1) ld_src + cols) elem_bytes) of every tensor, and perm) and the bytes it writes must not overlap —
 *             not within a tensor (refused, src == dst included) and not between two tensors of a call (not checked).
 *   access    per tensor, 16-byte loads and stores where both bases, ld_src * elem_bytes, ld_dst * elem_bytes and cols * elem_bytes are multiples of 16; else 4-byte
 *             ones where they are multiples of 4; else element by element.  The three paths give the same bytes.  A row of u such units is served by
 *             min(64, next power of two >= u) neighbouring lanes: a one-column tensor takes one thread per row, not one wavefront.
 * One launch on `stream`, no workspace, no atomics, no host synchronisation, nothing read back.  SS_ERR_INVALID, nothing launched: a null tensors, perm, src or dst;
 * count outside [1, 8]; elem_bytes not 2 or 4; cols < 1; ld_src or ld_dst < cols; dst_block_stride < block_rows; src_rows, rows or block_rows < 1; a base not
 * aligned to elem_bytes (perm: to 8 bytes); src and dst of a tensor overlapping; more than 2^31 - 1 workgroups. */
typedef struct ss_gather_tensor {
  const void *src;
  void *dst;
  int32_t elem_bytes;
  int32_t cols, ld_src, ld_dst;
  int32_t dst_block_stride;
} ss_gather_tensor;
int ss_gather_rows(const ss_gather_tensor *tensors, int32_t count, const int64_t *perm, int32_t src_rows, int32_t rows, int32_t block_rows, void *stream);

/* ss_episode_stats: the episode statistics of a rollout — what the reference's sampler collects step by step in a LoggerRL (smpl_sim/learning/logger_rl.py:
 * start_episode / step / end_episode, agents/agent.py:64-109) and its training line is made of (agent_humanoid.py:171-193).  N envs advance in lock step for T
 * steps, so an episode spans many rollouts: the return and the length of the episode every env is in the middle of are a per-env carry, read and rewritten.
 *   rewards, not_done   [T, N] f32, time-major, dense: the rollout tensors that ss_gae reads.
 *   parts               [T, N, P] f32, dense: the reward terms of every step; NULL when P == 0.  0 <= P <= SS_EPISODE_MAX_PARTS.
 *   ep_return [N] f64, ep_len [N] int32   the carry (a new env: 0, 0).
 *   stats [9 + P] f64   overwritten, in the order of the SS_EP_* indices; nothing behind element 9 + P - 1 is touched.
 * Per env column n, with t ascending from 0:  ep_return[n] += (double)rewards[t, n];  ep_len[n] += 1;  where not_done[t, n] == 0.0f (+0 or -0; any other value, a
 * NaN included, continues the episode) the episode ends: num_episodes += 1, total_episode_reward += ep_return[n], total_episode_len += ep_len[n], the episode
 * minimum and maximum take ep_return[n], and both carries go to zero.  Over all steps: num_steps = T * N, total_reward and the minimum and maximum reward, and
 * stats[9 + p] = the sum of parts[:, :, p].  With no episode ended min_episode_reward = +inf and max_episode_reward = -inf (LoggerRL's initial values).
 * Minima and maxima propagate a NaN (torch.amin / amax); a NaN reward makes the sums it enters NaN and its env's ep_return NaN until that episode ends; it changes
 * no other env's carry and no count.  ep_len wraps after 2^31 - 1 steps of one episode; counts and lengths are summed as integers held in fp64 (exact below 2^53).
 * Reproducible like the loss heads, ss_adam_step and ss_running_norm_update: no atomics, every output a function of the arguments and the input bytes alone — not
 * of the order in which workgroups run, nor of what the workspace held before.  Two launches on `stream` (scan, reduce), no host synchronisation, nothing read
 * back; the workspace is caller-owned, 16-byte aligned, and may be reused by the next call on the same stream.
 *   workspace  at least ss_episode_stats_workspace(T, N, P) = ceil(N / 64) * (9 + P) * 8 bytes.  After the call it holds G = ceil(N / 64) rows of 9 + P doubles, dense,
 *              in the layout of stats: row g is the statistics of the columns [64 g, min(64 g + 64, N)).
 *   order      an episode's return: the fp64 sum of its fp32 rewards with t ascending, continued from the carry (fixed by the definition: ep_return, ep_len, the
 *              counts and the four extremes are the same in any implementation).  The sums: workgroup g is ONE wavefront and owns the columns 64 g .. 64 g + 63, one
 *              per lane, so that every [t, :] row access is a coalesced segment; lane l adds what column 64 g + l contributes with t ascending (an episode's return
 *              and length at the step that ends it; with P == 4 and a 16-byte aligned parts a step's four terms come by one 16-byte load), a lane beyond N adds
 *              nothing; the 64 lanes meet by the xor butterfly (distances 32, 16, 8, 4, 2, 1) and lane 0 stores row g; the reduce, one wavefront with lane j on
 *              statistic j, folds (((row_0 + row_1) + row_2) + ... + row_{G-1}), ascending from row 0.  One wavefront per workgroup because the scan has only N
 *              columns to hand out: 4096 columns are 64 workgroups on 64 CUs rather than 16 of 256 lanes, without LDS or a barrier.  Not timed.
 * SS_ERR_INVALID, nothing launched: a null required pointer; parts null with P > 0; T < 1, N < 1 or P outside [0, 8]; a null, misaligned or too-small workspace.
 * The query returns a negative value (and sets ss_last_error) for invalid shapes. */
#define SS_EPISODE_MAX_PARTS 8
enum { SS_EP_NUM_STEPS, SS_EP_NUM_EPISODES, SS_EP_TOTAL_EPISODE_REWARD, SS_EP_TOTAL_EPISODE_LEN, SS_EP_MIN_EPISODE_REWARD,
       SS_EP_MAX_EPISODE_REWARD, SS_EP_TOTAL_REWARD, SS_EP_MIN_REWARD, SS_EP_MAX_REWARD, SS_EP_PARTS /* = 9: first of P part sums */ };
int64_t ss_episode_stats_workspace(int32_t T, int32_t N, int32_t P);
int ss_episode_stats(const float *rewards, const float *not_done, const float *parts, int32_t T, int32_t N, int32_t P,
                     double *ep_return, int32_t *ep_len, double *stats, void *workspace, int64_t workspace_bytes, void *stream);

/* ss_clip_outcomes: which clip every env of a motion-imitation rollout was tracking when it fell, when it finished and while it stepped, tallied into per-clip
 * counters — the input of the reference's failure-weighted sampling (smpl_sim/smpllib/motion_lib_base.py:219-267: termination_history,
 * update_soft_sampling_weight), which collects it on the host from the keys of the failed clips.
 *   clip_ids     [T, N] int32, time-major, dense: the clip env n was tracking DURING step t (the env's motion_ids before the step launch: the fused step
 *                overwrites them when it re-initialises a finished env).
 *   dead, done   [T, N] bytes, dense: the sampler's rows (torch.bool storage); any non-zero byte is set.
 *   counts       [M, 3] int64, dense, ACCUMULATED: the call adds to what it finds and never zeroes.  Columns: SS_CLIP_FAILED, SS_CLIP_COMPLETED, SS_CLIP_STEPS.
 * Per element (t, n) with c = clip_ids[t, n]:  counts[c, SS_CLIP_STEPS] += 1;  if dead[t, n] != 0, counts[c, SS_CLIP_FAILED] += 1;  otherwise, if done[t, n] != 0,
 * counts[c, SS_CLIP_COMPLETED] += 1.  A c outside [0, M) skips the element entirely: nothing is added anywhere for it, and the kernel compares c with the range
 * before it forms an address from it (as ss_gather_rows does with perm).  Nothing but the 3 M counters is written.  Sums wrap modulo 2^64.
 * Reproducible although it uses atomics: the additions are 64-bit INTEGER vector atomics (no return value), and integer addition is exact and independent of
 * order, so the counters are a function of the arguments and the input bytes alone — not of the order in which workgroups run.  No float is summed anywhere.
 *   order      irrelevant to the result; for the cost: workgroup g is ONE wavefront and owns the env columns 64 g .. 64 g + 63, one per lane (every [t, :] row
 *              access a coalesced segment); a lane walks t ascending, counts the steps of the clip it is on in a register and adds them to the clip's counter
 *              when the id changes, when dead or done is set, and at the end of the column: (episodes + id changes + N) adds instead of T * N (12 - 37 us for a
 *              25 x 2048 rollout, the more the fewer clips share the adds: profiles/clip_sampling.txt).
 * One launch on `stream`, no workspace, no host synchronisation, nothing read back.  SS_ERR_INVALID, nothing launched: a null pointer; T, N or M < 1; counts not
 * 8-byte aligned.
 *
 * ss_clip_sampling_cdf: the counters' failure column as the sampling CDF that ss_motion_resample and the fused imitation step search ("the smallest m with
 * cdf[m] > draw") — the reference's update_sampling_prob (p proportional to the termination history, uniform while nothing has failed), mixed with a uniform floor.
 *   counts       [M, 3] int64 as above, not modified; only column SS_CLIP_FAILED is read: f_m = max(counts[m, SS_CLIP_FAILED], 0) (a negative count is 0).
 *   uniform_mix  u in [0, 1]: the share of the uniform distribution.  u = 0 is the reference's rule; u > 0 keeps a clip that never failed in play (the floor is
 *                the u / M term alone: SS_CLIP_COMPLETED and SS_CLIP_STEPS play no part).
 *   cdf          [M] f32, overwritten.  Meant to be the array already bound into the fused step: the step launches behind this call on the stream draw from it.
 *   prob         [M] f64, overwritten, or NULL.
 * Every value is formed in fp64 and every operation is rounded on its own (no FMA: the kernel switches contraction off), in this order:
 *   S = sum_m f_m as an integer (int64; it must stay below 2^63), then (double)S;  keep = 1 - u,  floor = u / M,  uniform = 1 / M, each once;
 *   q_m = (double)f_m / (double)S if S > 0, else uniform;   p_m = keep * q_m + floor  (one multiplication, then one addition);
 *   c_0 = p_0,  c_m = c_{m-1} + p_m, added SEQUENTIALLY with m ascending (the order of numpy.cumsum);
 *   cdf[m] = (float)c_m for m < M - 1;  cdf[M - 1] = (float)(1 + 1e-6) = 1.00000095f, the sentinel MotionLibSMPL.load_motions writes: a draw below 1 always lands in
 *   a clip;  prob[m] = p_m.
 * With u = 0 a clip with f_m = 0 has p_m = 0 exactly, so cdf[m] == cdf[m - 1] (cdf[0] == 0) and no draw in [0, 1) selects it.  The sequential sum IS the contract:
 * one lane runs the chain (a parallel scan would change the bits); M is at most tens of thousands and the call runs once per rollout (7 us up to 256 clips, 0.93 ms at
 * 50 000: profiles/clip_sampling.txt).
 * A function of the arguments and the input bytes alone.  One launch on `stream` (one workgroup), no workspace, no host synchronisation.
 * SS_ERR_INVALID, nothing launched: a null counts or cdf; M < 1; u outside [0, 1] or NaN. */
enum { SS_CLIP_FAILED, SS_CLIP_COMPLETED, SS_CLIP_STEPS, SS_CLIP_COLUMNS /* = 3 */ };
int ss_clip_outcomes(const int32_t *clip_ids, const uint8_t *dead, const uint8_t *done, int32_t T, int32_t N, int32_t M, int64_t *counts, void *stream);
int ss_clip_sampling_cdf(const int64_t *counts, int32_t M, double uniform_mix, float *cdf, double *prob, void *stream);

/* Test hook: the GEMM instantiation launched last by an ss_linear_* / ss_wgrad_bf16* call on the calling host thread, as
 * "<family> mode=<G256 mode or -> bn=<BN> bk=<BK> waves=<waves per workgroup> out=<bf16|f32|f32acc|f32det> ksplit=<K shares> kper=<K tiles per share>"
 * with family linear / glds / train / gemm256 / wgrad (empty before the first launch).  The deterministic entries report their GEMM, not their reduce pass:
 * ss_wgrad_bf16_det with out=f32det, ss_linear_bf16_dx_det the line of ss_linear_bf16_dx with " colsum=det" appended.  Copies it, NUL-terminated and truncated to len - 1
 * characters, into buf; returns its full length. */
int ss_debug_last_gemm(char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif
