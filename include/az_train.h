/* az_train.h - the learner's device side: the training losses of a batch and their gradients
 * (alphazero-al_amd/csrc/train_kernels.hip), below them the clipping of the gradient norm with the AdamW step
 * (az_opt_*, alphazero-al_amd/csrc/optim_kernels.hip), the Connect4 residual block's training forward and
 * backward (az_train_*block*, alphazero-al_amd/csrc/train_block_kernels.hip), the Connect4 gated attention
 * block's (az_train_*attn*, alphazero-al_amd/csrc/train_attn_kernels.hip), the Connect4 stem's
 * (az_train_*stem*, alphazero-al_amd/csrc/train_stem_kernels.hip), the Connect4 heads'
 * (az_train_*heads*, alphazero-al_amd/csrc/train_heads_kernels.hip); and, declared between the optimiser and the blocks, the
 * native learner, which drives all of them for a whole batch or epoch (az_learn_*, alphazero-al_amd/csrc/learn_driver.hip).
 *
 * The reference's training step turns a batch and the network's three head outputs into up to five loss terms
 * (src/environments/NetworkBase.py:30-192: `_prepare_training_batch`, `_policy_loss`, `_value_loss`,
 * `_distill_value_loss`, `_td_consistency_loss`, `_aux_loss`), lets autograd run their mirror image, and reads the
 * confusion of the value head back for sklearn's f1_score.  Here that is two launches for the losses and the
 * counts and one for the gradients, on a batch exactly as az_replay_dev_batch (az_mcts.h) writes it.  Part of
 * libaz_mcts.so; error codes and az_last_error() as in az_mcts.h.
 *
 * Per sample n of N (A = 7 Connect4, 65 Othello; sign = +1 if state[n][2][0][0] >= 0, else -1):
 *   mask      sum_a prob[n][a] > 0
 *   class     0 if winner == 0, 1 if winner == sign, 2 otherwise
 *   policy    kl = sum_a prob_a (log prob_a - log_p_a), entries with prob_a == 0 contribute 0;
 *             mask * kl * (1 + psw_beta * kl)   [the weight carries no gradient]   - entropy_lambda * mask * H,
 *             H = -sum_a exp(log_p_a) log_p_a
 *   value     -sum_i z_i value_i, z = onehot(class), or d * onehot + (1 - d) / 3 with d = value_decay ^ steps_to_end
 *             when value_decay < 1
 *   distill   (distill_alpha > 0) rel = root_wdl with p1 and p2 swapped when sign == -1;
 *             [sum rel > 0] * KL(softmax(log(max(rel, 1e-8)) / T) || softmax(value / T))
 *   td        (td_alpha > 0) rows with steps_to_end > td_steps and sum of the relative future_root_wdl > 0:
 *             t = rel / max(sum rel, 1e-8), t = d t + (1 - d) / 3 with d = value_decay ^ td_steps when
 *             value_decay < 1; sum_i t_i (log t_i - value_i), zero targets contribute 0
 *   aux       smooth-L1 (beta 1) of steps[n] - aux_target[n] / aux_target_offset
 * Over the batch: policy, value, distill, aux are means over N, td is the mean over its own rows;
 *   value <- (1 - distill_alpha) value + distill_alpha T^2 distill       if distill_alpha > 0
 *   value <- (1 - td_alpha) value + td_alpha td                          if td_alpha > 0 and a td row exists
 * No floating-point atomics: every batch sum is per-wavefront partials in the workspace, added in a fixed order,
 * so two calls on the same inputs give the same bytes. */
#ifndef AZ_TRAIN_H
#define AZ_TRAIN_H

#include "az_mcts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The knobs of the reference's `train_step`, with its defaults in brackets. */
typedef struct az_train_loss_config {
    double  value_decay;        /* (0, 1]   [1] */
    double  distill_alpha;      /* [0, 1]   [0] */
    double  distill_temp;       /* > 0      [1] */
    double  psw_beta;           /* >= 0     [0] */
    double  entropy_lambda;     /* >= 0     [0] */
    double  td_alpha;           /* [0, 1]   [0] */
    int32_t td_steps;           /* >= 0     [5] */
    int32_t reserved;           /* 0 */
    double  aux_target_offset;  /* > 0; 42 (Connect4), 64 (Othello) */
} az_train_loss_config;
#define AZ_TRAIN_LOSS_CONFIG_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(az_train_loss_config) == AZ_TRAIN_LOSS_CONFIG_BYTES, "az_train_loss_config layout");
#else
_Static_assert(sizeof(az_train_loss_config) == AZ_TRAIN_LOSS_CONFIG_BYTES, "az_train_loss_config layout");
#endif

/* The three head outputs, float32 in DEVICE memory, contiguous. */
typedef struct az_train_heads {
    const float *log_p;         /* [N][A] log-probabilities, finite (illegal moves masked at -1e9 before the log-softmax) */
    const float *value;         /* [N][3] log-probabilities, relative order draw, win, loss */
    const float *steps;         /* [N] */
} az_train_heads;
#define AZ_TRAIN_HEADS_BYTES 24

/* What the loss pass leaves in DEVICE memory. */
typedef struct az_train_loss_out {
    float   *losses;            /* [4] policy, value (after the distill and td mixing), aux, policy entropy over all rows */
    int32_t *counts;            /* [11] confusion[3][3] (row = value class, column = argmax of value), policy rows, td rows */
    void    *workspace;         /* az_train_loss_workspace_bytes(game, N) bytes; its contents need not be kept */
} az_train_loss_out;
#define AZ_TRAIN_LOSS_OUT_BYTES 24

/* The gradients with respect to the three head outputs, float32 in DEVICE memory. */
typedef struct az_train_grads {
    float *d_log_p;             /* [N][A] */
    float *d_value;             /* [N][3] */
    float *d_steps;             /* [N] */
} az_train_grads;
#define AZ_TRAIN_GRADS_BYTES 24
#ifdef __cplusplus
static_assert(sizeof(az_train_heads) == AZ_TRAIN_HEADS_BYTES && sizeof(az_train_loss_out) == AZ_TRAIN_LOSS_OUT_BYTES &&
              sizeof(az_train_grads) == AZ_TRAIN_GRADS_BYTES, "az_train pointer structs");
#else
_Static_assert(sizeof(az_train_heads) == AZ_TRAIN_HEADS_BYTES && sizeof(az_train_loss_out) == AZ_TRAIN_LOSS_OUT_BYTES &&
               sizeof(az_train_grads) == AZ_TRAIN_GRADS_BYTES, "az_train pointer structs");
#endif

/* Bytes of workspace a loss pass over N rows needs; -1 for an unknown game, N <= 0 or N beyond 2^30. */
int64_t az_train_loss_workspace_bytes(int game, int64_t N);
/* The loss pass: two launches on `stream` (per-wavefront partials, then their reduction in a fixed order), nothing
 * waits for the device.  `batch` names N = S * B rows as az_replay_dev_batch writes them (valid_mask is not read).
 * AZ_ERR_ARG, with nothing enqueued and nothing written: an unknown game; N <= 0 or beyond 2^30; a null struct or
 * pointer; a pointer that is not 16-byte aligned (steps, losses, counts: 4-byte); value_decay outside (0, 1];
 * distill_alpha or td_alpha outside [0, 1]; distill_temp <= 0; a negative psw_beta, entropy_lambda or td_steps;
 * aux_target_offset <= 0. */
int az_train_dev_loss(int game, const az_replay_batch *batch, const az_train_heads *heads, int64_t N,
                      const az_train_loss_config *config, const az_train_loss_out *out, void *stream);
/* The gradient pass: one launch on `stream`.  grads = upstream[0] d(policy) + upstream[1] d(value) + upstream[2] d(aux)
 * with respect to log_p, value and steps; `upstream` is three float32 in DEVICE memory (what autograd hands
 * `backward`).  `out` is what az_train_dev_loss filled for the same batch, heads and config: the td term's scale and
 * the (1 - td_alpha) factor are read from out->counts on the device (out->workspace is not used and may be null).
 * AZ_ERR_ARG as above, plus a null or misaligned upstream (4-byte) or gradient (d_steps: 4-byte). */
int az_train_dev_loss_grad(int game, const az_replay_batch *batch, const az_train_heads *heads, int64_t N,
                           const az_train_loss_config *config, const az_train_loss_out *out, const float *upstream,
                           const az_train_grads *grads, void *stream);

/* ---- Gradient-norm clipping and the AdamW step over every tensor of an optimiser: three launches
 * (`torch.nn.utils.clip_grad_norm_` followed by `torch.optim.AdamW.step`, as the reference's `_optimize_batch` calls them).
 *
 *   total_norm = sqrt(sum over every tensor with a gradient of grad^2);  coef = min(1, max_norm / (total_norm + 1e-6))
 * and per element, in float32, in this order (t: the tensor's own step number; lr, beta1, beta2, eps, wd: its group's):
 *   g  = grad * coef                                   (only when clipping: max_norm > 0)
 *   p  = p * decay                                     decay = 1 - lr * wd
 *   m  = m + (g - m) * (1 - beta1)
 *   v  = v * beta2 + ((1 - beta2) * g) * g
 *   p  = p - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))
 *                                                      step_size = lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t)
 * decay, 1 - beta1, 1 - beta2, step_size and inv_sqrt_bc2 are formed in double on the host and rounded once; division and
 * square root are IEEE.  Non-finite values follow from the formulas (torch's error_if_nonfinite=False).
 * The GRADIENTS ARE READ AND NEVER WRITTEN: after a step `.grad` still holds the unclipped gradient, where
 * clip_grad_norm_ leaves the clipped one - the reference reads no gradient after the step.  A tensor whose gradient is
 * null is skipped whole: no decay, no change of its moments, no part in the norm.
 * The sum of squares is one partial per chunk of a tensor, added in a fixed order; no atomics: two calls on the same
 * inputs give the same bytes.  A handle's steps belong on one stream at a time (its workspace holds the partials and
 * coef between the launches). */
#define AZ_OPT_MAX_GROUPS 16
#define AZ_OPT_GROUP_HP 5                 /* lr, beta1, beta2, eps, weight_decay - doubles, per group */
typedef struct az_opt az_opt;             /* opaque */

/* A handle for n_tensors contiguous float32 tensors of numel[i] elements, tensor i in parameter group group[i]; the
 * table that maps a workgroup to a tensor and a chunk of it is built here.  `numel` and `group` are HOST arrays.  Touches
 * no device.  AZ_ERR_ARG: a null array or `out`; n_tensors <= 0; a numel <= 0; a group index outside [0, n_groups);
 * n_groups outside [1, AZ_OPT_MAX_GROUPS]. */
int  az_opt_create(int64_t n_tensors, const int64_t *numel, const int32_t *group, int32_t n_groups, az_opt **out);
void az_opt_destroy(az_opt *o);
/* The DEVICE addresses of every tensor's parameter and two moments (HOST arrays of n_tensors addresses each; 4-byte
 * aligned, 16 bytes are not needed), copied to the current device.  To be called before the first step and again
 * whenever one of the addresses has changed; may wait for the device.  AZ_ERR_ARG, with nothing changed: a null handle
 * or array, a null or misaligned address. */
int  az_opt_bind(az_opt *o, void *const *param, void *const *exp_avg, void *const *exp_avg_sq);
/* One step on `stream`: k_opt_sqsum, k_opt_norm, k_opt_clip_adamw (the first and the third once per 96 tensors); nothing
 * waits for the device, nothing is allocated or copied: the gradients' addresses travel as kernel arguments.
 * grad[i]: DEVICE address of tensor i's gradient (4-byte aligned) or null; step[i]: the step tensor i takes now, >= 1, or
 * 0 with a null grad[i]; group_hp[g * AZ_OPT_GROUP_HP ...]: lr, beta1, beta2, eps, weight_decay of group g (all HOST
 * arrays).  max_norm > 0: total_norm is written to `grad_norm` (one float32 in DEVICE memory); max_norm <= 0: no
 * clipping, the first two launches are skipped and grad_norm may be null.
 * AZ_ERR_ARG, with nothing enqueued: a null handle or array; a step before az_opt_bind; lr < 0, a beta outside [0, 1),
 * eps < 0 or weight_decay < 0; step[i] < 0; step[i] > 0 with a null grad[i], or step[i] == 0 with one; a misaligned
 * gradient; max_norm > 0 with a null or misaligned grad_norm; a max_norm that is not a number. */
int  az_opt_dev_step(az_opt *o, const void *const *grad, const int64_t *step, const double *group_hp,
                     float max_norm, float *grad_norm, void *stream);

/* ---- The native learner: a Connect4 training batch, or a whole epoch of them, as ONE call (alphazero-al_amd/csrc/learn_driver.hip).
 * What the Python route does through four autograd nodes, the loss node and ClipAdamW - stem, residual blocks, attention
 * block, heads, losses, their gradients, the backward chain, clipping and the AdamW step - az_learn_dev_step enqueues from
 * C in the same order, with the same arguments, on the same bytes: a network trained through either route holds the same
 * parameters and moments.  (Declared ahead of the units it drives: tests/test_train_heads_cpu.py holds the heads' three
 * functions to the end of this header.)  The handle owns every buffer a batch needs besides the network's own tensors; after
 * az_learn_create nothing is allocated.  Connect4 only.
 *
 * DROPOUT.  With a rate above 0 every dropout input of a batch is written by one launch, k_learn_keep, under this
 * contract (tests/learner_ref.py restates it in numpy):
 *   thr      = (uint32) floor(p * 2^32 + 0.5), formed in double on the host; a value of 2^32 counts as 2^32 - 1
 *   kept     iff the element's 32-bit draw is >= thr
 *   factor   1.0f / (1.0f - (float) p) for a kept element (rounded once, on the host; the attention block's keep_scale is
 *            the same expression), 0 for a dropped one
 *   draws    element or bit j of group a of tensor t is draw number j of the device generator's stream
 *            (seed, call, a, LEARN_STREAM + t) (csrc/dev_rng.h): with s0 the stream's state,
 *            mix64(s0 + (j + 1) * 0x9E3779B97F4A7C15) >> 32
 *   t, a     block k's factors [N][64]: t = k, a = n;   the attention block's bits [N][4][42]: t = AZ_LEARN_KEEP_ATTN,
 *            a = (4 n + h) * 42 + i, bit j of that word, bits 42 .. 63 zero;   the policy head's factors [N][7][64]:
 *            t = AZ_LEARN_KEEP_POLICY, a = 7 n + c;   the value head's pool factors [N][64]: t = AZ_LEARN_KEEP_POOL, a = n
 * A tensor whose rate is 0 is never written and its piece gets a null keep.
 *
 * The roles name the network's tensors to az_learn_bind.  (Defines, not an enum: apart from structs and assertions this
 * header holds prototypes only.) */
#define AZ_LEARN_MAX_BLOCKS 8
#define AZ_LEARN_ROLE_PIECE_EMB 0           /* [2][32] */
#define AZ_LEARN_ROLE_POS_EMB 1             /* [24][32] */
#define AZ_LEARN_ROLE_STEM_CONV_WEIGHT 2    /* [64][32][3][3] */
#define AZ_LEARN_ROLE_STEM_CONV_BIAS 3      /* [64] */
#define AZ_LEARN_ROLE_BLOCK 4               /* + 4 k + (0 norm_weight, 1 norm_bias, 2 conv_weight, 3 conv_bias), k < n_blocks */
#define AZ_LEARN_ROLE_ATTN 36               /* + the index of the field in az_train_attn_params (6) */
#define AZ_LEARN_ROLE_HEADS 42              /* + the index of the field in az_train_heads_params (18) */
#define AZ_LEARN_ROLES 60
#define AZ_LEARN_KEEP_ATTN 8                /* tensor ids of the dropout streams; block k is k */
#define AZ_LEARN_KEEP_POLICY 9
#define AZ_LEARN_KEEP_POOL 10
typedef struct az_learn az_learn;           /* opaque */

typedef struct az_learn_config {
    int64_t  max_rows;          /* the largest S * B of a batch, 1 .. 2^20 */
    int32_t  n_blocks;          /* residual blocks, 1 .. AZ_LEARN_MAX_BLOCKS */
    int32_t  max_workgroups;    /* the cap of every backward; 0: each unit's default */
    float    eps_block;         /* the blocks' GroupNorm */
    float    eps_attn;          /* the attention block's three norms */
    float    eps_heads;         /* the heads' four norms */
    float    max_norm;          /* gradient-norm clipping as az_opt_dev_step takes it */
    double   p_block;           /* the four dropout rates, each in [0, 1) */
    double   p_attn;
    double   p_policy;
    double   p_pool;
    uint64_t seed;              /* of the dropout draws */
} az_learn_config;
#define AZ_LEARN_CONFIG_BYTES 72

/* DEVICE addresses inside the handle, valid until az_learn_destroy. */
typedef struct az_learn_out {
    float    *sums;             /* [3] running sums of the policy, value and aux loss over the batches since the last reset */
    int32_t  *batches;          /* [1] how many */
    float    *entropy;          /* [1] the policy entropy of the last training batch (az_learn_dev_eval leaves it alone) */
    float    *losses;           /* [4] the last loss pass, as az_train_loss_out */
    int32_t  *counts;           /* [11] the last loss pass, as az_train_loss_out */
    float    *grad_norm;        /* [1] the last training batch's total gradient norm (max_norm > 0) */
    float    *keep_blocks;      /* block k's factors [N][64] start at keep_blocks + k * keep_block_stride */
    int64_t   keep_block_stride;    /* in floats: 64 * max_rows */
    uint64_t *keep_attn;        /* [N][4][42] */
    float    *keep_policy;      /* [N][7][64] */
    float    *keep_pool;        /* [N][64] */
    az_replay_batch batch;      /* the handle's own batch tensors, max_rows rows each: what az_learn_dev_epoch's last batch left */
} az_learn_out;
#define AZ_LEARN_OUT_BYTES 152
#ifdef __cplusplus
static_assert(sizeof(az_learn_config) == AZ_LEARN_CONFIG_BYTES && sizeof(az_learn_out) == AZ_LEARN_OUT_BYTES, "az_learn structs");
#else
_Static_assert(sizeof(az_learn_config) == AZ_LEARN_CONFIG_BYTES && sizeof(az_learn_out) == AZ_LEARN_OUT_BYTES, "az_learn structs");
#endif

/* Allocates, on the current device and once, everything a batch of up to max_rows rows needs: the activations (the stem's
 * output, every block's y, z and stats, the tokens, the three head outputs), the gradients of the chain, the keep
 * tensors, ONE workspace that serves the loss pass and the four backwards in turn, the stem's table apart from it, the
 * loss outputs, the upstream (1, 1, 1), the running sums, and batch tensors of its own for az_learn_dev_epoch.  Waits for
 * the device.  AZ_ERR_ARG, with *out null: a null argument; max_rows outside [1, 2^20]; n_blocks outside
 * [1, AZ_LEARN_MAX_BLOCKS]; an eps that is not positive and finite; a rate outside [0, 1), or so close to 1 that its float32 value is 1 (its
 * factor would not be finite); a negative max_workgroups; a
 * max_norm that is not a number. */
int  az_learn_create(const az_learn_config *config, az_learn **out);
void az_learn_destroy(az_learn *l);
/* The network's tensors in the OPTIMISER'S flat order (k_opt_sqsum adds the per-tensor partials in tensor order: only
 * that order gives the norm ClipAdamW gives).  role[i]: which tensor of the network tensor i is, every role of the
 * n_blocks-block network exactly once (n_tensors = 28 + 4 n_blocks); group[i]: its parameter group, as az_opt_create
 * takes it.  param, grad, exp_avg, exp_avg_sq: HOST arrays of DEVICE addresses; every backward writes its gradient
 * straight into grad[i].  Alignment as the five units ask: 16 bytes for param and grad of the blocks' conv_weight, the
 * attention block's qkv_weight and o_weight and the heads' three 64 x 64 weights, 4 bytes for everything else.  The handle
 * builds an az_opt of its own over them.  May wait for the device.  AZ_ERR_ARG, with nothing changed: a null argument; a
 * count that is not 28 + 4 n_blocks; a role out of range, missing or repeated; a null or misaligned address; what
 * az_opt_create refuses. */
int  az_learn_bind(az_learn *l, int64_t n_tensors, const int32_t *role, const int32_t *group, int32_t n_groups,
                   void *const *param, void *const *grad, void *const *exp_avg, void *const *exp_avg_sq);
/* One training batch of N rows on `stream`; only enqueues, nothing waits.  In order: k_learn_keep (when a rate is above
 * 0), az_train_dev_stem_fwd, az_train_dev_block_fwd per block (z and stats saved), az_train_dev_attn_fwd (x_token_major
 * 0), az_train_dev_heads_fwd (legal = batch->valid_mask), az_train_dev_loss, az_train_dev_loss_grad (upstream 1, 1, 1),
 * az_train_dev_heads_bwd, az_train_dev_attn_bwd, az_train_dev_block_bwd per block in reverse, az_train_dev_stem_bwd,
 * az_opt_dev_step (the norm to az_learn_out.grad_norm), k_learn_tail (sums += the three losses, batches += 1, the entropy
 * copied).  `batch` as az_replay_dev_batch writes it; `config` with aux_target_offset 42 for the reference's network;
 * step[i] and group_hp as az_opt_dev_step takes them (HOST arrays; every step >= 1); `call` numbers the batch for the
 * dropout draws.  A handle's steps belong on one stream at a time.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: a null argument; a step before az_learn_bind; N outside
 * [1, max_rows]; a null batch tensor or one that is not 16-byte aligned (valid_mask: any alignment); what
 * az_train_dev_loss refuses of `config` and az_opt_dev_step of step and group_hp. */
int  az_learn_dev_step(az_learn *l, const az_replay_batch *batch, int64_t N, const az_train_loss_config *config,
                       const int64_t *step, const double *group_hp, uint64_t call, void *stream);
/* One epoch over a sample of a replay ring: batch k = az_replay_dev_batch(Connect4, ring, idx, order, k B, min(B, n - k B))
 * into the handle's own batch tensors, then az_learn_dev_step on its 2 B rows with step[i] + k and call first_call + k; no
 * other host work between batches.  The last batch is short unless drop_last.  *n_batches: how many were enqueued.
 * AZ_ERR_ARG, with nothing enqueued: as az_learn_dev_step and az_replay_dev_batch, n <= 0, B <= 0, 2 B > max_rows, a
 * null n_batches, a sample that gives no batch. */
int  az_learn_dev_epoch(az_learn *l, const az_replay_tensors *ring, const int64_t *idx, const int64_t *order, int64_t n,
                        int64_t B, int drop_last, const az_train_loss_config *config, const int64_t *step,
                        const double *group_hp, uint64_t first_call, int64_t *n_batches, void *stream);
/* The forward without keeps, nothing saved, and az_train_dev_loss on it: az_learn_out.losses and .counts hold the batch's
 * losses and confusion afterwards; sums, batches, entropy, grad_norm and every network tensor stay as they are.
 * AZ_ERR_ARG as az_learn_dev_step. */
int  az_learn_dev_eval(az_learn *l, const az_replay_batch *batch, int64_t N, const az_train_loss_config *config, void *stream);
/* k_learn_keep alone, as az_learn_dev_step launches it for a batch of N rows numbered `call` - for tests and tools; with
 * every rate 0 nothing is enqueued.  AZ_ERR_ARG: a null handle, N outside [1, max_rows]. */
int  az_learn_dev_keep(az_learn *l, int64_t N, uint64_t call, void *stream);
/* The addresses of what the handle keeps for its caller.  AZ_ERR_ARG: a null argument. */
int  az_learn_outputs(az_learn *l, az_learn_out *out);
/* sums, batches and entropy to zero, on `stream`. */
int  az_learn_reset_sums(az_learn *l, void *stream);
/* What the learner has just trained, into a live evaluator: az_nn_model_publish (include/az_nn.h) with its source struct
 * filled from the tensors az_learn_bind holds by role.  One launch on `stream`, a 12-byte copy and ONE wait for `stream`
 * (the three head biases are kernel arguments of the evaluator); not to be captured, and no forward of `m` may be in
 * flight elsewhere meanwhile.  scalars_dev: three float32 in device memory, 4-byte aligned, the caller's.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: a null argument; a call before az_learn_bind; a model that is
 * not a Connect4 network or whose n_blocks differs from the learner's; whatever else az_nn_model_publish refuses. */
int  az_learn_publish(az_learn *l, struct az_nn_model *m, float *scalars_dev, void *stream);

/* ---- The Connect4 residual block's training forward and backward (alphazero-al_amd/csrc/train_block_kernels.hip):
 * y = x + keep * silu(conv3x3(GroupNorm(1, 64)(x))), the reference's `ResidualBlock(64, 64)` with its Dropout2d factor
 * handed in.  Everything float32, contiguous, in DEVICE memory; x, y, dy, dx are [N][64][6][7] (NCHW as torch holds
 * them), conv_weight [64][64][3][3] (OIHW), keep [N][64] (0 or 1 / (1 - p) per sample and channel) or null for all ones.
 *
 * Forward, one launch, per sample n (2688 values):
 *   mean = sum x / 2688;  rstd = 1 / sqrt(sum (x - mean)^2 / 2688 + eps)           (the biased variance, as group_norm)
 *   xn   = (x - mean) * rstd * norm_weight[c] + norm_bias[c]
 *   z    = conv3x3(xn, conv_weight) + conv_bias[o]     zero padding: a tap outside the board contributes nothing
 *   y    = x + keep[n][o] * (z * sigmoid(z))
 * Saved for the backward when asked: z [N][64][6][7] and stats [N][2] = (mean, rstd).  Nothing else is kept: the backward
 * reads x again and forms xn as the forward did.
 * Backward, two launches (s = sigmoid(z), xhat = (x - mean) * rstd):
 *   dz      = dy * keep * (s + z * s * (1 - s))
 *   d_conv_bias[o]           = sum over n, cell of dz
 *   d_conv_weight[o][c][tap] = sum over n, cell of dz[n][o][cell] * xn[n][c][cell + tap]
 *   dxn     = conv_transpose(dz, conv_weight)
 *   d_norm_bias[c] = sum dxn;   d_norm_weight[c] = sum dxn * xhat
 *   g = dxn * norm_weight[c];   dx = dy + rstd * (g - mean_n(g) - xhat * mean_n(g * xhat))       mean_n: over the sample
 * The four parameter gradients are sums over the batch: every workgroup of the first launch walks a contiguous run of
 * samples and leaves ONE partial row (37056 floats: d_conv_weight, d_conv_bias, d_norm_weight, d_norm_bias) in the
 * caller's workspace; the second launch adds the rows in row order.  No atomics, nothing cleared beforehand: two calls
 * on the same inputs give the same bytes.  `max_workgroups` caps the workgroups that walk the batch (and with them the
 * rows): 0 is the unit's default, 256; values above 1024 count as 1024; N below the cap gives N rows.
 * The matrix products run on the f32-input MFMA (a k-ordered chain of float32 fused multiply-adds): exact float32,
 * nothing narrower anywhere.  Different caps add in different orders: their results agree to rounding, not in bytes. */
typedef struct az_train_block_params {
    const float *norm_weight;   /* [64]  4-byte aligned */
    const float *norm_bias;     /* [64]  4-byte aligned */
    const float *conv_weight;   /* [64][64][3][3]  16-byte aligned */
    const float *conv_bias;     /* [64]  4-byte aligned */
} az_train_block_params;
#define AZ_TRAIN_BLOCK_PARAMS_BYTES 32
typedef struct az_train_block_saved {
    float *z;                   /* [N][64][6][7]  16-byte aligned */
    float *stats;               /* [N][2] mean, rstd  4-byte aligned */
} az_train_block_saved;
#define AZ_TRAIN_BLOCK_SAVED_BYTES 16
typedef struct az_train_block_grads {
    float  *dx;                 /* [N][64][6][7]  16-byte aligned */
    float  *d_norm_weight;      /* [64]  4-byte aligned */
    float  *d_norm_bias;        /* [64]  4-byte aligned */
    float  *d_conv_weight;      /* [64][64][3][3]  16-byte aligned */
    float  *d_conv_bias;        /* [64]  4-byte aligned */
    void   *workspace;          /* 16-byte aligned; its contents need not be kept */
    int64_t workspace_bytes;    /* at least az_train_block_workspace_bytes(N, max_workgroups) */
} az_train_block_grads;
#define AZ_TRAIN_BLOCK_GRADS_BYTES 56
#ifdef __cplusplus
static_assert(sizeof(az_train_block_params) == AZ_TRAIN_BLOCK_PARAMS_BYTES && sizeof(az_train_block_saved) == AZ_TRAIN_BLOCK_SAVED_BYTES &&
              sizeof(az_train_block_grads) == AZ_TRAIN_BLOCK_GRADS_BYTES, "az_train_block pointer structs");
#else
_Static_assert(sizeof(az_train_block_params) == AZ_TRAIN_BLOCK_PARAMS_BYTES && sizeof(az_train_block_saved) == AZ_TRAIN_BLOCK_SAVED_BYTES &&
               sizeof(az_train_block_grads) == AZ_TRAIN_BLOCK_GRADS_BYTES, "az_train_block pointer structs");
#endif

/* Bytes of workspace a backward over N samples needs under this cap; -1 for N <= 0, N beyond 2^30 or a negative cap. */
int64_t az_train_block_workspace_bytes(int64_t N, int max_workgroups);
/* The forward: one launch on `stream`, nothing waits for the device, nothing is allocated.  `saved` null, or both of its
 * pointers null: eval or no-grad, nothing is saved.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: N <= 0 or beyond 2^30; a null `params`, x, y or parameter;
 * x, y, conv_weight, keep (when given) or saved z not 16-byte aligned (the three 64-vectors and stats: 4-byte);
 * eps not positive or not finite; exactly one of the two save pointers null. */
int az_train_dev_block_fwd(const az_train_block_params *params, const float *x, const float *keep, int64_t N, float eps,
                           float *y, const az_train_block_saved *saved, void *stream);
/* The backward: two launches on `stream`, nothing waits for the device, nothing is allocated.  x, keep and `params` as
 * the forward had them, `saved` what it left.  Inputs are read, never written.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: as above, plus a null struct, dy, saved pointer, gradient or
 * workspace; dy, dx, d_conv_weight or the workspace not 16-byte aligned (the three 64-vectors: 4-byte);
 * max_workgroups < 0; workspace_bytes below what az_train_block_workspace_bytes(N, max_workgroups) says. */
int az_train_dev_block_bwd(const az_train_block_params *params, const float *x, const float *keep, const float *dy,
                           const az_train_block_saved *saved, int64_t N, int max_workgroups,
                           const az_train_block_grads *grads, void *stream);

/* ---- The Connect4 gated attention block's training forward and backward (alphazero-al_amd/csrc/train_attn_kernels.hip):
 * the reference's `AttentionBlock(64, 4, dropout)` round `GatedAttention`, the last layer of `hidden`, with its dropout
 * mask handed in.  Everything float32, contiguous, in DEVICE memory.  x and dx are [N][64][6][7] (x_token_major 0: NCHW,
 * cell t = 7 * row + col is token t) or [N][42][64] (x_token_major 1: the memory of a channels-last NCHW tensor); y and dy
 * are [N][42][64], token-major, as the heads take it.  dx leaves in the layout x came in.
 *
 * Forward, one launch, per sample, with rms(v, w) = v * (1 / sqrt(mean(v^2) + eps)) * w:
 *   tok[t][c] = x[c][t]
 *   h[t]      = rms(tok[t], prenorm_weight)                                 over the 64 channels
 *   qkv[t]    = qkv_weight @ h[t]        q, k, v of head a: elements 16 a .. 16 a + 15 of thirds 0, 1, 2
 *   g[t][a]   = gate_weight[a] . h[t]
 *   qh, kh    = rms(q[t][a], q_norm_weight), rms(k[t][a], k_norm_weight)    over the 16 of a head, the same eps
 *   P[a][i][:] = softmax_j(0.25 * qh[i][a] . kh[j][a])                      over the 42 keys, the row maximum taken out
 *   P'        = P * keep(a, i, j) * keep_scale
 *   O[i][a]   = sum_j P'[a][i][j] * v[j][a];   o[i][a] = sigmoid(g[i][a]) * O[i][a]
 *   y[i]      = o_weight @ concat_a o[i][a] + tok[i]
 * keep_bits is [N][4][42] uint64: bit j of word (n, a, i) says that probability (a, i, j) is kept; bits 42 .. 63 are
 * ignored.  Null: all kept, and keep_scale must be 1.  The mask is an input so that a float64 restatement can use the
 * same one and two calls are reproducible.
 * Backward, two launches.  NOTHING is saved between the passes: the backward reads x and keep_bits again and runs the
 * forward up to O once more (s = sigmoid(g), hn = tok * rinv, qn = q * rq: the normalised values before their weight):
 *   d_o_weight[c][c'] = sum over n, i of dy[i][c] * o[i][c'];        do = dy @ o_weight
 *   dO = do * s;   dg = (sum_d do * O) * s * (1 - s);   delta[i] = sum_d dO[i] * O[i]     (= sum_j P' dP')
 *   dP'[i][j] = dO[i] . v[j];   dv[j] = sum_i P'[i][j] * dO[i]
 *   dS[i][j]  = 0.25 * P[i][j] * (keep * keep_scale * dP'[i][j] - delta[i])
 *   dqh[i] = sum_j dS[i][j] * kh[j];   dkh[j] = sum_i dS[i][j] * qh[i]
 *   d_q_norm_weight[d] = sum dqh * qn;   u = dqh * q_norm_weight;   dq = rq * (u - qn * mean_d(u * qn))      (k alike)
 *   d_qkv_weight[o][c] = sum over n, t of dqkv[t][o] * h[t][c];      d_gate_weight[a][c] = sum dg[t][a] * h[t][c]
 *   dh = dqkv @ qkv_weight + dg @ gate_weight
 *   d_prenorm_weight[c] = sum dh * hn;   u = dh * prenorm_weight;   dx's token = dy + rinv * (u - hn * mean_c(u * hn))
 * The six parameter gradients are sums over the batch: every workgroup of the first launch walks a contiguous run of
 * samples and leaves ONE partial row (16736 floats: d_qkv_weight, d_o_weight, d_gate_weight, d_prenorm_weight,
 * d_q_norm_weight, d_k_norm_weight) in the caller's workspace; the second launch adds the rows in row order.  No atomics,
 * nothing cleared beforehand: two calls on the same inputs give the same bytes.  `max_workgroups` caps the workgroups
 * that walk the batch (and with them the rows): 0 is the unit's default, 256; values above 1024 count as 1024; N below
 * the cap gives N rows.  The matrix products run on the f32-input MFMA: exact float32, nothing narrower anywhere.
 * Different caps add in different orders: their results agree to rounding, not in bytes. */
typedef struct az_train_attn_params {
    const float *prenorm_weight;    /* [64]  4-byte aligned */
    const float *qkv_weight;        /* [192][64]  16-byte aligned */
    const float *gate_weight;       /* [4][64]  4-byte aligned */
    const float *o_weight;          /* [64][64]  16-byte aligned */
    const float *q_norm_weight;     /* [16]  4-byte aligned */
    const float *k_norm_weight;     /* [16]  4-byte aligned */
} az_train_attn_params;
#define AZ_TRAIN_ATTN_PARAMS_BYTES 48
typedef struct az_train_attn_grads {
    float  *dx;                     /* x's shape and layout  16-byte aligned */
    float  *d_prenorm_weight;       /* [64]  4-byte aligned */
    float  *d_qkv_weight;           /* [192][64]  16-byte aligned */
    float  *d_gate_weight;          /* [4][64]  4-byte aligned */
    float  *d_o_weight;             /* [64][64]  16-byte aligned */
    float  *d_q_norm_weight;        /* [16]  4-byte aligned */
    float  *d_k_norm_weight;        /* [16]  4-byte aligned */
    void   *workspace;              /* 16-byte aligned; its contents need not be kept */
    int64_t workspace_bytes;        /* at least az_train_attn_workspace_bytes(N, max_workgroups) */
} az_train_attn_grads;
#define AZ_TRAIN_ATTN_GRADS_BYTES 72
#ifdef __cplusplus
static_assert(sizeof(az_train_attn_params) == AZ_TRAIN_ATTN_PARAMS_BYTES && sizeof(az_train_attn_grads) == AZ_TRAIN_ATTN_GRADS_BYTES,
              "az_train_attn pointer structs");
#else
_Static_assert(sizeof(az_train_attn_params) == AZ_TRAIN_ATTN_PARAMS_BYTES && sizeof(az_train_attn_grads) == AZ_TRAIN_ATTN_GRADS_BYTES,
               "az_train_attn pointer structs");
#endif

/* Bytes of workspace a backward over N samples needs under this cap; -1 for N <= 0, N beyond 2^30 or a negative cap. */
int64_t az_train_attn_workspace_bytes(int64_t N, int max_workgroups);
/* The forward: one launch on `stream`, nothing waits for the device, nothing is allocated.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: N <= 0 or beyond 2^30; a null `params`, x, y or parameter;
 * x, y, qkv_weight or o_weight not 16-byte aligned (keep_bits, when given: 8-byte; the four small parameters: 4-byte);
 * eps not positive or not finite; keep_scale not finite or below 1, or not 1 with null keep_bits; x_token_major other
 * than 0 or 1. */
int az_train_dev_attn_fwd(const az_train_attn_params *params, const float *x, int x_token_major,
                          const uint64_t *keep_bits, float keep_scale, int64_t N, float eps, float *y, void *stream);
/* The backward: two launches on `stream`, nothing waits for the device, nothing is allocated.  x, x_token_major,
 * keep_bits, keep_scale, eps and `params` as the forward had them (the forward is run again, so its eps is needed here
 * too).  Inputs are read, never written.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: as above, plus a null struct, dy, gradient or workspace; dy, dx,
 * d_qkv_weight, d_o_weight or the workspace not 16-byte aligned (the four small gradients: 4-byte); max_workgroups < 0;
 * workspace_bytes below what az_train_attn_workspace_bytes(N, max_workgroups) says. */
int az_train_dev_attn_bwd(const az_train_attn_params *params, const float *x, int x_token_major,
                          const uint64_t *keep_bits, float keep_scale, const float *dy, int64_t N, float eps,
                          int max_workgroups, const az_train_attn_grads *grads, void *stream);

/* ---- The Connect4 stem's training forward and backward (alphazero-al_amd/csrc/train_stem_kernels.hip): the reference's
 * `_embed_state`, `hidden[0]` (Conv2d(32, 64, 3, padding 1)) and `hidden[1]` (SiLU) as one function.  Everything float32,
 * contiguous, in DEVICE memory: state [N][3][6][7] (planes 0 and 1 are MULTIPLIERS - own, opponent - of any value, plane
 * 2 is never read), piece_emb [2][32], pos_emb [24][32], conv_weight [64][32][3][3] (OIHW), conv_bias [64]; y and dy are
 * [N][64][6][7] (NCHW, contiguous: what the first residual block takes without a copy).
 *   orbit(cell) = 4 * (cell / 7) + min(cell % 7, 6 - cell % 7)                     a constant of the game, compiled in
 *   t[n][c][cell] = (state[n][0][cell] * piece_emb[0][c] + state[n][1][cell] * piece_emb[1][c]) + pos_emb[orbit(cell)][c]
 *   z = conv3x3(t, conv_weight) + conv_bias[o]        zero padding: a tap outside the board contributes an exact zero
 *   y = z * sigmoid(z)
 * Backward (s = sigmoid(z)):
 *   dz = dy * (s + z * s * (1 - s))
 *   d_conv_bias[o]           = sum over n, cell of dz
 *   d_conv_weight[o][c][tap] = sum over n, cell of dz[n][o][cell] * t[n][c][cell + tap]
 *   dt = conv_transpose(dz, conv_weight)
 *   d_piece_emb[j][c] = sum over n, cell of state[n][j][cell] * dt[n][c][cell]
 *   d_pos_emb[k][c]   = sum over n and the cells of orbit k of dt[n][c][cell]
 * state gets no gradient.
 * HOW it is computed.  The convolution is linear and t is linear in 26 features per cell, S[n][f][cell]: the two planes
 * (f = 0, 1) and the one-hot of the cell's orbit (f = 2 .. 25); with Emb = [piece_emb; pos_emb] ([26][32]), t = Emb^T S.
 * Forward, two launches: the first folds the parameters into a table of 3840 floats,
 *   T[o][f][tap] = sum_c conv_weight[o][c][tap] * piece_emb[f][c]   (f < 2)      Pz = conv3x3(pos_emb[orbit(.)]) + conv_bias
 * at the head of `workspace`; the second forms z[o][cell] = Pz[o][cell] + sum over f < 2, tap of state_f[cell + tap] *
 * T[o][f][tap] per sample: 18 terms where the direct form has 288.
 * Backward, three launches.  NOTHING per sample is saved: z is formed again from state and the table.  Everything follows
 * from G[o][f][tap] = sum over n, cell of dz[n][o][cell] * S[n][f][cell + tap]:
 *   d_conv_weight[o][c][tap] = sum_f G[o][f][tap] * Emb[f][c];       dEmb[f][c] = sum over o, tap of G[o][f][tap] * conv_weight[o][c][tap]
 * G's piece part (f < 2) is a [64][18] sum over the samples; its position part needs only D[o][cell] = sum_n dz[n][o][cell],
 * because the one-hot does not depend on n; d_conv_bias[o] = sum_cell D[o][cell].  Every workgroup of the first launch
 * walks a contiguous run of samples and leaves ONE partial row (3840 floats: D, G's piece part) in the caller's
 * workspace; the second adds the rows in row order; the third unfolds the sum into the four gradients.  No atomics,
 * nothing cleared beforehand: two calls on the same inputs give the same bytes.  `max_workgroups` caps the workgroups
 * that walk the batch (and with them the rows): 0 is the unit's default, 256; values above 1024 count as 1024; N below
 * the cap gives N rows.  Every sum is a chain of float32 fused multiply-adds; nothing narrower anywhere.  Different caps
 * add in different orders: their results agree to rounding, not in bytes.
 * `table`, although the backward is a function of state, the parameters and dy alone: the backward
 * takes the forward's table instead of folding the parameters a second time, which would cost a fourth launch or, inside
 * the sample walk, more than the walk itself at a thousand samples.  It is a function of the parameters alone: any
 * forward on the same parameters leaves the one the backward needs. */
typedef struct az_train_stem_params {
    const float *piece_emb;     /* [2][32]  4-byte aligned */
    const float *pos_emb;       /* [24][32]  4-byte aligned */
    const float *conv_weight;   /* [64][32][3][3]  4-byte aligned */
    const float *conv_bias;     /* [64]  4-byte aligned */
} az_train_stem_params;
#define AZ_TRAIN_STEM_PARAMS_BYTES 32
typedef struct az_train_stem_grads {
    float  *d_piece_emb;        /* [2][32]  4-byte aligned */
    float  *d_pos_emb;          /* [24][32]  4-byte aligned */
    float  *d_conv_weight;      /* [64][32][3][3]  4-byte aligned */
    float  *d_conv_bias;        /* [64]  4-byte aligned */
    void   *workspace;          /* 16-byte aligned; its contents need not be kept */
    int64_t workspace_bytes;    /* at least az_train_stem_workspace_bytes(N, max_workgroups) */
} az_train_stem_grads;
#define AZ_TRAIN_STEM_GRADS_BYTES 48
#define AZ_TRAIN_STEM_TABLE_BYTES 15360
#ifdef __cplusplus
static_assert(sizeof(az_train_stem_params) == AZ_TRAIN_STEM_PARAMS_BYTES && sizeof(az_train_stem_grads) == AZ_TRAIN_STEM_GRADS_BYTES,
              "az_train_stem pointer structs");
#else
_Static_assert(sizeof(az_train_stem_params) == AZ_TRAIN_STEM_PARAMS_BYTES && sizeof(az_train_stem_grads) == AZ_TRAIN_STEM_GRADS_BYTES,
               "az_train_stem pointer structs");
#endif

/* Bytes of a workspace that serves both passes over N samples under this cap: the forward's table
 * (AZ_TRAIN_STEM_TABLE_BYTES, at its head, which the backward never writes), the added row and the partial rows;
 * -1 for N <= 0, N beyond 2^30 or a negative cap. */
int64_t az_train_stem_workspace_bytes(int64_t N, int max_workgroups);
/* The forward: two launches on `stream`, nothing waits for the device, nothing is allocated.  It needs the first
 * AZ_TRAIN_STEM_TABLE_BYTES of `workspace` only and leaves the table there.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: N <= 0 or beyond 2^30; a null `params`, state, y, parameter or
 * workspace; y or the workspace not 16-byte aligned (state and the parameters: 4-byte); workspace_bytes below
 * AZ_TRAIN_STEM_TABLE_BYTES. */
int az_train_dev_stem_fwd(const az_train_stem_params *params, const float *state, int64_t N, float *y,
                          void *workspace, int64_t workspace_bytes, void *stream);
/* The backward: three launches on `stream`, nothing waits for the device, nothing is allocated.  state and `params` as
 * the forward had them; `table`: the AZ_TRAIN_STEM_TABLE_BYTES a forward on these parameters left at the head of its
 * workspace (it may be the head of `grads->workspace` itself).  Inputs, the table included, are read, never written.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: as above, plus a null struct, table, dy, gradient or workspace;
 * table, dy or the workspace not 16-byte aligned (the four gradients: 4-byte); max_workgroups < 0; workspace_bytes below
 * what az_train_stem_workspace_bytes(N, max_workgroups) says. */
int az_train_dev_stem_bwd(const az_train_stem_params *params, const float *state, const float *table, const float *dy,
                          int64_t N, int max_workgroups, const az_train_stem_grads *grads, void *stream);

/* ---- The Connect4 heads' training forward and backward (alphazero-al_amd/csrc/train_heads_kernels.hip): the reference's
 * `ColumnPolicyHead(64, dropout)` and `DualHead(64, 3, dropout)` as one function of the tokens, with their two dropout
 * factors handed in.  Everything float32, contiguous, in DEVICE memory.  tokens and d_tokens are [N][42][64], what
 * az_train_dev_attn_fwd writes and az_train_dev_attn_bwd takes as dy; token t = 7 * row + col.  legal is [N][7] bytes (a
 * bool tensor's memory; non-zero = legal) or null for all legal.  keep_policy is [N][7][64] and keep_pool [N][64]: 0 or
 * 1 / (1 - p) per element, or null for all ones.  log_p is [N][7], value [N][3], steps [N]: what az_train_dev_loss reads.
 *
 * Forward, one launch, per sample, with rms(v, w) = v * (1 / sqrt(mean(v^2) + eps)) * w over the 64 channels and ONE eps
 * for all four norms:
 *   policy:  xn[t]    = rms(tok[t], policy_norm_weight)
 *            s[t]     = row_gate_weight . xn[t] + row_gate_bias
 *            w[r][c]  = softmax over the 6 rows r of s[7 r + c], the column's maximum taken out
 *            colf[c]  = sum_r w[r][c] * xn[7 r + c]
 *            u[c]     = policy_fc_weight @ colf[c] + policy_fc_bias;     a[c] = u * sigmoid(u) * keep_policy[n][c]
 *            logit[c] = legal ? policy_out_weight . a[c] + policy_out_bias : -1e9
 *            log_p    = logit - max - log(sum exp(logit - max))       (all seven illegal: every entry is -log 7)
 *   value:   m        = (sum_t tok[t]) / 42
 *            z1       = pool_fc_weight @ rms(m, pool_norm_weight) + pool_fc_bias;   x1 = m + keep_pool[n] * z1 * sigmoid(z1)
 *            z2       = fc_weight @ rms(x1, norm_weight) + fc_bias;                 h  = rms(z2 * sigmoid(z2), out_norm_weight)
 *            value    = log_softmax(value_out_weight @ h + value_out_bias);         steps = sigmoid(aux_out_weight . h + aux_out_bias)
 * Backward, two launches.  NOTHING is saved between the passes: the backward reads tokens, legal and the keeps again and
 * runs the forward once more (a sample is 10.5 KB; forming it again is cheaper than writing intermediates), which is why
 * eps is its argument too.  With silu'(z) = s + z s (1 - s), s = sigmoid(z), and for y = rms(v, w), vn = v * r:
 * dv = r * (g * w - vn * mean(g * w * vn)), dw = sum g * vn:
 *   d_logit[c] = legal ? d_log_p[c] - exp(log_p[c]) * sum over ALL seven k of d_log_p[k] : 0
 *   d_policy_out_bias = sum d_logit;  d_policy_out_weight = sum d_logit[c] * a[c];  du[c] = d_logit[c] * policy_out_weight * keep_policy * silu'(u[c])
 *   d_policy_fc_bias = sum du;  d_policy_fc_weight[o][i] = sum du[c][o] * colf[c][i];  dcolf[c] = policy_fc_weight^T du[c]
 *   dw[r][c] = dcolf[c] . xn[7 r + c];  ds[r][c] = w[r][c] * (dw[r][c] - sum_r' w[r'][c] dw[r'][c])
 *   d_row_gate_bias = sum ds;  d_row_gate_weight = sum ds[t] * xn[t];  dxn[t] = w[t] * dcolf[col(t)] + ds[t] * row_gate_weight
 *   d_policy_norm_weight and the policy part of d_tokens through rms
 *   dzv = d_value - exp(value) * sum d_value;  dza = d_steps * steps * (1 - steps);  d_value_out_*, d_aux_out_* from them and h
 *   dh = value_out_weight^T dzv + dza * aux_out_weight -> rms(out_norm) -> * silu'(z2) -> d_fc_*, fc_weight^T -> rms(norm) -> dx1
 *   dz1 = dx1 * keep_pool * silu'(z1) -> d_pool_fc_*, pool_fc_weight^T -> rms(pool_norm) -> dm';   dm = dx1 + dm'
 *   d_tokens[t] = policy part[t] + dm / 42
 * d_row_gate_bias is zero in exact arithmetic (a softmax ignores a shift) and d_policy_out_bias is zero for an all-legal
 * row; both are the plain sums above, so what they hold is rounding.
 * The 18 parameter gradients are sums over the batch: every workgroup of the first launch walks a contiguous run of
 * samples, keeps its share of the sums in registers, and leaves ONE partial row (13126 floats, padded to 13128: the
 * gradients in the order of az_train_heads_params) in the caller's workspace; the second launch adds the rows in row
 * order.  No atomics, nothing cleared beforehand: two calls on the same inputs give the same bytes.  `max_workgroups` caps
 * the workgroups that walk the batch (and with them the rows): 0 is the unit's default, 256; values above 1024 count as
 * 1024; N below the cap gives N rows.  Every sum is a chain of float32 fused multiply-adds; nothing narrower anywhere.
 * Different caps add in different orders: their results agree to rounding, not in bytes. */
typedef struct az_train_heads_params {
    const float *policy_norm_weight;    /* [64]  policy_head.norm.weight  4-byte aligned */
    const float *row_gate_weight;       /* [1][64]  policy_head.row_gate.weight  4-byte aligned */
    const float *row_gate_bias;         /* [1]  4-byte aligned */
    const float *policy_fc_weight;      /* [64][64]  policy_head.fc.weight  16-byte aligned */
    const float *policy_fc_bias;        /* [64]  4-byte aligned */
    const float *policy_out_weight;     /* [1][64]  policy_head.out.weight  4-byte aligned */
    const float *policy_out_bias;       /* [1]  4-byte aligned */
    const float *pool_norm_weight;      /* [64]  dual_head.pool_norm.weight  4-byte aligned */
    const float *pool_fc_weight;        /* [64][64]  dual_head.pool_fc.weight  16-byte aligned */
    const float *pool_fc_bias;          /* [64]  4-byte aligned */
    const float *norm_weight;           /* [64]  dual_head.norm.weight  4-byte aligned */
    const float *fc_weight;             /* [64][64]  dual_head.fc.weight  16-byte aligned */
    const float *fc_bias;               /* [64]  4-byte aligned */
    const float *out_norm_weight;       /* [64]  dual_head.out_norm.weight  4-byte aligned */
    const float *value_out_weight;      /* [3][64]  dual_head.value_out.weight  4-byte aligned */
    const float *value_out_bias;        /* [3]  4-byte aligned */
    const float *aux_out_weight;        /* [1][64]  dual_head.aux_out.weight  4-byte aligned */
    const float *aux_out_bias;          /* [1]  4-byte aligned */
} az_train_heads_params;
#define AZ_TRAIN_HEADS_PARAMS_BYTES 144
typedef struct az_train_heads_grads {
    float  *d_tokens;                   /* [N][42][64]  16-byte aligned */
    float  *d_policy_norm_weight;       /* the parameters' shapes and alignments, in their order */
    float  *d_row_gate_weight;
    float  *d_row_gate_bias;
    float  *d_policy_fc_weight;
    float  *d_policy_fc_bias;
    float  *d_policy_out_weight;
    float  *d_policy_out_bias;
    float  *d_pool_norm_weight;
    float  *d_pool_fc_weight;
    float  *d_pool_fc_bias;
    float  *d_norm_weight;
    float  *d_fc_weight;
    float  *d_fc_bias;
    float  *d_out_norm_weight;
    float  *d_value_out_weight;
    float  *d_value_out_bias;
    float  *d_aux_out_weight;
    float  *d_aux_out_bias;
    void   *workspace;                  /* 16-byte aligned; its contents need not be kept */
    int64_t workspace_bytes;            /* at least az_train_heads_workspace_bytes(N, max_workgroups) */
} az_train_heads_grads;
#define AZ_TRAIN_HEADS_GRADS_BYTES 168
#ifdef __cplusplus
static_assert(sizeof(az_train_heads_params) == AZ_TRAIN_HEADS_PARAMS_BYTES && sizeof(az_train_heads_grads) == AZ_TRAIN_HEADS_GRADS_BYTES,
              "az_train_heads pointer structs");
#else
_Static_assert(sizeof(az_train_heads_params) == AZ_TRAIN_HEADS_PARAMS_BYTES && sizeof(az_train_heads_grads) == AZ_TRAIN_HEADS_GRADS_BYTES,
               "az_train_heads pointer structs");
#endif

/* Bytes of workspace a backward over N samples needs under this cap; -1 for N <= 0, N beyond 2^30 or a negative cap. */
int64_t az_train_heads_workspace_bytes(int64_t N, int max_workgroups);
/* The forward: one launch on `stream`, nothing waits for the device, nothing is allocated.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: N <= 0 or beyond 2^30; a null `params`, tokens, output or
 * parameter; tokens, the three 64 x 64 weights or a keep (when given) not 16-byte aligned (everything else: 4-byte;
 * legal: any); eps not positive or not finite. */
int az_train_dev_heads_fwd(const az_train_heads_params *params, const float *tokens, const uint8_t *legal,
                           const float *keep_policy, const float *keep_pool, int64_t N, float eps,
                           float *log_p, float *value, float *steps, void *stream);
/* The backward: two launches on `stream`, nothing waits for the device, nothing is allocated.  tokens, legal, the keeps,
 * eps and `params` as the forward had them; d_log_p [N][7], d_value [N][3], d_steps [N] are the gradients with respect to
 * the three outputs (what az_train_dev_loss_grad writes).  Inputs are read, never written.
 * AZ_ERR_ARG, with nothing enqueued and nothing written: as above, plus a null struct, upstream gradient, gradient or
 * workspace; d_tokens, the three 64 x 64 gradients or the workspace not 16-byte aligned (everything else: 4-byte);
 * max_workgroups < 0; workspace_bytes below what az_train_heads_workspace_bytes(N, max_workgroups) says. */
int az_train_dev_heads_bwd(const az_train_heads_params *params, const float *tokens, const uint8_t *legal,
                           const float *keep_policy, const float *keep_pool,
                           const float *d_log_p, const float *d_value, const float *d_steps,
                           int64_t N, float eps, int max_workgroups, const az_train_heads_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif
