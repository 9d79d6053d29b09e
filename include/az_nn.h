/*
 * az_nn.h - C ABI of the leaf evaluator's kernels (part of libaz_mcts.so).
 *
 * These do not replace a reference FFI entry point: the reference's evaluator is a PyTorch
 * module (src/environments/Connect4/Network.py).  Here its forward pass is three HIP launches -
 * stem + first residual block, the other residual blocks, attention + heads - issued either from
 * native code (az_nn_model_forward*, what az_mcts_dev_search runs) or per call from our inference
 * twin of that module (alphazero-al_amd/src/fast_net.py).  All tensors are DEVICE pointers to
 * contiguous bf16 data in token layout (batch, 42, channels) unless stated; `stream` is a
 * hipStream_t; every function only enqueues work and returns 0, or 1 on a bad argument.
 *
 * Compact batches: the kernels of the forward pass (the stem forms, conv_block, stem_conv_block,
 * attn_block, heads, attn_heads) take `batch_dev`, a device pointer to an int64 (or NULL): when
 * given, only the first min(batch, *batch_dev) samples are processed - `batch` sizes the launch,
 * the device decides the work (the leaves that missed the transposition table, az_mcts.h).
 * `gather[b]` (the stem) is the row of the feature tensor / of the positions that compact sample b
 * shows, `scatter[b]` (heads) the row of the mask and of the three output arrays it belongs to;
 * NULL = identity.
 *
 * In this order: the forward pass; the model object, its profiling and publishing weights into it; debug and self-test entry
 * points; kernels kept as test oracles; the Othello network.
 */
#ifndef AZ_NN_H
#define AZ_NN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the forward pass */

/* The stem with the embedding fused in: az_nn_embed + az_nn_conv_block(c_in 32) as one kernel
 * that builds its tokens from the feature planes (no (batch, 42, 32) tensor in HBM). */
int az_nn_stem_embed(const float *features, const void *emb_own, const void *emb_opp, const void *pos,
                     const void *weight_ohwi, const void *bias, void *y, int64_t batch, const int32_t *gather,
                     const int64_t *batch_dev, void *stream);
/* The same with the planes built from leaf POSITIONS in HBM instead of a feature tensor: per row two
 * bitboards (bit = 7 * column + height, Connect4.h:15-29; player +1 / player -1), the side to move and the
 * symmetry id the leaf is shown under (1 = columns mirrored, Connect4.h:249-262) - what selection leaves
 * behind for every leaf.  Saves the 504-byte feature row per leaf and the kernel that writes it. */
typedef struct az_nn_positions {
    const uint64_t *bb_p1, *bb_p2;
    const int32_t *turn, *sym;
} az_nn_positions;
int az_nn_stem_embed_positions(const az_nn_positions *positions, const void *emb_own, const void *emb_opp, const void *pos,
                               const void *weight_ohwi, const void *bias, void *y, int64_t batch, const int32_t *gather,
                               const int64_t *batch_dev, void *stream);
/* The stem from FOLDED tables (nn_stem.hip): the tokens are own * e_own + opp * e_opp + pos with own / opp in {0, 1} and the
 * convolution is linear, so the layer is a K = 18 GEMM on a 0/1 operand built from the planes / bitboards plus a per-cell
 * constant (same inputs, same output as az_nn_stem_embed[_positions], fp32-accurate sums instead of bf16 tokens):
 *   w_frag  bf16 [2][4][64][8]: the table  T[o][k], k = 2 * tap + plane (tap = 3 * ky + kx; plane 0 own, 1 opponent; k >= 18
 *           zero),  T[o][2 tap] = sum_c W[o][c][tap] e_own[c],  T[o][2 tap + 1] likewise with e_opp, split into a bf16 high
 *           part [0] and a bf16 low part [1] (T - high), each in MFMA fragment order: [channel tile i][lane][j] =
 *           part[32 (i / 2) + 8 (r / 4) + 4 (i % 2) + r % 4][8 (lane >> 4) + j] with r = lane & 15 (the rows of two
 *           neighbouring tiles that a lane ends up with are eight consecutive channels);
 *   pmap    float32 [48][68]: rows 0..41, columns 0..63 = conv3x3(pos map, W)[o, cell] + bias[o] (zero padding), the rest 0.
 * Both come from alphazero-al_amd/src/fast_net.py fold_stem. */
int az_nn_stem_folded(const float *features, const void *w_frag, const float *pmap, void *y, int64_t batch,
                      const int32_t *gather, const int64_t *batch_dev, void *stream);
int az_nn_stem_folded_positions(const az_nn_positions *positions, const void *w_frag, const float *pmap, void *y,
                                int64_t batch, const int32_t *gather, const int64_t *batch_dev, void *stream);
/* One whole convolution block as a single MFMA kernel (nn_conv.hip):
 *   y = [x +] silu(conv3x3([GroupNorm1(x) * gamma + beta]) + bias)        (Network.py:27-48,166-170)
 * x (batch, 42, c_in), y (batch, 42, 64); weight_ohwi = the (64, c_in, 3, 3) weight stored
 * output-major with the input channel fastest, i.e. (64, 3, 3, c_in) contiguous
 * (torch channels_last memory of the OIHW tensor).  gamma/beta NULL = no normalisation.
 * Supported: c_in 64 with normalisation (residual 0/1), c_in 32 without either (the stem). */
int az_nn_conv_block(const void *x, int c_in, const void *weight_ohwi, const void *bias, const void *gamma,
                     const void *beta, int residual, void *y, int64_t batch, float eps, const int64_t *batch_dev,
                     void *stream);
/* az_nn_stem_folded_positions followed by the first residual block - az_nn_conv_block(c_in 64, gamma, beta, residual 1) -
 * as ONE kernel (nn_conv.hip): each wavefront computes the stem's output of its sample from the leaf's position into
 * the tile in LDS the block would have staged from HBM, so the (batch, 42, 64) stem output is neither written nor read
 * back.  Arguments: those of the two calls (w_frag, pmap: the stem's tables; weight_ohwi .. beta: the block's).  The
 * arithmetic and the rounding points are those of the two kernels: y is byte-identical to the two launches. */
int az_nn_stem_conv_block_positions(const az_nn_positions *positions, const void *w_frag, const float *pmap,
                                    const void *weight_ohwi, const void *bias, const void *gamma, const void *beta, void *y,
                                    int64_t batch, float eps, const int32_t *gather, const int64_t *batch_dev, void *stream);
/* az_nn_stem_conv_block_positions followed by az_nn_conv_block(c_in 64, gamma, beta, residual 1) for blocks 1 ..
 * n_blocks - 1 as ONE kernel (nn_conv.hip, k_conv_chain): the layers run back to back inside the launch, each with the
 * grid, the tile order and the wave-to-sample rule its own launch has, so a wavefront reads in layer L + 1 only what it
 * stored itself in layer L and no workgroup waits for another.  weight_ohwi .. beta: arrays of n_blocks (1 ..
 * AZ_NN_MAX_BLOCKS) pointers, one per block.  Block i writes y_even (i even) or y_odd (i odd), two distinct (batch, 42,
 * 64) tensors - the buffers the separate launches ping-pong between - so the result is in y_even when n_blocks is odd
 * and in y_odd when it is even; rows from batch_dev on are not written in either.  Every layer is the text of its own
 * kernel: the bytes are those of the separate launches. */
int az_nn_stem_conv_chain_positions(const az_nn_positions *positions, const void *w_frag, const float *pmap, int n_blocks,
                                    const void *const *weight_ohwi, const void *const *bias, const void *const *gamma,
                                    const void *const *beta, void *y_even, void *y_odd, int64_t batch, float eps,
                                    const int32_t *gather, const int64_t *batch_dev, void *stream);
/* The whole gated attention block as a single MFMA kernel (nn_attn.hip):
 *   y = x + o_proj(sigmoid(gate) * softmax(qnorm(Q) knorm(K)^T / 4) V),  [Q|K|V|gate] = qkvg(RMSNorm(x))
 * (Network.py:51-93).  x, y (batch, 42, 64); qkvg_w (196, 64) row-major [out][in] with rows
 * 0-63 Q, 64-127 K, 128-191 V, 192-195 gate; o_w (64, 64) [out][in]; 4 heads of 16.
 * eps is the RMSNorms' epsilon (1e-5 in the reference).  The default forms of this kernel and of az_nn_attn_heads take
 * 1 / sqrt(mean square + eps) as one bare v_rsq_f32, which is exact only for arguments >= FLT_MIN; a call with
 * eps < FLT_MIN (0 included; NaN too) is therefore launched as a second instantiation of the same kernel that takes
 * rsqrtf() there, with its denormal-range guard.  Same output bytes either way. */
int az_nn_attn_block(const void *x, const void *prenorm_w, const void *qkvg_w, const void *q_norm_w,
                     const void *k_norm_w, const void *o_w, void *y, int64_t batch, float eps, const int64_t *batch_dev,
                     void *stream);
/* Both output heads as one kernel (nn_heads.hip): final tokens (batch, 42, 64) ->
 *   probs (batch, 7) f32       softmax of the column policy head, illegal columns (mask byte 0,
 *                              mask (batch, 7) uint8 or NULL) filled with -1e9 before the softmax
 *   wdl (batch, 3) f32         softmax of the value head, RELATIVE order [draw, win, loss]
 *   moves_left (batch) f32     aux_scale * sigmoid(aux head)
 * i.e. exactly the three arrays `predict` returns (Network.py:96-141, 267-288) and
 * az_mcts_dev_backprop consumes.  Weights are bf16 device arrays with the reference's
 * state-dict shapes ([out][in] row-major linears); the four scalars are host floats. */
typedef struct az_nn_heads_weights {
    const void *p_norm, *p_gate_w, *p_fc_w, *p_fc_b, *p_out_w;          /* policy_head.{norm,row_gate,fc,out} */
    const void *d_pool_norm, *d_pool_w, *d_pool_b, *d_norm, *d_fc_w, *d_fc_b, *d_out_norm;
    const void *d_val_w, *d_val_b, *d_aux_w;                             /* dual_head.{value_out,aux_out} */
    float p_gate_b, p_out_b, d_aux_b, aux_scale;
} az_nn_heads_weights;
int az_nn_heads(const void *tokens, const az_nn_heads_weights *w, const uint8_t *mask, float *probs, float *wdl,
                float *moves_left, int64_t batch, float eps, const int32_t *scatter, const int64_t *batch_dev,
                void *stream);
/* az_nn_attn_block followed by az_nn_heads as ONE kernel (nn_attn_heads.hip): the residual stream x (batch, 42, 64)
 * and the weights of both, as those two take them, in; probs, wdl, moves_left out, with mask / scatter / batch_dev as
 * az_nn_heads reads them.  The block's output stays on chip (no token tensor is written); the rounding points are
 * those of the two kernels, so results differ from them only through f32 summation order.  eps: as for
 * az_nn_attn_block (below FLT_MIN the rsqrtf() instantiation is launched). */
int az_nn_attn_heads(const void *x, const void *prenorm_w, const void *qkvg_w, const void *q_norm_w, const void *k_norm_w,
                     const void *o_w, const az_nn_heads_weights *w, const uint8_t *mask, float *probs, float *wdl,
                     float *moves_left, int64_t batch, float eps, const int32_t *scatter, const int64_t *batch_dev,
                     void *stream);

/* ---- the model object and its profiling */

/* The whole evaluator as one call (nn_model.hip), issued from native code on `stream` - what
 * alphazero-al_amd/src/fast_net.py does per call from Python.  The launches:
 *   the stem and the first residual block  az_nn_stem_conv_block_positions - ONE launch - when the model has the folded
 *       stem (stem_frag / stem_pmap) and n_blocks >= 1 and the call is given POSITIONS (AZ_STEM_FUSED=0 in the
 *       environment when the object is created: two launches; same bits either way).  Else a stem form of its own:
 *       az_nn_stem_folded[_positions] with the folded stem, az_nn_stem_embed[_positions] without;
 *       with n_blocks >= 2 that launch is az_nn_stem_conv_chain_positions, which runs every residual block behind the
 *       first one too (AZ_CONV_CHAIN=0 in the environment when the object is created: one launch per block; same bits);
 *   the blocks  az_nn_conv_block (64 -> 64, normalised, residual) for each of the n_blocks not yet run;
 *   attention and heads  az_nn_attn_heads (AZ_ATTN_HEADS_FUSED=0 in the environment when the object is created:
 *       az_nn_attn_block, then az_nn_heads).
 * The object keeps the POINTERS given here (the caller keeps the arrays alive) and nothing changes it or them except
 * az_nn_model_publish / az_nn_model_set_head_biases below; between such calls it may be used from several host threads /
 * streams at once; each call brings its own `scratch`
 * (device memory, az_nn_model_scratch_bytes(batch) bytes: two activation tensors).
 * rows / n_rows: the compact form described at the top (both NULL = every row 0..batch-1). */
#define AZ_NN_MAX_BLOCKS 8
typedef struct az_nn_model_weights {
    const void *emb_own, *emb_opp, *pos;                    /* as az_nn_stem_embed */
    const void *stem_w, *stem_b;
    int32_t n_blocks;                                       /* residual blocks (reference: 3) */
    const void *block_w[AZ_NN_MAX_BLOCKS], *block_b[AZ_NN_MAX_BLOCKS];          /* as az_nn_conv_block */
    const void *block_gamma[AZ_NN_MAX_BLOCKS], *block_beta[AZ_NN_MAX_BLOCKS];
    const void *pre_w, *qkvg_w, *qn_w, *kn_w, *o_w;         /* as az_nn_attn_block */
    az_nn_heads_weights heads;                              /* as az_nn_heads */
    float eps;
    const void *stem_frag;                                  /* as az_nn_stem_folded; both NULL: the stem runs az_nn_stem_embed */
    const float *stem_pmap;
} az_nn_model_weights;
typedef struct az_nn_model az_nn_model;
int az_nn_model_create(const az_nn_model_weights *w, az_nn_model **out);
/* The integer-hash evaluator as a model object (game: 0 Connect4, 1 Othello - AZ_GAME_*): a pure
 * function of the position shown by the feature planes, bit-identical to tests/scenarios.py
 * `hash_eval` / `ot_hash_eval` and to src/hash_eval.py.  Not a network: it exists so that the whole
 * native loop (az_mcts_dev_search) can be compared bit for bit with the CPU oracle, and so that the
 * tree kernels can be timed with no evaluator to speak of.  Needs no scratch. */
int az_nn_model_create_hash(int game, az_nn_model **out);
/* A second deterministic player: `salt` is XOR-ed into the first bitboard word of the position the evaluator
 * is shown (after the symmetry transform) before the hash.  Salt 0 is az_nn_model_create_hash.  Two salts give
 * two different evaluators that numpy reproduces bit for bit (src/hash_eval.py `salt`): the players of the
 * evaluation-match tests (az_match_* in az_mcts.h). */
int az_nn_model_create_hash_salted(int game, uint64_t salt, az_nn_model **out);
#define AZ_NN_KIND_CONNECT4_CNN  0
#define AZ_NN_KIND_HASH_CONNECT4 1
#define AZ_NN_KIND_HASH_OTHELLO  2
int az_nn_model_kind(const az_nn_model *m);
void az_nn_model_destroy(az_nn_model *m);
uint64_t az_nn_model_scratch_bytes(const az_nn_model *m, int64_t batch);
int az_nn_model_forward(const az_nn_model *m, const float *features, const uint8_t *mask, float *probs,
                        float *wdl, float *moves_left, int64_t batch, const int32_t *rows,
                        const int64_t *n_rows, void *scratch, uint64_t scratch_bytes, void *stream);
/* az_nn_model_forward with the leaves given as positions (az_nn_positions above; Othello: bit = 8 * row + col,
 * symmetry ids of Othello.h:45) instead of feature planes: what az_mcts_dev_search feeds the evaluator. */
int az_nn_model_forward_positions(const az_nn_model *m, const az_nn_positions *positions, const uint8_t *mask, float *probs,
                                  float *wdl, float *moves_left, int64_t batch, const int32_t *rows,
                                  const int64_t *n_rows, void *scratch, uint64_t scratch_bytes, void *stream);
/* Kernel timing inside az_nn_model_forward (bench.py's roofline of the evaluator, measured on the
 * launches of the timed region instead of a synthetic one): enable = n >= 1 puts a HIP event pair
 * around the FIRST residual convolution block of every n-th forward call (process-wide, at most
 * 4096 pairs between reads; not while the stream is capturing); az_nn_model_profile_read
 * synchronises the device and returns the summed milliseconds and the number of launches summed. */
int az_nn_model_profile(int enable);
int az_nn_model_profile_read(double *out_ms, int64_t *out_launches);
/* The same for every kernel kind of the forward pass: the stem, the first residual block, the attention
 * block, the heads (an event pair around each on every n-th call): summed milliseconds and launches
 * per kind, in the order of AZ_NN_PROFILE_*.  A call that carries event pairs runs az_nn_attn_block and
 * az_nn_heads as two launches (the fused az_nn_attn_heads has no split to time), and likewise the stem and the first
 * residual block as two (az_nn_stem_conv_block_positions has none either).  Reading empties the rings. */
#define AZ_NN_PROFILE_STEM  0
#define AZ_NN_PROFILE_CONV  1
#define AZ_NN_PROFILE_ATTN  2
#define AZ_NN_PROFILE_HEADS 3
int az_nn_model_profile_read_kernels(double out_ms[4], int64_t out_launches[4]);

/* Publishing trained weights into a live model (alphazero-al_amd/csrc/publish_kernels.hip, k_publish): the evaluator's
 * arrays are a pure function of the network's float32 parameters, and az_nn_publish_dev computes that function in ONE
 * launch, writing the arrays an az_nn_model_weights names IN PLACE - the model handle, the twin's buffers and every
 * pointer inside a captured graph stay valid.  This is the Connect4 network's; the Othello network's is
 * az_nn_othello_publish_dev at the end of this header.
 * Sources: the float32 tensors of the reference's Connect4 state dict in DEVICE memory, contiguous, 4-byte aligned, with
 * the shapes of AZ_LEARN_ROLE_* (az_train.h).  "bf16" = float32 rounded to nearest-even (torch's .to(torch.bfloat16)
 * for finite values and infinities).  Every destination byte is written.
 *   plain casts, same element order:  emb_own, emb_opp = piece_emb[0], [1];  stem_b;  every block's bias, gamma (norm
 *       weight), beta (norm bias);  pre_w, qn_w, kn_w, o_w;  qkvg_w rows 0 .. 191 = qkv_weight, rows 192 .. 195 =
 *       gate_weight;  the 15 pointers of az_nn_heads_weights from the policy_head.* / dual_head.* tensors of the same name
 *   pos[cell][c]       = bf16(pos_emb[orbit(cell)][c]),  orbit(cell) = 4 * (cell / 7) + min(cell % 7, 6 - cell % 7)
 *   stem_w[o][tap][c]  = bf16(W[o][c][tap]),  c_in 32;  every block_w the same with c_in 64  (OIHW -> OHWI)
 *   stem_frag, stem_pmap (when the destination has them): as az_nn_stem_folded above defines them, from
 *       w = float(bf16(W)), b = float(bf16(stem bias)) and the two embedding tables in float32.  The order of every sum
 *       is FIXED, each step one float32 multiply and one float32 add (no fused multiply-add), starting from +0:
 *         T[o][2 tap + plane] = sum over c = 0, 1, .. 31 of w[o][c][tap] * piece_emb[plane][c];   T[o][k >= 18] = 0
 *         hi = bf16(T),  lo = bf16(T - float(hi)),  both scattered into the fragment order
 *         pmap[cell][o] = (one running sum over the taps INSIDE the board, ascending (ky, then kx), and inside a tap over
 *                         c = 0 .. 31, of w[o][c][tap] * pos_emb[orbit(cell + tap)][c]) + b[o], the bias added last;
 *                         rows 42 .. 47 and columns 64 .. 67 are zeros
 *       so that a numpy float32 restatement (tests/publish_ref.py) reproduces the bytes.
 *   scalars_dev[0 .. 2] = row_gate_bias, policy_out_bias, aux_out_bias as float32 (the slot's fourth float is not written)
 * Every job reads sources only; no workgroup waits for another. */
typedef struct az_nn_publish_src {
    const float *piece_emb, *pos_emb, *stem_conv_weight, *stem_conv_bias;       /* [2][32], [24][32], [64][32][3][3], [64] */
    int32_t n_blocks;                                                           /* 1 .. AZ_NN_MAX_BLOCKS */
    const float *block_norm_weight[AZ_NN_MAX_BLOCKS], *block_norm_bias[AZ_NN_MAX_BLOCKS];       /* [64] each */
    const float *block_conv_weight[AZ_NN_MAX_BLOCKS], *block_conv_bias[AZ_NN_MAX_BLOCKS];       /* [64][64][3][3], [64] */
    const float *prenorm_weight, *qkv_weight, *gate_weight, *o_weight, *q_norm_weight, *k_norm_weight;  /* as az_train_attn_params */
    const float *policy_norm_weight, *row_gate_weight, *row_gate_bias, *policy_fc_weight, *policy_fc_bias;  /* as az_train_heads_params */
    const float *policy_out_weight, *policy_out_bias, *pool_norm_weight, *pool_fc_weight, *pool_fc_bias;
    const float *norm_weight, *fc_weight, *fc_bias, *out_norm_weight, *value_out_weight, *value_out_bias;
    const float *aux_out_weight, *aux_out_bias;
} az_nn_publish_src;
#define AZ_NN_PUBLISH_SRC_BYTES 488
#ifdef __cplusplus
static_assert(sizeof(az_nn_publish_src) == AZ_NN_PUBLISH_SRC_BYTES, "az_nn_publish_src");
#else
_Static_assert(sizeof(az_nn_publish_src) == AZ_NN_PUBLISH_SRC_BYTES, "az_nn_publish_src");
#endif
/* The one launch on `stream` and nothing else: it does not wait, allocate or copy, so it may be captured.  It WRITES
 * through dst's pointers (const in the struct because the evaluator only reads them): they must be writable device
 * memory owned by the caller.  dst->stem_frag and dst->stem_pmap may both be NULL: no folded stem; dst's scalars (the
 * four floats of its heads, eps) are not read.
 * Returns 1 with nothing enqueued and nothing written: a null struct, source, destination or scalars_dev; n_blocks
 * outside 1 .. AZ_NN_MAX_BLOCKS or different between src and dst; only one of stem_frag / stem_pmap; a source not 4-byte
 * aligned; a destination written with 16-byte stores - pos, stem_w, every block_w, qkvg_w, o_w, heads.p_fc_w,
 * heads.d_pool_w, heads.d_fc_w, stem_frag - not 16-byte aligned, another bf16 destination not 2-byte aligned, stem_pmap
 * or scalars_dev not 4-byte aligned.  2: the launch was refused. */
int az_nn_publish_dev(const az_nn_publish_src *src, const az_nn_model_weights *dst, float *scalars_dev, void *stream);
/* The three biases that travel to the evaluator kernels BY VALUE inside az_nn_heads_weights, on the host: set them / read
 * them back (out: p_gate_b, p_out_b, d_aux_b).  aux_scale is never touched.  Connect4 network kind only, else 1 (as for
 * a null argument; an Othello model has az_nn_model_set_othello_head_biases below).  A forward enqueued afterwards carries the new values; one captured before carries the old ones. */
int az_nn_model_set_head_biases(az_nn_model *m, float p_gate_b, float p_out_b, float d_aux_b);
int az_nn_model_head_biases(const az_nn_model *m, float out[3]);
/* az_nn_publish_dev on the model's own arrays, then the 12 bytes of scalars_dev to the host, a wait for `stream`, and
 * az_nn_model_set_head_biases with them.  Returns 1 with nothing enqueued as az_nn_publish_dev does, for a model of
 * another kind (an Othello model too: az_nn_model_publish_othello below), and for a stream that is capturing.
 * It WAITS once and must not be captured: the three biases are kernel arguments, so the host has to see them (reading
 * them on the device instead would change the evaluator kernels).
 * No forward of this model may be in flight on another stream, or be enqueued from another thread, during the call;
 * forwards enqueued on `stream` afterwards see the new weights. */
int az_nn_model_publish(az_nn_model *m, const az_nn_publish_src *src, float *scalars_dev, void *stream);

/* ---- debug and self-test entry points */

/* timing experiments on az_nn_conv_block: bit 0 skips its MFMA phase, bit 1 its epilogue and
 * stores, bit 4 records per-wavefront cycle totals of its phases (az_nn_conv_profile: 8 values
 * per wavefront - P1, barrier, MFMA + epilogue, staging wait, barrier, store, and for
 * az_nn_stem_conv_block_positions the stem phase - for the first n / 8 wavefronts of the last launch). */
/* Bit 8 is unused.  az_nn_debug() REPLACES all flags.
 * Bits 16-27 (AZ_NN_DEBUG_GRID_CAP(n)): at most n workgroups in az_nn_attn_heads' grid (0 = one per CU), so that tests
 * reach many samples per wavefront with few samples. */
#define AZ_NN_DEBUG_GRID_CAP(n) (((n) & 0xfff) << 16)
int az_nn_debug(int flags);
int az_nn_debug_flags(void);
int az_nn_conv_profile(unsigned long long *out, int n);
/* Self-test of the paired column reductions (nn_common.h col_sum2 / col_max2) on one wavefront: a, b = 64 floats each
 * (lane l's two values), out = 8 x 64 floats: col_sum2's a and b, col_sum(a), col_sum(b), then the same four with max.
 * Nothing on the evaluator's path calls it. */
int az_nn_debug_col_reduce2(const float *a, const float *b, float *out, void *stream);

/* ---- kept as test oracles: neither the model object nor fast_net's predict_device launches these.  (az_nn_heads_prep
 * also runs in fast_net's forward(), the log-probability path: its torch heads start from the pooled tokens.) */

/* tokens[b, cell, :] = pos[cell, :] + own(b, cell) * emb_own + opp(b, cell) * emb_opp
 * (Network.py:226-239).  features: float32 (batch, 3, 6, 7) relative planes; embed_dim 32. */
int az_nn_embed(const float *features, const void *emb_own, const void *emb_opp, const void *pos,
                void *tokens, int64_t batch, int embed_dim, const int32_t *gather, const int64_t *batch_dev,
                void *stream);
/* policy-head pooling and value-head mean of one pass over the final tokens (batch, 42, 64):
 * col (batch, 7, 64) = softmax-over-rows weighted sum of the RMS-normalised tokens of each
 * column, mean (batch, 64) = plain token mean (Network.py:107-113,135). */
int az_nn_heads_prep(const void *tokens, const void *p_norm_w, const void *p_gate_w, float p_gate_b,
                     void *col, void *mean, int64_t batch, float eps, void *stream);
/* az_nn_conv_block above with c_in 32 (no normalisation, no residual): the stem convolution on az_nn_embed's tokens -
 * the two-launch form that the stem kernels with the embedding fused in are held to, bit for bit. */

/* ---- Othello */

/* One 3x3 convolution layer of the reference's Othello network (Othello/Network.py:22-66,129-139:
 * 256 output channels on 10x10 / 8x8 maps) as an implicit-GEMM MFMA kernel (nn_othello.hip):
 *   y = silu( post_scale * conv3x3( zero_pad( [pre_scale * x + pre_shift] ) ) + post_shift [+ residual] )
 * x (batch, h_in, h_in, c_in) and y, residual (batch, h_out, h_out, 256) are NHWC bf16, h_out =
 * h_in + 2 * pad - 2.  pre_* (c_in floats, both or neither): the BatchNorm in front of the
 * convolution; post_* (256 floats, required: ones / zeros for none): the one behind it.
 * w_packed: the (256, c_in, 3, 3) weight as bf16 in fragment order [tap][c_in / 32][channel tile 16]
 * [lane 64 = 16 * k group + channel][8 input channels] (fast_othello.pack_conv_weight).
 * Supported (c_in, h_in, pad): (32, 8, 2), (256, 10, 1) with or without pre / residual, (256, 10, 0),
 * (256, 8, 1); apply_silu must be 1.  batch_dev (or NULL): device count of a compact batch, as above.
 * Returns 0, 1 on an unsupported combination. */
int az_nn_othello_conv(const void *x, const void *w_packed, const float *pre_scale, const float *pre_shift,
                       const float *post_scale, const float *post_shift, const void *residual, void *y,
                       int64_t batch, int c_in, int h_in, int pad, int apply_silu, const int64_t *batch_dev, void *stream);

/* The dual head's 8-channel bottleneck of the same network (Othello/Network.py:81-83): 3x3, no padding,
 * 256 -> 8 channels on the 10x10 map, BatchNorm, SiLU.  x (batch, 10, 10, 256) NHWC bf16 -> y (batch, 8, 8, 8)
 * NHWC bf16.  w_packed16: the (8, 256, 3, 3) weight padded with zeros to 16 output channels, packed like
 * az_nn_othello_conv's with ONE channel tile; post_*16: 16 floats each (entries 8..15 unused). */
int az_nn_othello_conv_narrow(const void *x, const void *w_packed16, const float *post_scale16,
                              const float *post_shift16, void *y, int64_t batch, const int64_t *batch_dev, void *stream);

/* The thin ends of the same network as kernels (nn_othello_heads.hip), so that the whole Othello evaluator can
 * be one native object.  az_nn_othello_embed: leaf positions (bit = 8 * row + col, symmetry ids of
 * Othello.h:45) + action masks (rows x 65, the symmetrised frame) -> tokens (batch, 8, 8, 32) NHWC bf16 through a
 * (64 cells x 4 kinds, 32) bf16 table: kind 0 own stone, 1 opponent stone, 2 empty and legal, 3 empty and illegal
 * (Othello/Network.py:201-211).  az_nn_othello_heads: the policy stem's output (batch, 8, 8, 256) and the
 * bottleneck (batch, 8, 8, 8), both NHWC bf16 -> probs (rows, 65), relative wdl (rows, 3), score utility (rows):
 * what `predict` returns (Othello/Network.py:40-104, 229-261).  gather / scatter / batch_dev: compact batches. */
typedef struct az_nn_othello_heads_weights {
    const void  *board_w;                 /* policy_head.board_out.weight, 256 bf16 */
    const float *pass_norm_w, *pass_fc_w; /* policy_head.pass_norm.weight, pass_fc.weight: 256 floats each */
    const float *v_conv_w;                /* dual_head.value_out[0].weight as (72, 8): [ci*9 + ky*3 + kx][co] */
    const float *v_bn_s, *v_bn_b;         /* its BatchNorm as scale / shift, 8 each */
    const float *v_fc_w, *v_fc_b;         /* value_out[5]: (3, 72) row-major, (3) */
    const float *a_fc_wt, *a_fc_b;        /* aux_out[1].weight TRANSPOSED to (512 in, 512 out), bias (512) */
    const float *a_norm_w, *a_out_w;      /* aux_out[2].weight (512), aux_out[5].weight (512) */
    float board_b, pass_fc_b, a_out_b;
    float aux_to_score;                   /* aux_target_offset / score_scale (64 / 8) */
    float eps;                            /* the RMSNorms' epsilon (1e-5) */
    const void *a_fc_w16;                 /* optional: aux_out[1].weight as bf16 (512 out, 512 in) with the INPUT index in the
                                           * bottleneck's NHWC order (8 * cell + channel) - the layer then runs on the matrix
                                           * cores, 16 samples per workgroup (k_oth_heads16); NULL: fp32 from a_fc_wt */
} az_nn_othello_heads_weights;
int az_nn_othello_embed(const az_nn_positions *positions, const uint8_t *mask, const void *embed_table, void *tokens,
                        int64_t batch, const int32_t *gather, const int64_t *batch_dev, void *stream);
int az_nn_othello_heads(const void *policy_map, const void *bottleneck, const az_nn_othello_heads_weights *w, float *probs,
                        float *wdl, float *utility, int64_t batch, const int32_t *scatter, const int64_t *batch_dev, void *stream);

/* The whole Othello evaluator as one az_nn_model (kind AZ_NN_KIND_OTHELLO_CNN) for az_mcts_dev_search /
 * az_nn_model_forward_positions: embedding, the body's convolutions in order - conv[0] the stem (32 -> 256,
 * 8x8, pad 2), then pairs (conv1, conv2 with the block's input as residual), then the last body convolution;
 * conv[n_body], conv[n_body + 1] the policy stem (10x10 pad 0, 8x8 pad 1) - the bottleneck convolution, the heads. */
#define AZ_NN_OTHELLO_MAX_CONVS 16
typedef struct az_nn_othello_conv_layer {
    const void *w_packed;
    const float *pre_scale, *pre_shift, *post_scale, *post_shift;
    int32_t residual, c_in, h_in, pad;
} az_nn_othello_conv_layer;
typedef struct az_nn_othello_weights {
    const void *embed_table;
    int32_t n_body, n_convs;                                   /* n_convs = n_body + 2 */
    az_nn_othello_conv_layer conv[AZ_NN_OTHELLO_MAX_CONVS];
    const void *dual_w16;                                      /* as az_nn_othello_conv_narrow */
    const float *dual_scale16, *dual_shift16;
    az_nn_othello_heads_weights heads;
} az_nn_othello_weights;
#define AZ_NN_KIND_OTHELLO_CNN 3
int az_nn_model_create_othello(const az_nn_othello_weights *w, az_nn_model **out);

/* Publishing trained weights into a live Othello model (alphazero-al_amd/csrc/publish_kernels.hip, k_publish_othello): what
 * az_nn_publish_dev above is for the Connect4 network.  The arrays of an az_nn_othello_weights are a pure function of the
 * network's float32 parameters and BatchNorm buffers, and az_nn_othello_publish_dev computes that function in ONE launch,
 * writing the arrays IN PLACE.
 * Sources: float32, DEVICE memory, contiguous, 4-byte aligned, the reference's Othello state dict (Othello/Network.py):
 *   conv_weight[i]  [256][c_in][3][3], in the order of az_nn_othello_weights.conv;  conv_pre[i] / conv_post[i]: the
 *                   BatchNorm in front of / behind convolution i as {weight, bias, running mean, running var}, c_in / 256
 *                   floats each; all four NULL = none (one to three NULL: an error)
 *   the rest        as commented in the struct
 * The destination is an az_nn_othello_weights whose pointers name WRITABLE device memory; c_in, h_in, pad and residual are
 * read from IT, not from the source.  "bf16" = float32 rounded to nearest-even by integer arithmetic (nn_common.h pack2).
 *   embed_table[4 cell + kind][c] = bf16(pos_emb[orbit(cell)][c] + K[kind][c]), ONE float32 add; K = piece_emb[0],
 *       piece_emb[1], legal_emb[1], legal_emb[0] in that order (own stone, opponent stone, empty + legal, empty + illegal);
 *       orbit(cell): with f(i) = min(i, 7 - i), a = min(f(row), f(col)), b = max(f(row), f(col)), the entry
 *       {0, 4, 7, 9}[a] + b - a - the 64 constants of the reference's table (Othello/Network.py _ORBIT_MAP)
 *   conv[i].w_packed[tap][kc][tile][lane = 16 g + tl][j] = bf16(W[16 tile + tl][32 kc + 8 g + j][tap]),  tap 0 .. 8,
 *       kc 0 .. c_in / 32 - 1, tile 0 .. 15, g 0 .. 3, tl 0 .. 15, j 0 .. 7  (fast_othello.pack_conv_weight)
 *   dual_w16        the same order with ONE tile from dual_weight [8][256][3][3]; rows tl = 8 .. 15 are +0
 *   a BatchNorm as an affine:  a = var + bn_eps;  r = sqrt(a);  scale = weight / r;  shift = bias - mean * scale,  each
 *       step ONE correctly rounded float32 operation, no fused multiply-add.  conv_pre[i] -> pre_scale / pre_shift,
 *       conv_post[i] -> post_scale / post_shift, v_bn -> heads.v_bn_s / v_bn_b, dual_bn -> entries 0 .. 7 of dual_scale16 /
 *       dual_shift16, whose entries 8 .. 15 are 1.0f / 0.0f.  A layer whose destination has pre_scale must have conv_pre[i]
 *       and the reverse, else 1.  A layer whose conv_post[i] is all NULL leaves the destination's post_* arrays UNWRITTEN
 *       (the caller's shared ones / zeros)
 *   heads.board_w = bf16(board_weight);  heads.v_conv_w[ci * 9 + k][co] = v_conv_weight[co][ci][k];
 *   heads.a_fc_wt[in][out] = a_fc_weight[out][in];  heads.a_fc_w16[out][8 cell + c] = bf16(a_fc_weight[out][64 c + cell]),
 *       only where the destination has the pointer
 *   plain float32 copies: heads.pass_norm_w, pass_fc_w, v_fc_w, v_fc_b, a_fc_b, a_norm_w, a_out_w
 *   scalars_dev[0 .. 2] = board_bias, pass_fc_bias, a_out_bias (the slot's fourth float is not written); aux_to_score and eps
 *       of the heads are never touched
 * Every destination byte named above is written by exactly one lane; every job reads sources only, so no workgroup waits
 * for another, and two calls on the same inputs give the same bytes. */
typedef struct az_nn_othello_bn_src {
    const float *weight, *bias, *mean, *var;
} az_nn_othello_bn_src;
typedef struct az_nn_othello_publish_src {
    const float *piece_emb, *pos_emb, *legal_emb;                  /* [2][32], [10][32], [2][32] */
    int32_t n_body, n_convs;                                       /* as az_nn_othello_weights */
    float bn_eps;                                                  /* the BatchNorms' common epsilon */
    const float *conv_weight[AZ_NN_OTHELLO_MAX_CONVS];
    az_nn_othello_bn_src conv_pre[AZ_NN_OTHELLO_MAX_CONVS], conv_post[AZ_NN_OTHELLO_MAX_CONVS];
    const float *dual_weight;                                      /* dual_head.stem.0.weight [8][256][3][3] */
    az_nn_othello_bn_src dual_bn;                                  /* dual_head.stem.1, 8 */
    const float *board_weight, *board_bias;                        /* policy_head.board_out: [256], [1] */
    const float *pass_norm_weight, *pass_fc_weight, *pass_fc_bias; /* policy_head.pass_norm, pass_fc: [256], [256], [1] */
    const float *v_conv_weight;                                    /* dual_head.value_out.0.weight [8][8][3][3] */
    az_nn_othello_bn_src v_bn;                                     /* dual_head.value_out.1, 8 */
    const float *v_fc_weight, *v_fc_bias;                          /* dual_head.value_out.5: [3][72], [3] */
    const float *a_fc_weight, *a_fc_bias;                          /* dual_head.aux_out.1: [512][512], [512] */
    const float *a_norm_weight, *a_out_weight, *a_out_bias;        /* dual_head.aux_out.2, aux_out.5: [512], [512], [1] */
} az_nn_othello_publish_src;
#define AZ_NN_OTHELLO_PUBLISH_SRC_BYTES 1368
#ifdef __cplusplus
static_assert(sizeof(az_nn_othello_publish_src) == AZ_NN_OTHELLO_PUBLISH_SRC_BYTES, "az_nn_othello_publish_src");
#else
_Static_assert(sizeof(az_nn_othello_publish_src) == AZ_NN_OTHELLO_PUBLISH_SRC_BYTES, "az_nn_othello_publish_src");
#endif
/* The one launch on `stream` and nothing else: it does not wait, allocate or copy, so it may be captured.  It WRITES
 * through dst's pointers (const in the struct because the evaluator only reads them).  dst's by-value floats are not read.
 * Returns 1 with nothing enqueued and nothing written: a null struct or scalars_dev; a null required pointer (every source
 * but the BatchNorms of layers that have none, every destination but pre_* / post_* of such layers and heads.a_fc_w16);
 * n_body / n_convs that az_nn_model_create_othello refuses, or different between src and dst; a (c_in, h_in, pad) that
 * az_nn_othello_conv does not support; bn_eps not finite or negative; a BatchNorm with only some of its four pointers, or
 * whose presence differs from the destination's (above); a pointer not aligned: 16 bytes for w_packed, dual_w16,
 * embed_table, a_fc_w16 and a_fc_wt, 4 bytes for float arrays and every source, 2 bytes for board_w.  2: the launch was
 * refused.
 * A plain float32 copy whose destination IS its source (the same address) gets no job - a twin hands the model such
 * aliases of the module's parameters; any other overlap of a copy's two ranges returns 1. */
int az_nn_othello_publish_dev(const az_nn_othello_publish_src *src, const az_nn_othello_weights *dst, float *scalars_dev,
                              void *stream);
/* The three biases that travel to the Othello heads kernel BY VALUE inside az_nn_othello_heads_weights, on the host: set
 * them / read them back (out: board_b, pass_fc_b, a_out_b).  aux_to_score and eps are never touched.  Kind
 * AZ_NN_KIND_OTHELLO_CNN only, else 1 (as for a null argument).  A forward enqueued afterwards carries the new values; one
 * captured before carries the old ones. */
int az_nn_model_set_othello_head_biases(az_nn_model *m, float board_b, float pass_fc_b, float a_out_b);
int az_nn_model_othello_head_biases(const az_nn_model *m, float out[3]);
/* az_nn_othello_publish_dev on the model's own arrays, then the 12 bytes of scalars_dev to the host, a wait for `stream`,
 * and az_nn_model_set_othello_head_biases with them.  Returns 1 with nothing enqueued as az_nn_othello_publish_dev does,
 * for a model of another kind, and for a stream that is capturing.
 * It WAITS once and must not be captured: the three biases are kernel arguments, so the host has to see them.
 * No forward of this model may be in flight on another stream, or be enqueued from another thread, during the call;
 * forwards enqueued on `stream` afterwards see the new weights. */
int az_nn_model_publish_othello(az_nn_model *m, const az_nn_othello_publish_src *src, float *scalars_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif