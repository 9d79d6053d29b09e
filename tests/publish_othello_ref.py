"""A numpy restatement of the Othello evaluator's layout function (include/az_nn.h, az_nn_othello_publish_dev): what
k_publish_othello is held to byte for byte.  State dict in as numpy float32 (the reference's Othello names), every
destination array out as uint16 (bf16 bits) or float32 under the names of az_nn_othello_weights: embed_table, conv{i}_w,
conv{i}_pre_scale / _pre_shift / _post_scale / _post_shift (only for layers that have the BatchNorm), dual_w16,
dual_scale16, dual_shift16, and the heads' board_w .. a_fc_w16, scalars.

Every step is one float32 operation (numpy's float32 sqrt and divide are correctly rounded); bf16 is rounded to
nearest-even by integer arithmetic (publish_ref.bf16_bits).  No torch arithmetic in here.  The keyword switches build the
WRONG variants the tests must tell apart from the right one."""
import numpy as np

from publish_ref import bf16_bits

CH, EMB, FC = 256, 32, 512
ORBIT = np.array([(0, 4, 7, 9)[min(min(r, 7 - r), min(c, 7 - c))] + abs(min(r, 7 - r) - min(c, 7 - c)) for r in range(8) for c in range(8)])
COPIES = (("pass_norm_w", "policy_head.pass_norm.weight"), ("pass_fc_w", "policy_head.pass_fc.weight"), ("v_fc_w", "dual_head.value_out.5.weight"),
          ("v_fc_b", "dual_head.value_out.5.bias"), ("a_fc_b", "dual_head.aux_out.1.bias"), ("a_norm_w", "dual_head.aux_out.2.weight"),
          ("a_out_w", "dual_head.aux_out.5.weight"))
SCALARS = ("policy_head.board_out.bias", "policy_head.pass_fc.bias", "dual_head.aux_out.5.bias")


def n_blocks_of(sd):
    n = 0
    while "stem.%d.conv1.weight" % (3 + n) in sd:
        n += 1
    return n


def conv_names(n_blocks):
    """[(weight, BatchNorm in front or None, BatchNorm behind or None)] in the order of az_nn_othello_weights.conv"""
    out = [("stem.0.weight", None, "stem.1")]
    for k in range(n_blocks):
        out += [("stem.%d.conv1.weight" % (3 + k), "stem.%d.norm1" % (3 + k), None), ("stem.%d.conv2.weight" % (3 + k), "stem.%d.norm2" % (3 + k), None)]
    out.append(("stem.%d.weight" % (3 + n_blocks), None, "stem.%d" % (4 + n_blocks)))
    return out + [("policy_head.stem.0.weight", None, "policy_head.stem.1"), ("policy_head.stem.4.weight", None, "policy_head.stem.5")]


def pack_conv(w, swap_lane=False):
    """[rows][c_in][3][3] float32 -> uint16 [tap][kc][tile][lane = 16 g + tl][j] = bf16(W[16 tile + tl][32 kc + 8 g + j][tap]); rows
    beyond the weight's (the bottleneck's 8 .. 15) are +0.  swap_lane: g and tl change places, lane = 4 tl + g (wrong)."""
    w = np.asarray(w, np.float32)
    rows, c_in = w.shape[0], w.shape[1]
    tiles, nkc = (rows + 15) // 16, c_in // 32
    full = np.zeros((16 * tiles, c_in, 9), np.float32)
    full[:rows] = w.reshape(rows, c_in, 9)
    bits = bf16_bits(full).reshape(tiles, 16, nkc, 4, 8, 9)                     # tile, tl, kc, g, j, tap
    order = (5, 2, 0, 1, 3, 4) if swap_lane else (5, 2, 0, 3, 1, 4)             # tap, kc, tile, then (g, tl) - or (tl, g) - and j
    return np.ascontiguousarray(bits.transpose(order)).reshape(9, nkc, tiles, 64, 8)


def bn_affine(weight, bias, mean, var, eps, eps_after_root=False, unrounded_scale=False):
    """a = var + eps; r = sqrt(a); scale = weight / r; shift = bias - mean * scale: four float32 steps, each rounded once."""
    weight, bias, mean, var = (np.asarray(x, np.float32) for x in (weight, bias, mean, var))
    eps = np.float32(eps)
    if eps_after_root:
        r = (np.sqrt(var) + eps).astype(np.float32)
    else:
        a = (var + eps).astype(np.float32)
        r = np.sqrt(a).astype(np.float32)
    scale = (weight / r).astype(np.float32)
    if unrounded_scale:
        prod = (mean.astype(np.float64) * (weight.astype(np.float64) / r.astype(np.float64))).astype(np.float32)
    else:
        prod = (mean * scale).astype(np.float32)
    return scale, (bias - prod).astype(np.float32)


def bn_affine64(weight, bias, mean, var, eps):
    """The same in float64 from the float32 inputs and the float32 eps."""
    weight, bias, mean, var = (np.asarray(x, np.float32).astype(np.float64) for x in (weight, bias, mean, var))
    scale = weight / np.sqrt(var + np.float64(np.float32(eps)))
    return scale, bias - mean * scale


def norm_of(sd, prefix):
    return tuple(sd["%s.%s" % (prefix, k)] for k in ("weight", "bias", "running_mean", "running_var"))


def embed_table(sd, swap_kinds=False):
    """[4 cell + kind][c] = bf16(pos_emb[orbit(cell)][c] + K[kind][c]), K = own, opponent, legal, illegal."""
    piece, legal = np.asarray(sd["piece_emb.weight"], np.float32), np.asarray(sd["legal_emb.weight"], np.float32)
    kinds = np.stack([piece[0], piece[1], legal[0], legal[1]] if swap_kinds else [piece[0], piece[1], legal[1], legal[0]])
    pos = np.asarray(sd["pos_emb.weight"], np.float32)[ORBIT]
    return bf16_bits((pos[:, None, :] + kinds[None, :, :]).astype(np.float32).reshape(256, EMB))


def a_fc_w16(w, channel_major=False):
    """[out][8 cell + c] = bf16(W[out][64 c + cell]); channel_major: the input index left as it is (wrong)."""
    w = np.asarray(w, np.float32)
    return bf16_bits(w if channel_major else w.reshape(FC, 8, 64).transpose(0, 2, 1).reshape(FC, FC))


def layout(sd, eps, w16=True):
    """name -> array of every destination the launch writes, for a module of `n_blocks_of(sd)` blocks."""
    out = {"embed_table": embed_table(sd)}
    for i, (weight, pre, post) in enumerate(conv_names(n_blocks_of(sd))):
        out["conv%d_w" % i] = pack_conv(sd[weight])
        if pre is not None:
            out["conv%d_pre_scale" % i], out["conv%d_pre_shift" % i] = bn_affine(*norm_of(sd, pre), eps)
        if post is not None:
            out["conv%d_post_scale" % i], out["conv%d_post_shift" % i] = bn_affine(*norm_of(sd, post), eps)
    out["dual_w16"] = pack_conv(sd["dual_head.stem.0.weight"])
    s8, b8 = bn_affine(*norm_of(sd, "dual_head.stem.1"), eps)
    out["dual_scale16"] = np.concatenate([s8, np.ones(8, np.float32)])
    out["dual_shift16"] = np.concatenate([b8, np.zeros(8, np.float32)])
    out["board_w"] = bf16_bits(sd["policy_head.board_out.weight"].reshape(CH))
    out["v_conv_w"] = np.ascontiguousarray(np.asarray(sd["dual_head.value_out.0.weight"], np.float32).reshape(8, 72).T)
    out["v_bn_s"], out["v_bn_b"] = bn_affine(*norm_of(sd, "dual_head.value_out.1"), eps)
    out["a_fc_wt"] = np.ascontiguousarray(np.asarray(sd["dual_head.aux_out.1.weight"], np.float32).T)
    if w16:
        out["a_fc_w16"] = a_fc_w16(sd["dual_head.aux_out.1.weight"])
    for name, key in COPIES:
        out[name] = np.ascontiguousarray(np.asarray(sd[key], np.float32).reshape(-1))
    out["scalars"] = np.array([np.asarray(sd[k], np.float32).reshape(-1)[0] for k in SCALARS], np.float32)
    return out
