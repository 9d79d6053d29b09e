"""Plain float64 references of the Othello evaluator's kernels (nn_othello.hip, nn_othello_heads.hip) and the
comparison functions the tests hold the kernels to.  No HIP, no bf16 arithmetic, no library convolution: inputs
are the kernels' own bf16 / fp32 arrays widened to float64, and a bf16 rounding is an explicit round-to-nearest-even
of a float64 number, placed exactly where nn_othello.hip's header puts it:

    1. the pre-affine's result          2. the convolution after the post-affine
    3. the sum with the residual        4. the SiLU's result

test_othello_ref_cpu.py anchors every function here to az_net.OthelloNet in float64 and feeds the comparison
functions deliberately wrong references; test_othello_kernels_gpu.py feeds them the kernels' outputs.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


# ---------------------------------------------------------------------------------------------
# bf16 as numbers

def bf16_round(x):
    """float64 -> the nearest bf16 number (ties to even), as float64.  One rounding, from the float64 value itself
    (not through fp32).  Normal range only: the tests stay far from bf16's subnormals and overflow."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)                               # x = m * 2^e, 0.5 <= |m| < 1: bf16 keeps 8 bits of m
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)   # np.rint rounds halves to even


def bf16_bits(x):
    """bf16-representable float64 values -> their bit patterns (uint16)"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), x, equal_nan=True), "not representable in fp32"
    u = f.view(np.uint32)
    assert not (u & np.uint32(0xffff)).any(), "not representable in bf16"
    return (u >> np.uint32(16)).astype(np.uint16)


def bf16_values(bits):
    """bf16 bit patterns (uint16 / int16 array) -> float64"""
    u = np.asarray(bits).view(np.uint16).astype(np.uint32) << np.uint32(16)
    return u.view(np.float32).astype(np.float64)


def bf16_ulp(x):
    """spacing of the bf16 numbers at |x| (of the binade x lies in), normal range"""
    _, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, e - 8)


def silu64(v):
    v = np.asarray(v, dtype=np.float64)
    return v / (1.0 + np.exp(-v))


def bf16_midpoint_band(s, v):
    """True where the float64 SiLU value s (of pre-SiLU value v) lies within (4 + 1.5 |v|) 2^-23 |s| of a midpoint
    between two neighbouring bf16 numbers.  The half-width bounds the error of the kernel's fp32 SiLU - v_mul, v_exp,
    v_add, v_rcp, v_mul at about one ulp each, the exponential's argument error scaled by |v| - so outside the band
    the kernel's rounding to bf16 must pick the same number as the reference's."""
    s = np.asarray(s, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(np.abs(s))
    t = m * 256.0                                    # in [128, 256): bf16 numbers are the integers
    dist = np.abs(t - np.floor(t) - 0.5) * np.ldexp(1.0, e - 8)
    return (s != 0.0) & (dist <= (4.0 + 1.5 * np.abs(v)) * 2.0 ** -23 * np.abs(s))


# ---------------------------------------------------------------------------------------------
# embedding

def unpack_board(bb):
    """uint64 bitboard -> (8, 8) bool, bit = 8 * row + col"""
    bb = int(bb)
    return np.array([[(bb >> (8 * r + c)) & 1 for c in range(8)] for r in range(8)], dtype=bool)


SYMMETRIES = {0: lambda b: b, 2: lambda b: b[::-1, ::-1], 6: lambda b: b.T, 7: lambda b: b[::-1, ::-1].T}


def embed_kinds(bb_p1, bb_p2, turn, sym, mask):
    """(B, 8, 8) cell kinds in the shown frame: 0 own stone, 1 opponent stone, 2 empty and legal, 3 empty and illegal.
    Stone i moves to T_sym(i); the mask (B, 65) is already in the shown frame; a mask bit on an occupied cell is
    ignored."""
    n = len(turn)
    kinds = np.empty((n, 8, 8), dtype=np.int64)
    for i in range(n):
        t = SYMMETRIES[int(sym[i])]
        p1, p2 = t(unpack_board(bb_p1[i])), t(unpack_board(bb_p2[i]))
        own, opp = (p1, p2) if int(turn[i]) > 0 else (p2, p1)
        legal = np.asarray(mask[i][:64]).reshape(8, 8) != 0
        kinds[i] = np.where(own, 0, np.where(opp, 1, np.where(legal, 2, 3)))
    return kinds


def embed_ref(bb_p1, bb_p2, turn, sym, mask, table):
    """-> (B, 8, 8, 32): row 4 * cell + kind of the (256, 32) table"""
    kinds = embed_kinds(bb_p1, bb_p2, turn, sym, mask)
    cell = np.arange(64).reshape(1, 8, 8)
    return np.asarray(table, dtype=np.float64)[4 * cell + kinds]


def embed_mismatch(got_bits, ref):
    """number of bf16 elements of the kernel's tokens (int16 / uint16 bit patterns) that differ from the reference"""
    return int((np.asarray(got_bits).view(np.uint16) != bf16_bits(ref)).sum())


# ---------------------------------------------------------------------------------------------
# convolutions

def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def conv_columns(x, pre, pad, rounded=True):
    """x (B, H, H, C_in) -> the zero-padded windows (B, tokens, C_in * 9), column index ci * 9 + 3 ky + kx.  The
    pre-affine touches real cells only (the padding stays zero) and is rounded to bf16 (rounding point 1)."""
    x = np.asarray(x, dtype=np.float64)
    if pre is not None:
        x = x * np.asarray(pre[0], dtype=np.float64) + np.asarray(pre[1], dtype=np.float64)
        if rounded:
            x = bf16_round(x)
    cols = F.unfold(_t(x).permute(0, 3, 1, 2), kernel_size=3, padding=pad)        # (B, C_in * 9, tokens)
    return cols.transpose(1, 2).contiguous()


def conv_finish(acc, post, residual, rounded=True):
    """the exact sums acc (B, tokens, C_out) -> (result, pre-SiLU value), both (B, H_out, H_out, C_out)"""
    acc = np.asarray(acc, dtype=np.float64)
    b, nt, co = acc.shape
    ho = int(round(math.sqrt(nt)))
    rnd = bf16_round if rounded else (lambda a: a)
    v = rnd(acc * np.asarray(post[0], dtype=np.float64) + np.asarray(post[1], dtype=np.float64))   # rounding point 2
    v = v.reshape(b, ho, ho, co)
    if residual is not None:
        v = rnd(v + np.asarray(residual, dtype=np.float64))                                       # rounding point 3
    return rnd(silu64(v)), v                                                                      # rounding point 4


def conv_sums(cols, w):
    """(B, tokens, C_in * 9) x (C_out, C_in, 3, 3) -> (B, tokens, C_out) in float64"""
    wm = _t(w).reshape(np.shape(w)[0], -1)
    return (cols @ wm.t()).numpy()


def conv_ref(x, w, pre, post, residual, pad, rounded=True):
    """silu(post_s * conv3x3(zero_pad(pre_s * x + pre_b)) + post_b [+ residual]) on NHWC maps, w (C_out, C_in, 3, 3);
    pre / post: (scale, shift) pairs, pre and residual may be None.  -> (result, pre-SiLU value)"""
    return conv_finish(conv_sums(conv_columns(x, pre, pad, rounded), w), post, residual, rounded)


def conv_narrow_ref(x, w8, scale, shift, rounded=True):
    """the bottleneck: x (B, 10, 10, 256), w8 (8, 256, 3, 3), no padding -> (B, 8, 8, 8) result and pre-SiLU value"""
    return conv_ref(x, w8, None, (np.asarray(scale)[:8], np.asarray(shift)[:8]), None, 0, rounded)


def conv_mismatch(got_bits, ref_y, ref_v):
    """What a convolution kernel's bf16 output (bit patterns) breaks of the exact-arithmetic contract: within one bf16
    ulp of the reference everywhere, and EQUAL (as values: -0 == +0) wherever the float64 SiLU value is outside the
    midpoint band.  -> dict(beyond_ulp=count, unequal_outside_band=count, excluded=fraction in the band)"""
    got = bf16_values(got_bits).reshape(np.shape(ref_y))
    ref_y = np.asarray(ref_y, dtype=np.float64)
    band = bf16_midpoint_band(silu64(ref_v), ref_v)
    diff = np.abs(got - ref_y)
    beyond = ~(diff <= np.maximum(bf16_ulp(ref_y), bf16_ulp(got)))               # NaN counts as beyond
    unequal = ~band & ~(got == ref_y)
    return dict(beyond_ulp=int(beyond.sum()), unequal_outside_band=int(unequal.sum()), excluded=float(band.mean()))


def conv_ok(m):
    return m["beyond_ulp"] == 0 and m["unequal_outside_band"] == 0


def pack_weight_ref(w):
    """(C_out, C_in, 3, 3) -> the kernels' fragment order as an index computation of its own (az_nn.h: [tap][C_in / 32]
    [channel tile][lane = 16 * k group + channel][8 input channels]); float64 in, float64 out (values unchanged)"""
    w = np.asarray(w, dtype=np.float64)
    co, ci = w.shape[:2]
    out = np.empty((9, ci // 32, co // 16, 64, 8), dtype=np.float64)
    for tap in range(9):
        for kc in range(ci // 32):
            for tile in range(co // 16):
                blk = w[16 * tile:16 * tile + 16, 32 * kc:32 * kc + 32, tap // 3, tap % 3]      # (channel, 32 inputs)
                out[tap, kc, tile] = blk.reshape(16, 4, 8).transpose(1, 0, 2).reshape(64, 8)
    return out


# ---------------------------------------------------------------------------------------------
# heads

HEADS_KEYS = ("board_w", "board_b", "pass_norm_w", "pass_fc_w", "pass_fc_b", "v_conv_w", "v_bn_s", "v_bn_b", "v_fc_w",
              "v_fc_b", "a_fc_w", "a_fc_b", "a_norm_w", "a_out_w", "a_out_b", "aux_to_score", "eps")


def _w(weights, dtype):
    return {k: torch.as_tensor(np.asarray(weights[k], dtype=np.float64)).to(dtype) for k in HEADS_KEYS}


def _rms(x, weight, eps):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * weight


def policy_ref(policy_map, w):
    """(B, 8, 8, 256) NHWC -> probs (B, 65): 64 square logits of the 1x1 convolution, then the pass logit"""
    pm = policy_map.reshape(policy_map.shape[0], 64, 256)
    squares = (pm * w["board_w"]).sum(-1) + w["board_b"]
    skip = (_rms(pm.mean(dim=1), w["pass_norm_w"], w["eps"]) * w["pass_fc_w"]).sum(-1, keepdim=True) + w["pass_fc_b"]
    return torch.softmax(torch.cat([squares, skip], dim=1), dim=-1)


def value_ref(bottleneck, w, stride=2):
    """(B, 8, 8, 8) NHWC -> wdl (B, 3): 3x3 convolution 8 -> 8 with stride 2 (3x3 outputs), BatchNorm as an affine, SiLU,
    flattened channel-major (co * 9 + position), Linear(72, 3), softmax.  v_conv_w is (co, ci, ky, kx)."""
    h = bottleneck.permute(0, 3, 1, 2)                                            # (B, ci, row, col)
    out = torch.zeros((h.shape[0], 8, 3, 3), dtype=h.dtype)
    for oy in range(3):
        for ox in range(3):
            win = h[:, :, stride * oy:stride * oy + 3, stride * ox:stride * ox + 3]               # (B, ci, ky, kx)
            out[:, :, oy, ox] = (win[:, None] * w["v_conv_w"][None]).sum(dim=(2, 3, 4))
    out = out * w["v_bn_s"].view(1, 8, 1, 1) + w["v_bn_b"].view(1, 8, 1, 1)
    out = out * torch.sigmoid(out)
    return torch.softmax(out.reshape(-1, 72) @ w["v_fc_w"].t() + w["v_fc_b"], dim=-1)


def utility_ref(bottleneck, w):
    """(B, 8, 8, 8) NHWC -> (B,): Linear(512, 512) on the map flattened CHANNEL-major (input 64 c + cell), RMSNorm, SiLU,
    Linear(512, 1), tanh, then atan(aux * aux_to_score) * 2 / pi"""
    flat = bottleneck.permute(0, 3, 1, 2).reshape(-1, 512)
    a = _rms(flat @ w["a_fc_w"].t() + w["a_fc_b"], w["a_norm_w"], w["eps"])
    a = a * torch.sigmoid(a)
    aux = torch.tanh((a * w["a_out_w"]).sum(-1) + w["a_out_b"])
    return torch.atan(aux * w["aux_to_score"]) * (2.0 / math.pi)


def heads_ref(policy_map, bottleneck, weights, dtype=F64):
    """-> probs (B, 65), wdl (B, 3), utility (B) as float64 numpy arrays.  No intermediate roundings.  weights: a dict
    with HEADS_KEYS, the module's shapes (a_fc_w (512 out, 512 in = 64 c + cell), v_conv_w (8, 8, 3, 3), v_fc_w (3, 72)).
    dtype=torch.float32 is the same operation stated in plain fp32: what the kernels' tolerance is measured with."""
    w = _w(weights, dtype)
    pm = torch.as_tensor(np.asarray(policy_map, dtype=np.float64)).to(dtype)
    h8 = torch.as_tensor(np.asarray(bottleneck, dtype=np.float64)).to(dtype)
    return tuple(t.to(F64).numpy() for t in (policy_ref(pm, w), value_ref(h8, w), utility_ref(h8, w)))


HEADS_NAMES = ("probs", "wdl", "utility")
HEADS_FLOOR = 2e-6          # what test_othello_native_model_object holds the two heads kernels to against each other


def heads_errors(got, ref):
    return tuple(float(np.abs(np.asarray(g, dtype=np.float64) - r).max()) for g, r in zip(got, ref))


def heads_problems(got, ref, e32):
    """What heads outputs break: every output at most max(8 * E32, 2e-6) from the float64 reference, E32 being the plain
    fp32 evaluation's own maximum error for that output (8: another summation order and the hardware exponential's
    argument scaling); probs and wdl rows sum to 1 within 1e-5; everything finite.  -> list of strings"""
    out = []
    for name, g, r, e in zip(HEADS_NAMES, got, ref, e32):
        g = np.asarray(g, dtype=np.float64)
        err = np.abs(g - r).max() if np.isfinite(g).all() else float("inf")
        if not err <= max(8.0 * e, HEADS_FLOOR):
            out.append("%s: %.3g from the reference, allowed %.3g" % (name, err, max(8.0 * e, HEADS_FLOOR)))
    for name, g in zip(HEADS_NAMES[:2], got[:2]):
        s = np.abs(np.asarray(g, dtype=np.float64).sum(-1) - 1.0).max()
        if not s <= 1e-5:
            out.append("%s rows sum to 1 +- %.3g" % (name, s))
    return out


def heads_weights_of(net):
    """the heads' weights of an az_net.OthelloNet as heads_ref takes them (float64 numpy)"""
    ph, dh = net.policy_head, net.dual_head
    bn = dh.value_out[1]
    f = lambda t: t.detach().double().cpu().numpy()                               # noqa: E731
    scale = f(bn.weight) / np.sqrt(f(bn.running_var) + bn.eps)
    return dict(board_w=f(ph.board_out.weight).reshape(256), board_b=float(ph.board_out.bias.item()),
                pass_norm_w=f(ph.pass_norm.weight), pass_fc_w=f(ph.pass_fc.weight).reshape(256),
                pass_fc_b=float(ph.pass_fc.bias.item()), v_conv_w=f(dh.value_out[0].weight), v_bn_s=scale,
                v_bn_b=f(bn.bias) - f(bn.running_mean) * scale, v_fc_w=f(dh.value_out[5].weight),
                v_fc_b=f(dh.value_out[5].bias), a_fc_w=f(dh.aux_out[1].weight), a_fc_b=f(dh.aux_out[1].bias),
                a_norm_w=f(dh.aux_out[2].weight), a_out_w=f(dh.aux_out[5].weight).reshape(512),
                a_out_b=float(dh.aux_out[5].bias.item()),
                aux_to_score=float(net.aux_target_offset) / float(net.score_scale), eps=1e-5)


# ---------------------------------------------------------------------------------------------
# the draws both test files share

CONV_CASES = ((32, 8, 2, False, False), (256, 10, 1, True, False), (256, 10, 1, True, True), (256, 10, 1, False, False),
              (256, 10, 0, False, False), (256, 8, 1, False, False))            # c_in, h_in, pad, pre-affine, residual
NARROW = "narrow"


def exact_conv_draw(case, n, seed):
    """Inputs of an exact-arithmetic convolution case: integer inputs in [-2, 2], weights in {-1, 0, +1} / 16 (about a
    quarter non-zero, drawn per tap, input and output channel), pre / post scales in {0.5, 1, 2}, pre shift in
    {-1, 0, 1}, post shift a multiple of 1/16 in [-0.5, 0.5], residual a multiple of 0.5 in [-2, 2].  Every product is a
    multiple of 2^-5 and every partial sum far below 2^24 * 2^-5, so an fp32 accumulation is exact in any order and the
    kernel rounds the same real numbers as the reference at rounding points 1-3.  case: one of CONV_CASES or NARROW.
    -> dict of float64 arrays (x, w, pre, post, residual, pad)"""
    rng = np.random.default_rng(seed)
    cin, hi, pad, pre, res = (256, 10, 0, False, False) if case == NARROW else case
    cout = 8 if case == NARROW else 256
    ho = hi + 2 * pad - 2
    x = rng.integers(-2, 3, (n, hi, hi, cin)).astype(np.float64)
    w = rng.choice([-1.0, 1.0], (cout, cin, 3, 3)) * (rng.random((cout, cin, 3, 3)) < 0.25) / 16.0
    scales = np.array([0.5, 1.0, 2.0])
    d = dict(x=x, w=w, pad=pad, pre=None, residual=None)
    if pre:
        d["pre"] = (rng.choice(scales, cin), rng.integers(-1, 2, cin).astype(np.float64))
    d["post"] = (rng.choice(scales, cout), rng.integers(-8, 9, cout) / 16.0)
    if res:
        d["residual"] = rng.integers(-4, 5, (n, ho, ho, cout)) / 2.0
    return d


def exact_conv_ref(d):
    return conv_ref(d["x"], d["w"], d["pre"], d["post"], d["residual"], d["pad"])


ALL_KERNELS = CONV_CASES + (NARROW,)            # the seven kernels: six geometries of az_nn_othello_conv and the narrow one


@functools.lru_cache(maxsize=None)
def conv_pool(idx):
    """The five distinct samples of kernel ALL_KERNELS[idx] that every exact-arithmetic test draws its batches from
    (sample i of a batch is pool sample i % 5), with their reference: computed once, shared, never changed.
    -> (draw, result, pre-SiLU value)"""
    d = exact_conv_draw(ALL_KERNELS[idx], 5, 100 + idx)
    y, v = exact_conv_ref(d)
    for a in (y, v, d["x"], d["w"]):
        a.setflags(write=False)
    return d, y, v


def random_positions(seed, n):
    """n asymmetric random boards (int8, +1 / -1 / 0), about 20 stones a side, and masks random over all 65 bytes - set on
    occupied cells as well"""
    rng = np.random.default_rng(seed)
    boards = rng.choice(np.array([1, -1, 0], np.int8), (n, 8, 8), p=[0.31, 0.31, 0.38])
    masks = (rng.random((n, 65)) < 0.4).astype(np.uint8)
    return boards, masks


def bitboards(boards):
    """(n, 8, 8) of +1 / -1 / 0 -> (player +1, player -1) as uint64, bit = 8 * row + col"""
    out = []
    for who in (1, -1):
        out.append(np.array([sum(1 << (8 * r + c) for r in range(8) for c in range(8) if b[r, c] == who) for b in boards],
                            dtype=np.uint64))
    return out


def embed_case():
    """The embedding tests' inputs: 11 positions, both turns, symmetry ids cycling through {0, 2, 6, 7}, and a table of 256
    pairwise distinct bf16 rows (8192 distinct bf16 numbers).  -> bb_p1, bb_p2, turn, sym, masks, table (float64)"""
    boards, masks = random_positions(9, 11)
    rng = np.random.default_rng(10)
    table = bf16_values(rng.permutation(np.arange(0x3000, 0x5000, dtype=np.uint16)).reshape(256, 32))
    bb1, bb2 = bitboards(boards)
    turn = np.where(np.arange(11) % 3 == 0, -1, 1).astype(np.int32)
    sym = np.array([0, 2, 6, 7], dtype=np.int32)[np.arange(11) % 4]
    return bb1, bb2, turn, sym, masks, table


def heads_draw(seed, sharp=1.0, n=37):
    """One heads weight set and n input maps whose reference is far from flat: unit-scale bf16 maps, board / pass
    weights about 0.15 N(0, 1) (times `sharp`), an aux_out[1] matrix that is bf16-representable (so the fp32 kernel
    and the matrix-core kernel, which takes it as bf16, share one reference).  -> (weights, policy_map, bottleneck)"""
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.standard_normal(s)                                         # noqa: E731
    w = dict(board_w=bf16_round(0.15 * sharp * g(256)), board_b=float(np.float32(0.1 * g())),
             pass_norm_w=1.0 + 0.1 * g(256), pass_fc_w=0.15 * sharp * g(256), pass_fc_b=float(np.float32(0.1 * g())),
             v_conv_w=0.25 * g(8, 8, 3, 3), v_bn_s=1.0 + 0.2 * g(8), v_bn_b=0.1 * g(8), v_fc_w=0.5 * g(3, 72),
             v_fc_b=0.1 * g(3), a_fc_w=bf16_round(g(512, 512) / math.sqrt(512.0)), a_fc_b=0.1 * g(512),
             a_norm_w=1.0 + 0.1 * g(512), a_out_w=0.08 * g(512), a_out_b=float(np.float32(0.05 * g())),
             aux_to_score=8.0, eps=1e-5)
    for k in HEADS_KEYS:                             # what the kernels are handed is fp32: the reference sees those values
        if isinstance(w[k], np.ndarray):
            w[k] = w[k].astype(np.float32).astype(np.float64)
    w["eps"] = float(np.float32(1e-5))
    pm = bf16_round(g(n, 8, 8, 256))
    h8 = bf16_round(g(n, 8, 8, 8))
    return w, pm, h8
