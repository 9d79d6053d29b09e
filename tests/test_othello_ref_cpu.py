"""The float64 references of tests/othello_ref.py, checked without a GPU.

Anchor: each reference equals az_net.OthelloNet in float64 (the module the kernels restate) to 1e-12, so a layout or
formula mistake in a reference shows here and not as a kernel "bug".  Sensitivity: the comparison functions that
test_othello_kernels_gpu.py applies to the kernels' outputs are fed deliberately wrong references and must reject every
one - the proof, for someone without a GPU, that those tests can fail.  Conditions: what the exact-arithmetic
convolution draws promise (exact fp32 partial sums, pre-SiLU values that sit on bf16 numbers, a thin midpoint band)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import othello_ref as R
import scenarios as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

ALL_KERNELS = R.ALL_KERNELS
_pool = R.conv_pool
_positions = R.random_positions
_embed_case = R.embed_case


@functools.lru_cache(maxsize=None)
def _net():
    """OthelloNet in float64 with BatchNorm statistics and output layers randomised as test_fused_gpu._rand_othello_net does"""
    from src.az_net import OthelloNet
    torch.manual_seed(5)
    net = OthelloNet(device="cpu").double()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.2); m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.7, 1.3); m.bias.normal_(0.0, 0.1)
        for m in (net.policy_head.board_out, net.policy_head.pass_fc, net.dual_head.value_out[-1], net.dual_head.aux_out[-1]):
            m.weight.normal_(0.0, 0.05); m.bias.normal_(0.0, 0.05)
    return net.eval()


def _affine(bn):
    f = lambda t: t.detach().double().numpy()                                     # noqa: E731
    scale = f(bn.weight) / np.sqrt(f(bn.running_var) + bn.eps)
    return scale, f(bn.bias) - f(bn.running_mean) * scale


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


# ---------------------------------------------------------------------------------------------
# anchor

@pytest.mark.parametrize("turn", [1, -1])
@pytest.mark.parametrize("sym", [0, 2, 6, 7])
def test_embed_ref_is_the_modules_embedding(sym, turn):
    net = _net()
    boards, masks = _positions(3, 6)
    assert (masks[:, :64].reshape(-1, 8, 8)[boards != 0] != 0).any()              # mask bits on occupied cells occur
    shown = np.stack([np.ascontiguousarray(R.SYMMETRIES[sym](b)) for b in boards])
    planes = np.stack([shown == turn, shown == -turn, np.ones_like(shown)], 1).astype(np.float64)
    with torch.no_grad():
        want = _nhwc(net.embed(torch.from_numpy(planes), torch.from_numpy(masks.astype(bool))))
        pos = net.pos_emb(net.orbit_map)
        kinds = torch.stack([net.piece_emb.weight[0], net.piece_emb.weight[1], net.legal_emb.weight[1], net.legal_emb.weight[0]])
        table = (pos[:, None, :] + kinds[None, :, :]).reshape(256, 32).numpy()    # fast_othello.py's table, unrounded
    bb1, bb2 = S.ot_bitboards(boards)
    assert np.array_equal(bb1, R.bitboards(boards)[0]) and np.array_equal(bb2, R.bitboards(boards)[1])
    n = len(boards)
    got = R.embed_ref(bb1, bb2, np.full(n, turn), np.full(n, sym), masks, table)
    assert got.shape == (n, 8, 8, 32)
    assert np.abs(got - want).max() < 1e-12


def test_heads_ref_is_the_modules_heads():
    net = _net()
    torch.manual_seed(1)
    hidden = torch.randn(5, 256, 10, 10, dtype=torch.float64)
    with torch.no_grad():
        pm, h8 = net.policy_head.stem(hidden), net.dual_head.stem(hidden)
        p0 = net.policy_head(hidden).exp().numpy()
        lv, aux = net.dual_head(hidden)
        w0 = lv.exp().numpy()
        u0 = (torch.atan(aux * float(net.aux_target_offset) / float(net.score_scale)) * (2.0 / np.pi)).numpy()   # `predict`
    p, w, u = R.heads_ref(_nhwc(pm), _nhwc(h8), R.heads_weights_of(net))
    assert p.shape == (5, 65) and w.shape == (5, 3) and u.shape == (5,)
    assert np.abs(p - p0).max() < 1e-12 and np.abs(w - w0).max() < 1e-12 and np.abs(u - u0).max() < 1e-12
    assert p0.std() > 1e-4 and w0.std() > 1e-3 and u0.std() > 1e-3               # not a comparison between constants


def test_conv_ref_without_roundings_is_the_modules_layers():
    net = _net()
    f = lambda t: t.detach().numpy()                                              # noqa: E731
    ones, zeros = np.ones(256), np.zeros(256)
    torch.manual_seed(2)
    with torch.no_grad():
        # the stem: 32 -> 256 on 8x8 with padding 2, BatchNorm behind it
        x = torch.randn(2, 32, 8, 8, dtype=torch.float64)
        want = net.stem[0:3](x)
        got, _ = R.conv_ref(_nhwc(x), f(net.stem[0].weight), None, _affine(net.stem[1]), None, 2, rounded=False)
        assert got.shape == (2, 10, 10, 256) and np.abs(got - _nhwc(want)).max() < 1e-12
        # a residual block: BatchNorm in FRONT of both convolutions, the block's input as residual of the second
        blk = net.stem[3]
        h = want
        y1 = torch.nn.functional.silu(blk.conv1(blk.norm1(h)))
        g1, _ = R.conv_ref(_nhwc(h), f(blk.conv1.weight), _affine(blk.norm1), (ones, zeros), None, 1, rounded=False)
        assert np.abs(g1 - _nhwc(y1)).max() < 1e-12
        g2, v2 = R.conv_ref(g1, f(blk.conv2.weight), _affine(blk.norm2), (ones, zeros), _nhwc(h), 1, rounded=False)
        assert np.abs(g2 - _nhwc(blk(h))).max() < 1e-12
        assert np.abs(v2 - _nhwc(blk.conv2(blk.norm2(y1)) + h)).max() < 1e-12     # the value next to the result: pre-SiLU
        # the policy stem: 10x10 without padding, then 8x8 with padding 1; the bottleneck
        ps = net.policy_head.stem
        hid = blk(h)
        p1 = ps[0:3](hid)
        g, _ = R.conv_ref(_nhwc(hid), f(ps[0].weight), None, _affine(ps[1]), None, 0, rounded=False)
        assert g.shape == (2, 8, 8, 256) and np.abs(g - _nhwc(p1)).max() < 1e-12
        g, _ = R.conv_ref(g, f(ps[4].weight), None, _affine(ps[5]), None, 1, rounded=False)
        assert np.abs(g - _nhwc(ps(hid))).max() < 1e-12
        ds = net.dual_head.stem
        s16, b16 = np.full(16, np.nan), np.full(16, np.nan)
        s16[:8], b16[:8] = _affine(ds[1])
        g, _ = R.conv_narrow_ref(_nhwc(hid), f(ds[0].weight), s16, b16, rounded=False)
        assert g.shape == (2, 8, 8, 8) and np.abs(g - _nhwc(ds(hid))).max() < 1e-12


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.00390625 + 2.0 ** -23, -1.01171875, 3.0e-3, 255.5, 0.0, 21.109375])
    want = torch.from_numpy(x).to(torch.float32).to(torch.bfloat16).double().numpy()   # exact in fp32: one rounding
    assert np.array_equal(R.bf16_round(x), want)
    assert R.bf16_round(1.00390625) == 1.0 and R.bf16_round(1.01171875) == 1.015625    # ties go to the even neighbour
    assert np.array_equal(R.bf16_values(R.bf16_bits(want)), want)
    rng = np.random.default_rng(0)
    y = rng.standard_normal(20000) * np.exp(rng.uniform(-8, 8, 20000))
    y32 = y.astype(np.float32).astype(np.float64)
    assert np.array_equal(R.bf16_round(y32), torch.from_numpy(y32).float().to(torch.bfloat16).double().numpy())


def test_pack_weight_ref_is_the_twins_packing():
    from src.fast_othello import pack_conv_weight
    rng = np.random.default_rng(4)
    for co, ci in ((256, 32), (16, 256), (256, 256)):
        w = R.bf16_round(rng.standard_normal((co, ci, 3, 3)))
        got = pack_conv_weight(torch.from_numpy(w)).double().numpy().reshape(9, ci // 32, co // 16, 64, 8)
        assert np.array_equal(got, R.pack_weight_ref(w))


# ---------------------------------------------------------------------------------------------
# conditions of the exact-arithmetic draws

@pytest.mark.parametrize("idx", range(len(ALL_KERNELS)))
def test_exact_draw_conditions(idx):
    d, y, v = _pool(idx)
    # every partial sum is exactly representable in fp32: operands and products are multiples of 2^-1, 2^-4, 2^-5, and the
    # sum of the products' magnitudes - a bound on every partial sum in every order - is below 2^24 * 2^-5
    cols = R.conv_columns(d["x"], d["pre"], d["pad"]).numpy()
    w = d["w"].reshape(d["w"].shape[0], -1)
    assert np.array_equal(cols * 2, np.rint(cols * 2)) and np.array_equal(w * 16, np.rint(w * 16))
    assert np.array_equal(R.bf16_round(cols), cols)                               # rounding point 1 changes nothing
    bound = (np.abs(cols) @ np.abs(w).T).max()
    assert bound * 32 < 2 ** 24, bound
    assert abs((w != 0).mean() - 0.25) < 0.02
    # the pre-SiLU values: at least 99 % are unchanged by their bf16 roundings (points 2 and 3)
    _, v_exact = R.conv_finish(R.conv_sums(torch.from_numpy(cols), d["w"]), d["post"], d["residual"], rounded=False)
    unchanged = (v == v_exact).mean()
    band = R.bf16_midpoint_band(R.silu64(v), v).mean()
    print("case %s: |z| <= %.4g, %.3f %% unchanged, %.3f %% in the midpoint band" % (ALL_KERNELS[idx], np.abs(v).max(), 100 * unchanged, 100 * band))
    assert unchanged >= 0.99, unchanged
    assert band <= 0.01, band
    assert np.abs(v).max() > 4.0 and len(np.unique(y)) > 200                      # and the outputs are not trivial
    m = R.conv_mismatch(R.bf16_bits(y), y, v)                                     # the reference passes its own comparison
    assert R.conv_ok(m) and m["excluded"] == band


def test_midpoint_band():
    lo, hi = 1.0, 1.0078125                                                       # neighbouring bf16 numbers, midpoint between
    mid = 0.5 * (lo + hi)
    v = np.array([2.0])
    width = (4 + 1.5 * 2.0) * 2.0 ** -23 * mid
    assert R.bf16_midpoint_band(np.array([mid]), v)[0] and R.bf16_midpoint_band(np.array([-mid]), -v)[0]
    assert R.bf16_midpoint_band(np.array([mid + 0.9 * width]), v)[0] and R.bf16_midpoint_band(np.array([mid - 0.9 * width]), v)[0]
    assert not R.bf16_midpoint_band(np.array([mid + 1.2 * width]), v)[0] and not R.bf16_midpoint_band(np.array([mid - 1.2 * width]), v)[0]
    assert not R.bf16_midpoint_band(np.array([lo, hi, 0.0]), np.array([2.0, 2.0, 0.0])).any()


# ---------------------------------------------------------------------------------------------
# sensitivity: the comparison functions reject wrong references

def _drop_term(idx, sample, token, tap):
    """The reference of pool kernel idx with ONE product term missing from one output element: output token `token` of
    `sample`, tap `tap`; the input and output channel are the first pair whose missing term still shows in the bf16
    result (a term can vanish in roundings 2-4; such a fault no test can see).  -> bit patterns of the wrong result"""
    d, y, v = _pool(idx)
    cols = R.conv_columns(d["x"][sample:sample + 1], d["pre"], d["pad"])
    acc = R.conv_sums(cols, d["w"])
    res = None if d["residual"] is None else d["residual"][sample:sample + 1]
    w = d["w"].reshape(d["w"].shape[0], -1)
    for ci in range(d["x"].shape[-1]):
        k = ci * 9 + tap
        x = float(cols[0, token, k])
        if x == 0.0:
            continue
        for co in np.nonzero(w[:, k])[0]:
            wrong = acc.copy()
            wrong[0, token, co] -= x * w[co, k]
            yw, _ = R.conv_finish(wrong, d["post"], res, rounded=True)
            if not np.array_equal(yw, y[sample:sample + 1]):
                full = y.copy()
                full[sample] = yw[0]
                return R.bf16_bits(full)
    raise AssertionError("no visible term at this place")


@pytest.mark.parametrize("idx", [0, 2, 4, 6])
def test_conv_comparison_rejects_a_dropped_term(idx):
    d, y, v = _pool(idx)
    ho = y.shape[1]
    nt = ho * ho
    first_real_tap = 4 * d["pad"]                     # the corner token's taps before (pad, pad) look at padding
    places = dict(corner=(1, 0, first_real_tap),     # the corner cell next to the zero padding
                  tail=(4, nt - 1, 0),               # the last token of the last token tile (tap 0 is a real cell at every padding)
                  middle=(2, nt // 2 + ho // 2, 8))
    for name, (sample, token, tap) in places.items():
        m = R.conv_mismatch(_drop_term(idx, sample, token, tap), y, v)
        assert not R.conv_ok(m), (ALL_KERNELS[idx], name, m)
        assert m["beyond_ulp"] + m["unequal_outside_band"] >= 1


@pytest.mark.parametrize("idx", [2, 6])
def test_conv_comparison_rejects_swapped_channel_chunks(idx):
    """two 8-channel chunks of the input swapped under one tap: one slot of the PERM permutation read for another"""
    d, y, v = _pool(idx)
    w = d["w"].copy()
    w[:, 8:16, 1, 2], w[:, 24:32, 1, 2] = d["w"][:, 24:32, 1, 2], d["w"][:, 8:16, 1, 2]
    yw, _ = R.conv_ref(d["x"], w, d["pre"], d["post"], d["residual"], d["pad"])
    assert not R.conv_ok(R.conv_mismatch(R.bf16_bits(yw), y, v))


def test_conv_comparison_rejects_nan_and_wrong_sign_of_nothing():
    d, y, v = _pool(0)
    bits = R.bf16_bits(y).copy()
    bits.reshape(-1)[7] = 0x7fc0                                                  # a prefill that was never overwritten
    assert R.conv_mismatch(bits, y, v)["beyond_ulp"] == 1
    zero = np.zeros((1, 1, 1, 2))
    assert R.conv_ok(R.conv_mismatch(np.array([0x8000, 0x0000], np.uint16), zero, zero))      # -0 equals +0


def test_embed_comparison_rejects_wrong_symmetry_and_side():
    bb1, bb2, turn, sym, masks, table = _embed_case()
    ref = R.embed_ref(bb1, bb2, turn, sym, masks, table)
    assert R.embed_mismatch(R.bf16_bits(ref), ref) == 0
    served = np.where(sym == 6, 7, sym)                                           # symmetry 6 served as 7
    assert R.embed_mismatch(R.bf16_bits(R.embed_ref(bb1, bb2, turn, served, masks, table)), ref) > 0
    swapped = R.embed_ref(np.where(turn < 0, bb2, bb1), np.where(turn < 0, bb1, bb2), turn, sym, masks, table)
    assert (turn < 0).any() and R.embed_mismatch(R.bf16_bits(swapped), ref) > 0   # own / opponent swapped for turn = -1
    # each of the four kinds occurs, and a mask bit on an occupied cell is ignored
    kinds = R.embed_kinds(bb1, bb2, turn, sym, masks)
    assert all((kinds == k).sum() > 20 for k in range(4))
    assert ((kinds < 2) & (masks[:, :64].reshape(-1, 8, 8) != 0)).sum() > 20


@functools.lru_cache(maxsize=None)
def _heads_case(sharp):
    w, pm, h8 = R.heads_draw(21, sharp=sharp, n=9)
    ref = R.heads_ref(pm, h8, w)
    e32 = R.heads_errors(R.heads_ref(pm, h8, w, dtype=torch.float32), ref)
    return w, pm, h8, ref, e32


@pytest.mark.parametrize("sharp", [1.0, 25.0])
def test_heads_comparison_rejects_wrong_layouts(sharp):
    w, pm, h8, ref, e32 = _heads_case(sharp)
    print("E32 (probs, wdl, utility) at sharp = %g:" % sharp, e32)
    assert R.heads_problems(ref, ref, e32) == []
    assert R.heads_problems(R.heads_ref(pm, h8, w, dtype=torch.float32), ref, e32) == []
    p, v, u = ref
    a = int(p[0, :64].argmax()); b = (a + 9) % 64
    swapped = p.copy(); swapped[:, [a, b]] = p[:, [b, a]]                          # two squares of the policy swapped
    assert R.heads_problems((swapped, v, u), ref, e32)
    assert R.heads_problems((np.roll(p, 1, axis=1), v, u), ref, e32)              # the pass logit placed at index 0
    wrong = dict(w); wrong["a_fc_w"] = w["a_fc_w"].reshape(512, 8, 64).transpose(0, 2, 1).reshape(512, 512).copy()
    assert R.heads_problems(R.heads_ref(pm, h8, wrong), ref, e32)                 # the auxiliary Linear fed channel-major weights in NHWC order
    t = lambda a: torch.from_numpy(a)                                             # noqa: E731
    wt = {k: torch.as_tensor(np.asarray(w[k])) for k in R.HEADS_KEYS}
    assert np.array_equal(R.value_ref(t(h8), wt).numpy(), v)
    assert R.heads_problems((p, R.value_ref(t(h8), wt, stride=1).numpy(), u), ref, e32)          # stride 1 offsets
    nan = p.copy(); nan[3, 64] = np.nan
    assert R.heads_problems((nan, v, u), ref, e32)
    off = p.copy(); off[:, 0] += 2e-5                                             # rows that do not sum to 1
    assert any("sum" in s for s in R.heads_problems((off, v, u), ref, e32))


@pytest.mark.parametrize("sharp", [1.0, 25.0])
def test_heads_draw_is_far_from_flat(sharp):
    w, pm, h8, ref, e32 = _heads_case(sharp)
    p, v, u = ref
    assert (p.max(1) / p.min(1)).min() > 100 and v.std() > 0.1 and u.std() > 0.2
    assert np.array_equal(R.bf16_round(w["a_fc_w"]), w["a_fc_w"]) and np.array_equal(R.bf16_round(w["board_w"]), w["board_w"])
    if sharp > 1:
        logits = np.log(np.maximum(p, 1e-300))
        assert (logits.max(1) - logits.min(1)).max() > 200                        # a logit range of a few hundred
