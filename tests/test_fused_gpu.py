"""GPU tests of the device-resident loop (fused.py), the network port and the self-play driver.

The fused path uses the engine's device generator, so bit-exact comparisons use the
configuration that consumes no randomness (use_symmetry=False, alpha<=0, eps=0) and the
integer-hash evaluator; there the fused path must equal the CPU oracle bit for bit.
"""
import os
import sys

import numpy as np
import pytest

import scenarios as S
from oracle import oracle as O
from test_oracle_golden import bits, load, load_split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import MCTS_cpp, fused, hash_eval, az_net, selfplay
    return dict(torch=torch, W=MCTS_cpp, F=fused, H=hash_eval, N=az_net, SP=selfplay)


def _planes(boards, turns):
    return np.stack([(boards == turns[:, None, None]), (boards == -turns[:, None, None]),
                     np.ones_like(boards) * turns[:, None, None]], 1).astype(np.float32)


def test_device_hash_evaluator_equals_numpy_twin(env):
    rng = np.random.default_rng(0)
    b, t = S.random_openings(rng, 500, 36)
    mask = b[:, 0, :] == 0
    p, w, ml = env["H"].HashEvaluator("cuda").predict(_planes(b, t), mask)
    p2, w2, ml2 = S.hash_eval(b, t)
    assert np.array_equal(bits(p), bits(p2 * mask)) and np.array_equal(bits(w), bits(w2))
    assert np.array_equal(bits(ml[:, 0]), bits(ml2))


def _oracle_plies(cfg, boards, turns, n, K, plies):
    o = O.BatchedMCTS_Connect4(boards.shape[0])
    S.apply_cfg(o, cfg)
    return S.play_plies(o, boards, turns, n, K, plies)


def _fused_plies(env, cfg, boards, turns, n, K, plies, graph):
    """graph: True = hipGraph replay of the Python loop, False = the Python loop issued call by call,
    "native" = the whole schedule from native code (az_mcts_dev_search with the hash model)."""
    os.environ["AZ_FUSED_GRAPH"] = "1" if graph is True else "0"
    os.environ["AZ_FUSED_NATIVE"] = "1" if graph == "native" else "0"
    try:
        B = boards.shape[0]
        w = env["W"].BatchedMCTS(B, c_init=cfg["c_init"], c_base=cfg["c_base"], alpha=cfg["dirichlet_alpha"],
                                 n_playout=n, noise_epsilon=cfg["noise_epsilon"], fpu_reduction=cfg["fpu_reduction"],
                                 use_symmetry=cfg["use_symmetry"], mlh_slope=cfg["mlh_slope"], mlh_cap=cfg["mlh_cap"],
                                 value_decay=cfg["value_decay"])
        w.mcts.config.vl_count = cfg["vl_count"]
        net = env["H"].HashEvaluator("cuda")
        boards, turns = boards.copy(), turns.copy()
        counts, stats = [], []
        for _ in range(plies):
            w.batch_playout(net, boards, turns, vl_batch=K)
            assert w._fused is not None, "the device-resident path did not engage"
            c = w.get_visits_count().astype(np.int32)
            counts.append(c); stats.append(np.array(w.mcts.get_all_root_stats()))
            acts = np.argmax(c, 1).astype(np.int32)
            w.prune_roots(acts)
            for i in range(B):
                if not S.np_done(boards[i]) and boards[i][0, acts[i]] == 0:
                    S.np_drop(boards[i], int(acts[i]), int(turns[i])); turns[i] = -turns[i]
        return np.stack(counts), np.stack(stats)
    finally:
        os.environ.pop("AZ_FUSED_GRAPH", None)
        os.environ.pop("AZ_FUSED_NATIVE", None)


@pytest.mark.parametrize("graph", [False, True, "native"])
@pytest.mark.parametrize("n,K", [(50, 4), (200, 4), (37, 1), (66, 8)])
def test_fused_path_bit_exact_vs_oracle(env, graph, n, K):
    rng = np.random.default_rng(n * 10 + K)
    boards, turns = S.random_openings(rng, 96, 12)
    cfg = dict(S.DET_CFG, c_base=5.0 * n)
    ref = _oracle_plies(cfg, boards, turns, n, K, 4)
    counts, stats = _fused_plies(env, cfg, boards, turns, n, K, 4, graph)
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(bits(stats), bits(ref["stats"]))


def test_fused_value_decay_and_eps_without_alpha(env):
    rng = np.random.default_rng(77)
    boards, turns = S.random_openings(rng, 64, 10)
    cfg = dict(S.DET_CFG, value_decay=0.97, noise_epsilon=0.25, vl_count=2)
    ref = _oracle_plies(cfg, boards, turns, 80, 4, 3)
    counts, stats = _fused_plies(env, cfg, boards, turns, 80, 4, 3, False)
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(bits(stats), bits(ref["stats"]))


def test_network_port_matches_reference_outputs_g7(env):
    """G7: fp32 on the GPU within 1e-4 of the reference's CPU fp32 outputs; bf16 autocast
    (what self-play uses, Network.py:275) within 5e-2 max / 5e-3 mean on probabilities - bf16
    has 8 significant bits and the trained heads are sharp.  Search parity never goes through
    the network."""
    torch = env["torch"]
    g = load("g7_network"); wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    planes = _planes(g["boards"], g["turns"]); masks = g["masks"].astype(bool)
    p, w, ml = net.predict(planes, masks)            # random init, bf16 autocast
    assert np.abs(p - g["init_probs"]).max() < 2e-2 and np.abs(w - g["init_wdl"]).max() < 2e-2
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    p, w, ml = net.predict(planes, masks)
    assert np.abs(p - g["ckpt_probs"]).max() < 5e-2 and np.abs(p - g["ckpt_probs"]).mean() < 5e-3
    assert np.abs(w - g["ckpt_wdl"]).max() < 5e-2 and np.abs(w - g["ckpt_wdl"]).mean() < 5e-3
    assert np.abs(ml - g["ckpt_ml"]).max() < 42 * 5e-2
    with torch.no_grad():
        lp, lv, st = net(torch.from_numpy(planes).cuda(), action_mask=torch.from_numpy(masks).cuda())
    assert np.abs(lp.exp().cpu().numpy() - g["ckpt_probs"]).max() < 1e-4
    assert np.abs(lv.exp().cpu().numpy() - g["ckpt_wdl"]).max() < 1e-4
    assert np.abs(st.cpu().numpy() - g["ckpt_steps"]).max() < 1e-4


def test_fast_inference_twin_g7(env):
    """fast_net.py computes the reference forward: fp32 build within 1e-4 of the reference's
    CPU outputs, bf16 build within the same band as the reference's own bf16 autocast."""
    torch = env["torch"]
    from src.fast_net import FastConnect4Net
    g = load("g7_network"); wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    planes = _planes(g["boards"], g["turns"]); masks = g["masks"].astype(bool)
    p, w, ml = FastConnect4Net.from_module(net, dtype=torch.float32).predict(planes, masks)
    assert np.abs(p - g["ckpt_probs"]).max() < 1e-4 and np.abs(w - g["ckpt_wdl"]).max() < 1e-4
    assert np.abs(ml - g["ckpt_ml"]).max() < 1e-2
    # bf16: the yardstick is the reference's OWN bf16 path on the same inputs (the module under autocast,
    # Network.py:275): measured on MI355X it is 1.6e-2 max / 8.9e-4 mean off its fp32 outputs on the policy
    # and 3.4e-2 / 1.4e-3 on WDL; the HIP twin 2.3e-2 / 7.7e-4 and 4.5e-2 / 1.3e-3, arg-max move identical
    # to fp32 on all 256 positions.  Bounds: means no worse than 1.25x the module's, maxima within 1.5x of
    # its worst (3.4e-2), i.e. 5e-2 - not the 8e-2 of round 1.
    pm, wm, _ = net.predict(planes, masks)
    p, w, ml = FastConnect4Net.from_module(net).predict(planes, masks)
    e = dict(p_max=np.abs(p - g["ckpt_probs"]).max(), p_mean=np.abs(p - g["ckpt_probs"]).mean(),
             w_max=np.abs(w - g["ckpt_wdl"]).max(), w_mean=np.abs(w - g["ckpt_wdl"]).mean(),
             ref_p_mean=np.abs(pm - g["ckpt_probs"]).mean(), ref_w_mean=np.abs(wm - g["ckpt_wdl"]).mean(),
             ref_p_max=np.abs(pm - g["ckpt_probs"]).max(), ref_w_max=np.abs(wm - g["ckpt_wdl"]).max(),
             argmax=(p.argmax(1) == g["ckpt_probs"].argmax(1)).mean())
    print("twin vs G7:", {k: round(float(v), 5) for k, v in e.items()})
    assert e["p_max"] < 3e-2 and e["w_max"] < 5e-2, e
    assert e["p_mean"] < 1.1 * e["ref_p_mean"] + 1e-4 and e["w_mean"] < 1.1 * e["ref_w_mean"] + 1e-4, e
    assert e["argmax"] >= 0.99, e
    # The whole error DISTRIBUTION of the twin sits at or below the module's own bf16 error: median, 90th and 99th
    # percentile within 1.1x (measured: 1.2e-4 / 2.5e-3 / 8.0e-3 against the module's 1.3e-4 / 2.9e-3 / 8.2e-3 on the
    # policy, 5.6e-4 / 3.4e-3 / 9.1e-3 against 5.4e-4 / 3.8e-3 / 1.05e-2 on WDL).  The maxima above are single values
    # out of 1792 and 768 - one position each - and move by tens of percent with ANY change of evaluation order: the
    # same architecture on plain PyTorch bf16 operations lands on 2.3e-2 / 4.0e-2 (tools/probe_twin_error.py, which also
    # shows that the heads add 3e-3 / 7e-3 and the body - bf16 activations between layers, as in the module - the rest).
    for q in (0.5, 0.9, 0.99):
        for mine, ref, want, tag in ((p, pm, g["ckpt_probs"], "policy"), (w, wm, g["ckpt_wdl"], "wdl")):
            a, b = np.quantile(np.abs(mine - want), q), np.quantile(np.abs(ref - want), q)
            assert a <= 1.1 * b + 1e-4, (tag, q, a, b)
    # weight updates on the source module are picked up by the fused path
    w_ = env["W"].BatchedMCTS(8, 1.4, 100, 0.0, 9, noise_epsilon=0.0, use_symmetry=False)
    b, t = S.random_openings(np.random.default_rng(1), 8, 4)
    w_.batch_playout(net, b, t, vl_batch=4)
    first = w_._fused.fast
    with torch.no_grad():
        net.dual_head.value_out.bias.add_(1.0)
    w_.batch_playout(net, b, t, vl_batch=4)
    assert w_._fused.fast is not first


def test_glue_kernels_match_torch(env):
    """nn_kernels.hip (the token embedding, the head pooling) against the torch ops they replace (same bf16 inputs,
    fp32 maths)."""
    torch = env["torch"]
    import ctypes as C
    import torch.nn.functional as TF
    from src.fast_net import glue
    L = glue()
    assert L is not None
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    bf = torch.bfloat16
    B = 333
    rnd = lambda *sh: torch.randn(*sh, device="cuda", generator=g)    # noqa: E731

    def close(a, b, tol=2e-2):
        d = (a.float() - b.float()).abs().max().item()
        assert d < tol, d

    # embed
    feats = (torch.rand(B, 3, 6, 7, device="cuda", generator=g) > 0.6).float()
    eo, ep, pos = rnd(32).to(bf), rnd(32).to(bf), rnd(42, 32).to(bf)
    tok = torch.empty(B, 42, 32, dtype=bf, device="cuda")
    L.az_nn_embed(feats.data_ptr(), eo.data_ptr(), ep.data_ptr(), pos.data_ptr(), tok.data_ptr(), B, 32, None, None, s)
    want = pos.float() + feats[:, 0].reshape(B, 42, 1) * eo.float() + feats[:, 1].reshape(B, 42, 1) * ep.float()
    close(tok, want)
    # head pooling (x: the final tokens)
    x = (rnd(B, 42, 64) * 2 + 0.5).to(bf)
    pw, gw = rnd(64).to(bf), (rnd(64) * 0.3).to(bf)
    col = torch.empty(B, 7, 64, dtype=bf, device="cuda"); mean = torch.empty(B, 64, dtype=bf, device="cuda")
    L.az_nn_heads_prep(x.data_ptr(), pw.data_ptr(), gw.data_ptr(), 0.25, col.data_ptr(), mean.data_ptr(), B, 1e-5, s)
    pn = TF.rms_norm(x.float(), (64,), pw.float(), 1e-5).to(bf).float().view(B, 6, 7, 64)
    sc = (pn * gw.float()).sum(-1) + 0.25
    wts = torch.softmax(sc, dim=1)
    close(col, (wts.unsqueeze(-1) * pn).sum(1), 6e-2)
    close(mean, x.float().mean(1), 2e-2)
    torch.cuda.synchronize()


def test_mfma_conv_block_matches_torch(env):
    """nn_conv.hip (implicit-GEMM 3x3 convolution on MFMA with fused GroupNorm / bias / SiLU /
    residual) against the same block in torch, fp32 maths on the same bf16 inputs."""
    torch = env["torch"]
    import ctypes as C
    import torch.nn.functional as TF
    from src.fast_net import glue
    L = glue()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    bf = torch.bfloat16
    for B in (1, 8, 37, 1024, 6150):             # one sample, full tiles, ragged tails, several tiles per workgroup
        for cin, norm, resid in ((64, True, True), (64, True, False), (32, False, False)):
            x = (torch.randn(B, 42, cin, device="cuda", generator=g) * 1.5 + 0.3).to(bf)
            w = (torch.randn(64, cin, 3, 3, device="cuda", generator=g) / (3.0 * cin ** 0.5)).to(bf)
            w_ohwi = w.contiguous(memory_format=torch.channels_last)
            bias = torch.randn(64, device="cuda", generator=g).to(bf)
            ga = (1 + 0.2 * torch.randn(cin, device="cuda", generator=g)).to(bf)
            be = (0.2 * torch.randn(cin, device="cuda", generator=g)).to(bf)
            y = torch.full((B, 42, 64), float("nan"), device="cuda").to(bf)
            rc = L.az_nn_conv_block(x.data_ptr(), cin, w_ohwi.data_ptr(), bias.data_ptr(),
                                    ga.data_ptr() if norm else None, be.data_ptr() if norm else None,
                                    1 if resid else 0, y.data_ptr(), B, 1e-5, None, s)
            assert rc == 0
            img = x.float().view(B, 6, 7, cin).permute(0, 3, 1, 2)
            h = TF.group_norm(img, 1, ga.float(), be.float(), 1e-5).to(bf).float() if norm else img
            ref = TF.silu(TF.conv2d(h, w.float(), bias.float(), padding=1))
            if resid:
                ref = ref + img
            ref = ref.permute(0, 2, 3, 1).reshape(B, 42, 64)
            torch.cuda.synchronize()
            err = (y.float() - ref).abs()
            assert torch.isfinite(y.float()).all()
            assert err.max().item() < 6e-2 and err.mean().item() < 4e-3, (B, cin, err.max().item(), err.mean().item())


def test_stem_with_fused_embedding_equals_two_kernels(env):
    """az_nn_stem_embed against az_nn_embed followed by the stem az_nn_conv_block: same arithmetic,
    bit-identical output; also through a gather list (compact batch)."""
    torch = env["torch"]
    import ctypes as C
    from src.fast_net import FastConnect4Net, glue
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    fast = FastConnect4Net.from_module(net)
    L = glue()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = load("g7_network")
    planes = torch.from_numpy(_planes(g["boards"], g["turns"])).cuda().float().contiguous()
    for B, gather in ((planes.shape[0], None), (100, torch.randperm(planes.shape[0], device="cuda")[:100].to(torch.int32))):
        gp = None if gather is None else gather.data_ptr()
        t0 = torch.empty((B, 42, 32), dtype=torch.bfloat16, device="cuda")
        y0 = torch.empty((B, 42, 64), dtype=torch.bfloat16, device="cuda")
        y1 = torch.empty_like(y0)
        assert L.az_nn_embed(planes.data_ptr(), fast.emb_own.data_ptr(), fast.emb_opp.data_ptr(), fast.pos.data_ptr(),
                             t0.data_ptr(), B, 32, gp, None, s) == 0
        assert L.az_nn_conv_block(t0.data_ptr(), 32, fast.stem_w.data_ptr(), fast.stem_b.data_ptr(), None, None, 0,
                                  y0.data_ptr(), B, 1e-5, None, s) == 0
        assert L.az_nn_stem_embed(planes.data_ptr(), fast.emb_own.data_ptr(), fast.emb_opp.data_ptr(), fast.pos.data_ptr(),
                                  fast.stem_w.data_ptr(), fast.stem_b.data_ptr(), y1.data_ptr(), B, gp, None, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))


def test_mfma_attention_block_matches_torch(env):
    """nn_attn.hip (RMSNorm -> QKV+gate projection -> per-head RMSNorm -> softmax attention ->
    gate -> output projection + residual, all on MFMA in registers) against torch fp32."""
    torch = env["torch"]
    import ctypes as C
    import torch.nn.functional as TF
    from src.fast_net import glue
    L = glue()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    bf = torch.bfloat16
    rnd = lambda *sh: torch.randn(*sh, device="cuda", generator=g)     # noqa: E731
    pre = (1 + 0.1 * rnd(64)).to(bf); qn0 = (1 + 0.1 * rnd(16)).to(bf); kn = (1 + 0.1 * rnd(16)).to(bf)
    wqkvg = (rnd(196, 64) / 8).to(bf); wo = (rnd(64, 64) / 8).to(bf)
    # 9001: more than one sample per wavefront of the grid, ragged.  q-norm weights x6: sharp
    # softmaxes, still inside the bound under which the kernel skips the running maximum;
    # x40: outside it (scores up to ~2^300 in the kernel's log2 units), the max-subtracting path
    for B, qscale in ((1, 1.0), (5, 1.0), (4096, 1.0), (9001, 1.0), (300, 6.0), (300, 40.0)):
        qn = (qn0.float() * qscale).to(bf)
        x = (rnd(B, 42, 64) * 1.2).to(bf)
        y = torch.full_like(x, float("nan"))
        assert L.az_nn_attn_block(x.data_ptr(), pre.data_ptr(), wqkvg.data_ptr(), qn.data_ptr(), kn.data_ptr(),
                                  wo.data_ptr(), y.data_ptr(), B, 1e-5, None, s) == 0
        xf = x.float()
        h = TF.rms_norm(xf, (64,), pre.float(), 1e-5).to(bf).float()
        proj = h @ wqkvg.float().t()
        q, k, v = proj[..., :192].view(B, 42, 3, 4, 16).unbind(2)
        gate = torch.sigmoid(proj[..., 192:])
        # q, k, v are MFMA operands in the kernel, i.e. bf16 (as under the reference's autocast);
        # sharp softmaxes magnify that rounding, so the comparison rounds them at the same place
        q = TF.rms_norm(q, (16,), qn.float(), 1e-5).to(bf).float().transpose(1, 2)
        k = TF.rms_norm(k, (16,), kn.float(), 1e-5).to(bf).float().transpose(1, 2)
        a = TF.scaled_dot_product_attention(q, k, v.to(bf).float().transpose(1, 2))
        a = a * gate.transpose(1, 2).unsqueeze(-1)
        ref = a.transpose(1, 2).reshape(B, 42, 64) @ wo.float().t() + xf
        torch.cuda.synchronize()
        err = (y.float() - ref).abs()
        assert torch.isfinite(y.float()).all()
        assert err.max().item() < (8e-2 if qscale == 1.0 else 0.2) and err.mean().item() < 6e-3, (B, qscale, err.max().item(), err.mean().item())


def test_fused_heads_kernel_matches_torch_heads(env):
    """az_nn_heads (nn_heads.hip) against the PyTorch heads of the same twin on random final
    tokens, with the reference checkpoint's trained weights (non-zero output layers, so every
    stage matters); ragged batch sizes exercise the grid-stride loop and its prefetch."""
    torch = env["torch"]
    import ctypes as C
    from src.fast_net import FastConnect4Net, glue
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    gen = torch.Generator(device="cuda").manual_seed(3)
    fast = FastConnect4Net.from_module(net)
    assert fast.hip
    L = glue()
    for B in (1, 3, 777, 4099):
        tok = (torch.randn((B, 42, 64), device="cuda", generator=gen) * 1.5).to(torch.bfloat16)
        mask = torch.rand((B, 7), device="cuda", generator=gen) > 0.25
        mask[:, 3] = True
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lp, lv, st = fast._heads_hip(tok, mask, B, L, s)
        probs = torch.empty((B, 7), dtype=torch.float32, device="cuda")
        wdl = torch.empty((B, 3), dtype=torch.float32, device="cuda")
        ml = torch.empty((B,), dtype=torch.float32, device="cuda")
        m8 = mask.to(torch.uint8).contiguous()
        assert L.az_nn_heads(tok.data_ptr(), C.byref(fast._heads_w), m8.data_ptr(), probs.data_ptr(), wdl.data_ptr(),
                             ml.data_ptr(), B, 1e-5, None, None, s) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(probs).all() and torch.isfinite(wdl).all() and torch.isfinite(ml).all()
        assert (probs[~mask] == 0).all()
        assert (probs.sum(1) - 1).abs().max().item() < 1e-5 and (wdl.sum(1) - 1).abs().max().item() < 1e-5
        ep, ew, em = (probs - lp.exp()).abs(), (wdl - lv.exp()).abs(), (ml - st * 42.0).abs()
        assert ep.max().item() < 3e-2 and ep.mean().item() < 2e-3, (B, ep.max().item(), ep.mean().item())
        assert ew.max().item() < 3e-2 and ew.mean().item() < 2e-3, (B, ew.max().item(), ew.mean().item())
        assert em.max().item() < 0.5, (B, em.max().item())
    # no mask = every column legal
    assert L.az_nn_heads(tok.data_ptr(), C.byref(fast._heads_w), None, probs.data_ptr(), wdl.data_ptr(),
                         ml.data_ptr(), B, 1e-5, None, None, s) == 0
    lp, _, _ = fast._heads_hip(tok, None, B, L, s)
    torch.cuda.synchronize()
    assert (probs - lp.exp()).abs().max().item() < 3e-2


def test_fast_net_hip_path_equals_torch_path(env):
    torch = env["torch"]
    from src.fast_net import FastConnect4Net
    g = load("g7_network"); wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    planes = _planes(g["boards"], g["turns"]); masks = g["masks"].astype(bool)
    fast = FastConnect4Net.from_module(net)
    assert fast.hip
    p1, w1, m1 = fast.predict(planes, masks)
    fast.hip = False
    p2, w2, m2 = fast.predict(planes, masks)
    assert np.abs(p1 - p2).max() < 4e-2 and np.abs(w1 - w2).max() < 5e-2 and np.abs(m1 - m2).max() < 2.0
    assert np.abs(p1 - g["ckpt_probs"]).max() < 3e-2 and np.abs(p1 - g["ckpt_probs"]).mean() < 1.5e-3
    assert np.abs(w1 - g["ckpt_wdl"]).max() < 5e-2 and np.abs(w1 - g["ckpt_wdl"]).mean() < 2.5e-3


def test_fused_with_network_statistical_agreement(env):
    """Same network, fused path vs host path: bf16 GEMMs are batch-shape dependent, so compare
    what must hold regardless - simulation budget, probability mass, and near-equal root Q."""
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    rng = np.random.default_rng(5)
    boards, turns = S.random_openings(rng, 128, 8)
    res = []
    for fused in (True, False):
        w = env["W"].BatchedMCTS(128, 1.4, 1000, 0.0, 200, noise_epsilon=0.0, fpu_reduction=0.2,
                                 use_symmetry=False, mlh_slope=0.1)
        w.batch_playout(net, boards, turns, vl_batch=4, fused=fused)
        assert (w._fused is not None) == fused
        res.append((w.get_visits_count(), np.array(w.mcts.get_all_root_stats())))
    (c1, s1), (c2, s2) = res
    assert (s1[:, 0] == 200).all() and (s2[:, 0] == 200).all()
    assert (c1.sum(1) == 199).all() and (c2.sum(1) == 199).all()
    q_gap = float(np.abs(s1[:, 1] - s2[:, 1]).mean())
    agree = float((np.argmax(c1, 1) == np.argmax(c2, 1)).mean())
    dist = float(np.abs(c1 / 199.0 - c2 / 199.0).sum(1).mean()) / 2          # total-variation distance of the visit distributions
    print("fused vs host with the network: root-Q gap %.4f, arg-max agreement %.3f, TV distance %.4f" % (q_gap, agree, dist))
    assert q_gap < 0.02 and agree > 0.95 and dist < 0.03       # measured on MI355X: 0.0076, 1.000, 0.0070


def test_device_transposition_table_leaves_the_search_unchanged(env):
    """SURVEY 8f row f2.  The evaluator kernels compute each row independently of its batch, so a
    cached output is bit-identical to a fresh one and the search must not change at all: same
    visit counts and root statistics with and without the table, zero mismatches in verify mode
    (every leaf evaluated densely as well and compared with what the table path produced), and a
    second search from the same roots is served almost entirely from the table."""
    torch = env["torch"]
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    rng = np.random.default_rng(9)
    boards, turns = S.random_openings(rng, 256, 9)
    boards[:64] = boards[0]; turns[:64] = turns[0]            # many trees on one position: transpositions across trees
    res = []
    for table in (False, True):
        w = env["W"].BatchedMCTS(256, 1.4, 400, 0.0, 80, noise_epsilon=0.25, fpu_reduction=0.2,
                                 use_symmetry=True, mlh_slope=0.1)
        w.seed(7)
        fs = w._fused_runner(net, True)
        if table:
            fs.enable_table(12, verify=True)                  # 4096 entries: replacement happens too
        w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
        res.append((w.get_visits_count().copy(), np.array(w.mcts.get_all_root_stats()).copy()))
        if table:
            st = fs.table_stats()
            assert st["mismatches"] == 0 and st["hits"] > 0 and st["lookups"] >= st["hits"] + st["inserts"] - 1
            assert st["replaced"] > 0
            first = st
            # the same roots again from fresh trees: nearly everything is known (capacity permitting)
            fs.enable_table(18, verify=True)
            for rep in range(2):
                for i in range(256):
                    w.mcts.reset_env(i)
                w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
                st = fs.table_stats()
                assert st["mismatches"] == 0
            assert st["hit_rate"] > 0.4, st
    (c0, s0), (c1, s1) = res
    assert np.array_equal(c0, c1)
    assert np.array_equal(bits(s0), bits(s1))
    # the wrapper's cache_size reaches the device table when the caller asks for the fused path
    w = env["W"].BatchedMCTS(256, 1.4, 400, 0.0, 80, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True,
                             mlh_slope=0.1, cache_size=3000)
    w.seed(7)
    w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    assert w._fused is not None and w._fused.table_log2 == 12 and w._fused.table_stats()["hits"] > 0
    assert np.array_equal(w.get_visits_count(), c0)
    w.refresh_cache(net)
    # the plain (no virtual loss) loop goes through the table as well
    plain = []
    for table in (False, True):
        w = env["W"].BatchedMCTS(256, 1.4, 400, 0.0, 24, noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False,
                                 mlh_slope=0.1)
        fs = w._fused_runner(net, True)
        if table:
            fs.enable_table(14, verify=True)
        w.batch_playout(net, boards, turns, vl_batch=1, fused=True)
        plain.append((w.get_visits_count().copy(), np.array(w.mcts.get_all_root_stats()).copy()))
        if table:
            st = fs.table_stats()
            assert st["mismatches"] == 0 and st["hits"] > 0
    assert np.array_equal(plain[0][0], plain[1][0]) and np.array_equal(bits(plain[0][1]), bits(plain[1][1]))


def test_native_search_call_equals_python_loop(env, monkeypatch):
    """az_mcts_dev_search (the whole schedule with az_nn_model_forward inside, one C call) against
    the Python loop over the single entry points: same visit counts and root statistics bit for
    bit, with virtual-loss batches, with the plain loop, and through the transposition table."""
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    rng = np.random.default_rng(21)
    boards, turns = S.random_openings(rng, 600, 11)      # > 512 trees: below that the loop is a graph replay
    for K, n_playout, table in ((4, 83, 0), (1, 17, 0), (4, 60, 12), (3, 41, 0)):
        res = []
        for native in ("1", "0"):
            monkeypatch.setenv("AZ_FUSED_NATIVE", native)
            w = env["W"].BatchedMCTS(600, 1.4, 400, 0.3, n_playout, noise_epsilon=0.25, fpu_reduction=0.2,
                                     use_symmetry=True, mlh_slope=0.1)
            w.seed(5)
            fs = w._fused_runner(net, True)
            if table:
                fs.enable_table(table)
            for rep in range(2):                                      # second search re-uses the trees
                w.batch_playout(net, boards, turns, vl_batch=K, fused=True)
            assert (fs._native_model() is not None) == (native == "1")
            res.append((w.get_visits_count().copy(), np.array(w.mcts.get_all_root_stats()).copy(),
                        env["F"].counters(fs.h)))
            if table:
                assert fs.table_stats()["hits"] > 0
        (c0, s0, k0), (c1, s1, k1) = res
        assert c0.sum() > 0 and np.array_equal(c0, c1), (K, n_playout, table)
        assert np.array_equal(bits(s0), bits(s1))
        assert k0 == k1


@pytest.mark.parametrize("native", ["1", "0"])
def test_time_budgeted_search_stays_on_the_device(env, monkeypatch, native):
    """`batch_playout(..., time_budget=...)` (MCTS_cpp.py:70-87,194-209,252-264 of the reference: wall-clock check and
    top-2 early exit between iterations) on the fused path, native loop and Python loop: with a generous budget the
    search runs its n_playout simulations and equals the n_playout-bounded search bit for bit (same launches, so the
    same device draws); with a small one it stops early, on a whole iteration, with no in-flight visit left."""
    monkeypatch.setenv("AZ_FUSED_NATIVE", native)
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    rng = np.random.default_rng(31)
    boards, turns = S.random_openings(rng, 700, 10)
    net = env["H"].HashEvaluator("cuda")

    def make():
        w = env["W"].BatchedMCTS(700, 1.4, 1000, 0.3, 200, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True)
        w.seed(8)
        return w
    for K in (4, 1):
        a, b = make(), make()
        a.batch_playout(net, boards, turns, vl_batch=K, fused=True)
        b.batch_playout(net, boards, turns, vl_batch=K, fused=True, time_budget=600.0)
        assert b.last_playouts == 200 and b._fused is not None
        assert np.array_equal(a.get_visits_count(), b.get_visits_count())
        assert np.array_equal(bits(np.array(a.mcts.get_all_root_stats())), bits(np.array(b.mcts.get_all_root_stats())))
    # a budget that ends the search long before n_playout = 10^6 simulations
    c = env["W"].BatchedMCTS(700, 1.4, 1000, 0.3, 1000000, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True)
    c.seed(8)
    import time
    t0 = time.perf_counter()
    c.batch_playout(net, boards, turns, vl_batch=4, fused=True, time_budget=0.25)
    dt = time.perf_counter() - t0
    done = c.last_playouts
    assert 1 <= done < 1000000 and (done - 1) % 4 == 0, done            # the warm-up simulation + whole batches of four
    assert dt < 0.25 * 1.6 + 0.3, dt                                   # at most about one chunk (a tenth of the budget) late
    st = np.array(c.mcts.get_all_root_stats())
    live = np.array([not S.np_done(b) for b in boards])
    assert (st[live, 0] == done).all() and (c.get_visits_count()[live].sum(1) == done - 1).all()
    c.mcts.remove_all_vl(4)                                             # nothing in flight: removing virtual losses changes nothing
    assert np.array_equal(bits(st), bits(np.array(c.mcts.get_all_root_stats())))
    # budget already over after the warm-up simulation
    d = make()
    d.batch_playout(net, boards, turns, vl_batch=4, fused=True, time_budget=1e-9)
    assert d.last_playouts == 1 and (np.array(d.mcts.get_all_root_stats())[live, 0] == 1).all()


def test_device_generator_noise_and_symmetry(env):
    torch = env["torch"]
    rng = np.random.default_rng(9)
    boards, turns = S.random_openings(rng, 256, 6)
    w = env["W"].BatchedMCTS(256, 1.4, 1000, 0.3, 40, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True)
    w.seed(3)
    net = env["H"].HashEvaluator("cuda")
    w.batch_playout(net, boards, turns, vl_batch=4)
    st = w.get_root_stats()
    noise, prior = st["noise"], st["prior"]
    valid = prior > 0
    assert (noise >= 0).all() and np.allclose(noise.sum(1), 1.0, atol=1e-5)
    assert (noise[~valid] == 0).all()
    assert noise[valid].std() > 0.05                       # Dirichlet(0.3) is spiky, not uniform
    # two engines with different seeds draw different noise; same seed reproduces
    w2 = env["W"].BatchedMCTS(256, 1.4, 1000, 0.3, 40, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True)
    w2.seed(3)
    w2.batch_playout(net, boards, turns, vl_batch=4)
    assert np.array_equal(w2.get_root_stats()["noise"], noise)
    assert np.array_equal(w2.get_visits_count(), w.get_visits_count())
    w3 = env["W"].BatchedMCTS(256, 1.4, 1000, 0.3, 40, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True)
    w3.seed(4)
    w3.batch_playout(net, boards, turns, vl_batch=4)
    assert not np.array_equal(w3.get_root_stats()["noise"], noise)
    # prune draws fresh noise for the new root
    acts = np.argmax(w.get_visits_count(), 1).astype(np.int32)
    F = env["F"]
    a = torch.from_numpy(acts).cuda()
    F.check(F.lib().az_mcts_dev_prune_roots(w._fused.h, a.data_ptr(), F._stream()))
    torch.cuda.synchronize()
    st2 = w.get_root_stats()
    exp = st2["prior"].sum(1) > 0
    assert np.allclose(st2["noise"][exp].sum(1), 1.0, atol=1e-5)


def test_device_selfplay_driver(env):
    torch = env["torch"]
    net = env["H"].HashEvaluator("cuda")
    sp = env["SP"].DeviceSelfPlay(net, 256, n_playout=40, vl_batch=4, seed=1, temp_decay_moves=6)
    steps = 50
    for _ in range(steps):
        sp.step()
    tot = sp.read_totals()
    cnt = sp.engine_counters()
    assert tot["positions"] == steps * 256
    assert cnt["sims"] == steps * 256 * 40
    assert tot["games"] > 256 and tot["games"] == tot["p1_wins"] + tot["p2_wins"] + tot["draws"]
    # every game is a legal position: piece counts match the ply counter and the side to move
    n0 = np.array([bin(int(v) & (2**64 - 1)).count("1") for v in sp.bb_p1.cpu().tolist()])
    n1 = np.array([bin(int(v) & (2**64 - 1)).count("1") for v in sp.bb_p2.cpu().tolist()])
    ply = sp.ply.cpu().numpy(); turn = sp.turn.cpu().numpy()
    assert np.array_equal(n0 + n1, ply) and ((n0 - n1 == 0) | (n0 - n1 == 1)).all()
    assert np.array_equal(turn, np.where(ply % 2 == 0, 1, -1))
    assert (sp.bb_p1 & sp.bb_p2).abs().sum().item() == 0
    # trees stay bounded by the arena and the engine reports no overflow
    used = env["F"].C.c_int64()
    env["F"].check(env["F"].lib().az_mcts_max_used(sp.h, env["F"].C.byref(used)))
    assert 1 < used.value <= env["F"].lib().az_mcts_capacity(sp.h)


def test_streamed_selfplay_equals_its_drivers_run_alone(env):
    """StreamedSelfPlay: the games cut into groups that run on separate HIP streams and host
    threads.  Every group must play exactly the games it plays when it runs alone with the same
    seed (concurrency changes the timing, never a result), and the aggregate views must add up."""
    torch = env["torch"]
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    kw = dict(n_playout=24, vl_batch=4, temp_decay_moves=6, record=True, td_steps=2)
    plies = 14
    sp = env["SP"].StreamedSelfPlay(net, 1300, streams=2, seed=3, **kw)     # 650 trees per driver: the native loop
    sp.step(plies)
    sp.synchronize()
    tot = sp.read_totals()
    assert tot["positions"] == plies * 1300 and tot["games"] == tot["p1_wins"] + tot["p2_wins"] + tot["draws"]
    assert sp.engine_counters()["sims"] == plies * 1300 * 24
    games = sp.drain()
    assert len(games) == tot["games"] > 0 and max(g[2] for g in games) >= 650
    for i, part in enumerate(sp.parts):
        alone = env["SP"].DeviceSelfPlay(net, sp.sizes[i], seed=3 * 2 + i, **kw)
        for _ in range(plies):
            alone.step()
        torch.cuda.synchronize()
        assert torch.equal(alone.bb_p1, part.bb_p1) and torch.equal(alone.bb_p2, part.bb_p2)
        assert torch.equal(alone.ply, part.ply) and torch.equal(alone.totals, part.totals)
        mine = [g for g in games if sp.offsets[i] <= g[2] < sp.offsets[i] + sp.sizes[i]]
        ref = alone.drain()
        assert len(ref) == len(mine)
        for (w0, play0, slot0), (w1, play1, slot1) in zip(ref, mine):
            assert w0 == w1 and slot0 + sp.offsets[i] == slot1 and len(play0) == len(play1)
            for a, b in zip(play0, play1):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
    sp.close()
    # with the device transposition table: per-driver tables, aggregated statistics, same games
    spt = env["SP"].StreamedSelfPlay(net, 1300, streams=2, seed=3, table_log2=14, **kw)
    spt.step(plies)
    st = spt.table_stats()
    assert st["hits"] > 0 and st["lookups"] >= st["hits"] + st["inserts"] - 2 and 0.0 < st["hit_rate"] < 1.0
    assert spt.read_totals() == tot
    for a, b in zip(sp.parts, spt.parts):
        assert torch.equal(a.bb_p1, b.bb_p1) and torch.equal(a.bb_p2, b.bb_p2)
    spt.close()


def test_device_selfplay_trajectories_equal_reference_harness_g10(env):
    """the device driver's recorded trajectories, drained into play_data
    tuples, against the reference's own Game.batch_self_play + AlphaZeroPlayer output (fixture
    G10: no Dirichlet noise, no symmetry, so every random draw is numpy's and the driver's
    `sampler="reference"` replays it).  Bit-exact: states, visit distributions, root WDL,
    masks, targets, td-step WDL and the terminal tuples of all 16 games."""
    g = load("g10_selfplay_numpy_rng")
    net = env["H"].HashEvaluator("cuda")
    np.random.seed(5)
    sp = env["SP"].DeviceSelfPlay(net, 16, n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0,
                                  noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=False, mlh_slope=0.1,
                                  mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
                                  record=True, td_steps=2, refill=False, sampler="reference")
    for _ in range(43):
        sp.step()
        if bool(sp.dead.all()):
            break
    assert bool(sp.dead.all())
    games = sorted(sp.drain(), key=lambda t: t[2])
    assert [t[2] for t in games] == list(range(16))
    for i, (winner, play, _slot) in enumerate(games):
        assert winner == int(g[f"g{i}_winner"][0]), i
        for j, nm in enumerate(("state", "prob", "z", "steps", "aux", "root_wdl", "mask", "fut")):
            got = np.array([np.asarray(t[j]) for t in play])
            ref = g[f"g{i}_{nm}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (i, nm, got.shape, ref.shape, got.dtype, ref.dtype)
            if ref.dtype.kind == "f":
                assert np.array_equal(bits(got), bits(ref)), (i, nm)
            else:
                assert np.array_equal(got, ref), (i, nm)
    # row f4: the actor's upload body for these games, byte for byte (same numpy / python as the
    # generator; otherwise the pickles must at least decode to the same structure)
    import pickle
    import sys as _sys
    from src.selfplay import pack_upload
    mine = pack_upload(games)
    ref_payload = g["upload_payload"].tobytes()
    same_env = (list(g["upload_numpy_version"]) == [int(x) for x in np.__version__.split(".")[:2]]
                and list(g["upload_python_version"]) == list(_sys.version_info[:2]))
    if same_env:
        assert mine == ref_payload
    a, b = pickle.loads(mine), pickle.loads(ref_payload)
    assert a["__az__"] is True and len(a["data"]) == len(b["data"]) == 16
    for pa, pb in zip(a["data"], b["data"]):
        assert len(pa) == len(pb)
        for ta, tb in zip(pa, pb):
            assert len(ta) == len(tb) and all(type(x) is type(y) and np.array_equal(x, y) for x, y in zip(ta, tb))


def test_device_selfplay_noise_epsilon_decay_g14(env):
    """Fixture G14: the reference harness with AlphaZeroPlayer.noise_steps = 6 (the epsilon that scales
    the root priors decays from 0.25 to 0.05 over the first plies, game.py:87-91).  The driver keeps
    one epsilon per game (az_mcts_dev_set_noise_epsilons); with all games started together that is the
    reference's single value, and the play data must match bit for bit."""
    g = load("g14_selfplay_noise_decay")
    net = env["H"].HashEvaluator("cuda")
    np.random.seed(29)
    sp = env["SP"].DeviceSelfPlay(net, 12, n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0,
                                  noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=False, mlh_slope=0.1,
                                  mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
                                  record=True, td_steps=2, refill=False, sampler="reference",
                                  noise_steps=6, noise_eps_min=0.05)
    for _ in range(43):
        sp.step()
        if bool(sp.dead.all()):
            break
    assert bool(sp.dead.all())
    games = sorted(sp.drain(), key=lambda t: t[2])
    assert [t[2] for t in games] == list(range(12))
    for i, (winner, play, _slot) in enumerate(games):
        assert winner == int(g[f"g{i}_winner"][0]), i
        for j, nm in enumerate(("state", "prob", "z", "steps", "aux", "root_wdl", "mask", "fut")):
            got = np.array([np.asarray(t[j]) for t in play])
            ref = g[f"g{i}_{nm}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (i, nm)
            if ref.dtype.kind == "f":
                assert np.array_equal(bits(got), bits(ref)), (i, nm)
            else:
                assert np.array_equal(got, ref), (i, nm)
    # the decay is observable: without it the same seeds give other games
    np.random.seed(29)
    flat = env["SP"].DeviceSelfPlay(net, 12, n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0,
                                    noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=False, mlh_slope=0.1,
                                    mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
                                    record=True, td_steps=2, refill=False, sampler="reference")
    for _ in range(43):
        flat.step()
        if bool(flat.dead.all()):
            break
    other = sorted(flat.drain(), key=lambda t: t[2])
    assert any(len(a[1]) != len(b[1]) or not all(np.array_equal(x[1], y[1]) for x, y in zip(a[1], b[1]))
               for a, b in zip(games, other))
    # refill mode: every game decays from its own first ply
    sp2 = env["SP"].DeviceSelfPlay(net, 64, n_playout=24, vl_batch=4, seed=1, noise_steps=5, noise_eps_min=0.05)
    for _ in range(30):
        sp2.step()
    want = 0.05 + (0.25 - 0.05) * np.maximum(0.0, 1.0 - (sp2.ply.cpu().numpy() - 1) / 5)      # set before the ply counter moved
    got = sp2.eps_tree.cpu().numpy()
    fresh = sp2.ply.cpu().numpy() == 0                               # slots refilled this ply still show the old game's value
    assert np.allclose(got[~fresh], want[~fresh].astype(np.float32), atol=1e-7) and len(set(np.round(got, 4))) > 2


def test_device_selfplay_trajectories_plain_search_g11(env):
    """Fixture G11: the same harness on its other branches - no virtual loss (vl_batch 1), no
    td-step targets (7-tuples), every move sampled (no temperature switch), value decay 0.98,
    FPU reduction 0.4, no prior scaling.  Bit-exact against the reference's output."""
    g = load("g11_selfplay_plain_search")
    net = env["H"].HashEvaluator("cuda")
    np.random.seed(17)
    sp = env["SP"].DeviceSelfPlay(net, 8, n_playout=40, vl_batch=1, c_init=1.25, c_base=500, alpha=0.0,
                                  noise_epsilon=0.0, fpu_reduction=0.4, use_symmetry=False, mlh_slope=0.0,
                                  mlh_cap=0.2, value_decay=0.98, temperature=0.8, temp_decay_moves=0,
                                  temp_endgame=0, seed=1, record=True, td_steps=0, refill=False, sampler="reference")
    for _ in range(43):
        sp.step()
        if bool(sp.dead.all()):
            break
    games = sorted(sp.drain(), key=lambda t: t[2])
    assert [t[2] for t in games] == list(range(8))
    for i, (winner, play, _slot) in enumerate(games):
        assert winner == int(g[f"g{i}_winner"][0]), i
        assert all(len(t) == 7 for t in play)
        for j, nm in enumerate(("state", "prob", "z", "steps", "aux", "root_wdl", "mask")):
            got = np.array([np.asarray(t[j]) for t in play])
            ref = g[f"g{i}_{nm}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (i, nm)
            if ref.dtype.kind == "f":
                assert np.array_equal(bits(got), bits(ref)), (i, nm)
            else:
                assert np.array_equal(got, ref), (i, nm)


def test_device_selfplay_othello_trajectories_g12(env):
    """Fixture G12: the reference harness on Othello (pass action, games that end on a full board
    or on two passes, terminal disc difference as auxiliary target, score utility 0.15 in the
    search) against the device driver with game="Othello".  Bit-exact."""
    g = load("g12_selfplay_othello")
    net = env["H"].OthelloHashEvaluator("cuda")
    np.random.seed(23)
    sp = env["SP"].DeviceSelfPlay(net, 8, n_playout=32, vl_batch=4, c_init=1.4, c_base=160, alpha=0.0,
                                  noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=False, mlh_slope=0.0,
                                  temperature=1.0, temp_decay_moves=10, temp_endgame=0, seed=4, record=True,
                                  td_steps=2, refill=False, sampler="reference", game="Othello",
                                  score_utility_factor=0.15, score_scale=8.0)
    for _ in range(130):
        sp.step()
        if bool(sp.dead.all()):
            break
    assert bool(sp.dead.all())
    games = sorted(sp.drain(), key=lambda t: t[2])
    assert [t[2] for t in games] == list(range(8))
    for i, (winner, play, _slot) in enumerate(games):
        assert winner == int(g[f"g{i}_winner"][0]), i
        for j, nm in enumerate(("state", "prob", "z", "steps", "aux", "root_wdl", "mask", "fut")):
            got = np.array([np.asarray(t[j]) for t in play])
            ref = g[f"g{i}_{nm}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (i, nm, got.shape, ref.shape, got.dtype, ref.dtype)
            if ref.dtype.kind == "f":
                assert np.array_equal(bits(got), bits(ref)), (i, nm)
            else:
                assert np.array_equal(got, ref), (i, nm)


def test_device_selfplay_recording_with_refill(env):
    """Recording in the production mode (device sampling, finished slots refilled at once):
    structural invariants of every drained game."""
    net = env["H"].HashEvaluator("cuda")
    sp = env["SP"].DeviceSelfPlay(net, 128, n_playout=24, vl_batch=4, seed=2, temp_decay_moves=6, record=True, td_steps=3)
    for _ in range(70):
        sp.step()
    games = sp.drain()
    tot = sp.read_totals()
    assert len(games) == tot["games"] > 128 and int(sp.n_dropped.item()) == 0
    assert sum(w == 1 for w, _, _ in games) == tot["p1_wins"] and sum(w == 0 for w, _, _ in games) == tot["draws"]
    for winner, play, slot in games:
        T = len(play) - 1
        assert 7 <= T <= 42 and 0 <= slot < 128
        for t, tup in enumerate(play[:-1]):
            state, prob, z, steps, aux, wdl, mask, fut = tup
            assert state.dtype == np.int8 and state.shape == (3, 6, 7) and prob.dtype == np.float32
            assert int(state[:2].sum()) == t and (state[2] == (1 if t % 2 == 0 else -1)).all()
            assert abs(float(prob.sum()) - 1.0) < 1e-6 and (prob[~mask] == 0).all()
            assert (mask == (state[:2, 0].sum(0) == 0)).all()
            assert z == winner and steps == T - t and aux == T - t
            assert abs(float(wdl.sum()) - 1.0) < 1e-4
            ref_fut = play[t + 3][5] if t + 3 < T else np.zeros(3, np.float32)
            assert np.array_equal(fut, ref_fut)
        end = play[-1]
        assert int(end[0][:2].sum()) == T and end[2] == winner and end[3] == 0 and (end[1] == 0).all() and end[6].all()
        # absolute board of the end state: plane 0 = side to move, plane 1 = the player who just moved
        to_move = 1 if T % 2 == 0 else -1
        board = end[0][0].astype(np.int8) * to_move - end[0][1].astype(np.int8) * to_move
        assert S.np_winner(board) == winner and S.np_done(board)
    # draining empties the store
    assert sp.drain() == []


def test_fused_path_othello_bit_exact_vs_oracle(env):
    """Config-4 game through the device-resident loop: 65 actions, passes, score utility."""
    rng = np.random.default_rng(44)
    boards, turns = S.ot_openings(rng, 48, 40)
    cfg = dict(S.OT_DET_CFG, c_base=400.0)
    n, K, plies = 80, 4, 4
    o = O.BatchedMCTS_Othello(48)
    S.apply_cfg(o, cfg)
    ref = S.play_plies(o, boards, turns, n, K, plies, game=S.OthelloGame)
    w = env["W"].BatchedMCTS(48, c_init=cfg["c_init"], c_base=cfg["c_base"], alpha=0.0, n_playout=n,
                             game_name="Othello", noise_epsilon=0.0, fpu_reduction=cfg["fpu_reduction"],
                             use_symmetry=False, score_utility_factor=cfg["score_utility_factor"],
                             score_scale=cfg["score_scale"])
    net = env["H"].OthelloHashEvaluator("cuda")
    b, t = boards.copy(), turns.copy()
    for ply in range(plies):
        w.batch_playout(net, b, t, vl_batch=K)
        assert w._fused is not None
        c = w.get_visits_count().astype(np.int32)
        assert np.array_equal(c, ref["counts"][ply])
        assert np.array_equal(bits(np.array(w.mcts.get_all_root_stats())), bits(ref["stats"][ply]))
        acts = np.argmax(c, 1).astype(np.int32)
        w.prune_roots(acts)
        for i in range(48):
            t[i] = S.OthelloGame.advance(b[i], int(t[i]), int(acts[i]))


def test_fused_othello_with_network(env):
    """BASELINE config 3's evaluator through the device loop: the Othello network (az_net.OthelloNet,
    fixture G13 weights) as a torch module under autocast, fused path vs host path - same simulation
    budget, near-equal root Q, mostly equal best moves - and the self-play driver on top of it."""
    torch = env["torch"]
    net = env["N"].OthelloNet(h_dim=32, num_res_blocks=2, device="cuda")
    env["N"].load_reference_weights(net, load_split("g13_othello_weights"))
    rng = np.random.default_rng(3)
    boards, turns = S.ot_openings(rng, 96, 20, 0)
    res = []
    for fused in (True, False):
        w = env["W"].BatchedMCTS(96, 1.4, 800, 0.0, 120, noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False,
                                 game_name="Othello", score_utility_factor=0.15, score_scale=8.0)
        w.batch_playout(net, boards, turns, vl_batch=4, fused=fused)
        assert (w._fused is not None) == fused
        res.append((w.get_visits_count(), np.array(w.mcts.get_all_root_stats())))
    (c1, s1), (c2, s2) = res
    assert (s1[:, 0] == 120).all() and (s2[:, 0] == 120).all()
    assert (c1.sum(1) == 119).all() and (c2.sum(1) == 119).all()
    assert np.abs(s1[:, 1] - s2[:, 1]).mean() < 0.05
    assert (np.argmax(c1, 1) == np.argmax(c2, 1)).mean() > 0.7
    sp = env["SP"].DeviceSelfPlay(net, 128, n_playout=32, vl_batch=4, seed=1, game="Othello", temp_decay_moves=8,
                                  score_utility_factor=0.15, record=True)
    for _ in range(70):
        sp.step()
    tot = sp.read_totals()
    assert tot["positions"] == 70 * 128 and sp.engine_counters()["sims"] == 70 * 128 * 32
    games = sp.drain()
    assert len(games) == tot["games"] > 0
    for winner, play, slot in games:
        end = play[-1][0]
        own, opp = int(end[0].sum()), int(end[1].sum())
        assert winner == np.sign(own - opp) * int(end[2][0, 0]) and 4 < own + opp <= 64


def _rand_othello_net(env, seed):
    """OthelloNet at the reference's width with trained-looking BatchNorm statistics and non-zero heads"""
    torch = env["torch"]
    torch.manual_seed(seed)
    net = env["N"].OthelloNet(device="cuda")
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.2); m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.7, 1.3); m.bias.normal_(0.0, 0.1)
        for m in (net.policy_head.board_out, net.policy_head.pass_fc, net.dual_head.value_out[-1], net.dual_head.aux_out[-1]):
            m.weight.normal_(0.0, 0.05); m.bias.normal_(0.0, 0.05)
    return net


def test_folded_stem_matches_torch_and_the_embedding_stem(env):
    """az_nn_stem_folded (nn_stem.hip: the stem as a K = 18 GEMM on the 0/1 planes + a per-cell constant, tables from
    fast_net.fold_stem) against the layer in torch fp32 (embedding, convolution with bf16-rounded weights, SiLU;
    Network.py:168-170,226-239) - within bf16 output rounding - and against az_nn_stem_embed (bf16 tokens, K = 288),
    which it must beat in accuracy; planes and bitboards give identical bits; compact batches (gather, device-side count)."""
    torch = env["torch"]
    import ctypes as C
    from src.fast_net import FastConnect4Net, fold_stem, glue
    from src.az_net import Connect4Net
    L = glue()
    vp = C.c_void_p
    torch.manual_seed(11)
    mod = Connect4Net(device="cuda").eval()
    with torch.no_grad():
        mod.hidden[0].weight.normal_(0.0, 0.08); mod.hidden[0].bias.normal_(0.0, 0.3)
        mod.piece_emb.weight.normal_(0.0, 1.0); mod.pos_emb.weight.normal_(0.0, 1.0)
    net = FastConnect4Net.from_module(mod)
    assert net.folded_stem
    s = vp(torch.cuda.current_stream().cuda_stream)
    F = torch.nn.functional
    bf = lambda t: t.to(torch.bfloat16).float()                                   # noqa: E731
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    for bsz in (1, 3, 4, 1023, 4097):
        # random legal-looking boards: every cell empty / own / opponent
        st = torch.randint(0, 3, (bsz, 6, 7), device="cuda", generator=g)
        feat = torch.zeros((bsz, 3, 6, 7), device="cuda")
        feat[:, 0] = (st == 1).float(); feat[:, 1] = (st == 2).float(); feat[:, 2] = 1.0
        y = torch.full((bsz, 42, 64), 7.0, dtype=torch.bfloat16, device="cuda")
        assert L.az_nn_stem_folded(feat.data_ptr(), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), y.data_ptr(), bsz, None, None, s) == 0
        y_old = torch.empty_like(y)
        L.az_nn_stem_embed(feat.data_ptr(), net.emb_own.data_ptr(), net.emb_opp.data_ptr(), net.pos.data_ptr(),
                           net.stem_w.data_ptr(), net.stem_b.data_ptr(), y_old.data_ptr(), bsz, None, None, s)
        with torch.no_grad():
            tok = mod.embed(feat)                                                 # (B, 32, 6, 7) fp32
            want = F.silu(F.conv2d(tok, bf(mod.hidden[0].weight), bf(mod.hidden[0].bias), padding=1))
        want = want.permute(0, 2, 3, 1).reshape(bsz, 42, 64)
        torch.cuda.synchronize()
        err = (y.float() - want).abs() / (1.0 + want.abs())
        err_old = (y_old.float() - want).abs() / (1.0 + want.abs())
        # one bf16 rounding of the output: 2^-9 relative; the K = 288 kernel also carries the tokens' rounding
        assert err.max().item() < 4.5e-3 and err.mean().item() < 8e-4, (bsz, err.max().item(), err.mean().item())
        assert err.mean().item() <= err_old.mean().item() * 1.02, (bsz, err.mean().item(), err_old.mean().item())
    # bitboards instead of planes (the native loop's form): identical bits, mirrored ids included
    bsz = 777
    h = torch.randint(0, 7, (bsz, 7), device="cuda", generator=g)                 # column heights
    colour = torch.randint(0, 2, (bsz, 7, 6), device="cuda", generator=g)
    bb1 = torch.zeros(bsz, dtype=torch.int64, device="cuda"); bb2 = torch.zeros_like(bb1)
    grid = torch.zeros((bsz, 6, 7), device="cuda")                                # +1 / -1 stones, row 0 on top
    for c in range(7):
        for k in range(6):
            on = h[:, c] > k
            p1 = on & (colour[:, c, k] == 1)
            p2 = on & (colour[:, c, k] == 0)
            bb1 |= p1.long() << (7 * c + k); bb2 |= p2.long() << (7 * c + k)
            grid[:, 5 - k, c] = p1.float() - p2.float()
    turn = (torch.randint(0, 2, (bsz,), device="cuda", generator=g) * 2 - 1).int()
    sym = torch.randint(0, 2, (bsz,), device="cuda", generator=g).int()
    gsym = torch.where(sym.view(-1, 1, 1) != 0, grid.flip(2), grid)
    feat = torch.stack([(gsym * turn.view(-1, 1, 1) > 0).float(), (gsym * turn.view(-1, 1, 1) < 0).float(), torch.ones_like(gsym)], 1).contiguous()

    from src.abi import Positions
    pos = Positions(bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), sym.data_ptr())
    ya = torch.empty((bsz, 42, 64), dtype=torch.bfloat16, device="cuda"); yb = torch.empty_like(ya)
    assert L.az_nn_stem_folded(feat.data_ptr(), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), ya.data_ptr(), bsz, None, None, s) == 0
    assert L.az_nn_stem_folded_positions(C.byref(pos), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), yb.data_ptr(), bsz, None, None, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    # compact batch: rows picked by gather, their number read on the device
    rows = torch.randperm(bsz, device="cuda", generator=g)[:300].int().contiguous()
    n_rows = torch.tensor([300], dtype=torch.int64, device="cuda")
    yc = torch.full((bsz, 42, 64), 5.0, dtype=torch.bfloat16, device="cuda")
    assert L.az_nn_stem_folded(feat.data_ptr(), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), yc.data_ptr(), bsz, rows.data_ptr(), n_rows.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(yc[:300].view(torch.int16), ya[rows.long()].view(torch.int16))
    assert (yc[300:].float() == 5.0).all()
    assert L.az_nn_stem_folded(None, net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), yc.data_ptr(), bsz, None, None, s) == 1


def test_othello_conv_kernel_matches_torch(env):
    """az_nn_othello_conv (nn_othello.hip) against the same layer in torch fp32 with the reference's
    bf16 roundings, every supported geometry; batch sizes that leave workgroups with 0, 1 and
    several samples."""
    torch = env["torch"]
    import ctypes as C
    from src.fast_othello import pack_conv_weight
    from src.fast_net import glue
    L = glue()
    F = torch.nn.functional
    bf = lambda t: t.to(torch.bfloat16).float()                                   # noqa: E731
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    rn = lambda *sh: torch.randn(*sh, device="cuda", generator=g)                 # noqa: E731
    for (cin, hi, pad, pre, res), bsz in (((32, 8, 2, False, False), 37), ((256, 10, 1, True, False), 5), ((256, 10, 1, True, True), 700),
                                          ((256, 10, 1, False, False), 1), ((256, 10, 0, False, False), 130), ((256, 8, 1, False, False), 513)):
        ho = hi + 2 * pad - 2
        x = rn(bsz, hi, hi, cin).to(torch.bfloat16)
        w = (rn(256, cin, 3, 3) * (1.5 / (9 * cin) ** 0.5))
        pre_s, pre_b = (rn(cin) * 0.2 + 1.0, rn(cin) * 0.2) if pre else (None, None)
        post_s, post_b = rn(256) * 0.2 + 1.0, rn(256) * 0.2
        r = rn(bsz, ho, ho, 256).to(torch.bfloat16) if res else None
        y = torch.empty((bsz, ho, ho, 256), dtype=torch.bfloat16, device="cuda")
        wp = pack_conv_weight(w)
        rc = L.az_nn_othello_conv(x.data_ptr(), wp.data_ptr(), pre_s.data_ptr() if pre else None, pre_b.data_ptr() if pre else None,
                                  post_s.data_ptr(), post_b.data_ptr(), r.data_ptr() if res else None, y.data_ptr(), bsz, cin, hi, pad, 1,
                                  None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        xin = x.float()
        if pre:
            xin = bf(xin * pre_s + pre_b)
        conv = F.conv2d(xin.permute(0, 3, 1, 2), bf(w), padding=pad).permute(0, 2, 3, 1)
        out = bf(conv * post_s + post_b)
        if res:
            out = bf(out + r.float())
        want = bf(F.silu(out))
        torch.cuda.synchronize()
        err = (y.float() - want).abs()
        assert err.max().item() < 0.06 and err.mean().item() < 2e-3, (cin, hi, pad, pre, res, err.max().item(), err.mean().item())
    assert L.az_nn_othello_conv(x.data_ptr(), wp.data_ptr(), None, None, post_s.data_ptr(), post_b.data_ptr(), None, y.data_ptr(),
                                4, 64, 8, 1, 1, None, None) == 1                 # unsupported geometry is refused
    # the narrow kernel of the dual head's bottleneck: 256 -> 8 channels, no padding
    for bsz in (3, 1000):
        x = rn(bsz, 10, 10, 256).to(torch.bfloat16)
        w = rn(8, 256, 3, 3) * (1.5 / 2304 ** 0.5)
        w16 = torch.zeros(16, 256, 3, 3, device="cuda"); w16[:8] = w
        s16, b16 = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
        s16[:8], b16[:8] = rn(8) * 0.2 + 1.0, rn(8) * 0.2
        y = torch.full((bsz, 8, 8, 8), 7.0, dtype=torch.bfloat16, device="cuda")
        assert L.az_nn_othello_conv_narrow(x.data_ptr(), pack_conv_weight(w16).data_ptr(), s16.data_ptr(), b16.data_ptr(), y.data_ptr(),
                                           bsz, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        conv = F.conv2d(x.float().permute(0, 3, 1, 2), bf(w)).permute(0, 2, 3, 1)
        want = bf(F.silu(bf(conv * s16[:8] + b16[:8])))
        torch.cuda.synchronize()
        err = (y.float() - want).abs()
        assert err.max().item() < 0.06 and err.mean().item() < 2e-3, (bsz, err.max().item(), err.mean().item())


def test_fast_othello_twin_matches_module(env):
    """The HIP twin of the Othello network (fast_othello.py) against the module it snapshots, fp32 on
    the GPU: probabilities, WDL and score utility within bf16 error; and the device loop picks it."""
    torch = env["torch"]
    from src.fast_othello import FastOthelloNet
    net = _rand_othello_net(env, 3)
    assert FastOthelloNet.recognises(net)
    twin = FastOthelloNet(net)
    rng = np.random.default_rng(8)
    boards, turns = S.ot_openings(rng, 200, 40, 0)
    planes = np.stack([(boards == turns[:, None, None]), (boards == -turns[:, None, None]),
                       np.ones_like(boards) * turns[:, None, None]], 1).astype(np.float32)
    masks = np.zeros((200, 65), bool)
    for i in range(200):
        mv = S.ot_moves(boards[i], int(turns[i]))
        masks[i, mv if mv else [64]] = True
    x = torch.from_numpy(planes).cuda(); m = torch.from_numpy(masks).cuda()
    with torch.no_grad():
        lp, lv, aux = net(x, m)
    p0, w0 = lp.exp(), lv.exp()
    u0 = torch.atan(aux * 8.0) * (2.0 / np.pi)
    p1, w1, u1 = twin.predict_device(x, m)
    torch.cuda.synchronize()
    assert p1.shape == (200, 65) and w1.shape == (200, 3) and u1.shape == (200,)
    assert (p1 - p0).abs().max().item() < 0.03 and (p1 - p0).abs().mean().item() < 1e-3
    # the utility is atan(8 * aux): an error of the tanh head is amplified ~5x around zero
    assert (w1 - w0).abs().max().item() < 0.06 and (u1 - u0).abs().max().item() < 0.15 and (u1 - u0).abs().mean().item() < 0.03
    assert p0.std().item() > 1e-3 and w0.std().item() > 1e-2                      # the comparison is not between constants
    w = env["W"].BatchedMCTS(200, 1.4, 800, 0.0, 40, noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False,
                             game_name="Othello", score_utility_factor=0.15, score_scale=8.0)
    w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    assert isinstance(w._fused.fast, FastOthelloNet)
    assert (w.get_visits_count().sum(1) == 39).all()
    # compact batches: only the rows a device-side list names are evaluated and scattered back - the live
    # leaves, or what missed the table.  The convolution kernel computes a sample on its own, the thin
    # library GEMMs of the heads need not be bit-stable across batch sizes: compare within bf16 error.
    rows = torch.tensor([5, 17, 3, 150, 42], dtype=torch.int32, device="cuda")
    out = (torch.zeros_like(p1), torch.zeros_like(w1), torch.zeros_like(u1))
    twin.predict_device(x, m, rows=rows, n_rows=torch.tensor([5], device="cuda"), out=out)
    idx = rows.long()
    assert (out[0][idx] - p1[idx]).abs().max().item() < 5e-3 and (out[1][idx] - w1[idx]).abs().max().item() < 5e-3
    untouched = torch.ones(200, dtype=torch.bool, device="cuda"); untouched[idx] = False
    assert out[0][untouched].abs().max().item() == 0.0
    # the device table with the network (the wrapper's cache_size on the fused path): two searches from the same
    # roots, the second served mostly from the table
    w = env["W"].BatchedMCTS(200, 1.4, 800, 0.0, 40, noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False,
                             game_name="Othello", score_utility_factor=0.15, score_scale=8.0, cache_size=200000)
    for rep in range(2):
        for i in range(200):
            w.mcts.reset_env(i)
        w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
        assert (w.get_visits_count().sum(1) == 39).all()
    st = w._fused.table_stats()
    assert w._fused.table_log2 == 18 and st["hits"] > 0.4 * st["lookups"], st      # the second search replays the first
    w.refresh_cache(net)                                # same weights: every resident key re-evaluated in place
    for i in range(200):
        w.mcts.reset_env(i)
    w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    st2 = w._fused.table_stats()
    assert st2["lookups"] > st["lookups"] and (w.get_visits_count().sum(1) == 39).all()


def test_othello_table_refresh_in_place(env):
    """`refresh_cache` (MCTS_cpp.py:361-377) for an Othello table: after a weight update every resident
    key - the leaf as the evaluator saw it, decoded back from the entry - is evaluated again by the
    native model and stored under the same key.  The native evaluator is a pure function per row, so
    a search served from the refreshed table must equal, bit for bit, a search with the new weights
    and no table; the same table NOT refreshed must not (the check can fail)."""
    os.environ["AZ_FUSED_GRAPH"] = "0"               # below 512 trees too: the native loop, with and without the table
    try:
        _othello_table_refresh(env)
    finally:
        os.environ.pop("AZ_FUSED_GRAPH", None)


def _othello_table_refresh(env):
    torch = env["torch"]
    net = _rand_othello_net(env, 5)
    rng = np.random.default_rng(77)
    boards, turns = S.ot_openings(rng, 128, 34, 0)
    boards[:32] = boards[0]; turns[:32] = turns[0]

    def wrapper(cache):
        w = env["W"].BatchedMCTS(128, 1.4, 1000, 0.3, 48, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True,
                                 game_name="Othello", score_utility_factor=0.15, score_scale=8.0, cache_size=cache)
        w.seed(21)
        return w

    def search(w):
        w.batch_playout(net, boards, turns, vl_batch=4, fused=True)
        return w.get_visits_count().copy(), bits(np.array(w.mcts.get_all_root_stats()))

    tabled, stale = wrapper(200000), wrapper(200000)
    for w in (tabled, stale):
        search(w)                                                   # fills both tables with the OLD weights' outputs
        assert w._fused.table_log2 == 18 and w._fused.table_stats()["inserts"] > 0
        assert w._fused._native_model() is not None                 # the native loop and the native model are what ran
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.05)
    plain = wrapper(0)
    c0, s0 = search(plain)
    assert plain._fused._native_model() is not None
    cf, sf = search(wrapper(200000))                                # a table filled with the new weights' outputs from the start
    assert np.array_equal(c0, cf) and np.array_equal(s0, sf)
    # refreshed: the wrapper notices the new weights and re-evaluates the resident keys
    before = tabled._fused.table_stats()
    for i in range(128):
        tabled.reset_env(i)
    tabled.seed(21)
    tabled.refresh_cache(net)
    c1, s1 = search(tabled)
    after = tabled._fused.table_stats()
    assert np.array_equal(c0, c1) and np.array_equal(s0, s1)
    assert after["hits"] - before["hits"] > 0.3 * (after["lookups"] - before["lookups"]), (before, after)
    # not refreshed: new weights snapshotted behind the table's back - old outputs are served and the search differs
    fs = stale._fused
    fs.fast = None; fs._fast_version = None
    log2, fs.table_log2 = fs.table_log2, 0
    fs._sync_fast_net()
    fs.table_log2 = log2
    for i in range(128):
        stale.reset_env(i)
    stale.seed(21)
    c2, s2 = search(stale)
    assert not np.array_equal(s0, s2)


def test_othello_native_model_object(env):
    """The Othello evaluator as ONE native object (az_nn_model, kind OTHELLO_CNN: embedding from the leaves'
    bitboards, the convolutions, the bottleneck and both heads in HIP) against the twin it is built from -
    whose thin ends are torch operations - and against the module: within bf16 error; a leaf given under a
    symmetry id equals, bit for bit, the transformed position given under id 0; compact lists evaluate and
    scatter only the named rows; and the native loop engages for Othello with the network."""
    torch = env["torch"]
    import ctypes as C
    from src.fast_othello import FastOthelloNet
    F = env["F"]
    net = _rand_othello_net(env, 5)
    twin = FastOthelloNet(net)
    model = twin.native_model()
    from src.abi import Positions as Pos
    L = F.lib()
    rng = np.random.default_rng(12)
    n = 150
    boards, turns = S.ot_openings(rng, n, 44, 0)

    def masks_of(bs, ts):
        m = np.zeros((len(bs), 65), np.uint8)
        for i in range(len(bs)):
            mv = S.ot_moves(bs[i], int(ts[i]))
            m[i, mv if mv else [64]] = 1
        return m

    def run(bs, ts, syms, masks, rows=None):
        bb0, bb1 = S.ot_bitboards(bs)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()          # noqa: E731
        t0, t1 = dev(bb0.view(np.int64), np.int64), dev(bb1.view(np.int64), np.int64)
        tt, sy, mk = dev(ts, np.int32), dev(syms, np.int32), dev(masks, np.uint8)
        k = len(bs)
        probs = torch.zeros((k, 65), device="cuda"); wdl = torch.zeros((k, 3), device="cuda"); ut = torch.zeros(k, device="cuda")
        nb = int(L.az_nn_model_scratch_bytes(model, k))
        scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
        pos = Pos(t0.data_ptr(), t1.data_ptr(), tt.data_ptr(), sy.data_ptr())
        r_ptr = n_ptr = None
        if rows is not None:
            r = dev(rows, np.int32); c = torch.tensor([len(rows)], dtype=torch.int64, device="cuda")
            r_ptr, n_ptr = r.data_ptr(), c.data_ptr()
        assert L.az_nn_model_forward_positions(model, C.byref(pos), mk.data_ptr(), probs.data_ptr(), wdl.data_ptr(), ut.data_ptr(),
                                               k, r_ptr, n_ptr, scratch.data_ptr(), nb, F._stream()) == 0
        torch.cuda.synchronize()
        return probs, wdl, ut

    masks = masks_of(boards, turns)
    p, w, u = run(boards, turns, np.zeros(n, np.int32), masks)
    planes = np.stack([(boards == turns[:, None, None]), (boards == -turns[:, None, None]),
                       np.ones_like(boards) * turns[:, None, None]], 1).astype(np.float32)
    x = torch.from_numpy(planes).cuda(); m = torch.from_numpy(masks.astype(bool)).cuda()
    p1, w1, u1 = twin.predict_device(x, m)
    with torch.no_grad():
        lp, lv, aux = net(x, m)
    p0, w0, u0 = lp.exp(), lv.exp(), torch.atan(aux * 8.0) * (2.0 / np.pi)
    err = dict(vs_twin=((p - p1).abs().max().item(), (w - w1).abs().max().item(), (u - u1).abs().max().item()),
               vs_module=((p - p0).abs().max().item(), (w - w0).abs().max().item(), (u - u0).abs().max().item()))
    print("othello native model:", err)
    assert err["vs_twin"][0] < 5e-3 and err["vs_twin"][1] < 1e-2 and err["vs_twin"][2] < 3e-2, err
    assert err["vs_module"][0] < 0.03 and err["vs_module"][1] < 0.06 and err["vs_module"][2] < 0.15, err
    assert abs(p.sum(1) - 1).max().item() < 1e-5 and abs(w.sum(1) - 1).max().item() < 1e-5
    # symmetry ids: the leaf under id s == the transformed position under id 0 (apply_symmetry moves stone i to T_s(i))
    tf = {2: lambda b: b[::-1, ::-1], 6: lambda b: b.T, 7: lambda b: b[::-1, ::-1].T}
    for sid, f in tf.items():
        tb = np.stack([np.ascontiguousarray(f(b)) for b in boards])
        tm = masks_of(tb, turns)
        pa, wa, ua = run(boards, turns, np.full(n, sid, np.int32), tm)
        pb, wb, ub = run(tb, turns, np.zeros(n, np.int32), tm)
        assert torch.equal(pa, pb) and torch.equal(wa, wb) and torch.equal(ua, ub), sid
    # compact list
    rows = np.array([7, 3, 140, 21], np.int32)
    pc, wc, uc = run(boards, turns, np.zeros(n, np.int32), masks, rows=rows)
    idx = torch.from_numpy(rows.astype(np.int64)).cuda()
    assert torch.equal(pc[idx], p[idx]) and torch.equal(wc[idx], w[idx]) and torch.equal(uc[idx], u[idx])
    rest = torch.ones(n, dtype=torch.bool, device="cuda"); rest[idx] = False
    assert pc[rest].abs().max().item() == 0.0
    # the heads' first version (k_oth_heads: fp32 matvec, four samples per workgroup) against the one in use
    # (k_oth_heads16: the auxiliary Linear on the matrix cores with bf16 weights, one wavefront per sample for the rest):
    # same policy and value to fp32 rounding, the utility within what bf16 weights of one 512 x 512 layer cost; a batch
    # that does not fill the last workgroup of sixteen
    import os
    os.environ["AZ_OTH_HEADS_MFMA"] = "0"
    try:
        twin_old = FastOthelloNet(net)
        model_new, model = model, twin_old.native_model()
        po, wo, uo = run(boards, turns, np.zeros(n, np.int32), masks)
    finally:
        del os.environ["AZ_OTH_HEADS_MFMA"]
        model = model_new
    assert (p - po).abs().max().item() < 2e-6 and (w - wo).abs().max().item() < 2e-6, ((p - po).abs().max().item(), (w - wo).abs().max().item())
    assert (u - uo).abs().max().item() < 5e-3, (u - uo).abs().max().item()
    # the device loop: above 512 trees the whole search is one native call for Othello as well
    b600 = np.tile(boards, (4, 1, 1)); t600 = np.tile(turns, 4)
    wr = env["W"].BatchedMCTS(600, 1.4, 800, 0.3, 24, noise_epsilon=0.25, fpu_reduction=0.2, use_symmetry=True,
                              game_name="Othello", score_utility_factor=0.15, score_scale=8.0)
    wr.batch_playout(net, b600, t600, vl_batch=4, fused=True)
    assert wr._fused._native_model() is not None and isinstance(wr._fused.fast, FastOthelloNet)
    st = np.array(wr.mcts.get_all_root_stats())
    assert (st[:, 0] == 24).all() and (wr.get_visits_count().sum(1) == 23).all()


def test_native_search_refuses_misuse_and_reservation_is_sized(env):
    """az_mcts_dev_search reports misuse through the error code / az_last_error (no evaluator, an
    Othello engine, a table that was never created); the self-play driver reserves the arena for the
    plies to come (a re-rooting compacts the trees that run out of room, so not for a whole game)."""
    torch = env["torch"]
    F = env["F"]
    L = F.lib()
    w = env["W"].BatchedMCTS(600, 1.4, 400, 0.3, 16)
    h = F.C.c_void_p(w.mcts.handle)
    s = F._stream()
    assert L.az_mcts_dev_search(h, None, 16, 4, 0, s) != 0 and b"model" in L.az_last_error()
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    from src.fast_net import FastConnect4Net
    twin = FastConnect4Net.from_module(net)          # owns the model object: keep it alive
    model = twin.native_model()
    assert model is not None
    assert L.az_mcts_dev_search(h, model, 16, 4, 1, s) != 0 and b"table" in L.az_last_error()
    assert L.az_mcts_dev_search(h, model, 16, 0, 0, s) != 0
    wo = env["W"].BatchedMCTS(64, 1.4, 400, 0.3, 16, game_name="Othello")
    assert L.az_mcts_dev_search(F.C.c_void_p(wo.mcts.handle), model, 16, 4, 0, s) != 0 and b"does not belong" in L.az_last_error()
    assert L.az_mcts_dev_search(h, model, 0, 4, 0, s) == 0                      # nothing to do is not an error
    torch.cuda.synchronize()
    sp = env["SP"].DeviceSelfPlay(env["H"].HashEvaluator("cuda"), 512, n_playout=100, vl_batch=4)
    assert L.az_mcts_capacity(sp.h) >= 6 * 100 * 7                    # six plies' worst-case growth per arena half
    sp = env["SP"].DeviceSelfPlay(env["H"].HashEvaluator("cuda"), 64, n_playout=40, vl_batch=4, reserve_slots=5000)
    assert L.az_mcts_capacity(sp.h) == 5000


def test_full_size_native_loop_properties(env):
    """BASELINE config 1's size through the product path (az_mcts_dev_search with the HIP evaluator,
    compact batches): 8192 trees x 200 simulations, K = 4, no randomness.  Size-independent
    properties: every root saw n_playout visits; 128 copies of 64 positions grow 128 identical
    forests (each leaf is evaluated independently of its batch, whatever rows it shares it with);
    and the first 64 trees equal a 64-tree engine run on the same positions - a different batch
    size, the hipGraph loop instead of the native one."""
    wts = load("g7_checkpoint_weights")
    net = env["N"].Connect4Net(device="cuda").eval()
    env["N"].load_reference_weights(net, {k: wts[k] for k in wts.files})
    B, n, K = 8192, 200, 4
    rng = np.random.default_rng(17)
    b64, t64 = S.random_openings(rng, 64, 12)
    boards = np.tile(b64, (B // 64, 1, 1)); turns = np.tile(t64, B // 64)
    kw = dict(noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False, mlh_slope=0.1)
    w = env["W"].BatchedMCTS(B, 1.4, 1000, 0.0, n, **kw)
    w.batch_playout(net, boards, turns, vl_batch=K, fused=True)
    assert w._fused._native_model() is not None
    c = w.get_visits_count()
    st = np.array(w.mcts.get_all_root_stats())
    assert (st[:, 0] == n).all() and (c.sum(1) == n - 1).all()
    assert np.array_equal(c.reshape(B // 64, 64, 7), np.broadcast_to(c[:64], (B // 64, 64, 7)))
    assert np.array_equal(bits(st).reshape(B // 64, 64, -1), np.broadcast_to(bits(st[:64]), (B // 64, 64, st.shape[1])))
    assert np.allclose(st[:, 3] + st[:, 4] + st[:, 5], 1.0, atol=1e-5)
    small = env["W"].BatchedMCTS(64, 1.4, 1000, 0.0, n, **kw)
    small.batch_playout(net, b64, t64, vl_batch=K, fused=True)
    assert small._fused._native_model() is None                      # 64 trees: graph replay of the Python loop
    assert np.array_equal(small.get_visits_count(), c[:64])
    assert np.array_equal(bits(np.array(small.mcts.get_all_root_stats())), bits(st[:64]))
