"""Every kernel of the Othello evaluator (nn_othello.hip, nn_othello_heads.hip) against the float64 references of
othello_ref.py, through its own entry point, and the model object (nn_model.hip) against those entry points in order.

  embedding     bit for bit
  convolutions  inputs drawn so that every fp32 partial sum is exact: the pre-SiLU values of kernel and reference are
                the same numbers, the output may differ by one bf16 ulp only where the float64 SiLU value sits on a
                midpoint between two bf16 numbers (othello_ref.bf16_midpoint_band) and is equal everywhere else
  heads         within max(8 * E32, 2e-6) of the float64 reference, E32 being the error of the same heads in plain fp32
  model object  bit for bit the chain of entry points

Output buffers start as NaN (bf16 0x7fc0 / float NaN) with guard rows behind the batch: what a kernel must not write is
checked next to what it must.  test_othello_ref_cpu.py shows, without a GPU, that the comparisons used here reject wrong
results and that the references are the module's arithmetic."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import othello_ref as R
import scenarios as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
GUARD = 2                       # rows behind the batch that nothing may write
NAN16 = 0x7fc0


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import az_net, fast_othello
    from src.fast_net import Positions, glue
    L = glue()
    return dict(torch=torch, N=az_net, FO=fast_othello, Positions=Positions, L=L, cache={})


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf16(torch, a):
    """bf16-representable float64 array -> bf16 tensor on the device, through its bit patterns"""
    return torch.from_numpy(R.bf16_bits(a).view(np.int16)).cuda().view(torch.bfloat16)


def _f32(torch, a):
    a32 = np.asarray(a, dtype=np.float32)
    assert np.array_equal(a32.astype(np.float64), np.asarray(a, dtype=np.float64), equal_nan=True)      # the kernel sees the reference's numbers
    return torch.from_numpy(np.ascontiguousarray(a32)).cuda()


def _nan16(torch, *shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _untouched16(torch, t):
    return bool((t.view(torch.int16) == NAN16).all().item())


def _count(torch, n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------------------------------------
# a. the embedding

def _embed(env, dev, tokens, batch, gather=None, count=None):
    torch, L = env["torch"], env["L"]
    pos = env["Positions"](dev["bb1"].data_ptr(), dev["bb2"].data_ptr(), dev["turn"].data_ptr(), dev["sym"].data_ptr())
    assert L.az_nn_othello_embed(C.byref(pos), dev["mask"].data_ptr(), dev["table"].data_ptr(), tokens.data_ptr(), batch,
                                 None if gather is None else gather.data_ptr(), None if count is None else count.data_ptr(),
                                 _stream(torch)) == 0
    torch.cuda.synchronize()
    return tokens.view(torch.int16).cpu().numpy()


def test_embed_bit_exact(env):
    torch = env["torch"]
    bb1, bb2, turn, sym, masks, table = R.embed_case()
    n = len(turn)
    assert n == 11 and set(turn) == {1, -1} and set(sym) == {0, 2, 6, 7}
    assert len({r.tobytes() for r in table}) == 256
    ref = R.embed_ref(bb1, bb2, turn, sym, masks, table)
    want = R.bf16_bits(ref).view(np.int16).reshape(n, 64, 32)
    dev = dict(bb1=torch.from_numpy(bb1.view(np.int64)).cuda(), bb2=torch.from_numpy(bb2.view(np.int64)).cuda(),
               turn=torch.from_numpy(turn.astype(np.int32)).cuda(), sym=torch.from_numpy(sym.astype(np.int32)).cuda(),
               mask=torch.from_numpy(masks).cuda(), table=_bf16(torch, table))
    got = _embed(env, dev, _nan16(torch, n + GUARD, 64, 32), n)
    assert R.embed_mismatch(got[:n].reshape(n, 8, 8, 32), ref) == 0
    assert (got[n:] == NAN16).all()
    # a gather list: sample b of the launch is row gather[b], six of them, their number on the device
    rows = np.array([9, 2, 10, 0, 5, 7], np.int32)
    got = _embed(env, dev, _nan16(torch, n + GUARD, 64, 32), n, torch.from_numpy(rows).cuda(), _count(torch, 6))
    assert np.array_equal(got[:6], want[rows]) and (got[6:] == NAN16).all()
    # a device-side count below the batch: the tokens of samples 4.. keep their prefill
    got = _embed(env, dev, _nan16(torch, n + GUARD, 64, 32), n, None, _count(torch, 4))
    assert np.array_equal(got[:4], want[:4]) and (got[4:] == NAN16).all()


# ---------------------------------------------------------------------------------------------
# b. the convolutions, exact arithmetic

def _conv_dev(env, idx):
    """the pool of kernel idx on the device (made once): inputs, packed weights, affines, residuals"""
    key = ("conv", idx)
    if key not in env["cache"]:
        torch = env["torch"]
        d, y, v = R.conv_pool(idx)
        dev = dict(x=_bf16(torch, d["x"]), pre=None, res=None)
        w = d["w"]
        if R.ALL_KERNELS[idx] == R.NARROW:            # 8 channels padded to one tile of 16; entries 8..15 of the affine are unused: NaN
            w = np.concatenate([w, np.zeros_like(w)])
            nan8 = np.full(8, np.nan)
            dev["post"] = tuple(_f32(torch, np.concatenate([a, nan8])) for a in d["post"])
        else:
            dev["post"] = tuple(_f32(torch, a) for a in d["post"])
        assert np.array_equal(R.bf16_round(w), w)
        dev["wp"] = env["FO"].pack_conv_weight(torch.from_numpy(np.array(w)).cuda())
        if d["pre"] is not None:
            dev["pre"] = tuple(_f32(torch, a) for a in d["pre"])
        if d["residual"] is not None:
            dev["res"] = _bf16(torch, d["residual"])
        env["cache"][key] = dev
    return env["cache"][key]


def _run_conv(env, idx, batch, count=None):
    """kernel idx on `batch` samples, sample i = pool sample i % 5 -> the output with its guard rows (device, bf16)"""
    torch, L = env["torch"], env["L"]
    dev = _conv_dev(env, idx)
    d, y, v = R.conv_pool(idx)
    pick = torch.arange(batch, device="cuda") % 5
    x = dev["x"][pick].contiguous()
    out = _nan16(torch, batch + GUARD, *y.shape[1:])
    cnt = None if count is None else _count(torch, count)
    cp = None if cnt is None else cnt.data_ptr()
    if R.ALL_KERNELS[idx] == R.NARROW:
        rc = L.az_nn_othello_conv_narrow(x.data_ptr(), dev["wp"].data_ptr(), dev["post"][0].data_ptr(), dev["post"][1].data_ptr(),
                                         out.data_ptr(), batch, cp, _stream(torch))
    else:
        cin, hi, pad, pre, res = R.ALL_KERNELS[idx]
        r = dev["res"][pick].contiguous() if res else None
        rc = L.az_nn_othello_conv(x.data_ptr(), dev["wp"].data_ptr(), dev["pre"][0].data_ptr() if pre else None,
                                  dev["pre"][1].data_ptr() if pre else None, dev["post"][0].data_ptr(), dev["post"][1].data_ptr(),
                                  r.data_ptr() if res else None, out.data_ptr(), batch, cin, hi, pad, 1, cp, _stream(torch))
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _check_conv(env, idx, out, n, tag):
    """rows 0..n-1 of `out` against the pool's reference (row i: pool sample i % 5)"""
    torch = env["torch"]
    d, y, v = R.conv_pool(idx)
    pick = np.arange(n) % 5
    m = R.conv_mismatch(out[:n].view(torch.int16).cpu().numpy(), y[pick], v[pick])
    print("othello conv %s %s: %s" % (R.ALL_KERNELS[idx], tag, m))
    assert R.conv_ok(m), (R.ALL_KERNELS[idx], tag, m)


KERNELS = range(len(R.ALL_KERNELS))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("idx", KERNELS)
def test_conv_exact(env, idx, batch):
    torch = env["torch"]
    out = _run_conv(env, idx, batch)
    _check_conv(env, idx, out, batch, "B=%d" % batch)
    assert _untouched16(torch, out[batch:])


@pytest.mark.parametrize("idx", KERNELS)
def test_conv_exact_past_the_grid_cap(env, idx):
    """two and three samples per workgroup: the stage / image of one sample is overwritten by the next one's, and
    consecutive samples of a workgroup differ.  The reference covers the five pool samples; every copy of a pool sample
    must then be the same bytes."""
    torch = env["torch"]
    batch = 1539 if R.ALL_KERNELS[idx] == R.NARROW else 1027                      # grid caps 768 and 512
    out = _run_conv(env, idx, batch)
    _check_conv(env, idx, out, 5, "B=%d" % batch)
    flat = out.view(torch.int16).reshape(batch + GUARD, -1)
    assert torch.equal(flat[:batch], flat[torch.arange(batch, device="cuda") % 5])
    assert _untouched16(torch, out[batch:])


@pytest.mark.parametrize("idx", KERNELS)
def test_conv_device_count(env, idx):
    torch = env["torch"]
    out = _run_conv(env, idx, 9, count=5)
    _check_conv(env, idx, out, 5, "B=9 count=5")
    assert _untouched16(torch, out[5:])                                           # rows 5..8 and the guard rows
    out = _run_conv(env, idx, 9, count=100)                                       # a count above the batch: the batch holds
    _check_conv(env, idx, out, 9, "B=9 count=100")
    assert _untouched16(torch, out[9:])


# ---------------------------------------------------------------------------------------------
# c. the heads

HEADS_SEED, HEADS_N = 21, 37


@functools.lru_cache(maxsize=None)
def _heads_ref(sharp):
    """weights, inputs, the float64 reference and the plain fp32 evaluation's error against it (E32), once per case"""
    import torch
    w, pm, h8 = R.heads_draw(HEADS_SEED, sharp=sharp, n=HEADS_N)
    ref = R.heads_ref(pm, h8, w)
    e32 = R.heads_errors(R.heads_ref(pm, h8, w, dtype=torch.float32), ref)
    return w, pm, h8, ref, e32


def _heads_dev(env, sharp):
    key = ("heads", sharp)
    if key not in env["cache"]:
        torch = env["torch"]
        w, pm, h8, ref, e32 = _heads_ref(sharp)
        t = dict(board_w=_bf16(torch, w["board_w"]), pass_norm_w=_f32(torch, w["pass_norm_w"]), pass_fc_w=_f32(torch, w["pass_fc_w"]),
                 v_conv_w=_f32(torch, w["v_conv_w"].reshape(8, 72).T),           # (72, 8): [ci * 9 + 3 ky + kx][co]
                 v_bn_s=_f32(torch, w["v_bn_s"]), v_bn_b=_f32(torch, w["v_bn_b"]), v_fc_w=_f32(torch, w["v_fc_w"]),
                 v_fc_b=_f32(torch, w["v_fc_b"]), a_fc_wt=_f32(torch, w["a_fc_w"].T),                  # (512 in = 64 c + cell, 512 out)
                 a_fc_b=_f32(torch, w["a_fc_b"]), a_norm_w=_f32(torch, w["a_norm_w"]), a_out_w=_f32(torch, w["a_out_w"]),
                 a_fc_w16=_bf16(torch, w["a_fc_w"].reshape(512, 8, 64).transpose(0, 2, 1).reshape(512, 512)))   # [out][8 cell + c]
        structs = {}
        for mfma in (False, True):
            s = env["FO"]._HeadsW()
            for name in env["FO"]._HeadsW._PTRS:
                setattr(s, name, t[name].data_ptr())
            for name in ("board_b", "pass_fc_b", "a_out_b", "aux_to_score", "eps"):
                assert float(np.float32(w[name])) == w[name]
                setattr(s, name, w[name])
            s.a_fc_w16 = t["a_fc_w16"].data_ptr() if mfma else None
            structs[mfma] = s
        env["cache"][key] = dict(keep=t, structs=structs, pm=_bf16(torch, pm), h8=_bf16(torch, h8))
    return env["cache"][key]


def _run_heads(env, sharp, mfma, batch, scatter=None, count=None):
    """-> (probs, wdl, utility) with GUARD rows behind the batch, NaN where the kernel wrote nothing (numpy)"""
    torch, L = env["torch"], env["L"]
    dev = _heads_dev(env, sharp)
    outs = [torch.full(s, float("nan"), device="cuda") for s in ((batch + GUARD, 65), (batch + GUARD, 3), (batch + GUARD,))]
    sc = None if scatter is None else torch.from_numpy(np.asarray(scatter, np.int32)).cuda()
    cnt = None if count is None else _count(torch, count)
    assert L.az_nn_othello_heads(dev["pm"].data_ptr(), dev["h8"].data_ptr(), C.byref(dev["structs"][mfma]), outs[0].data_ptr(),
                                 outs[1].data_ptr(), outs[2].data_ptr(), batch, None if sc is None else sc.data_ptr(),
                                 None if cnt is None else cnt.data_ptr(), _stream(torch)) == 0
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _check_heads(sharp, mfma, got, rows_out, rows_ref, tag):
    """rows `rows_out` of the kernel's outputs are samples `rows_ref` of the reference; every other row is still NaN"""
    w, pm, h8, ref, e32 = _heads_ref(sharp)
    sel = tuple(g[rows_out] for g in got)
    want = tuple(r[rows_ref] for r in ref)
    print("othello heads %s sharp=%g %s: E32 %s, kernel %s" % ("k_oth_heads16" if mfma else "k_oth_heads", sharp, tag,
                                                               "%.3g / %.3g / %.3g" % e32, "%.3g / %.3g / %.3g" % R.heads_errors(sel, want)))
    assert R.heads_problems(sel, want, e32) == []
    rest = np.ones(len(got[2]), bool); rest[rows_out] = False
    for g in got:
        assert np.isnan(g[rest]).all()


def _far_from_flat(sharp):
    w, pm, h8, (p, v, u), e32 = _heads_ref(sharp)
    assert (p.max(1) / p.min(1)).min() > 100 and v.std() > 0.1 and u.std() > 0.2


@pytest.mark.parametrize("mfma,batch", [(False, b) for b in (1, 3, 4, 5, 9)] + [(True, b) for b in (1, 3, 15, 16, 17, 37)])
def test_heads_batches(env, mfma, batch):
    """k_oth_heads (4 samples per workgroup) and k_oth_heads16 (16 per workgroup, wavefront w: samples w, w + 4, ...)
    at batches below, at and past a workgroup's share.

    Measured on an MI355X (probs / wdl / utility, maximum over the batches): E32 1.56e-7 / 4.81e-7 / 8.76e-7 (so the
    bounds are 2e-6 / 3.85e-6 / 7.0e-6); k_oth_heads 1.08e-7 / 2.43e-7 / 5.72e-8; k_oth_heads16 1.44e-7 / 4.85e-7 /
    7.01e-7."""
    _far_from_flat(1.0)
    got = _run_heads(env, 1.0, mfma, batch)
    _check_heads(1.0, mfma, got, np.arange(batch), np.arange(batch), "B=%d" % batch)


@pytest.mark.parametrize("mfma", [False, True])
def test_heads_sharp_softmax(env, mfma):
    """board and pass weights times 25: a logit range of a few hundred, probabilities from 1 down to nothing.

    Measured on an MI355X (probs / wdl / utility): E32 3.09e-6 / 4.81e-7 / 8.76e-7 (bounds 2.47e-5 / 3.85e-6 / 7.0e-6);
    k_oth_heads 3.21e-6 / 4.85e-7 / 9.76e-7; k_oth_heads16 2.59e-6 / 4.85e-7 / 7.01e-7."""
    w, pm, h8, (p, v, u), e32 = _heads_ref(25.0)
    _far_from_flat(25.0)
    logits = np.log(np.maximum(p, 1e-300))
    assert (logits.max(1) - logits.min(1)).max() > 200
    got = _run_heads(env, 25.0, mfma, 17)
    _check_heads(25.0, mfma, got, np.arange(17), np.arange(17), "B=17")


@pytest.mark.parametrize("mfma", [False, True])
def test_heads_scatter_with_stray_rows(env, mfma):
    """sample b goes to row scatter[b]; entries outside 0 .. batch - 1 (-1 and the batch itself) are skipped"""
    batch = 17 if mfma else 9
    rng = np.random.default_rng(6)
    scatter = rng.permutation(batch).astype(np.int32)
    scatter[2], scatter[batch - 3] = -1, batch
    live = np.array([b for b in range(batch) if 0 <= scatter[b] < batch])
    assert len(live) == batch - 2
    got = _run_heads(env, 1.0, mfma, batch, scatter=scatter)
    _check_heads(1.0, mfma, got, scatter[live], live, "scatter B=%d" % batch)


@pytest.mark.parametrize("mfma", [False, True])
def test_heads_device_count(env, mfma):
    batch, count = (37, 18) if mfma else (9, 5)
    got = _run_heads(env, 1.0, mfma, batch, count=count)
    _check_heads(1.0, mfma, got, np.arange(count), np.arange(count), "B=%d count=%d" % (batch, count))
    scatter = np.arange(batch, dtype=np.int32)[::-1].copy()                       # with a scatter list: the first `count` entries only
    got = _run_heads(env, 1.0, mfma, batch, scatter=scatter, count=count)
    _check_heads(1.0, mfma, got, scatter[:count], np.arange(count), "reversed B=%d count=%d" % (batch, count))


# ---------------------------------------------------------------------------------------------
# d. the model object is its entry points in order

def _rand_othello_net(env, seed):
    """as test_fused_gpu._rand_othello_net: trained-looking BatchNorm statistics and non-zero heads"""
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


def test_model_object_is_its_entry_points_in_order(env):
    torch, L = env["torch"], env["L"]
    net = _rand_othello_net(env, 5)
    twin = env["FO"].FastOthelloNet(net)
    model = twin.native_model()
    w = twin._model_w                                                             # the az_nn_othello_weights it was created from
    n = 21
    boards, turns = S.ot_openings(np.random.default_rng(31), n, 40, 0)
    syms = np.array([0, 2, 6, 7], np.int32)[np.arange(n) % 4]
    masks = np.zeros((n, 65), np.uint8)
    for i in range(n):                                                            # the mask is in the shown frame
        mv = S.ot_moves(np.ascontiguousarray(R.SYMMETRIES[int(syms[i])](boards[i])), int(turns[i]))
        masks[i, mv if mv else [64]] = 1
    bb1, bb2 = S.ot_bitboards(boards)
    dev = dict(bb1=torch.from_numpy(bb1.view(np.int64)).cuda(), bb2=torch.from_numpy(bb2.view(np.int64)).cuda(),
               turn=torch.from_numpy(turns.astype(np.int32)).cuda(), sym=torch.from_numpy(syms).cuda(), mask=torch.from_numpy(masks).cuda())
    pos = env["Positions"](dev["bb1"].data_ptr(), dev["bb2"].data_ptr(), dev["turn"].data_ptr(), dev["sym"].data_ptr())
    s = _stream(torch)
    bf = torch.bfloat16

    def outputs():
        return torch.zeros((n, 65), device="cuda"), torch.zeros((n, 3), device="cuda"), torch.zeros(n, device="cuda")

    def by_model(rows, cnt):
        nb = int(L.az_nn_model_scratch_bytes(model, n))
        scratch = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        out = outputs()
        assert L.az_nn_model_forward_positions(model, C.byref(pos), dev["mask"].data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr(), n, rows, cnt, scratch.data_ptr(), nb, s) == 0
        torch.cuda.synchronize()
        return out

    def by_hand(rows, cnt):
        def conv(i, x, res):
            wp, pre, post, has_res, c_in, h_in, pad = twin.layers[i]
            ho = h_in + 2 * pad - 2
            y = torch.zeros((n, ho, ho, 256), dtype=bf, device="cuda")
            assert L.az_nn_othello_conv(x.data_ptr(), wp.data_ptr(), None if pre is None else pre[0].data_ptr(),
                                        None if pre is None else pre[1].data_ptr(), post[0].data_ptr(), post[1].data_ptr(),
                                        res.data_ptr() if has_res else None, y.data_ptr(), n, c_in, h_in, pad, 1, cnt, s) == 0
            return y
        tok = torch.zeros((n, 8, 8, 32), dtype=bf, device="cuda")
        assert L.az_nn_othello_embed(C.byref(pos), dev["mask"].data_ptr(), twin.embed_table.data_ptr(), tok.data_ptr(), n, rows, cnt, s) == 0
        h = conv(0, tok, None)
        i = 1
        while i < twin.n_body - 1:                                                # the residual blocks: conv1, conv2 + the block's input
            y1 = conv(i, h, None)
            h = conv(i + 1, y1, h)
            i += 2
        hidden = conv(twin.n_body - 1, h, None)
        p = conv(twin.n_body + 1, conv(twin.n_body, hidden, None), None)          # the policy stem
        neck = torch.zeros((n, 8, 8, 8), dtype=bf, device="cuda")
        assert L.az_nn_othello_conv_narrow(hidden.data_ptr(), twin.dual_w.data_ptr(), twin.dual_s.data_ptr(), twin.dual_b.data_ptr(),
                                           neck.data_ptr(), n, cnt, s) == 0
        out = outputs()
        assert L.az_nn_othello_heads(p.data_ptr(), neck.data_ptr(), C.byref(w.heads), out[0].data_ptr(), out[1].data_ptr(),
                                     out[2].data_ptr(), n, rows, cnt, s) == 0
        torch.cuda.synchronize()
        return out

    assert twin.n_body == 8 and len(twin.layers) == 10 and w.n_body == 8 and w.n_convs == 10
    dense_m, dense_h = by_model(None, None), by_hand(None, None)
    for a, b in zip(dense_m, dense_h):
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert dense_m[0].std().item() > 1e-4 and (dense_m[0].sum(1) - 1).abs().max().item() < 1e-5
    rows = torch.tensor([7, 3, 20, 12], dtype=torch.int32, device="cuda")
    cnt = _count(torch, 4)
    comp_m, comp_h = by_model(rows.data_ptr(), cnt.data_ptr()), by_hand(rows.data_ptr(), cnt.data_ptr())
    idx = rows.long()
    rest = torch.ones(n, dtype=torch.bool, device="cuda"); rest[idx] = False
    for a, b, full in zip(comp_m, comp_h, dense_m):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a[idx].view(torch.int32), full[idx].view(torch.int32))  # a sample does not depend on its place in the batch
        assert (a[rest] == 0).all()                                                # rows not named stay zero
