"""Stand-alone timing of the evaluator kernels on synthetic activations (GPU box only).

    python tools/probe_nn.py                  # all kernels, HIP-event timings at 32768 leaves
    python tools/probe_nn.py conv 0 5         # only the residual conv block, debug mode 0, 5 launches
                                              # (the form to put under rocprofv3 --pmc ...)
    python tools/probe_nn.py dump DIR         # outputs of az_nn_attn_block / az_nn_heads / az_nn_attn_heads on seeded
                                              # inputs as DIR/*.npy: two builds of the library must agree bit for bit
    python tools/probe_nn.py stem_conv        # the fused stem + first block against its two launches (PROBE_B leaves)
Debug modes of the conv block (az_nn_debug): 1 skips the MFMA phase and its epilogue, 2 skips the
epilogue and the stores, 3 both: what is left is staging + GroupNorm.
"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphazero-al_amd"))
from src.fast_net import FastConnect4Net, Positions, glue  # noqa: E402
from src.az_net import Connect4Net  # noqa: E402

L = glue()


def random_positions(B, gen):
    """B positions as az_nn_positions: random column heights and colours (not necessarily reachable), either side to
    move, either symmetry id; the tensors are returned with the structure to keep them alive"""
    h = torch.randint(0, 7, (B, 7), device="cuda", generator=gen)
    colour = torch.randint(0, 2, (B, 7, 6), device="cuda", generator=gen)
    bb1 = torch.zeros(B, dtype=torch.int64, device="cuda")
    bb2 = torch.zeros_like(bb1)
    for c in range(7):
        for k in range(6):
            on = h[:, c] > k
            bb1 |= (on & (colour[:, c, k] == 1)).long() << (7 * c + k)
            bb2 |= (on & (colour[:, c, k] == 0)).long() << (7 * c + k)
    turn = (torch.randint(0, 2, (B,), device="cuda", generator=gen) * 2 - 1).int()
    sym = torch.randint(0, 2, (B,), device="cuda", generator=gen).int()
    keep = (bb1, bb2, turn, sym)
    return Positions(*[t.data_ptr() for t in keep]), keep


def dump(outdir):
    """The three kernels that end the evaluator on the inputs of tests/test_attn_heads_gpu.py (checkpoint weights and
    the q-norm weight x 40, with and without a mask, compact lists): every output array, NaN canaries included, as
    raw bits.  The kernels have no atomics, so the files of two builds are equal byte for byte or arithmetic moved."""
    import numpy as np
    from src import az_net
    os.makedirs(outdir, exist_ok=True)
    wts = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                               "g7_checkpoint_weights.npz"))
    mod = az_net.Connect4Net(device="cuda").eval()
    az_net.load_reference_weights(mod, {k: wts[k] for k in wts.files})
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(tag, fast, x, mask, B, rows=None, n_rows=None):
        mp = None if mask is None else mask.data_ptr()
        rp = None if rows is None else rows.data_ptr()
        npp = None if n_rows is None else n_rows.data_ptr()
        att = (fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(), fast.kn_w.data_ptr(), fast.o_w.data_ptr())
        y = torch.full(x.shape, float("nan"), device="cuda", dtype=x.dtype)
        assert L.az_nn_attn_block(x.data_ptr(), *att, y.data_ptr(), B, 1e-5, npp, s) == 0
        np.save(os.path.join(outdir, tag + "_attn_y.npy"), y.view(torch.int16).cpu().numpy())
        y = torch.nan_to_num(y)          # rows past a compact count: the heads never read them, keep them defined
        for name in ("heads", "attn_heads"):
            out = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
            ptrs = [t.data_ptr() for t in out]
            if name == "heads":
                assert L.az_nn_heads(y.data_ptr(), C.byref(fast._heads_w), mp, *ptrs, B, 1e-5, rp, npp, s) == 0
            else:
                assert L.az_nn_attn_heads(x.data_ptr(), *att, C.byref(fast._heads_w), mp, *ptrs, B, 1e-5, rp, npp, s) == 0
            torch.cuda.synchronize()
            for t, what in zip(out, ("probs", "wdl", "ml")):
                np.save(os.path.join(outdir, "%s_%s_%s.npy" % (tag, name, what)), t.view(torch.int32).cpu().numpy())

    for sharp in (False, True):
        fast = FastConnect4Net.from_module(mod)
        if sharp:       # scores outside the bound: the max-subtracting branch of the attention's softmax runs
            fast.qn_w = (fast.qn_w.float() * 40.0).to(fast.qn_w.dtype).contiguous()
        gen = torch.Generator(device="cuda").manual_seed(11)
        for B in (1, 3, 777, 4099, 26368):
            x = (torch.randn((B, 42, 64), device="cuda", generator=gen) * 1.5).to(torch.bfloat16)
            mask = torch.rand((B, 7), device="cuda", generator=gen) > 0.25
            mask[:, 3] = True
            m8 = mask.to(torch.uint8).contiguous()
            for mk in (m8, None):
                run("b%d_sharp%d_mask%d" % (B, sharp, mk is not None), fast, x, mk, B)
    # the fused stem + first residual block and the two launches it replaces: y, NaN canary behind a compact count
    fast = FastConnect4Net.from_module(mod)
    gen = torch.Generator(device="cuda").manual_seed(14)
    blk = [getattr(fast, n).data_ptr() for n in fast.res[0]]
    tabs = (fast.stem_frag.data_ptr(), fast.stem_pmap.data_ptr())
    for B, live in ((1, None), (3, None), (777, None), (4099, None), (26368, None), (9, 5), (4099, 3001), (26368, 20000)):
        pos, keep = random_positions(B, gen)
        rows = n_rows = rp = npp = None
        if live is not None:
            rows = torch.randperm(B, device="cuda", generator=gen).to(torch.int32).contiguous()
            n_rows = torch.tensor([live], dtype=torch.int64, device="cuda")
            rp, npp = rows.data_ptr(), n_rows.data_ptr()
        ys = [torch.full((B, 42, 64), float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(3)]
        assert L.az_nn_stem_conv_block_positions(C.byref(pos), *tabs, *blk, ys[0].data_ptr(), B, 1e-5, rp, npp, s) == 0
        assert L.az_nn_stem_folded_positions(C.byref(pos), *tabs, ys[1].data_ptr(), B, rp, npp, s) == 0
        assert L.az_nn_conv_block(ys[1].data_ptr(), 64, *blk, 1, ys[2].data_ptr(), B, 1e-5, npp, s) == 0
        torch.cuda.synchronize()
        tag = "b%d" % B if live is None else "compact%d_%d" % (B, live)
        np.save(os.path.join(outdir, tag + "_stem_conv_y.npy"), ys[0].view(torch.int16).cpu().numpy())
        np.save(os.path.join(outdir, tag + "_stem_then_conv_y.npy"), ys[2].view(torch.int16).cpu().numpy())
    gen = torch.Generator(device="cuda").manual_seed(12)
    for B, live in ((9, 5), (4099, 3001), (26368, 20000)):
        x = (torch.randn((B, 42, 64), device="cuda", generator=gen) * 1.5).to(torch.bfloat16)
        rows = torch.randperm(B, device="cuda", generator=gen).to(torch.int32).contiguous()
        mask = torch.rand((B, 7), device="cuda", generator=gen) > 0.25
        mask[:, 0] = True
        n_rows = torch.tensor([live], dtype=torch.int64, device="cuda")
        run("compact%d_%d" % (B, live), fast, x, mask.to(torch.uint8).contiguous(), B, rows, n_rows)
    print("dumped %d arrays to %s" % (len(os.listdir(outdir)), outdir))


if len(sys.argv) > 2 and sys.argv[1] == "dump":
    dump(sys.argv[2])
    sys.exit(0)

B = int(os.environ.get("PROBE_B", 32768))
bf = torch.bfloat16
dev = "cuda"
x = torch.randn(B, 42, 64, device=dev).to(bf)
y = torch.empty_like(x)
x32 = torch.randn(B, 42, 32, device=dev).to(bf)
w = (torch.randn(64, 64, 3, 3, device=dev) * 0.05).to(bf).contiguous(memory_format=torch.channels_last)
w32 = (torch.randn(64, 32, 3, 3, device=dev) * 0.05).to(bf).contiguous(memory_format=torch.channels_last)
b = torch.randn(64, device=dev).to(bf)
g = torch.ones(64, device=dev).to(bf)
be = torch.zeros(64, device=dev).to(bf)
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
net = FastConnect4Net.from_module(Connect4Net(device=dev).eval())
probs = torch.empty(B, 7, device=dev)
wdl = torch.empty(B, 3, device=dev)
ml = torch.empty(B, device=dev)
mask = torch.ones(B, 7, dtype=torch.uint8, device=dev)


def conv():
    L.az_nn_conv_block(x.data_ptr(), 64, w.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), 1, y.data_ptr(), B, 1e-5, None, s)


def stem():
    L.az_nn_conv_block(x32.data_ptr(), 32, w32.data_ptr(), b.data_ptr(), None, None, 0, y.data_ptr(), B, 1e-5, None, s)


def attn():
    L.az_nn_attn_block(x.data_ptr(), net.pre_w.data_ptr(), net.qkvg_w.data_ptr(), net.qn_w.data_ptr(),
                       net.kn_w.data_ptr(), net.o_w.data_ptr(), y.data_ptr(), B, 1e-5, None, s)


def heads():
    L.az_nn_heads(x.data_ptr(), C.byref(net._heads_w), mask.data_ptr(), probs.data_ptr(), wdl.data_ptr(), ml.data_ptr(),
                  B, 1e-5, None, None, s)


feat = (torch.rand(B, 3, 6, 7, device=dev) > 0.5).float()


def stem_embed():
    L.az_nn_stem_embed(feat.data_ptr(), net.emb_own.data_ptr(), net.emb_opp.data_ptr(), net.pos.data_ptr(),
                       w32.data_ptr(), b.data_ptr(), y.data_ptr(), B, None, None, s)


def stem_folded():
    L.az_nn_stem_folded(feat.data_ptr(), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), y.data_ptr(), B, None, None, s)


def attn_heads():
    L.az_nn_attn_heads(x.data_ptr(), net.pre_w.data_ptr(), net.qkvg_w.data_ptr(), net.qn_w.data_ptr(), net.kn_w.data_ptr(),
                       net.o_w.data_ptr(), C.byref(net._heads_w), mask.data_ptr(), probs.data_ptr(), wdl.data_ptr(),
                       ml.data_ptr(), B, 1e-5, None, None, s)


pos_c, pos_keep = random_positions(B, torch.Generator(device="cuda").manual_seed(5))


def stem_pos():
    L.az_nn_stem_folded_positions(C.byref(pos_c), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), x.data_ptr(), B, None, None, s)


def stem_then_conv():
    stem_pos()
    conv()


def stem_conv():
    L.az_nn_stem_conv_block_positions(C.byref(pos_c), net.stem_frag.data_ptr(), net.stem_pmap.data_ptr(), w.data_ptr(), b.data_ptr(),
                                      g.data_ptr(), be.data_ptr(), y.data_ptr(), B, 1e-5, None, None, s)


KERNELS = {"stem_pos": stem_pos, "stem_then_conv": stem_then_conv, "stem_conv": stem_conv, "conv": conv, "stem": stem, "stem_embed": stem_embed, "stem_folded": stem_folded, "attn": attn, "heads": heads,
           "attn_heads": attn_heads}


def timed(fn, n=20):
    for _ in range(3):
        fn()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def stem_conv_report():
    """the fused kernel against the two launches it replaces, and where its cycles go (az_nn_debug bit 4)"""
    import numpy as np
    L.az_nn_debug(0)
    t = {k: timed(KERNELS[k]) for k in ("stem_pos", "conv", "stem_then_conv", "stem_conv")}
    print("at %d leaves: stem (positions) %.1f us, block %.1f us, both %.1f us; fused %.1f us"
          % (B, t["stem_pos"], t["conv"], t["stem_then_conv"], t["stem_conv"]))
    L.az_nn_debug(16)
    stem_conv()
    torch.cuda.synchronize()
    buf = np.zeros(2048 * 8, dtype=np.uint64)
    L.az_nn_conv_profile(buf.ctypes.data, buf.size)
    L.az_nn_debug(0)
    ph = buf.reshape(2048, 8)[:, :7].astype(np.float64)
    names = ("P1 norm->img", "barrier 1", "MFMA+epilogue", "wait staged tile", "barrier 2", "P3 store", "P0 stem")
    for k, nm in enumerate(names):
        print("   fused %-18s mean %9.0f ticks/wave (%4.1f%%)" % (nm, ph[:, k].mean(), 100 * ph[:, k].mean() / ph.sum(1).mean()))
    return t


if len(sys.argv) > 1 and sys.argv[1] == "stem_conv" and len(sys.argv) == 2:
    stem_conv_report()
elif len(sys.argv) > 1:
    fn = KERNELS[sys.argv[1]]
    L.az_nn_debug(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    for _ in range(int(sys.argv[3]) if len(sys.argv) > 3 else 5):
        fn()
    torch.cuda.synchronize()
    if os.environ.get("PROBE_TIME"):
        print("%-20s %7.1f us at %d leaves" % (sys.argv[1], timed(fn), B))
else:
    for mode, name in ((0, "full"), (1, "no MFMA phase"), (2, "no epilogue/store"), (3, "staging + norm only")):
        L.az_nn_debug(mode)
        print("conv %-22s %7.1f us" % (name, timed(conv)))
    L.az_nn_debug(16)
    print("conv with phase stamps      %7.1f us" % timed(conv))
    import numpy as np
    buf = np.zeros(2048 * 8, dtype=np.uint64)
    L.az_nn_conv_profile(buf.ctypes.data, buf.size)
    ph = buf.reshape(2048, 8)[:, :6].astype(np.float64)
    names = ("P1 norm->img", "barrier 1", "MFMA+epilogue", "wait staged tile", "barrier 2", "P3 store")
    tot = ph.sum(1).mean()
    for k, nm in enumerate(names):
        print("   %-18s mean %9.0f cycles/wave (%4.1f%%)  min %9.0f max %9.0f" % (nm, ph[:, k].mean(), 100 * ph[:, k].mean() / tot, ph[:, k].min(), ph[:, k].max()))
    print("   total %9.0f cycles per wave (memtime ticks, 100 MHz?)" % tot)
    L.az_nn_debug(0)
    for name in ("stem", "stem_embed", "attn", "heads"):
        print("%-27s %7.1f us" % (name, timed(KERNELS[name])))
    stem_conv_report()
