"""What the GPU tests of the four training pieces (test_train_block_gpu.py, test_train_attn_gpu.py, test_train_stem_gpu.py,
test_train_heads_gpu.py) share: the built package, tensors between guard regions, the comparison against a piece's
reference module, the struct helpers of the argument-error tests, and the Connect4 module, batches and baselines of the
`train_step` tests.  A plain module: no fixture and no pytest setting lives here."""
import importlib
import os
import sys

import numpy as np

import train_loss_ref as TR
from test_train_loss_cpu import golden_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
AZ_ERR_ARG = 1
GUARD = 256
FILL = 0xA5
# the key a `src` module gets in the env dict
KEYS = dict(train_block="TB", train_attn="TA", train_stem="TS", train_heads="TH", train_loss="TL", az_net="NET", optim="O")
# (name in `module(adopt=...)`, the env key of its module, the function, what it returns on the Connect4 module)
ADOPTIONS = (("blocks", "TB", "adopt_blocks", 3), ("attention", "TA", "adopt_attention", 1), ("stem", "TS", "adopt_stem", 1))


def load_env(modules):
    """Builds the package and imports `src.abi` and the named `src` modules -> dict(torch, L, abi, and one entry per module
    under its key in KEYS).  The body of every `env` fixture."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import abi
    return dict(torch=torch, L=abi.lib(), abi=abi, **{KEYS[m]: importlib.import_module("src." + m) for m in modules})


# ---------------------------------------------------------------------------------------- tensors between guard regions

class Slab:
    """Every tensor of a call in one byte slab on the device, each 16-byte aligned with 256 guard bytes before and after;
    outputs start as the fill pattern."""

    def __init__(self, torch, inputs, out_bytes):
        self.torch, self.at, self.size = torch, {}, {}
        off = GUARD
        for name, nbytes in [(k, v.nbytes) for k, v in inputs.items() if v is not None] + list(out_bytes.items()):
            self.at[name], self.size[name] = off, nbytes
            off = (off + nbytes + 15) // 16 * 16 + GUARD
        self.host = np.full(off, FILL, np.uint8)
        for k, v in inputs.items():
            if v is not None:
                self.host[self.at[k]:self.at[k] + v.nbytes] = np.ascontiguousarray(v).view(np.uint8).ravel()
        self.dev = torch.empty(off, dtype=torch.uint8, device="cuda")
        assert self.dev.data_ptr() % 16 == 0
        self.upload()

    def upload(self):
        self.dev.copy_(self.torch.from_numpy(self.host))

    def ptr(self, name, shift=0):
        return self.dev.data_ptr() + self.at[name] + shift if name in self.at else None

    def untouched_outside(self, image, written):
        """Everything but the named outputs - guards, inputs, the other outputs' fill - is byte for byte what it was."""
        mask = np.ones(image.size, bool)
        for name in written:
            mask[self.at[name]:self.at[name] + self.size[name]] = False
        return np.array_equal(image[mask], self.host[mask])

    def get(self, image, name, shape):
        return image[self.at[name]:self.at[name] + self.size[name]].view(np.float32).reshape(shape).copy()


def held(R, got, ref, own, what, quantities=None):
    """Every quantity of `got` within `R.bound` of what float32 torch deviates (`own`) from the reference `ref`; R is the
    piece's reference module.  Prints each figure and its share of the bound before it asserts."""
    quantities = R.QUANTITIES if quantities is None else quantities
    devs = R.deviations(got, ref, quantities)
    width = max(len(q) for q in quantities)
    for q in quantities:
        print("%s %-*s kernel %.3e  torch %.3e  bound %.3e  share %.2f" % (what, width, q, devs[q], own[q], R.bound(own[q]),
                                                                           devs[q] / R.bound(own[q])))
    for q in quantities:
        assert devs[q] <= R.bound(own[q]), (what, q, devs[q], own[q])
    return devs


# ---------------------------------------------------------------------------------------- ctypes structs with one field changed

def fields(struct):
    return {f[0]: getattr(struct, f[0]) for f in struct._fields_}


def swap(struct, **kw):
    return type(struct)(**dict(fields(struct), **kw))


# ---------------------------------------------------------------------------------------- the Connect4 module under train_step

def module(env, dtype, device, adopt=(), stem_bias=False):
    """The seeded Connect4 module with the reference's optimiser, its heads' output weights (which the reference zeroes)
    moved off zero, and - with `stem_bias` - the first convolution's bias too.  `adopt`: which of "blocks", "attention",
    "stem" get their kernels, in that order."""
    torch = env["torch"]
    torch.manual_seed(11)
    net = env["NET"].Connect4Net(device="cpu")
    with torch.no_grad():
        for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
            lin.weight.normal_(0, 0.05)
        if stem_bias:
            net.hidden[0].bias.normal_(0, 0.1)
    net = net.to(dtype).to(device)
    net.opt = torch.optim.AdamW(env["O"].reference_param_groups(net, 1e-3), lr=1e-3, weight_decay=1e-2)
    net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
    for name, key, fn, count in ADOPTIONS:
        if name in adopt:
            assert getattr(env[key], fn)(net) == count
    return net


_LOADERS = {}


def loaders(env):
    """Three batches of 64 rows of fixture G16's Connect4 batch, under "cpu" and "cuda"."""
    if not _LOADERS:
        torch = env["torch"]
        batch = tuple(torch.from_numpy(x) for x in golden_batch("c4"))
        _LOADERS["cpu"] = [tuple(t[a:a + 64] for t in batch) for a in (0, 64, 32)]
        _LOADERS["cuda"] = [tuple(t.cuda() for t in b) for b in _LOADERS["cpu"]]
    return _LOADERS


def baselines(env, stem_bias=False):
    """`train_step` over the three batches on the unadopted float32 twin on the GPU ("twin") and the float64 net on the CPU
    ("exact").  The body of the `baselines` fixtures."""
    torch, TL = env["torch"], env["TL"]
    out = {}
    for which, dtype, device, route in (("twin", torch.float32, "cuda", "kernel"), ("exact", torch.float64, "cpu", "torch")):
        net = module(env, dtype, device, stem_bias=stem_bias)
        out[which] = TL.train_step(net, loaders(env)[device], lambda b: b, n_epochs=1, route=route, **dict(TR.CONFIGS["b"]))
    return out
