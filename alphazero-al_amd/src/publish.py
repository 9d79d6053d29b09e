"""Trained weights into a live evaluator, in place, as ONE launch: Connect4 (az_nn_publish_dev / az_nn_model_publish in
include/az_nn.h, csrc/publish_kernels.hip) and, in the second half of this file, Othello (az_nn_othello_publish_dev /
az_nn_model_publish_othello; `publish_othello`).

`FastConnect4Net.from_module(net)` builds a NEW inference twin from a module: about a hundred small torch operations, every
buffer allocated again, four device reads, a new az_nn_model - so every captured graph goes.  `publish(fast, source)`
writes the same layout function of the parameters into the buffers an EXISTING twin already has: the model handle, the
twin and every pointer baked into a captured graph stay valid.

    fast = FastConnect4Net.from_module(net)         # once
    ...                                             # train `net` in place (torch, ClipAdamW or a NativeLearner)
    fast.publish_from(net)                          # or learner.publish(fast), or FusedSearch.publish_weights()

The call waits for the device ONCE: the heads' three biases are kernel arguments of the evaluator, so the host has to see
them.  Everything else about the twin - the stem's folded tables included - is written by the device.

Opt-in; nothing else changes.  Anything that cannot be published is a ValueError with the reason: there is no silent
fallback.  Needs torch and src.abi only."""
import ctypes as C

import torch

from src.abi import MAX_BLOCKS, _stream, lib

CH, EMB, ORBITS = 64, 32, 24
HEADS = (("policy_norm_weight", "policy_head.norm.weight", (CH,)), ("row_gate_weight", "policy_head.row_gate.weight", (1, CH)),
         ("row_gate_bias", "policy_head.row_gate.bias", (1,)), ("policy_fc_weight", "policy_head.fc.weight", (CH, CH)),
         ("policy_fc_bias", "policy_head.fc.bias", (CH,)), ("policy_out_weight", "policy_head.out.weight", (1, CH)),
         ("policy_out_bias", "policy_head.out.bias", (1,)), ("pool_norm_weight", "dual_head.pool_norm.weight", (CH,)),
         ("pool_fc_weight", "dual_head.pool_fc.weight", (CH, CH)), ("pool_fc_bias", "dual_head.pool_fc.bias", (CH,)),
         ("norm_weight", "dual_head.norm.weight", (CH,)), ("fc_weight", "dual_head.fc.weight", (CH, CH)),
         ("fc_bias", "dual_head.fc.bias", (CH,)), ("out_norm_weight", "dual_head.out_norm.weight", (CH,)),
         ("value_out_weight", "dual_head.value_out.weight", (3, CH)), ("value_out_bias", "dual_head.value_out.bias", (3,)),
         ("aux_out_weight", "dual_head.aux_out.weight", (1, CH)), ("aux_out_bias", "dual_head.aux_out.bias", (1,)))
ATTN = (("prenorm_weight", "prenorm.weight", (CH,)), ("qkv_weight", "qkv_proj.weight", (3 * CH, CH)),
        ("gate_weight", "gate_proj.weight", (4, CH)), ("o_weight", "o_proj.weight", (CH, CH)),
        ("q_norm_weight", "q_norm.weight", (16,)), ("k_norm_weight", "k_norm.weight", (16,)))
STEM = (("piece_emb", "piece_emb.weight", (2, EMB)), ("pos_emb", "pos_emb.weight", (ORBITS, EMB)),
        ("stem_conv_weight", "hidden.0.weight", (CH, EMB, 3, 3)), ("stem_conv_bias", "hidden.0.bias", (CH,)))
BLOCK = (("block_norm_weight", "norm.weight", (CH,)), ("block_norm_bias", "norm.bias", (CH,)),
         ("block_conv_weight", "conv.weight", (CH, CH, 3, 3)), ("block_conv_bias", "conv.bias", (CH,)))


class PublishSrcC(C.Structure):
    """az_nn_publish_src (include/az_nn.h).  Passed by address to a c_void_p parameter: tests/test_abi_cpu.py fixes the
    number of entries of `abi.MIRRORS`, so this one has a table of its own here, as src/learner.py has for its two, and
    tests/test_publish_cpu.py holds its layout to the header."""
    _fields_ = ([(n, C.c_void_p) for n, _, _ in STEM] + [("n_blocks", C.c_int32)] +
                [(n, C.c_void_p * MAX_BLOCKS) for n, _, _ in BLOCK] + [(n, C.c_void_p) for n, _, _ in ATTN + HEADS])


MIRRORS = {"az_nn_publish_src": PublishSrcC}


def orbit_map():
    """orbit(cell) = 4 * (cell / 7) + min(cell % 7, 6 - cell % 7): the position table's row of every cell, as the kernel
    has it compiled in."""
    return [4 * (cell // 7) + min(cell % 7, 6 - cell % 7) for cell in range(42)]


def source_struct(net, fast):
    """The module's tensors as an az_nn_publish_src after every precondition -> (struct, the tensors it points at).
    ValueError with the reason otherwise."""
    sd = net.state_dict()
    n_blocks = 0
    while "hidden.%d.conv.weight" % (n_blocks + 2) in sd:
        n_blocks += 1
    if not 1 <= n_blocks <= MAX_BLOCKS or n_blocks != len(fast.res):
        raise ValueError("publish: the module has %d residual blocks, the twin %d (1 to %d can be published)" % (n_blocks, len(fast.res), MAX_BLOCKS))
    attn = "hidden.%d.attn." % (n_blocks + 2)
    named = [(field, name, shape, None) for field, name, shape in STEM]
    for k in range(n_blocks):
        named += [(field, "hidden.%d.%s" % (k + 2, name), shape, k) for field, name, shape in BLOCK]
    named += [(field, attn + name, shape, None) for field, name, shape in ATTN]
    named += [(field, name, shape, None) for field, name, shape in HEADS]
    device = fast.emb_own.device
    src, keep = PublishSrcC(), {}
    src.n_blocks = n_blocks
    for field, name, shape, k in named:
        t = sd.get(name)
        if t is None:
            raise ValueError("publish: the module has no tensor %r (the reference's Connect4 parameter names are needed)" % name)
        if tuple(t.shape) != shape:
            raise ValueError("publish: %s has shape %s, the evaluator's layout needs %s" % (name, tuple(t.shape), shape))
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("publish: %s must be a contiguous float32 CUDA tensor" % name)
        if t.device != device:
            raise ValueError("publish: %s is on %s, the twin on %s" % (name, t.device, device))
        if k is None:
            setattr(src, field, t.data_ptr())
        else:
            getattr(src, field)[k] = t.data_ptr()
        keep[name] = t
    om = sd.get("orbit_map")
    if om is None or om.numel() != 42:
        raise ValueError("publish: the module has no orbit_map of 42 cells")
    # a constant of the game: compared once per tensor, not per call (the comparison reads the device)
    seen = (om.data_ptr(), om._version)
    if fast.__dict__.get("_publish_orbit_ok") != seen:
        if om.reshape(-1).tolist() != orbit_map():
            raise ValueError("publish: the module's orbit_map is not 4 * (cell / 7) + min(cell % 7, 6 - cell % 7), which the kernel has compiled in")
        fast.__dict__["_publish_orbit_ok"] = seen
    return src, keep


def _twin_model(fast):
    if not getattr(fast, "hip", False) or not hasattr(fast, "native_model"):
        raise ValueError("publish: needs a FastConnect4Net on the all-HIP path (bf16, on a GPU, the reference's widths)")
    model = fast.native_model()
    if model is None:
        raise ValueError("publish: the twin has no native model (more than %d blocks)" % MAX_BLOCKS)
    return model


def publish(fast, source):
    """Writes the evaluator's layout of `source`'s parameters into `fast`'s existing buffers on torch's current stream and
    returns the three head biases (row_gate, policy out, aux out) as the device holds them in float32.

    fast: a `FastConnect4Net` on the all-HIP path.  source: a module with the reference's parameter names (every parameter
    float32, CUDA, contiguous, on the twin's device, the twin's number of blocks, the game's orbit_map) or a `NativeLearner`
    over such a module (then az_learn_publish reads the tensors the learner is bound to).

    Afterwards everything on `fast` that carries a bias holds the new value: the native model (created on demand),
    `_heads_w`, `p_gate_b_host` and the three one-element float32 buffers.  Waits for the stream once."""
    model = _twin_model(fast)
    learner = source if hasattr(source, "_handle") and hasattr(source, "net") else None
    net = learner.net if learner is not None else source
    src, keep = source_struct(net, fast)
    device = fast.emb_own.device
    slot = fast.__dict__.get("publish_slot")
    if slot is None:
        # a plain attribute, not a registered buffer: state_dict() stays what it was
        slot = fast.__dict__["publish_slot"] = torch.zeros(4, dtype=torch.float32, device=device)
    L = lib()
    with torch.cuda.device(device):
        if learner is not None:
            learner._require_open()
            learner._sync()
            rc = L.az_learn_publish(learner._handle, model, slot.data_ptr(), _stream())
        else:
            rc = L.az_nn_model_publish(model, C.byref(src), slot.data_ptr(), _stream())
        if rc != 0:
            raise ValueError("publish: the library refused the call (%d): %s" % (rc, L.az_last_error().decode() if learner is not None
                                                                                 else "az_nn_model_publish"))
        out = (C.c_float * 3)()
        if L.az_nn_model_head_biases(model, C.byref(out)) != 0:
            raise RuntimeError("az_nn_model_head_biases failed")
        # the float32 buffers follow on the device, the host copies from what the model now carries.  A twin built from a
        # float32 module on its own device holds these three as ALIASES of the module's parameters (`.to()` of a tensor
        # that already fits returns it): such a buffer already has the value, and writing it would count as a change of
        # the module (its version counter)
        for i, (buf, name) in enumerate(((fast.p_gate_b, "policy_head.row_gate.bias"), (fast.p_out_b, "policy_head.out.bias"),
                                         (fast.d_aux_b, "dual_head.aux_out.bias"))):
            if buf.data_ptr() != keep[name].data_ptr():
                buf.copy_(slot[i:i + 1])
    del keep
    biases = (float(out[0]), float(out[1]), float(out[2]))
    hw = fast._heads_w
    hw.p_gate_b, hw.p_out_b, hw.d_aux_b = biases
    fast.p_gate_b_host = biases[0]
    return biases


# ---------------------------------------------------------------------------------------------------------------- Othello
#
# `FastOthelloNet(net)` packs eleven convolution weights through permute chains, folds a dozen BatchNorms, transposes two
# 512 x 512 matrices and reads three biases back; `native_model()` then makes a new az_nn_model.  `publish_othello(fast)`
# writes the same function of `fast.net`'s parameters AND BatchNorm buffers into the arrays the twin and its model already
# have.  The BatchNorm affines are computed in correctly rounded float32 steps (az_nn.h), which torch's `sqrt` is not
# everywhere: they agree with `_bn_affine` within a few ulp, not in bytes.

O_CH, O_FC, OTHELLO_MAX_CONVS = 256, 512, 16
BN_FIELDS = (("weight", "weight"), ("bias", "bias"), ("mean", "running_mean"), ("var", "running_var"))
# (field of az_nn_othello_publish_src, state dict name, shape) of everything that is not a convolution of the chain
O_TENSORS = (("piece_emb", "piece_emb.weight", (2, EMB)), ("pos_emb", "pos_emb.weight", (10, EMB)), ("legal_emb", "legal_emb.weight", (2, EMB)),
             ("dual_weight", "dual_head.stem.0.weight", (8, O_CH, 3, 3)),
             ("board_weight", "policy_head.board_out.weight", (1, O_CH, 1, 1)), ("board_bias", "policy_head.board_out.bias", (1,)),
             ("pass_norm_weight", "policy_head.pass_norm.weight", (O_CH,)), ("pass_fc_weight", "policy_head.pass_fc.weight", (1, O_CH)),
             ("pass_fc_bias", "policy_head.pass_fc.bias", (1,)), ("v_conv_weight", "dual_head.value_out.0.weight", (8, 8, 3, 3)),
             ("v_fc_weight", "dual_head.value_out.5.weight", (3, 72)), ("v_fc_bias", "dual_head.value_out.5.bias", (3,)),
             ("a_fc_weight", "dual_head.aux_out.1.weight", (O_FC, O_FC)), ("a_fc_bias", "dual_head.aux_out.1.bias", (O_FC,)),
             ("a_norm_weight", "dual_head.aux_out.2.weight", (O_FC,)), ("a_out_weight", "dual_head.aux_out.5.weight", (1, O_FC)),
             ("a_out_bias", "dual_head.aux_out.5.bias", (1,)))
O_NORMS = (("dual_bn", "dual_head.stem.1", 8), ("v_bn", "dual_head.value_out.1", 8))
O_BIASES = ("policy_head.board_out.bias", "policy_head.pass_fc.bias", "dual_head.aux_out.5.bias")


class OthelloBnSrcC(C.Structure):
    """az_nn_othello_bn_src (include/az_nn.h)."""
    _fields_ = [(n, C.c_void_p) for n, _ in BN_FIELDS]


class OthelloPublishSrcC(C.Structure):
    """az_nn_othello_publish_src (include/az_nn.h).  Passed by address to a c_void_p parameter, as PublishSrcC is;
    tests/test_publish_othello_cpu.py holds its layout to the header."""
    _fields_ = ([(n, C.c_void_p) for n in ("piece_emb", "pos_emb", "legal_emb")] + [("n_body", C.c_int32), ("n_convs", C.c_int32), ("bn_eps", C.c_float)] +
                [("conv_weight", C.c_void_p * OTHELLO_MAX_CONVS), ("conv_pre", OthelloBnSrcC * OTHELLO_MAX_CONVS),
                 ("conv_post", OthelloBnSrcC * OTHELLO_MAX_CONVS), ("dual_weight", C.c_void_p), ("dual_bn", OthelloBnSrcC)] +
                [(n, C.c_void_p) for n in ("board_weight", "board_bias", "pass_norm_weight", "pass_fc_weight", "pass_fc_bias", "v_conv_weight")] +
                [("v_bn", OthelloBnSrcC)] +
                [(n, C.c_void_p) for n in ("v_fc_weight", "v_fc_bias", "a_fc_weight", "a_fc_bias", "a_norm_weight", "a_out_weight", "a_out_bias")])


# a table of their own: tests/test_publish_cpu.py fixes `MIRRORS` above at its one entry
OTHELLO_MIRRORS = {"az_nn_othello_bn_src": OthelloBnSrcC, "az_nn_othello_publish_src": OthelloPublishSrcC}


def othello_orbit_map():
    """The reference's 64-entry orbit table in closed form, as the kernel has it compiled in: fold the board onto one
    octant, number the triangle a <= b <= 3 row by row."""
    out = []
    for cell in range(64):
        fr, fc = min(cell // 8, 7 - cell // 8), min(cell % 8, 7 - cell % 8)
        a, b = min(fr, fc), max(fr, fc)
        out.append((0, 4, 7, 9)[a] + b - a)
    return out


def othello_conv_names(n_blocks):
    """[(convolution weight, BatchNorm in front or None, BatchNorm behind or None, c_in)] in the order of
    az_nn_othello_weights.conv, as state dict prefixes."""
    out = [("stem.0.weight", None, "stem.1", EMB)]
    for k in range(n_blocks):
        out += [("stem.%d.conv1.weight" % (3 + k), "stem.%d.norm1" % (3 + k), None, O_CH),
                ("stem.%d.conv2.weight" % (3 + k), "stem.%d.norm2" % (3 + k), None, O_CH)]
    out.append(("stem.%d.weight" % (3 + n_blocks), None, "stem.%d" % (4 + n_blocks), O_CH))
    return out + [("policy_head.stem.0.weight", None, "policy_head.stem.1", O_CH), ("policy_head.stem.4.weight", None, "policy_head.stem.5", O_CH)]


def othello_source_struct(fast):
    """`fast.net`'s tensors as an az_nn_othello_publish_src after every precondition -> (struct, the tensors it points at).
    ValueError with the reason otherwise."""
    net = fast.net
    sd = net.state_dict()
    n_blocks = 0
    while "stem.%d.conv1.weight" % (3 + n_blocks) in sd:
        n_blocks += 1
    if 2 * n_blocks + 2 != fast.n_body or fast.n_body + 2 > OTHELLO_MAX_CONVS:
        raise ValueError("publish_othello: the module has %d residual blocks, the twin's body %d convolutions (2 per block and 2)"
                         % (n_blocks, fast.n_body))
    device = fast.embed_table.device
    keep = {}

    def tensor(name, shape):
        t = sd.get(name)
        if t is None:
            raise ValueError("publish_othello: the module has no tensor %r (the reference's Othello parameter names are needed)" % name)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("publish_othello: %s has shape %s, the evaluator's layout needs %s" % (name, tuple(t.shape), tuple(shape)))
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("publish_othello: %s must be a contiguous float32 CUDA tensor" % name)
        if t.device != device:
            raise ValueError("publish_othello: %s is on %s, the twin on %s" % (name, t.device, device))
        keep[name] = t
        return t.data_ptr()

    def norm(into, prefix, channels):
        for field, key in BN_FIELDS:
            setattr(into, field, tensor("%s.%s" % (prefix, key), (channels,)))

    src = OthelloPublishSrcC()
    src.n_body, src.n_convs = fast.n_body, fast.n_body + 2
    for field, name, shape in O_TENSORS:
        setattr(src, field, tensor(name, shape))
    for i, (weight, pre, post, c_in) in enumerate(othello_conv_names(n_blocks)):
        src.conv_weight[i] = tensor(weight, (O_CH, c_in, 3, 3))
        if pre is not None:
            norm(src.conv_pre[i], pre, c_in)
        if post is not None:
            norm(src.conv_post[i], post, O_CH)
    for field, prefix, channels in O_NORMS:
        norm(getattr(src, field), prefix, channels)
    # one epsilon for every BatchNorm: it travels as one float
    eps = None
    for name, m in net.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            if eps is None:
                eps = float(m.eps)
            elif float(m.eps) != eps:
                raise ValueError("publish_othello: %s has eps %g, the BatchNorms before it %g (one common eps can be published)" % (name, m.eps, eps))
    if eps is None:
        raise ValueError("publish_othello: the module has no BatchNorm")
    src.bn_eps = eps
    om = sd.get("orbit_map")
    if om is None or om.numel() != 64:
        raise ValueError("publish_othello: the module has no orbit_map of 64 cells")
    # a constant of the game: compared once per tensor version, not per call (the comparison reads the device)
    seen = (om.data_ptr(), om._version)
    if fast.__dict__.get("_publish_orbit_ok") != seen:
        if om.reshape(-1).tolist() != othello_orbit_map():
            raise ValueError("publish_othello: the module's orbit_map is not the reference's table, which the kernel has compiled in")
        fast.__dict__["_publish_orbit_ok"] = seen
    return src, keep


def publish_othello(fast, source=None):
    """Writes the evaluator's layout of `fast.net`'s parameters and BatchNorm buffers into `fast`'s existing arrays on
    torch's current stream and returns the three head biases (board_out, pass_fc, aux_out[5]) as the device holds them.

    fast: a `FastOthelloNet`; its native model is created on demand.  source: `fast.net` itself, or None.  The twin's torch
    route reads the heads straight from `fast.net` and its native model aliases that module's parameters, so another
    module would leave the twin half old: `fast.net.load_state_dict(other.state_dict())` first.

    Afterwards `fast.board_b` and the three floats of `fast._model_w.heads` hold the new values.  Waits for the stream once."""
    if not hasattr(fast, "native_model") or not hasattr(fast, "embed_table") or not hasattr(fast, "n_body"):
        raise ValueError("publish_othello: needs a FastOthelloNet")
    if source is not None and source is not fast.net:
        raise ValueError("publish_othello: the source must be the twin's own module (fast.net): its torch route and its native model "
                         "read that module's parameters, so load_state_dict into fast.net first")
    src, keep = othello_source_struct(fast)
    model = fast.native_model()
    device = fast.embed_table.device
    slot = fast.__dict__.get("publish_slot")
    if slot is None:
        slot = fast.__dict__["publish_slot"] = torch.zeros(4, dtype=torch.float32, device=device)
    L = lib()
    with torch.cuda.device(device):
        rc = L.az_nn_model_publish_othello(model, C.byref(src), slot.data_ptr(), _stream())
    if rc != 0:
        raise ValueError("publish_othello: the library refused the call (%d): az_nn_model_publish_othello" % rc)
    del keep
    out = (C.c_float * 3)()
    if L.az_nn_model_othello_head_biases(model, C.byref(out)) != 0:
        raise RuntimeError("az_nn_model_othello_head_biases failed")
    biases = (float(out[0]), float(out[1]), float(out[2]))
    fast.board_b = biases[0]
    hw = fast._model_w.heads
    hw.board_b, hw.pass_fc_b, hw.a_out_b = biases
    return biases
