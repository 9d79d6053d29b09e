"""The native learner: a Connect4 training batch - or a whole epoch of them - as ONE call into the C ABI.

`adopt_all` + `train_step(route="kernel")` + `ClipAdamW` already run every piece of a batch as the project's kernels, but
Python drives them: four autograd nodes, an instance-attribute forward per module, a workspace per node, the optimiser's
pass over forty tensors.  `NativeLearner` hands the same launches, in the same order, on the same bytes, to
az_learn_dev_step / az_learn_dev_epoch (include/az_train.h, csrc/learn_driver.hip): the handle owns every buffer a batch
needs, each backward writes straight into one flat gradient tensor, and with dropout on all masks of a batch come from
one launch (k_learn_keep) of the device generator instead of torch's.

    learner = NativeLearner(net, max_rows=1024)             # net: az_net.Connect4Net or the reference's CNN, on a GPU
    stats = learner.train_step(buffer.sample(512), n_epochs=10)     # the 6-tuple of train_loss.train_step

Without dropout the parameters, moments and step counters after a batch are byte for byte what the Python route leaves,
and `net.opt` (a `ClipAdamW`) can take over at any batch: the two routes may alternate.  With dropout the DISTRIBUTION of
the masks is the same, the RANDOM STREAM is the learner's own (seed, batch number).

Opt-in; nothing else changes.  Anything the learner cannot take is a ValueError with the reason: there is no silent
fallback.  Needs torch and src.abi only: a learner does not import the engine."""
import ctypes as C

import torch

from src import optim as O
from src import train_attn as TA
from src import train_block as TB
from src import train_heads as TH
from src import train_loss as TL
from src import train_stem as TS
from src.abi import ReplayBatchC, _stream, check, lib
from src.replay import ReplayBatches, replay_tensors_c

MAX_BLOCKS = 8                          # AZ_LEARN_MAX_BLOCKS
ROLE_PIECE_EMB, ROLE_POS_EMB, ROLE_STEM_CONV_WEIGHT, ROLE_STEM_CONV_BIAS = 0, 1, 2, 3
ROLE_BLOCK, ROLE_ATTN, ROLE_HEADS, ROLES = 4, 36, 42, 60
KEEP_ATTN, KEEP_POLICY, KEEP_POOL = 8, 9, 10    # the dropout streams' tensor ids; block k is k
MAX_LEARN_ROWS = 1 << 20


class LearnConfigC(C.Structure):
    """az_learn_config (include/az_train.h).  Passed by address to a c_void_p parameter, as is the one below:
    tests/test_abi_cpu.py fixes the number of entries of `abi.MIRRORS`, so these two have a table of their own here and
    tests/test_learner_cpu.py holds their layouts to the header."""
    _fields_ = [("max_rows", C.c_int64), ("n_blocks", C.c_int32), ("max_workgroups", C.c_int32), ("eps_block", C.c_float),
                ("eps_attn", C.c_float), ("eps_heads", C.c_float), ("max_norm", C.c_float), ("p_block", C.c_double),
                ("p_attn", C.c_double), ("p_policy", C.c_double), ("p_pool", C.c_double), ("seed", C.c_uint64)]


class LearnOutC(C.Structure):
    """az_learn_out (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("sums", "batches", "entropy", "losses", "counts", "grad_norm", "keep_blocks")] + \
               [("keep_block_stride", C.c_int64)] + [(n, C.c_void_p) for n in ("keep_attn", "keep_policy", "keep_pool")] + \
               [("batch", ReplayBatchC)]


MIRRORS = {"az_learn_config": LearnConfigC, "az_learn_out": LearnOutC}


class _DeviceMemory:
    """Memory the library owns, as torch's `as_tensor` takes it (the CUDA array interface): no copy."""

    def __init__(self, address, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(address), False),
                                         "strides": None, "version": 2}


def device_view(address, shape, typestr, device):
    """A tensor over `address` on `device`: '<f4' float32, '<i4' int32, '<i8' int64."""
    return torch.as_tensor(_DeviceMemory(address, shape, typestr), device=device)


def keep_factor(p):
    """What a kept element is multiplied by: 1.0f / (1.0f - (float) p), in float32 as the library forms it."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return float(one / (one - torch.tensor(float(p), dtype=torch.float32)))


def _rate(module, attribute, inner="p"):
    """A dropout rate where the four adoptions read it; an absent attribute counts as 0."""
    drop = getattr(module, attribute, None)
    if inner is None:
        return float(drop or 0.0)
    return float(getattr(drop, inner, 0.0) or 0.0) if drop is not None else 0.0


def _layout(net):
    """The module's pieces after the shape checks of the four adoptions: (stem convolution, residual blocks, attention
    block, eps of the blocks, of the attention block, of the heads).  ValueError with the reason otherwise."""
    conv, _act = TS._check(net)
    attn_block = TA._find(net)
    eps_attn = TA._check(attn_block.attn)
    eps_heads = TH._check(net)
    layers = list(net.hidden.children())
    blocks = layers[2:-1]
    if layers[-1] is not attn_block or not blocks or len(blocks) > MAX_BLOCKS or not all(TB._is_block(b) for b in blocks):
        raise ValueError("NativeLearner takes a `hidden` of the stem convolution, a SiLU, 1 to %d 64-channel residual blocks and "
                         "the gated attention block, in that order" % MAX_BLOCKS)
    eps_block = {float(b.norm.eps) for b in blocks}
    if len(eps_block) != 1:
        raise ValueError("NativeLearner takes residual blocks with one GroupNorm eps, got %s" % sorted(eps_block))
    return conv, blocks, attn_block, eps_block.pop(), float(eps_attn), float(eps_heads)


def _roles(net, conv, blocks, attn_block):
    """[(parameter, role)]: every tensor of the network under its AZ_LEARN_ROLE_*."""
    attn = attn_block.attn
    out = [(net.piece_emb.weight, ROLE_PIECE_EMB), (net.pos_emb.weight, ROLE_POS_EMB), (conv.weight, ROLE_STEM_CONV_WEIGHT),
           (conv.bias, ROLE_STEM_CONV_BIAS)]
    for k, b in enumerate(blocks):
        out += [(t, ROLE_BLOCK + 4 * k + f) for f, t in enumerate((b.norm.weight, b.norm.bias, b.conv.weight, b.conv.bias))]
    out += [(t, ROLE_ATTN + f) for f, t in enumerate((attn.prenorm.weight, attn.qkv_proj.weight, attn.gate_proj.weight,
                                                      attn.o_proj.weight, attn.q_norm.weight, attn.k_norm.weight))]
    out += [(TH._resolve(net, path), ROLE_HEADS + i) for i, (_, path, _) in enumerate(TH.PARAMS)]
    return out


class NativeLearner:
    """One az_learn handle over a Connect4 module with the reference's names (az_net.Connect4Net, the reference's `CNN`) and
    its optimiser.

    net.opt must be a `ClipAdamW` on the kernel route; a plain `torch.optim.AdamW` is adopted in place (`optim.adopt`).
    The dropout rates are read once, here, from the attributes the four adoptions read (`dropout.p` of every block,
    `attn.dropout_p`, `policy_head.dropout.p`, `dual_head.pool_drop.p`; absent counts as 0).  `max_rows`: the largest
    batch in rows AFTER augmentation (2 x the batch size of `ReplayBatches`).  `max_workgroups`: the cap of every
    backward (0: each unit's default, what the Python route uses).  `max_norm`: the clipping `train_step` applies.

    Construction allocates ONE flat float32 gradient tensor and makes every `p.grad` a view of it, creates missing
    optimiser state as `ClipAdamW` does, and binds everything in the optimiser's flat order.  Nothing is allocated per
    batch afterwards."""

    def __init__(self, net, max_rows, seed=0, max_workgroups=0, max_norm=5.0):
        self._handle = None
        conv, blocks, attn_block, eps_block, eps_attn, eps_heads = _layout(net)
        max_rows, max_workgroups = int(max_rows), int(max_workgroups)
        if not 1 <= max_rows <= MAX_LEARN_ROWS:
            raise ValueError("NativeLearner takes max_rows in [1, 2^20]")
        if max_workgroups < 0:
            raise ValueError("NativeLearner needs max_workgroups >= 0")
        rates = {_rate(b, "dropout") for b in blocks}
        if len(rates) != 1:
            raise ValueError("NativeLearner takes residual blocks with one dropout rate, got %s" % sorted(rates))
        self.rates = (rates.pop(), _rate(attn_block.attn, "dropout_p", None), _rate(net.policy_head, "dropout"),
                      _rate(net.dual_head, "pool_drop"))
        for p in self.rates:
            if not (0.0 <= p < 1.0 and keep_factor(p) != float("inf")):
                raise ValueError("NativeLearner takes dropout rates in [0, 1), got %r" % (p,))
        named = _roles(net, conv, blocks, attn_block)
        role_of = {id(t): r for t, r in named}
        params = list(net.parameters())
        if len(role_of) != len(named) or {id(p) for p in params} != set(role_of):
            raise ValueError("NativeLearner takes a module whose parameters are exactly the stem's, the blocks', the attention "
                             "block's and the heads', none shared")
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.requires_grad):
                raise ValueError("NativeLearner needs every parameter as a contiguous float32 CUDA tensor that requires a gradient")
        device = params[0].device
        if any(p.device != device for p in params):
            raise ValueError("NativeLearner needs every parameter on one device")
        opt = getattr(net, "opt", None)
        if type(opt) is torch.optim.AdamW:
            opt = O.adopt(opt)
        if not isinstance(opt, O.ClipAdamW):
            raise ValueError("NativeLearner needs net.opt to be a torch.optim.AdamW or a ClipAdamW")
        if opt.route is None:
            opt._set_route(None)
        if opt.route != "kernel":
            raise ValueError("NativeLearner needs net.opt on the kernel route")
        flat = opt._params()
        if len(flat) != len(named) or {id(p) for p in flat} != set(role_of):
            raise ValueError("NativeLearner needs net.opt to hold every parameter of the module exactly once")

        self.net, self.opt, self.device = net, opt, device
        self.max_rows, self.max_workgroups, self.seed, self.max_norm = max_rows, max_workgroups, int(seed), float(max_norm)
        self.n_blocks = len(blocks)
        self.keep_scale = keep_factor(self.rates[1]) if self.rates[1] > 0.0 else 1.0
        self.calls = 0                          # batches so far: the `call` of the next one's dropout draws
        self._flat = flat
        n = len(flat)
        # one flat gradient tensor, every tensor's part 16-byte aligned
        offsets, total = [], 0
        for p in flat:
            offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.grad = torch.zeros(total, dtype=torch.float32, device=device)
        self._views = [self.grad[o:o + p.numel()].view_as(p) for o, p in zip(offsets, flat)]
        for p in flat:                          # missing state, exactly as ClipAdamW._kernel_step creates it
            s = opt.state[p]
            if len(s) == 0:
                s["step"] = torch.tensor(0.0, dtype=O._scalar_dtype())
                s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        opt._dirty = True
        self._roles = (C.c_int32 * n)(*(role_of[id(p)] for p in flat))
        self._groups = (C.c_int32 * n)(*(gi for gi, g in enumerate(opt.param_groups) for _ in g["params"]))
        self._step_no = (C.c_int64 * n)()
        self._hp = (C.c_double * (O.GROUP_HP * O.MAX_GROUPS))()
        self._t = [0] * n
        self._steps = [None] * n
        self._bound = None

        L = lib()
        cfg = LearnConfigC(max_rows, self.n_blocks, max_workgroups, eps_block, eps_attn, eps_heads, self.max_norm,
                           *self.rates, self.seed & (2 ** 64 - 1))
        handle = C.c_void_p()
        with torch.cuda.device(device):
            check(L.az_learn_create(C.byref(cfg), C.byref(handle)))
        self._handle = handle
        out = LearnOutC()
        check(L.az_learn_outputs(handle, C.byref(out)))
        self._out = out
        view = lambda a, shape, kind: device_view(a, shape, kind, device)       # noqa: E731
        self.sums, self.batches, self.entropy = view(out.sums, (3,), "<f4"), view(out.batches, (1,), "<i4"), view(out.entropy, (1,), "<f4")
        self.losses, self.counts, self.grad_norm = view(out.losses, (4,), "<f4"), view(out.counts, (11,), "<i4"), view(out.grad_norm, (1,), "<f4")
        self._sync()

    # ------------------------------------------------------------------------------------ the keeps, for tests and tools

    def keeps(self, n):
        """The dropout inputs of the last batch of n rows as tensors over the handle's memory: (the blocks' factors, a list
        of [n, 64]; the attention block's bits, int64 [n, 4, 42]; the policy head's factors [n, 7, 64]; the pool factors
        [n, 64]).  A tensor whose rate is 0 holds whatever its memory held: the library never writes it."""
        out, dev = self._out, self.device
        blocks = [device_view(out.keep_blocks + 4 * k * out.keep_block_stride, (n, 64), "<f4", dev) for k in range(self.n_blocks)]
        return (blocks, device_view(out.keep_attn, (n, 4, 42), "<i8", dev), device_view(out.keep_policy, (n, 7, 64), "<f4", dev),
                device_view(out.keep_pool, (n, 64), "<f4", dev))

    def draw_keeps(self, n, call):
        """k_learn_keep alone for a batch of n rows numbered `call` (az_learn_dev_keep): what `step` would draw; only
        enqueues.  For tests and tools."""
        self._require_open()
        if not 1 <= n <= self.max_rows:
            raise ValueError("NativeLearner: a batch of %d rows, max_rows is %d" % (n, self.max_rows))
        with torch.cuda.device(self.device):
            check(lib().az_learn_dev_keep(self._handle, n, int(call) & (2 ** 64 - 1), _stream()))

    # ------------------------------------------------------------------------------------ the optimiser's side

    def _sync(self):
        """Before a call: the gradients are the flat tensor's views, the bound addresses are the tensors' current ones, and
        the mirrored step numbers are the optimiser's - whoever stepped last."""
        opt, state = self.opt, self.opt.state
        rebind = False
        for i, p in enumerate(self._flat):
            if p.grad is not self._views[i]:
                p.grad = self._views[i]
            if state[p]["step"] is not self._steps[i]:
                rebind = True
        if not rebind and not opt._dirty and opt.__dict__.get("_t") is not None and len(opt._t) == len(self._t):
            self._t = list(opt._t)              # the Python route stepped since: its mirror is current
        addresses = [(p.data_ptr(), state[p]["exp_avg"].data_ptr(), state[p]["exp_avg_sq"].data_ptr()) for p in self._flat]
        if rebind or addresses != self._bound:
            for p in self._flat:
                s = state[p]
                if s["step"].is_cuda:
                    raise ValueError("NativeLearner: a step counter on the device (a capturable or fused state): reading it waits")
                for k in ("exp_avg", "exp_avg_sq"):
                    m = s[k]
                    if not (m.is_cuda and m.device == self.device and m.dtype == torch.float32 and m.is_contiguous() and m.numel() == p.numel()):
                        raise ValueError("NativeLearner needs every moment as a contiguous float32 tensor on the parameters' device")
            self._steps = [state[p]["step"] for p in self._flat]
            self._t = [int(s) for s in self._steps]
            n = len(self._flat)
            arr = C.c_void_p * n
            with torch.cuda.device(self.device):
                check(lib().az_learn_bind(self._handle, n, self._roles, self._groups, len(opt.param_groups),
                                          arr(*(a[0] for a in addresses)), arr(*(v.data_ptr() for v in self._views)),
                                          arr(*(a[1] for a in addresses)), arr(*(a[2] for a in addresses))))
            self._bound = addresses

    def _hyper(self):
        """lr, betas, eps and weight_decay as param_groups hold them NOW: torch's schedulers keep working."""
        for gi, g in enumerate(self.opt.param_groups):
            self._hp[O.GROUP_HP * gi:O.GROUP_HP * gi + O.GROUP_HP] = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
        for i, t in enumerate(self._t):
            self._step_no[i] = t + 1

    def _stepped(self, k):
        """After k batches: the optimiser's step counters and the mirrors follow, and `ClipAdamW` reads them again."""
        torch._foreach_add_(self._steps, k)
        self._t = [t + k for t in self._t]
        self.calls += k
        self.opt._dirty = True
        self.opt._opt_called = True

    # ------------------------------------------------------------------------------------ batches

    def _batch_c(self, batch):
        if len(batch) != 8:
            raise ValueError("batch must be the 8-tuple ReplayBatches yields")
        n = batch[0].shape[0]
        want = ((torch.float32, (3, 6, 7)), (torch.float32, (7,)), (torch.int8, None), (torch.int16, None), (torch.int16, None),
                (torch.float32, (3,)), (torch.bool, (7,)), (torch.float32, (3,)))
        for t, (dtype, tail) in zip(batch, want):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == dtype and t.is_contiguous() and
                    t.shape[0] == n and (t.numel() == n if tail is None else tuple(t.shape[1:]) == tail)):
                raise ValueError("NativeLearner needs a Connect4 batch as ReplayBatches yields it, on the module's GPU")
        if not 1 <= n <= self.max_rows:
            raise ValueError("NativeLearner: a batch of %d rows, max_rows is %d" % (n, self.max_rows))
        return ReplayBatchC(*(t.data_ptr() for t in batch)), n

    def _config_c(self, config):
        return TL.config_c(config, self.net.aux_target_offset)

    def _result(self):
        c = self.counts
        return TL.TrainingLoss(self.losses[0], self.losses[1], self.losses[2], self.losses[3], c[:9].reshape(3, 3), c[9], c[10])

    def step(self, batch, config=TL.LossConfig()):
        """One training batch: forward, losses, backward, clipping and the AdamW step, enqueued by one call; nothing waits
        for the device.  `batch`: the 8-tuple `ReplayBatches` yields.  Returns a `TrainingLoss` whose tensors are VIEWS of
        the handle's outputs (no autograd; the next call overwrites them); `self.grad_norm` holds the gradient norm."""
        self._require_open()
        batch_c, n = self._batch_c(batch)
        self._sync()
        self._hyper()
        with torch.cuda.device(self.device):
            check(lib().az_learn_dev_step(self._handle, C.byref(batch_c), n, C.byref(self._config_c(config)), self._step_no, self._hp,
                                          self.calls, _stream()))
        self._stepped(1)
        return self._result()

    def epoch(self, batches, config=TL.LossConfig()):
        """One epoch over a kernel-route `ReplayBatches` of a Connect4 buffer by az_learn_dev_epoch: every batch gathered
        into the handle's own tensors and trained on, no Python between batches.  Returns (the number of batches, the rows
        of the last one)."""
        self._require_open()
        if not (isinstance(batches, ReplayBatches) and batches.route == "kernel" and batches.game == "Connect4"):
            raise ValueError("NativeLearner.epoch takes a kernel-route ReplayBatches of a Connect4 buffer")
        if batches.device != self.device:
            raise ValueError("NativeLearner.epoch needs the buffer on the module's GPU")
        n, b = batches.indices.numel(), batches.batch_size
        count = len(batches)
        if count == 0:
            raise ValueError("NativeLearner.epoch: the sample gives no batch")
        if 2 * b > self.max_rows:
            raise ValueError("NativeLearner: a batch of %d rows, max_rows is %d" % (2 * b, self.max_rows))
        order = torch.randperm(n, device=batches.device, generator=batches.gen) if batches.shuffle else batches.order
        ring = replay_tensors_c(batches.buffer, batches.game, batches.device, "batches")
        self._sync()
        self._hyper()
        done = C.c_int64(0)
        with torch.cuda.device(self.device):
            check(lib().az_learn_dev_epoch(self._handle, C.byref(ring), batches.indices.data_ptr(), None if order is None else order.data_ptr(),
                                           n, b, int(batches.drop_last), C.byref(self._config_c(config)), self._step_no, self._hp,
                                           self.calls, C.byref(done), _stream()))
        assert done.value == count
        self._stepped(count)
        return count, 2 * min(b, n - (count - 1) * b)

    def evaluate(self, batch, config=TL.LossConfig()):
        """A no-grad forward of `batch` - the 8-tuple, or the number of rows of the handle's own last epoch batch - and the
        loss pass on it: a `TrainingLoss` of views, as `step` returns."""
        self._require_open()
        if isinstance(batch, int):
            batch_c, n = self._out.batch, batch
        else:
            batch_c, n = self._batch_c(batch)
        self._sync()
        with torch.cuda.device(self.device):
            check(lib().az_learn_dev_eval(self._handle, C.byref(batch_c), n, C.byref(self._config_c(config)), _stream()))
        return self._result()

    def reset_sums(self):
        self._require_open()
        with torch.cuda.device(self.device):
            check(lib().az_learn_reset_sums(self._handle, _stream()))

    def train_step(self, batches, n_epochs=10, **loss_knobs):
        """`train_loss.train_step` for this module: `n_epochs` passes over `batches` - az_learn_dev_epoch per pass when it
        is a kernel-route `ReplayBatches`, `step` per batch for any other iterable of 8-tuples - one scheduler step at the
        end, then the no-grad forward of the last batch.  `loss_knobs`: the fields of `LossConfig`.  Returns the same
        6-tuple (policy, value and aux loss as means over the batches; the last batch's policy entropy; its gradient
        norm; macro F1 of the final forward).  The device is read once, at the end."""
        config = TL.LossConfig(**loss_knobs)
        net = self.net
        native = isinstance(batches, ReplayBatches) and batches.route == "kernel"
        self.reset_sums()
        n_batches, last = 0, None
        for _ in range(n_epochs):
            net.train()
            if native:
                count, last = self.epoch(batches, config)
                n_batches += count
            else:
                for raw in batches:
                    last = tuple(raw)
                    self.step(last, config)
                    n_batches += 1
        net.eval()
        net.scheduler.step()
        if last is None:
            raise ValueError("train_step: the dataloader gave no batch")
        confusion = self.evaluate(last, config).confusion
        host = torch.cat([self.sums / n_batches, self.entropy, self.grad_norm, confusion.reshape(-1).to(torch.float32)]).cpu()
        return (float(host[0]), float(host[1]), float(host[2]), float(host[3]), float(host[4]), TL.macro_f1(host[5:14]))

    def publish(self, fast):
        """What this learner has trained into the live inference twin `fast` (a `FastConnect4Net`) by az_learn_publish: one
        launch into the twin's existing buffers and one wait (src/publish.py).  Returns the three head biases."""
        from src.publish import publish
        return publish(fast, self)

    # ------------------------------------------------------------------------------------ the end

    def _require_open(self):
        if self._handle is None:
            raise ValueError("NativeLearner: closed")

    def close(self):
        """Frees the handle's device memory (after the device has finished with it).  The module, its gradients (the flat
        tensor stays theirs) and the optimiser go on as they are."""
        handle, self._handle = self.__dict__.get("_handle"), None
        if handle is not None:
            try:
                with torch.cuda.device(self.device):
                    torch.cuda.synchronize()
                lib().az_learn_destroy(handle)
            except Exception:               # the interpreter is shutting down
                pass

    def __del__(self):
        self.close()
