"""Gradient-norm clipping and the AdamW step of a training batch: the piece after `loss.backward()`.

The reference's `_optimize_batch` ends with `clip_grad_norm_(self.parameters(), 5)` and `self.opt.step()`, `opt` a
`torch.optim.AdamW` over five or six parameter groups: a few dozen small launches per batch and torch's Python
bookkeeping around them.  Here:

    ClipAdamW   a `torch.optim.AdamW` - same constructor, same `param_groups`, same per-parameter state (`step`,
                `exp_avg`, `exp_avg_sq`, created as torch creates them), `state_dict()` interchangeable with torch's in
                both directions - whose `clip_step(max_norm)` clips and steps.  route="kernel" (the default for CUDA
                parameters) is az_opt_dev_step (include/az_train.h, csrc/optim_kernels.hip): three launches, nothing
                waits for the device.  route="torch" is literally `clip_grad_norm_` followed by `AdamW.step`: the only
                route on the CPU, the baseline on a GPU.
    reference_param_groups   the parameter groups the reference's nets build their AdamW over.
    adopt       turns the `torch.optim.AdamW` a net built in its `__init__` into a `ClipAdamW` in place, so that the
                schedulers built on it keep driving it: `adopt(net.opt)`.

On the kernel route `.grad` is read and never written: after a step it still holds the UNCLIPPED gradient, where
`clip_grad_norm_` leaves the clipped one.  `train_step` and the reference read no gradient after the step.

Needs torch and src.abi only: a learner does not import the engine."""
import ctypes as C
import weakref

import torch

from src.abi import _stream, check, lib

MAX_GROUPS, GROUP_HP = 16, 5                # AZ_OPT_MAX_GROUPS, AZ_OPT_GROUP_HP


def _plain(fn):
    """`fn` below the wrapper `Optimizer` puts round a class's `step` for its hooks (they have run already)."""
    return fn.__wrapped__ if getattr(fn, "hooked", False) else fn


def _scalar_dtype():
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32


class ClipAdamW(torch.optim.AdamW):
    """`torch.optim.AdamW` with `clip_step`.  Refused, with the reason, at construction: `amsgrad` (a third moment the
    kernel does not keep), `maximize`, `capturable` and `fused` (their step counters live on the device: reading them
    waits), `differentiable`, a tensor as `lr` or beta, parameters that are not float32.

    route: None ("kernel" when every parameter is a CUDA tensor of one device, else "torch"), "kernel" or "torch".
    Hooks registered with `register_step_pre_hook` / `register_step_post_hook` run for `clip_step` as for `step`."""
    _route = None
    _handle = None
    _dirty = True           # the flat view of param_groups, or a bound address, is out of date

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, route=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        self._set_route(route)

    # ------------------------------------------------------------------------------------ what is supported

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _set_route(self, route):
        if route not in (None, "kernel", "torch"):
            raise ValueError("route must be 'kernel' or 'torch'")
        for g in self.param_groups:
            for flag, why in (("amsgrad", "the kernel keeps two moments, amsgrad needs a third"),
                              ("maximize", "the kernel descends"),
                              ("capturable", "capturable keeps the step counters on the device, and reading them waits"),
                              ("fused", "fused keeps the step counters on the device, and reading them waits"),
                              ("differentiable", "the step is not recorded for autograd")):
                if g.get(flag):
                    raise ValueError("ClipAdamW does not take %s: %s" % (flag, why))
            if any(isinstance(x, torch.Tensor) for x in (g["lr"],) + tuple(g["betas"])):
                raise ValueError("ClipAdamW does not take a tensor as lr or beta: reading it each step may wait for a device")
        params = self._params()
        for p in params:
            if p.dtype != torch.float32:
                raise ValueError("ClipAdamW needs float32 parameters: the kernel reads and writes float32 (got %s)" % p.dtype)
        on_gpu = all(p.is_cuda for p in params) and len({p.device for p in params}) == 1
        if route is None:
            route = "kernel" if on_gpu else "torch"
        if route == "kernel":
            if not on_gpu:
                raise ValueError("route='kernel' needs every parameter on one CUDA device")
            if len(self.param_groups) > MAX_GROUPS:
                raise ValueError("route='kernel' takes at most %d parameter groups" % MAX_GROUPS)
        self._route = route
        self._dirty = True

    @property
    def route(self):
        return self._route

    # ------------------------------------------------------------------------------------ torch's interface

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._dirty = True
        if self._route is not None:
            self._set_route(self._route)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dirty = True
        self._set_route(self._route)

    def __getstate__(self):
        state = super().__getstate__()
        state["_route"] = self._route
        return state

    def __del__(self):
        self._release()

    def _release(self):
        handle, self._handle = self.__dict__.get("_handle"), None
        if handle is not None:
            try:
                lib().az_opt_destroy(handle)
            except Exception:               # the interpreter is shutting down
                pass

    @torch.no_grad()
    def step(self, closure=None, *, max_norm=0.0):
        """`torch.optim.AdamW.step`; with max_norm > 0 the gradient norm is clipped first (see `clip_step`)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._opt_called = True
        if self._route is None:
            self._set_route(None)
        if self._route == "kernel":
            self._norm = self._kernel_step(float(max_norm))
        else:
            self._norm = torch.nn.utils.clip_grad_norm_(self._params(), max_norm) if max_norm > 0 else None
            _plain(torch.optim.AdamW.step)(self)
        return loss

    def clip_step(self, max_norm):
        """`clip_grad_norm_(parameters, max_norm)` and one AdamW step.  Returns the total norm of the gradients as a 0-d
        tensor on the parameters' device, never read by the host here (None when max_norm <= 0: nothing is clipped)."""
        self.step(max_norm=max_norm)
        norm, self._norm = self._norm, None
        return norm

    # ------------------------------------------------------------------------------------ the kernel route

    def _rebuild(self):
        """The flat view of param_groups and, when the tensors' sizes or groups changed, a new handle."""
        params = self._params()
        if not params:
            raise ValueError("ClipAdamW: no parameters")
        for p in params:
            if not p.is_contiguous():
                raise ValueError("route='kernel' needs contiguous parameters")
        n = len(params)
        numel = [p.numel() for p in params]
        group = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        shape = (tuple(numel), tuple(group), len(self.param_groups))
        if self._handle is None or self.__dict__.get("_shape") != shape:
            self._release()
            handle = C.c_void_p()
            check(lib().az_opt_create(n, (C.c_int64 * n)(*numel), (C.c_int32 * n)(*group), len(self.param_groups), C.byref(handle)))
            self._handle, self._shape = handle, shape
            self._grad, self._step_no, self._hp = (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_double * (GROUP_HP * MAX_GROUPS))()
        self._flat = params
        self._ready = [len(self.state.get(p, ())) != 0 for p in params]
        self._steps = [self.state[p]["step"] if r else None for p, r in zip(params, self._ready)]
        for s in self._steps:
            if s is not None and s.is_cuda:
                raise ValueError("ClipAdamW: a step counter on the device (a capturable or fused state): reading it waits")
        self._t = [int(s) if s is not None else 0 for s in self._steps]
        self._device = params[0].device
        self._bind()

    def _bind(self):
        """Hands the addresses of the parameters and their moments to the handle; a tensor without state yet (it never had
        a gradient) lends its own address: it is skipped until it has one."""
        n = len(self._flat)
        p_ptr = [p.data_ptr() for p in self._flat]
        m_ptr = [self.state[p]["exp_avg"].data_ptr() if r else a for p, r, a in zip(self._flat, self._ready, p_ptr)]
        v_ptr = [self.state[p]["exp_avg_sq"].data_ptr() if r else a for p, r, a in zip(self._flat, self._ready, p_ptr)]
        arr = C.c_void_p * n
        with torch.cuda.device(self._device):
            check(lib().az_opt_bind(self._handle, arr(*p_ptr), arr(*m_ptr), arr(*v_ptr)))
        self._p_ptr = p_ptr
        self._dirty = False

    def _kernel_step(self, max_norm):
        if self._dirty or self._handle is None:
            self._rebuild()
        grad, step_no, t, ready, p_ptr, state = self._grad, self._step_no, self._t, self._ready, self._p_ptr, self.state
        rebind, bump = False, []
        try:
            for i, p in enumerate(self._flat):
                g = p.grad
                if g is None:
                    grad[i], step_no[i] = None, 0
                    continue
                if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.numel() != p.numel():
                    raise ValueError("route='kernel' needs every gradient dense, contiguous, float32 and on its parameter's device")
                if not ready[i]:
                    s = state[p]
                    s["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self._steps[i], ready[i], rebind = s["step"], True, True
                if p.data_ptr() != p_ptr[i]:
                    rebind = True
                t[i] += 1
                grad[i], step_no[i] = g.data_ptr(), t[i]
                bump.append(self._steps[i])
            if rebind:
                self._bind()
            for gi, g in enumerate(self.param_groups):
                self._hp[GROUP_HP * gi:GROUP_HP * gi + GROUP_HP] = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
            norm = torch.empty((), dtype=torch.float32, device=self._device) if max_norm > 0 else None
            with torch.cuda.device(self._device):
                check(lib().az_opt_dev_step(self._handle, grad, step_no, self._hp, max_norm,
                                            None if norm is None else norm.data_ptr(), _stream()))
        except BaseException:
            self._dirty = True              # the mirrored step numbers are read again from the state
            raise
        if bump:
            torch._foreach_add_(bump, 1)
        return norm


def reference_param_groups(net, lr, policy_lr_scale=0.3):
    """The parameter groups the reference's nets hand their AdamW (Connect4/Network.py:187-193, Othello/Network.py:152-163)
    for a module with the reference's names (az_net.Connect4Net, az_net.OthelloNet): the body (`hidden` or `stem`) and the
    value head at `lr` with the optimiser's weight decay, the embeddings without weight decay, the policy head at
    `lr * policy_lr_scale`.  Five groups for Connect4, six for Othello (its `legal_emb`).  Pass `lr=lr, weight_decay=1e-2`
    to the optimiser as the reference does."""
    body = net.hidden if hasattr(net, "hidden") else net.stem
    groups = [{"params": list(body.parameters())}, {"params": list(net.dual_head.parameters())}]
    for name in ("piece_emb", "pos_emb", "legal_emb"):
        if hasattr(net, name):
            groups.append({"params": list(getattr(net, name).parameters()), "weight_decay": 0})
    groups.append({"params": list(net.policy_head.parameters()), "lr": lr * policy_lr_scale})
    return groups


def adopt(opt, route=None):
    """Turns a `torch.optim.AdamW` into a `ClipAdamW` IN PLACE and returns it: the same object, so `LinearLR` /
    `SequentialLR` objects built on it keep driving it, its `param_groups` and state untouched, and no "scheduler before
    optimizer" warning appears.  The reference's nets build `opt` and `scheduler` together in `__init__`; the supported
    swap is `adopt(net.opt)` after construction.  Refuses what `ClipAdamW` refuses.

    Opt-in.  Measured on an MI355X (tools/measure_optim.py): clipping and the step alone take about
    130 us of host time against 660 to 870 us for torch's default AdamW and 320 to 410 us for AdamW(fused=True).  A whole
    `train_step` batch of 1024 rows gains 1.2 % on the Othello module (against the default and against fused=True) and
    NOTHING on the Connect4 module, where neither this class nor fused=True beats the default beyond the spread."""
    if isinstance(opt, ClipAdamW):
        if route is not None:
            opt._set_route(route)
        return opt
    if type(opt) is not torch.optim.AdamW:
        raise TypeError("adopt takes a torch.optim.AdamW, got %s" % type(opt).__name__)
    wrapped = opt.__dict__.get("step")
    opt.__class__ = ClipAdamW
    try:
        opt._set_route(route)
    except Exception:
        opt.__class__ = torch.optim.AdamW
        raise
    opt._patch_step_function()                  # the hook wrapper round ClipAdamW.step, as Optimizer.__init__ leaves it
    if wrapped is not None and getattr(wrapped, "_wrapped_by_lr_sched", False):
        # a scheduler wrapped the instance's `step` to see it called: the same wrapper round the new class's step
        ref = weakref.ref(opt)

        def step(*args, **kwargs):
            o = ref()
            o._opt_called = True
            return type(o).step(o, *args, **kwargs)
        step._wrapped_by_lr_sched = True
        opt.step = step
    return opt
