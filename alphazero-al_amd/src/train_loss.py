"""The training losses of a batch and their gradients: the piece between `ReplayBatches` and `loss.backward()`.

The reference's training step (src/environments/NetworkBase.py:30-311) derives the value class, turn sign, policy
mask and auxiliary target of a batch, forms up to five loss terms from the network's three head outputs, lets
autograd run their mirror image and reads the value head's predictions back for sklearn's `f1_score`.  Here:

    training_loss   the same terms as ONE autograd node over the three head outputs.  route="kernel" (the default
                    on a GPU) is az_train_dev_loss / az_train_dev_loss_grad (include/az_train.h,
                    csrc/train_kernels.hip): two launches forward, one backward, nothing waits for the device.
                    route="torch" is the same mathematics in plain torch: the only route on the CPU, the baseline
                    on a GPU.
    macro_f1        sklearn's macro F1 as a function of the nine confusion counts.
    train_step      the reference's `train_step` with the net as first argument: `net.train_step(loader, augment,
                    ...)` becomes `train_step(net, loader, augment, ...)`.  Scheduler, optimiser and gradient
                    clipping stay torch's unless `net.opt` is a `ClipAdamW` (src/optim.py: `adopt(net.opt)`), which
                    clips and steps in three launches; the device is read once, at the end.

The terms are stated in include/az_train.h.  Everything here is written from that statement."""
import ctypes as C
from dataclasses import dataclass

import torch

from src.abi import ReplayBatchC, TrainGradsC, TrainHeadsC, TrainLossConfigC, TrainLossOutC, _stream, check, lib
from src.abi import lib as train_lib      # noqa: F401  (train_lib: the name callers written before src/abi.py use)
from src.optim import ClipAdamW

GAME_OF_ACTIONS = {7: 0, 65: 1}             # the width of log_p names the game: Connect4, Othello


@dataclass(frozen=True)
class LossConfig:
    """az_train_loss_config without the offset (that one belongs to the net): the knobs of the reference's
    `train_step` with its defaults.  Checked on construction with the rules of az_train_dev_loss."""
    value_decay: float = 1.0
    distill_alpha: float = 0.0
    distill_temp: float = 1.0
    psw_beta: float = 0.0
    entropy_lambda: float = 0.0
    td_alpha: float = 0.0
    td_steps: int = 5

    def __post_init__(self):
        if not 0.0 < self.value_decay <= 1.0:
            raise ValueError("value_decay must lie in (0, 1]")
        if not 0.0 <= self.distill_alpha <= 1.0:
            raise ValueError("distill_alpha must lie in [0, 1]")
        if not 0.0 <= self.td_alpha <= 1.0:
            raise ValueError("td_alpha must lie in [0, 1]")
        if not self.distill_temp > 0.0:
            raise ValueError("distill_temp must be positive")
        if not (self.psw_beta >= 0.0 and self.entropy_lambda >= 0.0):
            raise ValueError("psw_beta and entropy_lambda must not be negative")
        if int(self.td_steps) != self.td_steps or self.td_steps < 0:
            raise ValueError("td_steps must be a whole number, not negative")


def config_c(config, aux_target_offset):
    return TrainLossConfigC(config.value_decay, config.distill_alpha, config.distill_temp, config.psw_beta,
                            config.entropy_lambda, config.td_alpha, int(config.td_steps), 0, float(aux_target_offset))


@dataclass
class TrainingLoss:
    """What `training_loss` returns.  `policy`, `value`, `aux`: 0-dim tensors with autograd back to the head
    outputs.  `entropy` (0-dim), `confusion` (int32 [3, 3]: row = value class, column = argmax of the value head),
    `policy_rows` and `td_rows` (0-dim int32): no gradient, on the inputs' device."""
    policy: torch.Tensor
    value: torch.Tensor
    aux: torch.Tensor
    entropy: torch.Tensor
    confusion: torch.Tensor
    policy_rows: torch.Tensor
    td_rows: torch.Tensor

    @property
    def total(self):
        return self.policy + self.value + self.aux


# ------------------------------------------------------------------------------------------ the torch route

def _relative(wdl, plus):
    """[draw, p1, p2] -> [draw, win, loss] of the side to move (`plus`: bool [N], the turn sign is +1)."""
    first = torch.where(plus, wdl[:, 1], wdl[:, 2])
    second = torch.where(plus, wdl[:, 2], wdl[:, 1])
    return torch.stack([wdl[:, 0], first, second], 1)


def _xlogx(t):
    return torch.xlogy(t, t)


def derived(batch, aux_target_offset):
    """The value class (int64 [N]), turn sign as a bool `plus` [N], policy mask (float [N]) and normalised
    auxiliary target (float [N]) of a batch."""
    state, prob, winner, _, aux_target = batch[:5]
    plus = state[:, 2, 0, 0] >= 0
    win = winner.reshape(-1).long()
    sign = torch.where(plus, 1, -1)
    cls = torch.where(win == 0, 0, torch.where(win == sign, 1, 2))
    mask = (prob.sum(1) > 0).to(prob.dtype)
    aux = aux_target.reshape(-1).to(prob.dtype) / float(aux_target_offset)
    return cls, plus, mask, aux


def _torch_loss(log_p, value, steps, batch, aux_target_offset, c):
    state, prob, winner, steps_to_end, aux_target, root_wdl, _, future_root_wdl = batch
    dt = log_p.dtype
    prob, root_wdl, future_root_wdl = prob.to(dt), root_wdl.to(dt), future_root_wdl.to(dt)
    cls, plus, mask, aux = derived((state, prob, winner, steps_to_end, aux_target), aux_target_offset)
    to_end = steps_to_end.reshape(-1)

    # policy
    kl = (_xlogx(prob) - prob * log_p).sum(1)
    weighted = kl * (1.0 + c.psw_beta * kl.detach()) if c.psw_beta > 0 else kl
    policy = (weighted * mask).mean()
    p = log_p.exp()
    H = -torch.where(p == 0, torch.zeros_like(p), p * log_p).sum(1)
    if c.entropy_lambda > 0:
        policy = policy - c.entropy_lambda * (H * mask).mean()

    # value
    z = torch.nn.functional.one_hot(cls, 3).to(dt)
    if c.value_decay < 1.0:
        d = (c.value_decay ** to_end.to(dt)).unsqueeze(1)
        z = d * z + (1 - d) * (1.0 / 3.0)
        v_loss = -(z * value).sum(1).mean()
    else:
        v_loss = -value.gather(1, cls.unsqueeze(1)).squeeze(1).mean()
    if c.distill_alpha > 0:
        rel = _relative(root_wdl, plus)
        has_q = (rel.sum(1) > 0).to(dt)
        teacher = torch.softmax(torch.log(rel.clamp(min=1e-8)) / c.distill_temp, 1)
        student = torch.log_softmax(value / c.distill_temp, 1)
        d_kl = (_xlogx(teacher) - teacher * student).sum(1)
        v_loss = (1 - c.distill_alpha) * v_loss + c.distill_alpha * ((d_kl * has_q).mean() * c.distill_temp ** 2)

    # td: the mean over its own rows, as a masked sum so that nothing waits for the count
    td_rows = torch.zeros((), dtype=torch.int32, device=log_p.device)
    if c.td_alpha > 0:
        rel = _relative(future_root_wdl, plus)
        mass = rel.sum(1)
        counted = (to_end > c.td_steps) & (mass > 0)
        t = rel / mass.clamp(min=1e-8).unsqueeze(1)
        if c.value_decay < 1.0:
            keep = c.value_decay ** c.td_steps
            t = keep * t + (1 - keep) / 3.0
        t_kl = (_xlogx(t) - t * value).sum(1)
        rows = counted.sum()
        td = torch.where(counted, t_kl, torch.zeros_like(t_kl)).sum() / rows.clamp(min=1).to(dt)
        v_loss = torch.where(rows > 0, (1 - c.td_alpha) * v_loss + c.td_alpha * td, v_loss)
        td_rows = rows.to(torch.int32)

    aux_loss = torch.nn.functional.smooth_l1_loss(steps, aux)

    with torch.no_grad():
        pred = value.argmax(1)
        confusion = torch.bincount(cls * 3 + pred, minlength=9).reshape(3, 3).to(torch.int32)
        out = TrainingLoss(policy, v_loss, aux_loss, H.mean().detach(), confusion, mask.sum().to(torch.int32), td_rows)
    return out


# ------------------------------------------------------------------------------------------ the kernel route

def _batch_c(batch):
    return ReplayBatchC(*(t.data_ptr() for t in batch))


class _KernelLoss(torch.autograd.Function):
    """(log_p, value, steps) -> (policy, value, aux, entropy, counts) through az_train_dev_loss, and back through
    az_train_dev_loss_grad.  Only enqueues on the current stream."""

    @staticmethod
    def forward(ctx, log_p, value, steps, batch, game, cfg):
        N = log_p.shape[0]
        dev = log_p.device
        L = lib()
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        counts = torch.empty(11, dtype=torch.int32, device=dev)
        work = torch.empty(L.az_train_loss_workspace_bytes(game, N), dtype=torch.uint8, device=dev)
        heads = TrainHeadsC(log_p.data_ptr(), value.data_ptr(), steps.data_ptr())
        out = TrainLossOutC(losses.data_ptr(), counts.data_ptr(), work.data_ptr())
        with torch.cuda.device(dev):
            check(L.az_train_dev_loss(game, C.byref(_batch_c(batch)), C.byref(heads), N, C.byref(cfg), C.byref(out), _stream()))
        ctx.save_for_backward(log_p, value, steps, losses, counts)
        ctx.batch, ctx.game, ctx.cfg = batch, game, cfg
        ctx.set_materialize_grads(False)
        policy, v_loss, aux, entropy = losses.unbind(0)
        ctx.mark_non_differentiable(entropy, counts)
        return policy, v_loss, aux, entropy, counts

    @staticmethod
    def backward(ctx, g_policy, g_value, g_aux, _g_entropy, _g_counts):
        log_p, value, steps, losses, counts = ctx.saved_tensors
        dev = log_p.device
        zero = None
        ups = []
        for g in (g_policy, g_value, g_aux):
            if g is None:
                zero = torch.zeros((), dtype=torch.float32, device=dev) if zero is None else zero
                g = zero
            ups.append(g.reshape(()).to(torch.float32))
        upstream = torch.stack(ups)
        d_log_p, d_value, d_steps = torch.empty_like(log_p), torch.empty_like(value), torch.empty_like(steps)
        heads = TrainHeadsC(log_p.data_ptr(), value.data_ptr(), steps.data_ptr())
        out = TrainLossOutC(losses.data_ptr(), counts.data_ptr(), None)
        grads = TrainGradsC(d_log_p.data_ptr(), d_value.data_ptr(), d_steps.data_ptr())
        with torch.cuda.device(dev):
            check(lib().az_train_dev_loss_grad(ctx.game, C.byref(_batch_c(ctx.batch)), C.byref(heads), log_p.shape[0],
                                               C.byref(ctx.cfg), C.byref(out), upstream.data_ptr(), C.byref(grads), _stream()))
        return d_log_p, d_value, d_steps, None, None, None


def _kernel_checks(log_p, value, steps, batch):
    for name, t in (("log_p", log_p), ("value", value), ("steps", steps)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("route='kernel' needs %s as a contiguous float32 CUDA tensor" % name)
    want = (torch.float32, torch.float32, torch.int8, torch.int16, torch.int16, torch.float32, torch.bool, torch.float32)
    for t, dt in zip(batch, want):
        if not (t.is_cuda and t.device == log_p.device and t.dtype == dt and t.is_contiguous()):
            raise ValueError("route='kernel' needs the batch as ReplayBatches yields it, on the heads' GPU")


def training_loss(log_p, value, steps, batch, aux_target_offset, config=LossConfig(), route=None):
    """The reference's loss terms of one batch: a `TrainingLoss`.

    log_p [N, A], value [N, 3] (log-probabilities; draw, win, loss) and steps [N] or [N, 1] are the net's three
    head outputs; `batch` is the 8-tuple `ReplayBatches` yields.  route: "kernel" (the default on a GPU; float32,
    contiguous CUDA tensors, ValueError otherwise - there is no silent fallback) or "torch"."""
    if len(batch) != 8:
        raise ValueError("batch must be the 8-tuple ReplayBatches yields")
    if not aux_target_offset > 0:
        raise ValueError("aux_target_offset must be positive")
    N = log_p.shape[0]
    if log_p.dim() != 2 or N <= 0 or tuple(value.shape) != (N, 3) or steps.numel() != N or any(t.shape[0] != N for t in batch):
        raise ValueError("log_p [N, A], value [N, 3], steps [N] and a batch of N rows are needed")
    if tuple(batch[1].shape) != tuple(log_p.shape):
        raise ValueError("prob and log_p differ in shape")
    if route is None:
        route = "kernel" if log_p.is_cuda else "torch"
    if route not in ("kernel", "torch"):
        raise ValueError("route must be 'kernel' or 'torch'")
    steps = steps.reshape(-1)
    if route == "torch":
        return _torch_loss(log_p, value, steps, tuple(batch), aux_target_offset, config)
    if log_p.shape[1] not in GAME_OF_ACTIONS:
        raise ValueError("route='kernel' knows Connect4 (7 actions) and Othello (65)")
    _kernel_checks(log_p, value, steps, batch)
    policy, v_loss, aux, entropy, counts = _KernelLoss.apply(log_p, value, steps, tuple(batch), GAME_OF_ACTIONS[log_p.shape[1]],
                                                             config_c(config, aux_target_offset))
    return TrainingLoss(policy, v_loss, aux, entropy, counts[:9].reshape(3, 3), counts[9], counts[10])


def macro_f1(confusion):
    """Macro F1 of a 3 x 3 confusion matrix (row = true class, column = predicted) as
    sklearn.metrics.f1_score(average='macro') gives it: the mean, over the classes that occur among the true or the
    predicted labels, of 2 tp / (2 tp + fp + fn); a class that occurs only on one side counts with 0."""
    c = torch.as_tensor(confusion).detach().to("cpu", torch.float64).reshape(3, 3)
    tp = c.diagonal()
    support = c.sum(1) + c.sum(0)                 # 2 tp + fn + fp
    present = support > 0
    if not bool(present.any()):
        return 0.0
    f1 = torch.where(present, 2 * tp / support.clamp(min=1), torch.zeros_like(tp))
    return float(f1.sum() / present.sum())


def train_step(net, dataloader, augment, ddp_model=None, n_epochs=10, distill_alpha=0.0, value_decay=1.0, distill_temp=1.0,
               psw_beta=0.0, entropy_lambda=0.0, td_alpha=0.0, td_steps=5, route=None):
    """The reference's `Base.train_step` with the losses from `training_loss`: `n_epochs` passes over `dataloader`
    (every batch through `augment`; `augmented` for `ReplayBatches`, which augment already), one optimiser step per
    batch with the gradient norm clipped at 5 (`net.opt.clip_step(5)` when net.opt is a `ClipAdamW`, else
    `clip_grad_norm_` and `net.opt.step()`), one scheduler step at the end.  Uses net.opt, net.scheduler and
    net.aux_target_offset.  Returns (policy loss, value loss, aux loss: means over the batches; policy entropy of the
    last batch; its gradient norm; macro F1 of a no-grad forward of the last batch after the last step).  The
    device is read once, at the end."""
    config = LossConfig(value_decay, distill_alpha, distill_temp, psw_beta, entropy_lambda, td_alpha, td_steps)
    model = ddp_model if ddp_model is not None else net
    dev = next(net.parameters()).device
    sums = torch.zeros(3, device=dev, dtype=next(net.parameters()).dtype)
    n_batches = 0
    last = entropy = None
    grad_norm = torch.zeros((), device=dev, dtype=sums.dtype)
    for _ in range(n_epochs):
        net.train()
        for raw in dataloader:
            last = tuple(augment(raw))
            net.opt.zero_grad(set_to_none=True)
            log_p, value, steps = model(last[0], action_mask=last[6])
            loss = training_loss(log_p, value, steps, last, net.aux_target_offset, config, route)
            loss.total.backward()
            if isinstance(net.opt, ClipAdamW):
                grad_norm = net.opt.clip_step(5)
            else:
                grad_norm = torch.nn.utils.clip_grad_norm_(net.parameters(), 5)
                net.opt.step()
            sums += torch.stack([loss.policy.detach(), loss.value.detach(), loss.aux.detach()])
            entropy = loss.entropy
            n_batches += 1
    net.eval()
    net.scheduler.step()
    if last is None:
        raise ValueError("train_step: the dataloader gave no batch")
    with torch.no_grad():
        log_p, value, steps = net(last[0], action_mask=last[6])
        confusion = training_loss(log_p, value, steps, last, net.aux_target_offset, config, route).confusion
    host = torch.cat([sums / n_batches, entropy.reshape(1), grad_norm.reshape(1).to(sums.dtype),
                      confusion.reshape(-1).to(sums.dtype)]).cpu()
    return (float(host[0]), float(host[1]), float(host[2]), float(host[3]), float(host[4]), macro_f1(host[5:14]))
