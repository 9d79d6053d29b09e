"""The reference for the clipping and the AdamW step (az_opt_dev_step in include/az_train.h, `ClipAdamW` in src/optim.py):
`torch.nn.utils.clip_grad_norm_(foreach=False)` followed by `torch.optim.AdamW(foreach=False).step()` on the CPU, in
float64 (the reference proper) or float32 (the deviation torch itself has from it, which the GPU tests' bounds rest on).

Also the inputs the CPU and the GPU tests share: `SIZES` (every granule of the kernels, one below, at, one above), three
parameter groups, seeded parameters and three steps of gradients per clip case.  Everything is computed once and cached."""
import functools

import numpy as np

# the kernels' granules (csrc/optim_kernels.hip): a 16-byte access, a wavefront's vector stride, the workgroup's, a chunk
VEC, WAVE_STRIDE, BLOCK_STRIDE, CHUNK, SLICE = 4, 256, 1024, 2048, 96
# (numel, which of g / p / m / v start 4 bytes into their storage); the tensor of 300 elements never has a gradient
SIZES = [(1, ""), (3, ""), (4, ""), (5, ""),
         (WAVE_STRIDE - 1, ""), (WAVE_STRIDE, ""), (WAVE_STRIDE + 1, ""),
         (300, ""),
         (BLOCK_STRIDE - 1, ""), (BLOCK_STRIDE, ""), (BLOCK_STRIDE + 1, ""),
         (CHUNK - 1, ""), (CHUNK, ""), (CHUNK + 1, ""),
         (3 * CHUNK + 5, ""),                       # four chunks, the last of five elements
         (BLOCK_STRIDE + 6, "gpmv"), (CHUNK + 5, "g"), (517, "p"), (CHUNK + 7, "gpmv")]
SKIPPED = 7
GROUPS = [dict(lr=1e-3, weight_decay=1e-2), dict(lr=1e-3, weight_decay=0.0), dict(lr=5e-4, weight_decay=1e-2)]
BETAS, EPS = (0.9, 0.999), 1e-8
MAX_NORM = 5.0
STEPS = 3
# gradient scale per clip case: 21 k elements of standard deviation s have norm about 145 s
CLIP_CASES = {"below": (0.01, MAX_NORM), "above": (0.1, MAX_NORM), "zero": (0.0, MAX_NORM), "noclip": (0.1, 0.0)}
QUANTITIES = ("p", "exp_avg", "exp_avg_sq")
FLOOR, FACTOR = 1e-6, 4.0


def group_of(i, n_groups=len(GROUPS)):
    return i % n_groups


@functools.lru_cache(maxsize=None)
def inputs(case, sizes=None, seed=20):
    """(parameters, [gradients of step 1, 2, 3]) as float32 arrays; a gradient is None for the skipped tensor."""
    numels = [n for n, _ in SIZES] if sizes is None else list(sizes)
    scale, _ = CLIP_CASES[case]
    rng = np.random.default_rng(seed)
    params = [(rng.standard_normal(n) * 0.5).astype(np.float32) for n in numels]
    grads = []
    for _ in range(STEPS):
        grads.append([None if (sizes is None and i == SKIPPED) else (rng.standard_normal(n) * scale).astype(np.float32)
                      for i, n in enumerate(numels)])
    return params, grads


def run(params, grads, max_norm, dtype, groups=GROUPS):
    """`len(grads)` steps of clip_grad_norm_ (max_norm > 0) and AdamW, foreach=False, on the CPU in `dtype`.
    -> per step a dict: p, exp_avg, exp_avg_sq (lists of float64 arrays; a tensor without state has zeros) and norm."""
    import torch
    dt = getattr(torch, dtype)
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dt)) for p in params]
    spec = [dict(g, params=[p for i, p in enumerate(ps) if group_of(i, len(groups)) == k]) for k, g in enumerate(groups)]
    opt = torch.optim.AdamW(spec, betas=BETAS, eps=EPS, foreach=False)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.from_numpy(g.copy()).to(dt)
        norm = None
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False).double())
        opt.step()
        state = [opt.state.get(p, {}) for p in ps]
        out.append(dict(p=[p.detach().double().numpy().copy() for p in ps],
                        exp_avg=[s["exp_avg"].double().numpy().copy() if s else np.zeros(p.numel()) for s, p in zip(state, ps)],
                        exp_avg_sq=[s["exp_avg_sq"].double().numpy().copy() if s else np.zeros(p.numel()) for s, p in zip(state, ps)],
                        norm=norm))
    return out


@functools.lru_cache(maxsize=None)
def reference(case, dtype="float64"):
    params, grads = inputs(case)
    return run(params, grads, CLIP_CASES[case][1], dtype)


def dev(got, want):
    """Largest absolute difference over the largest magnitude of `want`, over a list of arrays (0 / 0 counts as 0)."""
    gap = max(float(np.abs(np.asarray(g, np.float64) - w).max()) for g, w in zip(got, want))
    top = max(float(np.abs(w).max()) for w in want)
    return 0.0 if gap == 0 else (gap / top if top > 0 else float("inf"))


def deviations(got, ref, before_got, before_ref):
    """One step's deviations of `got` from `ref` per quantity; `step`: of the step the parameters took, relative to the
    largest step (before_*: the parameters the step started from)."""
    d = {q: dev(got[q], ref[q]) for q in QUANTITIES}
    d["step"] = dev([a - np.asarray(b, np.float64) for a, b in zip(got["p"], before_got)],
                    [a - np.asarray(b, np.float64) for a, b in zip(ref["p"], before_ref)])
    if ref["norm"] is not None:
        d["norm"] = dev([np.array([got["norm"]])], [np.array([ref["norm"]])])
    return d


@functools.lru_cache(maxsize=None)
def torch_deviations(case):
    """Per step, the deviations of float32 torch from float64 torch on the same inputs."""
    params, _ = inputs(case)
    exact, single = reference(case), reference(case, "float32")
    out = []
    for k in range(STEPS):
        out.append(deviations(single[k], exact[k], single[k - 1]["p"] if k else params, exact[k - 1]["p"] if k else params))
    return out


def bound(own):
    return max(FACTOR * own, FLOOR)
