"""fp64 reference of the RMSProp / Adam steps (TF1 semantics, --optimizer=rmsprop|adam) and the
inputs the optimizer tests share. A transcription of the formulas, independent of
ops/functional.py:

    gg  = g * grad_scale (+ wd * w for j < n_decay)
    RMSProp: ms = decay*ms + (1-decay)*gg^2; mom = momentum*mom + lr*gg/sqrt(ms+eps); w -= mom
    Adam:    m = b1*m + (1-b1)*gg; v = b2*v + (1-b2)*gg^2;
             w -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps), t from 1

The step's inputs are the fp32 numbers the kernel is handed -- w, g, the slots AND the
hyper-parameters as stored in the device tensors (0.999 or 1/3 rounded to fp32) -- widened to
fp64 exactly; every operation after that is fp64.
"""
import functools

import numpy as np
import torch

LR, WD, GRAD_SCALE = 0.01, 4e-5, 1.0 / 3.0
# (n, n_decay): tail only; the decay boundary inside a float4 and a non-empty tail; more than
# one grid-stride sweep at the 4096-block cap (4096 * 256 float4 per sweep)
SIZES = [(3, 2), (1027, 513), (4096 * 256 * 4 + 1027, 2_000_003)]
# name -> (kind, ohyper)
CONFIGS = {
    "rmsprop_eps1": ("rmsprop", [0.9, 0.9, 1.0, 0.0]),
    "rmsprop_eps1e-10": ("rmsprop", [0.9, 0.9, 1e-10, 0.0]),
    "adam": ("adam", [0.9, 0.999, 1e-8, 0.0]),
}
STEPS = 5


def hyper_tensor(found_inf=None, lr=LR):
    h = [lr, 0.0, WD, GRAD_SCALE]
    if found_inf is not None:
        h += [float(found_inf), 1.0, 0.0, 1000.0]
    return torch.tensor(h, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def inputs(n: int):
    """w ~ N(0,1) and STEPS gradients ~ 1e-2 N(0,1) with about 1% exact zeros (fp32, CPU)."""
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    w = torch.randn(n, generator=gen)
    gs = []
    for _ in range(STEPS):
        g = 1e-2 * torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.01] = 0.0
        gs.append(g)
    if n <= 4:
        gs[0][0] = 0.0  # the tiny case keeps one exact zero too
    return w, gs


def initial_state(kind: str, n: int, ohyper):
    """(slot, slot2, opt_state) as ParamStore.init_optimizer sets them."""
    slot = torch.zeros(n)
    if kind == "rmsprop":
        return slot, torch.ones(n), None
    oh = torch.tensor(ohyper, dtype=torch.float32)
    return slot, torch.zeros(n), oh[:2].clone()


def step64(kind, w, s1, s2, g, n_decay, hyper, ohyper, state):
    """One fp64 step on numpy float64 arrays (hyper / ohyper / state: the fp32 tensors' values).
    Returns (w, s1, s2, state, l2) -- new arrays; l2 = sum w^2 over the decayed range."""
    h = np.asarray(hyper, dtype=np.float64)
    oh = np.asarray(ohyper, dtype=np.float64)
    lr, wd, gsc = h[0], h[2], h[3]
    l2 = float(np.sum(w[:n_decay] ** 2))
    if h.size > 4 and h[4] != 0.0:
        return w, s1, s2, state, 0.0
    gg = g * gsc
    gg[:n_decay] += wd * w[:n_decay]
    if kind == "rmsprop":
        decay, mu, eps = oh[0], oh[1], oh[2]
        ms = decay * s2 + (1.0 - decay) * gg * gg
        mom = mu * s1 + lr * gg / np.sqrt(ms + eps)
        return w - mom, mom, ms, state, l2
    b1, b2, eps = oh[0], oh[1], oh[2]
    st = np.asarray(state, dtype=np.float64)
    m = b1 * s1 + (1.0 - b1) * gg
    v = b2 * s2 + (1.0 - b2) * gg * gg
    lr_t = lr * np.sqrt(1.0 - st[1]) / (1.0 - st[0])
    return w - lr_t * m / (np.sqrt(v) + eps), m, v, st * oh[:2], l2


@functools.lru_cache(maxsize=None)
def trajectory64(cfg: str, n: int, n_decay: int):
    """The fp64 trajectory of STEPS steps from the initial state: a list of (w, s1, s2) after each
    step, and per tensor the error scale |x_0| + sum over steps of |delta64| (float64 arrays)."""
    kind, ohyper = CONFIGS[cfg]
    w0, gs = inputs(n)
    s1, s2, state = initial_state(kind, n, ohyper)
    oh32 = torch.tensor(ohyper, dtype=torch.float32).numpy()
    cur = [w0.double().numpy(), s1.double().numpy(), s2.double().numpy()]
    st = None if state is None else state.double().numpy()
    scale = [np.abs(c) for c in cur]
    out = []
    for g in gs:
        nw, n1, n2, st, _ = step64(kind, cur[0], cur[1], cur[2], g.double().numpy(), n_decay,
                                   hyper_tensor().numpy(), oh32, st)
        new = [nw, n1, n2]
        scale = [s + np.abs(a - b) for s, a, b in zip(scale, new, cur)]
        cur = new
        out.append(tuple(cur))
    return out, scale


def run32(fn_module, cfg, n, n_decay, device, steps, l2_slots=0):
    """`steps` steps through ops.functional on `device` from the initial state; returns the fp32
    tensors (w, s1, s2, state, l2-of-the-last-step) on the CPU."""
    kind, ohyper = CONFIGS[cfg]
    w0, gs = inputs(n)
    s1, s2, state = initial_state(kind, n, ohyper)
    w, s1, s2 = w0.clone().to(device), s1.to(device), s2.to(device)
    state = None if state is None else state.to(device)
    hyper = hyper_tensor().to(device)
    oh = torch.tensor(ohyper, dtype=torch.float32, device=device)
    l2 = torch.zeros(l2_slots, device=device) if l2_slots else None
    for g in gs[:steps]:
        if l2 is not None and l2_slots == 1:
            l2.zero_()
        if kind == "rmsprop":
            fn_module.rmsprop(w, s1, s2, g.to(device), n_decay, hyper, oh, l2)
        else:
            fn_module.adam(w, s1, s2, g.to(device), n_decay, hyper, oh, state, l2)
    return (w.cpu(), s1.cpu(), s2.cpu(), None if state is None else state.cpu(),
            None if l2 is None else l2.cpu())


def scaled_err(xs, refs, scales):
    """max over the tensors and their elements of |x - x64| / scale (0/0 counts as 0)."""
    worst = 0.0
    for x, r, s in zip(xs, refs, scales):
        d = np.abs(x.double().numpy() - r)
        q = np.divide(d, s, out=np.zeros_like(d), where=s > 0)
        assert not np.any((s == 0) & (d > 0)), "a value moved where the fp64 trajectory never does"
        worst = max(worst, float(q.max()))
    return worst


SINGLE_STEP_BOUND = 16 * 2.0 ** -24  # ~ten fp32 roundings of 2^-24 relative each per element


def check_single_step(xs, cfg, n, n_decay):
    """|x - x64| <= 16 * 2^-24 * (|x_old| + |delta64|) per element, for w and both slots."""
    traj, _ = trajectory64(cfg, n, n_decay)
    kind, ohyper = CONFIGS[cfg]
    w0, _ = inputs(n)
    s1, s2, _ = initial_state(kind, n, ohyper)
    for name, x, old, new in zip(("w", "slot", "slot2"), xs, (w0, s1, s2), traj[0]):
        old = old.double().numpy()
        d = np.abs(x.double().numpy() - new)
        bound = SINGLE_STEP_BOUND * (np.abs(old) + np.abs(new - old))
        ratio = float(np.max(np.divide(d, bound, out=np.where(d > 0, np.inf, 0.0), where=bound > 0)))
        print(f"single step {cfg} n={n} {name}: worst |err| / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"{cfg} n={n} {name}: error {ratio:.2f}x the single-step bound"
