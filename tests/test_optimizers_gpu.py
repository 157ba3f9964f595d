"""rmsprop_kernel / adam_kernel (csrc/kernels/misc.hip) against the fp64 transcription of the TF1
formulas in tests/optimizer_ref.py, the loss-scaling skip, and graph replay against eager steps.

Five-step allowance: the GPU may be 4x as far from the fp64 trajectory as the CPU fp32 path of
ops/functional.py is on the same inputs (FMA contraction and evaluation order differ), in the
scaled error max |x - x64| / (|x_0| + sum of |delta64|) over w and both slots. Measured values of
both are recorded in profiles/optimizers.txt: at n = 4195331 the CPU path is 2.8e-07 (rmsprop) and
4.4e-06 (adam) from the fp64 trajectory, the GPU 2.7e-07 and 4.3e-06."""
import numpy as np
import pytest
import torch

import optimizer_ref as R
from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
L2_SLOTS = 4096  # the Trainer's per-block partial buffer (the grid's cap)


@pytest.mark.parametrize("cfg", list(R.CONFIGS))
@pytest.mark.parametrize("n,n_decay", R.SIZES)
def test_single_step_against_fp64(cfg, n, n_decay):
    w, s1, s2, state, l2 = R.run32(Fn, cfg, n, n_decay, DEV, 1, l2_slots=L2_SLOTS)
    R.check_single_step((w, s1, s2), cfg, n, n_decay)
    # per-block w^2 partials: their sum is the decayed range's, the slots past the grid are zero
    w0, _ = R.inputs(n)
    ref_l2 = float((w0[:n_decay].double() ** 2).sum())
    grid = min(((n + 3) // 4 + 255) // 256, 4096)  # sgd_grid(n): 256 threads x float4, capped
    rel = abs(float(l2.double().sum()) - ref_l2) / ref_l2
    print(f"l2 {cfg} n={n}: per-slot relative error {rel:.2e}")
    assert rel <= 1e-5
    assert not l2[grid:].any()
    if state is not None:
        oh = torch.tensor(R.CONFIGS[cfg][1], dtype=torch.float32)
        assert torch.equal(state, oh[:2] * oh[:2])


@pytest.mark.parametrize("cfg", ["rmsprop_eps1", "adam"])
@pytest.mark.parametrize("n,n_decay", R.SIZES)
def test_l2_single_slot_is_one_atomic_sum(cfg, n, n_decay):
    _, _, _, _, l2 = R.run32(Fn, cfg, n, n_decay, DEV, 1, l2_slots=1)
    w0, _ = R.inputs(n)
    ref_l2 = float((w0[:n_decay].double() ** 2).sum())
    # the per-slot mode's figure: one lost block of the 4096 would move the sum by 2.4e-4, while the
    # fp32 additions a value passes through cost about sqrt(13 + grid) * 2^-24 <= 4e-6
    rel = abs(float(l2[0]) - ref_l2) / ref_l2
    print(f"l2 {cfg} n={n}: atomic relative error {rel:.2e}")
    assert rel <= 1e-5


@pytest.mark.parametrize("cfg", list(R.CONFIGS))
@pytest.mark.parametrize("n,n_decay", R.SIZES)
def test_five_steps_against_fp64(cfg, n, n_decay):
    traj, scale = R.trajectory64(cfg, n, n_decay)
    cpu = R.run32(Fn, cfg, n, n_decay, "cpu", R.STEPS)
    gpu = R.run32(Fn, cfg, n, n_decay, DEV, R.STEPS)
    e_cpu = R.scaled_err(cpu[:3], traj[-1], scale)
    e_gpu = R.scaled_err(gpu[:3], traj[-1], scale)
    print(f"five steps {cfg} n={n}: scaled error cpu fp32 {e_cpu:.3e} gpu {e_gpu:.3e}")
    assert e_gpu <= 4.0 * e_cpu
    if gpu[3] is not None:  # the beta powers: the same five fp32 products on either device
        assert torch.equal(gpu[3], cpu[3])


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
@pytest.mark.parametrize("l2_slots", [1, L2_SLOTS])
def test_skip_leaves_everything_bitwise(kind, l2_slots):
    n, n_decay = 1027, 513
    cfg = "adam" if kind == "adam" else "rmsprop_eps1"
    ohl = R.CONFIGS[cfg][1]
    oh = torch.tensor(ohl, dtype=torch.float32, device=DEV)
    _, gs = R.inputs(n)
    g = gs[1].clone()
    g[5] = float("inf")
    g = g.to(DEV)
    w, s1, s2, state, _ = [None if t is None else t.to(DEV) for t in R.run32(Fn, cfg, n, n_decay, DEV, 1)]
    keep = [t.clone() for t in (w, s1, s2)] + ([state.clone()] if state is not None else [])
    h = R.hyper_tensor(found_inf=0.0).to(DEV)
    Fn.nonfinite(g, h[4:5])
    l2 = torch.full((l2_slots,), 7.0, device=DEV)
    if l2_slots == 1:
        l2.zero_()
    if kind == "rmsprop":
        Fn.rmsprop(w, s1, s2, g, n_decay, h, oh, l2)
    else:
        Fn.adam(w, s1, s2, g, n_decay, h, oh, state, l2)
    assert float(h[4]) == 1.0
    now = [w, s1, s2] + ([state] if state is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(keep, now))
    assert not l2.any()


def test_adam_step_after_a_skip_is_t1():
    n, n_decay = 1027, 513
    ohl = R.CONFIGS["adam"][1]
    oh = torch.tensor(ohl, dtype=torch.float32, device=DEV)
    w0, gs = R.inputs(n)
    m, v, state = [t.to(DEV) for t in R.initial_state("adam", n, ohl)]
    w, g = w0.clone().to(DEV), gs[0].to(DEV)
    h = R.hyper_tensor(found_inf=1.0).to(DEV)
    Fn.adam(w, m, v, g, n_decay, h, oh, state, None)
    assert torch.equal(state, oh[:2]) and torch.equal(w.cpu(), w0)
    h[4:5].zero_()
    Fn.adam(w, m, v, g, n_decay, h, oh, state, None)
    R.check_single_step((w.cpu(), m.cpu(), v.cpu()), "adam", n, n_decay)  # the reference's first step: t = 1
    assert torch.equal(state, oh[:2] * oh[:2])


def test_binding_checks():
    ops = _ext.ops()
    n = 1027
    w, a, b, g = (torch.zeros(n, device=DEV) for _ in range(4))
    h = R.hyper_tensor().to(DEV)
    oh = torch.tensor(R.CONFIGS["adam"][1], device=DEV)
    st = oh[:2].clone()
    with pytest.raises(RuntimeError, match="sizes"):
        ops.rmsprop(w, a, b[:-1], g, 0, h, oh, None)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.adam(w[1:], a[1:], b[1:], g[1:], 0, h, oh, st, None)
    with pytest.raises(RuntimeError, match="l2 must hold"):
        ops.adam(torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV),
                 torch.zeros(4096, device=DEV), 0, h, oh, st, torch.zeros(2, device=DEV))
    with pytest.raises(RuntimeError, match="ohyper"):
        ops.rmsprop(w, a, b, g, 0, h, oh[:2], None)
    with pytest.raises(RuntimeError, match="state"):
        ops.adam(w, a, b, g, 0, h, oh, st[:1], None)
    with pytest.raises(RuntimeError, match="float32"):
        ops.rmsprop(w, a, b.double(), g, 0, h, oh, None)


# ------------------------------------------------------------------ graph replay
def _run(kind, use_graph):
    m = create_model("trivial", image_size=32, device=DEV, seed=5, compute_dtype="fp32")
    img, lab = synthetic_batch(m, 8, seed=1)
    lr = lambda step: 0.01 if step < 2 else 0.003  # noqa: E731 -- moves after the capture at step 1
    t = Trainer(m, 8, lr, use_graph=use_graph, graph_warmup=1, optimizer=kind)
    losses = [float(t.step(img, lab)) for _ in range(4)]
    torch.cuda.synchronize()
    assert (t._g_all is not None) == use_graph
    ps = m.ps
    return losses, {k: getattr(ps, k).clone() for k in ("master", "momentum", "slot2", "opt_state")
                    if getattr(ps, k) is not None}


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_graph_replay_equals_eager_steps(kind):
    """4 steps, the last 3 replayed from the graph captured at step 1, against 4 eager steps: a
    learning rate or an Adam t baked into the capture would show at step 2."""
    Fn.set_deterministic(True)
    try:
        le, eager = _run(kind, False)
        lg, graph = _run(kind, True)
    finally:
        Fn.set_deterministic(False)
    assert set(eager) == set(graph) and "slot2" in eager and ("opt_state" in eager) == (kind == "adam")
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert le == lg and all(np.isfinite(le))
    if kind == "adam":
        b1, b2 = np.float32(0.9), np.float32(0.999)
        p1, p2 = b1, b2
        for _ in range(4):
            p1, p2 = np.float32(p1 * b1), np.float32(p2 * b2)
        assert graph["opt_state"].tolist() == [float(p1), float(p2)]
