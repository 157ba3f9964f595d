"""--optimizer=rmsprop|adam on the CPU path: the torch-fp32 implementation of ops/functional.py
against the fp64 transcription of the TF1 formulas (tests/optimizer_ref.py), the loss-scaling
skip, the Trainer / ParamStore plumbing, checkpoints and the command line. The HIP kernels are
held to the same reference in tests/test_optimizers_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optimizer_ref as R
from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch
from azure_hc_intel_tf_amd.utils import checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = R.SIZES[:2]  # the 4M-element sweep case is the GPU grid's business


@pytest.mark.parametrize("cfg", list(R.CONFIGS))
@pytest.mark.parametrize("n,n_decay", SMALL)
def test_cpu_single_step_against_fp64(cfg, n, n_decay):
    w, s1, s2, state, l2 = R.run32(Fn, cfg, n, n_decay, "cpu", 1, l2_slots=1)
    R.check_single_step((w, s1, s2), cfg, n, n_decay)
    w0, _ = R.inputs(n)
    ref_l2 = float((w0[:n_decay].double() ** 2).sum())
    assert abs(float(l2[0]) - ref_l2) <= 1e-5 * ref_l2
    if state is not None:  # [b1^2, b2^2]: one fp32 product each
        oh = torch.tensor(R.CONFIGS[cfg][1], dtype=torch.float32)
        assert torch.equal(state, oh[:2] * oh[:2])


@pytest.mark.parametrize("cfg", list(R.CONFIGS))
def test_cpu_five_steps_stay_near_fp64(cfg):
    """The figure the GPU test's 4x allowance starts from (profiles/optimizers.txt): here only
    that five fp32 steps stay within 5 x the single-step allowance of the fp64 trajectory."""
    n, n_decay = SMALL[1]
    w, s1, s2, _, _ = R.run32(Fn, cfg, n, n_decay, "cpu", R.STEPS)
    traj, scale = R.trajectory64(cfg, n, n_decay)
    err = R.scaled_err((w, s1, s2), traj[-1], scale)
    print(f"five steps {cfg} n={n}: cpu fp32 scaled error {err:.3e}")
    assert err <= R.STEPS * R.SINGLE_STEP_BOUND


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_skip_leaves_everything_bitwise(kind):
    n, n_decay = 1027, 513
    cfg = "adam" if kind == "adam" else "rmsprop_eps1"
    _, oh = R.CONFIGS[cfg]
    oh = torch.tensor(oh, dtype=torch.float32)
    w0, gs = R.inputs(n)
    g = gs[0].clone()
    g[5] = float("inf")
    # a mid-training state: one clean step first
    w, s1, s2, state, _ = R.run32(Fn, cfg, n, n_decay, "cpu", 1)
    keep = [t.clone() for t in (w, s1, s2)] + ([state.clone()] if state is not None else [])
    h = R.hyper_tensor(found_inf=0.0)
    Fn.nonfinite(g, h[4:5])
    assert float(h[4]) == 1.0
    l2 = torch.zeros(1)
    if kind == "rmsprop":
        Fn.rmsprop(w, s1, s2, g, n_decay, h, oh, l2)
    else:
        Fn.adam(w, s1, s2, g, n_decay, h, oh, state, l2)
    now = [w, s1, s2] + ([state] if state is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(keep, now))
    assert float(l2[0]) == 0.0


def test_adam_step_after_a_skip_is_t1():
    n, n_decay = 1027, 513
    _, ohl = R.CONFIGS["adam"]
    oh = torch.tensor(ohl, dtype=torch.float32)
    w0, gs = R.inputs(n)
    w, (m, v, state) = w0.clone(), R.initial_state("adam", n, ohl)
    h = R.hyper_tensor(found_inf=1.0)
    Fn.adam(w, m, v, gs[0], n_decay, h, oh, state, None)  # skipped: t stays 1
    assert torch.equal(state, oh[:2])
    h[4] = 0.0
    Fn.adam(w, m, v, gs[0], n_decay, h, oh, state, None)
    R.check_single_step((w, m, v), "adam", n, n_decay)  # the reference's first step is t = 1
    assert torch.equal(state, oh[:2] * oh[:2])


# ------------------------------------------------------------------ Trainer / ParamStore
def _train(optimizer, steps=2, loss_scale=None, lr=0.05, opt_args=None, seed=5):
    m = create_model("trivial", image_size=32, device="cpu", seed=seed)
    img, lab = synthetic_batch(m, 4, seed=1)
    img = (img - 127) / 60
    t = Trainer(m, 4, constant_lr(lr), loss_scale=loss_scale, optimizer=optimizer, opt_args=opt_args)
    for _ in range(steps):
        t.step(img, lab)
    return m, t, (img, lab)


def test_rmsprop_static_loss_scale_is_transparent():
    m0, _, _ = _train("rmsprop")
    m1, t1, _ = _train("rmsprop", loss_scale=256.0)
    assert torch.allclose(m0.ps.master, m1.ps.master, rtol=1e-4, atol=1e-6)
    assert float(t1.hyper[5]) == 256.0 and abs(float(t1.hyper[3]) - 1 / 256.0) < 1e-12
    assert not torch.equal(m1.ps.slot2, torch.ones_like(m1.ps.slot2))  # it trained


def test_trainer_allocates_the_state_of_its_optimizer():
    m, t, _ = _train("rmsprop", steps=1)
    assert m.ps.slot2 is not None and m.ps.opt_state is None
    assert t.ohyper.tolist() == pytest.approx([0.9, 0.9, 1.0, 0.0])
    m, t, _ = _train("adam", steps=3, opt_args={"beta2": 0.99})
    b1, b2 = np.float32(0.9), np.float32(0.99)
    assert m.ps.opt_state.tolist() == [float(b1 * b1 * b1 * b1), float(b2 * b2 * b2 * b2)]
    assert set(m.ps.state_dict()) >= {"optimizer", "slot2", "opt_state"}
    with pytest.raises(ValueError, match="beta3"):
        _train("adam", steps=0, opt_args={"beta3": 0.5})
    with pytest.raises(ValueError, match="lars"):
        _train("lars", steps=0)


def test_momentum_path_is_unchanged():
    m, t, (img, lab) = _train("momentum", steps=0)
    ps = m.ps
    assert getattr(ps, "slot2", None) is None and getattr(ps, "opt_state", None) is None
    assert set(ps.state_dict()) == {"master", "momentum", "buffers", "names", "offsets"}
    # one step through the Trainer == the same step with Fn.sgd_momentum called directly
    m2 = create_model("trivial", image_size=32, device="cpu", seed=5)
    t2 = Trainer(m2, 4, constant_lr(0.05))
    t2.hyper[0] = 0.05
    t2._forward_backward(img, lab)
    l2 = torch.zeros(1)
    Fn.sgd_momentum(m2.ps.master, m2.ps.momentum, m2.ps.grad, m2.ps.n_decay, t2.hyper, l2, False)
    Fn.loss_total(t2.row_loss, 4, l2, 0.5 * t2.wd, t2.loss)
    loss = t.step(img, lab)
    assert torch.equal(ps.master, m2.ps.master) and torch.equal(ps.momentum, m2.ps.momentum)
    assert torch.equal(loss, t2.loss)


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_checkpoint_resume_continues_bitwise(kind, tmp_path):
    """3 steps, save, restore into a fresh model, 3 more == 6 steps in one go."""
    ma, ta, (img, lab) = _train(kind, steps=6)
    mb, tb, _ = _train(kind, steps=3)
    checkpoint.save(str(tmp_path), 3, mb.ps)
    mc, tc, _ = _train(kind, steps=0, seed=77)  # other initial weights: everything must come from the file
    assert checkpoint.restore_latest(str(tmp_path), mc.ps) == 3
    for name in ("master", "momentum", "slot2", "opt_state"):
        a, b = getattr(mb.ps, name), getattr(mc.ps, name)
        assert (a is None and b is None) or torch.equal(a, b), name
    tc.steps_done = 3
    for _ in range(3):
        tc.step(img, lab)
    for name in ("master", "momentum", "slot2", "opt_state"):
        a, b = getattr(ma.ps, name), getattr(mc.ps, name)
        assert (a is None and b is None) or torch.equal(a, b), name


def test_checkpoint_of_another_optimizer_family_is_refused():
    src, _, _ = _train("momentum", steps=1)
    sd = src.ps.state_dict()
    dst, _, _ = _train("adam", steps=0, seed=77)
    with pytest.raises(ValueError, match=r"optimizer=momentum.*optimizer=adam"):
        dst.ps.load_state_dict(sd)
    # masters and BN buffers were restored before the refusal; the slots are still fresh
    assert torch.equal(dst.ps.master, src.ps.master) and torch.equal(dst.ps.buf, src.ps.buf)
    assert not dst.ps.momentum.any() and not dst.ps.slot2.any()
    back, _, _ = _train("sgd", steps=0, seed=77)
    back.ps.load_state_dict(sd)  # sgd <-> momentum stay interchangeable
    assert torch.equal(back.ps.momentum, src.ps.momentum)
    adam_sd = _train("adam", steps=1)[0].ps.state_dict()
    with pytest.raises(ValueError, match=r"optimizer=adam.*optimizer=sgd"):
        back.ps.load_state_dict(adam_sd)


def test_inference_store_loads_any_optimizers_checkpoint():
    """A store no optimizer owns (--forward_only) takes the weights of an adam checkpoint, ignores
    the slots, and hands them on unchanged if it writes a checkpoint itself."""
    src, _, _ = _train("adam", steps=2)
    sd = src.ps.state_dict()
    for kind in ("momentum", "adam"):  # whatever --optimizer the evaluation run names
        m = create_model("trivial", image_size=32, device="cpu", seed=77)
        Trainer(m, 4, constant_lr(0.0), forward_only=True, optimizer=kind)
        assert m.ps.optimizer is None and m.ps.slot2 is None
        m.ps.load_state_dict(sd)
        assert torch.equal(m.ps.master, src.ps.master) and torch.equal(m.ps.buf, src.ps.buf)
        out = m.ps.state_dict()
        assert out["optimizer"] == "adam"
        assert all(torch.equal(out[k], sd[k]) for k in ("momentum", "slot2", "opt_state"))
    mom_sd = _train("momentum", steps=1)[0].ps.state_dict()
    m.ps.load_state_dict(mom_sd)  # and a momentum checkpoint as before
    assert torch.equal(m.ps.momentum, mom_sd["momentum"]) and set(m.ps.state_dict()) == set(mom_sd)


def test_broadcast_global_variables_carries_the_new_state(monkeypatch):
    from azure_hc_intel_tf_amd.parallel import hvd

    sent = []
    monkeypatch.setattr(hvd, "broadcast_", lambda t, root: sent.append(t))
    m, _, _ = _train("adam", steps=0)
    hvd.broadcast_global_variables(m, 0)
    assert any(t is m.ps.slot2 for t in sent) and any(t is m.ps.opt_state for t in sent)
    sent.clear()
    m, _, _ = _train("momentum", steps=0)
    hvd.broadcast_global_variables(m, 0)
    assert len(sent) == 3


# ------------------------------------------------------------------ command line
def _cli(*args):
    cmd = [sys.executable, os.path.join(ROOT, "tf_cnn_benchmarks.py"), "--device=cpu", "--model=trivial",
           "--batch_size=4", "--image_size=32", "--num_batches=3", "--num_warmup_batches=1", "--display_every=1",
           "--init_learning_rate=0.01", *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def _pow32(b, t):
    p = np.float32(b)
    for _ in range(t - 1):
        p = np.float32(p * np.float32(b))
    return float(p)


def test_cli_rmsprop(tmp_path):
    out = tmp_path / "s.json"
    r = _cli("--optimizer=rmsprop", "--rmsprop_epsilon=0.5", f"--json_summary={out}")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Optimizer:   rmsprop decay=0.9 momentum=0.9 epsilon=0.5" in r.stdout
    import json

    s = json.loads(out.read_text())
    assert s["optimizer"] == "rmsprop" and s["optimizer_args"] == {"decay": 0.9, "momentum": 0.9, "epsilon": 0.5}


def test_cli_adam_checkpoint_round_trip(tmp_path):
    d = str(tmp_path / "ckpt")
    r = _cli("--optimizer=adam", f"--train_dir={d}")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Optimizer:   adam beta1=0.9 beta2=0.999 epsilon=1e-08" in r.stdout
    sd = torch.load(checkpoint.latest(d), map_location="cpu", weights_only=True)
    assert sd["global_step"] == 4 and sd["optimizer"] == "adam"
    assert sd["opt_state"].tolist() == [_pow32(0.9, 5), _pow32(0.999, 5)]  # the 5th step is next
    # restored bitwise into a fresh store
    m = create_model("trivial", image_size=32, device="cpu", seed=99)
    Trainer(m, 4, constant_lr(0.01), optimizer="adam")
    assert checkpoint.restore_latest(d, m.ps) == 4
    assert torch.equal(m.ps.slot2, sd["slot2"]) and torch.equal(m.ps.opt_state, sd["opt_state"])
    assert torch.equal(m.ps.momentum, sd["momentum"]) and bool(sd["slot2"].any())
    # the resumed run goes on from t = 5, not from 1
    r = _cli("--optimizer=adam", f"--train_dir={d}")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Restored checkpoint at step 4" in r.stdout
    sd2 = torch.load(checkpoint.latest(d), map_location="cpu", weights_only=True)
    assert sd2["global_step"] == 8
    assert sd2["opt_state"].tolist() == [_pow32(0.9, 9), _pow32(0.999, 9)]
    # train, then evaluate from the same --train_dir (no --optimizer on the evaluation run)
    r = _cli("--forward_only=True", f"--train_dir={d}")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Restored checkpoint at step 8" in r.stdout and "forward-only" in r.stdout
    sd3 = torch.load(checkpoint.latest(d), map_location="cpu", weights_only=True)
    assert sd3["optimizer"] == "adam" and torch.equal(sd3["slot2"], sd2["slot2"])
    assert torch.equal(sd3["opt_state"], sd2["opt_state"]) and torch.equal(sd3["master"], sd2["master"])


def test_cli_adam_from_a_momentum_checkpoint_names_both(tmp_path):
    d = str(tmp_path / "ckpt")
    src, _, _ = _train("momentum", steps=1, seed=1234)
    checkpoint.save(d, 1, src.ps)
    r = _cli("--optimizer=adam", f"--train_dir={d}")
    assert r.returncode != 0
    assert "--optimizer=momentum" in r.stderr and "--optimizer=adam" in r.stderr
