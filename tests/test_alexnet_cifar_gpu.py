"""The CIFAR-10 AlexNet (``--model=alexnet --data_name=cifar10``: two 5x5 convs with local response
normalisation, csrc/kernels/lrn.hip) on the MI355X: one captured-graph training step at fp32 and bf16
against the fp32 CPU step of the same weights, with the methods and bounds of tests/test_fp32_zoo_gpu.py
(fp32: loss to 1e-4 relative, gradient cosine > 0.9999, and the gradient to 1e-5 given the step's own ReLU /
max-pool decisions, tools/zoo_flip_probe.py) and tests/test_zoo_gpu.py (bf16: loss to 0.05, classifier-gradient
cosine > 0.97, descent); ``--forward_only`` logits at the bounds of tests/test_forward_only_gpu.py; the CLI."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.models.sequential import AlexNetCifar
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8


def _reset():
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def _pair(dtype, seed=9):
    kw = dict(data_name="cifar10", seed=seed, image_channels=8)  # the GPU layout: image channels padded to 8
    mg = create_model("alexnet", device="cuda", compute_dtype=dtype, **kw)
    mc = create_model("alexnet", device="cpu", **kw)
    assert isinstance(mg, AlexNetCifar) and mg.native and mg.image_size == 32 and mg.num_classes == 11
    assert torch.equal(mg.ps.master.cpu(), mc.ps.master)
    img, lab = synthetic_batch(mc, B, seed=4)
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
    if dtype != "fp32":
        img = img.to(torch.bfloat16).float()
    return mg, mc, img, lab


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_step_matches_the_fp32_cpu_step(dtype, monkeypatch):
    try:
        mg, mc, img, lab = _pair(dtype)
        ns = _ext.ops()
        calls = []
        for fn in ("lrn_fwd", "lrn_bwd"):
            real = getattr(ns, fn)
            monkeypatch.setattr(ns, fn, lambda *a, _n=fn, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
        for fn in ("conv2d", "local_response_norm", "max_pool2d"):
            real = getattr(F, fn)
            monkeypatch.setattr(F, fn, lambda *a, _n="F." + fn, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
        # lr 0, no weight decay: the warm-up steps before the capture leave the weights as they are
        tg = Trainer(mg, B, constant_lr(0.0), weight_decay=0.0, use_graph=True)
        assert tg.use_graph
        img_g, lab_g = img.to("cuda", mg.act_dtype), lab.cuda()
        per_step = []
        for _ in range(tg.graph_warmup + 2):  # eager warm-up, the capture (+ replay), one more replay
            n0 = len(calls)
            lg = float(tg.step(img_g, lab_g))
            per_step.append(calls[n0:])
        torch.cuda.synchronize()
        assert tg._g_all is not None, "the step was not captured"
        for c in per_step[:tg.graph_warmup + 1]:  # every pass through the Python step, the captured one included
            assert sorted(c) == ["lrn_bwd", "lrn_bwd", "lrn_fwd", "lrn_fwd"], c
        assert per_step[-1] == [], "a replay runs no Python"
        monkeypatch.undo()
        tc = Trainer(mc, B, constant_lr(0.0), weight_decay=0.0)
        lc = float(tc.step(img, lab))
        gg, gc = mg.ps.grad.float().cpu(), mc.ps.grad
        assert bool(torch.isfinite(gg).all())
        cos = float(gg @ gc / (gg.norm() * gc.norm()))
        print(f"{dtype}: loss gpu {lg:.6f} cpu {lc:.6f}, gradient cosine {cos:.6f}, "
              f"rel {float((gg - gc).norm() / gc.norm()):.3e}")
        if dtype == "fp32":
            assert abs(lg - lc) <= 1e-4 * abs(lc), (lg, lc)
            assert cos > 0.9999, cos
        else:
            assert abs(lg - lc) < 0.05, (lg, lc)
            fg = [p for p in mg.ps.params if p.name == "logits/affine/weights"][0].grad.float().cpu().flatten()
            fc = [p for p in mc.ps.params if p.name == "logits/affine/weights"][0].grad.float().flatten()
            assert (fg @ fc / (fg.norm() * fc.norm() + 1e-12)).item() > 0.97
            # descent along the GPU's own gradient (eager passes on the same model)
            te = Trainer(mg, B, constant_lr(0.0), weight_decay=0.0, use_graph=False)
            te._forward_backward(img_g, lab_g)
            torch.cuda.synchronize()
            base, g = te.row_loss.mean().item(), mg.ps.grad.clone()
            mg.ps.master.sub_(0.05 * g / g.norm() * mg.ps.master.norm() * 1e-2)
            te._forward_backward(img_g, lab_g)
            torch.cuda.synchronize()
            assert te.row_loss.mean().item() < base
    finally:
        _reset()


def test_fp32_gradient_given_its_decisions():
    """The fp32 GPU gradient against the fp64 mirror forced to the GPU step's own ReLU masks and max-pool
    argmaxes (tests/test_fp32_zoo_gpu.py's check and bounds; LRN has no decision in it and runs as torch's
    own op in the mirror)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import zoo_flip_probe as ZP

    r = ZP.probe("alexnet", 32, B, seed=9, img_seed=4, data_name="cifar10")
    flips = sum(f for _, _, f, _ in r["flips"])
    assert r["gpu_vs_mirror_gpu"] < 1e-5, r
    assert r["cpu_vs_mirror_cpu"] < 1e-5, r
    assert flips <= 2, r["flips"]
    if flips == 0:
        assert r["gpu_vs_cpu"] < 1e-5, r


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_only_logits_match_cpu(dtype):
    try:
        mg, mc, img, lab = _pair(dtype, seed=11)
        tg = Trainer(mg, B, constant_lr(0.0), forward_only=True, use_graph=False)
        tc = Trainer(mc, B, constant_lr(0.0), forward_only=True)
        tg.step(img.to("cuda", mg.act_dtype), lab.cuda())
        tc.step(img, lab)
        torch.cuda.synchronize()
        out_g, out_c = Fn.from_planes(tg.logits).float().cpu(), tc.logits.float()
        rel = float((out_g - out_c).norm() / out_c.norm())
        print(f"forward_only {dtype}: {rel:.3e}")
        assert rel < (1e-4 if dtype == "fp32" else 5e-2), rel
    finally:
        _reset()


def test_cli_three_steps():
    cmd = [sys.executable, os.path.join(ROOT, "tf_cnn_benchmarks.py"), "--data_name=cifar10", "--model=alexnet",
           "--num_batches=3", "--num_warmup_batches=1", "--display_every=1", "--autotune=false"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fp32 (HIP kernels)" in r.stdout and "Batch size:  128 global" in r.stdout, r.stdout[-2000:]
    losses = [float(l.split("\t")[-1]) for l in r.stdout.splitlines() if l[:1].isdigit() and "images/sec" in l]
    assert len(losses) == 3 and all(l == l and abs(l) != float("inf") for l in losses), r.stdout[-2000:]
