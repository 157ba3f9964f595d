"""The CIFAR-10 ResNets on the GPU kernels: the reduced network stem + one block per stage (an
identity block, then both plan-A pad-shortcut transitions 16 -> 32 and 32 -> 64) at 32x32, batch 4 -- one
step against the CPU step at fp32 and bf16, the captured step against the eager one, --forward_only
logits, one full ResNet-20 step, and the driver on a fake dataset.

fp32 follows tests/test_mobilenet_gpu.py / tests/test_fp32_zoo_gpu.py: the GPU gradient against an
fp64 autograd MIRROR of the network whose ReLU decisions (per element of every ReLU layer) are forced
to the GPU step's own, < 1e-5 relative; the CPU step against the mirror forced to ITS decisions,
< 1e-5; the decisions that differ between the two counted, at most 2; and with none differing the GPU
gradient against the CPU's, < 1e-5. Besides the flat gradient, the gamma and beta gradients of the two
BNs next to each pad shortcut (the BN that produces the shortcut's input and the BN pass that adds
its output) are held to the same bound tensor by tensor: they total 224 of 76,075 gradient elements, so
a wrong shortcut gradient could hide in the flat norm. Seed 9: the CPU step in float32 and in float64
(HCB_CPU_DTYPE) take the same 229,376 decisions, so no flip is expected from precision alone.
Measured on an MI355X: 0 of 229,376 decisions differ, GPU vs mirror 1.4e-7, CPU vs mirror 1.3e-7, GPU vs
CPU 1.8e-7. bf16: the bounds of tests/test_model_gpu.py (loss within 0.05, gradient cosine 0.97; measured
4e-5 and 0.99998); --forward_only: those of tests/test_forward_only_gpu.py (1e-4 / 5e-2; measured
3.7e-7 / 3.6e-3)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
SMALL = dict(layer_counts=(1, 1, 1), image_channels=8)
SEED = 9


def _reset():
    Fn.set_f32_native(False)
    Fn.set_deterministic(False)
    set_gpu_compute_dtype(torch.bfloat16)


def _batch(model, seed=4):
    img, lab = synthetic_batch(model, 4, seed=seed)
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
    return img, lab


def _pair(dtype, seed=SEED):
    mg = create_model("resnet20", device="cuda", compute_dtype=dtype, seed=seed, **SMALL)
    mc = create_model("resnet20", device="cpu", seed=seed, **SMALL)
    assert mg.native and [b.sc is not None for b in mg.blocks] == [False, True, True]
    assert torch.equal(mg.ps.master.cpu(), mc.ps.master)
    img, lab = _batch(mc)
    return mg, mc, img, lab


def _relu_layers(m):
    return [l for b in m.blocks for l in (b.c1, b.c2)]


def _record(m):
    """Wrap the forward of every ReLU layer: its decision per output element (1: the gradient passes),
    read from the activation the step wrote."""
    rec = {}
    for l in _relu_layers(m):
        f = l.forward

        def fw(x, *a, _l=l, _f=f, **k):
            y = _f(x, *a, **k)
            v = (Fn.from_planes(y) if Fn.is_planes(y) else y).float().cpu()
            rec[_l.name] = (v > 0).to(torch.int8)
            return y
        l.forward = fw
    return rec


def _same(x, k, s):
    H, W = x.shape[2:]
    ph, pw = max((-(-H // s) - 1) * s + k - H, 0), max((-(-W // s) - 1) * s + k - W, 0)
    return F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


def mirror_grads(mc, images, labels, dec):
    """fp64 forward / backward of the network (NCHW, batch-statistics BN, the plan-A shortcut as a
    strided slice + channel pad) with every ReLU decision taken from ``dec`` (layer name -> int8 NHWC).
    Returns {parameter name: gradient}."""
    P = {p.name: p.data.detach().double().clone().requires_grad_(True) for p in mc.ps.params}

    def cbn(l, x, res=None):
        z = F.conv2d(_same(x, l.spec.kh, l.spec.sh), P[l.w.name].permute(0, 3, 1, 2), stride=l.spec.sh)
        v = F.batch_norm(z, None, None, P[l.gamma.name], P[l.beta.name], True, 0.0, l.eps)
        if res is not None:
            v = v + res
        if not l.relu:
            return v
        return torch.where(dec[l.name].permute(0, 3, 1, 2) == 1, v, torch.zeros_like(v))

    x = cbn(mc.stem, images.double().permute(0, 3, 1, 2))
    for b in mc.blocks:
        sc = x
        if b.sc is not None:
            pad = (b.out_shape[2] - b.in_shape[2]) // 2
            sc = F.pad(x[:, :, ::b.sc.stride, ::b.sc.stride], (0, 0, 0, 0, pad, pad))
        x = cbn(b.c2, cbn(b.c1, x), res=sc)
    feat = x.mean(dim=(2, 3))
    logits = feat @ P[mc.fc.w.name].view(mc.fc.ncls, -1).t() + P[mc.fc.b.name]
    F.cross_entropy(logits, labels).backward()
    return {n: t.grad for n, t in P.items()}


def _flat(m, grads):
    return torch.cat([grads[p.name].reshape(-1) for p in m.ps.params])


def _own_grads(m):
    return {p.name: p.grad.detach().double().cpu().clone() for p in m.ps.params}


def _shortcut_bn_tensors(m):
    """gamma / beta of the BNs next to each pad shortcut: the producer of its input, the consumer of its output."""
    out = []
    for i, b in enumerate(m.blocks):
        if b.sc is not None:
            for l in (m.blocks[i - 1].c2, b.c2):
                out += [l.gamma.name, l.beta.name]
    return out


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_fp32_gradient_given_its_decisions():
    try:
        mg, mc, img, lab = _pair("fp32")
        rg, rc = _record(mg), _record(mc)
        tg = Trainer(mg, 4, constant_lr(0.0), weight_decay=0.0, use_graph=False)
        tg._forward_backward(img.cuda(), lab.cuda())
        torch.cuda.synchronize()
        gg = _own_grads(mg)
        tc = Trainer(mc, 4, constant_lr(0.0), weight_decay=0.0)
        tc._forward_backward(img, lab)
        gc = _own_grads(mc)
        names = [l.name for l in _relu_layers(mc)]
        assert sorted(rg) == sorted(rc) == sorted(names) and len(names) == 6
        flips = [(n, int((rg[n] != rc[n]).sum()), rg[n].numel()) for n in names]
        for n in names:  # both decisions occur in every layer
            assert rg[n].shape == rc[n].shape
            assert 0.1 < float(rg[n].float().mean()) < 0.9, n
        mirror_g, mirror_c = mirror_grads(mc, img, lab, rg), mirror_grads(mc, img, lab, rc)
        r = {"flips": flips, "gpu_vs_mirror_gpu": _rel(_flat(mc, gg), _flat(mc, mirror_g)),
             "cpu_vs_mirror_cpu": _rel(_flat(mc, gc), _flat(mc, mirror_c)), "gpu_vs_cpu": _rel(_flat(mc, gg), _flat(mc, gc))}
        per = {n: (_rel(gg[n], mirror_g[n]), _rel(gc[n], mirror_c[n])) for n in _shortcut_bn_tensors(mc)}
        print(r)
        print(per)
        assert len(per) == 6  # (stage 2's second BN is the consumer of one shortcut and the producer of the next)
        nflips = sum(f for _, f, _ in flips)
        assert r["gpu_vs_mirror_gpu"] < 1e-5, r
        assert r["cpu_vs_mirror_cpu"] < 1e-5, r  # the mirror itself reproduces the CPU step
        for n, (eg, ec) in per.items():
            assert eg < 1e-5 and ec < 1e-5, (n, eg, ec)
        assert nflips <= 2, flips
        if nflips == 0:
            assert r["gpu_vs_cpu"] < 1e-5, r
    finally:
        _reset()


def test_fp32_step_runs_no_pytorch_conv(monkeypatch):
    try:
        mg, mc, img, lab = _pair("fp32")
        calls = []
        real = F.conv2d
        monkeypatch.setattr(F, "conv2d", lambda *a, **k: (calls.append("conv2d"), real(*a, **k))[1])
        tg = Trainer(mg, 4, constant_lr(0.01), use_graph=False)
        lg = float(tg.step(img.cuda(), lab.cuda()))
        torch.cuda.synchronize()
        assert calls == [], "the GPU step must not run F.conv2d"
        monkeypatch.undo()
        lc = float(Trainer(mc, 4, constant_lr(0.01)).step(img, lab))
        assert abs(lg - lc) <= 1e-5 * abs(lc), (lg, lc)
    finally:
        _reset()


def test_bf16_step_matches_cpu_step():
    try:
        mg, mc, img, lab = _pair("bf16")
        lg = float(Trainer(mg, 4, constant_lr(0.01), use_graph=False).step(img.to("cuda", torch.bfloat16), lab.cuda()))
        lc = float(Trainer(mc, 4, constant_lr(0.01)).step(img, lab))
        gg, gc = mg.ps.grad.cpu(), mc.ps.grad
        cos = float(gg @ gc / (gg.norm() * gc.norm()))
        print(f"bf16: loss {lg} vs {lc}, gradient cosine {cos}")
        assert abs(lg - lc) < 0.05 and cos > 0.97, (lg, lc, cos)
    finally:
        _reset()


def _three_steps(use_graph, dtype="fp32"):
    m = create_model("resnet20", device="cuda", compute_dtype=dtype, seed=3, **SMALL)
    img, lab = _batch(m, seed=1)
    t = Trainer(m, 4, constant_lr(0.02), use_graph=use_graph, graph_warmup=1)
    losses = [float(t.step(img, lab)) for _ in range(3)]
    torch.cuda.synchronize()
    assert (t._g_all is not None) == use_graph
    return losses, m.ps.master.clone(), m.ps.buf.clone()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_equals_eager_bitwise_in_deterministic_mode(dtype):
    try:
        Fn.set_deterministic(True)
        eager = _three_steps(False, dtype)
        g1 = _three_steps(True, dtype)
        g2 = _three_steps(True, dtype)
        assert all(l == l for l in eager[0])
        assert g1[0] == g2[0] and torch.equal(g1[1], g2[1]) and torch.equal(g1[2], g2[2])
        assert g1[0] == eager[0] and torch.equal(g1[1], eager[1]) and torch.equal(g1[2], eager[2])
    finally:
        _reset()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_only_logits_match_cpu(dtype):
    try:
        mg, mc, img, lab = _pair(dtype, seed=11)
        g = torch.Generator().manual_seed(5)
        for a, b in zip(mg.layers, mc.layers):
            if hasattr(b, "rmean"):
                b.rmean.data.copy_(torch.randn(b.rmean.data.shape, generator=g) * 0.1)
                b.rvar.data.copy_(torch.rand(b.rvar.data.shape, generator=g) * 1.5 + 0.5)
                a.rmean.data.copy_(b.rmean.data)
                a.rvar.data.copy_(b.rvar.data)
        tg = Trainer(mg, 4, constant_lr(0.0), forward_only=True, use_graph=False)
        tc = Trainer(mc, 4, constant_lr(0.0), forward_only=True)
        tg.step(img.to("cuda", mg.act_dtype), lab.cuda())
        tc.step(img, lab)
        torch.cuda.synchronize()
        out_g, out_c = tg.logits.float().cpu(), tc.logits.float()
        rel = float((out_g - out_c).norm() / out_c.norm())
        print(f"forward_only {dtype}: {rel:.3e}")
        assert rel < (1e-4 if dtype == "fp32" else 5e-2), rel
    finally:
        _reset()


def test_full_resnet20_step_is_finite():
    try:
        m = create_model("resnet20", device="cuda", compute_dtype="fp32", seed=2)
        img, lab = synthetic_batch(m, 2, seed=1)
        img[..., :3] = (img[..., :3] - 127.0) / 60.0
        loss = float(Trainer(m, 2, constant_lr(0.01), use_graph=False).step(img, lab))
        torch.cuda.synchronize()
        assert loss == loss and abs(loss) < 1e4
        assert bool(torch.isfinite(m.ps.grad).all()) and float(m.ps.grad.abs().max()) > 0
    finally:
        _reset()


def test_driver_trains_and_evaluates_on_fake_pickles(tmp_path, capsys):
    import make_fake_cifar10

    from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN
    from azure_hc_intel_tf_amd.bench.flags import parse_flags

    per_file = 20
    make_fake_cifar10.make(str(tmp_path), per_file=per_file, seed=2)
    flags = ["--model=resnet20", "--data_name=cifar10", f"--data_dir={tmp_path}", "--num_batches=3",
             "--num_warmup_batches=1", "--autotune=false", "--batch_size=16", "--display_every=1"]
    try:
        b = BenchmarkCNN(parse_flags(flags))
        b.print_info()
        s = b.run()
        out = capsys.readouterr().out
        assert "Dataset:     cifar10 (python pickles" in out and "fp32 (HIP kernels)" in out
        assert s["data"] == "cifar10-pickle" and s["num_batches"] == 3 and s["hip_graph"]
        assert s["final_loss"] == s["final_loss"] and 0 < s["final_loss"] < 20
        # (no --num_batches: one pass over the test split)
        e = BenchmarkCNN(parse_flags([f for f in flags if not f.startswith("--num_batches")] + ["--eval"]))
        r = e.run()
        assert r["eval"]["examples"] == per_file  # 16 + 4 real rows, 12 padding rows skipped
        assert 0.0 <= r["eval"]["top_1_accuracy"] <= r["eval"]["top_5_accuracy"] <= 1.0
    finally:
        _reset()
