"""MobileNet-v2 on the GPU kernels: the reduced network stem + (1,16,1,1) + (6,24,2,2) + (6,24,1,1,
identity add) + tail at 32x32, batch 4 -- one step against the CPU step at fp32 and bf16, the
captured step against the eager one, --forward_only logits, and one full-size step.

fp32 follows tests/test_fp32_zoo_gpu.py: the GPU gradient against an fp64 autograd MIRROR of the
network whose ReLU6 decisions (below 0 / inside / above 6, per element of every ReLU6 layer) are
forced to the GPU step's own, < 1e-5 relative; the CPU step against the mirror forced to ITS
decisions, < 1e-5; the decisions that differ between the two counted, at most 2; and with none
differing the GPU gradient against the CPU's, < 1e-5. (The helper of that file serves BN-free
sequential nets; this one mirrors BN with batch statistics, depthwise convs and the identity add.)
Measured on an MI355X: 0 of 589,824 decisions differ, GPU vs mirror 1.4e-7, CPU vs mirror 1.0e-7, GPU
vs CPU 1.7e-7. bf16: the bounds of tests/test_model_gpu.py (loss within 0.05, gradient cosine 0.97);
--forward_only: those of tests/test_forward_only_gpu.py (1e-4 / 5e-2; measured 3.5e-7 / 3.1e-3)."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

pytestmark = pytest.mark.gpu
SMALL = dict(image_size=32, blocks=((1, 16, 1, 1), (6, 24, 2, 2)), image_channels=8)


def _reset():
    Fn.set_f32_native(False)
    Fn.set_deterministic(False)
    set_gpu_compute_dtype(torch.bfloat16)


def _pair(dtype, seed=9):
    mg = create_model("mobilenet", device="cuda", compute_dtype=dtype, seed=seed, **SMALL)
    mc = create_model("mobilenet", device="cpu", seed=seed, **SMALL)
    assert mg.native and [b.identity for b in mg.blocks] == [False, False, True]
    assert torch.equal(mg.ps.master.cpu(), mc.ps.master)
    img, lab = synthetic_batch(mc, 4, seed=4)
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
    return mg, mc, img, lab


def _relu6_layers(m):
    out = [m.stem]
    for b in m.blocks:
        out += [l for l in (b.expand, b.dw) if l is not None]
    return out + [m.tail]


def _record(m):
    """Wrap the forward of every ReLU6 layer: its decision per output element, 0 (clipped at 0),
    1 (inside, the gradient passes) or 2 (clipped at 6), read from the activation the step wrote."""
    rec = {}
    for l in _relu6_layers(m):
        f = l.forward

        def fw(x, *a, _l=l, _f=f, **k):
            y = _f(x, *a, **k)
            v = (Fn.from_planes(y) if Fn.is_planes(y) else y).float().cpu()
            rec[_l.name] = (v > 0).to(torch.int8) + (v >= 6).to(torch.int8)
            return y
        l.forward = fw
    return rec


def _same(x, k, s):
    H, W = x.shape[2:]
    ph, pw = max((-(-H // s) - 1) * s + k - H, 0), max((-(-W // s) - 1) * s + k - W, 0)
    return F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


def mirror_grads(mc, images, labels, dec):
    """fp64 forward / backward of the network (NCHW, batch-statistics BN) with every ReLU6 decision
    taken from ``dec`` (layer name -> int8 NHWC states): inside passes v, the clipped states are the
    constants 0 and 6. Returns the flat gradient in the ParamStore's parameter order."""
    P = {p.name: p.data.detach().double().clone().requires_grad_(True) for p in mc.ps.params}

    def cbn(l, x, dw=False):
        if dw:
            w = P[l.w.name].view(-1, 1, 3, 3)
            z = F.conv2d(_same(x, 3, l.stride), w, stride=l.stride, groups=w.shape[0])
        else:
            w = P[l.w.name].permute(0, 3, 1, 2)
            z = F.conv2d(_same(x, l.spec.kh, l.spec.sh), w, stride=l.spec.sh)
        v = F.batch_norm(z, None, None, P[l.gamma.name], P[l.beta.name], True, 0.0, l.eps)
        if not l.relu:
            return v
        st = dec[l.name].permute(0, 3, 1, 2)
        return torch.where(st == 1, v, torch.where(st == 2, torch.full_like(v, 6.0), torch.zeros_like(v)))

    x = cbn(mc.stem, images.double().permute(0, 3, 1, 2))
    for b in mc.blocks:
        h = cbn(b.expand, x) if b.expand is not None else x
        h = cbn(b.project, cbn(b.dw, h, dw=True))
        x = x + h if b.identity else h
    feat = cbn(mc.tail, x).mean(dim=(2, 3))
    logits = feat @ P[mc.fc.w.name].view(mc.fc.ncls, -1).t() + P[mc.fc.b.name]
    F.cross_entropy(logits, labels).backward()
    return torch.cat([P[p.name].grad.reshape(-1) for p in mc.ps.params])


def test_fp32_gradient_given_its_decisions():
    try:
        mg, mc, img, lab = _pair("fp32")
        # gamma 3, beta 2 in the ReLU6 layers (both models): bn(z) ~ N(2, 3^2) puts about a quarter
        # of the elements below 0 and a tenth above 6 -- at the initial gamma 1 almost nothing clips at 6
        for l in _relu6_layers(mg) + _relu6_layers(mc):
            l.gamma.data.fill_(3.0)
            l.beta.data.fill_(2.0)
        rg, rc = _record(mg), _record(mc)
        tg = Trainer(mg, 4, constant_lr(0.0), weight_decay=0.0, use_graph=False)
        tg._forward_backward(img.cuda(), lab.cuda())
        torch.cuda.synchronize()
        gg = torch.cat([p.grad.reshape(-1).double().cpu() for p in mg.ps.params])
        tc = Trainer(mc, 4, constant_lr(0.0), weight_decay=0.0)
        tc._forward_backward(img, lab)
        gc = torch.cat([p.grad.reshape(-1).double() for p in mc.ps.params])
        names = [l.name for l in _relu6_layers(mc)]
        assert sorted(rg) == sorted(rc) == sorted(names) and len(names) == 7
        flips = [(n, int((rg[n] != rc[n]).sum()), rg[n].numel()) for n in names]
        for n in names:  # the three states all occur somewhere: the clip at 6 is exercised
            assert rg[n].shape == rc[n].shape
            tot = rg[n].numel()
            assert int((rg[n] == 2).sum()) * 50 >= tot and int((rg[n] == 0).sum()) * 10 >= tot, n
        mirror_g, mirror_c = mirror_grads(mc, img, lab, rg), mirror_grads(mc, img, lab, rc)

        def rel(a, b):
            return float((a - b).norm() / b.norm())
        r = {"flips": flips, "gpu_vs_mirror_gpu": rel(gg, mirror_g), "cpu_vs_mirror_cpu": rel(gc, mirror_c),
             "gpu_vs_cpu": rel(gg, gc)}
        print(r)
        nflips = sum(f for _, f, _ in flips)
        assert r["gpu_vs_mirror_gpu"] < 1e-5, r
        assert r["cpu_vs_mirror_cpu"] < 1e-5, r  # the mirror itself reproduces the CPU step
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
        for b in mg.blocks:  # every depthwise kernel got a gradient
            assert float(b.dw.w.grad.abs().max()) > 0
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
    m = create_model("mobilenet", device="cuda", compute_dtype=dtype, seed=3, **SMALL)
    img, lab = synthetic_batch(m, 4, seed=1)
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
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


def test_full_size_step_is_finite():
    try:
        m = create_model("mobilenet", device="cuda", compute_dtype="fp32", seed=2)
        img, lab = synthetic_batch(m, 2, seed=1)
        img[..., :3] = (img[..., :3] - 127.0) / 60.0
        loss = float(Trainer(m, 2, constant_lr(0.01), use_graph=False).step(img, lab))
        torch.cuda.synchronize()
        assert loss == loss and abs(loss) < 1e4
        assert bool(torch.isfinite(m.ps.grad).all()) and float(m.ps.grad.abs().max()) > 0
    finally:
        _reset()
