"""A shrunken CIFAR-10 DenseNet (2 layers per block, k = 12, batch 4) on the MI355X against a plain PyTorch
fp64 autograd model on the TRUE channel counts, defined here: one captured-graph training step (loss, every
parameter gradient, the BN moving statistics) at the bounds tests/test_alexnet_cifar_gpu.py uses for its step
(fp32: loss 1e-4 relative, gradient cosine > 0.9999; bf16: loss 0.05, classifier-gradient cosine > 0.97); the
structural pads after three captured steps; FUSE_DENSE on / off."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn import layers as L
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

pytestmark = pytest.mark.gpu
B = 4


def _reset():
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)
    L.FUSE_DENSE = True


def _model(dtype):
    m = create_model("densenet40_k12", data_name="cifar10", device="cuda", compute_dtype=dtype, seed=5,
                     layers_per_block=2)
    img, lab = synthetic_batch(m, B, seed=4)
    img = img.float()
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
    if dtype != "fp32":
        img = img.to(torch.bfloat16).float()
    return m, img.to("cuda", m.act_dtype), lab.cuda()


def _selectors(m):
    """(parameter, index that picks its real channels) in the store's order, and the same for the BN buffers."""
    sel, bufs = {m.stem.w.name: (Ellipsis, slice(0, 3))}, []
    for b, blk in enumerate(m.blocks):
        for sub in blk.subs:
            keep = blk.keep[:sub.c_in]
            sel[sub.w.name] = (slice(0, blk.k), slice(None), slice(None), keep)
            sel[sub.gamma.name] = sel[sub.beta.name] = (keep,)
            bufs.append((sub.rmean, sub.rvar, keep))
        bn = m.trans[b][0] if b < 2 else m.final_bn
        sel[bn.gamma.name] = sel[bn.beta.name] = (blk.keep,)
        bufs.append((bn.rmean, bn.rvar, blk.keep))
        if b < 2:
            sel[m.trans[b][1].w.name] = (Ellipsis, blk.keep)
    sel[m.fc.w.name] = (Ellipsis, m.blocks[2].keep)
    return sel, bufs


def _reference(m, img, lab):
    """fp64 autograd DenseNet on the true channels; returns loss, gradients by name, moving (mean, var) per BN."""
    sel, _ = _selectors(m)
    P = {p.name: p.data.double().cpu()[sel.get(p.name, Ellipsis)].clone().requires_grad_(True) for p in m.ps.params}
    moving = []

    def bn_relu(x, name):
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        M = x.numel() // x.shape[1]
        moving.append((0.1 * mean.detach(), 0.9 + 0.1 * var.detach() * M / (M - 1)))
        v = lambda t: t[None, :, None, None]  # noqa: E731
        return F.relu((x - v(mean)) * v(torch.rsqrt(var + 1e-5) * P[f"{name}/batchnorm/gamma"]) + v(P[f"{name}/batchnorm/beta"]))

    conv = lambda x, w, pad: F.conv2d(x, w.permute(0, 3, 1, 2), padding=pad)  # noqa: E731
    x = img.double().cpu()[..., :3].permute(0, 3, 1, 2)
    x = conv(x, P["conv0/conv2d/kernel"], 1) + P["conv0/conv2d/bias"][None, :, None, None]
    for b in range(3):
        for i in range(m.n):
            name = f"block{b + 1}/layer{i + 1}"
            x = torch.cat([x, conv(bn_relu(x, name), P[f"{name}/conv2d/kernel"], 1)], 1)
        if b < 2:
            t = f"transition{b + 1}"
            x = F.relu(conv(bn_relu(x, t), P[f"{t}/conv/conv2d/kernel"], 0) + P[f"{t}/conv/conv2d/bias"][None, :, None, None])
            x = F.avg_pool2d(x, 2)
    x = bn_relu(x, "final").mean((2, 3))
    logits = x @ P["logits/affine/weights"].reshape(m.num_classes, -1).t() + P["logits/affine/biases"]
    loss = F.cross_entropy(logits, lab.cpu())
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in P.items()}, moving


def _cos(a, b):
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_step_matches_fp64_autograd(dtype):
    try:
        m, img, lab = _model(dtype)
        lr, gr, moving = _reference(m, img, lab)
        sel, bufs = _selectors(m)
        # lr 0, no weight decay: the warm-up step before the capture leaves the weights as they are; the moving
        # statistics are compared after ONE step, so they are put back before the last replay
        t = Trainer(m, B, constant_lr(0.0), weight_decay=0.0, use_graph=True)
        buf0 = m.ps.buf.clone()
        for _ in range(t.graph_warmup + 2):
            m.ps.buf.copy_(buf0)
            lg = float(t.step(img, lab))
        torch.cuda.synchronize()
        assert t._g_all is not None, "the step was not captured"
        names = [p.name for p in m.ps.params]
        gg = {p.name: p.grad.double().cpu()[sel.get(p.name, Ellipsis)].flatten() for p in m.ps.params}
        vg, vr = torch.cat([gg[n] for n in names]), torch.cat([gr[n].flatten() for n in names])
        # per parameter too, except where the true gradient is zero (the first conv's bias: every consumer of
        # its output is a batch norm, which removes a constant; both sides hold rounding noise there)
        worst = min((_cos(gg[n], gr[n].flatten()), n) for n in names if gr[n].norm() > 1e-6 * vr.norm())
        assert gr["conv0/conv2d/bias"].norm() < 1e-6 * vr.norm() and gg["conv0/conv2d/bias"].norm() < 1e-3 * vr.norm()
        ms = max(max(float((rm.data.double().cpu()[k] - a).norm() / a.norm()),
                     float((rv.data.double().cpu()[k] - v).norm() / v.norm())) for (rm, rv, k), (a, v) in zip(bufs, moving))
        print(f"{dtype}: loss {lg:.6f} ref {lr:.6f}, gradient cosine {_cos(vg, vr):.6f} rel "
              f"{float((vg - vr).norm() / vr.norm()):.3e}, worst parameter {worst}, moving statistics rel {ms:.3e}")
        assert bool(torch.isfinite(vg).all())
        if dtype == "fp32":
            assert abs(lg - lr) <= 1e-4 * abs(lr), (lg, lr)
            assert _cos(vg, vr) > 0.9999 and worst[0] > 0.9999, worst
            assert ms < 1e-4
        else:
            assert abs(lg - lr) < 0.05, (lg, lr)
            assert _cos(gg["logits/affine/weights"], gr["logits/affine/weights"].flatten()) > 0.97
            assert ms < 2e-2  # the 16-bit statistics bound of tests/test_kernels_gpu.py
    finally:
        _reset()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pads_stay_bit_zero_through_captured_training(dtype):
    try:
        m, img, lab = _model(dtype)
        t = Trainer(m, B, constant_lr(0.05), use_graph=True)
        for _ in range(t.graph_warmup + 3):
            loss = float(t.step(img, lab))
        torch.cuda.synchronize()
        assert t._g_all is not None and loss == loss
        sel, _ = _selectors(m)
        checked = 0
        for p in m.ps.params:
            if p.name not in sel or p.name == m.stem.w.name:
                continue
            real = torch.zeros(p.shape, dtype=torch.bool)
            real[sel[p.name]] = True
            mom = m.ps.momentum[p.offset:p.offset + p.numel].view(p.shape)
            for what, ten in (("value", p.data), ("gradient", p.grad), ("momentum", mom)):
                assert not ten.cpu()[~real].any(), (p.name, what)
            assert p.data.cpu()[real].any(), p.name
            checked += int((~real).sum())
        assert checked > 0
        m.forward(img)  # an eager forward: the blocks' buffers after training
        for blk in m.blocks:
            assert not blk._buf[..., ~blk.keep.to("cuda")].any(), blk.name
        m.clear()
    finally:
        _reset()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fuse_dense_on_and_off_give_the_same_loss(dtype):
    try:
        m, img, lab = _model(dtype)
        lr, _, _ = _reference(m, img, lab)
        losses = {}
        for on in (True, False):
            L.FUSE_DENSE = on
            t = Trainer(m, B, constant_lr(0.0), weight_decay=0.0, use_graph=False)
            losses[on] = float(t.step(img, lab))
        torch.cuda.synchronize()
        print(f"{dtype}: fused {losses[True]:.6f} unfused {losses[False]:.6f} ref {lr:.6f}")
        tol = 1e-4 * abs(lr) if dtype == "fp32" else 0.05
        assert abs(losses[True] - lr) <= tol and abs(losses[False] - lr) <= tol
        assert abs(losses[True] - losses[False]) <= tol
    finally:
        _reset()
