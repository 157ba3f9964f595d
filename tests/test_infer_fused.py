"""Fused inference conv + BN (``Fn.conv_bn_inference``, ``nn.layers.FUSE_INFER_BN``) on the CPU: there
the fused entry point is exactly ``conv_forward`` followed by ``bn_inference``, so the forward-only
numbers do not move with the switch."""
import pytest
import torch

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn import layers as L
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_cpu_fused_equals_conv_then_bn(relu, with_res):
    g = torch.Generator().manual_seed(3)
    spec = Fn.ConvSpec(cin=16, cin_pad=16, cout=24, kh=3, kw=3, sh=2, sw=2, pt=1, pl=1, pb=1, pr=1)
    x = torch.randn(2, 9, 9, 16, generator=g)
    w = torch.randn(24, 3, 3, 16, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(24, generator=g)
    beta = 0.2 * torch.randn(24, generator=g)
    mean = 0.1 * torch.randn(24, generator=g)
    var = torch.rand(24, generator=g) * 1.5 + 0.5
    P, Q = spec.out_hw(9, 9)
    res = torch.randn(2, P, Q, 24, generator=g) if with_res else None
    z = torch.empty(2, P, Q, 24)
    Fn.conv_forward(x, spec, None, w, z)
    want = Fn.bn_inference(z, gamma, beta, mean, var, 1e-5, torch.empty_like(z), relu, residual=res)
    got = Fn.conv_bn_inference(x, spec, None, w, gamma, beta, mean, var, 1e-5, torch.empty_like(z), relu,
                               residual=res)
    assert torch.equal(got, want)
    assert relu == bool((want >= 0).all())  # the case is not vacuous: negatives exist before the ReLU


def test_cpu_forward_only_resnet50_same_logits_with_switch(monkeypatch):
    logits = {}
    for on in (True, False):
        monkeypatch.setattr(L, "FUSE_INFER_BN", on)
        m = create_model("resnet50", device="cpu", image_size=64, seed=11, image_channels=8)
        gen = torch.Generator().manual_seed(5)
        for l in m.all_layers():
            if hasattr(l, "rmean"):
                l.rmean.data.copy_(torch.randn(l.rmean.data.shape, generator=gen) * 0.1)
                l.rvar.data.copy_(torch.rand(l.rvar.data.shape, generator=gen) * 1.5 + 0.5)
        img, lab = synthetic_batch(m, 2, seed=3)
        img[..., :3] = (img[..., :3] - 127.0) / 60.0
        t = Trainer(m, 2, constant_lr(0.0), forward_only=True)
        t.step(img, lab)
        logits[on] = t.logits.clone()
    assert torch.isfinite(logits[True]).all() and logits[True].abs().max() > 0
    assert torch.equal(logits[True], logits[False])


def test_switch_reads_environment(monkeypatch):
    monkeypatch.delenv("HCB_FUSE_INFER_BN", raising=False)
    assert L._env_on("HCB_FUSE_INFER_BN") is True
    monkeypatch.setenv("HCB_FUSE_INFER_BN", "0")
    assert L._env_on("HCB_FUSE_INFER_BN") is False
    monkeypatch.setenv("HCB_FUSE_INFER_BN", "1")
    assert L._env_on("HCB_FUSE_INFER_BN") is True
    # the module attribute is that reading, taken at import
    import os
    import subprocess
    import sys

    env = dict(os.environ, HCB_FUSE_INFER_BN="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c",
                        "from azure_hc_intel_tf_amd.nn import layers as L; print(L.FUSE_INFER_BN)"],
                       env=env, cwd=root, capture_output=True, text=True, check=True)
    assert r.stdout.strip() == "False"
