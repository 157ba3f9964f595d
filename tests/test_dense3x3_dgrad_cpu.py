"""The CPU path of Fn.dense_conv3x3_dgrad (the definition of the dense layer's fused data gradient with the ReLU and
BatchNorm backward) against autograd of the forward formula with batch statistics, in fp64."""
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.ops import functional as Fn


def test_dense_conv3x3_dgrad_cpu_is_the_formula():
    N, H, W, C, nout, slot, eps = 2, 5, 6, 16, 12, 24, 1e-5
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    buf, G = rnd(N, H, W, 48), rnd(N, H, W, 48)
    G[..., slot + nout:slot + 16] = 0
    w = rnd(16, 3, 3, C)
    x = buf[..., :C].clone().requires_grad_(True)
    gamma, beta = (rnd(C) * 0.2 + 1).requires_grad_(True), rnd(C).requires_grad_(True)
    mean, var = x.mean((0, 1, 2)), x.var((0, 1, 2), unbiased=False)
    a = torch.relu((x - mean) * torch.rsqrt(var + eps) * gamma + beta)
    y = F.conv2d(a.permute(0, 3, 1, 2), w[:nout].permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), G[..., slot:slot + nout])
    G0 = G.clone()
    dgamma, dbeta = torch.full((C,), 9.0, dtype=torch.float64), torch.full((C,), 9.0, dtype=torch.float64)
    Fn.dense_conv3x3_dgrad(buf, C, G[..., slot:slot + 16], w, gamma.detach(), beta.detach(), mean.detach(),
                           torch.rsqrt(var + eps).detach(), G[..., :C], dgamma, dbeta, nout)
    assert torch.allclose(G[..., :C] - G0[..., :C], dx, rtol=1e-10, atol=1e-10)
    assert torch.allclose(dgamma, dg, rtol=1e-10, atol=1e-10) and torch.allclose(dbeta, db, rtol=1e-10, atol=1e-10)
    assert torch.equal(G[..., C:], G0[..., C:])
