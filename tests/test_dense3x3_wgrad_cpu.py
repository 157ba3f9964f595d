"""The CPU path of Fn.dense_conv3x3_wgrad (the definition of the dense layer's fused weight gradient) against
autograd of the forward formula, in fp64."""
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.ops import functional as Fn


def test_dense_conv3x3_wgrad_cpu_is_the_formula():
    N, H, W, C, nout, slot = 2, 5, 6, 16, 12, 24
    g = torch.Generator().manual_seed(0)
    buf = torch.randn(N, H, W, 48, generator=g, dtype=torch.float64)
    G = torch.randn(N, H, W, 48, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    mean, invstd = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    w = torch.zeros(nout, 3, 3, C, dtype=torch.float64, requires_grad=True)
    a = torch.relu((buf[..., :C] - mean) * invstd * gamma + beta)
    y = F.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    (ref,) = torch.autograd.grad(y, w, G[..., slot:slot + nout])
    base = torch.randn(16, 9 * C, generator=g, dtype=torch.float64)
    dw = base.clone()
    Fn.dense_conv3x3_wgrad(buf, C, G[..., slot:slot + 16], gamma, beta, mean, invstd, dw, nout)
    assert torch.allclose(dw[:nout] - base[:nout], ref.reshape(nout, 9 * C), rtol=1e-12, atol=1e-12)
    assert torch.equal(dw[nout:], base[nout:])
