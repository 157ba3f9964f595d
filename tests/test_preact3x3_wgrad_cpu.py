"""The CPU path of Fn.preact_conv3x3_wgrad (the definition of the pre-activation conv's fused weight gradient)
against autograd through the CPU path of Fn.preact_conv3x3_forward, in fp64: both sides are the same sums in
another order, so they agree to 1e-12 norm-relative."""
import pytest
import torch

from azure_hc_intel_tf_amd.ops import functional as Fn

EPS = 1e-5


@pytest.mark.parametrize("shape", [(2, 6, 8, 16, 32, 1), (2, 9, 12, 32, 16, 2)], ids=lambda s: "x".join(map(str, s)))
def test_preact_conv3x3_wgrad_cpu_is_the_gradient_of_the_forward(shape):
    N, H, W, C, nout, s = shape  # (stride 2: odd H pads the top, even W does not pad the left)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C + 8, generator=g, dtype=torch.float64)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    gamma, beta = gamma.double(), beta.double()
    w = torch.randn(nout, 3, 3, C, generator=g, dtype=torch.float64, requires_grad=True)
    xm = x[..., :C].reshape(-1, C)
    acc = torch.stack([xm.sum(0), (xm * xm).sum(0)]).unsqueeze(0)
    P, Q = -(-H // s), -(-W // s)
    out = torch.zeros(N, P, Q, nout, dtype=torch.float64)
    saved = Fn.preact_conv3x3_forward(x, w, gamma, beta, EPS, out, s, acc=acc, R=1, saved_mean=torch.empty_like(gamma),
                                      saved_invstd=torch.empty_like(gamma))
    dz = torch.randn(N, P, Q, nout + 8, generator=g, dtype=torch.float64)[..., 8:]
    (out * dz).sum().backward()
    ref = w.grad.reshape(nout, 9 * C)

    base = torch.randn(nout, 9 * C, generator=g, dtype=torch.float64)
    dw = base.clone()
    Fn.preact_conv3x3_wgrad(x, C, dz, gamma, beta, saved.mean, saved.invstd, dw, s)
    err = ((dw - base - ref).norm() / ref.norm()).item()
    assert ref.norm() > 0 and err < 1e-12, err
