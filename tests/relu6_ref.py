"""Shared inputs and the fp64 reference of the ReLU6 BatchNorm tests (CPU and GPU)."""
import torch
import torch.nn.functional as F

EPS = 1e-3
MARGIN = 1e-3


def make_case(M: int, C: int, seed: int = 0, dtype=torch.float32):
    """z [M, C], gamma, beta, dy (z and dy already rounded to ``dtype``, returned as fp32) such that
    in fp64, on the rounded values, every bn(z) element is at least MARGIN away from 0 and from 6 and
    each of the three regions (< 0, inside, > 6) holds at least a fifth of the elements: draw, then
    push offenders away (in z, rounding and re-normalising until none is left). The caller asserts
    both conditions on the fp64 reference (assert_regions)."""
    g = torch.Generator().manual_seed(seed)
    gamma = 4.0 + torch.rand(C, generator=g, dtype=torch.float64)  # bn(z) ~ N(3, ~4.5^2): a quarter below 0 and above 6
    beta = 3.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    z = torch.randn(M, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gq, bq = gamma.float().double(), beta.float().double()
    for _ in range(500):
        zq = z.to(dtype).double()  # what the kernel will read
        v = bn64(zq, gq, bq)[0]
        bad = (v.abs() < 4 * MARGIN) | ((v - 6).abs() < 4 * MARGIN)
        if not bool(bad.any()):
            break
        z = torch.where(bad, zq + 0.05 * torch.sign(zq + 1e-12), zq)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    return z.to(dtype).float(), gamma.float(), beta.float(), dy.to(dtype).float()


def bn64(z, gamma, beta):
    """(v = bn(z), mean, invstd) in fp64 with batch statistics."""
    mean = z.mean(0)
    var = z.var(0, unbiased=False)
    invstd = torch.rsqrt(var + EPS)
    return (z - mean) * invstd * gamma + beta, mean, invstd


def ref64(z, gamma, beta, dy, act: str = "relu6"):
    """fp64 autograd of y = act(bn(z)), act in none | relu | relu6:
    (v, y, dz, dgamma, dbeta, gres = dy * mask)."""
    z = z.double().clone().requires_grad_(True)
    gamma = gamma.double().clone().requires_grad_(True)
    beta = beta.double().clone().requires_grad_(True)
    v, _, _ = bn64(z, gamma, beta)
    if act == "relu6":
        y, mask = F.hardtanh(v, 0.0, 6.0), (v > 0) & (v < 6)
    elif act == "relu":
        y, mask = torch.relu(v), v > 0
    else:
        y, mask = v, torch.ones_like(v, dtype=torch.bool)
    y.backward(dy.double())
    return v.detach(), y.detach(), z.grad, gamma.grad, beta.grad, dy.double() * mask.double()


def assert_regions(v):
    """The three regions each hold a fifth of the elements; no element within MARGIN of a threshold."""
    n = v.numel()
    assert int((v < 0).sum()) * 5 >= n and int((v > 6).sum()) * 5 >= n and int(((v > 0) & (v < 6)).sum()) * 5 >= n
    assert float(v.abs().min()) >= MARGIN and float((v - 6).abs().min()) >= MARGIN
