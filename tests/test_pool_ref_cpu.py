"""The fp64 pooling reference (tests/pool_ref.py) against fp64 F.max_pool2d / F.avg_pool2d autograd
over the whole pool case table, and the project's CPU path (Fn.pool_forward / pool_backward on fp32
CPU tensors, what the fp32-GPU-vs-CPU step tests take as the oracle) against the reference on
tie-heavy inputs: the first maximal element of a window keeps the gradient."""
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R
from azure_hc_intel_tf_amd.ops import functional as Fn

N, C = 2, 8


def _inputs(name):
    H, W, kh, kw, sh, sw, pads, is_max, incl_pad = R.CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    P, Q = R.out_hw(H, W, kh, kw, sh, sw, pads)
    if is_max:
        x = R.tie_heavy((N, H, W, C), gen)
        dy = R.int_grad((N, P, Q, C), gen)
        base = R.int_grad((N, H, W, C), gen)
    else:
        x = torch.randn((N, H, W, C), generator=gen)
        dy = torch.randn((N, P, Q, C), generator=gen)
        base = torch.randn((N, H, W, C), generator=gen)
    return x, dy, base


def _torch_pool(xt, kh, kw, sh, sw, pads, is_max, incl_pad):
    """NCHW fp64 pool by torch, padded as ops/functional.py pads: -inf (max) / 0 (average)."""
    pt, pb, pl, pr = pads
    if is_max:
        return F.max_pool2d(F.pad(xt, (pl, pr, pt, pb), value=-float("inf")), (kh, kw), (sh, sw))
    s = F.avg_pool2d(F.pad(xt, (pl, pr, pt, pb)), (kh, kw), (sh, sw), divisor_override=1)
    if incl_pad:
        return s / (kh * kw)
    ones = torch.ones_like(xt[:, :1])
    return s / F.avg_pool2d(F.pad(ones, (pl, pr, pt, pb)), (kh, kw), (sh, sw), divisor_override=1)


@pytest.mark.parametrize("name", list(R.CASES))
def test_pool_ref_matches_fp64_torch_autograd(name):
    H, W, kh, kw, sh, sw, pads, is_max, incl_pad = R.CASES[name]
    x, dy, _ = _inputs(name)
    x, dy = x.double(), dy.double()
    y, aux = R.pool_fwd_ref(x, kh, kw, sh, sw, pads, is_max, incl_pad)
    dx, mag = R.pool_bwd_ref(dy, x, kh, kw, sh, sw, pads, is_max, incl_pad)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    t = _torch_pool(xt, kh, kw, sh, sw, pads, is_max, incl_pad)
    (g,) = torch.autograd.grad(t, xt, dy.permute(0, 3, 1, 2))
    ty, tdx = t.detach().permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    if is_max:
        R.assert_exact(y, ty, "y")
        R.assert_exact(dx, tdx, "dx")
        assert int(aux.min()) >= 0 and int(aux.max()) < kh * kw
        # the recorded position holds the maximum, and no earlier tap of the window does
        for p in range(y.shape[1]):
            for q in range(y.shape[2]):
                for r in range(kh):
                    for s in range(kw):
                        h, w = p * sh - pads[0] + r, q * sw - pads[2] + s
                        if 0 <= h < H and 0 <= w < W:
                            eq = x[:, h, w] == y[:, p, q]
                            assert bool((eq | (aux[:, p, q] != r * kw + s)).all())
                            assert bool((~eq | (aux[:, p, q] <= r * kw + s)).all())
    else:
        assert float((y - ty).abs().max()) <= 1e-12
        assert float((dx - tdx).abs().max()) <= 1e-12
        assert bool((aux >= y.abs() - 1e-12).all()) and bool((mag >= dx.abs() - 1e-12).all())


def test_pool_ref_sampled_positions_equal_the_full_reference():
    H, W, kh, kw, sh, sw, pads, is_max, incl_pad = R.CASES["max_k5s2_same_9x11"]
    x, dy, _ = _inputs("max_k5s2_same_9x11")
    P, Q = R.out_hw(H, W, kh, kw, sh, sw, pads)
    gen = torch.Generator().manual_seed(1)
    for mx in (True, False):
        at = R.border_and_sample(P, Q, 4, gen)
        full = R.pool_fwd_ref(x, kh, kw, sh, sw, pads, mx)
        part = R.pool_fwd_ref(x, kh, kw, sh, sw, pads, mx, at=at)
        for f, s in zip(full, part):
            assert torch.equal(torch.stack([f[:, p, q] for p, q in at], 1), s)
        at = R.border_and_sample(H, W, 8, gen)
        assert {(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)} <= set(at)
        full = R.pool_bwd_ref(dy, x, kh, kw, sh, sw, pads, mx)
        part = R.pool_bwd_ref(dy, x, kh, kw, sh, sw, pads, mx, at=at)
        for f, s in zip(full, part):
            assert torch.equal(torch.stack([f[:, h, w] for h, w in at], 1), s)


def test_gap_ref_matches_fp64_torch():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(3, 7, 5, 8, generator=gen, dtype=torch.float64)
    y, mag = R.gap_fwd_ref(x)
    assert float((y - x.mean(dim=(1, 2))).abs().max()) <= 1e-14
    assert float((mag - x.abs().mean(dim=(1, 2))).abs().max()) <= 1e-14
    dx, dmag = R.gap_bwd_ref(y, 7, 5)
    assert torch.equal(dx, (y / 35).view(3, 1, 1, 8).expand(3, 7, 5, 8)) and torch.equal(dmag, dx.abs())


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_cpu_path_matches_pool_ref(name, accumulate):
    """fp32 CPU tensors through Fn.pool_forward / Fn.pool_backward: max pools exactly (ties to the
    first maximum), averages within fp32 rounding of the fp64 reference."""
    H, W, kh, kw, sh, sw, pads, is_max, incl_pad = R.CASES[name]
    x, dy, base = _inputs(name)
    ry, raux = R.pool_fwd_ref(x, kh, kw, sh, sw, pads, is_max, incl_pad)
    rdx, rmag = R.pool_bwd_ref(dy, x, kh, kw, sh, sw, pads, is_max, incl_pad)
    if accumulate:
        rdx, rmag = rdx + base.double(), rmag + base.double().abs()
    y = torch.empty(ry.shape, dtype=torch.float32)
    Fn.pool_forward(x, y, kh, kw, sh, sw, pads, is_max, incl_pad)
    dx = base.clone() if accumulate else torch.full(rdx.shape, float("nan"))
    Fn.pool_backward(dy, x, y, dx, kh, kw, sh, sw, pads, is_max, incl_pad, accumulate)
    if is_max:
        R.assert_exact(y, ry, "y")
        R.assert_exact(dx, rdx, "dx")
    else:
        R.assert_within(y, ry, raux, 2.0 ** -23, "y")
        R.assert_within(dx, rdx, rmag, 2.0 ** -23, "dx")
