"""ReLU6 in the reference BatchNorm (ops.functional.bn_forward / bn_backward, ``act_max`` and
``relu_mode`` 3) against fp64 autograd of hardtanh(bn(z), 0, 6); the calls without the new arguments
are unchanged."""
import pytest
import torch

from azure_hc_intel_tf_amd.ops import functional as Fn
from relu6_ref import EPS, assert_regions, make_case, ref64

SHAPES = [(6, 8), (6, 40), (130, 8), (130, 40)]


def _run(z, gamma, beta, dy, dtype, **fwd_kw):
    M, C = z.shape
    z4, dy4 = z.to(dtype).view(M, 1, 1, C), dy.to(dtype).view(M, 1, 1, C)
    gm, bt = gamma.to(dtype), beta.to(dtype)
    y = torch.empty_like(z4)
    saved = Fn.bn_forward(z4, gm, bt, None, None, 0.9, EPS, y, True, **fwd_kw)
    return z4, dy4, gm, bt, y, saved


@pytest.mark.parametrize("M,C", SHAPES)
def test_reference_relu6_matches_autograd(M, C):
    z, gamma, beta, dy = make_case(M, C)
    v, yr, dzr, dgr, dbr, gr = ref64(z, gamma, beta, dy)
    assert_regions(v)
    z4, dy4, gm, bt, y, saved = _run(z, gamma, beta, dy, torch.float64, act_max=6.0)
    assert torch.allclose(y.view(M, C), yr, rtol=1e-12, atol=1e-12)
    dz, gres = torch.empty_like(z4), torch.empty_like(z4)
    dg, db = torch.empty(C, dtype=torch.float64), torch.empty(C, dtype=torch.float64)
    Fn.bn_backward(dy4, None, z4, saved, gm, bt, 3, dg, db, dz, gres)
    for name, got, ref in (("dz", dz.view(M, C), dzr), ("dgamma", dg, dgr), ("dbeta", db, dbr),
                           ("gres", gres.view(M, C), gr)):
        assert torch.allclose(got, ref, rtol=1e-9, atol=1e-10), name


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_modes_without_the_new_argument_are_bitwise_unchanged(mode):
    z, gamma, beta, dy = make_case(130, 40, seed=1)
    a = _run(z, gamma, beta, dy, torch.float32)
    b = _run(z, gamma, beta, dy, torch.float32, act_max=None)
    assert torch.equal(a[4], b[4]) and torch.equal(a[4], torch.relu(a[4]))
    assert float(a[4].max()) > 6.0, "plain ReLU does not clip"
    outs = []
    for (z4, dy4, gm, bt, y, saved) in (a, b):
        dz, gres = torch.empty_like(z4), torch.empty_like(z4)
        dg, db = torch.empty(40), torch.empty(40)
        Fn.bn_backward(dy4, y, z4, saved, gm, bt, mode, dg, db, dz, gres)
        outs.append((dz, gres, dg, db))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    y1 = torch.empty_like(a[0])
    Fn.bn_inference(a[0], a[2], a[3], torch.zeros(40), torch.ones(40), EPS, y1, True)
    y2 = torch.empty_like(a[0])
    Fn.bn_inference(a[0], a[2], a[3], torch.zeros(40), torch.ones(40), EPS, y2, True, act_max=None)
    y3 = torch.empty_like(a[0])
    Fn.bn_inference(a[0], a[2], a[3], torch.zeros(40), torch.ones(40), EPS, y3, True, act_max=6.0)
    assert torch.equal(y1, y2) and torch.equal(y3, y1.clamp(max=6.0))
