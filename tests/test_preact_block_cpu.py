"""The CPU (definition) path of Fn.preact_block_inference against its parts composed in fp64:
Fn.preact_conv3x3_forward at inference, bn_inference + ReLU, F.conv2d and the add."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.ops import functional as Fn

EPS = 1e-5


@pytest.mark.parametrize("shape", [(2, 6, 8, 64, 64, 1), (3, 9, 7, 16, 32, 2)], ids=lambda s: "x".join(map(str, s)))
def test_preact_block_inference_cpu_is_its_parts(shape):
    N, H, W, C, nout, s = shape
    g = torch.Generator().manual_seed(7)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    x, w1, w2 = r(N, H, W, C + 8), r(nout, 3, 3, C) / 12, r(nout, 3, 3, nout) / 12
    bn1, bn2 = [[0.5 + r(c).abs(), r(c), r(c), 0.5 + r(c).abs()] for c in (C, nout)]
    P, Q = -(-H // s), -(-W // s)
    res = r(N, P, Q, nout)
    out = torch.full((N, P, Q, nout + 8), 7.0, dtype=torch.float64)
    Fn.preact_block_inference(x, w1, *bn1, EPS, w2, *bn2, EPS, res, out, s)

    z1 = torch.empty(N, P, Q, nout, dtype=torch.float64)
    Fn.preact_conv3x3_forward(x, w1, bn1[0], bn1[1], EPS, z1, s, running_mean=bn1[2], running_var=bn1[3])
    a2 = Fn.bn_inference(z1, *bn2, EPS, torch.empty_like(z1), True)
    ref = F.conv2d(a2.permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1) + res
    assert ((out[..., :nout] - ref).norm() / ref.norm()).item() < 1e-12
    assert bool((out[..., nout:] == 7.0).all())
