"""Fn.mbconv_block_inference on the CPU (the definition, at fp32) against its three parts composed in fp64."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.ops import functional as Fn

EPS = 1e-3


def parts_fp64(x, we, bn1, wd, bn2, wp, bn3, s, res):
    bn = lambda t, p: (t - p[2].double()) * torch.rsqrt(p[3].double() + EPS) * p[0].double() + p[1].double()
    h = x.double()
    if we is not None:
        h = bn(h @ we.double().reshape(we.shape[0], -1).t(), bn1).clamp(0, 6)
    (pt, pb), (pl, pr) = Fn.same_pads(x.shape[1], 3, s), Fn.same_pads(x.shape[2], 3, s)
    h = F.pad(h.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    h = F.conv2d(h, wd.double().unsqueeze(1), stride=s, groups=wd.shape[0]).permute(0, 2, 3, 1)
    o = bn(bn(h, bn2).clamp(0, 6) @ wp.double().reshape(wp.shape[0], -1).t(), bn3)
    return o + res.double() if res is not None else o


@pytest.mark.parametrize("shape", [(2, 6, 5, 8, 8, 6, 1), (1, 8, 6, 16, 24, 1, 2)], ids=["res", "t1_stride2"])
def test_cpu_definition_matches_fp64_parts(shape):
    N, H, W, cin, cout, t, s = shape
    mid = t * cin
    g = torch.Generator().manual_seed(3)
    r = lambda *sh: torch.randn(*sh, generator=g)
    bn = lambda c: [0.5 + torch.rand(c, generator=g), 0.3 * r(c), 0.2 * r(c), 0.5 + torch.rand(c, generator=g)]
    x = r(N, H, W, cin)
    we = r(mid, 1, 1, cin) * cin ** -0.5 if t != 1 else None
    wd, wp = r(mid, 3, 3) / 3, r(cout, 1, 1, mid) * mid ** -0.5
    bn1, bn2, bn3 = bn(mid), bn(mid), bn(cout)
    res = x if s == 1 and cin == cout else None
    out = torch.full((N, -(-H // s), -(-W // s), cout + 8), 7.0)
    Fn.mbconv_block_inference(x, we, bn1, EPS, wd, bn2, EPS, wp, bn3, EPS, out[..., :cout], s, res=res)
    ref = parts_fp64(x, we, bn1, wd, bn2, wp, bn3, s, res)
    assert bool((out[..., cout:] == 7.0).all())
    assert ((out[..., :cout].double() - ref).norm() / ref.norm()).item() < 1e-5
