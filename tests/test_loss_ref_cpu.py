"""The plain references of tests/loss_ref.py against something independent of them (fp64
F.cross_entropy(label_smoothing=) and its autograd gradient, an integer-arithmetic bf16 rounding,
math.fsum), and the project's CPU paths (Fn.softmax_xent / colsum / loss_total / relu_backward /
to_planes / from_planes on CPU tensors, the oracle of the GPU-vs-CPU step tests) against the
references. Also pins the domain on which the three-plane split of an fp32 value is exact."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from azure_hc_intel_tf_amd.ops import functional as Fn

NCLS = (5, 11, 100, 256, 257, 1000, 1001)


def _logits(B, ncls, ld, seed):
    gen = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, ld, generator=gen) * 3
    lab = torch.randint(0, ncls, (B,), generator=gen)
    lab[0], lab[-1] = 0, ncls - 1
    return lg, lab


# ------------------------------------------------------------------ references vs independent
@pytest.mark.parametrize("ls", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("ncls", NCLS)
def test_softmax_ref_matches_torch_cross_entropy_fp64(ncls, ls):
    lg, lab = _logits(3, ncls, ncls + 7, ncls)
    lg[1] += 1e4  # fp64 on both sides: the shift costs nothing
    z = lg[:, :ncls].double().clone().requires_grad_(True)
    loss = F.cross_entropy(z, lab, label_smoothing=ls, reduction="none")
    loss.sum().backward()
    rl, dl = R.softmax_xent_ref(lg, lab, ncls, 0.25, ls)
    # fp64 on both sides. logsumexp of the shifted row rounds at 1e4 * 2^-53 = 1.1e-12: that is the
    # absolute error of the loss and, through exp, the relative error of each probability (a few
    # such roundings on either side: 1e-11; absolute, as p - 1 at the label cancels)
    assert torch.allclose(rl, loss.detach(), rtol=1e-12, atol=1e-11)
    assert torch.allclose(dl, 0.25 * z.grad, rtol=0, atol=1e-11)
    assert dl.sum(1).abs().max().item() < 1e-11  # softmax - target sums to 0


def test_colsum_and_loss_total_refs_match_fsum():
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(37, 16, generator=gen)
    s, a = R.colsum_ref(g, 30, 11)
    assert s.shape == (11,) and a.shape == (11,)
    for n in range(11):
        col = [float(v) for v in g[:30, n]]
        assert abs(s[n].item() - math.fsum(col)) <= 1e-14 * a[n].item()
        assert abs(a[n].item() - math.fsum(abs(v) for v in col)) <= 1e-14 * a[n].item()
    row, l2 = torch.rand(20, generator=gen), torch.rand(9, generator=gen)
    want = math.fsum(float(v) for v in row[:13]) / 13
    assert abs(R.loss_total_ref(row, 13, None, 0.5) - want) <= 1e-15
    want += 0.25 * math.fsum(float(v) for v in l2)
    assert abs(R.loss_total_ref(row, 13, l2, 0.25) - want) <= 1e-15


def test_split3_ref_matches_integer_rounding():
    """torch's CPU bf16 cast is round-to-nearest-even: the same bits as the integer formula, for
    each of the three casts, on random bit patterns over the whole finite normal range."""
    x = R.domain_bits((1 << 16,), torch.Generator().manual_seed(3), emin=1, emax=253)
    hi, mid, lo = R.split3_ref(x)
    assert np.array_equal(R.bits16(hi).numpy().astype(np.uint16), R.bf16_rne_bits(x))
    r = x - hi.float()
    assert np.array_equal(R.bits16(mid).numpy().astype(np.uint16), R.bf16_rne_bits(r))
    assert np.array_equal(R.bits16(lo).numpy().astype(np.uint16), R.bf16_rne_bits(r - mid.float()))
    # x - hi is exact in fp32 (the residual has at most 16 significant bits)
    assert torch.equal(r.double(), x.double() - hi.double())


# ------------------------------------------------------------------ CPU paths vs references
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("ncls", NCLS)
def test_cpu_softmax_xent_matches_ref(ncls, ls):
    B, ld, lddl = 8, (ncls + 7) // 8 * 8 + 8, (ncls + 7) // 8 * 8
    lg, lab = _logits(B, ncls, ld, 100 + ncls)
    lg[:, ncls:] = float("inf")  # padding columns are never read
    lg[2, :ncls] = 1.5           # all equal
    lg[3, 1] = 60.0              # one dominant logit
    scale_dev = torch.tensor([128.0])
    rl = torch.full((B,), float("nan"))
    dl = torch.full((B, lddl), float("nan"))
    Fn.softmax_xent(lg, lab, ncls, rl, dl, 1.0 / B, scale_dev=scale_dev, label_smoothing=ls)
    ref_l, ref_d = R.softmax_xent_ref(lg, lab, ncls, 128.0 / B, ls)
    # fp32 torch arithmetic at logits of order 10 (test_label_smoothing.py's figures)
    assert torch.allclose(rl.double(), ref_l, rtol=1e-5, atol=1e-5)
    assert (dl[:, :ncls].double() - ref_d).abs().max().item() < 1e-6 * 128.0 / B
    assert torch.equal(dl[:, ncls:], torch.zeros(B, lddl - ncls))


def test_cpu_colsum_loss_total_relu_match_ref():
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(70, 264, generator=gen)
    g[65:] = float("nan")
    g[:, 257:] = float("nan")
    out = torch.full((260,), -77.0)
    Fn.colsum(g, 65, 257, out[:257])
    s, a = R.colsum_ref(g, 65, 257)
    assert ((out[:257].double() - s).abs() <= 65 * 2.0 ** -24 * a).all()
    assert torch.equal(out[257:], torch.full((3,), -77.0))

    row = torch.rand(300, generator=gen)
    row[257:] = float("nan")
    loss = torch.empty(1)
    for l2 in (None, torch.rand(1, generator=gen), torch.rand(300, generator=gen)):
        Fn.loss_total(row, 257, l2, 0.5 * 4e-5, loss)
        ref = R.loss_total_ref(row, 257, l2, 0.5 * 4e-5)
        assert abs(loss.item() - ref) <= 2e-6 * abs(ref), (l2 is None or l2.numel(), loss.item(), ref)

    y = torch.randn(8 * 33, generator=gen)
    y[:6] = torch.tensor([0.0, -0.0, float("inf"), float("nan"), -float("inf"), 1e-30])
    dy = torch.randn(8 * 33, generator=gen)
    dy[7] = -0.0
    dz = torch.full_like(dy, float("nan"))
    Fn.relu_backward(dy, y, dz)
    assert torch.equal(dz, torch.where(y > 0, dy, torch.zeros_like(dy)))
    assert torch.equal(R.bits32(dz)[y > 0], R.bits32(dy)[y > 0])


# ------------------------------------------------------------------ the plane split's domain
def _roundtrip(x):
    return Fn.from_planes(Fn.to_planes(x))


def test_cpu_planes_match_ref_and_are_exact_on_the_domain():
    """from_planes(to_planes(x)) is bit-exact for finite 2^-100 <= |x| <= 2^127 and for +0."""
    gen = torch.Generator().manual_seed(7)
    x = R.domain_bits((1 << 17, 8), gen)
    x[0] = torch.tensor([2.0 ** 127, -(2.0 ** 127), 2.0 ** -100, -(2.0 ** -100), 0.0, 1.0, -1.0, 3.0])
    p = Fn.to_planes(x)
    for got, want in zip(p.t, R.split3_ref(x)):
        assert torch.equal(R.bits16(got), R.bits16(want))
    # hi + mid + lo in fp64 is the value itself: the split loses nothing on the domain
    assert torch.equal(p.t[0].double() + p.t[1].double() + p.t[2].double(), x.double())
    assert torch.equal(R.bits32(_roundtrip(x)), R.bits32(x))


def test_cpu_planes_outside_the_domain():
    """What the docstring of to_planes states: -0 comes back as +0 (equal, other bits); below
    2^-110 the lo plane underflows bf16 (its last bit, 2^-23 |x|, is under the subnormal step 2^-133)
    and the value is no longer exact; where the hi plane
    rounds to Inf the merged value is NaN (Inf - Inf in the residual), as for Inf and NaN inputs."""
    z = _roundtrip(torch.full((8,), -0.0))
    assert torch.equal(z, torch.zeros(8)) and int(R.bits32(z).abs().max()) == 0
    tiny = R.domain_bits((1 << 14, 8), torch.Generator().manual_seed(8), emin=1, emax=16)  # 2^-126 <= |x| < 2^-110
    back = _roundtrip(tiny)
    assert not torch.equal(back, tiny)
    # the last plane written rounds to a multiple of the bf16 subnormal step 2^-133: half a step
    assert ((back.double() - tiny.double()).abs() <= 2.0 ** -134).all()
    big = torch.full((8,), 3.4e38)
    assert torch.isinf(Fn.to_planes(big).t[0].float()).all()
    assert torch.isnan(_roundtrip(big)).all()
    for v in (float("inf"), -float("inf"), float("nan")):  # hi = v, and v - v is NaN
        assert torch.isnan(_roundtrip(torch.full((8,), v))).all()
