"""Numerics of every hand-written gfx950 kernel against the fp32 PyTorch reference path of
the same op (the CPU implementation in ops/functional.py). Runs on an MI355X via gpurun."""
import math

import pytest
import torch

from azure_hc_intel_tf_amd.nn.params import ParamStore
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.ops.functional import ConvSpec

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bf(t):
    return t.to(torch.bfloat16)


def rel_err(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def make_conv(cin, cout, kh, kw, sh=1, sw=1, pads=(0, 0, 0, 0), seed=0, cin_pad=None, need_tr=True):
    cin_pad = cin_pad or cin
    pt, pb, pl, pr = pads
    spec = ConvSpec(cin=cin, cin_pad=cin_pad, cout=cout, kh=kh, kw=kw, sh=sh, sw=sw, pt=pt, pl=pl, pb=pb, pr=pr)
    ps = ParamStore(seed=seed)
    p = ps.add("w", (cout, kh, kw, cin_pad), True, ps.variance_scaling(kh * kw * cin, cin if cin != cin_pad else -1))
    pk = ps.add_pack(p, cout, kh, kw, cin_pad, spec.Kpad, spec.Kpad_t, want_tr=need_tr)
    ps.finalize(DEV)
    ps.repack()
    return spec, p, pk


CONV_CASES = [
    # cin, cout, kh, kw, stride, pads, H  (ResNet-50 shapes at small batch + Inception-style)
    (64, 256, 1, 1, 1, (0, 0, 0, 0), 14),
    (256, 64, 1, 1, 1, (0, 0, 0, 0), 14),
    (64, 64, 3, 3, 1, (1, 1, 1, 1), 14),
    (256, 512, 1, 1, 2, (0, 0, 0, 0), 14),
    (128, 128, 3, 3, 2, (1, 1, 1, 1), 14),
    (8, 64, 7, 7, 2, (3, 3, 3, 3), 32),      # stem (3 channels padded to 8)
    (80, 192, 3, 3, 1, (0, 0, 0, 0), 11),     # Inception: generic-C path, VALID
    (128, 192, 1, 7, 1, (0, 0, 3, 3), 9),     # asymmetric 1x7
    (160, 160, 7, 1, 1, (3, 3, 0, 0), 9),     # 7x1
    (48, 64, 5, 5, 1, (2, 2, 2, 2), 9),       # 5x5
    (32, 48, 3, 3, 2, (0, 0, 0, 0), 15),      # 3x3/2 VALID
    (2048, 1001 + 7, 1, 1, 1, (0, 0, 0, 0), 1),  # FC-like, Nout not a multiple of the tile
]


def cpu_ref_conv(x, spec, w):
    out = torch.empty((x.shape[0],) + spec.out_hw(x.shape[1], x.shape[2]) + (spec.cout,))
    return Fn.conv_forward(x.float().cpu(), spec, None, w.float().cpu(), out)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}x{c[1]}k{c[2]}{c[3]}s{c[4]}")
def test_conv_fwd_and_stats(case):
    cin, cout, kh, kw, s, pads, H = case
    torch.manual_seed(0)
    cpad = cin if cin % 8 == 0 else 8
    spec, p, pk = make_conv(cin, cout, kh, kw, s, s, pads, cin_pad=cpad)
    N = 3
    x = bf(torch.randn(N, H, H, cpad, device=DEV))
    P, Q = spec.out_hw(H, H)
    y = torch.empty(N, P, Q, cout, dtype=torch.bfloat16, device=DEV)
    slab, T, cfg = Fn.conv_stats_slab(x.shape, spec, DEV)
    Fn.conv_forward(x, spec, pk.pack, p.data, y, stats=slab, cfg=cfg)
    ref = cpu_ref_conv(x, spec, bf(p.data))
    assert rel_err(y, ref) < 1e-2
    s1 = slab.view(T, 2, cout).sum(0)[0].cpu()
    assert rel_err(s1, ref.reshape(-1, cout).sum(0)) < 2e-2


@pytest.mark.parametrize("case", CONV_CASES[:-1], ids=lambda c: f"{c[0]}x{c[1]}k{c[2]}{c[3]}s{c[4]}")
def test_conv_lds_dma_kernels_all_geometries(case):
    """The LDS-DMA ring kernels (cfg 4-16, and 22-26 with two k-steps per ring stage) on every
    geometry, forward and data-gradient."""
    cin, cout, kh, kw, s, pads, H = case
    torch.manual_seed(12)
    cpad = cin if cin % 8 == 0 else 8
    spec, p, pk = make_conv(cin, cout, kh, kw, s, s, pads, cin_pad=cpad)
    N = 2
    P, Q = spec.out_hw(H, H)
    x = bf(torch.randn(N, H, H, cpad, device=DEV))
    ref = cpu_ref_conv(x, spec, bf(p.data))
    dz = bf(torch.randn(N, P, Q, cout, device=DEV))
    dref = torch.empty(N, H, H, cpad)
    Fn.conv_dgrad(dz.float().cpu(), spec, None, bf(p.data).float().cpu(), dref, False)
    for cfg in list(range(4, 17)):
        y = torch.empty(N, P, Q, cout, dtype=torch.bfloat16, device=DEV)
        slab = torch.empty(math.ceil(N * P * Q / Fn._CONV_TILES[cfg][0]) * 2 * cout, device=DEV)
        Fn.conv_forward(x, spec, pk.pack, p.data, y, stats=slab, cfg=cfg)
        assert rel_err(y, ref) < 1e-2, cfg
        if cin % 8 == 0:
            dx = torch.zeros(N, H, H, cpad, dtype=torch.bfloat16, device=DEV)
            Fn.conv_dgrad(dz, spec, pk.tr, p.data, dx, False, cfg=cfg)
            assert rel_err(dx, dref) < 1e-2, cfg


@pytest.mark.parametrize("cfg", list(range(22)))
def test_conv_fwd_all_tile_configs(cfg):
    torch.manual_seed(1)
    spec, p, pk = make_conv(128, 192, 3, 3, 1, 1, (1, 1, 1, 1))
    x = bf(torch.randn(2, 13, 13, 128, device=DEV))
    y = torch.empty(2, 13, 13, 192, dtype=torch.bfloat16, device=DEV)
    Fn.conv_forward(x, spec, pk.pack, p.data, y, cfg=cfg)
    assert rel_err(y, cpu_ref_conv(x, spec, bf(p.data))) < 1e-2


@pytest.mark.parametrize("plan", [(4, 2), (4, 3), (12, 2), (13, 4), (14, 2), (16, 3), (6, 5), (22, 3), (23, 2),
                                  (26, 5)])
def test_conv_split_k_in_launch_reduction(plan):
    """split-K: partial tiles parked in the workspace, the last arriver (agent-scope ticket)
    sums them and runs the normal epilogue (BN statistics, beta-accumulate, BN-bwd fusion)."""
    torch.manual_seed(7)
    spec, p, pk = make_conv(128, 256, 3, 3, 1, 1, (1, 1, 1, 1))
    N, H = 4, 14
    x = bf(torch.randn(N, H, H, 128, device=DEV))
    y = torch.empty(N, H, H, 256, dtype=torch.bfloat16, device=DEV)
    acc = torch.zeros(8 * 2 * 256, device=DEV)
    for rep in range(2):  # second pass checks that the tickets were left re-armed
        acc.zero_()
        Fn.conv_forward(x, spec, pk.pack, p.data, y, stats=acc, stats_R=8, cfg=plan)
        ref = cpu_ref_conv(x, spec, bf(p.data))
        assert rel_err(y, ref) < 1e-2, rep
        assert rel_err(acc.view(8, 2, 256).sum(0)[0], ref.reshape(-1, 256).sum(0)) < 2e-2
    dz = bf(torch.randn(N, H, H, 256, device=DEV))
    base = bf(torch.randn(N, H, H, 128, device=DEV))
    dx = base.clone()
    Fn.conv_dgrad(dz, spec, pk.tr, p.data, dx, True, cfg=plan)
    dref = torch.empty(N, H, H, 128)
    Fn.conv_dgrad(dz.float().cpu(), spec, None, bf(p.data).float().cpu(), dref, False)
    assert rel_err(dx, dref + base.float().cpu()) < 1e-2
    assert int(Fn._splitk["cnt"].abs().sum().item()) == 0


def test_conv_fwd_channel_slice_views():
    """input is a channel window of a wider buffer and output lands in a concat window"""
    torch.manual_seed(2)
    spec, p, pk = make_conv(64, 96, 3, 3, 1, 1, (1, 1, 1, 1))
    big = bf(torch.randn(2, 9, 9, 192, device=DEV))
    x = big[..., 64:128]
    outbuf = torch.zeros(2, 9, 9, 256, dtype=torch.bfloat16, device=DEV)
    y = outbuf[..., 32:128]
    Fn.conv_forward(x, spec, pk.pack, p.data, y)
    ref = cpu_ref_conv(x.contiguous(), spec, bf(p.data))
    assert rel_err(y, ref) < 1e-2
    assert outbuf[..., :32].abs().max().item() == 0 and outbuf[..., 128:].abs().max().item() == 0


@pytest.mark.parametrize("case", CONV_CASES[:-1], ids=lambda c: f"{c[0]}x{c[1]}k{c[2]}{c[3]}s{c[4]}")
@pytest.mark.parametrize("accumulate", [False, True])
def test_conv_dgrad(case, accumulate):
    cin, cout, kh, kw, s, pads, H = case
    if cin % 8:
        pytest.skip("stem has no data gradient")
    torch.manual_seed(3)
    spec, p, pk = make_conv(cin, cout, kh, kw, s, s, pads)
    N = 2
    P, Q = spec.out_hw(H, H)
    dz = bf(torch.randn(N, P, Q, cout, device=DEV))
    base = bf(torch.randn(N, H, H, cin, device=DEV))
    # not accumulating: every pixel written (a strided 1x1 zeroes its stride cells' gaps itself)
    dx = base.clone() if accumulate else torch.full_like(base, float("nan"))
    Fn.conv_dgrad(dz, spec, pk.tr, p.data, dx, accumulate)
    ref = torch.empty(N, H, H, cin)
    Fn.conv_dgrad(dz.float().cpu(), spec, None, bf(p.data).float().cpu(), ref, False)
    if accumulate:
        ref = ref + base.float().cpu()
    assert rel_err(dx, ref) < 1e-2


@pytest.mark.parametrize("case", [CONV_CASES[1], CONV_CASES[2], CONV_CASES[3], CONV_CASES[6]],
                         ids=["1x1", "3x3", "1x1s2", "cin80"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("cfg", [2, 4, 5, 7, 12, 13, 14, 16])
def test_conv_dgrad_fused_bn_backward(case, mode, accumulate, cfg):
    """data-grad GEMM with the consuming BN layer's ReLU gating and backward sums fused into
    its epilogue (ConvParams::bnb_*), vs the CPU gating + fp32 reductions."""
    cin, cout, kh, kw, s, pads, H = case
    torch.manual_seed(21)
    spec, p, pk = make_conv(cin, cout, kh, kw, s, s, pads)
    N = 2
    P, Q = spec.out_hw(H, H)
    dz = bf(torch.randn(N, P, Q, cout, device=DEV))
    base = bf(torch.randn(N, H, H, cin, device=DEV))
    z = bf(torch.randn(N, H, H, cin, device=DEV) * 1.5 + 0.2)
    yact = bf(torch.relu(torch.randn(N, H, H, cin, device=DEV)))
    mean = torch.randn(cin, device=DEV) * 0.1 + 0.2
    invstd = torch.rand(cin, device=DEV) + 0.5
    gamma = torch.rand(cin, device=DEV) + 0.5
    beta = torch.randn(cin, device=DEV) * 0.2
    saved = Fn.BNSaved(mean, invstd)
    R = 8
    acc = torch.zeros(R * 2 * cin, device=DEV)
    strided_1x1 = s > 1 and kh == 1 and kw == 1
    if strided_1x1:
        # precondition of a fused strided-1x1 (remap) dgrad: the pixels it does not visit are 0
        keep = torch.zeros(1, H, H, 1, dtype=torch.bool, device=DEV)
        keep[:, ::s, ::s] = True
        base = base * keep
    dx = base.clone() if accumulate else torch.full_like(base, float("nan"))
    bnb = Fn.BNBwdFuse(z, yact, saved, gamma, beta, mode, acc, R)
    Fn.conv_dgrad(dz, spec, pk.tr, p.data, dx, accumulate, cfg=cfg, bnb=bnb)
    ref = torch.empty(N, H, H, cin)
    Fn.conv_dgrad(dz.float().cpu(), spec, None, bf(p.data).float().cpu(), ref, False)
    if accumulate:
        ref = ref + base.float().cpu()
    zc = z.float().cpu()
    cpu_bnb = Fn.BNBwdFuse(zc, yact.float().cpu(), Fn.BNSaved(mean.cpu(), invstd.cpu()), gamma.cpu(), beta.cpu(),
                           mode, None, R)
    g = cpu_bnb.gate_cpu(ref.clone())
    assert rel_err(dx, g) < 1e-2
    xhat = (zc - mean.cpu()) * invstd.cpu()
    sums = acc.view(R, 2, cin).sum(0).cpu()
    assert rel_err(sums[0], g.reshape(-1, cin).sum(0)) < 2e-2
    assert rel_err(sums[1], (g * xhat).reshape(-1, cin).sum(0)) < 2e-2


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}x{c[1]}k{c[2]}{c[3]}s{c[4]}")
def test_conv_wgrad(case):
    cin, cout, kh, kw, s, pads, H = case
    torch.manual_seed(4)
    cpad = cin if cin % 8 == 0 else 8
    spec, p, pk = make_conv(cin, cout, kh, kw, s, s, pads, cin_pad=cpad)
    N = 4
    P, Q = spec.out_hw(H, H)
    x = bf(torch.randn(N, H, H, cpad, device=DEV))
    dz = bf(torch.randn(N, P, Q, cout, device=DEV))
    dw = torch.zeros(cout, kh, kw, cpad, dtype=torch.float32, device=DEV)
    Fn.conv_wgrad(dz, x, spec, dw.view(cout, -1))
    ref = torch.zeros(cout, kh, kw, cpad)
    Fn.conv_wgrad(dz.float().cpu(), x.float().cpu(), spec, ref)
    assert rel_err(dw, ref) < 1e-2


@pytest.mark.parametrize("cfg", list(range(15)))
def test_conv_wgrad_all_configs(cfg):
    """Every weight-grad tile config (register-staged 0-2 and 13-14, LDS-DMA ring 3-9,
    intra-workgroup k-split 10-12) with split-K on
    1x1 / 3x3 / strided / odd-channel geometries (partial tiles in Nout, K and pixels)."""
    torch.manual_seed(6)
    for cin, cout, k, s, pads, H, splits in [(64, 256, 1, 1, (0, 0, 0, 0), 14, 3),
                                             (128, 128, 3, 2, (1, 1, 1, 1), 15, 2),
                                             (80, 192, 3, 1, (0, 0, 0, 0), 11, 1),
                                             (256, 72, 1, 1, (0, 0, 0, 0), 9, 4)]:
        spec, p, pk = make_conv(cin, cout, k, k, s, s, pads)
        N = 3
        P, Q = spec.out_hw(H, H)
        x = bf(torch.randn(N, H, H, cin, device=DEV))
        dz = bf(torch.randn(N, P, Q, cout, device=DEV))
        dw = torch.zeros(cout, spec.K, dtype=torch.float32, device=DEV)
        Fn.conv_wgrad(dz, x, spec, dw, cfg=(cfg, splits))
        ref = torch.zeros(cout, k, k, cin)
        Fn.conv_wgrad(dz.float().cpu(), x.float().cpu(), spec, ref)
        assert rel_err(dw, ref.view(cout, -1)) < 1e-2, (cfg, cin, cout, k)


@pytest.mark.parametrize("cfg", [0, 1, 2, 10, 11, 12, 13, 14])
def test_conv_wgrad_row_incremental_loaders(cfg):
    """The register-staged row-incremental loaders (mixed-radix pixel stepping; per-lane rows,
    and rows shared through ds_bpermute when a column tile lies in one filter tap) against the
    fp32 CPU reference, one split (no atomics: two runs are bitwise equal). Geometries cover a
    k-step spanning images (7x7 output: dn > 0), output-row carries, stride 2 with padding,
    partial Nout / pixel tiles."""
    torch.manual_seed(8)
    for cin, cout, k, s, pads, H, N in [(64, 64, 3, 1, (1, 1, 1, 1), 14, 3),
                                        (128, 72, 3, 1, (1, 1, 1, 1), 7, 5),
                                        (96, 128, 3, 2, (1, 1, 1, 1), 15, 2),
                                        (256, 192, 1, 1, (0, 0, 0, 0), 9, 4),
                                        (64, 256, 1, 2, (0, 0, 0, 0), 13, 3)]:
        spec, p, pk = make_conv(cin, cout, k, k, s, s, pads)
        P, Q = spec.out_hw(H, H)
        x = bf(torch.randn(N, H, H, cin, device=DEV))
        dz = bf(torch.randn(N, P, Q, cout, device=DEV))
        out = []
        for _ in range(2):
            dw = torch.zeros(cout, spec.K, dtype=torch.float32, device=DEV)
            Fn.conv_wgrad(dz, x, spec, dw, cfg=(cfg, 1))
            out.append(dw)
        assert torch.equal(out[0], out[1]), (cfg, cin, cout, k, s)
        ref = torch.zeros(cout, k, k, cin)
        Fn.conv_wgrad(dz.float().cpu(), x.float().cpu(), spec, ref)
        assert rel_err(out[0], ref.view(cout, -1)) < 1e-2, (cfg, cin, cout, k)


def test_conv_wgrad_split_k_large_reduction():
    torch.manual_seed(5)
    spec, p, pk = make_conv(64, 64, 3, 3, 1, 1, (1, 1, 1, 1))
    x = bf(torch.randn(8, 56, 56, 64, device=DEV))
    dz = bf(torch.randn(8, 56, 56, 64, device=DEV))
    dw = torch.zeros(64, 3 * 3 * 64, dtype=torch.float32, device=DEV)
    Fn.conv_wgrad(dz, x, spec, dw)
    ref = torch.zeros(64, 3, 3, 64)
    Fn.conv_wgrad(dz.float().cpu(), x.float().cpu(), spec, ref)
    assert rel_err(dw, ref.view(64, -1)) < 1e-2


@pytest.mark.parametrize("C", [64, 256, 80, 2048])
@pytest.mark.parametrize("relu,residual", [(True, False), (True, True), (False, False)])
def test_bn_fwd_bwd(C, relu, residual):
    """The path BNReLU trains with -- bn_stats_acc into R = 8 zeroed replicas, bn_forward_acc, then
    bn_backward_acc through a zeroed backward accumulator -- against the PyTorch reference on the CPU.
    Both sides read the same bf16-rounded z; the GPU's moments are 196-term fp32 sums (atomics over
    the replicas) of a single-pass variance without cancellation (mean 1, std 3): an fp32 emulation of
    those sums on the CPU (same seed, any summation order) is within 6e-8 of the reference mean and
    running mean and 2.1e-7 of its invstd and running variance (relative), far inside the 1e-4 bounds
    (profiles/bn_one_path.txt)."""
    torch.manual_seed(6)
    N, H, R = 4, 7, 8
    z = bf(torch.randn(N, H, H, C, device=DEV) * 3 + 1)
    gamma = torch.rand(C, device=DEV) + 0.5
    beta = torch.randn(C, device=DEV) * 0.1
    res = bf(torch.randn(N, H, H, C, device=DEV)) if residual else None
    rm = torch.zeros(C, device=DEV)
    rv = torch.ones(C, device=DEV)
    y = torch.empty_like(z)
    acc_f = torch.zeros(R, 2, C, device=DEV)
    Fn.bn_stats_acc(z, acc_f, R)
    saved = Fn.bn_forward_acc(z, gamma, beta, rm, rv, 0.9, 1e-5, y, relu, acc_f, R, torch.empty(C, device=DEV),
                              torch.empty(C, device=DEV), residual=res)
    zc, gc, bc = z.float().cpu(), gamma.cpu(), beta.cpu()
    rmc, rvc = torch.zeros(C), torch.ones(C)
    yc = torch.empty(N, H, H, C)
    sc = Fn.bn_forward(zc, gc, bc, rmc, rvc, 0.9, 1e-5, yc, relu, residual=None if res is None else res.float().cpu())
    assert rel_err(y, yc) < 1e-2
    assert rel_err(saved.mean, sc.mean) < 1e-4 and rel_err(saved.invstd, sc.invstd) < 1e-4
    assert rel_err(rm, rmc) < 1e-4 and rel_err(rv, rvc) < 1e-4
    dy = bf(torch.randn(N, H, H, C, device=DEV))
    mode = (1 if residual else 2) if relu else 0
    dz = torch.empty_like(z)
    gres = torch.empty_like(z)
    dg = torch.empty(C, device=DEV)
    db = torch.empty(C, device=DEV)
    Fn.bn_backward_acc(dy, y, z, saved, gamma, beta, mode, dg, db, dz, torch.zeros(R, 2, C, device=DEV), R, gres)
    dzc, gresc, dgc, dbc = torch.empty(N, H, H, C), torch.empty(N, H, H, C), torch.empty(C), torch.empty(C)
    Fn.bn_backward(dy.float().cpu(), y.float().cpu(), zc, sc, gc, bc, mode, dgc, dbc, dzc, gresc)
    assert rel_err(db, dbc) < 1e-2 and rel_err(dg, dgc) < 1e-2
    assert rel_err(dz, dzc) < 2e-2
    assert rel_err(gres, gresc) < 1e-2


def test_bn_reference_entry_points_reject_native_tensors():
    """Fn.bn_forward / Fn.bn_backward are the PyTorch reference path: a native tensor (one the HIP
    kernels own) must go through the _acc forms, and handing it to them is an error, not a fall-back."""
    C = 64
    z = torch.zeros(2, 3, 3, C, dtype=torch.bfloat16, device=DEV)
    assert Fn.native(z)
    v = torch.ones(C, device=DEV)
    with pytest.raises(AssertionError, match="bn_stats_acc.*bn_forward_acc"):
        Fn.bn_forward(z, v, v, v.clone(), v.clone(), 0.9, 1e-5, torch.empty_like(z), True)
    with pytest.raises(AssertionError, match="bn_backward_acc"):
        Fn.bn_backward(z, z, z, Fn.BNSaved(v, v), v, v, 0, v.clone(), v.clone(), torch.empty_like(z))


@pytest.mark.parametrize("kind", ["max3s2same", "avg3s1same", "max3s2valid", "avg8valid", "max3s1same",
                                  "avg3s1valid", "max3s2same_even", "max3s2valid_even"])
def test_pool_fwd_bwd(kind):
    from azure_hc_intel_tf_amd.nn.layers import Pool

    torch.manual_seed(7)
    N, H, C = 2, 17, 64
    if kind.endswith("_even"):  # even H: the 2x2-block argmax gather (maxpool_bwd_amax_s2_kernel)
        H = 16
        layer = Pool("p", (H, H, C), 3, 3, 2, 2, "SAME" if "same" in kind else "VALID", is_max=True)
    elif kind == "max3s2same":
        layer = Pool("p", (H, H, C), 3, 3, 2, 2, "SAME", is_max=True)
    elif kind == "avg3s1same":
        layer = Pool("p", (H, H, C), 3, 3, 1, 1, "SAME", is_max=False)
    elif kind == "max3s2valid":
        layer = Pool("p", (H, H, C), 3, 3, 2, 2, "VALID", is_max=True)
    elif kind == "max3s1same":  # Inception's last module (3x3/1 kernels, argmax over 3x3 windows)
        layer = Pool("p", (H, H, C), 3, 3, 1, 1, "SAME", is_max=True)
    elif kind == "avg3s1valid":
        layer = Pool("p", (H, H, C), 3, 3, 1, 1, "VALID", is_max=False)
    else:
        H = 8
        layer = Pool("p", (H, H, C), 8, 8, 1, 1, "VALID", is_max=False)
    x = bf(torch.randn(N, H, H, C, device=DEV))
    yc = layer.forward(x.float().cpu())
    dy = bf(torch.randn(yc.shape, device=DEV))
    dxc = layer.backward(dy.float().cpu())
    y = layer.forward(x)
    assert rel_err(y, yc) < 1e-2
    dx = layer.backward(dy)
    assert rel_err(dx, dxc) < 1e-2
    if layer.is_max:  # the recompute path (no argmax buffer) must agree with the argmax path
        dx2 = torch.empty_like(dx)
        Fn.pool_backward(dy, x, y, dx2, *layer.k, *layer.s, layer.pads, True, False, False, argmax=None)
        assert torch.equal(dx, dx2)


def test_gap_and_softmax_and_colsum():
    torch.manual_seed(8)
    x = bf(torch.randn(4, 7, 7, 2048, device=DEV))
    y = torch.empty(4, 2048, dtype=torch.bfloat16, device=DEV)
    Fn.gap_forward(x, y)
    assert rel_err(y, x.float().cpu().mean(dim=(1, 2))) < 1e-2
    dx = torch.empty_like(x)
    Fn.gap_backward(y, dx)
    assert rel_err(dx, (y.float().cpu() / 49).view(4, 1, 1, 2048).expand(4, 7, 7, 2048)) < 1e-2
    B, ncls, ldl = 8, 1001, 1008
    logits = torch.randn(B, ldl, device=DEV) * 3
    labels = torch.randint(0, ncls, (B,), device=DEV)
    rl = torch.empty(B, device=DEV)
    dl = torch.empty(B, ldl, dtype=torch.bfloat16, device=DEV)
    Fn.softmax_xent(logits, labels, ncls, rl, dl, 1.0 / B)
    rlc, dlc = torch.empty(B), torch.empty(B, ldl)
    Fn.softmax_xent(logits.cpu(), labels.cpu(), ncls, rlc, dlc, 1.0 / B)
    assert rel_err(rl, rlc) < 1e-4
    assert rel_err(dl, dlc) < 1e-2
    assert dl[:, ncls:].abs().max().item() == 0
    cs = torch.empty(ncls, device=DEV)
    Fn.colsum(dl, B, ncls, cs)
    assert rel_err(cs, dl.float().cpu()[:, :ncls].sum(0)) < 1e-3


@pytest.mark.parametrize("M,N,f32", [(200_003, 64, False), (1_000, 1001, False), (5_000, 24, True), (3, 256, False)])
def test_colsum_large_reductions(M, N, f32):
    """bias gradients: the parallel column sum over up to millions of rows (row-strided
    vectors, LDS partials, one atomic per column and block)."""
    torch.manual_seed(13)
    ldg = (N + 7) // 8 * 8
    g = torch.randn(M, ldg, device=DEV)
    g = g if f32 else bf(g)
    out = torch.full((N,), 123.0, device=DEV)  # overwritten, not accumulated
    Fn.colsum(g, M, N, out)
    ref = g.float().cpu()[:, :N].double().sum(0)
    assert rel_err(out, ref.float()) < 1e-4


def test_sgd_momentum_flat():
    torch.manual_seed(9)
    n, nd = 100_003, 60_000
    w = torch.randn(n, device=DEV)
    m = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    hyper = torch.tensor([0.1, 0.9, 4e-5, 0.5], device=DEV)
    l2 = torch.zeros(1, device=DEV)
    wc, mc, gc, l2c = w.cpu(), m.cpu(), g.cpu(), torch.zeros(1)
    Fn.sgd_momentum(w, m, g, nd, hyper, l2)
    Fn.sgd_momentum(wc, mc, gc, nd, hyper.cpu(), l2c)
    assert rel_err(w, wc) < 1e-6 and rel_err(m, mc) < 1e-6
    assert abs(l2.item() - l2c.item()) / l2c.item() < 1e-4


def test_sgd_l2_partials_deterministic_and_summed_by_loss_total():
    """The trainer's form: per-block w^2 partials (one slot per optimizer block, every slot written,
    the slots past the grid cleared) summed in a fixed order by loss_total -- bitwise equal on
    repeats (no atomics), equal to the fp64 sum; a skipped (non-finite) step reports l2 = 0."""
    torch.manual_seed(4)
    n, nd = 1_000_003, 700_000
    hyper = torch.tensor([0.0, 0.9, 4e-5, 1.0, 0.0], device=DEV)  # lr 0: w unchanged between repeats
    w, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    row = torch.rand(16, device=DEV)
    outs = []
    for rep in range(3):
        m = torch.zeros(n, device=DEV)
        l2 = torch.full((4096,), float("nan"), device=DEV)  # stale garbage: must all be overwritten
        Fn.sgd_momentum(w, m, g, nd, hyper, l2)
        out = torch.empty(1, device=DEV)
        Fn.loss_total(row, 16, l2, 0.5, out)
        outs.append(out.item())
    assert outs[0] == outs[1] == outs[2]
    ref = row.double().mean() + 0.5 * (w[:nd].double() ** 2).sum()
    assert abs(outs[0] - ref.item()) <= 2e-6 * abs(ref.item())
    hyper[4] = 1.0  # found_inf: the update is skipped, the l2 term reads 0
    l2 = torch.full((4096,), 7.0, device=DEV)
    Fn.sgd_momentum(w, torch.zeros(n, device=DEV), g, nd, hyper, l2)
    assert float(l2.abs().sum()) == 0.0


@pytest.mark.parametrize("cin,cout,k", [(16, 24, 3), (136, 200, 3), (64, 128, 1), (256, 1001, 1), (8, 64, 7)])
def test_weight_pack_transposed_flip(cin, cout, k):
    """Vector copy + LDS-tiled transpose of the weight pack kernel (partial and full 64x64
    tiles, odd Nout) against a torch reference."""
    torch.manual_seed(10)
    spec, p, pk = make_conv(cin, cout, k, k, 1, 1, (k // 2,) * 4)
    w = p.data.cpu()
    packed = pk.pack.view(cout, spec.Kpad).float().cpu()
    assert torch.allclose(packed[:, :spec.K], bf(w).float().reshape(cout, -1))
    assert spec.K == spec.Kpad or packed[:, spec.K:].abs().max() == 0
    tr = pk.tr.view(cin, spec.Kpad_t).float().cpu()
    # tr[c][(r'*S+s')*Cout + k] = W[k][R-1-r'][S-1-s'][c]
    ref = bf(w).float().flip(1).flip(2).permute(3, 1, 2, 0).reshape(cin, -1)
    assert torch.allclose(tr[:, :spec.Kt], ref)
    assert spec.Kt == spec.Kpad_t or tr[:, spec.Kt:].abs().max() == 0


def test_synthetic_data_stats():
    img = torch.empty(16, 64, 64, 8, dtype=torch.bfloat16, device=DEV)
    _ext.ops().synth_images(img, 3, 8, 127.0, 60.0, 7)
    f = img.float()[..., :3]
    assert abs(f.mean().item() - 127.0) < 2.0
    assert 45 < f.std().item() < 60  # truncated at 2 sigma: sd ~ 0.88 * 60
    assert f.min().item() >= 127 - 121 and f.max().item() <= 127 + 121
    assert img[..., 3:].abs().max().item() == 0
    lab = torch.empty(4096, dtype=torch.int64, device=DEV)
    _ext.ops().synth_labels(lab, 1000, 3)
    assert lab.min().item() >= 0 and lab.max().item() < 1000 and lab.unique().numel() > 900


@pytest.mark.parametrize("C", [64, 256, 2048, 80, 48])
@pytest.mark.parametrize("relu,residual", [(True, False), (True, True), (False, False)])
def test_bn_finalize_free_path(C, relu, residual):
    """conv-epilogue atomics -> bn_apply_acc (stats finalized in-kernel) and the bwd reduce /
    apply pair with replica accumulators, vs the fp32 CPU reference."""
    torch.manual_seed(13)
    spec, p, pk = make_conv(64, C, 3, 3, 1, 1, (1, 1, 1, 1))
    N, H = 4, 9
    x = bf(torch.randn(N, H, H, 64, device=DEV))
    z = torch.empty(N, H, H, C, dtype=torch.bfloat16, device=DEV)
    R = 8
    acc_f = torch.zeros(R * 2 * C, device=DEV)
    Fn.conv_forward(x, spec, pk.pack, p.data, z, stats=acc_f, stats_R=R, cfg=2)
    gamma = torch.rand(C, device=DEV) + 0.5
    beta = torch.randn(C, device=DEV) * 0.1
    res = bf(torch.randn(N, H, H, C, device=DEV)) if residual else None
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    y = torch.empty_like(z)
    saved = Fn.bn_forward_acc(z, gamma, beta, rm, rv, 0.9, 1e-5, y, relu, acc_f, R, mean, invstd, residual=res)
    zc = z.float().cpu()
    yc = torch.empty(N, H, H, C)
    rmc, rvc = torch.zeros(C), torch.ones(C)
    sc = Fn.bn_forward(zc, gamma.cpu(), beta.cpu(), rmc, rvc, 0.9, 1e-5, yc, relu,
                       residual=None if res is None else res.float().cpu())
    assert rel_err(y, yc) < 1e-2
    # the kernel's statistics come from the fp32 accumulators, the reference's from the
    # bf16-rounded z: the mean differs by O(bf16 eps * std / sqrt(n)), so measure it in stds
    mean_err = ((saved.mean.cpu() - sc.mean).abs() * sc.invstd).max().item()
    assert mean_err < 2e-3 and rel_err(saved.invstd, sc.invstd) < 1e-3
    assert ((rm.cpu() - rmc).abs() * sc.invstd).max().item() < 2e-3 and rel_err(rv, rvc) < 1e-3
    dy = bf(torch.randn(N, H, H, C, device=DEV))
    mode = (1 if residual else 2) if relu else 0
    dz, gres = torch.empty_like(z), torch.empty_like(z)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    acc_b = torch.zeros(R * 2 * C, device=DEV)
    Fn.bn_backward_acc(dy, y, z, saved, gamma, beta, mode, dg, db, dz, acc_b, R, gres)
    dzc, gresc, dgc, dbc = torch.empty(N, H, H, C), torch.empty(N, H, H, C), torch.empty(C), torch.empty(C)
    # the reference uses the kernel's own batch moments so both sides gate with the same ReLU mask
    gsv = Fn.BNSaved(saved.mean.cpu(), saved.invstd.cpu())
    Fn.bn_backward(dy.float().cpu(), y.float().cpu(), zc, gsv, gamma.cpu(), beta.cpu(), mode, dgc, dbc, dzc, gresc)
    assert rel_err(db, dbc) < 2e-2 and rel_err(dg, dgc) < 2e-2
    assert rel_err(dz, dzc) < 3e-2 and rel_err(gres, gresc) < 1e-2


def test_loss_scale_ops_gpu():
    """device-side loss scaling: scaled dlogits, Inf/NaN detection, skipped update, scale step"""
    torch.manual_seed(31)
    B, ncls, ldl = 8, 1001, 1008
    logits = torch.randn(B, ldl, device=DEV)
    labels = torch.randint(0, ncls, (B,), device=DEV)
    rl, rl2 = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    d1 = torch.empty(B, ldl, dtype=torch.bfloat16, device=DEV)
    d2 = torch.empty_like(d1)
    S = torch.tensor([64.0], device=DEV)
    Fn.softmax_xent(logits, labels, ncls, rl, d1, 1.0 / B)
    Fn.softmax_xent(logits, labels, ncls, rl2, d2, 1.0 / B, S)
    assert torch.allclose(d2.float(), d1.float() * 64, rtol=1e-2, atol=1e-4) and torch.equal(rl, rl2)
    h = torch.tensor([0.1, 0.9, 0.0, 1.0 / 1024, 0.0, 1024.0, 0.0, 1000.0], device=DEV)
    g = torch.ones(100_003, device=DEV)
    w, mom = torch.ones_like(g), torch.zeros_like(g)
    Fn.nonfinite(g, h[4:5])
    assert float(h[4]) == 0.0
    g[77_777] = float("nan")
    Fn.nonfinite(g, h[4:5])
    assert float(h[4]) == 1.0
    Fn.sgd_momentum(w, mom, g, 0, h)
    assert torch.equal(w, torch.ones_like(w))
    Fn.loss_scale_update(h, 1, True)
    assert float(h[5]) == 512.0 and abs(float(h[3]) - 1 / 512) < 1e-9


def test_fused_stem_bn_relu_maxpool_matches_unfused():
    """ResNet stem: conv -> [BN + ReLU + max pool in one kernel] against conv -> BN+ReLU -> pool,
    forward values, running statistics, and the backward through the argmax + BN."""
    from azure_hc_intel_tf_amd.nn.layers import ConvBN, Pool
    from azure_hc_intel_tf_amd.nn.params import ParamStore

    torch.manual_seed(21)
    res = []
    for fused in (False, True):
        ps = ParamStore(seed=3)
        stem = ConvBN(ps, "conv0", (64, 64, 8), 64, 7, 7, 2, 2, "SAME_RESNET", relu=True, need_dx=False,
                      logical_cin=3)
        pool = Pool("mpool0", stem.out_shape, 3, 3, 2, 2, "SAME", is_max=True)
        ps.finalize(DEV)
        ps.repack()
        ps.zero_stats()
        ps.zero_grad()
        g = torch.Generator().manual_seed(5)
        x = bf(torch.randn(4, 64, 64, 8, generator=g).to(DEV))
        x[..., 3:] = 0
        y = stem.forward_maxpool(x, pool) if fused else pool.forward(stem.forward(x))
        dy = bf(torch.randn(y.shape, generator=g).to(DEV))
        stem.backward(pool.backward(dy))
        torch.cuda.synchronize()
        res.append((y.float().cpu(), stem.rmean.data.cpu().clone(), stem.w.grad.float().cpu().clone(),
                    stem.gamma.grad.cpu().clone()))
    (y0, rm0, gw0, gg0), (y1, rm1, gw1, gg1) = res
    assert torch.equal(y0, y1)
    assert torch.allclose(rm0, rm1, atol=1e-6)
    # the fused kernel picks the window max in fp32, the unfused pool among bf16-rounded values:
    # near-ties (common with 8-bit mantissas) route a few gradients to a neighbouring pixel
    assert rel_err(gw1, gw0) < 5e-2 and rel_err(gg1, gg0) < 5e-2
