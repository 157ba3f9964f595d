"""The plane (fp32, bf16x6) 3x3 / stride 1 kernels with the input patch resident in LDS
(csrc/kernels/conv_p3_patch.h, the cfgs of gemm_cfg.h HCB_P3PATCH_CFGS, numbered from 64): forward with fused BN
statistics, data gradient without / with the fused BN-backward epilogue and with accumulate, against
fp64 CPU convolutions at the plane GEMMs' bound (3e-6 relative, tests/test_fp32_native_gpu.py); the
fallback to the row's per-tile cfg; bitwise reproducibility; and the host-side patch-size / LDS-fit
function (CPU)."""
import functools
import os

import pytest
import torch

from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.nn.params import ParamStore
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.ops.functional import ConvSpec

DEV = "cuda"
CFGS = sorted(Fn._P3_PATCH_TILES)
# (N, H, W, cin, cout): one slab, the patch spans an image boundary, M = 98 has a row tail; two slabs
# (the patch double buffer), a column tail on cout, more than one M tile; three slabs (a buffer reused
# with odd parity) on a non-square image
SHAPES = [(2, 7, 7, 32, 64), (3, 14, 14, 64, 96), (1, 6, 10, 96, 32)]
IDS = [f"n{s[0]}h{s[1]}w{s[2]}c{s[3]}k{s[4]}" for s in SHAPES]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.fixture
def fp32_mode():
    set_gpu_compute_dtype(torch.float32)
    Fn.set_f32_native(True)
    yield
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def _conv(cin, cout, k=3, s=1, pad=1):
    spec = ConvSpec(cin=cin, cin_pad=cin, cout=cout, kh=k, kw=k, sh=s, sw=s, pt=pad, pl=pad, pb=pad, pr=pad)
    ps = ParamStore(seed=5)
    p = ps.add("w", (cout, k, k, cin), True, ps.variance_scaling(k * k * cin))
    pk = ps.add_pack(p, cout, k, k, cin, spec.Kpad, spec.Kpad_t, want_tr=True)
    ps.finalize(DEV, dtype_pack=torch.bfloat16, pack_lo=True)
    ps.repack()
    return spec, p, pk


@functools.lru_cache(maxsize=None)
def _problem(shape, stride=1):
    """The operands of one shape and their fp64 references, computed once."""
    N, H, W, cin, cout = shape
    spec, p, pk = _conv(cin, cout, s=stride)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, cin, generator=g)
    P, Q = spec.out_hw(H, W)
    dz = torch.randn(N, P, Q, cout, generator=g)
    wd = p.data.double().cpu().permute(0, 3, 1, 2)
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(xr, wd, stride=stride, padding=1)
    y.backward(dz.double().permute(0, 3, 1, 2))
    return dict(spec=spec, p=p, pk=pk, x=x.to(DEV), dz=dz.to(DEV), y=y.detach().permute(0, 2, 3, 1),
                dx=xr.grad.permute(0, 2, 3, 1), P=P, Q=Q)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("cfg", CFGS)
def test_forward_and_fused_statistics_match_fp64(fp32_mode, cfg, shape):
    N, H, W, cin, cout = shape
    q = _problem(shape)
    assert Fn.p3_patch_fits(cfg, H, W)
    y = torch.full((N, H, W, cout), float("nan"), dtype=torch.float32, device=DEV)
    R = 8
    st = torch.zeros(R, 2, cout, device=DEV)
    Fn.conv_forward(q["x"], q["spec"], q["pk"].pack, q["p"].data, y, stats=st, cfg=cfg, stats_R=R)
    assert rel_err(y, q["y"]) < 3e-6
    s = st.double().sum(0).cpu()
    v = q["y"].reshape(-1, cout)
    assert rel_err(s[0], v.sum(0)) < 1e-5 and rel_err(s[1], (v * v).sum(0)) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("cfg", CFGS)
def test_data_gradient_plain_fused_and_accumulate_match_fp64(fp32_mode, cfg, shape):
    N, H, W, cin, cout = shape
    q = _problem(shape)
    spec, p, pk, ref = q["spec"], q["p"], q["pk"], q["dx"]
    dx = torch.full((N, H, W, cin), float("nan"), dtype=torch.float32, device=DEV)
    Fn.conv_dgrad(q["dz"], spec, pk.tr, p.data, dx, False, cfg=cfg)
    assert rel_err(dx, ref) < 3e-6
    g0 = torch.Generator().manual_seed(9)
    base = torch.randn(N, H, W, cin, generator=g0).to(DEV)
    dx = base.clone()
    Fn.conv_dgrad(q["dz"], spec, pk.tr, p.data, dx, True, cfg=cfg)
    assert rel_err(dx, ref + base.double().cpu()) < 3e-6
    # the fused BN-backward epilogue: ReLU gate from the y hi plane (1) and from z (2), none (0)
    z = (torch.randn(N, H, W, cin, generator=g0) * 1.5 + 0.2).to(DEV)
    mean, invstd = (torch.randn(cin, generator=g0) * 0.1).to(DEV), (torch.rand(cin, generator=g0) + 0.5).to(DEV)
    gamma, beta = (torch.rand(cin, generator=g0) + 0.5).to(DEV), (torch.randn(cin, generator=g0) * 0.1).to(DEV)
    yf = torch.relu(torch.randn(N, H, W, cin, generator=g0)).to(DEV)
    yp = Fn.to_planes(yf)
    dzp = Fn.to_planes(q["dz"])
    xh = ((z.double() - mean.double()) * invstd.double()).cpu()
    for mode, accumulate in ((0, False), (1, False), (2, False), (1, True), (2, True)):
        g = ref + (base.double().cpu() if accumulate else 0)
        if mode == 1:
            g = g * (yf.cpu() > 0).double()
        elif mode == 2:
            g = g * ((xh * gamma.double().cpu() + beta.double().cpu()) > 0).double()
        R = 8
        acc = torch.zeros(R, 2, cin, device=DEV)
        dx = base.clone() if accumulate else torch.full((N, H, W, cin), float("nan"), device=DEV)
        bnb = Fn.BNBwdFuse(z, yp, Fn.BNSaved(mean, invstd), gamma, beta, mode, acc, R)
        Fn.conv_dgrad(dzp, spec, pk.tr, p.data, dx, accumulate, cfg=(cfg, 1), bnb=bnb)
        assert rel_err(dx, g) < 3e-6, (mode, accumulate)
        a = acc.double().sum(0).cpu()
        assert rel_err(a[0], g.reshape(-1, cin).sum(0)) < 1e-5, (mode, accumulate)
        assert rel_err(a[1], (g.reshape(-1, cin) * xh.reshape(-1, cin)).sum(0)) < 1e-5, (mode, accumulate)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("case", ["stride2", "c48", "rowcap"])
def test_unserved_problem_runs_the_fallback(fp32_mode, cfg, case):
    """Stride 2, C % 32 != 0 and a patch over the LDS row cap run the row's per-tile cfg: the result is
    bitwise that of an explicit launch of it, and matches fp64."""
    shape, stride = {"stride2": ((2, 14, 14, 32, 64), 2), "c48": ((2, 7, 7, 48, 64), 1),
                     "rowcap": ((1, 3, 200, 32, 32), 1)}[case]
    N, H, W, cin, cout = shape
    if case == "rowcap":
        assert not Fn.p3_patch_fits(cfg, H, W)
    q = _problem(shape, stride)
    outs = []
    for c in (cfg, Fn._P3_PATCH_FB[cfg]):
        y = torch.full((N, q["P"], q["Q"], cout), float("nan"), dtype=torch.float32, device=DEV)
        Fn.conv_forward(q["x"], q["spec"], q["pk"].pack, q["p"].data, y, cfg=c)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    assert rel_err(outs[0], q["y"]) < 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_deterministic_launches_are_bitwise_equal(fp32_mode, cfg):
    shape = SHAPES[1]
    N, H, W, cin, cout = shape
    q = _problem(shape)
    g0 = torch.Generator().manual_seed(4)
    z = torch.randn(N, H, W, cin, generator=g0).to(DEV)
    mean, invstd = torch.zeros(cin, device=DEV), torch.ones(cin, device=DEV)
    gamma, beta = torch.ones(cin, device=DEV), torch.zeros(cin, device=DEV)
    dzp = Fn.to_planes(q["dz"])
    Fn.set_deterministic(True)
    try:
        Rd = Fn.det_replicas(N * H * W)
        runs = []
        for _ in range(2):
            y = torch.empty(N, H, W, cout, dtype=torch.float32, device=DEV)
            st = torch.zeros(Rd, 2, cout, device=DEV)
            Fn.conv_forward(q["x"], q["spec"], q["pk"].pack, q["p"].data, y, stats=st, cfg=cfg, stats_R=Rd)
            a = torch.zeros(Rd, 2, cin, device=DEV)
            dx = torch.empty(N, H, W, cin, dtype=torch.float32, device=DEV)
            Fn.conv_dgrad(dzp, q["spec"], q["pk"].tr, q["p"].data, dx, False, cfg=(cfg, 1),
                          bnb=Fn.BNBwdFuse(z, None, Fn.BNSaved(mean, invstd), gamma, beta, 2, a, Rd))
            runs.append((y, st, a, dx))
    finally:
        Fn.set_deterministic(False)
    assert all(torch.equal(u, v) for u, v in zip(*runs))


# ---------------------------------------------------------------- host side (no GPU)
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "azure_hc_intel_tf_amd")


def _max_span(H, W, bm, N=3):
    """The largest padded span over every bm-pixel tile start, by enumeration."""
    lp = [(n * (H + 1) + p) * (W + 1) + q for n in range(N) for p in range(H) for q in range(W)]
    return max(lp[min(m + bm, len(lp)) - 1] - lp[m] for m in range(0, len(lp))) + 2 * (W + 1) + 3


def test_patch_rows_and_lds_fit_of_the_resnet_stages():
    """The four ResNet stage widths: the row bound covers the enumerated span and is tight to one
    16-row piece; the 128x128 tile fits stages 2-4 beside a 3-slot ring and not stage 1, where a
    128x64 tile (N = 64) would; the exported C++ function agrees with the planner's."""
    for W in (7, 14, 28, 56):
        rows = Fn.p3_patch_rows(W, W, 128)
        span = _max_span(W, W, 128, N=6)
        assert span <= rows < span + 32, (W, span, rows)
    assert [Fn.p3_patch_rows(W, W, 128) for W in (7, 14, 28, 56)] == [192, 192, 224, 304]
    for W in (7, 14, 28):
        assert all(Fn.p3_patch_fits(c, W, W) for c in Fn._P3_PATCH_TILES)
    assert not Fn.p3_patch_fits(64, 56, 56)
    # stage 1 with a 128x64 tile (BN = 64): 3 x 3 x 64 x 64 of ring + two 304-row buffers + sink + parameters
    assert 3 * 3 * 64 * 64 + 2 * 3 * Fn.p3_patch_rows(56, 56, 128) * 64 + 1024 + 64 * 16 <= 160 * 1024
    assert Fn.p3_patch_candidates(200704, 64, 576, 9, 56, 56) == []
    assert Fn.p3_patch_candidates(12544, 256, 2304, 9, 14, 14) == [(64, 1)]
    assert Fn.p3_patch_candidates(50176, 128, 1152, 1, 28, 28) == []
    path = os.path.join(PKG, "_hcb_kernels.so")
    if not os.path.exists(path):
        pytest.skip("_hcb_kernels.so not built (python __graft_entry__.py builds it)")
    torch.ops.load_library(path)
    for cfg, (bm, bn) in Fn._P3_PATCH_TILES.items():
        for H, W in ((7, 7), (14, 14), (28, 28), (56, 56), (6, 10), (3, 200)):
            for bnb in (False, True):
                lds, rows, cap = torch.ops.hcb.p3_patch_fit(cfg, H, W, bnb)
                assert rows == Fn.p3_patch_rows(H, W, bm)
                assert cap == 160 * 1024 and (lds <= cap) == Fn.p3_patch_fits(cfg, H, W, bnb)
    flat = list(torch.ops.hcb.gemm_cfg_table("p3_patch"))
    rows = [flat[i:i + 12] for i in range(0, len(flat), 12)]
    assert {r[0]: (r[2] * r[4], r[3] * r[5]) for r in rows} == Fn._P3_PATCH_TILES
    assert {r[0]: r[10] for r in rows} == Fn._P3_PATCH_FB and all(r[7] == Fn._P3_PATCH_NST for r in rows)
