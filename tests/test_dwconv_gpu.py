"""The depthwise 3x3 kernels (csrc/kernels/dwconv.hip) against fp64 PyTorch on the CPU, computed from
the exact inputs the kernels got.

Bounds. fp32: ||out - ref|| / ||ref|| < 3e-6, the bound and normalisation of the plane GEMMs
(tests/test_fp32_native_gpu.py). 16-bit (bf16 library, fp16 through hcb16): the inputs are rounded to
the type first; an output element may differ from the fp64 reference of the rounded inputs by one
rounding to nearest of the output, 2^-8 |ref| (bf16: 8 significant bits) or 2^-11 |ref| (fp16: 11),
plus the fp32 accumulation bound above per element, 3e-6 * ||ref|| / sqrt(numel). The weight gradient
is an fp32 tensor in every mode: the fp32 bound alone. Fused statistics: the bounds of the conv-epilogue
statistics tests (fp32 1e-5, tests/test_fp32_native_gpu.py; 16-bit 2e-2, tests/test_kernels_gpu.py).

Measured maxima on an MI355X: fp32 forward / data gradient / weight gradient <= 1.7e-7 relative (bound
3e-6), fused statistics <= 1.6e-7 (bound 1e-5); bf16 and fp16 excess over the one output rounding <=
1.7e-7 absolute where 3.4e-6 .. 5.0e-6 was allowed, weight gradient <= 1.7e-7 relative.
"""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"

# N, H, W, C, stride, (pt, pl), ld
CASES = [
    (2, 7, 7, 8, 1, (1, 1), 8),
    (2, 8, 8, 24, 2, (0, 0), 24),    # even size, SAME: bottom / right padding only
    (2, 7, 9, 24, 2, (1, 1), 24),    # odd sizes, non-square
    (1, 5, 5, 144, 1, (1, 1), 144),
    (2, 3, 3, 8, 1, (1, 1), 8),      # every output touches the halo
    (3, 14, 14, 40, 1, (1, 1), 64),  # a column window of a wider tensor
]
IDS = [f"n{c[0]}h{c[1]}w{c[2]}c{c[3]}s{c[4]}p{c[5][0]}{c[5][1]}ld{c[6]}" for c in CASES]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
EPS_OUT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


@pytest.fixture(params=["fp32", "bf16", "fp16"])
def mode(request):
    """Selects the kernel library (fp16: hcb16) and makes fp32 tensors native for the test."""
    name = request.param
    _ext.set_act("fp16" if name == "fp16" else "bf16")
    Fn.set_f32_native(name == "fp32")
    yield name
    _ext.set_act("bf16")
    Fn.set_f32_native(False)


def out_hw(H, W, s):
    return (H + s - 1) // s, (W + s - 1) // s  # 'SAME'


def windowed(shape, C, ld, dtype):
    """A NaN-filled [.., ld] buffer and its [.., :C] window."""
    buf = torch.full(shape[:-1] + (ld,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[..., :C]


def ref64(x, w, dz, s, pt, pl, P, Q):
    """(z, dx, dw) in fp64 on the CPU for NHWC x, [C,3,3] w, NHWC dz."""
    N, H, W, C = x.shape
    xr = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.double().cpu().reshape(C, 1, 3, 3).requires_grad_(True)
    pb, pr = max((P - 1) * s + 3 - H - pt, 0), max((Q - 1) * s + 3 - W - pl, 0)
    z = F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr, stride=s, groups=C)
    assert z.shape[2:] == (P, Q)
    z.backward(dz.double().cpu().permute(0, 3, 1, 2))
    return z.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad.reshape(C, 3, 3)


def check(name, got, ref, mode, out_rounded=True):
    got, ref = got.double().cpu(), ref.double()
    rms = float(ref.norm()) / ref.numel() ** 0.5
    rel = float((got - ref).norm() / (ref.norm() + 1e-300))
    eps = EPS_OUT[mode] if out_rounded else 0.0
    if eps == 0.0:
        print(f"{name} {mode}: rel {rel:.3e}")
        assert rel < 3e-6, (name, rel)
        return
    excess = float(((got - ref).abs() - eps * ref.abs()).max())
    print(f"{name} {mode}: rel {rel:.3e}, max excess over one rounding {excess:.3e} (allowed {3e-6 * rms:.3e})")
    assert excess <= 3e-6 * rms, (name, excess, 3e-6 * rms)


def make(case, mode, seed=0):
    N, H, W, C, s, (pt, pl), ld = case
    dt = DTYPES[mode]
    g = torch.Generator().manual_seed(seed)
    P, Q = out_hw(H, W, s)
    xb, x = windowed((N, H, W, C), C, ld, dt)
    x.copy_(torch.randn(N, H, W, C, generator=g).to(dt))
    dzb, dz = windowed((N, P, Q, C), C, ld, dt)
    dz.copy_(torch.randn(N, P, Q, C, generator=g).to(dt))
    w = (torch.randn(C, 3, 3, generator=g) * 0.5).to(DEV)
    return x, dz, w, P, Q, xb


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_forward_dgrad_wgrad(case, mode):
    N, H, W, C, s, (pt, pl), ld = case
    dt = DTYPES[mode]
    x, dz, w, P, Q, _ = make(case, mode)
    zr, dxr, dwr = ref64(x, w, dz, s, pt, pl, P, Q)
    # forward with fused statistics; output, workspace and accumulators start as NaN / exact zeros
    zb, z = windowed((N, P, Q, C), C, ld, dt)
    R = 8
    acc = torch.zeros(R, 2, C, device=DEV)
    shift = (torch.randn(C) * 0.1).to(DEV)
    Fn.dwconv_forward(x, w, z, s, pt, pl, stats=acc, stats_R=R, stats_shift=shift)
    check("fwd", z, zr, mode)
    if ld > C:
        assert bool(torch.isnan(zb[..., C:]).all()), "the forward wrote outside its channel window"
    d = zr.reshape(-1, C) - shift.double().cpu()
    st = acc.double().sum(0).cpu()
    tol = 1e-5 if mode == "fp32" else 2e-2
    for got, ref in ((st[0], d.sum(0)), (st[1], (d * d).sum(0))):
        rel = float((got - ref).norm() / ref.norm())
        print(f"stats {mode}: rel {rel:.3e}")
        assert rel < tol
    z2b, z2 = windowed((N, P, Q, C), C, ld, dt)
    Fn.dwconv_forward(x, w, z2, s, pt, pl)
    assert torch.equal(z2, z), "the statistics must not change the output"
    # data gradient, then accumulate = True on top of prior contents
    dxb, dx = windowed((N, H, W, C), C, ld, dt)
    Fn.dwconv_dgrad(dz, w, dx, s, pt, pl)
    check("dgrad", dx, dxr, mode)
    if ld > C:
        assert bool(torch.isnan(dxb[..., C:]).all()), "the data gradient wrote outside its channel window"
    prior = torch.randn(N, H, W, C).to(dt).to(DEV)
    _, dx2 = windowed((N, H, W, C), C, ld, dt)
    dx2.copy_(prior)
    Fn.dwconv_dgrad(dz, w, dx2, s, pt, pl, accumulate=True)
    check("dgrad+=", dx2, prior.double().cpu() + dxr, mode)
    # weight gradient: NaN workspace, NaN output, two launches bitwise equal
    ws = Fn.dwconv_wgrad_workspace(x.shape, dz.shape, DEV)
    runs = []
    for _ in range(2):
        ws.fill_(float("nan"))
        dw = torch.full((C, 3, 3), float("nan"), device=DEV)
        Fn.dwconv_wgrad(dz, x, dw, s, pt, pl, ws=ws)
        runs.append(dw)
    check("wgrad", runs[0], dwr, mode, out_rounded=False)
    assert torch.equal(runs[0], runs[1]), "the weight gradient must be bitwise reproducible"


def test_dwconv_wgrad_many_slabs(mode):
    """More pixels than one slab pass covers (several workgroups, several pixels per thread): the
    fold over the slabs, against fp64."""
    case = (4, 28, 28, 32, 1, (1, 1), 32)
    x, dz, w, P, Q, _ = make(case, mode, seed=3)
    _, _, dwr = ref64(x, w, dz, 1, 1, 1, P, Q)
    ws = Fn.dwconv_wgrad_workspace(x.shape, dz.shape, DEV)
    assert ws.shape[0] > 1
    ws.fill_(float("nan"))
    dw = torch.full((32, 3, 3), float("nan"), device=DEV)
    Fn.dwconv_wgrad(dz, x, dw, 1, 1, 1, ws=ws)
    check("wgrad slabs", dw, dwr, mode, out_rounded=False)


def test_dwconv_stats_deterministic_replicas(mode):
    """Deterministic mode: the grid is capped at R = det_replicas row blocks, so every replica slot
    receives one add -- bitwise reproducible sums, and both shifted moments right against fp64."""
    case = (3, 14, 14, 40, 1, (1, 1), 40)
    N, H, W, C = case[:4]
    x, _, w, P, Q, _ = make(case, mode, seed=5)
    R = Fn.det_replicas(N * P * Q)
    shift = (torch.randn(C, generator=torch.Generator().manual_seed(6)) * 0.1).to(DEV)
    Fn.set_deterministic(True)
    try:
        accs = []
        for _ in range(2):
            acc = torch.zeros(R, 2, C, device=DEV)
            z = torch.empty(N, P, Q, C, dtype=DTYPES[mode], device=DEV)
            Fn.dwconv_forward(x, w, z, 1, 1, 1, stats=acc, stats_R=R, stats_shift=shift)
            accs.append(acc)
    finally:
        Fn.set_deterministic(False)
    assert torch.equal(accs[0], accs[1])
    d = ref64(x, w, torch.zeros(N, P, Q, C), 1, 1, 1, P, Q)[0].reshape(-1, C) - shift.double().cpu()
    got = accs[0].double().sum(0).cpu()
    tol = 1e-5 if mode == "fp32" else 2e-2
    for g, r in ((got[0], d.sum(0)), (got[1], (d * d).sum(0))):
        rel = float((g - r).norm() / r.norm())
        print(f"det stats {mode}: rel {rel:.3e}")
        assert rel < tol


def test_dwconv_host_checks():
    _ext.set_act("bf16")
    ops = _ext.ops()
    bf = torch.bfloat16
    x = torch.zeros(1, 4, 4, 16, dtype=bf, device=DEV)
    z = torch.zeros(1, 4, 4, 16, dtype=bf, device=DEV)
    w = torch.zeros(16, 3, 3, device=DEV)
    g = [1, 4, 4, 16, 16, 4, 4, 16, 1, 1, 1, 1]
    ops.dwconv_fwd(x, w, z, g)  # the well-formed call passes
    g12 = [1, 4, 4, 12, 16, 4, 4, 16, 1, 1, 1, 1]
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.dwconv_fwd(x, torch.zeros(12, 3, 3, device=DEV), z, g12)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.dwconv_fwd(x, w, z.float(), g)
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.dwconv_dgrad(z, w, x.to(torch.float16), g, False)
    dw = torch.zeros(16, 3, 3, device=DEV)
    need = ops.dwconv_wgrad_blocks(g) * 9 * 16
    with pytest.raises(RuntimeError, match="workspace"):
        ops.dwconv_wgrad(z, x, torch.zeros(need - 1, device=DEV), dw, g)
    with pytest.raises(RuntimeError, match="addressable"):
        ops.dwconv_fwd(x, w, z, [2] + g[1:])  # a batch the tensors do not hold
    torch.cuda.synchronize()
