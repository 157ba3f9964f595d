"""The fused DenseNet dense-layer kernel (csrc/kernels/dense3x3.hip) through Fn.dense_conv3x3_forward against
the same formula in fp64 on the CPU: BN (batch statistics) -> ReLU -> conv 3x3 SAME into a 16-channel slot of
a wider buffer. Bounds are the project's: the fp32 path at the 3e-6 (statistics 1e-5) of
tests/test_fp32_native_gpu.py, the 16-bit paths at the 1e-2 (statistics 2e-2) of test_conv_fwd_and_stats in
tests/test_kernels_gpu.py; all are norm-relative, as there."""
import math

import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
R = 8
NOUT = 12
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TOL = {"bf16": (1e-2, 2e-2), "fp16": (1e-2, 2e-2), "fp32": (3e-6, 1e-5)}  # (output, statistics)
SHAPES = [
    (1, 4, 4, 8),       # a quarter-filled chunk (channel masking) with the masked weight rows; three idle waves
    (2, 8, 8, 16),      # one chunk, two half-image strips, half the waves without a tile
    (1, 9, 12, 48),     # partial last chunk of 32, H = 5 + 4 strip rows, a partial last tile, W != H
    (2, 32, 32, 208),   # the widest block-1 layer of densenet40_k12: many chunks, the double buffer wraps
]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.fixture(params=list(DTYPES))
def precision(request):
    dt = DTYPES[request.param]
    set_gpu_compute_dtype(dt)
    Fn.set_f32_native(dt == torch.float32)
    yield request.param
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_conv3x3_forward(precision, shape):
    N, H, W, C = shape
    dt = DTYPES[precision]
    M = N * H * W
    slot, ldb = C + 8, C + 40  # the slot at a non-zero offset inside a wider buffer
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g)
    x[..., 1] += 50.0                      # |mean| >> std
    x[..., 5] = 0.25 * x[..., 5] - 20.0
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[3] = beta[C - 2] = -8.0           # entirely negative after BN: all masked by the ReLU
    w = torch.randn(NOUT, 3, 3, C, generator=g) * math.sqrt(2.0 / 9 / NOUT)
    buf = torch.full((N, H, W, ldb), 7.0).to(dt)  # sentinel
    buf[..., :C] = x.to(dt)

    # fp64 reference on the stored input
    xd = buf[..., :C].double()
    mean, var = xd.mean((0, 1, 2)), xd.var((0, 1, 2), unbiased=False)
    a = torch.relu((xd - mean) * torch.rsqrt(var + EPS) * gamma.double() + beta.double())
    ref = F.conv2d(a.permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)

    # the buffer's statistics as the producers leave them: shifted sums spread over R replicas
    shift = (mean + 0.1 * var.sqrt()).float()
    dx = xd.reshape(M, C) - shift.double()
    acc = torch.zeros(R, 2, ldb)
    acc[:, 0, :C] = (dx.sum(0) / R).float()
    acc[:, 1, :C] = ((dx * dx).sum(0) / R).float()
    kout = 0.1 * torch.randn(NOUT, generator=g)

    buf, acc = buf.to(DEV), acc.to(DEV)
    before, acc0 = buf.clone(), acc.clone()
    sv_mean, sv_inv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    Fn.dense_conv3x3_forward(buf, C, slot, w.to(DEV), gamma.to(DEV), beta.to(DEV), EPS, acc=acc, R=R,
                             shift=shift.to(DEV), saved_mean=sv_mean, saved_invstd=sv_inv, stats=acc, stats_R=R,
                             stats_shift=kout.to(DEV))
    torch.cuda.synchronize()

    tol_y, tol_s = TOL[precision]
    e = rel_err(buf[..., slot:slot + NOUT], ref)
    print(f"{precision} {shape}: output rel err {e:.3e} (bound {tol_y})")
    assert e < tol_y
    assert torch.equal(buf[..., :slot], before[..., :slot]) and torch.equal(buf[..., slot + 16:], before[..., slot + 16:])
    assert not buf[..., slot + NOUT:slot + 16].any(), "slot channels 12..15 are exact zeros"
    assert rel_err(sv_mean, mean) < 1e-5 and rel_err(sv_inv, torch.rsqrt(var + EPS)) < 1e-5

    st = acc[:, :, slot:slot + 16].double().sum(0).cpu()
    d = ref.reshape(M, NOUT) - kout.double()
    e1, e2 = rel_err(st[0, :NOUT], d.sum(0)), rel_err(st[1, :NOUT], (d * d).sum(0))
    print(f"{precision} {shape}: statistics rel err {e1:.3e} {e2:.3e} (bound {tol_s})")
    assert e1 < tol_s and e2 < tol_s
    assert not st[:, NOUT:].any() and torch.equal(acc[:, :, :slot], acc0[:, :, :slot])
    assert torch.equal(acc[:, :, slot + 16:], acc0[:, :, slot + 16:])


@pytest.mark.parametrize("mode", ["train_deterministic", "inference"])
def test_dense_conv3x3_modes_with_store_pack(precision, mode):
    """The other forms of the same launch, with the operands of a ParamStore pack (16 rows, 4 of them pad):
    deterministic mode (grid capped at the replica count, strips strided) with the moving-statistics
    update, and inference from the moving statistics."""
    from azure_hc_intel_tf_amd.nn.params import ParamStore

    N, H, W, C = 3, 8, 8, 40  # 6 strips of 32 pixels on 3 replicas: the capped grid strides over two strips each
    dt = DTYPES[precision]
    M, slot, ldb = N * H * W, C, C + 16
    g = torch.Generator().manual_seed(2)
    ps = ParamStore(seed=0)
    p = ps.add("w", (16, 3, 3, C), True, ps.trunc_normal(math.sqrt(2.0 / 9 / NOUT)))
    kpad = (9 * C + 63) // 64 * 64
    pk = ps.add_pack(p, 16, 3, 3, C, kpad, 192, want_tr=False)
    ps.finalize(DEV, dtype_pack=torch.bfloat16 if dt == torch.float32 else dt, pack_lo=dt == torch.float32)
    p.data[NOUT:] = 0
    ps.repack()
    w = p.data[:NOUT]
    buf = torch.full((N, H, W, ldb), 7.0).to(dt)
    buf[..., :C] = torch.randn(N, H, W, C, generator=g).to(dt)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    xd = buf[..., :C].double()
    if mode == "inference":
        mean, var = torch.randn(C, generator=g).double(), (0.5 + torch.rand(C, generator=g)).double()
    else:
        mean, var = xd.mean((0, 1, 2)), xd.var((0, 1, 2), unbiased=False)
    a = torch.relu((xd - mean) * torch.rsqrt(var + EPS) * gamma.double() + beta.double())
    ref = F.conv2d(a.permute(0, 3, 1, 2), w.double().cpu().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    buf, gamma, beta = buf.to(DEV), gamma.to(DEV), beta.to(DEV)
    if mode == "inference":
        rm, rv = mean.float().to(DEV), var.float().to(DEV)
        Fn.dense_conv3x3_forward(buf, C, slot, w, gamma, beta, EPS, running_mean=rm, running_var=rv, wpack=pk.pack)
        assert torch.equal(rm.cpu(), mean.float()) and torch.equal(rv.cpu(), var.float())
        assert rel_err(buf[..., slot:slot + NOUT], ref) < TOL[precision][0]
        return
    Rd = Fn.det_replicas(M)
    assert Rd < 6, "fewer replicas than strips: the capped grid must stride"
    d = xd.reshape(M, C)
    acc0 = torch.zeros(Rd, 2, ldb)
    acc0[0, 0, :C], acc0[0, 1, :C] = d.sum(0).float(), (d * d).sum(0).float()
    runs = []
    Fn.set_deterministic(True)
    try:
        for _ in range(2):
            acc, rm, rv = acc0.to(DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            Fn.dense_conv3x3_forward(buf, C, slot, w, gamma, beta, EPS, acc=acc, R=Rd, momentum=0.9, running_mean=rm,
                                     running_var=rv, stats=acc, stats_R=Rd, wpack=pk.pack)
            runs.append((acc.cpu(), buf.cpu().clone()))
    finally:
        Fn.set_deterministic(False)
    assert rel_err(buf[..., slot:slot + NOUT], ref) < TOL[precision][0]
    assert rel_err(rm, 0.1 * mean) < 1e-5 and rel_err(rv, 0.9 + 0.1 * var * M / (M - 1)) < 1e-5
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # bitwise reproducible
    st = runs[0][0][:, :, slot:slot + NOUT].double().sum(0)
    assert rel_err(st[0], ref.reshape(M, NOUT).sum(0)) < TOL[precision][1]


@pytest.mark.parametrize("shape", [(2, 8, 8, 16), (1, 9, 12, 32)], ids=lambda s: "x".join(map(str, s)))
def test_dense_matches_preact_bitwise(precision, shape):
    """The dense layer's and the pre-activation conv's forward kernels are built from one set of helpers
    (csrc/kernels/patch3x3.h). Per output pixel both sum K in the same
    order (chunk, then tap) whatever the strip split -- 2 x 8 x 8: 4-row strips (dense) against 8-row strips (preact);
    1 x 9 x 12: a short last strip and a partial last tile -- so on a problem both ops accept y is bitwise equal.
    The statistics sum the strips in another order: they agree within the statistics bound of this file."""
    N, H, W, C = shape
    nout = 16
    dt = DTYPES[precision]
    M = N * H * W
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, C, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = (torch.randn(nout, 3, 3, C, generator=g) * math.sqrt(2.0 / 9 / nout)).to(DEV)
    buf = torch.full((N, H, W, C + 16), 7.0).to(dt)
    buf[..., :C] = x.to(dt)
    d = buf[..., :C].double().reshape(M, C)
    Rd = Fn.det_replicas(M)
    acc = torch.zeros(Rd, 2, C + 16)
    acc[0, 0, :C], acc[0, 1, :C] = d.sum(0).float(), (d * d).sum(0).float()
    buf, acc, gamma, beta = buf.to(DEV), acc.to(DEV), gamma.to(DEV), beta.to(DEV)
    acc_p = acc[:, :, :C].contiguous()
    out = torch.zeros(N, H, W, nout, dtype=dt, device=DEV)
    st_p = torch.zeros(Rd, 2, nout, device=DEV)
    Fn.set_deterministic(True)
    try:
        sv = Fn.preact_conv3x3_forward(buf[..., :C], w, gamma, beta, EPS, out, stride=1, acc=acc_p, R=Rd,
                                       out_stats=st_p, out_stats_R=Rd)
        sv_mean, sv_inv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        Fn.dense_conv3x3_forward(buf, C, C, w, gamma, beta, EPS, acc=acc, R=Rd, saved_mean=sv_mean,
                                 saved_invstd=sv_inv, stats=acc, stats_R=Rd)
        torch.cuda.synchronize()
    finally:
        Fn.set_deterministic(False)
    assert torch.equal(buf[..., C:], out), "y of the two ops differs"
    assert torch.equal(sv_mean, sv.mean[:C]) and torch.equal(sv_inv, sv.invstd[:C])
    st_d, st_q = acc[:, :, C:].sum(0), st_p.sum(0)
    e1, e2 = rel_err(st_d[0], st_q[0]), rel_err(st_d[1], st_q[1])
    print(f"{precision} {shape}: statistics dense against preact rel err {e1:.3e} {e2:.3e} (bound {TOL[precision][1]})")
    assert e1 < TOL[precision][1] and e2 < TOL[precision][1]
