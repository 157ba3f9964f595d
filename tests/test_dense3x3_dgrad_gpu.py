"""The dense layer's fused data-gradient / ReLU / BatchNorm-backward kernel (csrc/kernels/dense3x3_dgrad.hip) through
Fn.dense_conv3x3_dgrad against the same formula in fp64 on the CPU. Bounds are the project's, norm-relative: the
updated gin 3e-6 (fp32) / 1e-2 (16-bit), dgamma and dbeta 1e-5 / 1e-2 (tests/test_fp32_native_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.nn import layers
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.nn.params import ParamStore
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
NOUT = 12
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TOL_GIN = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 3e-6}
TOL_BN = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-5}
SHAPES = [
    (2, 8, 8, 16),      # less than one chunk (one live half), a strip = a whole image: the halo must not leak across images
    (1, 9, 12, 48),     # a partial second chunk, W != H, one strip of 108 pixels: a partial last tile, an idle eighth tile
    (3, 16, 16, 104),   # four chunks with C % 32 == 8, three slabs of two 128-pixel strips, images split across slabs
    (1, 41, 12, 24),    # strips of 10 + 10 + 10 + 10 + 1 rows in slabs of 3 + 2: the double buffer wraps, a short last strip
    (1, 50, 16, 40),    # seven strips (the last of 2 rows) in slabs of 3 + 3 + 1, two chunks
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
def test_dense_conv3x3_dgrad(precision, shape):
    N, H, W, C = shape
    dt, M = DTYPES[precision], N * H * W
    slot, ldb = C + 8, C + 40  # the slot at a non-zero offset inside a wider gradient buffer
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g)
    x[..., 1] += 50.0                      # |mean| >> std
    x[..., 5] = 0.25 * x[..., 5] - 20.0
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[3] = beta[C - 2] = -8.0           # entirely negative after BN: all masked by the ReLU
    w = torch.randn(16, 3, 3, C, generator=g) * 0.1
    G = torch.full((N, H, W, ldb), 3.0).to(dt)  # sentinel
    G[..., :C] = torch.randn(N, H, W, C, generator=g).to(dt)
    G[..., slot:slot + NOUT] = torch.randn(N, H, W, NOUT, generator=g).to(dt)
    G[..., slot + NOUT:slot + 16] = 0

    # statistics once, from the stored x, rounded to fp32: the op and the reference use the same values
    xd = x.to(dt).double()
    mean = xd.mean((0, 1, 2)).float()
    invstd = torch.rsqrt(xd.var((0, 1, 2), unbiased=False) + EPS).float()
    sc = gamma.double() * invstd.double()
    sh = beta.double() - mean.double() * sc
    # a reference mask that differs at one element costs ~ 1 / sqrt(n): move pre-activations off zero, once
    xd = torch.where((xd * sc + sh).abs() < 1e-3, (xd + 0.5).to(dt).double(), xd)
    pre = xd * sc + sh
    assert not (pre.abs() < 1e-3).any()
    buf = torch.full((N, H, W, ldb), 7.0).to(dt)  # sentinel
    buf[..., :C] = xd.to(dt)
    assert torch.equal(buf[..., :C].double(), xd)

    da = F.conv_transpose2d(G[..., slot:slot + NOUT].double().permute(0, 3, 1, 2), w[:NOUT].double().permute(0, 3, 1, 2),
                            padding=1).permute(0, 2, 3, 1)
    gm = torch.where(pre > 0, da, torch.zeros_like(da))
    xhat = (xd - mean.double()) * invstd.double()
    db_ref, dg_ref = gm.sum((0, 1, 2)), (gm * xhat).sum((0, 1, 2))
    gin_ref = G[..., :C].double() + sc * (gm - db_ref / M - xhat * dg_ref / M)

    buf, G = buf.to(DEV), G.to(DEV)
    buf0, G0 = buf.clone(), G.clone()
    dgamma, dbeta = torch.full((C,), 9.0, device=DEV), torch.full((C,), 9.0, device=DEV)
    ws = Fn.dense_dgrad_workspace(buf.shape, C, buf.dtype, DEV).fill_(float("nan"))
    Fn.dense_conv3x3_dgrad(buf, C, G[..., slot:slot + 16], w.to(DEV), gamma.to(DEV), beta.to(DEV), mean.to(DEV),
                           invstd.to(DEV), G[..., :C], dgamma, dbeta, NOUT, ws=ws)
    torch.cuda.synchronize()
    e = rel_err(G[..., :C], gin_ref), rel_err(dgamma, dg_ref), rel_err(dbeta, db_ref)
    print(f"{precision} {shape}: gin {e[0]:.3e} (bound {TOL_GIN[precision]}), dgamma {e[1]:.3e}, dbeta {e[2]:.3e} "
          f"(bound {TOL_BN[precision]})")
    assert not torch.isnan(G).any() and not torch.isnan(dgamma).any() and not torch.isnan(dbeta).any()
    assert e[0] < TOL_GIN[precision] and e[1] < TOL_BN[precision] and e[2] < TOL_BN[precision]
    assert torch.equal(buf, buf0) and torch.equal(G[..., C:], G0[..., C:])


def test_dense_conv3x3_dgrad_reproducible(precision):
    N, H, W, C = 3, 16, 16, 104
    g = torch.Generator().manual_seed(2)
    buf = torch.randn(N, H, W, C + 16, generator=g).to(DTYPES[precision]).to(DEV)
    G = torch.randn(N, H, W, C + 16, generator=g).to(DTYPES[precision]).to(DEV)
    w = torch.randn(16, 3, 3, C, generator=g).to(DEV)
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV)
    mean, invstd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    out = []
    try:
        for det in (False, False, True, True):
            Fn.set_deterministic(det)
            Gi, dg, db = G.clone(), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            Fn.dense_conv3x3_dgrad(buf, C, Gi[..., C:], w, gamma, beta, mean, invstd, Gi[..., :C], dg, db, NOUT)
            out.append((Gi.cpu(), dg.cpu(), db.cpu()))
    finally:
        Fn.set_deterministic(False)
    assert not torch.equal(out[0][0], G.cpu()) and out[0][1].abs().sum() > 0 and out[0][2].abs().sum() > 0
    assert all(torch.equal(a, b) for o in out[1:] for a, b in zip(out[0], o))


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_dense_block_backward_with_fused_dgrad(name):
    dt = DTYPES[name]
    set_gpu_compute_dtype(dt)
    Fn.set_f32_native(dt == torch.float32)
    saved = layers.FUSE_DENSE_DGRAD
    try:
        ps = ParamStore(seed=0)
        blk = layers.DenseBlock(ps, "b", (8, 8, 16), 3, 12)
        ps.finalize(DEV, dtype_pack=torch.bfloat16, pack_lo=dt == torch.float32)
        gen = torch.Generator().manual_seed(3)
        x = torch.randn(2, 8, 8, 16, generator=gen).to(dt).to(DEV)
        keep = blk.keep.to(DEV)
        G0 = torch.randn(2, 8, 8, blk.ctot, generator=gen).to(dt).to(DEV) * keep
        ps.repack()
        Fn.set_deterministic(True)  # atomics-free statistics: the two runs differ in the data-gradient path alone
        res = {}
        for on in (True, False):
            layers.FUSE_DENSE_DGRAD = on
            ps.zero_grad()
            ps.zero_stats()
            ps.persistbuf.zero_()
            blk.input_view(2, DEV).copy_(x)
            blk.forward()
            G = G0.clone()
            dx = blk.backward(G).clone()
            res[on] = (dx, G, [[p.grad.clone() for p in L.params()] for L in blk.subs])
        e = rel_err(res[True][0], res[False][0])
        print(f"{name}: input gradient fused against unfused rel err {e:.3e}")
        assert e < TOL_GIN[name] and res[False][0].abs().sum() > 0
        assert not res[True][1][..., ~keep].any(), "pad channels receive an exact zero update"
        for L, (w1, b1, g1), (w0, b0, g0) in zip(blk.subs, res[True][2], res[False][2]):
            ew, eb, eg = rel_err(w1, w0), rel_err(b1, b0), rel_err(g1, g0)
            print(f"{name} c_in {L.c_in}: fused against unfused rel err w.grad {ew:.3e} beta.grad {eb:.3e} gamma.grad {eg:.3e}")
            assert ew < TOL_GIN[name] and eb < TOL_BN[name] and eg < TOL_BN[name] and g0.abs().sum() > 0
            pad = ~keep[:L.c_in]
            assert not b1[pad].any() and not g1[pad].any()
    finally:
        layers.FUSE_DENSE_DGRAD = saved
        Fn.set_deterministic(False)
        Fn.set_f32_native(False)
        set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("what, match", [
    ("c_in", "C_in must be a multiple of 8"),
    ("nout", "Nout <= 16"),
    ("ws", "workspace"),
    ("dtype", "dtypes differ"),
    ("overlap", "dz and gin overlap"),
])
def test_dense_conv3x3_dgrad_refusals(what, match):
    ops = _ext.ops()
    N, H, W, C = 1, 4, 4, 16
    x = torch.zeros(N, H, W, 32, dtype=torch.bfloat16, device=DEV)
    G = torch.zeros(N, H, W, 32, dtype=torch.float16 if what == "dtype" else torch.bfloat16, device=DEV)
    dz = G[..., 8:24] if what == "overlap" else G[..., 16:]
    v = torch.ones(C, device=DEV)
    w = torch.zeros(16, 3, 3, C, device=DEV)
    geom = [N, H, W, 12 if what == "c_in" else C, 32, 32, 32, 17 if what == "nout" else 12]
    need = ops.dense_conv3x3_dgrad_ws([N, H, W, C, 32, 32, 32, 12], False)
    ws = torch.zeros(need - 1 if what == "ws" else need, device=DEV)
    with pytest.raises(RuntimeError, match="dense_conv3x3_dgrad.*" + match):
        ops.dense_conv3x3_dgrad(x, dz, G[..., :C], w, v, v, v, v, ws, v.clone(), v.clone(), geom)
