"""The dense layer's fused BN-ReLU weight-gradient kernel (csrc/kernels/dense3x3_wgrad.hip) through
Fn.dense_conv3x3_wgrad against the same formula in fp64 on the CPU. Bounds are the project's, norm-relative:
3e-6 on the fp32 path (the weight-gradient bound of tests/test_fp32_native_gpu.py), 1e-2 on the 16-bit paths
(tests/test_kernels_gpu.py::test_conv_wgrad)."""
import pytest
import torch

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
TOL = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 3e-6}
SHAPES = [
    (1, 4, 8, 16),      # one strip, one slab: the fold adds a single partial; rows 12..15 of dw stay untouched
    (2, 8, 8, 16),      # less than one chunk, two strips of two K blocks
    (1, 9, 12, 48),     # a partial second chunk, one strip with a partial last K block, W != H
    (3, 16, 16, 104),   # several chunks, slabs of unequal strip counts, the double buffer wraps
    (1, 41, 12, 24),    # strips of 10 + 10 + 10 + 10 + 1 rows in slabs of 3 + 2: a short last strip, unequal slabs
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
def test_dense_conv3x3_wgrad(precision, shape):
    N, H, W, C = shape
    dt = DTYPES[precision]
    slot, ldb = C + 8, C + 40  # the slot at a non-zero offset inside a wider gradient buffer
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g)
    x[..., 1] += 50.0                      # |mean| >> std
    x[..., 5] = 0.25 * x[..., 5] - 20.0
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[3] = beta[C - 2] = -8.0           # entirely negative after BN: all masked by the ReLU
    buf = torch.full((N, H, W, ldb), 7.0).to(dt)  # sentinel
    buf[..., :C] = x.to(dt)
    G = torch.full((N, H, W, ldb), 3.0).to(dt)
    G[..., slot:slot + NOUT] = torch.randn(N, H, W, NOUT, generator=g).to(dt)
    G[..., slot + NOUT:slot + 16] = 0

    # fp64 reference on the stored tensors
    xd = buf[..., :C].double()
    mean, var = xd.mean((0, 1, 2)), xd.var((0, 1, 2), unbiased=False)
    invstd = torch.rsqrt(var + EPS)
    a = torch.relu((xd - mean) * invstd * gamma.double() + beta.double())
    ref = torch.nn.grad.conv2d_weight(a.permute(0, 3, 1, 2), (NOUT, C, 3, 3),
                                      G[..., slot:slot + NOUT].double().permute(0, 3, 1, 2), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(NOUT, 9 * C)

    buf, G = buf.to(DEV), G.to(DEV)
    buf0, G0 = buf.clone(), G.clone()
    base = torch.randn(16, 9 * C, generator=g).to(DEV)
    dw = base.clone()
    ws = Fn.dense_wgrad_workspace(buf.shape, C, buf.dtype, DEV).fill_(float("nan"))
    Fn.dense_conv3x3_wgrad(buf, C, G[..., slot:slot + 16], gamma.to(DEV), beta.to(DEV), mean.float().to(DEV),
                           invstd.float().to(DEV), dw, NOUT, ws=ws)
    torch.cuda.synchronize()
    e = rel_err((dw - base)[:NOUT], ref)
    print(f"{precision} {shape}: dw rel err {e:.3e} (bound {TOL[precision]})")
    assert not torch.isnan(dw).any()
    assert e < TOL[precision]
    assert torch.equal(dw[NOUT:], base[NOUT:]), "rows 12..15 receive nothing"
    assert torch.equal(buf, buf0) and torch.equal(G, G0)


def test_dense_conv3x3_wgrad_reproducible(precision):
    N, H, W, C = 3, 16, 16, 104
    g = torch.Generator().manual_seed(2)
    buf = torch.randn(N, H, W, C + 16, generator=g).to(DTYPES[precision]).to(DEV)
    G = torch.randn(N, H, W, C + 16, generator=g).to(DTYPES[precision]).to(DEV)
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV)
    mean, invstd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    out = []
    try:
        for det in (False, False, True, True):
            Fn.set_deterministic(det)
            dw = torch.zeros(16, 9 * C, device=DEV)
            Fn.dense_conv3x3_wgrad(buf, C, G[..., C:], gamma, beta, mean, invstd, dw, NOUT)
            out.append(dw.cpu())
    finally:
        Fn.set_deterministic(False)
    assert out[0].abs().sum() > 0 and all(torch.equal(out[0], o) for o in out[1:])


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_dense_block_backward_with_fused_wgrad(name):
    dt = DTYPES[name]
    set_gpu_compute_dtype(dt)
    Fn.set_f32_native(dt == torch.float32)
    saved = layers.FUSE_DENSE_WGRAD
    try:
        ps = ParamStore(seed=0)
        blk = layers.DenseBlock(ps, "b", (8, 8, 16), 3, 12)
        ps.finalize(DEV, dtype_pack=torch.bfloat16, pack_lo=dt == torch.float32)
        gen = torch.Generator().manual_seed(3)
        x = torch.randn(2, 8, 8, 16, generator=gen).to(dt).to(DEV)
        G0 = torch.randn(2, 8, 8, blk.ctot, generator=gen).to(dt).to(DEV) * blk.keep.to(DEV)
        ps.repack()
        Fn.set_deterministic(True)  # atomics-free statistics: the two runs differ in the weight gradient alone
        res = {}
        for on in (True, False):
            layers.FUSE_DENSE_WGRAD = on
            ps.zero_grad()
            ps.zero_stats()
            ps.persistbuf.zero_()
            blk.input_view(2, DEV).copy_(x)
            blk.forward()
            dx = blk.backward(G0.clone()).clone()
            res[on] = (dx, [[p.grad.clone() for p in L.params()] for L in blk.subs])
        assert torch.equal(res[True][0], res[False][0])
        for L, (w1, b1, g1), (w0, b0, g0) in zip(blk.subs, res[True][1], res[False][1]):
            e = rel_err(w1, w0)
            print(f"{name} c_in {L.c_in}: w.grad fused against unfused rel err {e:.3e}")
            assert e < TOL[name] and w0.abs().sum() > 0
            assert torch.equal(b1, b0) and torch.equal(g1, g0)
            assert not w1[12:].any() and not w1[..., ~blk.keep[:L.c_in].to(DEV)].any()
    finally:
        layers.FUSE_DENSE_WGRAD = saved
        Fn.set_deterministic(False)
        Fn.set_f32_native(False)
        set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("what, match", [
    ("c_in", "C_in must be a multiple of 8"),
    ("nout", "Nout <= 16"),
    ("ws", "workspace"),
    ("dtype", "dtypes differ"),
])
def test_dense_conv3x3_wgrad_refusals(what, match):
    ops = _ext.ops()
    N, H, W, C = 1, 4, 4, 16
    x = torch.zeros(N, H, W, 32, dtype=torch.bfloat16, device=DEV)
    dz = torch.zeros(N, H, W, 32, dtype=torch.float16 if what == "dtype" else torch.bfloat16, device=DEV)[..., 16:]
    v = torch.ones(C, device=DEV)
    dw = torch.zeros(16, 9 * C, device=DEV)
    geom = [N, H, W, 12 if what == "c_in" else C, 32, 16, 32, 17 if what == "nout" else 12]
    need = ops.dense_conv3x3_wgrad_ws([N, H, W, C, 32, 16, 32, 12], False)
    ws = torch.zeros(need - 1 if what == "ws" else need, device=DEV)
    with pytest.raises(RuntimeError, match="dense_conv3x3_wgrad.*" + match):
        ops.dense_conv3x3_wgrad(x, dz, v, v, v, v, ws, dw, geom)
