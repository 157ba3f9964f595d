"""The fused BN-ReLU weight gradient of the ResNet-v2 pre-activation conv (csrc/kernels/preact3x3_wgrad.hip) through
Fn.preact_conv3x3_wgrad against the definition in fp64 on the CPU, on the stored (rounded) tensors. Bounds are the
project's, norm-relative, those of tests/test_dense3x3_wgrad_gpu.py: 3e-6 on the fp32 path, 1e-2 on the 16-bit paths."""
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
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TOL = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 3e-6}
SHAPES = [  # (N, H, W, C_in, Nout, stride)
    (1, 4, 8, 16, 16, 1),     # one strip, one slab: the fold adds a single partial; one K block, three waves idle
    (2, 8, 8, 16, 16, 1),     # half a chunk; four waves split two K blocks
    (2, 6, 8, 64, 64, 1),     # two chunks, four row tiles (two units per wave), H != W
    (1, 32, 32, 16, 32, 2),   # the widest stride-2 patch (17 x 33), 128-pixel strips, halo rows shared between strips
    (2, 12, 16, 32, 64, 2),   # asymmetric pad (none on top / left, one below / right)
    (3, 9, 12, 64, 16, 2),    # odd H: pt = 1 at stride 2 while pl = 0; 30 pixels = a partial last K block
    (5, 16, 16, 32, 32, 1),   # 10 strips in slabs of 3 + 3 + 3 + 1: unequal slabs, the double buffer wraps
    (1, 20, 16, 16, 16, 1),   # strips of 8 + 8 + 4 rows: a short last strip (the plan takes the 12 x 16 map above whole)
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


def inputs(shape, dt, seed=1):
    """x inside rows of C + 8 channels (sentinel in the gap), dz a channel-slice view of a wider tensor."""
    N, H, W, C, nout, s = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.full((N, H, W, C + 8), 7.0)
    x[..., :C] = torch.randn(N, H, W, C, generator=g)
    x[..., 1] += 50.0                      # |mean| = 50 std
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[3] = -8.0                         # entirely negative after BN: all masked by the ReLU
    G = torch.full((N, -(-H // s), -(-W // s), nout + 16), 3.0)
    G[..., 8:8 + nout] = torch.randn(N, -(-H // s), -(-W // s), nout, generator=g)
    return x.to(dt), G.to(dt), gamma, beta, g


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_preact_conv3x3_wgrad(precision, shape):
    N, H, W, C, nout, s = shape
    x, G, gamma, beta, g = inputs(shape, DTYPES[precision])
    xd = x[..., :C].double()
    mean, var = xd.mean((0, 1, 2)), xd.var((0, 1, 2), unbiased=False)
    invstd = torch.rsqrt(var + EPS)
    a = torch.relu((xd - mean) * invstd * gamma.double() + beta.double())
    (pt, pb), (pl, pr) = Fn.same_pads(H, 3, s), Fn.same_pads(W, 3, s)
    ref = torch.nn.grad.conv2d_weight(F.pad(a.permute(0, 3, 1, 2), (pl, pr, pt, pb)), (nout, C, 3, 3),
                                      G[..., 8:8 + nout].double().permute(0, 3, 1, 2), stride=s)
    ref = ref.permute(0, 2, 3, 1).reshape(nout, 9 * C)

    x, G = x.to(DEV), G.to(DEV)
    x0, G0 = x.clone(), G.clone()
    base = torch.randn(nout, 9 * C, generator=g).to(DEV)
    dw = base.clone()
    ws = Fn.preact_wgrad_workspace(x.shape, C, nout, s, x.dtype, DEV).fill_(float("nan"))
    Fn.preact_conv3x3_wgrad(x, C, G[..., 8:8 + nout], gamma.to(DEV), beta.to(DEV), mean.float().to(DEV),
                            invstd.float().to(DEV), dw, s, ws=ws)
    torch.cuda.synchronize()
    e = rel_err(dw - base, ref)
    print(f"{precision} {shape}: dw rel err {e:.3e} (bound {TOL[precision]})")
    assert not torch.isnan(dw).any()
    assert e < TOL[precision]
    assert torch.equal(x, x0) and torch.equal(G, G0)


def test_preact_conv3x3_wgrad_reproducible(precision):
    shape = (5, 16, 16, 32, 32, 1)
    x, G, gamma, beta, _ = inputs(shape, DTYPES[precision], seed=2)
    x, dz, gamma, beta = x.to(DEV), G.to(DEV)[..., 8:40], gamma.to(DEV), beta.to(DEV)
    mean, invstd = torch.zeros(32, device=DEV), torch.ones(32, device=DEV)
    out = []
    try:
        for det in (False, False, True, True):
            Fn.set_deterministic(det)
            dw = torch.zeros(32, 9 * 32, device=DEV)
            Fn.preact_conv3x3_wgrad(x, 32, dz, gamma, beta, mean, invstd, dw, 1)
            out.append(dw.cpu())
    finally:
        Fn.set_deterministic(False)
    assert out[0].abs().sum() > 0 and all(torch.equal(out[0], o) for o in out[1:])


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_preact_conv_backward_with_fused_wgrad(name):
    dt = DTYPES[name]
    set_gpu_compute_dtype(dt)
    Fn.set_f32_native(dt == torch.float32)
    saved = layers.FUSE_PREACT_WGRAD
    try:
        ps, scratch = ParamStore(seed=0), {}
        pc = layers.PreActConv(ps, "b", (12, 16, 32), 64, 2, scratch)
        ps.finalize(DEV, dtype_pack=torch.bfloat16, pack_lo=dt == torch.float32)
        gen = torch.Generator().manual_seed(3)
        x = (torch.randn(4, 12, 16, 32, generator=gen) + 0.5).to(dt).to(DEV)
        d1 = torch.randn(4, 6, 8, 64, generator=gen).to(dt).to(DEV)
        add = torch.randn(4, 12, 16, 32, generator=gen).to(dt).to(DEV)
        ps.repack()
        Fn.set_deterministic(True)  # atomics-free statistics: the two runs differ in conv1's weight gradient alone
        res = {}
        for on in (True, False):
            layers.FUSE_PREACT_WGRAD = on
            ps.zero_grad()
            ps.zero_stats()
            ps.persistbuf.zero_()
            scratch.clear()
            pc.forward(x)
            assert pc._fused
            dx = pc.backward(d1.clone(), add.clone()).clone()
            torch.cuda.synchronize()
            operands = [k for k, v in scratch.items() if tuple(v.shape) == tuple(x.shape)]
            res[on] = (dx, pc.conv.w.grad.clone(), [p.grad.clone() for p in pc.pre.params()],
                       [p.grad.clone() for p in pc.conv.params()[1:]], operands)
        assert torch.equal(res[True][0], res[False][0]) and res[True][0].abs().sum() > 0
        e = rel_err(res[True][1], res[False][1])
        print(f"{name}: conv1 w.grad fused against unfused rel err {e:.3e}")
        assert e < TOL[name] and res[False][1].abs().sum() > 0
        for a, b in zip(res[True][2] + res[True][3], res[False][2] + res[False][3]):
            assert torch.equal(a, b)
        assert not res[True][4] and len(res[False][4]) == 1, "fused: no re-materialised operand in the scratch"
    finally:
        layers.FUSE_PREACT_WGRAD = saved
        Fn.set_deterministic(False)
        Fn.set_f32_native(False)
        set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("what, match", [
    ("c_in", "C_in must be 16, 32 or 64"),
    ("nout", "Nout must be 16, 32 or 64"),
    ("stride", "stride must be 1 or 2"),
    ("ws", "workspace"),
    ("dtype", "dtypes differ"),
])
def test_preact_conv3x3_wgrad_refusals(what, match):
    ops = _ext.ops()
    N, H, W, C, nout = 1, 4, 4, 16, 16
    x = torch.zeros(N, H, W, 32, dtype=torch.bfloat16, device=DEV)
    dz = torch.zeros(N, H, W, nout, dtype=torch.float16 if what == "dtype" else torch.bfloat16, device=DEV)
    v = torch.ones(C, device=DEV)
    dw = torch.zeros(nout, 9 * C, device=DEV)
    geom = [N, H, W, 24 if what == "c_in" else C, 32, nout, 48 if what == "nout" else nout, 3 if what == "stride" else 1]
    need = ops.preact_conv3x3_wgrad_ws([N, H, W, C, 32, nout, nout, 1], False)
    ws = torch.zeros(need - 1 if what == "ws" else need, device=DEV)
    with pytest.raises(RuntimeError, match="preact_conv3x3_wgrad.*" + match):
        ops.preact_conv3x3_wgrad(x, dz, v, v, v, v, ws, dw, geom)
