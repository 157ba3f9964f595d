"""The one-launch pre-activation basic block of 16-bit inference (csrc/kernels/preact_block.hip) through
Fn.preact_block_inference against the definition in fp64 on the CPU. The output bound is 2x the largest norm-relative
error that the unfused 16-bit chain (bn_inference + conv_bn_inference + conv with the residual add) shows against the
same reference on the same inputs over SHAPES, per dtype (measured on an MI355X, profiles/resnet_cifar_v2_block.txt:
chain bf16 3.152e-3, fp16 3.797e-4); both paths round a1 and a2 to 16 bits once. The chain's error is printed beside the
kernel's."""
import math

import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn import layers as L
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Evaluator, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
BOUND = {"bf16": 2 * 3.152e-3, "fp16": 2 * 3.797e-4}
SHAPES = [  # (N, H, W, C_in, Nout, stride)
    (2, 8, 8, 16, 16, 1),    # half a chunk; the whole image in one strip, both halo rows outside the image
    (1, 10, 32, 16, 16, 1),  # several strips with a short last one; recomputed halo rows inside the image
    (2, 6, 8, 64, 64, 1),    # two chunks in both phases, four column tiles, H != W
    (2, 12, 16, 32, 64, 2),  # stride 2, asymmetric pad, C_in != Nout
    (3, 9, 7, 16, 32, 2),    # odd sizes (symmetric pads), N not a power of two
]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bn_relu_conv(t, w, bn, s):
    gamma, beta, mean, var = (v.double() for v in bn)
    a = torch.relu((t - mean) * torch.rsqrt(var + EPS) * gamma + beta)
    (pt, pb), (pl, pr) = Fn.same_pads(t.shape[1], 3, s), Fn.same_pads(t.shape[2], 3, s)
    a = F.pad(a.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(a, w.double().permute(0, 3, 1, 2), stride=s).permute(0, 2, 3, 1)


def reference(x, res, w1, bn1, w2, bn2, s):
    """The definition in fp64 on the 16-bit inputs; NHWC in and out."""
    return bn_relu_conv(bn_relu_conv(x.double(), w1, bn1, s), w2, bn2, 1) + res.double()


def inputs(shape, dt, seed=1, positive=False):
    """x, res, the kernels and [gamma, beta, moving mean, moving variance] of both BNs. Default: a channel of x with
    |mean| = 50 std, a channel of each BN driven entirely negative. ``positive``: relu(shift) > 0 on every channel."""
    N, H, W, C, nout, s = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g)
    res = torch.randn(N, -(-H // s), -(-W // s), nout, generator=g)
    w1 = torch.randn(nout, 3, 3, C, generator=g) * math.sqrt(2.0 / 9 / C)
    w2 = torch.randn(nout, 3, 3, nout, generator=g) * math.sqrt(2.0 / 9 / nout)
    bns = []
    for c in (C, nout):
        gamma, beta = 0.5 + torch.rand(c, generator=g), 0.3 * torch.randn(c, generator=g)
        mean, var = 0.2 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
        if positive:
            beta = beta.abs() + 1.0 + (mean * gamma * torch.rsqrt(var + EPS)).abs()
        else:
            beta[3] = -40.0
        bns.append([gamma, beta, mean, var])
    if not positive:
        x[..., 1] += 50.0
        bns[0][2][1] += 50.0
    return x.to(dt), res.to(dt), w1, bns[0], w2, bns[1]


def run_kernel(x, res, w1, bn1, w2, bn2, s):
    """The op on rows wider than the channels: NaN past C_in in x's rows, a sentinel past Nout in out's."""
    N, H, W, C = x.shape
    nout = w1.shape[0]
    xp = torch.full((N, H, W, C + 8), float("nan"), dtype=x.dtype)
    xp[..., :C] = x
    out = torch.full(tuple(res.shape[:3]) + (nout + 8,), 7.0).to(x.dtype).to(DEV)
    d = lambda bn: [v.to(DEV) for v in bn]
    Fn.preact_block_inference(xp.to(DEV)[..., :C], w1.to(DEV), *d(bn1), EPS, w2.to(DEV), *d(bn2), EPS, res.to(DEV),
                              out[..., :nout], s)
    torch.cuda.synchronize()
    assert bool((out[..., nout:] == 7.0).all()), "the gap of out's rows is not the kernel's to write"
    return out[..., :nout]


def run_chain(x, res, w1, bn1, w2, bn2, s):
    """Today's unfused 16-bit chain: bn_inference, conv1 with BN2 + ReLU in its epilogue, conv2 with the residual."""
    N, H, W, C = x.shape
    nout = w1.shape[0]
    (pt, pb), (pl, pr) = Fn.same_pads(H, 3, s), Fn.same_pads(W, 3, s)
    d = lambda bn: [v.to(DEV) for v in bn]
    x, res, w1, w2 = x.to(DEV), res.to(DEV), w1.to(DEV), w2.to(DEV)
    a1 = Fn.bn_inference(x, *d(bn1), EPS, torch.empty_like(x), True)
    s1 = Fn.ConvSpec(C, C, nout, 3, 3, s, s, pt, pl, pb, pr)
    a2 = Fn.conv_bn_inference(a1, s1, Fn.dense_pack(w1, x.dtype)[0], w1, *d(bn2), EPS, torch.empty_like(res), True)
    s2 = Fn.ConvSpec(nout, nout, nout, 3, 3, 1, 1, 1, 1, 1, 1)
    return Fn.conv_forward(a2, s2, Fn.dense_pack(w2, x.dtype)[0], w2, torch.empty_like(res), residual=res)


@pytest.fixture(params=list(DTYPES))
def precision(request):
    set_gpu_compute_dtype(DTYPES[request.param])
    yield request.param
    set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_preact_block_output(precision, shape):
    args = inputs(shape, DTYPES[precision])
    ref = reference(*args, shape[5])
    ek, ec = rel_err(run_kernel(*args, shape[5]), ref), rel_err(run_chain(*args, shape[5]), ref)
    print(f"{precision} {shape}: kernel {ek:.3e}, unfused chain {ec:.3e} (bound {BOUND[precision]:.2e})")
    assert ek < BOUND[precision]


def test_preact_block_borders_are_zero_not_relu_shift(precision):
    shape = (2, 12, 16, 32, 64, 2)  # two strips: halo rows inside and outside the image, asymmetric pads
    args = inputs(shape, DTYPES[precision], seed=2, positive=True)
    assert rel_err(run_kernel(*args, 2), reference(*args, 2)) < BOUND[precision]


def _refusal_args(case):
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=DEV)
    a = dict(x=z(1, 8, 8, 16), c=16, nout=16, s=1, res=z(1, 8, 8, 16), out=z(1, 8, 8, 16))
    big = lambda: torch.empty(8192, 1024, 8, 16, dtype=torch.bfloat16, device=DEV)  # exactly 2^31 bytes, never touched
    a.update({
        "c_in": lambda: dict(x=z(1, 8, 8, 24), c=24),
        "nout": lambda: dict(nout=48, res=z(1, 8, 8, 48), out=z(1, 8, 8, 48)),
        "stride": lambda: dict(s=3, res=z(1, 3, 3, 16), out=z(1, 3, 3, 16)),
        "ld": lambda: dict(x=z(1, 8, 8, 20)[..., :16]),
        "rows": lambda: dict(x=z(1, 16, 8, 16)[:, ::2]),
        "dtype": lambda: dict(res=z(1, 8, 8, 16, dt=torch.float16)),
        "fp32": lambda: dict(x=z(1, 8, 8, 16, dt=torch.float32)),
        "planes": lambda: dict(x=Fn.Planes(z(3, 1, 8, 8, 16))),
        "alias": lambda: dict(out=a["x"]),
        "alias_res": lambda: dict(out=a["res"]),
        "res_shape": lambda: dict(res=z(1, 4, 8, 16)),
        "out_shape": lambda: dict(out=z(1, 8, 4, 16)),
        "fit": lambda: dict(x=z(1, 8, 64, 64), c=64, nout=64, res=z(1, 8, 64, 64), out=z(1, 8, 64, 64)),
        "2gib": lambda: (lambda x: dict(x=x, res=x, out=big()))(big()),
    }[case]())
    return a


@pytest.mark.parametrize("case,msg", [
    ("c_in", "C_in must be 16, 32 or 64"), ("nout", "Nout must be 16, 32 or 64"), ("stride", "stride must be 1 or 2"),
    ("ld", "ld must be a multiple of 8"), ("rows", "non-contiguous rows"), ("dtype", "dtypes differ"),
    ("fp32", "float32 tensors are not taken"), ("planes", "not Planes"), ("alias", "out aliases x"),
    ("alias_res", "out aliases res"), ("res_shape", "res must be"), ("out_shape", "out must be"),
    ("fit", "does not fit"), ("2gib", "below 2 GiB")])
def test_preact_block_refusals(case, msg):
    a = _refusal_args(case)
    c, nout = a["c"], a["nout"]
    v1, v2 = torch.ones(c, device=DEV), torch.ones(nout, device=DEV)
    Fn.set_f32_native(case == "fp32")
    try:
        with pytest.raises(RuntimeError, match=msg):
            Fn.preact_block_inference(a["x"], torch.zeros(nout, 3, 3, c, device=DEV), v1, v1, v1, v1, EPS,
                                      torch.zeros(nout, 3, 3, nout, device=DEV), v2, v2, v2, v2, EPS, a["res"], a["out"],
                                      a["s"])
    finally:
        Fn.set_f32_native(False)


def _model_logits(on, calls):
    """resnet20_v2, bf16, forward-only, captured: logits of two replays, BN2's gamma of block 2 changed between them."""
    L.FUSE_PREACT_BLOCK = on
    m = create_model("resnet20_v2", data_name="cifar10", device="cuda", compute_dtype="bf16", seed=5)
    img, lab = synthetic_batch(m, 4, seed=4)
    for l in m.all_layers():  # non-trivial moving statistics
        if hasattr(l, "rmean"):
            n = l.rmean.data.numel()
            l.rmean.data.copy_(0.1 * torch.sin(torch.arange(n, device="cuda").float()))
            l.rvar.data.copy_(1.0 + 0.5 * torch.cos(torch.arange(n, device="cuda").float()))
    ev = Evaluator(m, 4, use_graph=True, graph_warmup=1)
    ev.step(img, lab)  # eager: the spies count this forward
    calls.update(block=Fn.preact_block_inference.n, bn=Fn.bn_inference.n)
    out = []
    for scale in (1.0, 3.0):
        m.blocks[1].c1.gamma.data.mul_(scale)
        ev.step(img, lab)
        torch.cuda.synchronize()
        out.append(ev.logits[:, :m.num_classes].double().cpu())
    assert ev._g is not None, "the forward was not captured"
    return out


def test_model_forward_only_one_launch_blocks(monkeypatch):
    def spy(name):
        f = getattr(Fn, name)

        def g(*a, **k):
            g.n += 1
            return f(*a, **k)
        g.n = 0
        monkeypatch.setattr(Fn, name, g)
    default = L.FUSE_PREACT_BLOCK
    try:
        res = {}
        for on in (True, False):
            spy("preact_block_inference")
            spy("bn_inference")
            calls = {}
            res[on] = (_model_logits(on, calls), calls)
    finally:
        L.FUSE_PREACT_BLOCK = default
        set_gpu_compute_dtype(torch.bfloat16)
    (a, ca), (b, cb) = res[True], res[False]
    assert ca == dict(block=9, bn=1) and cb == dict(block=0, bn=10), (ca, cb)  # bn: the post-norm, + one per block
    e = rel_err(a[0], b[0])
    print(f"forward-only logits, one-launch blocks against the chain: rel err {e:.3e}; gamma x3 moves them by "
          f"{rel_err(a[1], a[0]):.3e}")
    assert e < BOUND["bf16"]
    assert rel_err(a[1], a[0]) > 10 * BOUND["bf16"], "a BN2 gamma changed between replays must be picked up"
    assert rel_err(a[1], b[1]) < BOUND["bf16"]
