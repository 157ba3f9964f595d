"""The one-launch MobileNet-v2 inverted-residual block of 16-bit inference (csrc/kernels/mbconv_block.hip) through
Fn.mbconv_block_inference against the definition in fp64 on the CPU. The output bound is 2x the largest norm-relative
error that today's unfused 16-bit chain (conv_forward, bn_inference, dwconv_forward, bn_inference, conv_forward,
bn_inference with the residual) shows against the same reference on the same inputs over SHAPES, per dtype (measured on
an MI355X, profiles/mobilenet_block.txt: chain bf16 1.534e-2, fp16 2.263e-3; kernel 1.235e-2 / 1.652e-3); the kernel rounds h1 and h2 once each,
the chain also rounds its three raw conv outputs. The chain's error is printed beside the kernel's. The +-40 betas go to
BN1 and BN2 (a ReLU6 to drive); on BN3, which has none, they would only swell the norm the error is measured against."""
import math

import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn import layers as L
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-3
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
CHAIN = {"bf16": 1.534e-2, "fp16": 2.263e-3}  # the unfused chain's largest error over SHAPES, measured
BOUND = {k: 2 * v for k, v in CHAIN.items()}
SHAPES = [  # (N, H, W, cin, cout, t, stride)
    (2, 7, 7, 160, 320, 6, 1),  # whole image below one pixel-tile multiple; the widest cout; 30 chunks; no res
    (1, 9, 16, 24, 24, 6, 1),   # identity res; K padded 24 -> 32; mid 144 (a partial last chunk); a short last strip
    (2, 8, 12, 16, 24, 6, 2),   # stride 2 on even sizes (pads bottom / right only); cout padded 24 -> 32
    (3, 7, 5, 32, 64, 6, 2),    # odd sizes (symmetric pads), N not a power of two
    (2, 5, 6, 64, 96, 6, 1),    # stride 1 without res; two K steps in the expand
    (1, 6, 16, 32, 16, 1, 1),   # the t = 1 form
]
SMALL = dict(image_size=32, blocks=((1, 16, 1, 1), (6, 24, 2, 2)), image_channels=8)  # tests/test_mobilenet_gpu.py's


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def reference(x, we, bn1, wd, bn2, wp, bn3, s, res):
    """The definition in fp64 on the 16-bit inputs; NHWC in and out."""
    bn = lambda t, p: (t - p[2].double()) * torch.rsqrt(p[3].double() + EPS) * p[0].double() + p[1].double()
    h = x.double()
    if we is not None:
        h = bn(h @ we.double().reshape(we.shape[0], -1).t(), bn1).clamp(0, 6)
    (pt, pb), (pl, pr) = Fn.same_pads(x.shape[1], 3, s), Fn.same_pads(x.shape[2], 3, s)
    h = F.pad(h.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    h = F.conv2d(h, wd.double().unsqueeze(1), stride=s, groups=wd.shape[0]).permute(0, 2, 3, 1)
    o = bn(bn(h, bn2).clamp(0, 6) @ wp.double().reshape(wp.shape[0], -1).t(), bn3)
    return o + res.double() if res is not None else o


def inputs(shape, dt, seed=1):
    """x, the kernels, the three BNs and res. Channel 1 of x has |mean| = 50 std, matched by the moving mean of the BN
    behind it; channel 3 of BN1 and BN2 is driven entirely negative, channel 5 above 6."""
    N, H, W, cin, cout, t, s = shape
    mid = t * cin
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g)
    x = r(N, H, W, cin)
    x[..., 1] += 50.0
    x = x.to(dt)
    we = r(mid, 1, 1, cin) * math.sqrt(2.0 / cin) if t != 1 else None
    wd, wp = r(mid, 3, 3) * math.sqrt(2.0 / 9), r(cout, 1, 1, mid) * math.sqrt(1.0 / mid)
    bns = []
    for c in (mid, mid, cout):
        bns.append([0.5 + torch.rand(c, generator=g), 0.3 * r(c) + 1.0, 0.2 * r(c), 0.5 + torch.rand(c, generator=g)])
    if t != 1:
        bns[0][2] += 50.0 * we[:, 0, 0, 1]
    else:
        bns[1][2][1] += 50.0 * wd[1].sum()
    for b in bns[:2] if t != 1 else bns[1:2]:
        b[1][3], b[1][5] = -40.0, 40.0
    res = r(N, H, W, cout).to(dt) if s == 1 and cin == cout else None
    return x, we, bns[0], wd, bns[1], wp, bns[2], s, res


def run_kernel(x, we, bn1, wd, bn2, wp, bn3, s, res):
    """The op on rows wider than the channels: NaN past cin in x's rows, a sentinel past cout in out's."""
    N, H, W, cin = x.shape
    cout = wp.shape[0]
    xp = torch.full((N, H, W, cin + 8), float("nan"), dtype=x.dtype)
    xp[..., :cin] = x
    out = torch.full((N, -(-H // s), -(-W // s), cout + 8), 7.0).to(x.dtype).to(DEV)
    d = lambda bn: [v.to(DEV) for v in bn]
    Fn.mbconv_block_inference(xp.to(DEV)[..., :cin], we.to(DEV) if we is not None else None, d(bn1), EPS, wd.to(DEV),
                              d(bn2), EPS, wp.to(DEV), d(bn3), EPS, out[..., :cout], s,
                              res=res.to(DEV) if res is not None else None)
    torch.cuda.synchronize()
    assert bool((out[..., cout:] == 7.0).all()), "the gap of out's rows is not the kernel's to write"
    return out[..., :cout]


def run_chain(x, we, bn1, wd, bn2, wp, bn3, s, res):
    """Today's unfused 16-bit chain: expand GEMM, BN + ReLU6, depthwise stencil, BN + ReLU6, projection GEMM, BN + res."""
    N, H, W, cin = x.shape
    mid, cout = wd.shape[0], wp.shape[0]
    P, Q = -(-H // s), -(-W // s)
    d = lambda bn: [v.to(DEV) for v in bn]
    e = lambda *sh: torch.empty(*sh, dtype=x.dtype, device=DEV)
    h = x.to(DEV)
    if we is not None:
        z = Fn.conv_forward(h, Fn.ConvSpec(cin, cin, mid, 1, 1), Fn.pointwise_pack(we.to(DEV), x.dtype), we.to(DEV), e(N, H, W, mid))
        h = Fn.bn_inference(z, *d(bn1), EPS, e(N, H, W, mid), True, act_max=6.0)
    z = Fn.dwconv_forward(h, wd.to(DEV), e(N, P, Q, mid), s, Fn.same_pads(H, 3, s)[0], Fn.same_pads(W, 3, s)[0])
    h = Fn.bn_inference(z, *d(bn2), EPS, e(N, P, Q, mid), True, act_max=6.0)
    z = Fn.conv_forward(h, Fn.ConvSpec(mid, mid, cout, 1, 1), Fn.pointwise_pack(wp.to(DEV), x.dtype), wp.to(DEV), e(N, P, Q, cout))
    return Fn.bn_inference(z, *d(bn3), EPS, e(N, P, Q, cout), False, residual=res.to(DEV) if res is not None else None)


@pytest.fixture(params=list(DTYPES))
def precision(request):
    set_gpu_compute_dtype(DTYPES[request.param])
    yield request.param
    set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mbconv_block_output(precision, shape):
    args = inputs(shape, DTYPES[precision])
    ref = reference(*args)
    ek, ec = rel_err(run_kernel(*args), ref), rel_err(run_chain(*args), ref)
    print(f"{precision} {shape}: kernel {ek:.3e}, unfused chain {ec:.3e} (bound {BOUND[precision]:.2e})")
    assert ek < BOUND[precision]


def _refusal_args(case):
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=DEV)
    a = dict(x=z(1, 8, 8, 16), cin=16, t=6, mid=96, cout=16, s=1, res=z(1, 8, 8, 16), out=z(1, 8, 8, 16))
    big = lambda: torch.empty(8192, 1024, 8, 16, dtype=torch.bfloat16, device=DEV)  # exactly 2^31 bytes, never touched
    a.update({
        "channels": lambda: dict(x=z(1, 8, 8, 12), cin=12, mid=72, res=None),
        "mid": lambda: dict(mid=104),
        "stride": lambda: dict(s=3, res=None, out=z(1, 3, 3, 16)),
        "ld": lambda: dict(x=z(1, 8, 8, 20)[..., :16]),
        "rows": lambda: dict(x=z(1, 16, 8, 16)[:, ::2]),
        "dtype": lambda: dict(out=z(1, 8, 8, 16, dt=torch.float16)),
        "fp32": lambda: dict(x=z(1, 8, 8, 16, dt=torch.float32)),
        "planes": lambda: dict(x=Fn.Planes(z(3, 1, 8, 8, 16))),
        "alias": lambda: dict(out=a["x"]),
        "alias_res": lambda: dict(out=a["res"]),
        "res_stride": lambda: dict(s=2, out=z(1, 4, 4, 16), res=z(1, 4, 4, 16)),
        "res_cout": lambda: dict(cout=24, out=z(1, 8, 8, 24), res=z(1, 8, 8, 24)),
        "fit": lambda: dict(x=z(1, 4, 256, 16), res=None, out=z(1, 4, 256, 16)),
        "2gib": lambda: (lambda x: dict(x=x, res=x, out=big()))(big()),
    }[case]())
    return a


@pytest.mark.parametrize("case,msg", [
    ("channels", "channels must be multiples of 8"), ("mid", "mid must be t \\* cin"), ("stride", "stride must be 1 or 2"),
    ("ld", "ld must be a multiple of 8"), ("rows", "non-contiguous rows"), ("dtype", "dtypes differ"),
    ("fp32", "float32 tensors are not taken"), ("planes", "not Planes"), ("alias", "out aliases x"),
    ("alias_res", "out aliases res"), ("res_stride", "only with stride 1 and cin == cout"),
    ("res_cout", "only with stride 1 and cin == cout"), ("fit", "does not fit"), ("2gib", "below 2 GiB")])
def test_mbconv_block_refusals(case, msg):
    a = _refusal_args(case)
    cin, mid, cout = a["cin"], a["mid"], a["cout"]
    v1, v3 = [torch.ones(mid, device=DEV)] * 4, [torch.ones(cout, device=DEV)] * 4
    Fn.set_f32_native(case == "fp32")
    try:
        with pytest.raises(RuntimeError, match=msg):
            Fn.mbconv_block_inference(a["x"], torch.zeros(mid, 1, 1, cin, device=DEV), v1, EPS,
                                      torch.zeros(mid, 3, 3, device=DEV), v1, EPS, torch.zeros(cout, 1, 1, mid, device=DEV),
                                      v3, EPS, a["out"], a["s"], res=a["res"])
    finally:
        Fn.set_f32_native(False)


def test_graph_replay_sees_changed_bn_vectors(precision):
    shape = (2, 8, 12, 16, 24, 6, 2)
    x, we, bn1, wd, bn2, wp, bn3, s, res = inputs(shape, DTYPES[precision], seed=2)
    d = lambda bn: [v.to(DEV) for v in bn]
    x, we, wd, wp, bn1, bn2, bn3 = x.to(DEV), we.to(DEV), wd.to(DEV), wp.to(DEV), d(bn1), d(bn2), d(bn3)
    run = lambda o: Fn.mbconv_block_inference(x, we, bn1, EPS, wd, bn2, EPS, wp, bn3, EPS, o, s)
    out = torch.empty(2, 4, 6, 24, dtype=x.dtype, device=DEV)
    run(out)  # (warm-up outside the capture)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(out)
    before = out.clone()
    bn1[0].mul_(1.5), bn2[2].add_(0.25), bn3[1].sub_(0.5)
    eager = run(torch.empty_like(out)).clone()
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "a replay must compute with the BN vectors as they are now"
    assert not torch.equal(eager, before)


def _spy(monkeypatch, name):
    f = getattr(Fn, name)

    def g(*a, **k):
        g.n += 1
        return f(*a, **k)
    g.n = 0
    monkeypatch.setattr(Fn, name, g)
    return g


def test_model_forward_only_one_launch_blocks(monkeypatch, precision):
    default = L.FUSE_MBCONV_BLOCK
    try:
        logits, calls = {}, {}
        for on in (True, False):
            L.FUSE_MBCONV_BLOCK = on
            spies = [_spy(monkeypatch, n) for n in ("mbconv_block_inference", "bn_inference", "dwconv_forward")]
            m = create_model("mobilenet", device="cuda", compute_dtype=precision, seed=11, **SMALL)
            img, lab = synthetic_batch(m, 4, seed=4)
            for l in m.layers:  # non-trivial moving statistics
                if hasattr(l, "rmean"):
                    l.rmean.data.copy_(0.1 * torch.sin(torch.arange(l.rmean.data.numel(), device=DEV).float()))
                    l.rvar.data.copy_(1.0 + 0.5 * torch.cos(torch.arange(l.rvar.data.numel(), device=DEV).float()))
            tr = Trainer(m, 4, constant_lr(0.0), forward_only=True, use_graph=False)
            tr.step(img.to(DEV, m.act_dtype), lab.cuda())
            logits[on], calls[on] = tr.logits.double().cpu(), [sp.n for sp in spies]
            monkeypatch.undo()
        # on: one block op per bottleneck, bn_inference only for the stem and conv_last; off: + 2 expand and 3 depthwise BNs
        assert calls[True] == [3, 2, 0] and calls[False] == [0, 7, 3], calls
        assert rel_err(logits[True], logits[False]) < BOUND[precision]
        L.FUSE_MBCONV_BLOCK = True
        sp = _spy(monkeypatch, "mbconv_block_inference")
        m = create_model("mobilenet", device="cuda", compute_dtype=precision, seed=11, **SMALL)
        img, lab = synthetic_batch(m, 4, seed=4)
        Trainer(m, 4, constant_lr(0.01), use_graph=False).step(img.to(DEV, m.act_dtype), lab.cuda())
        torch.cuda.synchronize()
        assert sp.n == 0, "a training step never takes the inference block"
    finally:
        L.FUSE_MBCONV_BLOCK = default
        set_gpu_compute_dtype(torch.bfloat16)
