"""The fused pre-activation conv of the CIFAR ResNet-v2 block (csrc/kernels/preact3x3.hip) through
Fn.preact_conv3x3_forward against the definition in fp64 on the CPU: BN -> ReLU -> conv 3x3 'SAME' (TF's
asymmetric pads at stride 2) into a tensor of its own. Bounds are those of tests/test_dense3x3_gpu.py: output
3e-6 (fp32) / 1e-2 (16-bit), statistics 1e-5 / 2e-2, saved moments 1e-5, all norm-relative. The model tests hold
FUSE_PREACT on against off at the fp32 step bounds of tests/test_densenet_gpu.py (loss 1e-4 relative, gradient
cosine > 0.9999)."""
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
EPS = 1e-5
R = 8
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
TOL = {"bf16": (1e-2, 2e-2), "fp16": (1e-2, 2e-2), "fp32": (3e-6, 1e-5)}  # (output, statistics)
SHAPES = [  # (N, H, W, C_in, Nout, stride)
    (2, 8, 8, 16, 16, 1),    # half a 32-channel chunk; strip = part of an image
    (2, 6, 8, 64, 64, 1),    # two chunks, four column tiles, H != W
    (1, 32, 32, 16, 32, 1),  # many strips; halo rows shared between strips
    (2, 12, 16, 32, 64, 2),  # stride 2 with asymmetric pad; short last strip
    (3, 8, 8, 64, 16, 2),    # 4 x 4 output; N not a power of two
]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def reference(xd, w, gamma, beta, mean, var, s):
    """The definition in fp64: conv3x3 'SAME' (stride s) of the zero-padded relu(bn(x)); NHWC in and out."""
    a = torch.relu((xd - mean) * torch.rsqrt(var + EPS) * gamma.double() + beta.double())
    (pt, pb), (pl, pr) = Fn.same_pads(xd.shape[1], 3, s), Fn.same_pads(xd.shape[2], 3, s)
    a = F.pad(a.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(a, w.double().permute(0, 3, 1, 2), stride=s).permute(0, 2, 3, 1)


def inputs(shape, dt, seed=1):
    N, H, W, C, nout, s = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g)
    x[..., 1] += 50.0                      # |mean| = 50 std
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[3] = -8.0                         # entirely negative after BN: all masked by the ReLU
    w = torch.randn(nout, 3, 3, C, generator=g) * math.sqrt(2.0 / 9 / nout)
    return x.to(dt), gamma, beta, w, g


@pytest.fixture(params=list(DTYPES))
def precision(request):
    dt = DTYPES[request.param]
    set_gpu_compute_dtype(dt)
    Fn.set_f32_native(dt == torch.float32)
    yield request.param
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_preact_conv3x3_forward(precision, shape):
    N, H, W, C, nout, s = shape
    dt = DTYPES[precision]
    x, gamma, beta, w, g = inputs(shape, dt)
    xd = x.double()
    M = N * H * W
    mean, var = xd.mean((0, 1, 2)), xd.var((0, 1, 2), unbiased=False)
    ref = reference(xd, w, gamma, beta, mean, var, s)
    P, Q = ref.shape[1:3]

    shift = (mean + 0.1 * var.sqrt()).float()  # x's statistics as bn_stats_acc leaves them: shifted, over R replicas
    dx = xd.reshape(M, C) - shift.double()
    acc = torch.zeros(R, 2, C)
    acc[:, 0], acc[:, 1] = (dx.sum(0) / R).float(), ((dx * dx).sum(0) / R).float()
    kout = 0.1 * torch.randn(nout, generator=g)
    out = torch.full((N, P, Q, nout + 8), 7.0).to(dt).to(DEV)  # a row stride larger than Nout, sentinel in the gap
    stats = torch.zeros(R, 2, nout, device=DEV)
    saved = Fn.preact_conv3x3_forward(x.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV), EPS, out[..., :nout], s,
                                      acc=acc.to(DEV), R=R, shift=shift.to(DEV), out_stats=stats, out_stats_R=R,
                                      out_stats_shift=kout.to(DEV))
    torch.cuda.synchronize()

    tol_y, tol_s = TOL[precision]
    e = rel_err(out[..., :nout], ref)
    em, ei = rel_err(saved.mean, mean), rel_err(saved.invstd, torch.rsqrt(var + EPS))
    d = ref.reshape(-1, nout) - kout.double()
    st = stats.double().sum(0).cpu()
    e1, e2 = rel_err(st[0], d.sum(0)), rel_err(st[1], (d * d).sum(0))
    print(f"{precision} {shape}: output {e:.3e} (bound {tol_y}), moments {em:.3e} {ei:.3e} (1e-5), "
          f"statistics {e1:.3e} {e2:.3e} (bound {tol_s})")
    assert e < tol_y
    assert bool((out[..., nout:] == 7.0).all()), "the gap of y's rows is not the kernel's to write"
    assert em < 1e-5 and ei < 1e-5
    assert e1 < tol_s and e2 < tol_s


def test_preact_conv3x3_inference(precision):
    shape = (2, 12, 16, 32, 64, 2)
    x, gamma, beta, w, g = inputs(shape, DTYPES[precision], seed=2)
    mean, var = torch.randn(32, generator=g), 0.5 + torch.rand(32, generator=g)
    mean[1] += 50.0
    ref = reference(x.double(), w, gamma, beta, mean.double(), var.double(), 2)
    out = torch.empty(ref.shape, dtype=x.dtype, device=DEV)
    rm, rv = mean.to(DEV), var.to(DEV)
    assert Fn.preact_conv3x3_forward(x.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV), EPS, out, 2, running_mean=rm,
                                     running_var=rv) is None
    assert torch.equal(rm.cpu(), mean) and torch.equal(rv.cpu(), var)
    assert rel_err(out, ref) < TOL[precision][0]


def test_preact_conv3x3_deterministic_is_bitwise(precision):
    shape = (3, 8, 8, 64, 16, 2)  # 3 strips on det_replicas(48) = 1 replica: the capped grid strides
    N, H, W, C, nout, s = shape
    x, gamma, beta, w, _ = inputs(shape, DTYPES[precision], seed=3)
    xd = x.double().reshape(-1, C)
    Rd = Fn.det_replicas(N * 4 * 4)
    acc = torch.zeros(1, 2, C)
    acc[0, 0], acc[0, 1] = xd.sum(0).float(), (xd * xd).sum(0).float()
    args = [t.to(DEV) for t in (x, w, gamma, beta)]
    runs = []
    Fn.set_deterministic(True)
    try:
        for _ in range(2):
            out, stats = torch.empty(N, 4, 4, nout, dtype=x.dtype, device=DEV), torch.zeros(Rd, 2, nout, device=DEV)
            Fn.preact_conv3x3_forward(*args, EPS, out, s, acc=acc.to(DEV), R=1, out_stats=stats, out_stats_R=Rd)
            runs.append((out.cpu(), stats.cpu()))
    finally:
        Fn.set_deterministic(False)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref = reference(x.double(), w, gamma, beta, xd.mean(0), xd.var(0, unbiased=False), s)
    assert rel_err(runs[0][0], ref) < TOL[precision][0]
    assert rel_err(runs[0][1].sum(0)[0], ref.reshape(-1, nout).sum(0)) < TOL[precision][1]


@pytest.mark.parametrize("c_in,nout,s,alias,msg", [
    (24, 16, 1, False, "C_in must be 16, 32 or 64"), (16, 48, 1, False, "Nout must be 16, 32 or 64"),
    (16, 16, 3, False, "stride must be 1 or 2"), (16, 16, 1, True, "y aliases x")])
def test_preact_conv3x3_refusals(c_in, nout, s, alias, msg):
    x = torch.zeros(1, 8, 8, c_in, dtype=torch.bfloat16, device=DEV)
    out = x if alias else torch.zeros(1, -(-8 // s), -(-8 // s), nout, dtype=torch.bfloat16, device=DEV)
    v = torch.ones(c_in, device=DEV)
    with pytest.raises(RuntimeError, match=msg):
        Fn.preact_conv3x3_forward(x, torch.zeros(nout, 3, 3, c_in, device=DEV), v, v, EPS, out, s,
                                  acc=torch.zeros(1, 2, c_in, device=DEV))


def _run_model(on, forward_only):
    L.FUSE_PREACT = on
    m = create_model("resnet20_v2", data_name="cifar10", device="cuda", compute_dtype="fp32", seed=5,
                     layer_counts=(1, 2, 1), image_size=16)
    img, lab = synthetic_batch(m, 4, seed=4)
    img = img.float()
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
    img, lab = img.to("cuda", m.act_dtype), lab.cuda()
    if forward_only:
        for l in m.all_layers():  # non-trivial moving statistics
            if hasattr(l, "rmean"):
                l.rmean.data.copy_(0.1 * torch.sin(torch.arange(l.rmean.data.numel(), device="cuda").float()))
                l.rvar.data.copy_(1.0 + 0.5 * torch.cos(torch.arange(l.rvar.data.numel(), device="cuda").float()))
        t = Trainer(m, 4, constant_lr(0.0), forward_only=True)
        t._forward(img, lab)
        torch.cuda.synchronize()
        return t.logits[:, :m.num_classes].double().cpu()
    t = Trainer(m, 4, constant_lr(0.0), weight_decay=0.0, use_graph=True)
    for _ in range(t.graph_warmup + 2):
        loss = float(t.step(img, lab))
    torch.cuda.synchronize()
    assert t._g_all is not None, "the step was not captured"
    return loss, torch.cat([p.grad.double().cpu().flatten() for p in m.ps.params])


@pytest.fixture
def model_switch():
    default = L.FUSE_PREACT
    yield
    L.FUSE_PREACT = default
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def test_model_captured_step_fused_matches_unfused(model_switch):
    (l1, g1), (l0, g0) = _run_model(True, False), _run_model(False, False)
    cos = float(g1 @ g0 / (g1.norm() * g0.norm()))
    print(f"loss fused {l1:.6f} unfused {l0:.6f}, gradient cosine {cos:.7f}")
    assert abs(l1 - l0) <= 1e-4 * abs(l0) and cos > 0.9999 and bool(torch.isfinite(g1).all())


def test_model_forward_only_fused_matches_unfused(model_switch):
    a, b = _run_model(True, True), _run_model(False, True)
    print(f"forward-only logits rel err {rel_err(a, b):.3e}")
    assert rel_err(a, b) < 1e-4
