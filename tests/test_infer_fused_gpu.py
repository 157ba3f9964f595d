"""Inference conv + BN fused into the GEMM epilogue (``Fn.conv_bn_inference``, the INF kernel
instantiations of csrc/kernels/igemm_epilogue.h; ``nn.layers.FUSE_INFER_BN``): the op against an fp64
reference and against the unfused chain (conv_forward + bn_inference) at fp32 (Planes / fp32 output)
and in both 16-bit builds, on every cfg the op accepts; exact write extents into a concat window; live
moving statistics under graph replay; what a forward-only step launches; fused against unfused models."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.nn import layers as L
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.nn.params import ParamStore
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.ops.functional import ConvSpec
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5

# (cin, cout, kh, kw, stride, (ph, pw), H, N)
CASES = {
    "1x1_m784": (64, 256, 1, 1, 1, (0, 0), 14, 4),      # M = 784: a row tail against 128 / 256-row tiles
    "3x3_k720": (80, 96, 3, 3, 1, (1, 1), 9, 4),        # K = 720, 96 columns against 64 / 128-wide tiles
    "3x3_s2": (128, 128, 3, 3, 2, (1, 1), 14, 4),       # strided 3x3
    "1x1_n40": (256, 40, 1, 1, 1, (0, 0), 23, 5),       # 40 columns, M = 2645
    "1x7": (64, 64, 1, 7, 1, (0, 3), 17, 2),            # an Inception class
}
P3_CFGS = list(range(18))    # every cfg hcb.conv_p3_inf accepts
A16_CFGS = list(range(17))   # every cfg hcb.conv_igemm_inf accepts


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


@pytest.fixture
def restore_modes():
    fuse = L.FUSE_INFER_BN
    yield
    L.FUSE_INFER_BN = fuse
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def _problem(case, dtype):
    """The conv, its weight pack for ``dtype`` (fp32: hi / mid / lo planes), an input, a residual and
    non-trivial BN parameters; 16-bit dtypes: x / residual rounded to the type."""
    cin, cout, kh, kw, s, (ph, pw), H, N = CASES[case]
    spec = ConvSpec(cin=cin, cin_pad=cin, cout=cout, kh=kh, kw=kw, sh=s, sw=s, pt=ph, pl=pw, pb=ph, pr=pw)
    ps = ParamStore(seed=5)
    p = ps.add("w", (cout, kh, kw, cin), True, ps.variance_scaling(kh * kw * cin))
    pk = ps.add_pack(p, cout, kh, kw, cin, spec.Kpad, spec.Kpad_t, want_tr=False)
    if dtype == torch.float32:
        ps.finalize(DEV, dtype_pack=torch.bfloat16, pack_lo=True)
    else:
        ps.finalize(DEV, dtype_pack=dtype)
    ps.repack()
    g = torch.Generator().manual_seed(7)
    P, Q = spec.out_hw(H, H)
    x = torch.randn(N, H, H, cin, generator=g).to(dtype).to(DEV)
    res = torch.randn(N, P, Q, cout, generator=g).to(dtype).to(DEV)
    bn = dict(gamma=(1 + 0.2 * torch.randn(cout, generator=g)).to(DEV), beta=(0.2 * torch.randn(cout, generator=g)).to(DEV),
              mean=(0.1 * torch.randn(cout, generator=g)).to(DEV), var=(torch.rand(cout, generator=g) * 1.5 + 0.5).to(DEV))
    w = p.data if dtype == torch.float32 else p.data.to(dtype)
    # fp64 reference of the same (rounded) operands: gamma * (conv - mean) / sqrt(var + eps) + beta
    conv = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(0, 3, 1, 2), stride=s,
                    padding=(ph, pw)).permute(0, 2, 3, 1)
    b = {k: v.double().cpu() for k, v in bn.items()}
    pre = b["gamma"] * (conv - b["mean"]) / torch.sqrt(b["var"] + EPS) + b["beta"]
    return spec, p, pk, x, res, bn, pre, ps


def _ref(pre, res, relu, with_res):
    r = pre + res.double().cpu() if with_res else pre
    return torch.relu(r) if relu else r


def _args(bn):
    return bn["gamma"], bn["beta"], bn["mean"], bn["var"], EPS


# ------------------------------------------------------------------ 1. the fp32 op against fp64
@pytest.mark.parametrize("case", list(CASES))
def test_fp32_op_matches_fp64_on_every_cfg(fp32_mode, case):
    """Fused error <= max(3e-6, 1.5 x the unfused chain's) -- 3e-6 is the plane-GEMM bound, the 1.5 the
    one extra fma rounding per element -- for Planes output with / without a Planes residual and fp32
    output with / without an fp32 residual, with and without ReLU."""
    spec, p, pk, x, res, bn, pre, _ = _problem(case, torch.float32)
    N, H = x.shape[0], x.shape[1]
    P, Q = spec.out_hw(H, H)
    shape = (N, P, Q, spec.cout)
    xp, resp = Fn.to_planes(x), Fn.to_planes(res)
    cfgs = [None] + P3_CFGS + [19, 22]  # 19 / 22: persistent cfgs, run as their per-tile twins 14 / 7
    if case == "3x3_k720":
        cfgs += [(0, 2), (7, 2), (13, 3)]
    worst = (0.0, 0.0)
    for planes_out in (True, False):
        for with_res in (False, True):
            for relu in (False, True):
                ref = _ref(pre, res, relu, with_res)
                r = (resp if planes_out else res) if with_res else None
                new = (lambda: Fn.Planes.empty(shape, DEV)) if planes_out else (
                    lambda: torch.empty(shape, dtype=torch.float32, device=DEV))
                z = torch.empty(shape, dtype=torch.float32, device=DEV)
                Fn.conv_forward(xp, spec, pk.pack, p.data, z)
                e_unf = rel_err(Fn.from_planes(Fn.bn_inference(z, *_args(bn), new(), relu, residual=r)), ref)
                for cfg in cfgs:
                    out = Fn.conv_bn_inference(xp, spec, pk.pack, p.data, *_args(bn), new(), relu, residual=r, cfg=cfg)
                    e = rel_err(Fn.from_planes(out), ref)
                    worst = max(worst, (e, e_unf))
                    assert e <= max(3e-6, 1.5 * e_unf), (cfg, planes_out, with_res, relu, e, e_unf)
    print(f"fp32 {case}: worst fused rel err {worst[0]:.3e} (unfused chain {worst[1]:.3e})")


# ------------------------------------------------------------------ 2. the 16-bit op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", ["1x1_m784", "3x3_k720", "3x3_s2"])
def test_16bit_op_matches_fp64_on_every_cfg(restore_modes, case, dtype):
    """fp64 reference from the 16-bit-rounded operands; fused error <= max(1e-2, the unfused chain's):
    the fused form rounds once where the unfused rounds z and y."""
    set_gpu_compute_dtype(dtype)
    spec, p, pk, x, res, bn, pre, _ = _problem(case, dtype)
    assert pk.pack.dtype == dtype
    N, H = x.shape[0], x.shape[1]
    P, Q = spec.out_hw(H, H)
    shape = (N, P, Q, spec.cout)
    cfgs = [None] + A16_CFGS + [17, 20]  # 17 / 20: 3x3 patch cfgs, run as their LDS-DMA twins 13 / 5
    if case == "3x3_k720":
        cfgs += [(4, 2), (13, 2), (6, 3)]
    worst = (0.0, 0.0)
    for with_res in (False, True):
        for relu in (False, True):
            ref = _ref(pre, res, relu, with_res)
            r = res if with_res else None
            z = torch.empty(shape, dtype=dtype, device=DEV)
            Fn.conv_forward(x, spec, pk.pack, p.data, z)
            e_unf = rel_err(Fn.bn_inference(z, *_args(bn), torch.empty_like(z), relu, residual=r), ref)
            for cfg in cfgs:
                out = Fn.conv_bn_inference(x, spec, pk.pack, p.data, *_args(bn), torch.empty(shape, dtype=dtype, device=DEV),
                                           relu, residual=r, cfg=cfg)
                e = rel_err(out, ref)
                worst = max(worst, (e, e_unf))
                assert e <= max(1e-2, 1.0 * e_unf), (cfg, with_res, relu, e, e_unf)
    print(f"{dtype} {case}: worst fused rel err {worst[0]:.3e} (unfused chain {worst[1]:.3e})")


# ------------------------------------------------------------------ 3. write extents
SENTINEL = 0x7FC1  # a bf16 / fp16 NaN bit pattern no kernel output carries


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_window_fully_written_and_nothing_else_touched(restore_modes, mode):
    """out = the 96-channel window at channel 32 of a 160-channel buffer with two guard rows after the
    last pixel, pre-filled with a NaN bit pattern: no sentinel left in the window, every other element
    (all three planes on the fp32 path) bitwise untouched."""
    f32 = mode == "fp32"
    if f32:
        set_gpu_compute_dtype(torch.float32)
        Fn.set_f32_native(True)
    dtype = torch.float32 if f32 else torch.bfloat16
    spec, p, pk, x, res, bn, pre, _ = _problem("3x3_k720", dtype)
    N, H = x.shape[0], x.shape[1]
    P, Q = spec.out_hw(H, H)
    M, C, W0, WIDE = N * P * Q, spec.cout, 32, 160
    lead = (3,) if f32 else ()
    for cfg in (None, 1, 10, (7, 2)) if f32 else (None, 2, 15, (13, 2)):
        buf = torch.empty(lead + (M + 2, WIDE), dtype=torch.bfloat16, device=DEV)
        bits = buf.view(torch.int16)
        bits.fill_(SENTINEL)
        body = buf[..., :M, :].view(lead + (N, P, Q, WIDE))
        out = (Fn.Planes(body) if f32 else body)[..., W0:W0 + C]
        x_in = Fn.to_planes(x) if f32 else x
        Fn.conv_bn_inference(x_in, spec, pk.pack, p.data, *_args(bn), out, True, cfg=cfg)
        torch.cuda.synchronize()
        win = torch.zeros(WIDE, dtype=torch.bool, device=DEV)
        win[W0:W0 + C] = True
        rows = torch.zeros(M + 2, dtype=torch.bool, device=DEV)
        rows[:M] = True
        inside = (rows[:, None] & win[None, :]).expand(bits.shape)
        assert not (bits[inside] == SENTINEL).any(), cfg
        assert (bits[~inside] == SENTINEL).all(), cfg
        assert rel_err(Fn.from_planes(out) if f32 else out, _ref(pre, res, True, False)) < (3e-6 if f32 else 1e-2)


# ------------------------------------------------------------------ models
def _bn_layers(m):
    todo, out = list(m.all_layers()), []
    while todo:
        l = todo.pop()
        if hasattr(l, "layers") and callable(l.layers):
            todo += l.layers()
        if hasattr(l, "rmean") and hasattr(l, "rvar"):
            out.append(l)
    return out


def _model(name, size, dtype, seed=11):
    m = create_model(name, device=DEV, compute_dtype=dtype, image_size=size, seed=seed, image_channels=8)
    assert m.native
    g = torch.Generator().manual_seed(5)
    for l in _bn_layers(m):
        l.rmean.data.copy_(torch.randn(l.rmean.data.shape, generator=g) * 0.1)
        l.rvar.data.copy_(torch.rand(l.rvar.data.shape, generator=g) * 1.5 + 0.5)
    return m


def _batch(m, n):
    img, lab = synthetic_batch(m, n, seed=3)
    img = img.float()
    img[..., :3] = (img[..., :3] - 127.0) / 60.0
    return img.to(m.act_dtype), lab


def _logits(t):
    torch.cuda.synchronize()
    return Fn.from_planes(t.logits).float().clone()


# ------------------------------------------------------------------ 4. live statistics under replay
def test_graph_replay_sees_moving_statistics_changed_after_capture(restore_modes):
    m = _model("resnet50", 64, "fp32")
    img, lab = _batch(m, 4)
    t = Trainer(m, 4, constant_lr(0.0), forward_only=True, use_graph=True, graph_warmup=1)
    t.step(img, lab)  # eager warm-up
    t.step(img, lab)  # capture + replay
    assert t._g_all is not None, "the forward-only step was not graph-captured"
    first = _logits(t)
    layer = m.blocks[2].c2
    layer.rmean.data.add_(0.5)  # in place: the captured kernels read this tensor
    t.step(img, lab)  # replay
    second = _logits(t)
    te = Trainer(m, 4, constant_lr(0.0), forward_only=True, use_graph=False)
    te.step(img, lab)
    eager = _logits(te)
    assert torch.equal(second, eager)
    assert not torch.equal(second, first)


# ------------------------------------------------------------------ 5. what the step launches
def _count_step(monkeypatch, name, size, dtype):
    m = _model(name, size, dtype)
    img, lab = _batch(m, 2)
    calls = {"bn_inference": 0, "to_planes_act": 0}
    bn_inf, to_pl = Fn.bn_inference, Fn.to_planes

    def bn_wrapped(*a, **k):
        calls["bn_inference"] += 1
        return bn_inf(*a, **k)

    def tp_wrapped(a):
        if not Fn.is_planes(a) and a is not img:  # (the input image is not an activation)
            calls["to_planes_act"] += 1
        return to_pl(a)

    monkeypatch.setattr(Fn, "bn_inference", bn_wrapped)
    monkeypatch.setattr(Fn, "to_planes", tp_wrapped)
    t = Trainer(m, 2, constant_lr(0.0), forward_only=True, use_graph=False)
    t.step(img, lab)
    torch.cuda.synchronize()
    assert torch.isfinite(Fn.from_planes(t.logits).float()).all()
    n_bnrelu = sum(isinstance(l, L.BNReLU) for l in _bn_layers(m))
    return calls, n_bnrelu


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,size", [("resnet50", 64), ("inception3", 75), ("resnet50_v2", 64)])
def test_forward_only_step_contains_no_bn_pass(restore_modes, monkeypatch, name, size, dtype):
    L.FUSE_INFER_BN = True
    calls, n_bnrelu = _count_step(monkeypatch, name, size, dtype)
    if name == "resnet50_v2":  # the pre-activation BNs have no producing GEMM: they keep bn_inference
        assert n_bnrelu > 0 and calls["bn_inference"] == n_bnrelu
        return
    assert calls["bn_inference"] == 0
    if dtype == "fp32":
        assert calls["to_planes_act"] == 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_switch_off_restores_the_bn_passes(restore_modes, monkeypatch, dtype):
    L.FUSE_INFER_BN = False
    calls, _ = _count_step(monkeypatch, "resnet50", 64, dtype)
    assert calls["bn_inference"] > 0
    if dtype == "fp32":
        assert calls["to_planes_act"] > 0


# ------------------------------------------------------------------ 6. / 7. fused against unfused
def _fused_vs_unfused(name, size, dtype, batch):
    m = _model(name, size, dtype)
    stats = [(l.rmean.data.clone(), l.rvar.data.clone()) for l in _bn_layers(m)]
    img, lab = _batch(m, batch)
    out = {}
    for on in (True, False):
        L.FUSE_INFER_BN = on
        t = Trainer(m, batch, constant_lr(0.0), forward_only=True, use_graph=False)
        t.step(img, lab)
        out[on] = _logits(t)
    rel = ((out[True] - out[False]).norm() / out[False].norm()).item()
    print(f"{name} {dtype}: fused vs unfused logits rel err {rel:.3e}")
    assert torch.isfinite(out[True]).all() and out[False].norm() > 0
    assert rel < (1e-4 if dtype == "fp32" else 5e-2), rel
    for l, (a, b) in zip(_bn_layers(m), stats):
        assert torch.equal(l.rmean.data, a) and torch.equal(l.rvar.data, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,size", [("resnet50", 64), ("inception3", 75)])
def test_fused_logits_match_unfused(restore_modes, name, size, dtype):
    _fused_vs_unfused(name, size, dtype, 4)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stem_s2d_inference_fused_matches_unfused(restore_modes, dtype):
    m = _model("resnet50", 64, dtype)
    assert isinstance(m.stem, L.StemS2D)
    m.set_training(False)
    m.activate() if hasattr(m, "activate") else None
    img, _ = _batch(m, 2)
    out = {}
    for on in (True, False):
        L.FUSE_INFER_BN = on
        y = m.stem.forward(img)
        torch.cuda.synchronize()
        assert Fn.is_planes(y) == (on and dtype == "fp32")
        out[on] = Fn.from_planes(y).float()
    rel = rel_err(out[True], out[False])
    assert out[False].norm() > 0 and rel < (1e-4 if dtype == "fp32" else 5e-2), rel
