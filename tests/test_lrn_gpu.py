"""The local response normalisation kernels (csrc/kernels/lrn.hip: ``lrn_fwd`` / ``lrn_bwd``) against
``Fn.lrn_forward`` / ``Fn.lrn_backward`` in fp64 on the CPU, computed from the exact, already-rounded inputs
the kernels got.

Bounds, the project's own (tests/test_dwconv_gpu.py). fp32 and Planes outputs: ||got - ref|| / ||ref|| < 3e-6.
16-bit outputs (bf16 library, fp16 through hcb16): an element may differ from the reference by one rounding
of the output, 2^-8 |ref| (bf16) or 2^-11 |ref| (fp16), plus 3e-6 * rms(ref).

Parameters: (bias 1, alpha 1, beta 0.75) and (bias 2, alpha 0.5, beta 0.5) on randn inputs put s at about
2 .. 26, where one dropped tap moves an output by 7-13 %: a wrong window cannot pass any of the bounds. The
model's alpha = 0.001 / 9 moves it by 1.4e-4 only, less than a bf16 rounding, so the model's parameters are an
additional fp32-only case. beta = 0.6 takes the kernels' general exp2 / log2 form.

Measured maxima on an MI355X: fp32 / Planes forward <= 8.1e-8 relative, backward <= 1.1e-7 (bound 3e-6), with
the model's parameters 5.3e-8 / 5.9e-8; bf16 excess over the one output rounding < 0 everywhere (5.6e-7 ..
8.8e-7 allowed); fp16 forward < 0, backward <= 8.8e-8 absolute where 1.2e-6 was allowed.
"""
import pytest
import torch

from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"

# N, H, W, C, r
SHAPES = [
    (1, 3, 5, 8, 4),    # the window is wider than C
    (2, 2, 3, 16, 2),
    (1, 3, 5, 72, 4),   # 9 lanes per pixel, 7 pixels per wave: pixels meet wave boundaries
    (3, 7, 7, 64, 4),   # the model's C; 147 pixels are no multiple of the 32 a block holds
    (1, 1, 1, 24, 1),
]
# bias, alpha, beta
PARAMS = [(1.0, 1.0, 0.75), (2.0, 0.5, 0.5)]
GENERAL_POW = (1.5, 0.7, 0.6)
MODEL_PARAMS = (1.0, 0.001 / 9.0, 0.75)
IDS = [f"n{s[0]}h{s[1]}w{s[2]}c{s[3]}r{s[4]}" for s in SHAPES]
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


_REF = {}


def problem(shape, prm, mode, seed=0):
    """(x, dy) on the GPU in the mode's dtype and the fp64 CPU reference (y, dx) of exactly those values;
    computed once per (shape, parameters, mode) and never modified."""
    key = (shape, prm, mode, seed)
    if key not in _REF:
        N, H, W, C, r = shape
        g = torch.Generator().manual_seed(seed + 17 * C + r)
        x = torch.randn(N, H, W, C, generator=g).to(DTYPES[mode])
        dy = torch.randn(N, H, W, C, generator=g).to(DTYPES[mode])
        x64, dy64 = x.double(), dy.double()
        y = Fn.lrn_forward(x64, torch.empty_like(x64), r, *prm)
        dx = Fn.lrn_backward(dy64, x64, torch.empty_like(x64), r, *prm)
        _REF[key] = (x.to(DEV), dy.to(DEV), y, dx)
    return _REF[key]


def check(name, got, ref, mode, mask=None):
    """``mask``: the elements compared (the others are checked by the caller)."""
    got, ref = Fn.from_planes(got).double().cpu(), ref.double()
    if mask is not None:
        got, ref = got[mask], ref[mask]
    assert bool(torch.isfinite(got).all()), f"{name}: an element was not written (NaN fill) or is not finite"
    rms = float(ref.norm()) / ref.numel() ** 0.5
    rel = float((got - ref).norm() / (ref.norm() + 1e-300))
    eps = EPS_OUT[mode]
    if eps == 0.0:
        print(f"{name} {mode}: rel {rel:.3e}")
        assert rel < 3e-6, (name, rel)
        return
    excess = float(((got - ref).abs() - eps * ref.abs()).max())
    print(f"{name} {mode}: rel {rel:.3e}, max excess over one rounding {excess:.3e} (allowed {3e-6 * rms:.3e})")
    assert excess <= 3e-6 * rms, (name, excess, 3e-6 * rms)


def nan_like(x, planes=False):
    if planes:
        return Fn.Planes(torch.full((3,) + tuple(x.shape), float("nan"), dtype=torch.bfloat16, device=DEV))
    return torch.full(tuple(x.shape), float("nan"), dtype=x.dtype, device=DEV)


def format_pairs(mode):
    """(x as Planes, out as Planes) of the forward; backward: x in each format the mode has."""
    return [(False, False), (False, True), (True, True)] if mode == "fp32" else [(False, False)]


def run_all(shape, prm, mode, x=None, dy=None):
    """Every forward format pair and every saved-x format of the backward: [(name, tensor)], outputs NaN-filled."""
    r = shape[4]
    if x is None:
        x, dy, _, _ = problem(shape, prm, mode)
    xp = Fn.to_planes(x) if mode == "fp32" else None
    fw, bw = [], []
    for xin, pout in format_pairs(mode):
        y = nan_like(x, planes=pout)
        Fn.lrn_forward(xp if xin else x, y, r, *prm)
        fw.append((f"fwd[{'planes' if xin else 'plain'}->{'planes' if pout else 'plain'}]", y))
    for xin in ([False, True] if mode == "fp32" else [False]):
        dx = nan_like(dy)
        Fn.lrn_backward(dy, xp if xin else x, dx, r, *prm)
        bw.append((f"bwd[x {'planes' if xin else 'plain'}]", dx))
    return fw, bw


@pytest.mark.parametrize("prm", PARAMS + [GENERAL_POW], ids=["b1a1beta.75", "b2a.5beta.5", "b1.5a.7beta.6"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lrn_forward_backward(shape, prm, mode):
    _, _, yr, dxr = problem(shape, prm, mode)
    fw, bw = run_all(shape, prm, mode)
    fw2, bw2 = run_all(shape, prm, mode)
    for (name, got), (_, again) in zip(fw, fw2):
        check(name, got, yr, mode)
        assert torch.equal(Fn._pl(got), Fn._pl(again)), f"{name}: two launches differ"
    for (name, got), (_, again) in zip(bw, bw2):
        check(name, got, dxr, mode)
        assert torch.equal(got, again), f"{name}: two launches differ"


def test_lrn_model_parameters_fp32():
    """alpha = 0.001 / 9 (the CIFAR-10 AlexNet's layers): fp32 only -- under a 16-bit rounding a wrong window
    would not show."""
    _ext.set_act("bf16")
    Fn.set_f32_native(True)
    try:
        for shape in (SHAPES[3], SHAPES[2]):
            _, _, yr, dxr = problem(shape, MODEL_PARAMS, "fp32")
            fw, bw = run_all(shape, MODEL_PARAMS, "fp32")
            for name, got in fw:
                check("model " + name, got, yr, "fp32")
            for name, got in bw:
                check("model " + name, got, dxr, "fp32")
            # the bound does see a dropped tap here: measured against the same reference with r - 1
            x, _, _, _ = problem(shape, MODEL_PARAMS, "fp32")
            x64 = x.double().cpu()
            y_short = Fn.lrn_forward(x64, torch.empty_like(x64), shape[4] - 1, *MODEL_PARAMS)
            assert float((y_short - yr).norm() / yr.norm()) > 3e-5
    finally:
        Fn.set_f32_native(False)


@pytest.mark.parametrize("shape,pixel", [(SHAPES[2], (0, 1, 1)), (SHAPES[2], (0, 1, 2)), (SHAPES[3], (1, 3, 3))],
                         ids=["c72-last-of-wave", "c72-first-of-wave", "c64"])
def test_lrn_nan_pixel_stays_in_its_pixel(shape, pixel, mode):
    """One interior pixel of x is NaN: exactly that pixel's outputs and dx are NaN, every other element meets
    the bound (a lane at a pixel's edge takes zeros, never its neighbour pixel's values). With C = 72 pixel 6
    is the last of the first wave and pixel 7 the first of the second."""
    prm = PARAMS[0]
    x0, dy, yr, dxr = problem(shape, prm, mode)
    x = x0.clone()
    x[pixel] = float("nan")
    keep = torch.ones(shape[:4], dtype=torch.bool)
    keep[pixel] = False
    fw, bw = run_all(shape, prm, mode, x=x, dy=dy)
    for name, got in fw + bw:
        full = Fn.from_planes(got).cpu()
        assert bool(torch.isnan(full[pixel]).all()), f"{name}: the NaN pixel's own elements must be NaN"
        check("nan " + name, got, dxr if name.startswith("bwd") else yr, mode, mask=keep)


def test_lrn_native_refusals(mode):
    """r = 5, C = 12 and a strided view are refused on the host, by name, before any launch -- by the Python
    wrapper and by the op itself."""
    dt = DTYPES[mode]
    ops = _ext.ops()

    def t(*s):
        return torch.zeros(*s, dtype=dt, device=DEV)

    x = t(1, 2, 2, 16)
    Fn.lrn_forward(x, t(1, 2, 2, 16), 4, 1.0, 1.0, 0.75)  # the well-formed call passes
    with pytest.raises(ValueError, match=r"r <= 4"):
        Fn.lrn_forward(x, t(1, 2, 2, 16), 5, 1.0, 1.0, 0.75)
    with pytest.raises(ValueError, match=r"C % 8"):
        Fn.lrn_forward(t(1, 2, 2, 12), t(1, 2, 2, 12), 2, 1.0, 1.0, 0.75)
    with pytest.raises(ValueError, match=r"contiguous"):
        Fn.lrn_forward(t(1, 2, 2, 32)[..., :16], t(1, 2, 2, 16), 2, 1.0, 1.0, 0.75)
    with pytest.raises(ValueError, match=r"dx must be contiguous"):
        Fn.lrn_backward(x, x, t(1, 2, 2, 32)[..., :16], 2, 1.0, 1.0, 0.75)
    with pytest.raises(ValueError, match=r"C <= 512"):
        Fn.lrn_forward(t(1, 1, 1, 520), t(1, 1, 1, 520), 2, 1.0, 1.0, 0.75)
    with pytest.raises(ValueError, match=r"bias"):
        Fn.lrn_backward(x, x, t(1, 2, 2, 16), 2, 0.0, 1.0, 0.75)
    for bad, word in (((x, t(1, 2, 2, 16), 5, 1.0, 1.0, 0.75), "r"),
                      ((t(1, 2, 2, 12), t(1, 2, 2, 12), 2, 1.0, 1.0, 0.75), "C"),
                      ((t(1, 2, 2, 32)[..., :16], t(1, 2, 2, 16), 2, 1.0, 1.0, 0.75), "contiguous"),
                      ((x, t(1, 2, 2, 16), 2, 0.0, 1.0, 0.75), "bias"),
                      ((x, t(1, 2, 2, 16), 2, 1.0, -1.0, 0.75), "alpha"),
                      ((x, t(1, 2, 3, 16), 2, 1.0, 1.0, 0.75), "shape"),
                      ((x, t(1, 2, 2, 16).to(torch.float32 if mode != "fp32" else torch.bfloat16), 2, 1.0, 1.0, 0.75),
                       "16-bit")):
        with pytest.raises(RuntimeError, match=word):
            ops.lrn_fwd(*bad)
    with pytest.raises(RuntimeError, match="plain activations"):
        ops.lrn_bwd(x, x, torch.zeros(3, 1, 2, 2, 16, dtype=torch.bfloat16, device=DEV), 2, 1.0, 1.0, 0.75)
    torch.cuda.synchronize()
