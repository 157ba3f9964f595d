"""The plan-A shortcut kernels (csrc/kernels/shortcut.hip: ``shortcut_pad_fwd`` / ``shortcut_pad_bwd``)
against a torch construction -- ``x[:, ::s, ::s]`` + ``F.pad`` on the channels, and its adjoint -- BITWISE:
both are copies. Every format a residual arrives in (16-bit of either kernel library, plain fp32, the
fp32 path's Planes) forward, the two plain activation types backward; N = 3 with H = W = 7 (odd: P = 4,
and 3 * 4 * 4 * K / 8 vectors are no multiple of the 256-thread block) and 8; both strides; 16 -> 32,
32 -> 64 and 8 -> 24. Outputs are pre-filled with NaN: the kernels write every element themselves."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.nn.layers import PadShortcut, set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

SHAPES = [(H, s, C, K) for H in (7, 8) for s in (1, 2) for C, K in ((16, 32), (32, 64), (8, 24))]


def _reset():
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def _activate(dtype):
    set_gpu_compute_dtype(dtype)
    Fn.set_f32_native(dtype == torch.float32)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _fwd_ref(x, s, K):
    pad = (K - x.shape[-1]) // 2
    return F.pad(x[:, ::s, ::s], (pad, pad))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_forward_plain_tensor_is_bitwise(dtype):
    try:
        _activate(dtype)
        g = torch.Generator().manual_seed(0)
        for H, s, C, K in SHAPES:
            x = torch.randn((3, H, H, C), generator=g).to("cuda", dtype)
            P = -(-H // s)
            y = torch.full((3, P, P, K), float("nan"), dtype=dtype, device="cuda")
            assert Fn.native(x)
            Fn.shortcut_pad_forward(x, y, s)
            torch.cuda.synchronize()
            assert torch.equal(_bits(y), _bits(_fwd_ref(x, s, K))), (H, s, C, K)
    finally:
        _reset()


def test_forward_planes_is_bitwise_per_plane():
    try:
        _activate(torch.float32)
        g = torch.Generator().manual_seed(1)
        for H, s, C, K in SHAPES:
            x = Fn.to_planes(torch.randn((3, H, H, C), generator=g).cuda())
            layer = PadShortcut("sc", (H, H, C), K, s)
            y = layer.forward(x)
            torch.cuda.synchronize()
            assert Fn.is_planes(y) and tuple(y.shape) == (3,) + layer.out_shape
            for t in range(3):
                assert torch.equal(_bits(y.t[t]), _bits(_fwd_ref(x.t[t], s, K))), (H, s, C, K, t)
            # (hence the fp32 value: subsampling and zero padding commute with the hi / mid / lo split)
            assert torch.equal(y.float(), _fwd_ref(x.float(), s, K))
    finally:
        _reset()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_backward_is_bitwise_and_writes_every_element(dtype):
    try:
        _activate(dtype)
        gen = torch.Generator().manual_seed(2)
        for H, s, C, K in SHAPES:
            P = -(-H // s)
            pad = (K - C) // 2
            g = torch.randn((3, P, P, K), generator=gen).to("cuda", dtype)
            dx = torch.full((3, H, H, C), float("nan"), dtype=dtype, device="cuda")
            Fn.shortcut_pad_backward(g, dx, s)
            torch.cuda.synchronize()
            want = torch.zeros((3, H, H, C), dtype=dtype, device="cuda")
            want[:, ::s, ::s] = g[..., pad:pad + C]
            assert torch.equal(_bits(dx), _bits(want)), (H, s, C, K)
            # the adjoint of the forward: <fwd(x), g> == <x, bwd(g)> in float64
            x = torch.randn((3, H, H, C), generator=gen).to("cuda", dtype)
            lhs = (_fwd_ref(x, s, K).double() * g.double()).sum()
            assert float((lhs - (x.double() * dx.double()).sum()).abs()) <= 1e-9 * float(lhs.abs() + 1)
    finally:
        _reset()


def test_binding_refuses_other_geometries_by_name():
    try:
        _activate(torch.bfloat16)
        op = _ext.ops()

        def t(*shape):
            return torch.zeros(shape, dtype=torch.bfloat16, device="cuda")

        with pytest.raises(RuntimeError, match="K - C must be even"):
            op.shortcut_pad_fwd(t(2, 8, 8, 8), t(2, 8, 8, 17), 1)
        with pytest.raises(RuntimeError, match="pad % 8 == 0"):
            op.shortcut_pad_fwd(t(2, 8, 8, 8), t(2, 8, 8, 16), 1)
        with pytest.raises(RuntimeError, match="pad % 8 == 0"):
            op.shortcut_pad_bwd(t(2, 4, 4, 16), t(2, 8, 8, 8), 2)
        with pytest.raises(RuntimeError, match="C % 8 == 0"):
            op.shortcut_pad_fwd(t(2, 8, 8, 4), t(2, 8, 8, 20), 1)
        with pytest.raises(RuntimeError, match="K - C must be even"):
            op.shortcut_pad_fwd(t(2, 8, 8, 32), t(2, 8, 8, 16), 1)
        with pytest.raises(RuntimeError, match="stride 1 or 2"):
            op.shortcut_pad_fwd(t(2, 9, 9, 16), t(2, 3, 3, 32), 3)
        with pytest.raises(RuntimeError, match=r"ceil\(H / s\)"):
            op.shortcut_pad_fwd(t(2, 7, 7, 16), t(2, 3, 3, 32), 2)
        with pytest.raises(RuntimeError, match="contiguous"):
            op.shortcut_pad_fwd(t(2, 8, 8, 32)[..., :16], t(2, 8, 8, 32), 1)
        with pytest.raises(RuntimeError, match="one dtype"):
            op.shortcut_pad_fwd(t(2, 8, 8, 16), t(2, 8, 8, 32).float(), 1)
        torch.cuda.synchronize()
    finally:
        _reset()
