"""Elementwise checks of the pooling kernels (csrc/kernels/pool.hip) on every branch of their host
dispatch, against the fp64 loops of tests/pool_ref.py and nothing else. Maps are never square, max
pools run on tie-heavy post-ReLU-like inputs with integer gradients (every expected value is exact:
torch.equal on y, the argmax bytes and dx), averages within a derived bound (pool_ref.assert_within).

Kernel reached by each row of pool_ref.CASES (launch_pool_fwd / launch_pool_bwd, by reading):

    row                         forward                    backward with the argmax
    max_k3s2_same_6x10          pool_fwd_kernel            maxpool_bwd_amax_s2_kernel, ph = pw = 0
    max_k3s2_pad1_6x10          pool_fwd_kernel            maxpool_bwd_amax_s2_kernel, ph = pw = 1
    max_k3s2_valid_6x10         pool_fwd_kernel            maxpool_bwd_amax_s2_kernel, last row / column uncovered
    max_k3s2_same_7x9           pool_fwd_kernel            maxpool_bwd_amax_kernel<2> (odd map)
    max_k3s2_valid_7x10         pool_fwd_kernel            maxpool_bwd_amax_kernel<2> (odd H, even W)
    max_k2s2_valid_6x10         pool_fwd_kernel            maxpool_bwd_amax_kernel<2> (kh != 3)
    max_k3s1_same_5x7           pool3s1_fwd_kernel<true>   maxpool_bwd_amax_kernel<3>
    max_k5s2_same_9x11          pool_fwd_kernel            maxpool_bwd_amax_kernel<3> (ceil(5/2) = 3)
    max_k5s1_same_6x7           pool_fwd_kernel            pool_bwd_kernel, argmax branch (ceil(5/1) = 5)
    max_k3x2s1_5x7              pool_fwd_kernel            pool_bwd_kernel, argmax branch (kh != kw)
    avg_k3s1_same[_inclpad]_5x7 pool3s1_fwd_kernel<false>  avgpool3s1_bwd_kernel
    avg_k3s1_valid_5x7          pool3s1_fwd_kernel<false>  avgpool3s1_bwd_kernel
    avg_k5s3_valid_17x14        pool_fwd_kernel            pool_bwd_kernel, average branch
    avg_k8s1_valid_8x9          pool_fwd_kernel            pool_bwd_kernel, average branch (P = 1, Q = 2)
    avg_k3s2_same[_inclpad]_7x10 pool_fwd_kernel           pool_bwd_kernel, average branch, padded windows

Every max row also runs with argmax=None: pool_bwd_kernel's recompute branch. fp32 gradients take
the <float> instances of the argmax gathers and of avgpool3s1_bwd_kernel."""
import functools
from types import SimpleNamespace

import pytest
import torch

import pool_ref as R
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS16 = 2.0 ** -8   # bf16 output rounding (an IEEE-fp16 build: 2^-11)
EPS32 = 2.0 ** -23
N = 2
CS = (8, 24, 64)  # channel vectors per pixel: 1, 3 (not a power of two: the idx / CV decode), 8
SENT = -77.0      # exact in bf16; never produced by the inputs below

# C = 24 rows whose W * CV (W / 2 * CV for the 2x2-block kernel) exceeds one 256-thread block
WIDE = {
    "max_k3s2_same_5x88": (5, 88, 3, 3, 2, 2, R.same_pads(5, 88, 3, 3, 2, 2), True, False),    # <2>
    "max_k3s1_same_4x88": (4, 88, 3, 3, 1, 1, (1, 1, 1, 1), True, False),                       # <3>
    "max_k3s2_same_4x172": (4, 172, 3, 3, 2, 2, (0, 1, 0, 1), True, False),                     # _s2
}
ROWS = [(n, c) for n in R.CASES for c in CS] + [(n, 24) for n in WIDE]
MAX_ROWS = [(n, c) for n, c in ROWS if n.startswith("max")]
AVG_ROWS = [(n, c) for n, c in ROWS if n.startswith("avg")]
STRIDED = ["max_k3s2_same_6x10", "max_k3s2_same_7x9", "max_k3s1_same_5x7", "avg_k3s1_same_5x7"]
F32_ROWS = ["max_k3s2_same_6x10", "max_k3s2_same_7x9", "max_k3s1_same_5x7", "max_k5s2_same_9x11",
            "avg_k3s1_same_5x7"]


def bf(t):
    return t.to(torch.bfloat16)


def geom(name):
    return R.CASES[name] if name in R.CASES else WIDE[name]


@functools.lru_cache(maxsize=None)
def case(name, C):
    """Inputs (CPU fp32, exact in bf16) and their fp64 reference, computed once per (row, C)."""
    H, W, kh, kw, sh, sw, pads, is_max, incl_pad = geom(name)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 100 + C)
    P, Q = R.out_hw(H, W, kh, kw, sh, sw, pads)
    if is_max:
        x = R.tie_heavy((N, H, W, C), gen)
        dy, base = R.int_grad((N, P, Q, C), gen), R.int_grad((N, H, W, C), gen)
    else:
        x = bf(torch.randn((N, H, W, C), generator=gen)).float()
        dy = bf(torch.randn((N, P, Q, C), generator=gen)).float()
        base = bf(torch.randn((N, H, W, C), generator=gen)).float()
    assert torch.equal(bf(x).float(), x) and torch.equal(bf(dy).float(), dy)
    y, aux = R.pool_fwd_ref(x, kh, kw, sh, sw, pads, is_max, incl_pad)
    dx, mag = R.pool_bwd_ref(dy, x, kh, kw, sh, sw, pads, is_max, incl_pad)
    return SimpleNamespace(x=x, dy=dy, base=base, y=y, aux=aux, dx=dx, mag=mag, P=P, Q=Q,
                           args=(kh, kw, sh, sw, pads, is_max, incl_pad), is_max=is_max)


def gpu_forward(c, x, C):
    y = torch.full((N, c.P, c.Q, C), SENT, dtype=x.dtype, device=DEV)
    amax = torch.full((N, c.P, c.Q, C), 254, dtype=torch.uint8, device=DEV) if c.is_max else None
    Fn.pool_forward(x, y, *c.args, argmax=amax)
    return y, amax


def check_dx(c, dx, accumulate, eps, what):
    ref = c.dx + c.base.double() if accumulate else c.dx
    if c.is_max:
        R.assert_exact(dx, ref, what)
    else:
        R.assert_within(dx, ref, c.mag + c.base.double().abs() if accumulate else c.mag, eps, what)


@pytest.fixture
def fp32_mode():
    set_gpu_compute_dtype(torch.float32)
    Fn.set_f32_native(True)
    yield
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("name,C", ROWS)
def test_pool_forward(name, C):
    c = case(name, C)
    x = bf(c.x).to(DEV)
    y, amax = gpu_forward(c, x, C)
    if c.is_max:
        R.assert_exact(y, c.y, "y")
        R.assert_exact(amax, c.aux, "argmax")
        y2 = torch.full_like(y, SENT)
        Fn.pool_forward(x, y2, *c.args, argmax=None)  # no argmax buffer: the same y
        R.assert_exact(y2, c.y, "y (no argmax buffer)")
    else:
        R.assert_within(y, c.y, c.aux, EPS16, "y")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("use_argmax", [True, False], ids=["amax", "recompute"])
@pytest.mark.parametrize("name,C", MAX_ROWS)
def test_max_pool_backward(name, C, use_argmax, accumulate):
    """The argmax gathers and, with argmax=None, pool_bwd_kernel's recompute branch: both equal the
    first-maximum reference exactly, written or accumulated."""
    c = case(name, C)
    x, dy = bf(c.x).to(DEV), bf(c.dy).to(DEV)
    y, amax = gpu_forward(c, x, C)
    dx = bf(c.base).to(DEV) if accumulate else torch.full(c.x.shape, SENT, dtype=torch.bfloat16, device=DEV)
    Fn.pool_backward(dy, x, y, dx, *c.args, accumulate=accumulate, argmax=amax if use_argmax else None)
    check_dx(c, dx, accumulate, EPS16, "dx")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("name,C", AVG_ROWS)
def test_avg_pool_backward(name, C, accumulate):
    c = case(name, C)
    x, dy = bf(c.x).to(DEV), bf(c.dy).to(DEV)
    y, _ = gpu_forward(c, x, C)
    dx = bf(c.base).to(DEV) if accumulate else torch.full(c.x.shape, SENT, dtype=torch.bfloat16, device=DEV)
    Fn.pool_backward(dy, x, y, dx, *c.args, accumulate=accumulate)
    check_dx(c, dx, accumulate, EPS16, "dx")


def window(t, width, dtype=torch.bfloat16):
    """t as the channel window [..., 8:8+C] of a sentinel-filled buffer C + width channels wide."""
    C = t.shape[-1]
    wide = torch.full(tuple(t.shape[:-1]) + (C + width,), SENT, dtype=dtype, device=DEV)
    v = wide[..., 8:8 + C]
    v.copy_(t)
    return wide, v


def assert_outside_untouched(wide, C, what):
    assert bool((wide[..., :8] == SENT).all()) and bool((wide[..., 8 + C:] == SENT).all()), \
        f"{what}: bytes outside the channel window were written"


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("shared", [True, False], ids=["same_ld", "other_ld"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("name,use_argmax", [(n, a) for n in STRIDED for a in (True, False) if a or n.startswith("max")],
                         ids=lambda v: v if isinstance(v, str) else ("amax" if v else "recompute"))
def test_pool_on_channel_windows(name, use_argmax, C, shared, accumulate):
    """x / dx and y / dy as channel windows of wider buffers (Inception's concat slots): same
    values as the contiguous case, nothing outside a window written, inputs unchanged. other_ld:
    dx and dy live in buffers of another width than x and y, the realignment branch of
    Fn.pool_backward."""
    c = case(name, C)
    xw, x = window(c.x, 24)
    yw, y = window(torch.full((N, c.P, c.Q, C), SENT), 24)
    amax = torch.full((N, c.P, c.Q, C), 254, dtype=torch.uint8, device=DEV) if c.is_max else None
    x0 = xw.clone()
    Fn.pool_forward(x, y, *c.args, argmax=amax)
    if c.is_max:
        R.assert_exact(y, c.y, "y")
        R.assert_exact(amax, c.aux, "argmax")
    else:
        R.assert_within(y, c.y, c.aux, EPS16, "y")
    assert_outside_untouched(yw, C, "y")
    assert torch.equal(xw, x0), "the forward wrote its input"
    other = 24 if shared else 40
    dyw, dy = window(c.dy, other)
    dxw, dx = window(c.base if accumulate else torch.full(c.x.shape, SENT), other)
    y0, dy0 = yw.clone(), dyw.clone()
    Fn.pool_backward(dy, x, y, dx, *c.args, accumulate=accumulate, argmax=amax if use_argmax else None)
    check_dx(c, dx, accumulate, EPS16, "dx")
    assert_outside_untouched(dxw, C, "dx")
    assert torch.equal(xw, x0) and torch.equal(yw, y0) and torch.equal(dyw, dy0), "the backward wrote an input"


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("name", F32_ROWS)
def test_pool_backward_fp32_gradients(fp32_mode, name, C, accumulate):
    """The fp32 path: fp32 dy / dx, the argmax of the 16-bit forward, fp32 tensors of x's and y's
    shapes standing in for them (the gathers read dy and the argmax only)."""
    c = case(name, C)
    _, amax = gpu_forward(c, bf(c.x).to(DEV), C)
    dy = c.dy.to(DEV)
    xs, ys = torch.zeros(c.x.shape, device=DEV), dy
    dx = c.base.to(DEV) if accumulate else torch.full(c.x.shape, SENT, device=DEV)
    Fn.pool_backward(dy, xs, ys, dx, *c.args, accumulate=accumulate, argmax=amax)
    assert dx.dtype == torch.float32
    check_dx(c, dx, accumulate, EPS32, "dx")


def test_pool_backward_fp32_rejects_the_generic_average(fp32_mode):
    c = case("avg_k5s3_valid_17x14", 8)
    dy, dx = c.dy.to(DEV), torch.zeros(c.x.shape, device=DEV)
    with pytest.raises(RuntimeError, match="fp32 supports"):
        Fn.pool_backward(dy, dx, dy, dx, *c.args)


# ---- the grid-stride loop: just over 8192 blocks x 256 threads of eight-channel items ----
GN, GH, GW, GC = 8, 64, 66, 512
assert GN * GH * GW * (GC // 8) > 8192 * 256


def at_index(t, at):
    a = torch.tensor(at, device=t.device)
    return t[:, a[:, 0], a[:, 1]]


def test_grid_stride_generic_forward():
    """pool_fwd_kernel, max k3 s2 SAME onto a 64 x 66 map; the reference on every border pixel and
    4096 random ones."""
    torch.manual_seed(11)
    H, W = 2 * GH, 2 * GW
    args = (3, 3, 2, 2, (0, 1, 0, 1), True, False)
    assert R.out_hw(H, W, *args[:5]) == (GH, GW)
    x = bf(R.tie_heavy((GN, H, W, GC), device=DEV))
    y = torch.full((GN, GH, GW, GC), SENT, dtype=torch.bfloat16, device=DEV)
    amax = torch.full((GN, GH, GW, GC), 254, dtype=torch.uint8, device=DEV)
    Fn.pool_forward(x, y, *args, argmax=amax)
    at = R.border_and_sample(GH, GW, 4096 // GN, torch.Generator().manual_seed(11))
    ry, ra = R.pool_fwd_ref(x.cpu(), *args, at=at)
    R.assert_exact(at_index(y, at), ry, "y")
    R.assert_exact(at_index(amax, at), ra, "argmax")


def test_grid_stride_avg3s1_forward():
    """pool3s1_fwd_kernel<false>."""
    torch.manual_seed(12)
    args = (3, 3, 1, 1, (1, 1, 1, 1), False, False)
    x = bf(torch.randn((GN, GH, GW, GC), device=DEV))
    y = torch.full((GN, GH, GW, GC), SENT, dtype=torch.bfloat16, device=DEV)
    Fn.pool_forward(x, y, *args)
    at = R.border_and_sample(GH, GW, 4096 // GN, torch.Generator().manual_seed(12))
    ry, rm = R.pool_fwd_ref(x.cpu(), *args, at=at)
    R.assert_within(at_index(y, at), ry, rm, EPS16, "y")


@pytest.mark.parametrize("kind", ["avg3s1", "avg5s3"])
def test_grid_stride_avg_backward(kind):
    """avgpool3s1_bwd_kernel and pool_bwd_kernel (average k5 s3 VALID) over a 64 x 66 input map."""
    torch.manual_seed(13)
    args = (3, 3, 1, 1, (1, 1, 1, 1), False, False) if kind == "avg3s1" else (5, 5, 3, 3, R.VALID, False, False)
    P, Q = R.out_hw(GH, GW, *args[:5])
    dy = bf(torch.randn((GN, P, Q, GC), device=DEV))
    x = torch.zeros((GN, GH, GW, GC), dtype=torch.bfloat16, device=DEV)  # not read by an average pool
    dx = torch.full((GN, GH, GW, GC), SENT, dtype=torch.bfloat16, device=DEV)
    Fn.pool_backward(dy, x, dy, dx, *args)
    at = R.border_and_sample(GH, GW, 4096 // GN, torch.Generator().manual_seed(13))
    rdx, rmag = R.pool_bwd_ref(dy.cpu(), torch.zeros(1, 1, 1, 1).expand(GN, GH, GW, GC), *args, at=at)
    R.assert_within(at_index(dx, at), rdx, rmag, EPS16, "dx")


# ---- global average pool ----
@pytest.mark.parametrize("f32", [False, True], ids=["act16", "fp32"])
@pytest.mark.parametrize("C", [8, 24, 2048])
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (8, 8)], ids=["hw1", "hw49", "hw64"])
def test_gap_forward_backward(request, hw, C, f32):
    if f32:
        request.getfixturevalue("fp32_mode")
    H, W = hw
    gen = torch.Generator().manual_seed(H * 1000 + C)
    dt, eps = (torch.float32, EPS32) if f32 else (torch.bfloat16, EPS16)
    x = torch.randn((3, H, W, C), generator=gen).to(dt).to(DEV)
    dy = torch.randn((3, C), generator=gen).to(dt).to(DEV)
    y = torch.full((3, C), SENT, dtype=dt, device=DEV)
    Fn.gap_forward(x, y)
    ry, rm = R.gap_fwd_ref(x.cpu())
    R.assert_within(y, ry, rm, eps, "y")
    dx = torch.full((3, H, W, C), SENT, dtype=dt, device=DEV)
    Fn.gap_backward(dy, dx)
    rdx, rmag = R.gap_bwd_ref(dy.cpu(), H, W)
    R.assert_within(dx, rdx, rmag, eps, "dx")


def test_gap_forward_on_planes():
    """gap_fwd_p3: planes in, planes out; the merged planes against fp64."""
    gen = torch.Generator().manual_seed(49)
    x = torch.randn((3, 7, 7, 24), generator=gen).to(DEV)
    xp = Fn.to_planes(x)
    assert torch.equal(xp.float(), x)  # the split is exact
    out = Fn.Planes.empty((3, 24), DEV)
    Fn.gap_forward(xp, out)
    ry, rm = R.gap_fwd_ref(x.cpu())
    R.assert_within(out.float(), ry, rm, EPS32, "y")
