"""Elementwise checks of the loss-head and elementwise kernels (csrc/kernels/misc.hip:
softmax_xent, colsum, loss_total, nonfinite, zero_bufs, relu_bwd, add_bf16, dropout_fwd / _bwd;
csrc/kernels/conv_p3.hip: split_planes / merge_planes) on every branch of their launchers, against
the plain references of tests/loss_ref.py: exact (bitwise) wherever the result is determined, a
derived bound elsewhere. Every output buffer is prefilled with NaN or a sentinel and every input's
padding with NaN / Inf poison, so a missed store, an accumulate-instead-of-store and a read of
the padding all show.

The 16-bit cases run in the bf16 build and in the IEEE-fp16 build (torch.ops.hcb16); the fp32
instances (fp32 dlogits, relu_bwd / dropout / colsum on fp32) exist in the bf16 build only and are
reached with Fn.set_f32_native(True) -- without it an fp32 tensor takes the PyTorch path.

Grid caps (second trip of the grid-stride loops): grid_for / p3_grid 4096 blocks x 256 threads x 8
elements = 8388608 elements, nonfinite 4096 x 256 x 4 floats, zero_bufs 2048 x 256 x 4 floats,
colsum ceil(2048 / gy) block rows."""
import contextlib
import math

import pytest
import torch

import loss_ref as R
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
NAN, INF = float("nan"), float("inf")
GRID8 = 8 * 4096 * 256          # elements one trip of an 8-per-thread elementwise grid covers
BIG8 = GRID8 + 8 * 3            # three vectors into the second trip
SENT = -77.0


@contextlib.contextmanager
def build(dtype):
    """Run in the kernel build of ``dtype``: bf16, IEEE fp16, or fp32 (= the bf16 build with the
    fp32-native switch on). bf16 and the switch's previous state are restored afterwards."""
    prev = Fn.planes_mode()  # the fp32-native switch has no getter of its own: planes_mode() reads it
    try:
        set_gpu_compute_dtype(FP16 if dtype == FP16 else BF16)
        Fn.set_f32_native(dtype == FP32)
        yield
    finally:
        Fn.set_f32_native(prev)
        set_gpu_compute_dtype(BF16)


def round8(n):
    return (n + 7) // 8 * 8


def nan_like(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# ====================================================================== softmax_xent
NCLS = (5, 11, 100, 256, 257, 1000, 1001)
# dom_w<k>: one logit 120 above the rest in a column that wave k of the block reads (thread c % 256,
# wave (c % 256) / 64): a row maximum that misses that wave's partial overflows exp (e^120 > FLT_MAX)
ROW_KINDS = ("dom_w0", "dom_w1", "dom_w2", "dom_w3", "dominant_label", "equal", "shift+", "shift-")
ROWS_OF_B = {8: ROW_KINDS, 3: ("shift+", "equal", "dom_w3"), 1: ("shift-",)}


def _softmax_inputs(ncls, B):
    gen = torch.Generator().manual_seed(1000 * ncls + B)
    lddl = round8(ncls + 1)  # 3 / 5 / 4 / 8 / 7 / 8 / 7 padding columns
    ld = lddl + 8
    lg = torch.randn(B, ld, generator=gen) * 3
    lab = torch.randint(0, ncls, (B,), generator=gen)
    shifted = torch.zeros(B, dtype=torch.bool)
    for r, kind in enumerate(ROWS_OF_B[B]):
        if kind.startswith("dom_w"):  # the other classes' probabilities are e^-100 and below
            k = int(kind[-1])
            d = min(64 * k + 63, ncls - 1)  # the last column of wave k's first 64, or the last class
            lg[r, d] = 120.0
            lab[r] = 0 if k % 2 == 0 else ncls - 1  # labels 0 and ncls - 1, never the dominant class
            if lab[r] == d:
                lab[r] = (d + 1) % ncls
        elif kind == "dominant_label":  # p[label] about 0.9: 1 - p is still well conditioned
            lg[r, :ncls] = torch.randn(ncls, generator=gen)
            lg[r, lab[r]] = math.log(9.0 * ncls) + 0.5
        elif kind == "equal":
            lg[r, :ncls] = 1.5
        elif kind in ("shift+", "shift-"):
            lg[r] += 1e4 if kind == "shift+" else -1e4
            lab[r] = 0 if kind == "shift+" else ncls - 1
            shifted[r] = True
    lg[:, ncls::2] = INF  # poison: the padding columns are never read
    lg[:, ncls + 1::2] = NAN
    return lg, lab, shifted, ld, lddl


def _row_loss_tol(lg, ncls, ls, shifted, ref):
    """1e-5 absolute + 1e-5 relative (test_label_smoothing.py's figures at logits of order 10), and
    for the rows shifted by +-1e4 a term K * u, u = ulp(A) of the row's largest |logit| A. K counts
    the kernel's fp32 roundings whose operand is of order A (each at most u: half an ulp of a value
    below 2A): lse = mx + log(s) and lse - (...) make 2. With smoothing there are also 1 - ls,
    pos * z[label] and the second subtraction (3 more), and the uniform term neg * sum(z): the sum
    has ceil(ncls / 256) serial adds per thread, 6 shuffle levels and 3 LDS adds, each rounding a
    partial sum of at most ncls * A, i.e. at most ls * u after the factor neg = ls / ncls, and the
    roundings of neg itself and of the product are ls * u each: ls * (ceil(ncls / 256) + 11).
    (dlogits needs no such term: z - mx is exact for two floats of one binade.)"""
    A = lg[:, :ncls].abs().max(1).values.double()
    u = torch.exp2(torch.floor(torch.log2(A)) - 23)
    K = 2.0 if ls == 0.0 else 5.0 + ls * (math.ceil(ncls / 256) + 11)
    return 1e-5 + 1e-5 * ref.abs() + torch.where(shifted, K * u, torch.zeros_like(u))


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_dl32", "fp16", "fp16_dl32"])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("ncls", NCLS)
def test_softmax_xent_every_element(ncls, B, mode):
    dtype = {"f32": FP32, "bf1": BF16, "fp1": FP16}[mode[:3]]
    lg, lab, shifted, ld, lddl = _softmax_inputs(ncls, B)
    lgd, labd = lg.to(DEV), lab.to(DEV)
    with build(dtype):
        for ls in (0.0, 0.1):
            for sdev in (None, 128.0):
                scale = 1.0 / B
                eff = scale * (sdev or 1.0)
                rl = torch.full((B + 1,), SENT, device=DEV)
                dl = nan_like((B, lddl), dtype)
                dl32 = nan_like((B, lddl), FP32) if mode.endswith("dl32") else None
                sd = None if sdev is None else torch.tensor([sdev], device=DEV)
                assert Fn.native(dl)  # the HIP kernel, not the PyTorch path
                Fn.softmax_xent(lgd, labd, ncls, rl, dl, scale, scale_dev=sd, dl32=dl32, label_smoothing=ls)
                ref_l, ref_d = R.softmax_xent_ref(lg, lab, ncls, eff, ls)
                tag = (ncls, B, mode, ls, sdev)
                # row loss
                assert rl[B].item() == SENT, tag
                err = (rl[:B].double().cpu() - ref_l).abs()
                tol = _row_loss_tol(lg, ncls, ls, shifted, ref_l)
                print("softmax row_loss", tag, "worst err/tol %.3g" % (err / tol).max().item())
                assert (err <= tol).all(), (tag, err, tol)
                # every element written, the padding exactly zero
                for t in (dl, dl32):
                    if t is not None:
                        assert not torch.isnan(t).any(), tag
                        assert torch.equal(t[:, ncls:], torch.zeros(B, lddl - ncls, dtype=t.dtype, device=DEV)), tag
                full = dl if dtype == FP32 else dl32
                if full is not None:  # the fp32 values, element by element
                    e = (full[:, :ncls].double().cpu() - ref_d).abs().max().item()
                    print("softmax dlogits fp32", tag, "worst err %.3g of %.3g" % (e, 1e-5 * eff))
                    assert e <= 1e-5 * eff, (tag, e)
                    s = full[:, :ncls].double().sum(1).abs().max().item()  # softmax - target sums to 0
                    print("softmax dlogits row sum", tag, "%.3g of %.3g" % (s, ncls * 2.0 ** -23 * eff))
                    assert s <= ncls * 2.0 ** -23 * eff, (tag, s)
                if dl32 is not None:  # the 16-bit copy is the rounding of the fp32 one, bit for bit
                    assert torch.equal(R.bits16(dl), R.bits16(dl32.to(dtype))), tag
                elif dtype != FP32:
                    dist = R.ulp16_distance(dl[:, :ncls], ref_d.to(dtype))
                    assert int(dist.max()) <= 1, (tag, int(dist.max()))


# ====================================================================== colsum
def colsum_launch(M, N, det):
    """(gx, gy, mode) by launch_colsum2's formula."""
    gy = (N + 255) // 256
    gx0 = 1 if det else (M + 63) // 64
    cap = (2048 + gy - 1) // gy
    gx = max(1, min(gx0, cap))
    mode = "det" if det else "direct" if gx == 1 else "capped" if gx0 > cap else "atomic"
    return gx, gy, mode


# (M, N, extra ld, dtype, deterministic)
COLSUM_CASES = [
    (1, 8, 0, BF16, False), (3, 24, 0, FP16, False), (64, 255, 0, BF16, False), (64, 257, 8, FP32, False),
    (3, 1001, 0, FP32, False), (1, 256, 16, FP16, False),
    (65, 256, 0, BF16, False), (65, 24, 0, FP32, False), (3001, 257, 16, FP16, False), (2777, 1001, 0, FP32, False),
    (5000, 8, 8, BF16, False),
    (64 * 512 + 65, 1001, 0, BF16, False), (64 * 512 + 1, 1001, 8, FP16, False),
    (5000, 24, 0, BF16, True), (4099, 257, 8, FP32, True), (3001, 1001, 0, FP16, True),
]


def test_colsum_cases_cover_every_launch_mode():
    modes = {colsum_launch(M, N, det)[2] for M, N, _, _, det in COLSUM_CASES}
    assert modes == {"direct", "atomic", "capped", "det"}
    assert {1, 3, 64, 65} <= {c[0] for c in COLSUM_CASES}
    assert {8, 24, 255, 256, 257, 1001} <= {c[1] for c in COLSUM_CASES}
    for dt in (BF16, FP16, FP32):  # each type in each non-deterministic mode but the capped one (16-bit)
        assert {"direct", "atomic"} <= {colsum_launch(M, N, det)[2] for M, N, _, d, det in COLSUM_CASES if d == dt}
    assert any(det and (M + 63) // 64 > 1 for M, _, _, _, det in COLSUM_CASES)  # det forces one block row
    gx, gy, mode = colsum_launch(64 * 512 + 65, 1001, False)
    assert (gx, gy, mode) == (512, 4, "capped")


@pytest.mark.parametrize("M,N,extra,dtype,det", COLSUM_CASES)
def test_colsum_every_column(M, N, extra, dtype, det):
    gx, gy, mode = colsum_launch(M, N, det)
    ld = round8(N) + extra
    torch.manual_seed(M * 7 + N)
    back = nan_like((M + 2, ld), dtype)  # NaN in the columns N..ld and in the rows past M
    back[:M, :N] = torch.randn(M, N, device=DEV).to(dtype)
    g = back[:, :round8(N)]  # extra > 0: a strided view, ld > round8(N)
    assert g.stride(0) == ld
    ref, absum = R.colsum_ref(back, M, N)
    # fp32 additions on the longest path to out[n]: the serial adds of one thread (rows m, m + 8 gx,
    # ...), the 8 LDS partials, and one atomic per block row (none with a single block row)
    d = math.ceil(M / (8 * gx)) + 8 + (gx if gx > 1 else 0)
    with build(dtype):
        assert Fn.native(g)  # the HIP kernel, not the PyTorch path
        _ext.ops()  # load this build's library first: set_deterministic reaches the loaded ones
        was = Fn.deterministic()
        try:
            Fn.set_deterministic(det)
            outs = []
            for rep in range(2 if det else 1):
                out = torch.full((N + 5,), SENT, device=DEV)
                out[:N] = NAN  # garbage: overwritten, never accumulated into
                Fn.colsum(g, M, N, out)
                outs.append(out)
        finally:
            Fn.set_deterministic(was)
    out = outs[0]
    assert torch.equal(out[N:], torch.full((5,), SENT, device=DEV))
    assert not torch.isnan(out[:N]).any()
    err = (out[:N].double() - ref).abs()
    bound = d * 2.0 ** -24 * absum
    print("colsum", (M, N, ld, dtype, mode, gx, gy), "d", d, "worst err/bound %.3g" % (err / bound).max().item())
    assert (err <= bound).all()
    if det:
        assert torch.equal(R.bits32(outs[0]), R.bits32(outs[1]))


# ====================================================================== loss_total
@pytest.mark.parametrize("slots", [None, 1, 300, 4096])
@pytest.mark.parametrize("B", [1, 63, 64, 255, 256, 257, 1000])
def test_loss_total_rows_and_slots(B, slots):
    gen = torch.Generator().manual_seed(B * 10 + (slots or 0))
    row = torch.full((B + 5,), NAN)
    row[:B] = torch.rand(B, generator=gen) * 7
    l2 = None if slots is None else torch.rand(slots, generator=gen) * 1000
    loss = torch.full((2,), SENT, device=DEV)
    Fn.loss_total(row.to(DEV), B, None if l2 is None else l2.to(DEV), 0.5 * 4e-5, loss)
    ref = R.loss_total_ref(row, B, l2, 0.5 * 4e-5)
    print("loss_total", (B, slots), "rel err %.3g of 2e-6" % (abs(loss[0].item() - ref) / abs(ref)))
    assert abs(loss[0].item() - ref) <= 2e-6 * abs(ref)
    assert loss[1].item() == SENT


# ====================================================================== nonfinite
NF_BIG = 4 * 4096 * 256 + 8 + 3  # two body vectors into the second grid trip, and a 3-element tail


def _nf_positions(n):
    n4 = n // 4
    pos = {0, n - 1} | set(range(n4 * 4, n))  # the first, the last, every tail position
    if n4:
        pos |= {n4 * 4 - 1, n4 * 4 - 4}  # the last body element, the start of the last body vector
    return sorted(pos)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, NF_BIG])
def test_nonfinite_every_loop_position(n):
    gen = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=gen)
    base[0] = torch.finfo(FP32).max
    base[-1] = -torch.finfo(FP32).max
    if n > 2:
        base[n // 2] = torch.finfo(FP32).tiny  # the smallest normal value
    g = base.to(DEV)
    flag = torch.zeros(1, device=DEV)
    Fn.nonfinite(g, flag)
    assert R.bits32(flag).item() == 0  # all finite: the zeroed flag stays exactly +0
    flag.fill_(1.0)
    Fn.nonfinite(g, flag)
    assert flag.item() == 1.0  # the kernel never clears: that is the caller's job
    cases = [(p, v) for p in _nf_positions(n) for v in (INF, -INF, NAN)]
    flags = torch.zeros(len(cases), device=DEV)
    for i, (p, v) in enumerate(cases):
        keep = g[p].clone()
        g[p] = v
        Fn.nonfinite(g, flags[i:i + 1])
        g[p] = keep
    got = flags.cpu()
    missed = [c for c, f in zip(cases, got.tolist()) if f != 1.0]
    assert not missed, missed


# ====================================================================== zero_bufs
ZB = 2 ** 20 + 1
ZERO_CASES = [
    (1,), (3, 4), (5, 1023, 1), (4, 1, 1023, 3), (1023, 5, 4, 3, 1),
    (ZB, 1, 3, 4, 5, 1023),
    (ZB, ZB, 1023, 5),  # 2098182 floats: more than the 4 * 2048 * 256 one grid trip covers
]


def _carve(sizes):
    """Buffers at 16-byte-aligned offsets of one NaN arena, 4 to 7 guard floats around each."""
    offs, off = [], 4
    for n in sizes:
        offs.append(off)
        off = (off + n + 4 + 3) // 4 * 4
    arena = nan_like((off + 4,), FP32)
    return arena, [arena[o:o + n] for o, n in zip(offs, sizes)], offs


@pytest.mark.parametrize("sizes", ZERO_CASES, ids=lambda s: "x".join(map(str, s)))
def test_zero_bufs_tails_and_guards(sizes):
    assert sum(ZERO_CASES[-1]) > 4 * 2048 * 256
    arena, bufs, offs = _carve(sizes)
    before = R.bits32(arena).clone()
    Fn.zero_bufs(bufs)
    inside = torch.zeros(arena.numel(), dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        inside[o:o + n] = True
    after = R.bits32(arena)
    assert int(after[inside].abs().max()) == 0            # all +0
    assert torch.equal(after[~inside], before[~inside])   # every guard bit-unchanged


def test_zero_bufs_seven_buffers_raise():
    _, bufs, _ = _carve((4,) * 7)
    with pytest.raises(RuntimeError):
        Fn.zero_bufs(bufs)


# ====================================================================== relu_backward, add
def _relu_inputs(n, dtype):
    gen = torch.Generator().manual_seed(n)
    y = torch.randn(n, generator=gen).to(dtype)
    dy = torch.randn(n, generator=gen).to(dtype)
    # fp32 and bf16 subnormals are left out: whether y = 1e-40 counts as > 0 depends on the
    # compiler's fp32 denormal mode (both types unpack to fp32 subnormals). An fp16 subnormal
    # unpacks to a normal fp32 value and must pass the gradient.
    sp = [0.0, -0.0, -1.0, INF, NAN, -INF, 2.0]
    y[:len(sp)] = torch.tensor(sp).to(dtype)
    if dtype == FP16:
        y[7] = 2.0 ** -24  # the smallest positive fp16 subnormal
    dy[1], dy[3], dy[-1] = -0.0, -0.0, -0.0
    dy[4] = -3.0
    assert torch.isfinite(dy.float()).all()
    return y.to(DEV), dy.to(DEV)


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=str)
@pytest.mark.parametrize("n", [8, 8 * 257, BIG8])
def test_relu_backward_exact(n, dtype):
    y, dy = _relu_inputs(n, dtype)
    dz = nan_like((n,), dtype)
    with build(dtype):
        assert Fn.native(dy)
        Fn.relu_backward(dy, y, dz)
    passed = y.float() > 0
    want = torch.where(passed, dy, torch.zeros_like(dy))
    assert torch.equal(dz, want)  # by value (a blocked gradient may be either zero)
    if dtype == FP32:
        assert torch.equal(R.bits32(dz)[passed], R.bits32(dy)[passed])
    else:
        assert torch.equal(dz.view(torch.int16)[passed], dy.view(torch.int16)[passed])
    if dtype == FP16:
        assert bool(passed[7]) and dz[7].item() == dy[7].item()


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=str)
@pytest.mark.parametrize("n", [8, 8 * 257, BIG8])
def test_add_exact(n, dtype):
    """out = round(a + b): the fp32 sum of two 16-bit values rounded once. (No call site in nn/ or
    models/ passes ``out`` aliasing an input, so no aliasing form is tested.)"""
    torch.manual_seed(n + 1)
    a = torch.randn(n, device=DEV).to(dtype)
    b = (torch.randn(n, device=DEV) * 3).to(dtype)
    b[:2] = -a[:2]  # exact cancellation
    out = nan_like((n,), dtype)
    with build(dtype):
        got = Fn.add(a, b, out)
    assert got is out
    assert torch.equal(out.view(torch.int16), (a.float() + b.float()).to(dtype).view(torch.int16))


# ====================================================================== dropout
def _unpack_bits(mask, n):
    sh = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return ((mask[:n // 8, None] >> sh) & 1).bool().view(-1)


def _dropout(x, keep, seed, step, dtype):
    n = x.numel()
    y = nan_like((n,), dtype)
    mask = torch.full((n // 8 + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    with build(dtype):
        assert Fn.native(x)
        Fn.dropout_forward(x, y, mask, keep, seed, torch.tensor([step], device=DEV))
    return y, mask


@pytest.mark.parametrize("dtype", [BF16, FP16, FP32], ids=str)
@pytest.mark.parametrize("keep", [1.0, 0.5, 0.9])
@pytest.mark.parametrize("n", [8, 8 * 4099, BIG8])
def test_dropout_mask_bits_and_values(n, keep, dtype):
    torch.manual_seed(n)
    x = torch.randn(n, device=DEV)
    x = torch.where(x.to(dtype).float() == 0, torch.ones_like(x), x).to(dtype)  # no zeros
    dy = torch.randn(n, device=DEV).to(dtype)
    # test_dropout_kernel's seed and the step counter's first value. The per-position bound below
    # is only 2.6 standard deviations at the middle size, so it holds for some (seed, step) pairs
    # and not for others: (7, 3) keeps 0.4704 at position 5, keep = 0.5 (3.8 sigma; a host replica
    # of the hash gives the same figure, and no position is off at the largest size)
    seed, step = 7, 0
    y, mask = _dropout(x, keep, seed, step, dtype)
    n8 = n // 8
    assert bool((mask[n8:] == 0xA5).all())  # 7. the over-long mask's tail is untouched
    bit = _unpack_bits(mask, n)
    assert torch.equal(bit, y.float() != 0)  # 1. bit e of mask[i] <=> y[8 i + e] kept
    # 2. kept y = x * (1 / keep), both in fp32 as the kernel scales (tf.nn.dropout's x * scale),
    # rounded to the type: bitwise. Against the true quotient x / keep that is two fp32 roundings
    # (the reciprocal, the product: 2^-24 each) and the type's own; for keep = 1 and 0.5 the
    # reciprocal and the product are exact and it IS x / keep rounded to the type.
    inv = torch.tensor(1.0, device=DEV) / torch.tensor(keep, dtype=FP32, device=DEV)
    zero = torch.zeros((), dtype=dtype, device=DEV)
    want = torch.where(bit, (x.float() * inv).to(dtype), zero)
    bits = R.bits32 if dtype == FP32 else (lambda t: t.view(torch.int16))
    assert torch.equal(bits(y), bits(want))  # dropped: +0
    q = x.double() / keep
    eps = {BF16: 2.0 ** -8, FP16: 2.0 ** -11, FP32: 2.0 ** -24}[dtype]  # unit roundoff of the type
    if keep in (1.0, 0.5):
        assert torch.equal(bits(y)[bit], bits(q.to(dtype))[bit])
    else:
        tiny = 2.0 ** -25 if dtype == FP16 else 0.0  # half an fp16 subnormal step
        assert bool(((y.double() - q).abs()[bit] <= ((2.0 ** -23 + eps) * q.abs() + tiny)[bit]).all())
    if keep == 1.0:
        assert bool(bit.all()) and torch.equal(bits(y), bits(x))  # 5.
    # 3. the backward from the mask bytes alone
    dx = nan_like((n,), dtype)
    with build(dtype):
        Fn.dropout_backward(dy, mask, dx, keep)
    assert torch.equal(bits(dx), bits(torch.where(bit, (dy.float() * inv).to(dtype), zero)))
    # 4. the mask is a function of (seed, step, index) alone: the same for a repeat and for the
    # other element type, different for another step or seed
    y2, mask2 = _dropout(x, keep, seed, step, dtype)
    assert torch.equal(mask2, mask) and torch.equal(bits(y2), bits(y))
    other = BF16 if dtype == FP32 else FP32
    _, mask_o = _dropout(x.to(other), keep, seed, step, other)
    assert torch.equal(mask_o, mask)
    if keep < 1.0 and n >= 8 * 4099:
        assert not torch.equal(_dropout(x, keep, seed, step + 1, dtype)[1], mask)
        assert not torch.equal(_dropout(x, keep, seed + 1, step, dtype)[1], mask)
        # 6. kept fraction, whole tensor and each of the eight bit positions (0.02: the bound of
        # test_dropout_kernel; at n = 32792 one standard deviation of a fair coin's per-position
        # fraction is sqrt(0.25 / 4099) = 0.0078, of the whole tensor's 0.0028)
        frac = bit.view(-1, 8).float().mean(0)
        print("dropout kept fraction", (n, keep), "all %.5f per bit" % bit.float().mean().item(), frac.tolist())
        assert abs(bit.float().mean().item() - keep) < 0.02
        assert bool(((frac - keep).abs() < 0.02).all())
        if n > GRID8:  # enough samples to see a biased hash: 5 standard deviations of a fair coin
            s5 = 5 * math.sqrt(keep * (1 - keep) / (n // 8))
            assert abs(bit.float().mean().item() - keep) < s5 and bool(((frac - keep).abs() < s5).all())


# ====================================================================== to_planes / from_planes
PLANE_SHAPES = [(1, 8), (3, 24), (1000, 1008), (GRID8 // 24 + 2, 24)]  # the last: 8388656 elements


def _domain(shape, seed):
    x = R.domain_bits(shape, torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    edge = torch.tensor([2.0 ** 127, -(2.0 ** 127), 2.0 ** -100, -(2.0 ** -100), 0.0, 1.0, -1.5, 3.0])
    flat[:8] = edge  # the ends of the domain and +0
    return x


def _assert_planes(p, x_cpu):
    assert p.t.dtype == BF16 and tuple(p.shape) == tuple(x_cpu.shape)
    for name, got, want in zip(("hi", "mid", "lo"), p.t, R.split3_ref(x_cpu)):
        assert torch.equal(R.bits16(got), R.bits16(want)), name


# the copy branch (non-uniform rows) hands the kernel a contiguous tensor: the small shapes do
PLANE_CASES = ([(r, c, f) for r, c in PLANE_SHAPES for f in ("contiguous", "channel_slice")]
               + [(r, c, "non_uniform") for r, c in PLANE_SHAPES[:3]])


@pytest.mark.parametrize("rows,C,form", PLANE_CASES)
def test_planes_split_and_merge_bitwise(rows, C, form):
    assert PLANE_SHAPES[-1][0] * PLANE_SHAPES[-1][1] > GRID8
    if form == "contiguous":
        x_cpu = _domain((rows, C), rows + C)
        x = x_cpu.to(DEV)
    elif form == "channel_slice":  # a uniform row stride ldx = C + 16 > C, no copy
        wide = _domain((rows, C + 16), rows + C + 1)
        x_cpu, x = wide[:, 8:8 + C], wide.to(DEV)[:, 8:8 + C]
        assert Fn._rows_uniform(x, C) and (rows == 1 or x.stride(0) == C + 16)
    else:  # rows of two strides: the wrapper falls back to a contiguous copy
        wide = _domain((2, rows + 1, C + 8), rows + C + 2)
        x_cpu, x = wide[:, :rows, :C], wide.to(DEV)[:, :rows, :C]
        assert not Fn._rows_uniform(x, C)
    with build(BF16):
        p = Fn.to_planes(x)
        _assert_planes(p, x_cpu.contiguous())
        back = Fn.from_planes(p.view(-1, C))
    assert torch.equal(R.bits32(back).cpu(), R.bits32(x_cpu.reshape(-1, C)))  # bit-exact on the domain


def test_planes_vector_input_and_negative_zero():
    x_cpu = _domain((24,), 5)  # dim() < 2: one row
    x_cpu[9] = -0.0
    p = Fn.to_planes(x_cpu.to(DEV))
    _assert_planes(p, x_cpu)
    back = Fn.from_planes(p.view(1, 24)).cpu().view(-1)
    assert torch.equal(back, x_cpu)  # by value: -0 comes back as +0
    keep = torch.arange(24) != 9
    assert torch.equal(R.bits32(back)[keep], R.bits32(x_cpu)[keep])


def test_planes_merge_of_a_channel_window():
    """from_planes on a Planes view x[..., a:b] (ldi > C), as a concat buffer's branch window."""
    rows, C = 37, 24
    wide_cpu = _domain((rows, C + 16), 11)
    wide = Fn.to_planes(wide_cpu.to(DEV))
    win = wide[:, 8:8 + C]
    assert Fn.ld(win) == C + 16
    back = Fn.from_planes(win)
    assert torch.equal(R.bits32(back).cpu(), R.bits32(wide_cpu[:, 8:8 + C].contiguous()))


def test_split_planes_leaves_unwritten_storage_alone():
    """The rows past ``rows`` and the columns past C of a wider plane buffer keep their sentinel."""
    rows, C, ldo = 5, 24, 40
    x_cpu = _domain((rows, C), 13)
    out = torch.full((3, rows + 2, ldo), SENT, dtype=BF16, device=DEV)
    _ext.ops().split_planes(x_cpu.to(DEV), C, rows, C, out, ldo)
    for got, want in zip(out, R.split3_ref(x_cpu)):
        assert torch.equal(R.bits16(got[:rows, :C]), R.bits16(want))
    written = torch.zeros((3, rows + 2, ldo), dtype=torch.bool, device=DEV)
    written[:, :rows, :C] = True
    assert bool((out[~written].float() == SENT).all())
