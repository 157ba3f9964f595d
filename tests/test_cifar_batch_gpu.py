"""The ``cifar_batch`` HIP kernel (csrc/kernels/cifar.hip, both kernel libraries) against
``cifar_batch_reference`` in float64, elementwise, and ``Cifar10Loader`` on the GPU against the same
loader on the CPU.

A 20-image dataset and B = 7 (grid rows that are no power of two); every corner offset, both flips, an
index -1 row, Cpad 8 and 16. Bounds, from the number formats alone: the reference multiplies by the
float32 constant 1 / 127.5 and subtracts 1 in float64; the kernel does the same in float32, at most two
roundings of values below 2 -> |err| <= 2 * 2^-24 for fp32 output; a 16-bit output rounds that once more,
so it lies within one unit in the last place (of the reference rounded to the type) of it. Pad pixels
(-1.0), zero channels, index -1 rows and labels are exact."""
import os
import sys

import numpy as np
import pytest
import torch

from azure_hc_intel_tf_amd.data.cifar10 import Cifar10Loader, cifar_batch_reference
from azure_hc_intel_tf_amd.nn.layers import set_gpu_compute_dtype
from azure_hc_intel_tf_amd.ops import _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

N, B = 20, 7
DESC = [(19, 0, 0, 0), (3, 8, 8, 1), (0, 0, 8, 0), (-1, 4, 4, 0), (11, 8, 0, 1), (7, 4, 4, 0), (19, 0, 0, 1)]
_CASE = {}


def _case():
    """The dataset and the float64 references (per Cpad), computed once and left unchanged."""
    if not _CASE:
        rng = np.random.default_rng(7)
        data = torch.from_numpy(rng.integers(0, 256, size=(N, 3, 32, 32), dtype=np.uint8))
        labels = torch.from_numpy(rng.integers(0, 10, size=N))
        _CASE.update(data=data, labels=labels, desc=torch.tensor(DESC, dtype=torch.int32))
        for cpad in (8, 16):
            ref = torch.empty((B, 32, 32, cpad), dtype=torch.float64)
            _CASE[cpad] = cifar_batch_reference(data, labels, DESC, ref, dtype=torch.float64)
    return _CASE


def _ulp(v: torch.Tensor, mant_bits: int) -> torch.Tensor:
    """One unit in the last place of each (float64-held) value of a type with ``mant_bits`` stored bits."""
    _, e = torch.frexp(v)  # v = m * 2^e, 0.5 <= |m| < 1
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 1 - mant_bits))


def _check(out, lab, ref, ref_lab, dtype):
    got = out.cpu().double()
    pad = ref[..., :3] == -1.0
    assert bool(pad.any()) and torch.equal(got[..., :3][pad], ref[..., :3][pad])  # padded pixels: exactly -1
    assert float(got[..., 3:].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
    if dtype == torch.float32:
        err = float((got - ref).abs().max())
        print(f"fp32 max |err| = {err:.3e} (bound {2 * 2.0 ** -24:.3e})")
        assert err <= 2 * 2.0 ** -24, err
    else:
        rr = ref.to(dtype).double()
        ulps = float(((got - rr).abs() / _ulp(rr, 7 if dtype == torch.bfloat16 else 10).clamp(min=1e-300)).max())
        print(f"{dtype} max error {ulps} ulp")
        assert bool(((got - rr).abs() <= _ulp(rr, 7 if dtype == torch.bfloat16 else 10)).all()), ulps
    assert torch.equal(lab.cpu(), ref_lab)


@pytest.mark.parametrize("cpad", [8, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_kernel_matches_float64_reference(dtype, cpad):
    c = _case()
    ref, ref_lab = c[cpad]
    try:
        set_gpu_compute_dtype(torch.float16 if dtype == torch.float16 else torch.bfloat16)
        out = torch.full((B, 32, 32, cpad), 7.0, dtype=dtype, device="cuda")
        lab = torch.full((B,), 99, dtype=torch.int64, device="cuda")
        _ext.ops().cifar_batch(c["data"].cuda(), c["labels"].cuda(), c["desc"].cuda(), c["desc"], out, lab)
        torch.cuda.synchronize()
        _check(out, lab, ref, ref_lab, dtype)
    finally:
        set_gpu_compute_dtype(torch.bfloat16)


def test_binding_refuses_bad_rows_and_operands():
    c = _case()
    data, labels, desc = c["data"].cuda(), c["labels"].cuda(), c["desc"]
    out = torch.empty((B, 32, 32, 8), dtype=torch.bfloat16, device="cuda")
    lab = torch.empty(B, dtype=torch.int64, device="cuda")
    op = _ext.ops().cifar_batch

    def bad(row, col, val):
        d = desc.clone()
        d[row, col] = val
        return d

    for d, msg in [(bad(2, 0, N), "index"), (bad(2, 0, -2), "index"), (bad(1, 1, 9), "crop offset"),
                   (bad(1, 2, -1), "crop offset"), (bad(5, 3, 2), "flip")]:
        with pytest.raises(RuntimeError, match=msg):
            op(data, labels, d.cuda(), d, out, lab)
    with pytest.raises(RuntimeError, match="desc_host"):
        op(data, labels, desc.cuda(), desc[:B - 1].contiguous(), out, lab)
    with pytest.raises(RuntimeError, match="desc_host"):
        op(data, labels, desc.cuda(), desc.cuda(), out, lab)
    wide = torch.empty((B, 32, 32, 16), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):
        op(data, labels, desc.cuda(), desc, wide[..., :8], lab)
    with pytest.raises(RuntimeError, match="out"):
        op(data, labels, desc.cuda(), desc, out[:B - 1], lab)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loader_on_gpu_matches_loader_on_cpu(tmp_path, dtype):
    import make_fake_cifar10

    make_fake_cifar10.make(str(tmp_path), per_file=4, seed=1)  # 20 training images
    try:
        set_gpu_compute_dtype(torch.bfloat16)
        lg = Cifar10Loader(str(tmp_path), B, "cuda", rank=0, world=1, train=True, seed=21)
        lc = Cifar10Loader(str(tmp_path), B, "cpu", rank=0, world=1, train=True, seed=21)
        img_g = torch.empty((B, 32, 32, 8), dtype=dtype, device="cuda")
        lab_g = torch.empty(B, dtype=torch.int64, device="cuda")
        img_c = torch.empty((B, 32, 32, 8), dtype=torch.float64)
        lab_c = torch.empty(B, dtype=torch.int64)
        for _ in range(3):  # 21 rows of a 20-image split: the third batch crosses the epoch boundary
            assert lg.next_into(img_g, lab_g) == B and lc.next_into(img_c, lab_c) == B
            torch.cuda.synchronize()
            assert np.array_equal(lg.last_desc, lc.last_desc)
            got = img_g.cpu().double()
            if dtype == torch.float32:
                assert float((got - img_c).abs().max()) <= 2 * 2.0 ** -24
            else:
                rr = img_c.to(dtype).double()
                assert bool(((got - rr).abs() <= _ulp(rr, 7)).all())
            assert torch.equal(lab_g.cpu(), lab_c)
        lg.close()
        lc.close()
    finally:
        set_gpu_compute_dtype(torch.bfloat16)
