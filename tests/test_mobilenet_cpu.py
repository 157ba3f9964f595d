"""MobileNet-v2 (``--model=mobilenet``) on the CPU path: parameter count from the table, block
shapes, one training step of a two-block network against an independent torch.nn + autograd model
in fp64, the CLI, and a checkpoint round trip. On a tree without the model these fail with
``unknown model``."""
import os
import subprocess
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def count_from_table(ncls: int) -> int:
    """Trainable parameters of MobileNet-v2 1.0: conv kernels (no bias) + BN gamma / beta + classifier."""
    n = 3 * 9 * 32 + 2 * 32
    cin = 32
    for t, c, reps, _ in TABLE:
        for _ in range(reps):
            mid = cin * t
            if t != 1:
                n += cin * mid + 2 * mid
            n += 9 * mid + 2 * mid
            n += mid * c + 2 * c
            cin = c
    n += cin * 1280 + 2 * 1280
    return n + 1280 * ncls + ncls


def test_builds_with_the_published_parameter_count():
    assert count_from_table(1000) == 3_504_872  # the published total, as a cross-check of the formula
    m = create_model("mobilenet", device="cpu")
    assert m.num_params() == count_from_table(m.num_classes) == 3_504_872 + 1_281 * (m.num_classes - 1000)
    assert m.default_batch_size == 32 and m.image_size == 224


def test_block_output_shapes_at_224():
    m = create_model("mobilenet", device="cpu")
    assert m.stem.out_shape == (112, 112, 32)
    want = [(112, 16)] + [(56, 24)] * 2 + [(28, 32)] * 3 + [(14, 64)] * 4 + [(14, 96)] * 3 + [(7, 160)] * 3 + [(7, 320)]
    assert [(b.out_shape[0], b.out_shape[2]) for b in m.blocks] == want
    assert all(b.out_shape[0] == b.out_shape[1] for b in m.blocks)
    assert m.tail.out_shape == (7, 7, 1280)
    assert sorted({b.dw.in_shape[2] for b in m.blocks}) == [32, 96, 144, 192, 384, 576, 960]
    assert len(m.blocks) == 17 and sum(b.identity for b in m.blocks) == 10
    assert m.blocks[0].dw.flops(2) == 2 * 2 * 112 * 112 * 32 * 9


class _RefNet(nn.Module):
    """An independent torch.nn MobileNet-v2 (TF 'SAME' padding, batch-statistics BN, ReLU6)."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    @staticmethod
    def same(x, k, s):
        H, W = x.shape[2:]
        ph = max((-(-H // s) - 1) * s + k - H, 0)
        pw = max((-(-W // s) - 1) * s + k - W, 0)
        return F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))

    def cbn(self, l, x, P, dw=False):
        if dw:
            w = P[l.w.name].view(-1, 1, 3, 3)
            z = F.conv2d(self.same(x, 3, l.stride), w, stride=l.stride, groups=w.shape[0])
        else:
            w = P[l.w.name].permute(0, 3, 1, 2)
            z = F.conv2d(self.same(x, l.spec.kh, l.spec.sh), w, stride=l.spec.sh)
        y = F.batch_norm(z, None, None, P[l.gamma.name], P[l.beta.name], True, 0.0, l.eps)
        return y

    def forward(self, img, P):
        m = self.m
        x = F.hardtanh(self.cbn(m.stem, img.permute(0, 3, 1, 2), P), 0, 6)
        for b in m.blocks:
            h = x
            if b.expand is not None:
                h = F.hardtanh(self.cbn(b.expand, h, P), 0, 6)
            h = F.hardtanh(self.cbn(b.dw, h, P, dw=True), 0, 6)
            h = self.cbn(b.project, h, P)
            x = x + h if b.identity else h
        x = F.hardtanh(self.cbn(m.tail, x, P), 0, 6).mean(dim=(2, 3))
        return x @ P[m.fc.w.name].view(m.fc.ncls, -1).t() + P[m.fc.b.name]


def test_two_block_step_matches_autograd_fp64(monkeypatch):
    monkeypatch.setenv("HCB_CPU_DTYPE", "float64")
    # stem + (1,16,1,1) + (6,24,2,2) + (6,24,1,1): no expand / stride 2 on an even size / identity add
    m = create_model("mobilenet", device="cpu", image_size=32, seed=5, blocks=((1, 16, 1, 1), (6, 24, 2, 2)))
    assert [b.identity for b in m.blocks] == [False, False, True]
    img, lab = synthetic_batch(m, 4)
    img = ((img - 127.0) / 60.0).double()
    P = {p.name: p.data.detach().clone().double().requires_grad_(True) for p in m.ps.params}
    loss = F.cross_entropy(_RefNet(m)(img, P), lab)
    loss.backward()
    t = Trainer(m, 4, constant_lr(0.0), weight_decay=0.0)
    t._forward_backward(img, lab)
    assert torch.allclose(t.row_loss.mean().double(), loss.detach(), rtol=1e-6, atol=1e-7)
    for p in m.ps.params:
        r = P[p.name].grad
        err = (p.grad.double() - r).abs().max().item()
        assert err <= 1e-5 * r.abs().max().item() + 1e-12, f"{p.name}: max err {err}"


def test_cli_two_steps_on_cpu():
    from azure_hc_intel_tf_amd.bench.flags import parse_flags

    assert parse_flags(["--model=mobilenet"]).model == "mobilenet"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tf_cnn_benchmarks.py"), "--model=mobilenet", "--device=cpu",
                        "--image_size=32", "--batch_size=4", "--num_batches=2", "--num_warmup_batches=0"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "total images/sec" in r.stdout


def test_checkpoint_round_trip(tmp_path):
    kw = dict(device="cpu", image_size=32, blocks=((1, 16, 1, 1), (6, 24, 2, 2)))
    m = create_model("mobilenet", seed=1, **kw)
    img, lab = synthetic_batch(m, 4)
    Trainer(m, 4, constant_lr(0.05)).step((img - 127.0) / 60.0, lab)  # moves the weights and the BN buffers
    path = str(tmp_path / "ck.pt")
    torch.save(m.ps.state_dict(), path)
    m2 = create_model("mobilenet", seed=2, **kw)
    dw, dw2 = m.blocks[1].dw, m2.blocks[1].dw
    assert not torch.equal(dw.w.data, dw2.w.data)
    m2.ps.load_state_dict(torch.load(path))
    assert torch.equal(dw.w.data, dw2.w.data) and dw.w.name.endswith("depthwise/kernel")
    assert torch.equal(dw.rmean.data, dw2.rmean.data) and torch.equal(dw.rvar.data, dw2.rvar.data)
    assert float(dw.rmean.data.abs().max()) > 0
    assert torch.equal(m.ps.master, m2.ps.master) and torch.equal(m.ps.buf, m2.ps.buf)


def test_width_multiplier_rounds_channels_and_trains():
    from azure_hc_intel_tf_amd.models.mobilenet import _make_divisible

    # slim's rounding: to a multiple of 8, at least 8, never more than 10 % below the request
    assert [_make_divisible(v) for v in (32 * 0.5, 24 * 0.5, 16 * 0.35, 32 * 0.75, 96 * 0.75, 10.0)] == [16, 16, 8, 24, 72, 16]
    m = create_model("mobilenet", device="cpu", image_size=32, width=0.5, blocks=((1, 16, 1, 1), (6, 24, 2, 2)))
    assert m.stem.out_shape[2] == 16 and [b.out_shape[2] for b in m.blocks] == [8, 16, 16]
    assert m.blocks[1].dw.in_shape[2] == 48 and m.tail.out_shape[2] == 1280  # the tail never shrinks
    wide = create_model("mobilenet", device="cpu", image_size=32, width=1.4, blocks=((1, 16, 1, 1),))
    assert wide.stem.out_shape[2] == 48 and wide.blocks[0].out_shape[2] == 24 and wide.tail.out_shape[2] == 1792
    img, lab = synthetic_batch(m, 4)
    t = Trainer(m, 4, constant_lr(0.01))
    losses = [float(t.step((img - 127.0) / 60.0, lab)) for _ in range(3)]
    assert all(l == l for l in losses) and losses[-1] < losses[0]
