"""The eval_metrics HIP kernel (csrc/kernels/metrics.hip, both kernel libraries) and the Evaluator's
captured graph on the MI355X. Every comparison is exact integer equality against the numpy
transcription in tests/eval_ref.py."""
import numpy as np
import pytest
import torch

from eval_ref import eval_ref, make_case
from azure_hc_intel_tf_amd.models import create_model
from azure_hc_intel_tf_amd.ops import _ext
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Evaluator, Trainer, constant_lr, synthetic_batch

pytestmark = pytest.mark.gpu

# the CPU cases, plus more rows than one block covers with a row tail past any vector width,
# and ncls = 5 (every finite target is a top-5 hit)
CASES = [(1, 3), (5, 10), (64, 1001), (70, 257), (257, 1001), (33, 5)]


def _op(ns):
    _ext.load(act="fp16" if ns == "hcb16" else "bf16")
    return getattr(torch.ops, ns).eval_metrics


def _counters():
    return torch.zeros(3, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("ns", ["hcb", "hcb16"])
@pytest.mark.parametrize("B,ncls", CASES)
def test_kernel_matches_reference(ns, B, ncls):
    lg, lab = make_case(B, ncls)
    c = _counters()
    _op(ns)(torch.from_numpy(lg).cuda(), lg.shape[1], torch.from_numpy(lab).cuda(), ncls, c)
    assert tuple(c.tolist()) == eval_ref(lg, lab, ncls)


@pytest.mark.parametrize("ns", ["hcb", "hcb16"])
def test_kernel_accumulates(ns):
    c = _counters()
    want = np.zeros(3, dtype=np.int64)
    for seed in range(3):
        lg, lab = make_case(70, 257, seed=seed)
        _op(ns)(torch.from_numpy(lg).cuda(), lg.shape[1], torch.from_numpy(lab).cuda(), 257, c)
        want += eval_ref(lg, lab, 257)
    assert c.tolist() == want.tolist()


@pytest.mark.parametrize("ns", ["hcb", "hcb16"])
def test_rows_are_not_read_past_ncls(ns):
    """ld == ncls == 1001 (rows not 16-byte aligned), the logits at the very end of an allocation
    whose following bytes hold 3e38: a read past a row's (or the tensor's) end would count it."""
    B, ncls = 9, 1001
    lg, lab = make_case(B, ncls)
    lg = np.ascontiguousarray(lg[:, :ncls])
    buf = torch.full((B * ncls + 64,), 3e38, dtype=torch.float32, device="cuda")
    for start in (0, 1, 2, 3):  # every alignment of the first row
        view = buf[start:start + B * ncls].view(B, ncls)
        buf.fill_(3e38)
        view.copy_(torch.from_numpy(lg))
        c = _counters()
        _op(ns)(view, ncls, torch.from_numpy(lab).cuda(), ncls, c)
        assert tuple(c.tolist()) == eval_ref(lg, lab, ncls), start
    # and flush against the end of its own storage
    tail = torch.from_numpy(lg).cuda()
    c = _counters()
    _op(ns)(tail, ncls, torch.from_numpy(lab).cuda(), ncls, c)
    assert tuple(c.tolist()) == eval_ref(lg, lab, ncls)


def test_graph_replay_keeps_accumulating():
    B, ncls = 70, 257
    cases = [make_case(B, ncls, seed=s) for s in range(3)]
    lg = torch.from_numpy(cases[0][0]).cuda()
    lab = torch.from_numpy(cases[0][1]).cuda()
    c = _counters()
    op = _op("hcb")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        op(lg, lg.shape[1], lab, ncls, c)
    want = np.zeros(3, dtype=np.int64)
    for l, y in cases:  # static buffers rewritten in place; no reset between the replays
        lg.copy_(torch.from_numpy(l))
        lab.copy_(torch.from_numpy(y))
        g.replay()
        want += eval_ref(l, y, ncls)
    torch.cuda.synchronize()
    assert c.tolist() == want.tolist()


@pytest.mark.parametrize("ns", ["hcb", "hcb16"])
def test_binding_checks(ns):
    op = _op(ns)
    lg = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    lab = torch.zeros(4, dtype=torch.int64, device="cuda")
    c = _counters()
    op(lg, 16, lab, 10, c)  # the well-formed call
    with pytest.raises(RuntimeError):
        op(lg.half(), 16, lab, 10, c)
    with pytest.raises(RuntimeError):
        op(lg, 16, lab.int(), 10, c)
    with pytest.raises(RuntimeError):
        op(lg, 8, lab, 10, c)  # ld < ncls
    with pytest.raises(RuntimeError):
        op(lg, 16, lab, 10, c.int())
    with pytest.raises(RuntimeError):
        op(lg, 32, lab, 10, c)  # B * ld past the logits
    assert c.tolist() == [4, 4, 4]  # (all-zero rows: every class ties with the target)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluator_graph_counts_what_the_logits_say(dtype):
    B = 8
    m = create_model("lenet", device="cuda", seed=5, compute_dtype=dtype)
    img, lab = synthetic_batch(m, B, seed=1)
    ev = Evaluator(m, B, use_graph=True, graph_warmup=1)
    ev.reset()
    want = np.zeros(3, dtype=np.int64)
    g = torch.Generator().manual_seed(0)
    for i in range(4):  # eager warm-up, capture + replay, replay, replay
        y = torch.randint(0, m.num_classes, (B,), generator=g)
        if i == 3:
            y[5:] = -1  # a padded last batch
        lab.copy_(y)
        img.copy_(torch.randn(img.shape, generator=g).mul_(60).add_(127).to(img.dtype))
        ev.step(img, lab)
        want += eval_ref(ev.logits.float().cpu().numpy(), y.numpy(), m.num_classes)
    assert ev._g is not None, "the eval step was not graph-captured"
    assert ev.result() == tuple(want.tolist())
    assert ev.result()[0] == 32 - 3


def test_evaluator_counts_32_examples():
    B = 8
    m = create_model("lenet", device="cuda", seed=5, compute_dtype="bf16")
    img, lab = synthetic_batch(m, B, seed=1)
    ev = Evaluator(m, B, use_graph=True, graph_warmup=1)
    for _ in range(4):
        ev.step(img, lab)
    ex, t1, t5 = ev.result()
    assert ex == 32 and 0 <= t1 <= t5 <= 32
    ev.reset()
    assert ev.result() == (0, 0, 0)


def _train(with_eval, steps=4, size=96, batch=16):
    """The BatchNorm configuration tests/test_determinism_gpu.py trains."""
    torch.manual_seed(0)
    m = create_model("resnet50", image_size=size, device="cuda", seed=21, compute_dtype="bf16")
    img, lab = synthetic_batch(m, batch, seed=3)
    t = Trainer(m, batch, constant_lr(0.05), use_graph=True, graph_warmup=1)
    ev = Evaluator(m, batch, use_graph=True, graph_warmup=1, trainer=t) if with_eval else None
    for i in range(steps):
        t.step(img, lab)
        if ev is not None and i == 1:
            eimg, elab = synthetic_batch(m, batch, seed=9)
            for _ in range(3):  # eager, capture + replay, replay -- beside the captured training graph
                ev.step(eimg, elab)
            assert ev._g is not None and ev.result()[0] == 3 * batch
    torch.cuda.synchronize()
    ps = m.ps
    return [x.clone() for x in (ps.master, ps.momentum, ps.buf, ps.persistbuf, t.hyper)]


def test_eval_pass_leaves_training_bitwise_untouched():
    Fn.set_deterministic(True)
    try:
        a = _train(False)
        b = _train(True)
    finally:
        Fn.set_deterministic(False)
    for name, x, y in zip(("masters", "momentum", "BN moving statistics", "BN shifts", "hyper"), a, b):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} elements differ after an eval pass"
