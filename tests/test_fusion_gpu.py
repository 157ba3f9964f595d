"""The multi-tensor fusion kernels (csrc/kernels/fusion.hip) against their PyTorch reference,
bitwise, and the hvd API on a forced 1-rank native engine (RCCL refuses two ranks on one GPU;
the multi-rank probe / fallback logic is covered on gloo by tests/test_fusion_cpu.py)."""
import json

import pytest
import torch

from azure_hc_intel_tf_amd.parallel.fusion import (FusionBuffer, fusion_pack_reference,
                                                   fusion_unpack_reference)

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 0, 255, 256, 1023, 4097, 70001]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SCALES = [1.0, 0.125, 1.0 / 3.0]
SENTINEL = 77.0
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _bits(t):
    return t.view(_INT[t.dtype])


def _views(fill=None, seed=0):
    """Every count x dtype twice: a view at element 4 of its allocation (16-byte aligned for fp32,
    8-byte for the 16-bit types: the vector path) and a view at storage offset 1 (misaligned: the
    scalar path). Returns (views, allocations, guard elements in front)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    views, bufs, fronts = [], [], []
    for front in (4, 1):
        for dt in DTYPES:
            for n in COUNTS:
                if fill is None:
                    buf = torch.randn(n + 2 * front, device="cuda", generator=g).to(dt)
                else:
                    buf = torch.full((n + 2 * front,), fill, device="cuda", dtype=dt)
                views.append(buf[front:front + n])
                bufs.append(buf)
                fronts.append(front)
    return views, bufs, fronts


@pytest.fixture(scope="module")
def sources():
    views, _, fronts = _views()
    for v, f in zip(views, fronts):
        esz = v.element_size()
        assert v.numel() == 0 or v.data_ptr() % (4 * esz) == (0 if f == 4 else esz)
    return views, FusionBuffer(views, bucket_bytes=1 << 16)


@pytest.mark.parametrize("scale", SCALES)
def test_pack_matches_reference_bitwise(sources, scale):
    views, fb = sources
    fb.flat.zero_()
    flat = fb.pack(scale)
    ref = fusion_pack_reference(views, scale)
    torch.cuda.synchronize()
    assert flat.numel() == ref.numel() == fb.total
    assert torch.equal(_bits(flat), _bits(ref))
    pad = torch.ones(fb.total, dtype=torch.bool, device="cuda")
    for off, v in zip(fb.offsets, views):
        assert off % 4 == 0
        pad[off:off + v.numel()] = False
    assert int(pad.sum()) > 0 and torch.all(_bits(flat)[pad] == 0), "padding written"


@pytest.mark.parametrize("scale", SCALES)
def test_unpack_matches_reference_bitwise_and_stays_in_its_views(sources, scale):
    views, _ = sources
    dst, bufs, fronts = _views(fill=SENTINEL)
    fb = FusionBuffer(dst, bucket_bytes=1 << 16)
    fb.flat.copy_(torch.randn(fb.total, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 3)
    # ties of the bf16 rounding: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7 (even: 1), 1 + 3*2^-8
    # halfway between 1 + 2^-7 and 1 + 2^-6 (even: 1 + 2^-6)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20], device="cuda")
    tie_rows = [i for i, d in enumerate(dst) if d.dtype == torch.bfloat16 and d.numel() == 255]
    assert len(tie_rows) == 2  # one on the vector path, one on the scalar path
    for i in tie_rows:
        fb.flat[fb.offsets[i]:fb.offsets[i] + 4] = ties / scale if scale != 1.0 / 3.0 else ties
    want = [torch.empty_like(d) for d in dst]
    fusion_unpack_reference(fb.flat, want, scale)
    fb.unpack(scale)
    torch.cuda.synchronize()
    for d, w in zip(dst, want):
        assert torch.equal(_bits(d), _bits(w)), (d.dtype, d.numel(), d.data_ptr() % 16)
    if scale != 1.0 / 3.0:  # power-of-two scales restore the ties exactly: round to nearest even
        for i in tie_rows:
            assert dst[i][:4].float().tolist() == [1.0, 1.015625, -1.0, 1.0078125]
    for d, b, f in zip(dst, bufs, fronts):
        assert torch.all(b[:f] == SENTINEL) and torch.all(b[f + d.numel():] == SENTINEL), "wrote outside a view"


def test_many_small_entries_and_one_bucket():
    """300 tensors of 1..17 elements in one launch (the block -> entry search crosses a boundary
    at every block), then a pack of one bucket's run of entries only."""
    g = torch.Generator(device="cuda").manual_seed(3)
    xs = [torch.randn(i % 17 + 1, device="cuda", generator=g).to(DTYPES[i % 3]) for i in range(300)]
    fb = FusionBuffer(xs, bucket_bytes=1024)
    assert len(fb.ranges) > 8 and len(fb.ranges) == len(fb.runs)
    assert torch.equal(_bits(fb.pack(0.125)), _bits(fusion_pack_reference(xs, 0.125)))
    ys = [torch.zeros_like(x) for x in xs]
    fb2 = FusionBuffer(ys, bucket_bytes=1024)
    fb2.flat.copy_(fb.flat)
    fb2.unpack(8.0)
    for x, y in zip(xs, ys):
        assert torch.equal(_bits(x), _bits(y))
    want = fb.flat.clone()
    for x in xs:
        x.mul_(2.0)
    k = len(fb.runs) // 2
    fusion_pack_reference(xs, 1.0, fb.offsets, want, fb.runs[k])
    fb.pack(1.0, fb.runs[k])
    torch.cuda.synchronize()
    assert torch.equal(_bits(fb.flat), _bits(want))
    off, n = fb.ranges[k]
    assert not torch.equal(fb.flat[off:off + n], fusion_pack_reference(xs, 0.125)[off:off + n])
    # unpack of the same run touches the other tensors no more than pack touched the other slots
    zs = [torch.full_like(x, SENTINEL) for x in xs]
    fb3 = FusionBuffer(zs, bucket_bytes=1024)
    fb3.flat.copy_(fb.flat)
    fb3.unpack(1.0, fb3.runs[k])
    want_z = [torch.full_like(x, SENTINEL) for x in xs]
    fusion_unpack_reference(fb.flat, want_z, 1.0, fb.offsets, fb.runs[k])
    for z, w in zip(zs, want_z):
        assert torch.equal(_bits(z), _bits(w))


def test_table_checks_and_row_cache():
    from azure_hc_intel_tf_amd.ops import _ext

    xs =[torch.randn(10, device="cuda"), torch.randn(6, device="cuda").half()]
    fb = FusionBuffer(xs)
    assert fb.rebuilds == 1 and not fb.bind(xs) and fb.rebuilds == 1
    assert fb.table.shape == (2, 5) and fb.table[:, 0].tolist() == [x.data_ptr() for x in xs]
    ops = _ext.ops()
    with pytest.raises(RuntimeError, match="table"):
        ops.fusion_pack(fb.table[:, :4].contiguous(), fb.flat, 1.0)
    with pytest.raises(RuntimeError, match="table"):
        ops.fusion_pack(fb.table.int(), fb.flat, 1.0)
    with pytest.raises(RuntimeError, match="float32"):
        ops.fusion_unpack(fb.table, fb.flat.half(), 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.fusion_pack(fb.table, torch.zeros(64, device="cuda")[::2], 1.0)
    with pytest.raises(ValueError, match="not contiguous"):
        FusionBuffer([torch.zeros(4, 6, device="cuda").t()])


@pytest.fixture
def hvd_native(monkeypatch, tmp_path):
    """hvd on a forced 1-rank native engine, threshold 16 KiB, the engine's timeline on."""
    from azure_hc_intel_tf_amd.parallel import hvd

    monkeypatch.delenv("HCB_HVD_ENGINE", raising=False)
    monkeypatch.setenv("HOROVOD_FUSION_THRESHOLD", "16384")
    monkeypatch.setenv("HOROVOD_TIMELINE", str(tmp_path / "hvd_timeline.json"))
    hvd.shutdown()
    hvd.init(engine="native", force=True)
    assert hvd.engine() == "native" and hvd.size() == 1 and hvd.reducer() is not None
    yield hvd
    hvd.shutdown()
    assert hvd.engine() == "torch" and hvd.reducer() is None


def test_hvd_collectives_on_forced_native_engine(hvd_native):
    hvd = hvd_native
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(s, device="cuda", generator=g) for s in [(7,), (3, 3), (1000,), (70001,), (0,)]]
    x0 = [x.clone() for x in xs]
    issued = hvd.reducer().comm.buckets_issued()
    hvd.grouped_allreduce_(xs, average=True)
    torch.cuda.synchronize()
    for a, b in zip(xs, x0):
        assert torch.equal(_bits(a), _bits(b))
    (fb,) = hvd._state["fusion"].values()
    # 70001 floats exceed the 16 KiB threshold: a range of their own, cut further by the engine
    assert hvd.reducer().comm.buckets_issued() - issued > len(fb.ranges) >= 2
    ptr, rebuilds = fb.flat.data_ptr(), fb.rebuilds
    hvd.grouped_allreduce_(xs, average=False, compression=hvd.Compression.bf16)
    torch.cuda.synchronize()
    for a, b in zip(xs, x0):
        assert torch.equal(a, b.bfloat16().float())
    (fb2,) = hvd._state["fusion"].values()
    assert fb2 is fb and fb.flat.data_ptr() == ptr and fb.rebuilds == rebuilds
    t = x0[3].clone()
    assert hvd.allreduce_(t, compression=hvd.Compression.fp16) is t
    assert torch.equal(t, x0[3].half().float())
    assert torch.equal(hvd.allreduce(x0[2]), x0[2]) and torch.equal(hvd.broadcast(x0[1], 0), x0[1])
    i = torch.arange(5, device="cuda")
    assert torch.equal(hvd.allreduce(i, average=False), i)


def _mlp(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.ReLU(), torch.nn.Linear(64, 32)).cuda()


def _weights_equal(a, b):
    return all(torch.equal(_bits(p.detach()), _bits(q.detach())) for p, q in zip(a.parameters(), b.parameters()))


@pytest.mark.parametrize("set_to_none", [False, True])
def test_distributed_optimizer_matches_plain_sgd_bitwise(hvd_native, set_to_none, tmp_path):
    hvd = hvd_native
    model, twin = _mlp(0), _mlp(0)
    opt = hvd.DistributedOptimizer(torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9))
    ref = torch.optim.SGD(twin.parameters(), lr=0.1, momentum=0.9)
    fb, comm = opt._fb, hvd.reducer().comm
    # reverse parameter order: b2 + W2 + b1 fill the first 16 KiB bucket, W1 the second
    assert fb is not None and len(fb.ranges) == 2 and [len(b) for b in opt._buckets] == [3, 1]
    x = torch.randn(3, 16, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    ptr = fb.flat.data_ptr()
    keep = []
    for s in range(3):
        if set_to_none:  # hold the old .grad tensors so the new ones cannot come back at their addresses
            keep.append([p.grad for p in model.parameters()])
        opt.zero_grad(set_to_none=set_to_none)
        ref.zero_grad(set_to_none=set_to_none)
        issued, rebuilds = comm.buckets_issued(), fb.rebuilds
        model(x[s]).pow(2).mean().backward()
        twin(x[s]).pow(2).mean().backward()
        if set_to_none or s == 0:
            assert fb.rebuilds > rebuilds, "new .grad tensors must rebuild their rows"
        else:
            assert fb.rebuilds == rebuilds
        opt.step()
        ref.step()
        torch.cuda.synchronize()
        assert comm.buckets_issued() - issued == len(fb.ranges)
        assert _weights_equal(model, twin), f"step {s}"
        assert fb.flat.data_ptr() == ptr
    hvd.shutdown()  # the engine writes its timeline when it closes
    ev = json.loads((tmp_path / "hvd_timeline.json").read_text())
    assert isinstance(ev, list)
    assert len([e for e in ev if e.get("ph") == "X" and "ALLREDUCE" in e.get("name", "")]) >= 3 * len(fb.ranges)


def test_distributed_optimizer_backward_passes_per_step(hvd_native):
    """Two micro-batches per step: the unpack scale 1/2 replaces the separate division; the twin
    accumulates the same two gradients and halves them by hand (a power of two: bitwise)."""
    hvd = hvd_native
    model, twin = _mlp(1), _mlp(1)
    opt = hvd.DistributedOptimizer(torch.optim.SGD(model.parameters(), lr=0.05), backward_passes_per_step=2)
    ref = torch.optim.SGD(twin.parameters(), lr=0.05)
    x = torch.randn(6, 16, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    comm = hvd.reducer().comm
    for s in range(3):
        issued = comm.buckets_issued()
        for k in range(2):
            opt.zero_grad()
            model(x[2 * s + k]).pow(2).mean().backward()
            opt.step()
        ref.zero_grad()
        for k in range(2):
            twin(x[2 * s + k]).pow(2).mean().backward()
        for p in twin.parameters():
            p.grad.mul_(0.5)
        ref.step()
        torch.cuda.synchronize()
        assert comm.buckets_issued() - issued == len(opt._fb.ranges)
        assert _weights_equal(model, twin), f"step {s}"


def test_distributed_optimizer_zero_fills_a_parameter_without_gradient(hvd_native):
    hvd = hvd_native
    torch.manual_seed(0)
    used, unused = torch.nn.Linear(4, 4).cuda(), torch.nn.Linear(4, 4).cuda()
    w0 = used.weight.detach().clone()
    opt = hvd.DistributedOptimizer(torch.optim.SGD(list(used.parameters()) + list(unused.parameters()), lr=1.0))
    x = torch.ones(2, 4, device="cuda")
    opt.zero_grad()
    used(x).sum().backward()
    opt.step()
    assert unused.weight.grad is not None and torch.all(unused.weight.grad == 0)
    assert torch.equal(used.weight.detach(), w0 - torch.full_like(w0, 2.0))
