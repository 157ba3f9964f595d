"""Tensor fusion of the hvd API without a GPU: the layout arithmetic, the PyTorch reference of the
pack / unpack kernels, engine selection on a gloo world, and the startup cross-check's fallback
branches driven by a fake engine."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from azure_hc_intel_tf_amd.parallel.fusion import (FusionBuffer, fusion_layout, fusion_pack_reference,
                                                   fusion_unpack_reference)

COUNTS = [1, 3, 4, 5, 0, 255, 1023, 4097]


@pytest.mark.parametrize("bucket_bytes", [1, 16, 64, 1024, 4096, 4100 * 4, 1 << 20, 1 << 40])
def test_layout_slots_and_ranges(bucket_bytes):
    offsets, total, ranges = fusion_layout(COUNTS, bucket_bytes)
    assert len(offsets) == len(COUNTS) and total % 4 == 0
    end = 0
    for off, n in zip(offsets, COUNTS):
        assert off % 4 == 0
        assert off >= end, "slots overlap or are out of order"
        end = off + n
    assert end <= total < end + 4
    # the ranges tile [0, total) exactly once, in order, and start at tensor boundaries only
    pos = 0
    for off, n in ranges:
        assert off == pos and n > 0
        assert off in offsets
        pos = off + n
    assert pos == total
    for off, n in ranges:
        inside = [c for o, c in zip(offsets, COUNTS) if off <= o < off + n and c > 0]
        if n * 4 > bucket_bytes:  # over the threshold only as ONE tensor larger than it, alone
            assert len(inside) == 1 and inside[0] * 4 > bucket_bytes - 16
    for o, c in zip(offsets, COUNTS):
        if c * 4 > bucket_bytes:  # a tensor larger than the threshold is alone in its range
            (r,) = [(a, b) for a, b in ranges if a <= o < a + b]
            assert [cc for oo, cc in zip(offsets, COUNTS) if r[0] <= oo < r[0] + r[1] and cc > 0] == [c]


def test_layout_accepts_tensors_and_is_deterministic():
    ts = [torch.zeros(n) for n in COUNTS]
    assert fusion_layout(ts, 4096) == fusion_layout(COUNTS, 4096)
    assert fusion_layout([], 4096) == ([], 0, [])


def _sources(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype) for n in COUNTS]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("scale", [2.0, 0.125])
def test_reference_round_trip_power_of_two_scale(dtype, scale):
    x = _sources(dtype)
    offsets, total, _ = fusion_layout(x, 1 << 20)
    flat = fusion_pack_reference(x, scale)
    assert flat.dtype == torch.float32 and flat.numel() == total
    pad = torch.ones(total, dtype=torch.bool)
    for off, t in zip(offsets, x):
        pad[off:off + t.numel()] = False
        assert torch.equal(flat[off:off + t.numel()], t.float() * scale)
    assert torch.all(flat[pad] == 0), "padding written"
    y = [torch.full_like(t, 7.0) for t in x]
    fusion_unpack_reference(flat, y, 1.0 / scale)
    for a, b in zip(x, y):
        assert torch.equal(a, b)
    assert torch.all(flat[pad] == 0)


def test_fusion_buffer_on_cpu_uses_the_reference_and_caches_rows():
    x = _sources(torch.float32) + _sources(torch.bfloat16, 1)
    fb = FusionBuffer(x, bucket_bytes=4096)
    assert fb.rebuilds == 1 and not fb.bind(x) and fb.rebuilds == 1  # same tensors: nothing rebuilt
    ptr = fb.flat.data_ptr()
    assert torch.equal(fb.pack(0.5), fusion_pack_reference(x, 0.5))
    want = [t.clone() for t in x]
    for t in x:
        t.zero_()
    fb.unpack(2.0)
    for a, b in zip(x, want):
        assert torch.equal(a, b)
    # one bucket: a contiguous run of entries; the other slots stay as they are
    before = fb.flat.clone()
    lo, hi = fb.runs[1]
    for t in x:
        t.fill_(3.0)
    fb.pack(1.0, (lo, hi))
    off, n = fb.ranges[1]
    assert torch.equal(fb.flat[:off], before[:off]) and torch.equal(fb.flat[off + n:], before[off + n:])
    assert torch.all(fb.flat[off:off + n][fb.flat[off:off + n] != 0] == 3.0)
    # a replaced tensor (new storage) rebuilds its row; the flat buffer persists
    x2 = list(x)
    x2[3] = x[3].clone()
    assert fb.bind(x2) and fb.rebuilds == 2 and fb.flat.data_ptr() == ptr
    with pytest.raises(ValueError, match="not contiguous"):
        FusionBuffer([torch.zeros(4, 6).t()])
    with pytest.raises(ValueError, match="elements"):
        fb.bind([torch.zeros(2)])
    with pytest.raises(TypeError, match="dtype"):
        FusionBuffer([torch.zeros(3, dtype=torch.int32)])
    unbound = FusionBuffer(x, bind=False)
    with pytest.raises(RuntimeError, match="not bound"):
        unbound.pack(1.0)


# ---- world 2 on gloo (the spawn helper pattern of tests/test_hvd_dist.py)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, fn, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    try:
        from azure_hc_intel_tf_amd.parallel import hvd

        hvd.init(backend="gloo")
        fn(hvd)
        hvd.shutdown()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc()))


def run(world, fn):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, fn, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=240) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    errs = [r for r in res if r[1] != "ok"]
    assert not errs, errs


def _torch_engine_on_gloo(hvd):
    r, n = hvd.rank(), hvd.size()
    assert hvd.engine() == "torch" and hvd.reducer() is None
    ts = [torch.full((7,), float(r)), torch.full((3, 3), 2.0 * r), torch.full((5,), float(r + 1)).bfloat16()]
    hvd.grouped_allreduce_(ts)
    assert torch.equal(ts[0], torch.full((7,), (n - 1) / 2))
    assert torch.equal(ts[1], torch.full((3, 3), float(n - 1)))
    assert torch.equal(ts[2], torch.full((5,), (n + 1) / 2).bfloat16())
    s = [torch.full((4,), float(r + 1))]
    hvd.grouped_allreduce_(s, average=False)
    assert torch.equal(s[0], torch.full((4,), n * (n + 1) / 2))
    # DistributedOptimizer: the fresh-buffer path, replicas in sync and equal to the hand average
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    twin = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))
    twin.load_state_dict(model.state_dict())
    opt = hvd.DistributedOptimizer(torch.optim.SGD(model.parameters(), lr=0.1))
    assert opt._fb is None
    xs = [torch.randn(4, 8, generator=torch.Generator().manual_seed(10 + k)) for k in range(n)]
    opt.zero_grad()
    model(xs[r]).pow(2).mean().backward()
    opt.step()
    grads = []
    for k in range(n):
        twin.zero_grad()
        twin(xs[k]).pow(2).mean().backward()
        grads.append([p.grad.clone() for p in twin.parameters()])
    with torch.no_grad():
        for i, p in enumerate(twin.parameters()):
            p -= 0.1 * sum(g[i] for g in grads) / n
    for a, b in zip(model.parameters(), twin.parameters()):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)
    # a second init on the live gloo group: the engine argument is validated, native is refused
    hvd._state["initialized"] = False
    with pytest.raises(ValueError):
        hvd.init(backend="gloo", engine="mpi")
    with pytest.raises(RuntimeError, match="RCCL process group"):
        hvd.init(backend="gloo", engine="native")
    hvd.init(backend="gloo", engine="torch")
    assert hvd.engine() == "torch" and hvd.is_initialized()


def test_gloo_world_stays_on_torch_engine():
    run(2, _torch_engine_on_gloo)


class _FakeComm:
    def __init__(self, hvd, mode):
        self.hvd, self.mode = hvd, mode

    def allreduce_(self, t, average=False):
        from azure_hc_intel_tf_amd.parallel.native import xgmi_probe

        if self.mode == "raise_rank0" and self.hvd.rank() == 0:
            raise RuntimeError("ncclAllReduce failed")
        t.copy_(sum(xgmi_probe(t.numel(), r) for r in range(self.hvd.size())))
        if self.mode == "wrong_rank1" and self.hvd.rank() == 1:
            t[11] += 0.5
        return t


class _FakeReducer:
    closed = 0

    def __init__(self, hvd, mode):
        self.comm = _FakeComm(hvd, mode)

    def close(self):
        type(self).closed += 1


def _probe_branches(hvd):
    r = hvd.rank()

    def start(mode, factory=None):
        hvd._state.update(engine="torch", reducer=None)
        hvd._start_native(factory or (lambda: _FakeReducer(hvd, mode)), device=None, n=4096)
        return hvd.engine()

    assert start("good") == "native" and isinstance(hvd.reducer(), _FakeReducer)
    # CPU tensors never take the native path, whatever the engine
    t = torch.full((3,), float(r + 1))
    hvd.allreduce_(t, average=False)
    assert torch.all(t == 3.0)
    closed = _FakeReducer.closed
    e = start("wrong_rank1")
    assert e.startswith("torch(fallback: ") and hvd.reducer() is None and _FakeReducer.closed == closed + 1
    assert ("mismatch vs torch.distributed in 1/4096" in e) if r == 1 else ("failed on another rank" in e), e
    e = start("raise_rank0")
    assert e.startswith("torch(fallback: RuntimeError: ncclAllReduce failed" if r == 0 else
                        "torch(fallback: failed on another rank"), e

    def broken_on_rank1():
        if r == 1:
            raise OSError("_hcb_comm.so: cannot open shared object file")
        return _FakeReducer(hvd, "good")

    e = start(None, broken_on_rank1)
    assert e.startswith("torch(fallback: OSError: _hcb_comm.so" if r == 1 else
                        "torch(fallback: failed on another rank"), e
    # after a fallback the collectives are torch.distributed's, and still matched across ranks
    ts = [torch.full((6,), float(r))]
    hvd.grouped_allreduce_(ts)
    assert torch.equal(ts[0], torch.full((6,), 0.5))


def test_startup_probe_falls_back_on_every_rank(capfd):
    run(2, _probe_branches)
    err = capfd.readouterr().err
    assert err.count("[hcb] hvd: native engine not used") == 3  # rank 0 only, once per failed start
