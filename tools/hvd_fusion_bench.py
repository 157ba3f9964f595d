#!/usr/bin/env python
"""A/B of the hvd API's tensor fusion on ResNet-50's gradient tensor set, one GPU, one process:

  arm a  what hvd did before the fused path: a fresh ``torch.cat`` of every gradient per bucket,
         one division for the average, one ``copy_`` per tensor on the way back;
  arm b  ``FusionBuffer.pack`` + ``FusionBuffer.unpack`` (one HIP launch each, the average folded
         into the unpack scale).

Both arms leave the same values in the gradients (checked before timing). The collective between
the two halves is the same in both arms and is left out. Blocks of ``--steps`` steps are timed with
device events in ABBA order; the A/A spread is the relative difference between the arm-a blocks in
the first and in the last position of the ABBA groups (the same code, measured apart in time).
Writes ``profiles/hvd_fusion.txt``.

    python tools/hvd_fusion_bench.py [--steps 20] [--groups 6] [--out profiles/hvd_fusion.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def gradient_shapes():
    from azure_hc_intel_tf_amd.models import create_model

    m = create_model("resnet50", image_size=224, device="cpu")
    return [tuple(p.shape) for p in m.ps.params]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--groups", type=int, default=6, help="ABBA groups")
    ap.add_argument("--world", type=int, default=8, help="world size of the average (the scale only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hvd_fusion.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU timing says nothing about this path"
    from azure_hc_intel_tf_amd.parallel import hvd
    from azure_hc_intel_tf_amd.parallel.fusion import FusionBuffer
    from azure_hc_intel_tf_amd.parallel.reducer import fusion_threshold_bytes

    hvd.init(engine="native", force=True)
    assert hvd.engine() == "native"
    shapes = gradient_shapes()
    g = torch.Generator(device="cuda").manual_seed(0)
    order = [torch.randn(s, device="cuda", generator=g) for s in reversed(shapes)]  # the optimizer's bucket order
    elems = sum(t.numel() for t in order)
    limit = fusion_threshold_bytes()
    fb = FusionBuffer(order, limit)
    buckets = [order[lo:hi] for lo, hi in fb.runs]
    inv = 1.0 / a.world

    def arm_a():
        for grads in buckets:
            flat = torch.cat([t.reshape(-1) for t in grads])
            out = flat / a.world
            o = 0
            for t in grads:
                t.copy_(out[o:o + t.numel()].view_as(t))
                o += t.numel()

    def arm_b():
        for run in fb.runs:
            fb.pack(1.0, run)
        fb.unpack(inv)

    # same result (world is a power of two: the division and the multiplication agree bitwise)
    ref = [t.clone() for t in order]
    arm_a()
    got_a = [t.clone() for t in order]
    for t, r in zip(order, ref):
        t.copy_(r)
    arm_b()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(got_a, order))
    assert same or a.world & (a.world - 1), "the two arms disagree"

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps  # us per step

    for _ in range(3):
        block(arm_a)
        block(arm_b)
    a_first, a_last, b_all = [], [], []
    for _ in range(a.groups):
        a_first.append(block(arm_a))
        b_all.append(block(arm_b))
        b_all.append(block(arm_b))
        a_last.append(block(arm_a))
    hvd.shutdown()
    ta, tb = statistics.median(a_first + a_last), statistics.median(b_all)
    aa = abs(statistics.median(a_first) - statistics.median(a_last)) / ta
    moved = 4 * elems * 4  # pack: read + write, unpack: read + write, 4 bytes each (padding aside)
    lines = [
        "hvd tensor fusion, ResNet-50 gradient set, one MI355X, forced 1-rank native engine",
        f"tensors {len(order)}  elements {elems}  fp32 bytes {elems * 4}  buckets {len(buckets)} "
        f"(HOROVOD_FUSION_THRESHOLD {limit})",
        f"blocks of {a.steps} steps, {a.groups} ABBA groups, device events, median over blocks",
        f"arm a  torch.cat + divide + per-tensor copy_ : {ta:10.1f} us/step  "
        f"(min {min(a_first + a_last):.1f} max {max(a_first + a_last):.1f})  "
        f"launches/step {sum(len(b) + 2 for b in buckets)} (cat, divide, one copy_ per tensor)",
        f"arm b  fusion_pack + fusion_unpack           : {tb:10.1f} us/step  "
        f"(min {min(b_all):.1f} max {max(b_all):.1f})  launches/step {len(fb.runs) + 1}",
        f"arm b bytes moved {moved}  effective {moved / (tb * 1e-6) / 1e12:.2f} TB/s",
        "  (back to back: unpack re-reads the flat buffer that pack just wrote, and the gradients of the",
        "   step before; both sets fit the 256 MB Infinity Cache, so this is not an HBM rate)",
        f"A/A spread (arm a, first vs last position of the groups): {aa * 100:.2f} %",
        f"a/b {ta / tb:.2f}x  difference {(ta - tb) / ta * 100:.1f} % of arm a  "
        f"-> {'outside' if (ta - tb) / ta > aa else 'INSIDE'} the A/A spread",
        f"results of the two arms bitwise equal: {same}",
    ]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
