#!/usr/bin/env python
"""The local response normalisation kernels (csrc/kernels/lrn.hip) at the CIFAR-10 AlexNet's layer, x
[128, 16, 16, 64] with lrn(4, 1.0, 0.001 / 9, 0.75), in the three format pairs the model runs -- bf16 in / bf16
out, fp32 in / Planes out (lrn2 of the fp32 step), Planes in / Planes out (lrn1) -- against
``torch.nn.functional.local_response_norm`` (NCHW view of the same channels-last memory, alpha * 9) and its
autograd on the same machine in the same process.

Method: every op is warmed up, then timed as ITERS back-to-back launches between two events; the median of
ROUNDS such rounds is reported, the variants interleaved round by round. The tensors (8 MiB in fp32) stay in
the 256 MiB Infinity Cache between launches, as they do inside the training step: the GB/s column is a
cache-warm rate, not an HBM rate. Bytes per element are the algorithmic ones: a 16-bit tensor moves 2, an fp32
tensor 4, Planes 6 (three bf16 planes); the forward reads x and writes y, the backward reads x and dy and
writes dx. PyTorch's backward is one autograd call on a retained graph (its saved intermediates are not
charged).

    python tools/lrn_bench.py [--batch 128] [--iters 50] [--rounds 9]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azure_hc_intel_tf_amd.ops import _ext  # noqa: E402
from azure_hc_intel_tf_amd.ops import functional as Fn  # noqa: E402

R, BIAS, ALPHA, BETA = 4, 1.0, 0.001 / 9.0, 0.75
BYTES = {"bf16": 2, "fp32": 4, "planes": 6}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    shape = (args.batch, 16, 16, 64)
    n = args.batch * 16 * 16 * 64
    _ext.set_act("bf16")
    print(f"# x {list(shape)}, lrn(r={R}, bias={BIAS}, alpha=0.001/9, beta={BETA}); {args.iters} launches per round, "
          f"median of {args.rounds} rounds, random data, cache-warm")
    print("# pair             | fwd us  B/elem  GB/s  torch us | bwd us  B/elem  GB/s  torch us")
    # (name, x format, y format, gradient format, torch dtype)
    for name, xf, yf, gf, dt in (("bf16->bf16", "bf16", "bf16", "bf16", torch.bfloat16),
                                 ("fp32->planes", "fp32", "planes", "fp32", torch.float32),
                                 ("planes->planes", "planes", "planes", "fp32", torch.float32)):
        Fn.set_f32_native(dt == torch.float32)
        xt = torch.randn(shape, device="cuda").to(dt)
        dy = torch.randn(shape, device="cuda").to(dt)
        x = Fn.to_planes(xt) if xf == "planes" else xt
        y = Fn.Planes.empty(shape, "cuda") if yf == "planes" else torch.empty_like(xt)
        dx = torch.empty_like(dy)
        xn = xt.permute(0, 3, 1, 2).detach().requires_grad_(True)  # NCHW view of NHWC memory
        dyn = dy.permute(0, 3, 1, 2)

        def t_fwd():
            with torch.no_grad():
                return F.local_response_norm(xn, 2 * R + 1, alpha=ALPHA * (2 * R + 1), beta=BETA, k=BIAS)

        yn = F.local_response_norm(xn, 2 * R + 1, alpha=ALPHA * (2 * R + 1), beta=BETA, k=BIAS)
        ops = {
            "fwd": lambda: Fn.lrn_forward(x, y, R, BIAS, ALPHA, BETA),
            "bwd": lambda: Fn.lrn_backward(dy, x, dx, R, BIAS, ALPHA, BETA),
            "t_fwd": t_fwd,
            "t_bwd": lambda: torch.autograd.grad(yn, xn, dyn, retain_graph=True),
        }
        # the kernels against PyTorch on these very tensors, before anything is timed
        ops["fwd"]()
        ops["bwd"]()
        ref_y, (ref_dx,) = t_fwd().permute(0, 2, 3, 1).float(), ops["t_bwd"]()
        ey = float((Fn.from_planes(y).float() - ref_y).norm() / ref_y.norm())
        ed = float((dx.float() - ref_dx.permute(0, 2, 3, 1).float()).norm() / ref_dx.float().norm())
        for fn in ops.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in ops}
        for _ in range(args.rounds):
            for k, fn in ops.items():
                t[k].append(timed(fn, args.iters))
        m = {k: statistics.median(v) for k, v in t.items()}
        bf, bb = BYTES[xf] + BYTES[yf], BYTES[xf] + 2 * BYTES[gf]
        print(f"{name:18s} | {m['fwd']:6.1f} {bf:6d} {n * bf / (m['fwd'] * 1e-6) / 1e9:6.0f} {m['t_fwd']:8.1f} | "
              f"{m['bwd']:6.1f} {bb:6d} {n * bb / (m['bwd'] * 1e-6) / 1e9:6.0f} {m['t_bwd']:8.1f}"
              f"   (vs torch: fwd {ey:.1e}, bwd {ed:.1e})")
    Fn.set_f32_native(False)


if __name__ == "__main__":
    main()
