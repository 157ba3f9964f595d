#!/usr/bin/env python
"""The depthwise 3x3 kernels (csrc/kernels/dwconv.hip) on the 17 depthwise problems of MobileNet-v2
at batch 32, fp32 and bf16, against ``F.conv2d(groups=C)`` (channels-last) and its autograd on the
same machine in the same process.

Method: every op is warmed up, then timed as ITERS back-to-back launches between two events; the
median of ROUNDS such rounds is reported, the variants interleaved round by round. Inputs are random.
The tensors of the small problems stay in the 256 MiB Infinity Cache between launches ("warm"); a
problem is marked "cold" when one launch's traffic exceeds the cache and "part" when the buffers of
all its interleaved variants together (about three times one launch's traffic) do. Bytes moved are the algorithmic ones:
forward x + z, data gradient dz + dx, weight gradient x + dz (weights and the slab workspace are
noise). The PyTorch backward is timed as ONE autograd call producing dx and dw, so its column
stands against dgrad + wgrad together. PyTorch is never charged a padding copy: symmetric pads go
through conv2d's own ``padding=``; the bottom / right-only pad of a stride-2 'SAME' conv on an even
size is applied once, outside the timed region, and conv2d and its autograd run on the padded
tensor (which favours PyTorch by that copy).

    python tools/dwconv_bench.py [--batch 32] [--iters 20] [--rounds 7]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azure_hc_intel_tf_amd.models import create_model  # noqa: E402
from azure_hc_intel_tf_amd.ops import _ext  # noqa: E402
from azure_hc_intel_tf_amd.ops import functional as Fn  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    N = args.batch
    problems = [(b.dw.in_shape, b.dw.stride, b.dw.pads) for b in create_model("mobilenet", device="cpu").blocks]
    _ext.set_act("bf16")
    print(f"# batch {N}, {args.iters} launches per round, median of {args.rounds} rounds, random data")
    print("# dtype  H   C  s | fwd us  GB/s  torch us | dgrad us  GB/s | wgrad us  GB/s | torch bwd us | cache")
    slower = []
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        Fn.set_f32_native(name == "fp32")
        e = 4 if name == "fp32" else 2
        for (H, W, C), s, (pt, pb, pl, pr) in problems:
            P, Q = (H + pt + pb - 3) // s + 1, (W + pl + pr - 3) // s + 1
            x = torch.randn(N, H, W, C, device="cuda").to(dt)
            dz = torch.randn(N, P, Q, C, device="cuda").to(dt)
            w = torch.randn(C, 3, 3, device="cuda") * 0.3
            z, dx, dw = torch.empty_like(dz), torch.empty_like(x), torch.empty_like(w)
            ws = Fn.dwconv_wgrad_workspace(x.shape, dz.shape, "cuda")
            xt = x.permute(0, 3, 1, 2)  # NCHW view of NHWC memory: channels-last
            if pt == pb and pl == pr:
                pad = (pt, pl)
            else:  # padded once, untimed; still channels-last
                xt = F.pad(xt, (pl, pr, pt, pb)).contiguous(memory_format=torch.channels_last)
                pad = (0, 0)
            xt = xt.detach().requires_grad_(True)
            wt = w.to(dt).view(C, 1, 3, 3).detach().requires_grad_(True)
            dzt = dz.permute(0, 3, 1, 2)

            def t_fwd():
                with torch.no_grad():
                    return F.conv2d(xt, wt, stride=s, padding=pad, groups=C)

            zt = F.conv2d(xt, wt, stride=s, padding=pad, groups=C)
            assert zt.shape == dzt.shape
            ops = {
                "fwd": lambda: Fn.dwconv_forward(x, w, z, s, pt, pl),
                "dgrad": lambda: Fn.dwconv_dgrad(dz, w, dx, s, pt, pl),
                "wgrad": lambda: Fn.dwconv_wgrad(dz, x, dw, s, pt, pl, ws=ws),
                "t_fwd": t_fwd,
                "t_bwd": lambda: torch.autograd.grad(zt, (xt, wt), dzt, retain_graph=True),
            }
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            nb = (x.numel() + dz.numel()) * e
            gbs = {k: nb / (m[k] * 1e-6) / 1e9 for k in ("fwd", "dgrad", "wgrad")}
            # every buffer the interleaved variants of this problem touch (x, dx, z, dz and PyTorch's
            # copies of them) against the 256 MiB cache: "part" = they do not all stay resident
            cache = "cold" if nb > 256 << 20 else ("part" if 3 * nb > 256 << 20 else "warm")
            print(f"{name:5s} {H:4d} {C:4d} {s:2d} | {m['fwd']:7.1f} {gbs['fwd']:6.0f} {m['t_fwd']:8.1f} | "
                  f"{m['dgrad']:7.1f} {gbs['dgrad']:6.0f} | {m['wgrad']:7.1f} {gbs['wgrad']:6.0f} | {m['t_bwd']:9.1f} | {cache}")
            if m["fwd"] > m["t_fwd"]:
                slower.append((name, H, C, s, "fwd", round(gbs["fwd"])))
            if m["dgrad"] + m["wgrad"] > m["t_bwd"]:
                slower.append((name, H, C, s, "bwd", round(min(gbs["dgrad"], gbs["wgrad"]))))
    Fn.set_f32_native(False)
    print("# slower than PyTorch (dtype, H, C, stride, which, GB/s):", slower or "none")


if __name__ == "__main__":
    main()
