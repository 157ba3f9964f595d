#!/usr/bin/env python
"""Kernel time of the real-data preprocessing ops on one batch: ``preprocess_images`` (bilinear,
no colour) against ``preprocess_distort`` (colour + each resize method), same crops, one process,
device events around ``--iters`` back-to-back calls after ``--warmup`` calls.

  python tools/distort_bench.py [--batch 64] [--size 224] [--iters 200] [--warmup 20]

Crop sizes follow what the loader hands over after the decoder's DCT downscale: each side between
1x and 2x the output size. Prints one line per op and dtype with the time per call and the output
bytes written per second."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from azure_hc_intel_tf_amd.data.imagenet import BIAS, SCALE, distort_work_numel
    from azure_hc_intel_tf_amd.ops import _ext

    assert torch.cuda.is_available(), "distort_bench needs the GPU"
    ops = _ext.ops()
    B, S = a.batch, a.size
    rng = np.random.default_rng(0)
    off, desc, chunks = 0, [], []
    for i in range(B):
        h, w = (int(v) for v in rng.integers(S, 2 * S, size=2))
        c = rng.integers(0, 256, size=h * w * 3, dtype=np.uint8)
        desc.append((off, h, w, i & 1))
        pad = (-c.size) % 16
        chunks += [c, np.zeros(pad, dtype=np.uint8)]
        off += c.size + pad
    src = torch.from_numpy(np.concatenate(chunks)).cuda()
    desc_h = torch.tensor(desc, dtype=torch.int64)
    desc_d = desc_h.cuda()
    work = torch.empty(distort_work_numel(B, S), dtype=torch.float32, device="cuda")
    print(f"B={B} S={S} source {src.numel() / 1e6:.1f} MB, {a.iters} calls after {a.warmup} warm-up calls")

    def params(colour, method):
        p = np.zeros((B, 8), dtype=np.float32)
        p[:, 1] = p[:, 3] = 1
        p[:, 4] = -1
        p[:, 5] = np.arange(B) % 4 if method < 0 else method
        if colour:
            p[:, 0] = rng.uniform(-32 / 255, 32 / 255, B)
            p[:, 1] = rng.uniform(0.5, 1.5, B)
            p[:, 2] = rng.uniform(-0.2, 0.2, B)
            p[:, 3] = rng.uniform(0.5, 1.5, B)
            p[:, 4] = np.arange(B) % 2
        return torch.from_numpy(p)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3  # us per call

    for dtype in (torch.float32, torch.bfloat16):
        out = torch.empty(B, S, S, 8, dtype=dtype, device="cuda")
        nbytes = out.numel() * out.element_size()
        rows = [("preprocess_images (bilinear)",
                 lambda: ops.preprocess_images(src, desc_d, desc_h, out, list(SCALE), list(BIAS)))]
        for name, colour, method in [("distort bilinear, no colour", False, 1), ("distort bilinear + colour", True, 1),
                                     ("distort nearest + colour", True, 0), ("distort bicubic + colour", True, 2),
                                     ("distort area + colour", True, 3), ("distort round_robin + colour", True, -1)]:
            ph = params(colour, method)
            pd = ph.cuda()
            rows.append((name, lambda ph=ph, pd=pd: ops.preprocess_distort(src, desc_d, desc_h, pd, ph, out, work,
                                                                           list(SCALE), list(BIAS))))
        for name, fn in rows:
            us = timed(fn)
            print(f"{str(dtype).replace('torch.', ''):9s} {name:32s} {us:9.1f} us/call  "
                  f"{nbytes / us / 1e3:8.1f} GB/s written (host checks and launches included)")


if __name__ == "__main__":
    main()
