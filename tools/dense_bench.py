#!/usr/bin/env python
"""The fused DenseNet dense-layer kernel (csrc/kernels/dense3x3.hip, Fn.dense_conv3x3_forward) against the
unfused chain of existing kernels on the same padded layout -- bn_apply_acc writes the normalised operand
of the C_in channels, then the conv GEMM (16 output channels) reads it back and writes the slot -- on the
dense-layer shapes of densenet40_k12 (three blocks of 12 layers, 32 / 16 / 8 pixels, 16-channel slots), fp32
and bf16, same machine, same process.

Method (as tools/dwconv_bench.py): every form is warmed up, then timed as ITERS back-to-back launches
between two events; the median of ROUNDS rounds is reported, the forms interleaved round by round, and the
fused form is timed twice (A/A) so the spread of the method shows beside the ratio. Inputs are random. All
of these layers' tensors stay in the 256 MiB Infinity Cache between launches, so the numbers are warm-cache
ones. The unfused chain is not charged the accumulator copy it needs (its apply kernel takes statistics
with C_in columns, the fused one the buffer's).

--wgrad times the weight gradient of the same layers instead: the fused kernel (csrc/kernels/dense3x3_wgrad.hip,
Fn.dense_conv3x3_wgrad: two launches, partials + fold) against bn_apply_acc re-materialising the operand and
conv_wgrad reading it back, by the same method (the unfused chain is again not charged its accumulator copy,
nor the fp32 path's split of dz, which the data gradient needs either way).

--dgrad times the data gradient with the ReLU and BatchNorm backward of the same layers: the fused op
(csrc/kernels/dense3x3_dgrad.hip, Fn.dense_conv3x3_dgrad: three launches, reduce + fold + apply) against
conv_dgrad writing the operand's gradient and bn_backward_acc (bn_bwd_reduce_acc + bn_bwd_apply_acc) reading it
back, by the same method. The unfused chain is charged the fp32 path's split of dz (to_planes: with the fused
weight gradient nothing else needs it); it is not charged the per-step zeroing of its statistics accumulator.

--preact times the pre-activation conv of the CIFAR ResNet-v2 blocks instead (csrc/kernels/preact3x3.hip,
Fn.preact_conv3x3_forward: one launch, output statistics included) against bn_apply_acc writing the operand and
the existing conv GEMM (statistics in its epilogue) reading it back, on the five layer shapes of those models
(default batch 128 there: pass --batch 128), by the same method. Neither side is charged bn_stats_acc.

--preact-wgrad times the weight gradient of those five layers: the fused kernel (csrc/kernels/preact3x3_wgrad.hip,
Fn.preact_conv3x3_wgrad: two launches, partials + fold) against bn_apply_acc re-materialising the operand and
conv_wgrad reading it back, by the same method. The fused side is not charged the fp32 path's merge of dz's Planes
(the layer gets dz as Planes from conv1's BN backward), the unfused side not its split.

--preact-block times the whole pre-activation block of 16-bit inference on those five geometries: the one-launch
kernel (csrc/kernels/preact_block.hip, Fn.preact_block_inference) against today's chain -- bn_inference,
conv_bn_inference and the conv with the residual add -- in bf16 and fp16, by the same method. shortcut_pad_fwd, which
both sides run on the two stride-2 blocks, is timed beside them and charged to neither.

    python tools/dense_bench.py [--batch 64] [--iters 20] [--rounds 7] [--all]
                                [--wgrad | --dgrad | --preact | --preact-wgrad | --preact-block]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azure_hc_intel_tf_amd.nn.layers import empty_act, empty_op, set_gpu_compute_dtype  # noqa: E402
from azure_hc_intel_tf_amd.nn.params import ParamStore  # noqa: E402
from azure_hc_intel_tf_amd.ops import functional as Fn  # noqa: E402
from azure_hc_intel_tf_amd.ops.functional import ConvSpec  # noqa: E402

K, SLOT, EPS, R = 12, Fn.DENSE_SLOT, 1e-5, 8


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def layer_shapes(n: int, every: bool):
    """(H, C_in) of the dense layers: block b starts at C0 (16, then the padded width of the block before)."""
    out, c0 = [], 16
    for H in (32, 16, 8):
        idx = range(n) if every else sorted({0, n // 2, n - 1})
        out += [(H, c0 + SLOT * i) for i in idx]
        c0 += SLOT * n
    return out


def wgrad_main(args):
    N = args.batch
    print(f"# weight gradient: batch {N}, {args.iters} launches per round, median of {args.rounds} rounds, random data, "
          "warm cache")
    print("# dtype  H  C_in | fused us  fused(A/A) us | bn apply us + wgrad us = unfused us | unfused / fused | fused GB/s")
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        set_gpu_compute_dtype(dt)
        Fn.set_f32_native(name == "fp32")
        e = 4 if name == "fp32" else 2
        for H, C in layer_shapes(12, args.all):
            M = N * H * H
            buf = torch.randn(N, H, H, C + SLOT, device="cuda").to(dt)
            G = torch.randn(N, H, H, C + SLOT, device="cuda").to(dt)
            spec = ConvSpec(cin=C, cin_pad=C, cout=SLOT, kh=3, kw=3, pt=1, pl=1, pb=1, pr=1)
            gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
            x = buf[..., :C].float().reshape(M, C)
            acc_c = torch.zeros(R, 2, C, device="cuda")
            acc_c[:, 0], acc_c[:, 1] = x.sum(0) / R, (x * x).sum(0) / R
            sv = torch.empty(2, C, device="cuda")
            op = empty_op((N, H, H, C), "cuda")
            dw = torch.zeros(SLOT, 9 * C, device="cuda")
            ws = Fn.dense_wgrad_workspace(buf.shape, C, dt, "cuda")
            dz = G[..., C:]
            dzp = Fn.to_planes(dz) if name == "fp32" else dz

            def bn():
                Fn.bn_forward_acc(buf[..., :C], gamma, beta, None, None, 1.0, EPS, op, True, acc_c, R, sv[0], sv[1])

            def fused():
                Fn.dense_conv3x3_wgrad(buf, C, dz, gamma, beta, sv[0], sv[1], dw, K, ws=ws)

            def wgrad():
                Fn.conv_wgrad(dzp, op, spec, dw)

            ops = {"bn": bn, "fused": fused, "fused2": fused, "conv": wgrad}
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            un = m["bn"] + m["conv"]
            gbs = M * (C + SLOT) * e / (m["fused"] * 1e-6) / 1e9  # algorithmic bytes: the input once, the slot once
            print(f"{name:5s} {H:3d} {C:5d} | {m['fused']:8.1f} {m['fused2']:8.1f} | {m['bn']:8.1f} + {m['conv']:8.1f} = "
                  f"{un:8.1f} | {un / m['fused']:5.2f} | {gbs:6.0f}", flush=True)
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def dgrad_main(args):
    N = args.batch
    print(f"# data gradient + BN-ReLU backward: batch {N}, {args.iters} launches per round, median of {args.rounds} "
          "rounds, random data, warm cache")
    print("# dtype  H  C_in | fused us  fused(A/A) us | split us + dgrad us + bn bwd us = unfused us | unfused / fused | fused GB/s")
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        set_gpu_compute_dtype(dt)
        Fn.set_f32_native(name == "fp32")
        e = 4 if name == "fp32" else 2
        for H, C in layer_shapes(12, args.all):
            M = N * H * H
            buf = torch.randn(N, H, H, C + SLOT, device="cuda").to(dt)
            G = (torch.randn(N, H, H, C + SLOT, device="cuda") * 1e-3).to(dt)
            spec = ConvSpec(cin=C, cin_pad=C, cout=SLOT, kh=3, kw=3, pt=1, pl=1, pb=1, pr=1)
            ps = ParamStore(seed=0)
            p = ps.add("w", (SLOT, 3, 3, C), True, ps.trunc_normal((2.0 / 9 / K) ** 0.5))
            pk = ps.add_pack(p, SLOT, 3, 3, C, spec.Kpad, spec.Kpad_t, want_tr=True)
            ps.finalize("cuda", pack_lo=name == "fp32")
            p.data[K:] = 0  # the pad rows
            ps.repack()
            gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
            x = buf[..., :C].float().reshape(M, C)
            mean = x.mean(0)
            invstd = torch.rsqrt(x.var(0, unbiased=False) + EPS)
            dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            acc_b = torch.zeros(R, 2, C, device="cuda")
            da = empty_act((N, H, H, C), "cuda")
            ws = Fn.dense_dgrad_workspace(buf.shape, C, dt, "cuda")
            dz, gin = G[..., C:], G[..., :C]
            dzp = [Fn.to_planes(dz) if name == "fp32" else dz]

            def fused():
                Fn.dense_conv3x3_dgrad(buf, C, dz, p.data, gamma, beta, mean, invstd, gin, dg, db, K, ws=ws)

            def split():
                if name == "fp32":
                    dzp[0] = Fn.to_planes(dz)

            def dgrad():
                Fn.conv_dgrad(dzp[0], spec, pk.tr, p.data, da, False)

            def bnb():
                Fn.bn_backward_acc(da, None, buf[..., :C], Fn.BNSaved(mean, invstd), gamma, beta, 2, dg, db, gin, acc_b, R,
                                   add=gin)

            ops = {"fused": fused, "fused2": fused, "split": split, "conv": dgrad, "bn": bnb}
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            if name != "fp32":
                m["split"] = 0.0
            un = m["split"] + m["conv"] + m["bn"]
            gbs = M * 4 * C * e / (m["fused"] * 1e-6) / 1e9  # algorithmic bytes: x twice, gin read and written
            print(f"{name:5s} {H:3d} {C:5d} | {m['fused']:8.1f} {m['fused2']:8.1f} | {m['split']:6.1f} + {m['conv']:8.1f} + "
                  f"{m['bn']:8.1f} = {un:8.1f} | {un / m['fused']:5.2f} | {gbs:6.0f}", flush=True)
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


# (H, C_in, Nout, stride) of the pre-activation convs of resnet20_v2 .. resnet110_v2
PREACT_SHAPES = ((32, 16, 16, 1), (32, 16, 32, 2), (16, 32, 32, 1), (16, 32, 64, 2), (8, 64, 64, 1))


def preact_main(args):
    N = args.batch
    print(f"# pre-activation conv: batch {N}, {args.iters} launches per round, median of {args.rounds} rounds, random "
          "data, warm cache")
    print("# dtype  H  C_in Nout s | fused us  fused(A/A) us | bn apply us + conv us = unfused us | unfused / fused | fused GB/s")
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        set_gpu_compute_dtype(dt)
        Fn.set_f32_native(name == "fp32")
        e = 4 if name == "fp32" else 2
        for H, C, nout, s in PREACT_SHAPES:
            M, P = N * H * H, H // s
            x = torch.randn(N, H, H, C, device="cuda").to(dt)
            pads = Fn.same_pads(H, 3, s)
            spec = ConvSpec(cin=C, cin_pad=C, cout=nout, kh=3, kw=3, sh=s, sw=s, pt=pads[0], pl=pads[0], pb=pads[1],
                            pr=pads[1])
            ps = ParamStore(seed=0)
            p = ps.add("w", (nout, 3, 3, C), True, ps.variance_scaling(9 * C))
            pk = ps.add_pack(p, nout, 3, 3, C, spec.Kpad, spec.Kpad_t, want_tr=False)
            ps.finalize("cuda", dtype_pack=torch.bfloat16, pack_lo=name == "fp32")
            gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
            xf = x.float().reshape(M, C)
            acc = torch.zeros(R, 2, C, device="cuda")
            acc[:, 0], acc[:, 1] = xf.sum(0) / R, (xf * xf).sum(0) / R
            acc_o = torch.zeros(R, 2, nout, device="cuda")
            sv = torch.empty(2, C, device="cuda")
            op = empty_op((N, H, H, C), "cuda")  # the normalised operand of the unfused chain (Planes on fp32)
            z = empty_act((N, P, P, nout), "cuda")

            def fused():
                Fn.preact_conv3x3_forward(x, p.data, gamma, beta, EPS, z, s, acc=acc, R=R, out_stats=acc_o, out_stats_R=R,
                                          saved_mean=sv[0], saved_invstd=sv[1], wpack=pk.pack)

            def bn():
                Fn.bn_forward_acc(x, gamma, beta, None, None, 1.0, EPS, op, True, acc, R, sv[0], sv[1])

            def conv():
                Fn.conv_forward(op, spec, pk.pack, p.data, z, stats=acc_o, stats_R=R)

            ops = {"fused": fused, "fused2": fused, "bn": bn, "conv": conv}
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            un = m["bn"] + m["conv"]
            gbs = (M * C + N * P * P * nout) * e / (m["fused"] * 1e-6) / 1e9  # algorithmic bytes: x once, y once
            print(f"{name:5s} {H:3d} {C:4d} {nout:4d} {s} | {m['fused']:8.1f} {m['fused2']:8.1f} | {m['bn']:8.1f} + "
                  f"{m['conv']:8.1f} = {un:8.1f} | {un / m['fused']:5.2f} | {gbs:6.0f}", flush=True)
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def preact_wgrad_main(args):
    N = args.batch
    print(f"# pre-activation conv weight gradient: batch {N}, {args.iters} launches per round, median of {args.rounds} "
          "rounds, random data, warm cache")
    print("# dtype  H  C_in Nout s | fused us  fused(A/A) us | bn apply us + wgrad us = unfused us | unfused / fused | fused GB/s")
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        set_gpu_compute_dtype(dt)
        Fn.set_f32_native(name == "fp32")
        e = 4 if name == "fp32" else 2
        for H, C, nout, s in PREACT_SHAPES:
            M, P = N * H * H, H // s
            x = torch.randn(N, H, H, C, device="cuda").to(dt)
            dz = torch.randn(N, P, P, nout, device="cuda").to(dt)
            pads = Fn.same_pads(H, 3, s)
            spec = ConvSpec(cin=C, cin_pad=C, cout=nout, kh=3, kw=3, sh=s, sw=s, pt=pads[0], pl=pads[0], pb=pads[1],
                            pr=pads[1])
            gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
            xf = x.float().reshape(M, C)
            acc = torch.zeros(R, 2, C, device="cuda")
            acc[:, 0], acc[:, 1] = xf.sum(0) / R, (xf * xf).sum(0) / R
            sv = torch.empty(2, C, device="cuda")
            op = empty_op((N, H, H, C), "cuda")  # the re-materialised operand of the unfused chain (Planes on fp32)
            dw = torch.zeros(nout, 9 * C, device="cuda")
            ws = Fn.preact_wgrad_workspace(x.shape, C, nout, s, dt, "cuda")
            dzp = Fn.to_planes(dz) if name == "fp32" else dz

            def bn():
                Fn.bn_forward_acc(x, gamma, beta, None, None, 1.0, EPS, op, True, acc, R, sv[0], sv[1])

            def fused():
                Fn.preact_conv3x3_wgrad(x, C, dz, gamma, beta, sv[0], sv[1], dw, s, ws=ws)

            def wgrad():
                Fn.conv_wgrad(dzp, op, spec, dw)

            ops = {"bn": bn, "fused": fused, "fused2": fused, "conv": wgrad}
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            un = m["bn"] + m["conv"]
            gbs = (M * C + N * P * P * nout) * e / (m["fused"] * 1e-6) / 1e9  # algorithmic bytes: x once, dz once
            print(f"{name:5s} {H:3d} {C:4d} {nout:4d} {s} | {m['fused']:8.1f} {m['fused2']:8.1f} | {m['bn']:8.1f} + "
                  f"{m['conv']:8.1f} = {un:8.1f} | {un / m['fused']:5.2f} | {gbs:6.0f}", flush=True)
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


def preact_block_main(args):
    N = args.batch
    print(f"# pre-activation block, 16-bit inference: batch {N}, {args.iters} launches per round, median of {args.rounds} "
          "rounds, random data, warm cache")
    print("# dtype  H  C_in Nout s | block us  block(A/A) us | bn us + conv1 us + conv2 us (+ pad us) = chain us | "
          "chain / block | block GB/s")
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        set_gpu_compute_dtype(dt)
        for H, C, nout, s in PREACT_SHAPES:
            P = H // s
            x = torch.randn(N, H, H, C, device="cuda").to(dt)
            pads = Fn.same_pads(H, 3, s)
            s1 = ConvSpec(cin=C, cin_pad=C, cout=nout, kh=3, kw=3, sh=s, sw=s, pt=pads[0], pl=pads[0], pb=pads[1], pr=pads[1])
            s2 = ConvSpec(cin=nout, cin_pad=nout, cout=nout, kh=3, kw=3, pt=1, pl=1, pb=1, pr=1)
            w1 = torch.randn(nout, 3, 3, C, device="cuda") * (2.0 / 9 / C) ** 0.5
            w2 = torch.randn(nout, 3, 3, nout, device="cuda") * (2.0 / 9 / nout) ** 0.5
            pk1, pk2 = Fn.dense_pack(w1, dt)[0], Fn.dense_pack(w2, dt)[0]
            bn1, bn2 = [[torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.1,
                         torch.randn(c, device="cuda") * 0.1, torch.rand(c, device="cuda") + 0.5] for c in (C, nout)]
            a1 = empty_act((N, H, H, C), "cuda")
            a2, res, out = (empty_act((N, P, P, nout), "cuda") for _ in range(3))
            res.copy_(torch.randn(N, P, P, nout, device="cuda"))

            def block():
                Fn.preact_block_inference(x, w1, *bn1, EPS, w2, *bn2, EPS, res if C != nout else x, out, s, wpack1=pk1,
                                          wpack2=pk2)

            def bn():
                Fn.bn_inference(x, *bn1, EPS, a1, True)

            def conv1():
                Fn.conv_bn_inference(a1, s1, pk1, w1, *bn2, EPS, a2, True)

            def conv2():
                Fn.conv_forward(a2, s2, pk2, w2, out, residual=res if C != nout else x)

            def pad():
                Fn.shortcut_pad_forward(x, res, s)

            ops = {"block": block, "block2": block, "bn": bn, "conv1": conv1, "conv2": conv2}
            if C != nout:
                ops["pad"] = pad  # (both sides run it on the two stride-2 blocks; the chain is not charged it)
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            un = m["bn"] + m["conv1"] + m["conv2"]
            gbs = (N * H * H * C + 2 * N * P * P * nout) * 2 / (m["block"] * 1e-6) / 1e9  # x once, res once, out once
            print(f"{name:5s} {H:3d} {C:4d} {nout:4d} {s} | {m['block']:8.1f} {m['block2']:8.1f} | {m['bn']:8.1f} + "
                  f"{m['conv1']:8.1f} + {m['conv2']:8.1f} (+ {m.get('pad', 0.0):5.1f}) = {un:8.1f} | {un / m['block']:5.2f} | "
                  f"{gbs:6.0f}", flush=True)
    set_gpu_compute_dtype(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--all", action="store_true", help="every layer (default: first, middle and last of each block)")
    ap.add_argument("--wgrad", action="store_true", help="the weight gradient instead of the forward pass")
    ap.add_argument("--dgrad", action="store_true", help="the data gradient with the BN-ReLU backward instead")
    ap.add_argument("--preact", action="store_true", help="the CIFAR ResNet-v2 pre-activation conv instead")
    ap.add_argument("--preact-wgrad", action="store_true", help="the weight gradient of the pre-activation conv instead")
    ap.add_argument("--preact-block", action="store_true", help="the one-launch 16-bit inference block against its chain")
    args = ap.parse_args()
    if args.preact_block:
        return preact_block_main(args)
    if args.preact_wgrad:
        return preact_wgrad_main(args)
    if args.preact:
        return preact_main(args)
    if args.wgrad:
        return wgrad_main(args)
    if args.dgrad:
        return dgrad_main(args)
    N = args.batch
    print(f"# batch {N}, {args.iters} launches per round, median of {args.rounds} rounds, random data, warm cache")
    print("# dtype  H  C_in | fused us  fused(A/A) us | bn apply us + conv us = unfused us | unfused / fused | fused GB/s")
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        set_gpu_compute_dtype(dt)
        Fn.set_f32_native(name == "fp32")
        e = 4 if name == "fp32" else 2
        for H, C in layer_shapes(12, args.all):
            M = N * H * H
            buf = torch.randn(N, H, H, C + SLOT, device="cuda").to(dt)
            spec = ConvSpec(cin=C, cin_pad=C, cout=SLOT, kh=3, kw=3, pt=1, pl=1, pb=1, pr=1)
            ps = ParamStore(seed=0)
            p = ps.add("w", (SLOT, 3, 3, C), True, ps.trunc_normal((2.0 / 9 / K) ** 0.5))
            pk = ps.add_pack(p, SLOT, 3, 3, C, spec.Kpad, spec.Kpad_t, want_tr=False)
            ps.finalize("cuda", pack_lo=name == "fp32")
            p.data[K:] = 0  # the pad rows
            ps.repack()
            gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
            x = buf[..., :C].float().reshape(M, C)
            acc = torch.zeros(R, 2, C + SLOT, device="cuda")
            acc[:, 0, :C], acc[:, 1, :C] = x.sum(0) / R, (x * x).sum(0) / R
            acc_c = acc[:, :, :C].contiguous()
            acc_o = torch.zeros(R, 2, SLOT, device="cuda")
            sv = torch.empty(2, C, device="cuda")
            op = empty_op((N, H, H, C), "cuda")  # the normalised operand of the unfused chain (Planes on fp32)
            slot = buf[..., C:C + SLOT]

            def fused():
                Fn.dense_conv3x3_forward(buf, C, C, p.data[:K], gamma, beta, EPS, acc=acc, R=R, saved_mean=sv[0],
                                         saved_invstd=sv[1], stats=acc, stats_R=R, wpack=pk.pack)

            def bn():
                Fn.bn_forward_acc(buf[..., :C], gamma, beta, None, None, 1.0, EPS, op, True, acc_c, R, sv[0], sv[1])

            def conv():
                Fn.conv_forward(op, spec, pk.pack, p.data, slot, stats=acc_o, stats_R=R)

            ops = {"fused": fused, "fused2": fused, "bn": bn, "conv": conv}
            for fn in ops.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in ops}
            for _ in range(args.rounds):
                for k, fn in ops.items():
                    t[k].append(timed(fn, args.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            un = m["bn"] + m["conv"]
            gbs = M * (C + SLOT) * e / (m["fused"] * 1e-6) / 1e9  # algorithmic bytes: the input once, the slot once
            print(f"{name:5s} {H:3d} {C:5d} | {m['fused']:8.1f} {m['fused2']:8.1f} | {m['bn']:8.1f} + {m['conv']:8.1f} = "
                  f"{un:8.1f} | {un / m['fused']:5.2f} | {gbs:6.0f}")
    Fn.set_f32_native(False)
    set_gpu_compute_dtype(torch.bfloat16)


if __name__ == "__main__":
    main()
