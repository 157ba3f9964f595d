"""Host decode stage alone: images per second of decode_crop (Pillow) against the native JPEG entropy
decoder, over the same fake-ImageNet records and the same crop windows, at 1 and N threads, in
interleaved rounds (A B A B ...), with the spread. With --gpu also the isolated times of the jpeg_idct and
jpeg_crop_rgb kernels for one batch (device events around each launch, warmed up).

  python tools/jpeg_decode_bench.py --dir <fake set> [--images 256] [--threads 1 16] [--rounds 5] [--gpu]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def samples_of(data_dir, n, seed):
    from azure_hc_intel_tf_amd.data.tfrecord import find_shards, native

    pf = native().Prefetcher(find_shards(data_dir, "train"), threads=1, shuffle_buffer=1, capacity=8192, seed=seed,
                             train=True, loop=True)
    out = pf.next(n)
    pf.stop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--gpu", action="store_true")
    a = ap.parse_args()
    from azure_hc_intel_tf_amd.data import jpeg as J
    from azure_hc_intel_tf_amd.data.imagenet import decode_crop
    from azure_hc_intel_tf_amd.data.tfrecord import native

    nat = native()
    S, max_side = a.size, 4 * a.size
    budget = J.coef_budget(max_side)
    smp = samples_of(a.dir, a.images, 0)
    src_bytes = sum(len(s[0]) for s in smp)
    print(f"{len(smp)} images, mean JPEG {src_bytes / len(smp) / 1024:.1f} KiB, mean crop "
          f"{np.mean([s[2][2] * s[2][3] for s in smp]) / 1e3:.1f} kpx, out {S}")
    for nt in a.threads:
        bufs = [np.zeros(budget, dtype=np.uint8) for _ in range(nt)]
        pool = ThreadPoolExecutor(max_workers=nt)

        def pillow(i):
            s = smp[i]
            return decode_crop(s[0], s[2], s[4], S, max_side).size

        def entropy(i):
            s = smp[i]
            r = nat.jpeg_entropy_decode(s[0], s[2], bufs[i % nt])
            return 0 if isinstance(r, str) else r

        rates = {"pillow": [], "native": []}
        declined = sum(1 for r in pool.map(entropy, range(len(smp))) if r == 0)  # warm-up, both
        list(pool.map(pillow, range(len(smp))))
        for _ in range(a.rounds):
            for name, fn in (("pillow", pillow), ("native", entropy)):
                t0 = time.perf_counter()
                list(pool.map(fn, range(len(smp))))
                rates[name].append(len(smp) / (time.perf_counter() - t0))
        pool.shutdown()
        for name, r in rates.items():
            print(f"threads={nt:2d} {name:6s} img/s: median {np.median(r):8.1f}  min {min(r):8.1f}  max {max(r):8.1f}  "
                  f"({a.rounds} interleaved rounds)")
        print(f"threads={nt:2d} native / pillow (medians): {np.median(rates['native']) / np.median(rates['pillow']):.2f}x, "
              f"declined {declined} of {len(smp)}")
    if a.gpu:
        import torch

        from azure_hc_intel_tf_amd.ops import _ext

        B = min(64, len(smp))
        coef = torch.empty(B * budget, dtype=torch.uint8).pin_memory()
        cb = coef.numpy()
        headers, rs = [None] * B, [1] * B
        desc = np.zeros((B, 4), dtype=np.int64)
        off = 0
        for i in range(B):
            r = nat.jpeg_entropy_decode(smp[i][0], smp[i][2], cb[i * budget:(i + 1) * budget])
            if isinstance(r, str):
                desc[i] = desc[0]
                continue
            hdr = J.parse_record(cb[i * budget:i * budget + r])[0]
            headers[i], rs[i] = hdr, J.reduction(hdr["ch"], hdr["cw"], S)
            desc[i] = (off, hdr["ch"] // rs[i], hdr["cw"] // rs[i], 0)
            off += (int(desc[i, 1] * desc[i, 2]) * 3 + 15) // 16 * 16
        segs, imgs, plane_bytes, groups = J.build_tables(headers, [i * budget for i in range(B)], rs)
        dcoef = coef.cuda()
        planes = torch.empty(plane_bytes, dtype=torch.uint8, device="cuda")
        stage = torch.empty(off, dtype=torch.uint8, device="cuda")
        segs_h, imgs_h, desc_h = torch.from_numpy(segs), torch.from_numpy(imgs), torch.from_numpy(desc)
        dsegs, dimgs, ddesc = segs_h.cuda(), imgs_h.cuda(), desc_h.cuda()
        ops = _ext.ops()
        t_idct, t_crop = [], []
        for it in range(25):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            ops.jpeg_idct(dcoef, dsegs, segs_h, planes)
            e[1].record()
            ops.jpeg_crop_rgb(planes, dimgs, imgs_h, ddesc, desc_h, stage)
            e[2].record()
            torch.cuda.synchronize()
            if it >= 5:
                t_idct.append(e[0].elapsed_time(e[1]))
                t_crop.append(e[1].elapsed_time(e[2]))
        nblk = int(segs[:, 1].sum())
        print(f"bs={B}: {nblk} blocks ({nblk * 128 / 1e6:.1f} MB of coefficients), {off / 1e6:.1f} MB of RGB crops, "
              f"reductions {sorted(set(rs))}")
        print(f"jpeg_idct     ms: median {np.median(t_idct):.3f} min {min(t_idct):.3f} max {max(t_idct):.3f} "
              f"(event-timed, includes the host-side checks of the launch)")
        print(f"jpeg_crop_rgb ms: median {np.median(t_crop):.3f} min {min(t_crop):.3f} max {max(t_crop):.3f}")


if __name__ == "__main__":
    main()
