#!/usr/bin/env python3
"""Write a small CIFAR-10-format dataset (the six python pickles, seeded random bytes, labels in
[0, 9]) for exercising ``--data_name=cifar10 --data_dir=...`` without the real dataset:

    python tools/make_fake_cifar10.py /tmp/fake_cifar10 --per_file 64

Files are named like the standard set (``data_batch_1 .. data_batch_5``, ``test_batch``) and hold what
``pickle.load(f, encoding="bytes")`` expects: ``b"data"`` uint8 [n, 3072], ``b"labels"`` a list of n ints.
"""
import argparse
import os
import pickle

import numpy as np

FILES = tuple(f"data_batch_{i}" for i in range(1, 6)) + ("test_batch",)


def make(out_dir, per_file=64, seed=0):
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    paths = []
    for name in FILES:
        data = rng.integers(0, 256, size=(per_file, 3072), dtype=np.uint8)
        labels = [int(v) for v in rng.integers(0, 10, size=per_file)]
        p = os.path.join(out_dir, name)
        with open(p, "wb") as f:
            pickle.dump({b"batch_label": name.encode(), b"labels": labels, b"data": data,
                         b"filenames": [f"{name}_{i}.png".encode() for i in range(per_file)]}, f, protocol=2)
        paths.append(p)
    return paths


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--per_file", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    for p in make(a.out_dir, a.per_file, a.seed):
        print(p)
