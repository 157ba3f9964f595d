"""CIFAR-10 input pipeline (``--data_name=cifar10 --data_dir=...``): the split lives on the device.

tf_cnn_benchmarks' second image dataset. There is nothing to decode: a split is 3,072 bytes per image
(the python pickles ``data_batch_1 .. data_batch_5`` / ``test_batch``: ``b"data"`` uint8 [n, 3072], planar
1,024 R + 1,024 G + 1,024 B, and ``b"labels"``), 153.6 MB for the 50,000 training images, so the loader
uploads it once and every step costs one H2D copy of ``B x 16`` bytes of descriptors plus ONE kernel
launch (``cifar_batch``, csrc/kernels/cifar.hip) that gathers, pads, crops, flips and normalises the
batch and gathers its labels, writing IN PLACE into the static input buffers the captured step graph
reads. No threads, no staging of pixels, nothing per image on the host.

Preprocessing (upstream's Cifar10ImagePreprocessor, from memory -- not pinned against the upstream
source): training with distortions zero-pads the image to 40 x 40, takes a random 32 x 32 crop and flips
it with probability 1/2; evaluation, and training with ``--distortions=false``, take the image as it is.
Normalisation is this engine's x / 127.5 - 1 (``data.imagenet`` SCALE / BIAS), so a padded pixel is -1.0.
A descriptor row is (index, oy, ox, flip): crop offsets oy, ox in [0, 8] into the padded image (4, 4 =
the identity crop), index -1 = a padding row of a one-pass run's short last batch (all-zero image,
label -1, which ``eval_metrics`` skips). ``cifar_batch_reference`` is the definition, the
``--device=cpu`` path and, in float64, the tests' reference.

Order: a rank owns the strided share ``rank::world`` of the split; with ``train`` it draws a fresh
permutation of its share per epoch, and with ``train and distort`` the offsets and flips, all from
``np.random.default_rng([seed, rank])`` in batch order, so (seed, rank) reproduces a run on any device.
"""
from __future__ import annotations

import os
import pickle
from typing import Tuple

import numpy as np
import torch

from .imagenet import BIAS, SCALE

IMAGE_SIZE = 32
IMAGE_BYTES = 3 * IMAGE_SIZE * IMAGE_SIZE
NUM_CLASSES = 11  # upstream's Cifar10Dataset(num_classes=11), from memory; the labels are 0..9
NUM_TRAIN_IMAGES = 50000
NUM_VAL_IMAGES = 10000
TRAIN_FILES = tuple(f"data_batch_{i}" for i in range(1, 6))
VAL_FILES = ("test_batch",)
SUBDIR = "cifar-10-batches-py"
PAD = 4  # the zero border of the training crop: offsets are in [0, 2 * PAD]


def find_dir(data_dir: str, files) -> str:
    """``data_dir`` or its cifar-10-batches-py/ subdirectory, whichever holds the first of ``files``."""
    for d in (data_dir, os.path.join(data_dir, SUBDIR)):
        if os.path.isfile(os.path.join(d, files[0])):
            return d
    raise FileNotFoundError(f"no CIFAR-10 file {files[0]} in {data_dir} or {os.path.join(data_dir, SUBDIR)}")


def read_batch_file(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """One python pickle -> (uint8 [n, 3072], int64 [n])."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"CIFAR-10 file missing: {path}")
    with open(path, "rb") as f:
        d = pickle.load(f, encoding="bytes")
    if not isinstance(d, dict) or b"data" not in d or b"labels" not in d:
        raise ValueError(f"{path}: not a CIFAR-10 batch (a pickled dict with b'data' and b'labels')")
    data = np.asarray(d[b"data"])
    labels = np.asarray(d[b"labels"], dtype=np.int64)
    if data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != IMAGE_BYTES or labels.shape != (data.shape[0],):
        raise ValueError(f"{path}: expected uint8 data [n, {IMAGE_BYTES}] and n labels, found {data.dtype} "
                         f"{tuple(data.shape)} and {tuple(labels.shape)}")
    return np.ascontiguousarray(data), labels


def read_split(data_dir: str, train: bool) -> Tuple[np.ndarray, np.ndarray]:
    """The train (data_batch_1..5) or validation (test_batch) split: (uint8 [N, 3, 32, 32], int64 [N])."""
    files = TRAIN_FILES if train else VAL_FILES
    d = find_dir(data_dir, files)
    parts = [read_batch_file(os.path.join(d, f)) for f in files]
    data = np.concatenate([p[0] for p in parts]).reshape(-1, 3, IMAGE_SIZE, IMAGE_SIZE)
    return data, np.concatenate([p[1] for p in parts])


def check_desc(desc, n_images: int) -> None:
    """The range check of the ``cifar_batch`` binding, for the CPU path."""
    d = np.asarray(desc)
    if d.ndim != 2 or d.shape[1] != 4:
        raise ValueError("desc must be [B, 4] = (index, oy, ox, flip)")
    if ((d[:, 0] < -1) | (d[:, 0] >= n_images)).any():
        raise ValueError(f"cifar_batch: an index outside [-1, {n_images})")
    if ((d[:, 1:3] < 0) | (d[:, 1:3] > 2 * PAD)).any():
        raise ValueError(f"cifar_batch: a crop offset outside [0, {2 * PAD}]")
    if ((d[:, 3] != 0) & (d[:, 3] != 1)).any():
        raise ValueError("cifar_batch: flip must be 0 or 1")


def cifar_batch_reference(data: torch.Tensor, labels: torch.Tensor, desc, out: torch.Tensor,
                          labels_out: torch.Tensor = None, dtype=torch.float32):
    """Definition of the ``cifar_batch`` HIP kernel and the CPU path. ``data`` uint8 [N, 3, 32, 32],
    ``labels`` int64 [N], ``desc`` [B, 4] = (index | -1, oy, ox, flip), ``out`` [B, 32, 32, Cpad]:
      x' = 31 - x if flip else x;  r = y + oy - 4;  c = x' + ox - 4
      out[b, y, x, ch] = (data[index, ch, r, c] if 0 <= r, c < 32 else 0) * scale + bias    (ch < 3)
    with scale = 1 / 127.5 and bias = -1 as float32 values, channels 3.. zero; an index -1 row is an
    all-zero image with label -1. Arithmetic in ``dtype`` (float64: the tests' reference), rounded once
    to ``out``'s dtype. Returns (out, labels_out)."""
    d = torch.as_tensor(np.asarray(desc), dtype=torch.int64)
    check_desc(d.numpy(), data.shape[0])
    B, S = d.shape[0], IMAGE_SIZE
    idx, oy, ox, flip = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    real = idx >= 0
    yy = torch.arange(S).view(1, S, 1)
    xx = torch.arange(S).view(1, 1, S)
    xs = torch.where(flip.view(B, 1, 1) == 1, S - 1 - xx, xx)
    r = (yy + oy.view(B, 1, 1) - PAD).expand(B, S, S)
    c = (xs + ox.view(B, 1, 1) - PAD).expand(B, S, S)
    inside = (r >= 0) & (r < S) & (c >= 0) & (c < S) & real.view(B, 1, 1)
    src = data.cpu()[idx.clamp(min=0)]  # [B, 3, 32, 32]
    raw = src[torch.arange(B).view(B, 1, 1), :, r.clamp(0, S - 1), c.clamp(0, S - 1)]  # [B, 32, 32, 3]
    raw = torch.where(inside.unsqueeze(-1), raw, torch.zeros_like(raw)).to(dtype)
    sc = torch.tensor(SCALE, dtype=torch.float32).to(dtype)
    bi = torch.tensor(BIAS, dtype=torch.float32).to(dtype)
    v = raw * sc + bi
    v = torch.where(real.view(B, 1, 1, 1), v, torch.zeros_like(v))
    out.zero_()
    out[..., :3] = v.to(out.dtype)
    lab = torch.where(real, labels.cpu()[idx.clamp(min=0)], torch.full_like(idx, -1))
    if labels_out is None:
        labels_out = lab
    else:
        labels_out.copy_(lab)
    return out, labels_out


class Cifar10Loader:
    """Fills a model's static (images, labels) buffers with the next CIFAR-10 batch: ``ImageNetLoader``'s
    consumer interface (``next_into(images, labels) -> real rows``, ``close()``), no threads."""

    SLOTS = 4  # pinned descriptor blocks in flight (an H2D copy must finish before its block is rewritten)
    decode_s = 0.0  # (the summary's input_decode_s: there is no decode)

    def __init__(self, data_dir: str, batch_size: int, device, rank: int = 0, world: int = 1, train: bool = True,
                 seed: int = 0, loop: bool = True, distort: bool = True):
        data, labels = read_split(data_dir, train)
        self.B = int(batch_size)
        self.N = int(data.shape[0])
        self.device = torch.device(device)
        self.train = bool(train)
        self.random_crop = bool(train and distort)
        self.loop = bool(loop)
        self.files = [os.path.join(find_dir(data_dir, TRAIN_FILES if train else VAL_FILES), f)
                      for f in (TRAIN_FILES if train else VAL_FILES)]
        self.share = np.arange(self.N, dtype=np.int64)[rank::world]
        if len(self.share) == 0:
            raise ValueError(f"CIFAR-10 split of {self.N} images has none for rank {rank} of {world}")
        self._rng = np.random.default_rng([seed, rank])
        self._order = np.empty(0, dtype=np.int64)
        self._pos = 0
        self._epochs = 0
        self._exhausted = False
        self.batches = 0
        self.last_desc = None  # the descriptors of the latest batch (tests, diagnostics)
        self.data = torch.from_numpy(data).to(self.device)  # the ONE upload of the split
        self.labels_all = torch.from_numpy(labels).to(self.device)
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu:
            self._slots = [torch.empty((self.B, 4), dtype=torch.int32, pin_memory=True) for _ in range(self.SLOTS)]
            self._events = [None] * self.SLOTS
            self.dev_desc = torch.empty((self.B, 4), dtype=torch.int32, device=self.device)

    def _next_indices(self) -> np.ndarray:
        """The next B indices of this rank's share (-1 past the end of a one-pass run)."""
        out = np.full(self.B, -1, dtype=np.int64)
        n = 0
        while n < self.B:
            if self._pos == len(self._order):
                if self._epochs and not self.loop:
                    break
                self._order = self._rng.permutation(self.share) if self.train else self.share
                self._pos = 0
                self._epochs += 1
            k = min(self.B - n, len(self._order) - self._pos)
            out[n:n + k] = self._order[self._pos:self._pos + k]
            self._pos += k
            n += k
        return out

    def _next_desc(self) -> Tuple[np.ndarray, int]:
        idx = self._next_indices()
        real = int((idx >= 0).sum())
        desc = np.empty((self.B, 4), dtype=np.int32)
        desc[:, 0] = idx
        desc[:, 1:3] = PAD
        desc[:, 3] = 0
        if self.random_crop and real:
            desc[:, 1:3] = self._rng.integers(0, 2 * PAD + 1, size=(self.B, 2))
            desc[:, 3] = self._rng.integers(0, 2, size=self.B)
        return desc, real

    def next_into(self, images: torch.Tensor, labels: torch.Tensor) -> int:
        """Write the next batch into ``images`` [B, 32, 32, C] / ``labels`` [B] in place (stream ordered on
        the current stream). Returns the number of real rows: B, or with ``loop=False`` fewer for the
        padded last batch (label -1 rows) and 0, with the buffers untouched, once the pass is over."""
        if self._exhausted:
            return 0
        desc, real = self._next_desc()
        if real == 0:
            self._exhausted = True
            return 0
        self.last_desc = desc
        if self.on_gpu:
            from ..ops import _ext

            slot = self.batches % self.SLOTS
            if self._events[slot] is not None:
                self._events[slot].synchronize()  # the copy out of this block, SLOTS batches ago, is done
            host = self._slots[slot]
            host.numpy()[...] = desc
            self.dev_desc.copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._events[slot] = ev
            _ext.ops().cifar_batch(self.data, self.labels_all, self.dev_desc, host, images, labels)
        else:
            cifar_batch_reference(self.data, self.labels_all, desc, images, labels,
                                  dtype=images.dtype if images.dtype == torch.float64 else torch.float32)
        self.batches += 1
        return real

    def close(self):
        pass
