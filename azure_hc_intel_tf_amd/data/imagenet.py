"""Real-ImageNet input pipeline (``--data_dir``): native prefetch -> JPEG decode -> GPU resize.

tf_cnn_benchmarks' ImageNet training preprocessing (SURVEY.md §2.2 "preprocessing.py +
datasets.py"; the reference points ``--data_dir`` at 20 TFRecord shards,
/root/reference/benchmark-scripts/run-tf-sing-ucx-openmpi.sh:19,80) rebuilt for one process
per MI355X:

  C++ prefetcher (csrc/data/tfrecord.cpp)   reader threads over this rank's shards, CRC check,
                                            Example parse, shuffle pool, crop window
                                            (sample_distorted_bounding_box) + flip coin
  -> decode pool (Pillow, GIL released)     JPEG DCT-domain downscale ("draft") when the crop
                                            is >= 2x the output, crop, RGB uint8
  -> pinned staging slot                    crops packed back to back
  -> one H2D copy + HIP preprocess kernel   bilinear resize, flip, x/127.5 - 1, NHWC bf16
                                            written IN PLACE into the static input buffer
                                            the captured HIP graph reads

A background thread keeps ``depth`` batches in flight, so host decode overlaps the GPU step;
with fewer CPU cores than the GPU can consume, the run is input-bound and the log says so
(the headline benchmark uses synthetic data, as BASELINE.json specifies).
Eval mode (``train=False``) uses the 87.5 % central crop without flips; ``loop=False`` reads the
split exactly once (``--eval``), padding the short last batch with label -1 rows.
Normalisation x/127.5 - 1 is this engine's convention (parity with the TF build unpinned).
"""
from __future__ import annotations

import io
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Tuple

import numpy as np
import torch

from .tfrecord import find_shards, native

SCALE = (1.0 / 127.5,) * 3
BIAS = (-1.0,) * 3


def decode_crop(jpeg: bytes, win: Tuple[int, int, int, int], full_hw: Tuple[int, int], out_size: int,
                max_side: int) -> np.ndarray:
    """Decode ``jpeg`` and return the crop window (y, x, h, w in full-resolution pixels) as
    contiguous RGB uint8, DCT-downscaled while every side stays >= out_size and capped at
    max_side per side."""
    from PIL import Image

    img = Image.open(io.BytesIO(jpeg))
    H, W = full_hw
    if H <= 0 or W <= 0:
        W, H = img.size
    y, x, h, w = win
    if h <= 0 or w <= 0:
        y, x, h, w = 0, 0, H, W
    red = 1
    while red < 8 and min(h, w) // (red * 2) >= out_size:
        red *= 2
    if red > 1 and img.format == "JPEG":
        img.draft("RGB", (max(1, W // red), max(1, H // red)))
    img = img.convert("RGB")
    sw, sh = img.size
    fy, fx = sh / float(H), sw / float(W)
    box = (int(x * fx), int(y * fy), max(int(x * fx) + 1, int(round((x + w) * fx))),
           max(int(y * fy) + 1, int(round((y + h) * fy))))
    box = (min(box[0], sw - 1), min(box[1], sh - 1), min(box[2], sw), min(box[3], sh))
    crop = img.crop(box)
    cw, ch = crop.size
    if max(cw, ch) > max_side:
        s = max_side / float(max(cw, ch))
        crop = crop.resize((max(1, int(cw * s)), max(1, int(ch * s))), Image.BILINEAR)
    return np.asarray(crop, dtype=np.uint8)


def preprocess_reference(crops: List[np.ndarray], flips: List[int], out: torch.Tensor,
                         scale=SCALE, bias=BIAS) -> torch.Tensor:
    """PyTorch reference of the HIP kernel (CPU path / tests): TF1 resize_bilinear
    (src = dst * in / out), optional flip, x*scale+bias, NHWC with zero pad channels."""
    S = out.shape[1]
    out.zero_()
    for i, (c, fl) in enumerate(zip(crops, flips)):
        img = torch.from_numpy(np.array(c, dtype=np.uint8)).float()
        h, w = img.shape[:2]
        ys = torch.arange(S, dtype=torch.float32) * (h / float(S))
        xo = torch.arange(S)
        xs = (S - 1 - xo if fl else xo).float() * (w / float(S))
        y0 = ys.long().clamp(max=h - 1)
        x0 = xs.long().clamp(max=w - 1)
        y1 = (y0 + 1).clamp(max=h - 1)
        x1 = (x0 + 1).clamp(max=w - 1)
        ly = (ys - y0.float()).view(S, 1, 1)
        lx = (xs - x0.float()).view(1, S, 1)
        a = img[y0][:, x0]
        b = img[y0][:, x1]
        cc = img[y1][:, x0]
        d = img[y1][:, x1]
        top = a + (b - a) * lx
        bot = cc + (d - cc) * lx
        v = top + (bot - top) * ly
        v = v * torch.tensor(scale) + torch.tensor(bias)
        out[i, :, :, :3] = v.to(out.dtype)
    return out


_END = object()  # producer -> consumer: a loop=False pass is exhausted


class ImageNetLoader:
    """Fills a model's static (images, labels) buffers with the next real batch."""

    def __init__(self, data_dir: str, batch_size: int, image_size: int, channels: int, device,
                 rank: int = 0, world: int = 1, train: bool = True, seed: int = 0, reader_threads: int = 4,
                 decode_threads: int = 8, depth: int = 3, shuffle_buffer: int = 4096, subset: Optional[str] = None,
                 loop: bool = True):
        self.B = batch_size
        # loop=False: ONE pass over this rank's share of the split (evaluation): a short last batch
        # is padded (label -1, an already-decoded image repeated) and next_into returns the number
        # of real rows, 0 once the data is exhausted
        self.loop = loop
        self._exhausted = False
        self.S = image_size
        self.C = channels
        self.device = torch.device(device)
        self.train = train
        if subset is None and not train:
            # inference (--forward_only): the validation shards when the directory has them, else the
            # train shards (a train-only set, e.g. a benchmark copy), still with the eval preprocessing
            try:
                self.files = find_shards(data_dir, "validation")
            except FileNotFoundError:
                self.files = find_shards(data_dir, "train")
        else:
            self.files = find_shards(data_dir, subset or ("train" if train else "validation"))
        self.max_side = 4 * image_size
        self.pf = native().Prefetcher(self.files, rank=rank, world=world, threads=reader_threads,
                                      shuffle_buffer=shuffle_buffer if train else 1, capacity=max(8192, shuffle_buffer),
                                      seed=seed, train=train, loop=loop)
        self.pool = ThreadPoolExecutor(max_workers=decode_threads, thread_name_prefix="hcb-decode")
        cap = batch_size * self.max_side * self.max_side * 3
        pin = self.device.type == "cuda"
        self.slots = [torch.empty(cap, dtype=torch.uint8, pin_memory=pin) for _ in range(depth)]
        self.dev_stage = torch.empty(cap, dtype=torch.uint8, device=self.device) if pin else None
        self.dev_desc = torch.empty((batch_size, 4), dtype=torch.int64, device=self.device) if pin else None
        self.free: "queue.Queue" = queue.Queue()
        for i in range(depth):
            self.free.put((i, None))
        self.ready: "queue.Queue" = queue.Queue(maxsize=depth)
        self.decode_s = 0.0
        self.batches = 0
        self._stop = False
        self._err = None
        self._thr = threading.Thread(target=self._produce, name="hcb-input", daemon=True)
        self._thr.start()

    # ---------------------------------------------------------------- producer thread
    def _produce(self):
        import time

        try:
            while not self._stop:
                slot, ev = self.free.get()
                if slot is None:
                    return
                if ev is not None:
                    ev.synchronize()  # the previous H2D copy out of this slot has finished
                t0 = time.perf_counter()
                samples = self.pf.next(self.B)
                real = len(samples)
                if real < self.B:
                    if self.loop:
                        raise RuntimeError("input pipeline ran dry")
                    if real == 0:  # one pass done: the consumer returns 0 from here on
                        self.ready.put(_END)
                        return
                crops = list(self.pool.map(
                    lambda s: decode_crop(s[0], s[2], s[4], self.S, self.max_side), samples))
                buf = self.slots[slot].numpy()
                desc = np.zeros((self.B, 4), dtype=np.int64)
                off = 0
                for i, (c, s) in enumerate(zip(crops, samples)):
                    n = c.size
                    buf[off:off + n] = c.reshape(-1)
                    desc[i] = (off, c.shape[0], c.shape[1], s[3])
                    off += (n + 15) // 16 * 16
                desc[real:] = desc[0]  # padding rows of a short last batch: the first image again
                crops += [crops[0]] * (self.B - real)
                labels = np.full(self.B, -1, dtype=np.int64)
                labels[:real] = [s[1] for s in samples]
                self.decode_s += time.perf_counter() - t0
                self.ready.put((slot, desc, labels, crops if self.device.type != "cuda" else None, real))
        except Exception as e:  # surfaced on the consumer side
            self._err = e
            self.ready.put(None)

    # ---------------------------------------------------------------- consumer
    def next_into(self, images: torch.Tensor, labels: torch.Tensor) -> int:
        """Write the next batch into ``images`` [B, S, S, C] / ``labels`` [B] in place (stream
        ordered on the current stream, so a following graph replay sees it). Returns the number of
        real rows: the batch size, or with ``loop=False`` fewer for the padded last batch (its
        padding rows carry label -1) and 0, with the buffers untouched, once the data is exhausted."""
        if self._exhausted:
            return 0
        item = self.ready.get()
        if item is None:
            raise RuntimeError(f"input pipeline failed: {self._err!r}")
        if item is _END:
            self._exhausted = True
            return 0
        slot, desc, lab, crops, real = item
        if self.device.type == "cuda":
            nbytes = int(desc[real - 1, 0] + desc[real - 1, 1] * desc[real - 1, 2] * 3)
            self.dev_stage[:nbytes].copy_(self.slots[slot][:nbytes], non_blocking=True)
            desc_t = torch.from_numpy(desc)
            self.dev_desc.copy_(desc_t, non_blocking=True)
            labels.copy_(torch.from_numpy(lab), non_blocking=True)
            from ..ops import _ext

            _ext.ops().preprocess_images(self.dev_stage, self.dev_desc, desc_t, images, list(SCALE), list(BIAS))
            ev = torch.cuda.Event()
            ev.record()
            self.free.put((slot, ev))
        else:
            preprocess_reference(crops, [int(d[3]) for d in desc], images)
            labels.copy_(torch.from_numpy(lab))
            self.free.put((slot, None))
        self.batches += 1
        return real

    def close(self):
        self._stop = True
        self.free.put((None, None))
        try:
            self.pf.stop()
        except Exception:
            pass
        self.pool.shutdown(wait=False)
