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
                                            the captured HIP graph reads; with colour
                                            distortion or another resize method the
                                            ``preprocess_distort`` kernels instead (below)

A background thread keeps ``depth`` batches in flight, so host decode overlaps the GPU step;
with fewer CPU cores than the GPU can consume, the run is input-bound and the log says so
(the headline benchmark uses synthetic data, as BASELINE.json specifies).
Eval mode (``train=False``) uses the 87.5 % central crop without flips; ``loop=False`` reads the
split exactly once (``--eval``), padding the short last batch with label -1 rows.
Normalisation x/127.5 - 1 is this engine's convention (parity with the TF build unpinned).

Distortions (tf_cnn_benchmarks' ``--distortions`` / ``--resize_method``; the loader's ``distort``,
``color`` and ``resize_method`` arguments). ``distort=False`` trains on the eval crop: shuffled train
shards, 87.5 % central crop, no flip, no colour, bilinear. ``color=True`` adds upstream's
``distort_color`` after the resize: brightness x + db, saturation (s <- clamp(s * fs, 0, 1) in HSV),
hue (h <- frac(h + dh)) and contrast ((x - m) * fc + m, m the per-channel mean of the image at that
point), on x = v / 255, as brightness-saturation-hue-contrast at even batch positions and
brightness-contrast-saturation-hue at odd ones, then clamp to [0, 1]. The producer thread, the only
one that draws, takes db ~ U(-32/255, 32/255), fs ~ U(0.5, 1.5), dh ~ U(-0.2, 0.2), fc ~ U(0.5, 1.5)
from a numpy Generator seeded with (seed, rank), so a seed reproduces a run. ``resize_method`` is
nearest | bilinear | bicubic | area, or round_robin = batch position % 4 in that order (upstream also
rotates it with the global step; not reproduced). bicubic is Keys cubic convolution (a = -0.75) with
weights from the exact fraction, not TF's 1024-entry weight table (parity unpinned). The defaults
(crop + flip, no colour, bilinear) keep the ``preprocess_images`` kernel; anything else runs
``preprocess_distort`` (csrc/kernels/distort.hip) on the GPU and ``preprocess_distort_reference``,
the definition of both, on ``--device=cpu``.

GPU JPEG decode (``gpu_decode=True``, ``--gpu_jpeg_decode``; data/jpeg.py). The decode pool calls the
native entropy decoder (csrc/data/jpeg.cpp, GIL released) once per sample with the destination inside
the pinned slot: image i of a batch owns ``coef_budget(max_side)`` bytes there, 3 bytes per source pixel
of a max_side x max_side window (about 2.4 MB at 224 px), and an image whose window needs more is
declined. The records go to the device one copy per image, ``jpeg_idct`` and ``jpeg_crop_rgb`` write the
RGB crops into ``dev_stage`` under the usual (offset, h, w, flip) rows, and the preprocess kernels run
unchanged. Declined images (progressive, CMYK, PNG, damaged, over budget, reduced crop over max_side)
are decoded by ``decode_crop`` and uploaded into ``dev_stage`` behind the kernel-written crops, so a
batch may mix both; ``gpu_decoded`` / ``gpu_declined`` / ``decline_reasons`` count them. Crop windows,
flips, labels, shuffle order and distortion draws do not depend on the flag; the reduced crop is
(h // r, w // r) by the r x r box mean instead of Pillow's DCT-domain draft. On ``--device=cpu``
``jpeg_decode_reference`` runs in place of the kernels.
"""
from __future__ import annotations

import io
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import jpeg as _jpeg
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


RESIZE_METHODS = ("nearest", "bilinear", "bicubic", "area")  # method codes 0..3; round_robin cycles them


def distort_work_numel(batch: int, size: int) -> int:
    """float32 elements of scratch ``preprocess_distort`` needs: the per-block partial sums of the
    contrast mean, 4 per 256-pixel block of every image."""
    return batch * ((size * size + 255) // 256) * 4


def _keys_weights(t: torch.Tensor):
    """Keys cubic-convolution weights (a = -0.75) of the taps at -1, 0, 1, 2 for the fraction t."""
    a = -0.75
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    return [((a * x0 - 5 * a) * x0 + 8 * a) * x0 - 4 * a, ((a + 2) * x1 - (a + 3)) * x1 * x1 + 1,
            ((a + 2) * x2 - (a + 3)) * x2 * x2 + 1, ((a * x3 - 5 * a) * x3 + 8 * a) * x3 - 4 * a]


def resize_reference(img: torch.Tensor, S: int, flip: int, method: int) -> torch.Tensor:
    """``img`` [h, w, 3] (float32 or float64, values 0..255) -> [S, S, 3] in the same dtype: TF1
    resizing, source coordinate dst * in / out, the flip applied to the output x."""
    dt = img.dtype
    h, w = img.shape[:2]
    yo = torch.arange(S)
    xo = S - 1 - torch.arange(S) if flip else torch.arange(S)
    if method == 1:  # preprocess_reference's bilinear, operation for operation
        ys = yo.to(dt) * (h / float(S))
        xs = xo.to(dt) * (w / float(S))
        y0 = ys.long().clamp(max=h - 1)
        x0 = xs.long().clamp(max=w - 1)
        y1 = (y0 + 1).clamp(max=h - 1)
        x1 = (x0 + 1).clamp(max=w - 1)
        ly = (ys - y0.to(dt)).view(S, 1, 1)
        lx = (xs - x0.to(dt)).view(1, S, 1)
        a = img[y0][:, x0]
        b = img[y0][:, x1]
        cc = img[y1][:, x0]
        d = img[y1][:, x1]
        top = a + (b - a) * lx
        bot = cc + (d - cc) * lx
        return top + (bot - top) * ly
    if method == 0:  # index (dst * in) / out in integers
        return img[(yo * h) // S][:, (xo * w) // S]
    if method == 2:  # Keys bicubic, taps clamped to the edge, weights from the exact fraction
        iy, ix = (yo * h) // S, (xo * w) // S
        wy = _keys_weights((yo * h - iy * S).to(dt) / S)
        wx = _keys_weights((xo * w - ix * S).to(dt) / S)
        v = torch.zeros(S, S, 3, dtype=dt)
        for i in range(4):
            rows = img[(iy + i - 1).clamp(0, h - 1)]
            row = torch.zeros(S, S, 3, dtype=dt)
            for j in range(4):
                row = row + wx[j].view(1, S, 1) * rows[:, (ix + j - 1).clamp(0, w - 1)]
            v = v + wy[i].view(S, 1, 1) * row
        return v
    if method == 3:  # area: overlap of [i*in/out, (i+1)*in/out) with each source pixel, in 1/out units
        def overlap(dst, n):
            lo = (dst * n).view(S, 1)
            j = torch.arange(n).view(1, n)
            return (torch.minimum((j + 1) * S, lo + n) - torch.maximum(j * S, lo)).clamp(min=0).to(dt)

        return torch.einsum("yh,hwc,xw->yxc", overlap(yo, h), img, overlap(xo, w)) / float(h * w)
    raise ValueError(f"resize method {method}: 0 nearest | 1 bilinear | 2 bicubic | 3 area")


def _rgb_to_hcv(x: torch.Tensor):
    """RGB -> (hue in [0, 1], chroma = max - min = s * v, value = max): HSV with the saturation
    kept multiplied by the value, so nothing divides by a maximum that may be <= 0."""
    r, g, b = x.unbind(-1)
    mx, mn = x.max(-1).values, x.min(-1).values
    d = mx - mn
    ds = torch.where(d > 0, d, torch.ones_like(d))
    h6 = torch.where(r == mx, (g - b) / ds, torch.where(g == mx, 2 + (b - r) / ds, 4 + (r - g) / ds))
    h = torch.where(d > 0, h6, torch.zeros_like(d)) / 6
    return h - torch.floor(h), d, mx


def _hcv_to_rgb(h: torch.Tensor, c: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    h6 = h * 6
    fl = torch.floor(h6)
    f = h6 - fl
    i = (fl.long() % 6).unsqueeze(-1)
    p, q, t = v - c, v - c * f, v - c * (1 - f)
    r = torch.stack([v, q, p, p, t, v], -1).gather(-1, i)
    g = torch.stack([t, v, v, q, p, p], -1).gather(-1, i)
    b = torch.stack([p, p, t, v, v, q], -1).gather(-1, i)
    return torch.cat([r, g, b], -1)


def adjust_saturation(x: torch.Tensor, fs: float) -> torch.Tensor:
    """RGB -> HSV, s <- clamp(s * fs, 0, 1), HSV -> RGB (a pixel whose maximum is <= 0 turns grey)."""
    h, c, v = _rgb_to_hcv(x)
    return _hcv_to_rgb(h, torch.minimum(c * fs, v.clamp(min=0)), v)


def adjust_hue(x: torch.Tensor, dh: float) -> torch.Tensor:
    """RGB -> HSV, h <- frac(h + dh), HSV -> RGB."""
    h, c, v = _rgb_to_hcv(x)
    h = h + dh
    return _hcv_to_rgb(h - torch.floor(h), c, v)


def distort_color_reference(x: torch.Tensor, db: float, fs: float, dh: float, fc: float,
                            ordering: int) -> torch.Tensor:
    """The colour stage on one image x [S, S, 3] in 0..1 units (not yet clamped on entry)."""
    def contrast(x):
        m = x.mean(dim=(0, 1), keepdim=True)
        return (x - m) * fc + m

    x = x + db
    if ordering == 0:
        x = contrast(adjust_hue(adjust_saturation(x, fs), dh))
    elif ordering == 1:
        x = adjust_hue(adjust_saturation(contrast(x), fs), dh)
    else:
        raise ValueError(f"colour ordering {ordering}: 0 or 1 (-1: no colour stage)")
    return x.clamp(0, 1)


def preprocess_distort_reference(crops: List[np.ndarray], flips: List[int], params, out: torch.Tensor,
                                 scale=SCALE, bias=BIAS, dtype=torch.float32) -> torch.Tensor:
    """Definition of the ``preprocess_distort`` HIP kernels and the CPU path of the distortions.
    ``params`` [B][8] float32: brightness delta, saturation factor, hue delta, contrast factor,
    colour ordering (0 | 1, -1 = no colour stage), resize method (0 nearest | 1 bilinear | 2 bicubic |
    3 area), 0, 0. Per image: resize the crop to S x S (``resize_reference``), the colour stage on
    v / 255 (``distort_color_reference``), v * scale + bias with scale and bias as float32 values,
    NHWC with zero pad channels. Arithmetic in ``dtype`` (float64: the tests' reference)."""
    S = out.shape[1]
    out.zero_()
    params = np.asarray(params, dtype=np.float32).reshape(-1, 8)
    sc = torch.tensor(scale, dtype=torch.float32).to(dtype)
    bi = torch.tensor(bias, dtype=torch.float32).to(dtype)
    for i, (c, fl) in enumerate(zip(crops, flips)):
        db, fs, dh, fc = (float(p) for p in params[i, :4])
        ordering, method = int(params[i, 4]), int(params[i, 5])
        if not (np.isfinite(params[i]).all() and fs >= 0 and fc >= 0 and params[i, 6] == 0 and params[i, 7] == 0):
            raise ValueError(f"distortion parameters of image {i}: {params[i].tolist()}")
        v = resize_reference(torch.from_numpy(np.array(c, dtype=np.uint8)).to(dtype), S, int(fl), method)
        if ordering != -1:
            v = 255 * distort_color_reference(v / 255, db, fs, dh, fc, ordering)
        out[i, :, :, :3] = (v * sc + bi).to(out.dtype)
    return out


_END = object()  # producer -> consumer: a loop=False pass is exhausted


class ImageNetLoader:
    """Fills a model's static (images, labels) buffers with the next real batch."""

    def __init__(self, data_dir: str, batch_size: int, image_size: int, channels: int, device,
                 rank: int = 0, world: int = 1, train: bool = True, seed: int = 0, reader_threads: int = 4,
                 decode_threads: int = 8, depth: int = 3, shuffle_buffer: int = 4096, subset: Optional[str] = None,
                 loop: bool = True, distort: bool = True, color: bool = False, resize_method: str = "bilinear",
                 gpu_decode: bool = False):
        self.B = batch_size
        # distort / color / resize_method: see the module docstring; evaluation loaders ignore them
        if resize_method != "round_robin" and resize_method not in RESIZE_METHODS:
            raise ValueError(f"resize_method {resize_method!r}: round_robin | " + " | ".join(RESIZE_METHODS))
        self.distort = bool(distort) or not train
        self.color = bool(color) and train and self.distort
        self.resize_method = resize_method if train and self.distort else "bilinear"
        # the defaults keep the preprocess_images kernel / preprocess_reference
        self.distort_op = self.color or self.resize_method != "bilinear"
        self._rng = np.random.default_rng([seed, rank])
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
                                      seed=seed, train=train, loop=loop, distort=self.distort)
        self.pool = ThreadPoolExecutor(max_workers=decode_threads, thread_name_prefix="hcb-decode")
        cap = batch_size * self.max_side * self.max_side * 3
        pin = self.device.type == "cuda"
        self.slots = [torch.empty(cap, dtype=torch.uint8, pin_memory=pin) for _ in range(depth)]
        self.dev_stage = torch.empty(cap, dtype=torch.uint8, device=self.device) if pin else None
        self.dev_desc = torch.empty((batch_size, 4), dtype=torch.int64, device=self.device) if pin else None
        if pin and self.distort_op:
            self.dev_params = torch.empty((batch_size, 8), dtype=torch.float32, device=self.device)
            self.dev_work = torch.empty(distort_work_numel(batch_size, image_size), dtype=torch.float32,
                                        device=self.device)
        # gpu_decode: every slot grows by one entropy-decoder record of coef_budget bytes per image, in
        # front of the RGB area that now only holds the crops of declined images
        self.gpu_decode = bool(gpu_decode)
        self.gpu_decoded = 0
        self.gpu_declined = 0
        self.decline_reasons: dict = {}
        self._gpu_info = [None] * depth  # per slot: the kernels' tables and copies of the batch it holds
        if self.gpu_decode:
            self.budget = _jpeg.coef_budget(self.max_side)
            self.coef_slots = [torch.empty(batch_size * self.budget, dtype=torch.uint8, pin_memory=pin)
                               for _ in range(depth)]
            if pin:
                self.dev_coef = torch.empty(batch_size * self.budget, dtype=torch.uint8, device=self.device)
                # one byte of plane per int16 coefficient
                self.dev_planes = torch.empty(batch_size * (self.budget // 2), dtype=torch.uint8, device=self.device)
                self.dev_segs = torch.empty((3 * batch_size, _jpeg.SEG_COLS), dtype=torch.int64, device=self.device)
                self.dev_imgs = torch.empty((batch_size, _jpeg.IMG_COLS), dtype=torch.int64, device=self.device)
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
    def _draw_params(self) -> np.ndarray:
        """[B][8] rows for preprocess_distort: one draw per image and batch, in batch order."""
        B = self.B
        prm = np.zeros((B, 8), dtype=np.float32)
        prm[:, 1] = prm[:, 3] = 1.0
        prm[:, 4] = -1.0
        pos = np.arange(B)
        prm[:, 5] = pos % 4 if self.resize_method == "round_robin" else RESIZE_METHODS.index(self.resize_method)
        if self.color:
            prm[:, 0] = self._rng.uniform(-32.0 / 255.0, 32.0 / 255.0, B)
            prm[:, 1] = self._rng.uniform(0.5, 1.5, B)
            prm[:, 2] = self._rng.uniform(-0.2, 0.2, B)
            prm[:, 3] = self._rng.uniform(0.5, 1.5, B)
            prm[:, 4] = pos % 2
        return prm

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
                if self.gpu_decode:
                    item = self._produce_gpu_decode(slot, samples, real)
                    self.decode_s += time.perf_counter() - t0
                    self.ready.put(item)
                    continue
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
                prm = self._draw_params() if self.distort_op else None
                self.decode_s += time.perf_counter() - t0
                self.ready.put((slot, desc, labels, crops if self.device.type != "cuda" else None, real, prm))
        except Exception as e:  # surfaced on the consumer side
            self._err = e
            self.ready.put(None)

    def _produce_gpu_decode(self, slot: int, samples, real: int):
        """One batch with gpu_decode: entropy-decode every sample into its record of the slot (decode
        pool), fall back to decode_crop per declined image, lay out the stage (GPU crops first, in batch
        order, then the fallback crops) and build the kernels' tables. Descriptor order is batch order."""
        nat = native()
        cbuf = self.coef_slots[slot].numpy()
        budget = self.budget
        on_gpu = self.device.type == "cuda"

        def work(i):
            s = samples[i]
            res = nat.jpeg_entropy_decode(s[0], s[2], cbuf[i * budget:(i + 1) * budget])
            if isinstance(res, str):
                return res, None, decode_crop(s[0], s[2], s[4], self.S, self.max_side)
            hdr, qt, coef = _jpeg.parse_record(cbuf[i * budget:i * budget + res])
            r = _jpeg.reduction(hdr["ch"], hdr["cw"], self.S)
            if max(hdr["ch"] // r, hdr["cw"] // r) > self.max_side:
                return "declined: reduced crop over max_side", None, decode_crop(s[0], s[2], s[4], self.S, self.max_side)
            if not on_gpu:  # the definition is the CPU path
                return None, (hdr, r), _jpeg.jpeg_decode_reference(coef, hdr, qt, r)
            return None, (hdr, r), None

        res = list(self.pool.map(work, range(real)))
        desc = np.zeros((self.B, 4), dtype=np.int64)
        headers, rs, crops = [None] * self.B, [1] * self.B, [None] * self.B
        off = 0
        for i, (why, hr, crop) in enumerate(res):  # kernel-written crops first
            if why is not None:
                self.gpu_declined += 1
                self.decline_reasons[why[len("declined: "):]] = self.decline_reasons.get(why[len("declined: "):], 0) + 1
                continue
            self.gpu_decoded += 1
            headers[i], rs[i] = hr
            oh, ow = hr[0]["ch"] // hr[1], hr[0]["cw"] // hr[1]
            desc[i] = (off, oh, ow, samples[i][3])
            crops[i] = crop
            off += (oh * ow * 3 + 15) // 16 * 16
        gpu_bytes = off
        buf = self.slots[slot].numpy()
        for i, (why, hr, crop) in enumerate(res):  # then the Pillow-decoded ones, packed from the slot's start
            if why is None:
                continue
            n = crop.size
            buf[off - gpu_bytes:off - gpu_bytes + n] = crop.reshape(-1)
            desc[i] = (off, crop.shape[0], crop.shape[1], samples[i][3])
            crops[i] = crop
            off += (n + 15) // 16 * 16
        desc[real:] = desc[0]  # padding rows of a short last batch: the first image again (no second decode)
        crops[real:] = [crops[0]] * (self.B - real)
        labels = np.full(self.B, -1, dtype=np.int64)
        labels[:real] = [s[1] for s in samples]
        prm = self._draw_params() if self.distort_op else None
        gpu = None
        if on_gpu:
            segs, imgs, plane_bytes, _ = _jpeg.build_tables(headers, [i * budget for i in range(self.B)], rs)
            copies = [(i * budget, headers[i]["nbytes"]) for i in range(self.B) if headers[i] is not None]
            gpu = (segs, imgs, copies, gpu_bytes, off - gpu_bytes)
        self._gpu_info[slot] = gpu  # the slot is the producer's until the item is taken, then the consumer's
        return slot, desc, labels, None if on_gpu else crops, real, prm

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
        slot, desc, lab, crops, real, prm = item
        gpu = self._gpu_info[slot] if self.gpu_decode else None
        if self.device.type == "cuda":
            from ..ops import _ext

            desc_t = torch.from_numpy(desc)
            self.dev_desc.copy_(desc_t, non_blocking=True)
            labels.copy_(torch.from_numpy(lab), non_blocking=True)
            if gpu is None:
                nbytes = int(desc[real - 1, 0] + desc[real - 1, 1] * desc[real - 1, 2] * 3)
                self.dev_stage[:nbytes].copy_(self.slots[slot][:nbytes], non_blocking=True)
            else:
                segs, imgs, copies, gpu_bytes, fb_bytes = gpu
                for o, n in copies:  # one record per GPU-decoded image
                    self.dev_coef[o:o + n].copy_(self.coef_slots[slot][o:o + n], non_blocking=True)
                if fb_bytes:  # the Pillow-decoded crops, behind the kernel-written ones
                    self.dev_stage[gpu_bytes:gpu_bytes + fb_bytes].copy_(self.slots[slot][:fb_bytes], non_blocking=True)
                if len(copies):
                    segs_t, imgs_t = torch.from_numpy(segs), torch.from_numpy(imgs)
                    dev_segs = self.dev_segs[:segs.shape[0]]
                    dev_segs.copy_(segs_t, non_blocking=True)
                    self.dev_imgs.copy_(imgs_t, non_blocking=True)
                    _ext.ops().jpeg_idct(self.dev_coef, dev_segs, segs_t, self.dev_planes)
                    _ext.ops().jpeg_crop_rgb(self.dev_planes, self.dev_imgs, imgs_t, self.dev_desc, desc_t, self.dev_stage)

            if prm is None:
                _ext.ops().preprocess_images(self.dev_stage, self.dev_desc, desc_t, images, list(SCALE), list(BIAS))
            else:
                prm_t = torch.from_numpy(prm)
                self.dev_params.copy_(prm_t, non_blocking=True)
                _ext.ops().preprocess_distort(self.dev_stage, self.dev_desc, desc_t, self.dev_params, prm_t, images,
                                              self.dev_work, list(SCALE), list(BIAS))
            ev = torch.cuda.Event()
            ev.record()
            self.free.put((slot, ev))
        else:
            if prm is None:
                preprocess_reference(crops, [int(d[3]) for d in desc], images)
            else:
                preprocess_distort_reference(crops, [int(d[3]) for d in desc], prm, images)
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
