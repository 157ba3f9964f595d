"""Tensor fusion for the hvd API: a persistent flat fp32 fusion buffer, filled from and drained
into a set of scattered tensors by ONE multi-tensor HIP launch each way
(``csrc/kernels/fusion.hip``; ops ``hcb.fusion_pack`` / ``hcb.fusion_unpack``).

    pack:    flat[off_i + j] = float(src_i[j]) * scale
    unpack:  dst_i[j]        = T_i(flat[off_i + j] * scale)

``fusion_layout`` places the tensors (every slot starts at a multiple of 4 floats; the padding is
zeroed once and never written again, so it reduces to zero) and cuts the buffer into the bucket
ranges the RCCL engine reduces. ``FusionBuffer`` owns the flat buffer and the device table of one
tensor set; ``fusion_pack_reference`` / ``fusion_unpack_reference`` are the same functions in
PyTorch: they define the kernels, serve CPU tensors and are the tests' reference.

Where the table is validated: the kernels trust the device table, so its host mirror is checked
here, in ``FusionBuffer._validate_layout`` (once, when the layout is built: ``off % 4 == 0``,
``off + n <= flat.numel()``, slots disjoint and in order) and ``FusionBuffer.bind`` (whenever a row
changes: dtype tag 0..2, element count equal to the slot's, contiguous, on the buffer's device,
pointer aligned to the element size).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

FUSION_CHUNK = 4096  # elements one workgroup handles at a time (csrc/kernels/kernels.h)
SLOT_ALIGN = 4  # floats: every slot is 16-byte aligned
TAGS = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
ROW = 5  # ptr, off, n, tag, chunk0


class FusionLayout(NamedTuple):
    offsets: List[int]  # slot offset of every tensor (elements, multiples of 4)
    total: int  # length of the flat buffer (a multiple of 4)
    ranges: List[Tuple[int, int]]  # bucket ranges (offset, n): they tile [0, total)


def _numel(t) -> int:
    return int(t) if isinstance(t, int) else int(t.numel())


def _layout(tensors: Sequence, bucket_bytes: int):
    """fusion_layout plus, per range, the run of entries [lo, hi) it holds."""
    pad = lambda n: (n + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN  # noqa: E731
    offsets, off = [], 0
    for t in tensors:
        offsets.append(off)
        off += pad(_numel(t))
    total = off
    limit = max(int(bucket_bytes) // 4, 1)
    ranges, runs = [], []
    lo, start = 0, 0
    for i, t in enumerate(tensors):
        size = pad(_numel(t))
        # cut in front of tensor i when it would push the open range over the threshold; a tensor
        # larger than the threshold therefore ends up alone (the engine cuts its range further)
        if i > lo and offsets[i] + size - start > limit and offsets[i] > start:
            ranges.append((start, offsets[i] - start))
            runs.append((lo, i))
            lo, start = i, offsets[i]
    if tensors:
        ranges.append((start, total - start))
        runs.append((lo, len(tensors)))
    return FusionLayout(offsets, total, ranges), runs


def fusion_layout(tensors: Sequence, bucket_bytes: int) -> FusionLayout:
    """Slots and bucket ranges for ``tensors`` (tensors, or plain element counts) in the given
    order: ``(offsets, total, ranges)``. Ranges are cut at tensor boundaries only and hold at most
    ``bucket_bytes`` of fp32, except that a single tensor larger than that is a range of its own."""
    return _layout(tensors, bucket_bytes)[0]


def fusion_pack_reference(tensors, scale: float, offsets=None, flat: Optional[torch.Tensor] = None,
                          entries: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """``flat[off_i + j] = float(src_i[j]) * scale`` in PyTorch (one fp32 multiply per element).
    ``flat`` defaults to a zeroed buffer of the layout's length; padding is not written."""
    if offsets is None or flat is None:
        lay = fusion_layout(tensors, 1 << 62)
        offsets = lay.offsets if offsets is None else offsets
        if flat is None:
            dev = tensors[0].device if len(tensors) else "cpu"
            flat = torch.zeros(lay.total, dtype=torch.float32, device=dev)
    lo, hi = entries if entries is not None else (0, len(tensors))
    for t, off in zip(tensors[lo:hi], offsets[lo:hi]):
        n = t.numel()
        if n:
            flat[off:off + n] = t.detach().reshape(-1).to(torch.float32) * scale
    return flat


def fusion_unpack_reference(flat: torch.Tensor, tensors, scale: float, offsets=None,
                            entries: Optional[Tuple[int, int]] = None):
    """``dst_i[j] = T_i(flat[off_i + j] * scale)`` in PyTorch, in place; returns ``tensors``."""
    if offsets is None:
        offsets = fusion_layout(tensors, 1 << 62).offsets
    lo, hi = entries if entries is not None else (0, len(tensors))
    with torch.no_grad():
        for t, off in zip(tensors[lo:hi], offsets[lo:hi]):
            n = t.numel()
            if n:
                t.copy_((flat[off:off + n] * scale).to(t.dtype).view_as(t))
    return tensors


class FusionBuffer:
    """The persistent flat fp32 buffer and the device table of one tensor set.

    The layout (slots, bucket ranges, per-range entry runs ``runs``) is fixed by the element counts
    at construction. Rows of the table are bound to tensors with ``bind`` (all of them at
    construction unless ``bind=False``); a row is rewritten, and the changed rows uploaded, only
    when the tensor's ``(data_ptr, dtype, numel)`` differs from the cached tuple -- e.g. after
    ``zero_grad(set_to_none=True)`` produced new ``.grad`` tensors. The bound tensors are kept
    alive here, so the pointers in the table stay valid."""

    def __init__(self, tensors: Sequence[torch.Tensor], bucket_bytes: Optional[int] = None, bind: bool = True):
        if bucket_bytes is None:
            from .reducer import fusion_threshold_bytes

            bucket_bytes = fusion_threshold_bytes()
        tensors = list(tensors)
        if not tensors:
            raise ValueError("FusionBuffer: empty tensor set")
        self.device = tensors[0].device
        self.numels = [int(t.numel()) for t in tensors]
        self.layout, self.runs = _layout(self.numels, bucket_bytes)
        self.offsets, self.total, self.ranges = self.layout
        self._validate_layout()
        chunks = [(n + FUSION_CHUNK - 1) // FUSION_CHUNK for n in self.numels]
        self._chunk0 = [0] * len(chunks)
        for i in range(1, len(chunks)):
            self._chunk0[i] = self._chunk0[i - 1] + chunks[i - 1]
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=self.device)  # padding: zero for good
        self._tensors: List[Optional[torch.Tensor]] = [None] * len(tensors)
        self._keys: List[Optional[tuple]] = [None] * len(tensors)
        self.rebuilds = 0  # table uploads so far
        self.table = None
        if self.device.type == "cuda":
            from ..ops import _ext

            self._ops = _ext.ops()
            if int(self._ops.fusion_chunk()) != FUSION_CHUNK:
                raise RuntimeError("FusionBuffer: FUSION_CHUNK differs from the kernel library's")
            # rows not bound yet hold a null pointer: pack / unpack refuse a run that has one (_run)
            self.table = torch.zeros(len(tensors), ROW, dtype=torch.int64, device=self.device)
        if bind:
            self.bind(tensors)

    def _validate_layout(self):
        end = 0
        for off, n in zip(self.offsets, self.numels):
            if off % SLOT_ALIGN or off < end or n < 0 or off + n > self.total:
                raise ValueError(f"FusionBuffer: bad slot (offset {off}, n {n}, previous end {end}, total {self.total})")
            end = off + n
        if self.total % SLOT_ALIGN:
            raise ValueError("FusionBuffer: total not padded")

    def __len__(self):
        return len(self.numels)

    def bind(self, tensors: Sequence[torch.Tensor], lo: int = 0) -> bool:
        """Bind rows ``lo .. lo + len(tensors)`` to ``tensors``; True if any row changed."""
        if lo < 0 or lo + len(tensors) > len(self):
            raise IndexError(f"FusionBuffer.bind: rows {lo}..{lo + len(tensors)} of {len(self)}")
        dlo, dhi = None, None
        for i, t in enumerate(tensors, lo):
            key = (t.data_ptr(), t.dtype, t.numel())
            if key == self._keys[i]:
                self._tensors[i] = t
                continue
            if t.dtype not in TAGS:
                raise TypeError(f"FusionBuffer: entry {i} has dtype {t.dtype}; float32, bfloat16 or float16 only")
            if t.numel() != self.numels[i]:
                raise ValueError(f"FusionBuffer: entry {i} has {t.numel()} elements, its slot {self.numels[i]} "
                                 "(a changed shape needs a new FusionBuffer)")
            if not t.is_contiguous():
                raise ValueError(f"FusionBuffer: entry {i} (shape {tuple(t.shape)}, strides {t.stride()}) is not "
                                 "contiguous; pass a contiguous tensor")
            if t.device != self.device:
                raise ValueError(f"FusionBuffer: entry {i} is on {t.device}, the buffer on {self.device}")
            if t.data_ptr() % t.element_size():
                raise ValueError(f"FusionBuffer: entry {i} is not aligned to its element size")
            self._tensors[i], self._keys[i] = t, key
            dlo, dhi = (i if dlo is None else dlo), i + 1
        if dlo is None:
            return False
        if self.table is not None:
            rows = [[self._keys[i][0], self.offsets[i], self.numels[i], TAGS[self._keys[i][1]], self._chunk0[i]]
                    if self._keys[i] is not None else [0, self.offsets[i], 0, 0, self._chunk0[i]]
                    for i in range(dlo, dhi)]
            self.table[dlo:dhi].copy_(torch.tensor(rows, dtype=torch.int64))
        self.rebuilds += 1
        return True

    def release(self) -> None:
        """Drop the references to the bound tensors but keep their cached tuples: memory freed by
        ``zero_grad(set_to_none=True)`` can then be handed out again, and a ``.grad`` that comes
        back at the same address rebuilds nothing. ``pack`` / ``unpack`` of an entry are refused
        until it is bound again (the hvd paths bind before every pack)."""
        self._tensors = [None] * len(self)

    def _run(self, entries):
        lo, hi = (0, len(self)) if entries is None else (int(entries[0]), int(entries[1]))
        if not 0 <= lo <= hi <= len(self):
            raise IndexError(f"FusionBuffer: entries {lo}..{hi} of {len(self)}")
        for i in range(lo, hi):
            if self._keys[i] is None or self._tensors[i] is None:
                raise RuntimeError(f"FusionBuffer: entry {i} is not bound to a tensor")
        return lo, hi

    def pack(self, scale: float = 1.0, entries: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """Fill the slots of ``entries`` (a contiguous run ``(lo, hi)``; default: all) -- one launch."""
        lo, hi = self._run(entries)
        if hi > lo:
            if self.table is not None:
                self._ops.fusion_pack(self.table[lo:hi], self.flat, float(scale))
            else:
                fusion_pack_reference(self._tensors, float(scale), self.offsets, self.flat, (lo, hi))
        return self.flat

    def unpack(self, scale: float = 1.0, entries: Optional[Tuple[int, int]] = None) -> None:
        """Write the slots of ``entries`` back into their tensors -- one launch."""
        lo, hi = self._run(entries)
        if hi > lo:
            if self.table is not None:
                self._ops.fusion_unpack(self.table[lo:hi], self.flat, float(scale))
            else:
                fusion_unpack_reference(self.flat, self._tensors, float(scale), self.offsets, (lo, hi))
