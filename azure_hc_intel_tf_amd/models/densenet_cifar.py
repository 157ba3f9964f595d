"""CIFAR-10 DenseNets as tf_cnn_benchmarks ``--model=densenet40_k12 | densenet100_k12 --data_name=cifar10``
builds them (upstream ``models/densenet_model.py`` ``DensenetCifar10Model``), input 32 x 32:

  conv 3x3 'SAME' (16, bias, no activation)
  -> three dense blocks of n = (depth - 4) / 3 layers, each BN (decay 0.9, epsilon 1e-5, scale) -> ReLU ->
     conv 3x3 (k = 12, truncated normal stddev sqrt(2 / 9 / k), no bias, no activation) -> concat
  -> after blocks 1 and 2 a transition: BN -> ReLU -> conv 1x1 keeping the channel count (stddev
     sqrt(2 / 9 / C), bias + ReLU as upstream's default ``conv``) -> average pool 2x2 / 2
  -> BN -> ReLU -> spatial mean -> affine -> classes.
Default batch 64; learning rate 0.1 / 0.01 / 0.001 / 0.0001 from epochs 150 / 225 / 300 of 50,000 images.
The architecture and the hyper-parameters follow upstream from memory; they are not pinned against the
upstream source.

Layout (``nn.layers.DenseBlock`` / ``dense_channel_mask``): a block's concat lives in one NHWC buffer with
the 12-channel growth slots padded to 16, so every kernel keeps its C % 8 == 0 contract; the pads are
structural zeros in activations, gradients and parameters, and parameter counts, checkpoints' logical
tensors and the L2 term are those of the real channels. The producer of a block's input (the first conv, a
transition's pool) writes straight into the buffer. The transition's 2x2 / 2 average pool runs as the
depthwise 3x3 / 2 kernel with the fixed weights 1/4 on its top-left 2x2 taps (csrc/kernels/dwconv.hip, forward and
data gradient): the pool kernels' fp32 backward takes the 3x3 / 1 average pool only, while the depthwise
kernels take 16-bit and plain fp32 tensors alike and write through a row stride.

``densenet100_k24`` is refused by name: its third block reaches 2,320 channels and the BatchNorm kernels
stop at C <= 2048.
"""
from __future__ import annotations

import math

import torch

from ..nn.layers import BNReLU, ConvBN, DenseBlock, GlobalAvgPool, Layer, Logits, empty_act, mask_param
from ..ops import functional as Fn
from .base import CNNModel

NUM_TRAIN_IMAGES = 50000


class AvgPool2(Layer):
    """Average pool 2x2 / 2 through the depthwise-conv kernels (see the module text); ``out``: where the
    pooled map goes (a dense block's input view)."""

    def __init__(self, name, in_shape):
        H, W, C = in_shape
        assert H % 2 == 0 and W % 2 == 0
        self.name, self.in_shape, self.out_shape = name, in_shape, (H // 2, W // 2, C)
        self._w = None

    def _weights(self, dev):
        if self._w is None or self._w.device != dev:
            w = torch.zeros(self.in_shape[2], 3, 3, dtype=torch.float32)
            w[:, :2, :2] = 0.25
            self._w = w.to(dev)
        return self._w

    def forward(self, x, out):
        return Fn.dwconv_forward(x, self._weights(x.device), out, 2, 0, 0)

    def backward(self, dy):
        dx = empty_act((dy.shape[0],) + tuple(self.in_shape), dy.device)
        return Fn.dwconv_dgrad(dy, self._weights(dy.device), dx, 2, 0, 0)


class DenseNetCifar(CNNModel):
    default_image_size = 32
    default_batch_size = 64
    F32_NATIVE_OK = True

    def __init__(self, depth: int = 40, growth: int = 12, layers_per_block: int = None, num_classes: int = 11, **kw):
        self.n = layers_per_block if layers_per_block is not None else (depth - 4) // 3
        self.k = growth
        assert (16 + self.k * self.n) % 8 == 0, "the transitions' channel count must be a multiple of 8"
        self.name = f"densenet{depth}_k{growth}"
        super().__init__(num_classes=num_classes, **kw)

    @staticmethod
    def lr_schedule(global_batch: int):
        per_epoch = int(NUM_TRAIN_IMAGES / global_batch)
        bounds, vals = [per_epoch * e for e in (150, 225, 300)], (0.1, 0.01, 0.001, 0.0001)

        def lr(step: int) -> float:
            for b, v in zip(bounds, vals):
                if step < b:
                    return v
            return vals[-1]

        return lr

    def build(self):
        ps, S = self.ps, self.image_size
        self.stem = ConvBN(ps, "conv0", (S, S, self.image_channels), 16, 3, 3, 1, 1, "SAME", relu=False, bn=False,
                           need_dx=False, logical_cin=3)
        shape = self.stem.out_shape
        self.blocks, self.trans = [], []
        for b in range(3):
            blk = DenseBlock(ps, f"block{b + 1}", shape, self.n, self.k)
            self.blocks.append(blk)
            shape = blk.out_shape
            real = int(blk.keep.sum())
            bn = BNReLU(ps, f"transition{b + 1}" if b < 2 else "final", shape)
            mask_param(bn.gamma, blk.keep, 0)
            mask_param(bn.beta, blk.keep, 0)
            if b == 2:
                self.final_bn = bn
                break
            conv = ConvBN(ps, f"transition{b + 1}/conv", shape, real, 1, 1, 1, 1, "SAME", relu=True, bn=False,
                          init=("trunc_normal", math.sqrt(2.0 / 9 / real)))
            mask_param(conv.w, blk.keep, 3)
            pool = AvgPool2(f"transition{b + 1}/apool", conv.out_shape)
            self.trans.append((bn, conv, pool))
            shape = pool.out_shape
        self.gap = GlobalAvgPool("spatial_mean", shape)
        self.fc = Logits(ps, "logits", shape[2], self.num_classes)
        mask_param(self.fc.w, self.blocks[2].keep, 3)
        self.layers = [self.stem]
        for b in range(3):
            self.layers.append(self.blocks[b])
            self.layers += list(self.trans[b]) if b < 2 else [self.final_bn]
        self.layers += [self.gap, self.fc]

    def forward(self, images):
        N, dev = images.shape[0], images.device
        self.stem.forward(images, out=self.blocks[0].input_view(N, dev))
        for b in range(3):
            x = self.blocks[b].forward()
            if b < 2:
                bn, conv, pool = self.trans[b]
                pool.forward(conv.forward(bn.forward(x)), self.blocks[b + 1].input_view(N, dev))
        return self.fc.forward(self.gap.forward(self.final_bn.forward(x)))

    def backward(self, dlogits):
        G = self.final_bn.backward(self.gap.backward(self.fc.backward(dlogits)))
        for b in (2, 1, 0):
            g = self.blocks[b].backward(G)
            if b > 0:
                bn, conv, pool = self.trans[b - 1]
                dx, _ = conv.backward(pool.backward(g))
                G = bn.backward(dx)
        self.stem.backward(g)
