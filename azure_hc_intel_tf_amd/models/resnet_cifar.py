"""CIFAR-10 ResNets (20 / 32 / 44 / 56 / 110) as tf_cnn_benchmarks ``--model=resnet20 ...
--data_name=cifar10`` builds them (upstream ``models/resnet_model.py`` ``ResnetCifar10Model`` with the v1
``residual_block``).

Architecture (input 32 x 32):
  conv 3x3/1 'SAME' (16) + BN, NO ReLU (upstream's v1 branch passes activation=None to the stem)
  -> three stages of n basic blocks at 16 / 32 / 64 channels, n = 3 / 5 / 7 / 9 / 18; the first block of
     stages 2 and 3 has stride 2. A block: 3x3 (stride) conv + BN + ReLU -> 3x3 conv + BN ->
     ReLU(shortcut + .), the add and the ReLU inside the second BN pass. Padding is 'SAME' (TF's
     asymmetric form on the stride-2 convs), not 'SAME_RESNET'.
     Shortcut: the identity while the channel count stays, else "plan A": a stride-2 subsample and a
     centred zero pad of the channels (``nn.layers.PadShortcut``, csrc/kernels/shortcut.hip) -- no
     parameters.
  -> spatial mean -> affine 64 -> classes.
BN: decay 0.9, epsilon 1e-5, scale=True. ResNet-20 has 269,722 trainable parameters at 10 classes
(convs 267,696, BN 1,376, logits 650) and 269,787 at this project's 11 (upstream's
``Cifar10Dataset(num_classes=11)``).

Learning rate: piecewise constant 0.1 / 0.01 / 0.001 / 0.0002 with boundaries at epochs 82, 123 and 300
of 50,000 images, boundary step = int(50000 / batch) * epoch; default batch 128.

The architecture, the class count and the hyper-parameters follow upstream from memory; they are not
pinned against the upstream source.

Backward as ``resnet.Bottleneck``: conv1's BN-backward reduction runs in the epilogue of conv2's data
gradient, the previous block's in the epilogue of conv1's; conv1's data gradient is beta-accumulated
onto the shortcut's gradient -- the residual gradient itself (identity), or the dx that
``shortcut_pad_bwd`` wrote in full (plan A). The stride-2 3x3 data gradient runs as four stride-phase
GEMMs that together visit every pixel of dx once, each reading the pixels it accumulates into, so the
pad-shortcut blocks take the same order as the projection blocks of the ImageNet ResNets: no
accumulate mode in the shortcut kernel, no unfused BN reduction.
"""
from __future__ import annotations

import torch

from ..nn import layers as L
from ..nn.layers import BNReLU, ConvBN, GlobalAvgPool, Logits, PadShortcut, PreActConv, empty_act
from ..ops import functional as Fn
from .base import CNNModel

LAYER_COUNTS = {20: (3, 3, 3), 32: (5, 5, 5), 44: (7, 7, 7), 56: (9, 9, 9), 110: (18, 18, 18)}
STAGE_CHANNELS = (16, 32, 64)
NUM_TRAIN_IMAGES = 50000


def cifar_lr_schedule(global_batch: int, num_examples_per_epoch: int = NUM_TRAIN_IMAGES):
    """Piecewise constant 0.1 / 0.01 / 0.001 / 0.0002, boundaries int(examples / batch) * (82, 123, 300)."""
    per_epoch = int(num_examples_per_epoch / global_batch)
    bounds = [per_epoch * e for e in (82, 123, 300)]
    vals = (0.1, 0.01, 0.001, 0.0002)

    def lr(step: int) -> float:
        for b, v in zip(bounds, vals):
            if step < b:
                return v
        return vals[-1]

    return lr


class BasicBlock:
    def __init__(self, ps, name, in_shape, depth: int, stride: int):
        C = in_shape[2]
        self.c1 = ConvBN(ps, f"{name}/conv1", in_shape, depth, 3, 3, stride, stride, "SAME")
        self.c2 = ConvBN(ps, f"{name}/conv2", self.c1.out_shape, depth, 3, 3, 1, 1, "SAME", relu=True)
        if C != depth:
            self.sc = PadShortcut(f"{name}/shortcut", in_shape, depth, stride)
            assert self.sc.out_shape == self.c2.out_shape
        else:
            assert stride == 1, "identity shortcut with stride is not used by these ResNets"
            self.sc = None
        self.in_shape = in_shape
        self.out_shape = self.c2.out_shape

    def layers(self):
        return [self.c1, self.c2]

    def forward(self, x):
        sc = self.sc.forward(x) if self.sc is not None else x
        return self.c2.forward(self.c1.forward(x), residual=sc)

    def backward(self, dy, prev_bn=None):
        """``prev_bn``: the ConvBN producing this block's input (the previous block's conv2), whose BN
        backward is fused into the data-grad GEMM(s) that complete dx."""
        d1, gres = self.c2.backward(dy, want_gres=True, dx_bn=self.c1)
        if self.sc is not None:
            # plan A: the shortcut kernel writes ALL of dx, then conv1's stride phases accumulate
            dx = self.sc.backward(gres)
            self.c1.backward(d1, dx=dx, accumulate=True, dx_bn=prev_bn)
        else:
            dx, _ = self.c1.backward(d1, dx=gres, accumulate=True, dx_bn=prev_bn)
        return dx


class ResNetCifar(CNNModel):
    default_image_size = 32
    default_batch_size = 128
    F32_NATIVE_OK = True  # plane GEMMs, fp32 BN passes; the shortcut kernels copy planes as they copy 16-bit

    def __init__(self, depth: int = 20, layer_counts=None, num_classes: int = 11, **kw):
        self.depth = depth
        self.layer_counts = tuple(layer_counts) if layer_counts is not None else LAYER_COUNTS[depth]
        assert len(self.layer_counts) == len(STAGE_CHANNELS)
        self.name = f"resnet{depth}"
        super().__init__(num_classes=num_classes, **kw)

    @staticmethod
    def lr_schedule(global_batch: int):
        return cifar_lr_schedule(global_batch)

    def build(self):
        ps = self.ps
        S = self.image_size
        self.stem = ConvBN(ps, "conv0", (S, S, self.image_channels), STAGE_CHANNELS[0], 3, 3, 1, 1, "SAME",
                           relu=False, need_dx=False, logical_cin=3)
        shape = self.stem.out_shape
        self.blocks = []
        for si, (n, depth) in enumerate(zip(self.layer_counts, STAGE_CHANNELS)):
            for bi in range(n):
                stride = 2 if (si > 0 and bi == 0) else 1
                blk = BasicBlock(ps, f"stage{si + 1}/block{bi + 1}", shape, depth, stride)
                blk.stage = si
                self.blocks.append(blk)
                shape = blk.out_shape
        self.gap = GlobalAvgPool("spatial_mean", shape)
        self.fc = Logits(ps, "logits", shape[2], self.num_classes)
        self.layers = [self.stem] + [l for b in self.blocks for l in b.layers()] + [self.gap, self.fc]

    def forward(self, images):
        x = self.stem.forward(images)
        for b in self.blocks:
            x = b.forward(x)
        return self.fc.forward(self.gap.forward(x))

    def backward(self, dlogits):
        for _ in self.backward_segments(dlogits):
            pass

    def _stem_backward(self, dx):
        self.stem.backward(dx)
        return None

    def backward_segments(self, dlogits):
        dx = self.gap.backward(self.fc.backward(dlogits))
        units = []
        for i in range(len(self.blocks) - 1, -1, -1):
            # (the stem's BN has no ReLU and feeds block 1's identity shortcut too: its reduction runs
            # in its own backward, like the first block of the ImageNet ResNets after the max pool)
            prev = self.blocks[i - 1].c2 if i > 0 else None
            units.append((lambda d, b=self.blocks[i], p=prev: b.backward(d, p), self.blocks[i].layers()))
        units.append((self._stem_backward, [self.stem]))
        yield from self._segments_from_units(dx, [self.fc, self.gap], units)


class PreActBasicBlock:
    """The v2 basic block: a = relu(bn(x)); conv 3x3 (stride) on a + BN + ReLU (``nn.layers.PreActConv``: one
    fused launch with FUSE_PREACT) -> conv 3x3 without BN, bias or activation, whose GEMM epilogue adds the
    shortcut; no ReLU after the add. The shortcut is taken from x, not from a: the identity, or plan A
    (``PadShortcut``). 16-bit inference runs the whole block -- both BatchNorms, both convs and the add -- as one
    launch (``Fn.preact_block_inference``, FUSE_PREACT_BLOCK) wherever the kernel's plan fits. Backward: conv1's BN-backward reduction runs in the epilogue of conv2's data gradient;
    the shortcut's gradient (dy itself, or plan A's dx) is added in the pre-activation BN's backward apply."""

    def __init__(self, ps, name, in_shape, depth: int, stride: int, scratch: dict):
        C = in_shape[2]
        self.pc = PreActConv(ps, name, in_shape, depth, stride, scratch)
        self.pre, self.c1 = self.pc.pre, self.pc.conv
        self.c2 = ConvBN(ps, f"{name}/conv2", self.c1.out_shape, depth, 3, 3, 1, 1, "SAME", relu=False, bn=False,
                         bias=False)
        if C != depth:
            self.sc = PadShortcut(f"{name}/shortcut", in_shape, depth, stride)
            assert self.sc.out_shape == self.c2.out_shape
        else:
            assert stride == 1, "identity shortcut with stride is not used by these ResNets"
            self.sc = None
        self.in_shape = in_shape
        self.out_shape = self.c2.out_shape

    def layers(self):
        return [self.pre, self.c1, self.c2]

    def _one_launch(self, x) -> bool:
        """16-bit inference on native plain tensors of a geometry the block kernel's plan fits (FUSE_PREACT_BLOCK)."""
        return (L.FUSE_PREACT_BLOCK and not self.c1.training and Fn.native(x) and not Fn.is_planes(x)
                and x.dtype != torch.float32
                and Fn.preact_block_fits(x.shape, self.in_shape[2], self.out_shape[2], self.pc.stride))

    def forward(self, x):
        sc = self.sc.forward(x) if self.sc is not None else x
        if self._one_launch(x):
            pre, c1, c2 = self.pre, self.c1, self.c2
            out = empty_act((x.shape[0],) + tuple(self.out_shape), x.device)
            return Fn.preact_block_inference(x, c1.w.data, *pre._bn_params(), pre.eps, c2.w.data, *c1._bn_params(),
                                             c1.eps, sc, out, self.pc.stride, wpack1=c1.pack.pack, wpack2=c2.pack.pack)
        return self.c2.forward(self.pc.forward(x), residual=sc)

    def backward(self, dy):
        d1, gres = self.c2.backward(dy, want_gres=True, dx_bn=self.c1)  # gres = dy: the shortcut's gradient
        return self.pc.backward(d1, self.sc.backward(gres) if self.sc is not None else gres)


class ResNetCifarV2(CNNModel):
    """CIFAR-10 pre-activation ResNets ``--model=resnet20_v2 | 32 | 44 | 56 | 110 --data_name=cifar10`` (upstream
    ``ResnetCifar10Model`` with the v2 ``residual_block``; from memory, not pinned against the upstream source):

      conv 3x3 (16) + BN + ReLU (the v2 stem keeps the ReLU that v1 drops)
      -> three stages of n ``PreActBasicBlock`` at 16 / 32 / 64 channels, stride 2 on the first block of stages
         2 and 3
      -> BN + ReLU -> spatial mean -> affine -> classes.
    ResNet-20 v2 has 269,754 trainable parameters at 10 classes (convs 267,696, BN 1,408, logits 650): v1's
    count with the 32 parameters of one more BN over 16 channels. Learning rate, default batch and BN constants are
    ``ResNetCifar``'s. Block inputs are plain tensors (16-bit or fp32, never Planes): they feed a BatchNorm
    and a shortcut, not a GEMM."""

    default_image_size = 32
    default_batch_size = 128
    F32_NATIVE_OK = True

    def __init__(self, depth: int = 20, layer_counts=None, num_classes: int = 11, **kw):
        self.depth = depth
        self.layer_counts = tuple(layer_counts) if layer_counts is not None else LAYER_COUNTS[depth]
        assert len(self.layer_counts) == len(STAGE_CHANNELS)
        self.name = f"resnet{depth}_v2"
        self._scratch = {}  # the re-materialised conv1 operands of the fused blocks' backward, one per shape
        super().__init__(num_classes=num_classes, **kw)

    @staticmethod
    def lr_schedule(global_batch: int):
        return cifar_lr_schedule(global_batch)

    def build(self):
        ps = self.ps
        S = self.image_size
        self.stem = ConvBN(ps, "conv0", (S, S, self.image_channels), STAGE_CHANNELS[0], 3, 3, 1, 1, "SAME",
                           relu=True, need_dx=False, logical_cin=3)
        shape = self.stem.out_shape
        self.blocks = []
        for si, (n, depth) in enumerate(zip(self.layer_counts, STAGE_CHANNELS)):
            for bi in range(n):
                stride = 2 if (si > 0 and bi == 0) else 1
                blk = PreActBasicBlock(ps, f"stage{si + 1}/block{bi + 1}", shape, depth, stride, self._scratch)
                self.blocks.append(blk)
                shape = blk.out_shape
        self.post = BNReLU(ps, "postnorm", shape)
        self.gap = GlobalAvgPool("spatial_mean", shape)
        self.fc = Logits(ps, "logits", shape[2], self.num_classes)
        self.layers = [self.stem] + [l for b in self.blocks for l in b.layers()] + [self.post, self.gap, self.fc]

    def forward(self, images):
        x = self.stem.forward(images, out=empty_act((images.shape[0],) + tuple(self.stem.out_shape), images.device))
        for b in self.blocks:
            x = b.forward(x)
        return self.fc.forward(self.gap.forward(self.post.forward(x)))

    def backward(self, dlogits):
        for _ in self.backward_segments(dlogits):
            pass

    def _stem_backward(self, dx):
        self.stem.backward(dx)
        return None

    def backward_segments(self, dlogits):
        dx = self.post.backward(self.gap.backward(self.fc.backward(dlogits)))
        units = [(b.backward, b.layers()) for b in reversed(self.blocks)]
        units.append((self._stem_backward, [self.stem]))
        yield from self._segments_from_units(dx, [self.fc, self.gap, self.post], units)
        self._scratch.clear()

    def clear(self):
        super().clear()
        self._scratch.clear()
