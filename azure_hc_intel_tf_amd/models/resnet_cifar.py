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

from ..nn.layers import ConvBN, GlobalAvgPool, Logits, PadShortcut
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
