"""MobileNet-v2 (1.0, 224) as tf_cnn_benchmarks ``--model=mobilenet`` builds it (upstream
``models/mobilenet_v2.py`` on slim's mobilenet_v2).

Architecture:
  conv 3x3/2 'SAME' (32) + BN + ReLU6
  -> inverted-residual bottlenecks (t, c, n, s) = (1,16,1,1) (6,24,2,2) (6,32,3,2) (6,64,4,2)
     (6,96,3,1) (6,160,3,2) (6,320,1,1): a 1x1 expand to t*cin + BN + ReLU6 (omitted when t = 1), a
     depthwise 3x3 (stride s on a stage's first block) + BN + ReLU6, a 1x1 linear projection + BN with
     no activation, and the identity add when the stride is 1 and cin == cout
  -> conv 1x1 (1280) + BN + ReLU6 -> spatial mean -> affine -> 1001 classes.
3,504,872 trainable parameters at 1000 classes (3,506,153 at this project's 1001).

The 1x1 convs are the implicit-GEMM kernels of every other model; the depthwise 3x3s are the stencil
kernels of csrc/kernels/dwconv.hip (``nn.layers.DepthwiseConvBN``), and ReLU6 is the BN passes' upper
clip. Hyper-parameters (default batch 32, base learning rate 0.005, BN decay 0.997, epsilon 1e-3)
follow upstream from memory; they are not pinned against the upstream source.
"""
from __future__ import annotations

from ..nn.layers import ConvBN, DepthwiseConvBN, GlobalAvgPool, Logits, empty_act
from ..ops import functional as Fn
from .base import CNNModel

# (expansion t, output channels c, repeats n, stride s of the first repeat)
BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
BN = dict(eps=1e-3, decay=0.997)


def _make_divisible(v: float, d: int = 8) -> int:
    """slim's channel rounding for width multipliers: to a multiple of d, never below 90 % of v."""
    n = max(d, int(v + d / 2) // d * d)
    return n + d if n < 0.9 * v else n


class InvertedResidual:
    def __init__(self, ps, name, in_shape, t: int, cout: int, stride: int):
        cin = in_shape[2]
        self.identity = stride == 1 and cin == cout
        self.expand = (ConvBN(ps, f"{name}/expand", in_shape, t * cin, 1, 1, relu6=True, **BN) if t != 1 else None)
        mid = self.expand.out_shape if self.expand is not None else in_shape
        self.dw = DepthwiseConvBN(ps, f"{name}/depthwise", mid, stride, **BN)
        self.project = ConvBN(ps, f"{name}/project", self.dw.out_shape, cout, 1, 1, relu=False, **BN)
        self.in_shape = in_shape
        self.out_shape = self.project.out_shape

    def layers(self):
        return [l for l in (self.expand, self.dw, self.project) if l is not None]

    def forward(self, x):
        h = x
        if self.expand is not None:
            # the depthwise stencil reads a plain tensor: the expand BN writes one, not GEMM planes
            N = x.shape[0]
            h = self.expand.forward(x, out=empty_act((N,) + tuple(self.expand.out_shape), x.device))
        h = self.dw.forward(h)
        res = x if self.identity else None
        if res is not None and Fn.planes_mode() and Fn.native(res) and not Fn.is_planes(res):
            res = Fn.to_planes(res)  # (the BN apply reads a residual in its output's format)
        return self.project.forward(h, residual=res)

    def backward(self, dy):
        """dy is consumed: with the identity add it also is the shortcut's gradient (the projection
        has no activation), and the block's first layer accumulates its data gradient into it."""
        d, _ = self.project.backward(dy)
        if self.expand is None:
            return self.dw.backward(d, dx=dy if self.identity else None, accumulate=self.identity)
        d = self.dw.backward(d)
        dx, _ = self.expand.backward(d, dx=dy if self.identity else None, accumulate=self.identity)
        return dx


class MobileNetV2(CNNModel):
    name = "mobilenet"
    default_image_size = 224
    default_batch_size = 32
    default_lr = 0.005
    F32_NATIVE_OK = True  # plane GEMMs for the 1x1s, the fp32 stencil kernels, fp32 BN passes

    def __init__(self, blocks=None, width: float = 1.0, **kw):
        self.block_table = tuple(tuple(b) for b in (blocks if blocks is not None else BLOCKS))
        self.width = width
        super().__init__(**kw)

    def build(self):
        ps = self.ps
        S = self.image_size
        wm = self.width
        self.stem = ConvBN(ps, "conv0", (S, S, self.image_channels), _make_divisible(32 * wm), 3, 3, 2, 2, "SAME",
                           relu6=True, need_dx=False, logical_cin=3, **BN)
        shape = self.stem.out_shape
        self.blocks = []
        for si, (t, c, n, s) in enumerate(self.block_table):
            for bi in range(n):
                blk = InvertedResidual(ps, f"stage{si + 1}/block{bi + 1}", shape, t, _make_divisible(c * wm),
                                       s if bi == 0 else 1)
                blk.cut = bi == 0 and s == 2  # a resolution boundary: the segmented backward cuts here
                self.blocks.append(blk)
                shape = blk.out_shape
        self.tail = ConvBN(ps, "conv_last", shape, _make_divisible(1280 * max(1.0, wm)), 1, 1, relu6=True, **BN)
        self.gap = GlobalAvgPool("spatial_mean", self.tail.out_shape)
        self.fc = Logits(ps, "logits", self.tail.out_shape[2], self.num_classes)
        self.layers = ([self.stem] + [l for b in self.blocks for l in b.layers()] + [self.tail, self.gap, self.fc])

    def forward(self, images):
        N = images.shape[0]
        # (plain output: block 1 has no expand conv, its depthwise reads the stem's activation)
        x = self.stem.forward(images, out=empty_act((N,) + tuple(self.stem.out_shape), images.device))
        for b in self.blocks:
            x = b.forward(x)
        return self.fc.forward(self.gap.forward(self.tail.forward(x)))

    def backward(self, dlogits):
        for _ in self.backward_segments(dlogits):
            pass

    def backward_segments(self, dlogits):
        """One segment per resolution: cut after the backward of each stride-2 block, so the
        gradients of the layers behind it are reduced while the earlier stages still run."""
        dx, _ = self.tail.backward(self.gap.backward(self.fc.backward(dlogits)))
        seg = [self.fc, self.gap, self.tail]
        for blk in reversed(self.blocks):
            dx = blk.backward(dx)
            seg += blk.layers()
            if blk.cut:
                yield seg, False
                seg = []
        self.stem.backward(dx)
        yield seg + [self.stem], True
