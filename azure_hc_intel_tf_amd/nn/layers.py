"""Layer DSL with explicit forward / backward (the convnet_builder role of tf_cnn_benchmarks,
SURVEY.md §2.2 "convnet_builder.py": conv(+BN+ReLU), mpool, apool, affine, spatial_mean,
inception concat).

Layers run on NHWC activations and call the primitive ops of ``ops.functional`` (HIP
kernels on the GPU, PyTorch on the CPU). Backward is written out by hand instead of using
autograd so that
  * BN statistics come fused from the conv epilogue,
  * the ReLU mask / residual-gradient fan-out is produced by the BN-backward kernel,
  * the residual add of a bottleneck block becomes the beta-accumulate of the data-grad
    GEMM epilogue (no separate add kernel),
  * weight gradients land directly in the flat gradient (allreduce) buffer, and
  * the whole step (fwd + bwd + optimizer) is a fixed kernel sequence that is captured in
    a HIP graph.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Tuple

import torch

from ..ops import functional as Fn
from ..ops.functional import ConvSpec, same_pads
from .params import ParamStore


_GPU_ACT_DTYPE = [torch.bfloat16]


def set_gpu_compute_dtype(dt: torch.dtype) -> None:
    """Activation dtype of GPU models built / stepped from now on: bf16 or IEEE fp16 (the
    hand-written HIP kernels, bf16 / fp16 builds) or fp32 (the reference-precision PyTorch
    path, --compute_dtype)."""
    from ..ops import _ext

    _GPU_ACT_DTYPE[0] = dt
    _ext.set_act("fp16" if dt == torch.float16 else "bf16")


def act_dtype(device) -> torch.dtype:
    """bf16 activations on the GPU (or the reference-precision dtype); fp32 on the CPU
    (HCB_CPU_DTYPE=float64 for exact tests)."""
    if torch.device(device).type == "cuda":
        return _GPU_ACT_DTYPE[0]
    return torch.float64 if os.environ.get("HCB_CPU_DTYPE") == "float64" else torch.float32


def empty_act(shape, device, zero=False):
    f = torch.zeros if zero else torch.empty
    return f(shape, dtype=act_dtype(device), device=device)


def empty_op(shape, device):
    """A tensor that a GEMM consumes next (a BN output, a BN-backward dz): on the fp32 path the
    Planes format the bf16x6 GEMMs read (written by the producing kernel); otherwise empty_act."""
    if torch.device(device).type == "cuda" and Fn.planes_mode():
        return Fn.Planes.empty(tuple(shape), device)
    return empty_act(shape, device)


def resolve_pads(mode, H, W, kh, kw, sh, sw, dh=1, dw=1):
    """Padding (pt, pb, pl, pr) for tf_cnn_benchmarks modes 'SAME', 'VALID', 'SAME_RESNET'."""
    if isinstance(mode, (tuple, list)):
        return tuple(mode)
    if mode == "VALID":
        return (0, 0, 0, 0)
    if mode == "SAME_RESNET":  # explicit symmetric (k-1)//2 padding then VALID
        ph = (dh * (kh - 1)) // 2
        pw = (dw * (kw - 1)) // 2
        return (ph, dh * (kh - 1) - ph, pw, dw * (kw - 1) - pw)
    if mode == "SAME":
        pt, pb = same_pads(H, kh, sh, dh)
        pl, pr = same_pads(W, kw, sw, dw)
        return (pt, pb, pl, pr)
    raise ValueError(mode)


# Fusion switches (module attributes, set before a model is built; the tests flip them to
# compare against the unfused forms):
# ResNet stem: BN+ReLU+max pool in one kernel on the GPU
FUSE_STEM_POOL = True
# replicas of the BN statistic accumulators (spreads the fp32 atomic contention)
STAT_R = 8
# fold a BN layer's backward reduction into the data-grad GEMM that produces its dy
FUSE_BN_BWD = True
# projection blocks: the shortcut's BN is applied inside the block output's BN pass
# (act(BN3(z3) + BN_sc(z_sc)) in one kernel), so the shortcut's normalised tensor is never written
FUSE_RES_BN = True
# shifted single-pass BN statistics: the conv epilogue sums (v - K), (v - K)^2 with K = the
# layer's previous batch mean, so E[x^2] - E[x]^2 does not cancel in fp32 when |mean| >> std
# (False: K = 0, the plain single-pass form)
BN_SHIFT = True
# forward-only (inference) conv + BN layers: the BN affine step, the residual add and the ReLU run in
# the conv GEMM's epilogue (Fn.conv_bn_inference: one launch, the output written once in the next
# GEMM's operand format, no raw conv output); False (HCB_FUSE_INFER_BN=0): conv_forward + bn_inference
def _env_on(name: str) -> bool:
    """A default-on switch read from the environment (``NAME=0`` turns it off)."""
    return os.environ.get(name, "1") != "0"


FUSE_INFER_BN = _env_on("HCB_FUSE_INFER_BN")


class _FixedParam:
    """A non-trainable per-channel constant with a scratch gradient sink (BN scale=False)."""

    def __init__(self, value_buf, sink_buf):
        self._v = value_buf
        self._g = sink_buf

    @property
    def data(self):
        return self._v.data

    @property
    def grad(self):
        return self._g.data


class Layer:
    in_shape: Tuple[int, int, int]
    out_shape: Tuple[int, int, int]

    def clear(self):
        pass


class _BatchNorm(Layer):
    """The BatchNorm half of ConvBN (and StemS2D) and of BNReLU: its parameters and buffers, and the
    one place where their bundle is spelled out for the ``Fn.bn_*`` calls. The layer provides
    ``relu``, ``eps``, ``decay`` and ``out_shape``."""

    _acc = None  # (fwd acc, bwd acc, replicas) of the current step
    relu6 = False  # the activation is ReLU6: min(max(v, 0), 6), backward mask 0 < v < 6 (relu_mode 3)

    @property
    def act_max(self):
        return 6.0 if self.relu6 else None

    def _init_bn(self, ps: ParamStore, name: str, C: int, scale: bool = True):
        if scale:
            self.gamma = ps.add(f"{name}/batchnorm/gamma", (C,), False, ParamStore.const(1.0))
        else:  # tf batch_norm(scale=False): gamma fixed at 1, not a variable
            self.gamma = _FixedParam(ps.add_buffer(f"{name}/batchnorm/gamma_fixed", (C,), 1.0),
                                     ps.add_buffer(f"{name}/batchnorm/gamma_grad_sink", (C,), 0.0))
        self.beta = ps.add(f"{name}/batchnorm/beta", (C,), False, ParamStore.const(0.0))
        self.rmean = ps.add_buffer(f"{name}/batchnorm/moving_mean", (C,), 0.0)
        self.rvar = ps.add_buffer(f"{name}/batchnorm/moving_variance", (C,), 1.0)
        # GPU: statistic accumulators (R replicas of [2][C]) and saved batch moments
        self.acc_f = ps.add_stat(f"{name}/bn_acc_fwd", (STAT_R, 2, C))
        self.acc_b = ps.add_stat(f"{name}/bn_acc_bwd", (STAT_R, 2, C))
        self.sv_mean = ps.add_stat(f"{name}/bn_mean", (C,))
        self.sv_invstd = ps.add_stat(f"{name}/bn_invstd", (C,))
        # statistics shift K: the previous step's batch mean (written by the BN backward); the
        # producer accumulates (v - K) so the single-pass variance does not cancel (|mean| >> std)
        self.shift = ps.add_persist(f"{name}/bn_shift", (C,)) if BN_SHIFT else None

    def _stat_bufs(self, N: int, dev):
        """(forward acc, backward acc, replicas) of this step's BN statistics: the persistent
        STAT_R-replica buffers, or in deterministic mode fresh ones with a replica per 64 rows
        (each fp32 slot then receives a single add)."""
        if not Fn.deterministic():
            self._acc = (self.acc_f.data, self.acc_b.data, STAT_R)
        else:
            P, Q, C = self.out_shape
            R = Fn.det_replicas(N * P * Q)
            self._acc = (torch.zeros((R, 2, C), dtype=torch.float32, device=dev),
                         torch.zeros((R, 2, C), dtype=torch.float32, device=dev), R)
        return self._acc

    def _shift(self):
        return self.shift.data if self.shift is not None else None

    def _bn_params(self):
        return self.gamma.data, self.beta.data, self.rmean.data, self.rvar.data

    def _bn_inference(self, z, y, residual=None):
        return Fn.bn_inference(z, *self._bn_params(), self.eps, y, self.relu, residual=residual, act_max=self.act_max)

    def _bn_forward_acc(self, z, y, residual=None, res_bn=None):
        """Finalize-free GPU BN of z from this step's forward accumulator (``_stat_bufs``)."""
        acc_f, _, R = self._acc
        return Fn.bn_forward_acc(z, *self._bn_params(), self.decay, self.eps, y, self.relu, acc_f, R,
                                 self.sv_mean.data, self.sv_invstd.data, residual=residual, shift=self._shift(),
                                 res_bn=res_bn, act_max=self.act_max)

    def _bn_backward_acc(self, dy, y, z, saved, relu_mode, dz, gres=None, **kw):
        """GPU BN backward through this step's backward accumulator; leaves the next step's shift."""
        _, acc_b, R = self._acc
        return Fn.bn_backward_acc(dy, y, z, saved, self.gamma.data, self.beta.data, relu_mode, self.gamma.grad,
                                  self.beta.grad, dz, acc_b, R, gres, shift_out=self._shift(), **kw)

    def _bn_forward_ref(self, z, y, residual=None):
        return Fn.bn_forward(z, *self._bn_params(), self.decay, self.eps, y, self.relu, residual=residual,
                             act_max=self.act_max)

    def _bn_backward_ref(self, dy, y, z, saved, relu_mode, dz, gres=None):
        return Fn.bn_backward(dy, y, z, saved, self.gamma.data, self.beta.data, relu_mode, self.gamma.grad,
                              self.beta.grad, dz, gres)

    def res_bn_args(self):
        """The residual-BN operands of a deferred BN (bn_forward_acc res_bn)."""
        return (self._acc[0], self.gamma.data, self.beta.data, self.sv_mean.data, self.sv_invstd.data,
                self.rmean.data, self.rvar.data, self._shift())


class ConvBN(_BatchNorm):
    """conv(k x k, stride, padding) -> BatchNorm(train) -> [residual add] -> [ReLU]."""

    _pool_fused = None  # the Pool whose forward ran fused into this layer's BN (forward_maxpool)

    def __init__(self, ps: ParamStore, name: str, in_shape, cout: int, kh: int, kw: int, sh: int = 1,
                 sw: int = 1, mode="SAME", relu: bool = True, bn: bool = True, need_dx: bool = True,
                 eps: float = 1e-5, decay: float = 0.9, logical_cin: Optional[int] = None,
                 dilation: int = 1, scale: bool = True, init="variance_scaling", bias: bool = True,
                 relu6: bool = False, bias_init: float = 0.0):
        """``init``: "variance_scaling" | "glorot" | ("trunc_normal", stddev) -- the kernel initialiser;
        ``bias_init``: the constant the bias of a BN-free layer starts at."""
        H, W, cin = in_shape
        assert not relu6 or (relu and bn), "ReLU6 is the BN pass's activation"
        self.relu6 = relu6
        self.name = name
        self.in_shape = in_shape
        pt, pb, pl, pr = resolve_pads(mode, H, W, kh, kw, sh, sw, dilation, dilation)
        self.spec = ConvSpec(cin=logical_cin or cin, cin_pad=cin, cout=cout, kh=kh, kw=kw, sh=sh, sw=sw,
                             pt=pt, pl=pl, pb=pb, pr=pr, dh=dilation, dw=dilation)
        P, Q = self.spec.out_hw(H, W)
        assert P > 0 and Q > 0, f"{name}: empty output"
        self.out_shape = (P, Q, cout)
        self.relu = relu
        self.bn = bn
        self.need_dx = need_dx
        self.eps = eps
        self.decay = decay
        lc = logical_cin or cin
        fan_in = kh * kw * lc
        if isinstance(init, tuple):
            assert init[0] == "trunc_normal", init
            winit = ps.trunc_normal_padded(init[1], lc if lc != cin else -1)
        else:
            winit = (ps.glorot_uniform(fan_in, kh * kw * cout, lc if lc != cin else -1) if init == "glorot"
                     else ps.variance_scaling(fan_in, lc if lc != cin else -1))
        self.w = ps.add(f"{name}/conv2d/kernel", (cout, kh, kw, cin), True, winit, logical_numel=cout * kh * kw * lc)
        self.pack = ps.add_pack(self.w, cout, kh, kw, cin, self.spec.Kpad, self.spec.Kpad_t, want_tr=need_dx)
        if bn:
            self._init_bn(ps, name, cout, scale)
        else:
            # ResNet-v2's un-normalised convs (shortcut, conv3) have no bias in tf_cnn_benchmarks
            self.bias = ps.add(f"{name}/conv2d/bias", (cout,), True, ParamStore.const(bias_init)) if bias else None
        self._saved = None
        self._pre_reduced = False
        self.training = True  # False: inference BN from the moving statistics (forward-only)

    def flops(self, batch: int) -> int:
        P, Q, C = self.out_shape
        return 2 * batch * P * Q * C * self.spec.kh * self.spec.kw * self.spec.cin

    def params(self):
        """Trainable ParamRefs of this layer (gradient slots in the flat buffer)."""
        if not self.bn:
            return [self.w, self.bias] if self.bias is not None else [self.w]
        out = [self.w, self.beta]
        if not isinstance(self.gamma, _FixedParam):
            out.append(self.gamma)
        return out

    # ------------------------------------------------------------------ forward
    def forward_deferred(self, x):
        """GPU training forward of a conv + BN whose BN apply is left to the consumer (a
        projection shortcut: the block output's BN pass normalises z_sc on the fly, see
        ``forward(residual_bn=)``). Returns z; the saved batch moments are written by that pass."""
        assert self.bn and not self.relu and self.training and Fn.native(x)
        P, Q, C = self.out_shape
        z = empty_act((x.shape[0], P, Q, C), x.device)
        x = self._conv_fwd_stats(x, z)
        self._saved = (x, z, None, Fn.BNSaved(self.sv_mean.data, self.sv_invstd.data), False)
        return z

    def forward(self, x, out=None, residual=None, residual_bn=None):
        """``residual_bn``: the ConvBN (run with forward_deferred) whose raw output ``residual``
        is BN-normalised inside this layer's BN pass before the add."""
        N = x.shape[0]
        P, Q, C = self.out_shape
        dev = x.device
        if self.bn and not self.training and FUSE_INFER_BN and not self.relu6:  # (no clip in the GEMM epilogue)
            y = out if out is not None else empty_op((N, P, Q, C), dev)
            Fn.conv_bn_inference(x, self.spec, self.pack.pack if Fn.native(x) else None, self.w.data,
                                 *self._bn_params(), self.eps, y, self.relu, residual=residual)
            self._saved = None
            return y
        if self.bn and not self.training:
            z = empty_act((N, P, Q, C), dev)
            y = out if out is not None else empty_act((N, P, Q, C), dev)
            if Fn.planes_mode() and Fn.native(x) and not Fn.is_planes(x):  # fp32 path: the GEMM operand as planes
                x = Fn.to_planes(x)
            Fn.conv_forward(x, self.spec, self.pack.pack if Fn.native(x) else None, self.w.data, z)
            self._saved = None
            return self._bn_inference(z, y, residual)
        if self.bn:
            z = empty_act((N, P, Q, C), dev)
            if Fn.native(x):
                y = out if out is not None else empty_op((N, P, Q, C), dev)
                # conv epilogue accumulates the batch statistics; the apply kernel finalizes them
                x = self._conv_fwd_stats(x, z)
                if residual_bn is not None:
                    assert residual_bn._acc[2] == self._acc[2], "residual BN accumulators must match the replica count"
                saved = self._bn_forward_acc(z, y, residual,
                                             residual_bn.res_bn_args() if residual_bn is not None else None)
            else:
                y = out if out is not None else empty_act((N, P, Q, C), dev)
                Fn.conv_forward(x, self.spec, None, self.w.data, z)
                saved = self._bn_forward_ref(z, y, residual)
            self._saved = (x, z, y, saved, residual is not None)
            return y
        assert residual is None or not self.relu, "conv without BN: residual add only without ReLU"
        y = out if out is not None else empty_act((N, P, Q, C), dev)
        if Fn.planes_mode() and Fn.native(x) and not Fn.is_planes(x):
            # fp32 path, conv + bias + ReLU layers (the zoo): the fp32 input split into the GEMM's
            # planes once, for the forward and the weight gradient
            x = Fn.to_planes(x)
        Fn.conv_forward(x, self.spec, self.pack.pack if Fn.native(x) else None, self.w.data, y,
                        bias=self.bias.data if self.bias is not None else None, relu=self.relu, residual=residual)
        self._saved = (x, None, y, None, False)
        return y

    def forward_maxpool(self, x, pool: "Pool", out_planes: bool = True):
        """GPU training forward of conv -> BN -> ReLU -> max pool (the ResNet stem) in two
        launches: the conv (BN statistics in its epilogue) and one BN+ReLU+pool kernel. The
        full-size BN+ReLU activation is never written; ``pool`` keeps the argmax for its
        backward and this layer recomputes the ReLU mask from z. ``out_planes=False``: on the fp32
        path the pooled map is written as an fp32 tensor, not as GEMM planes (its consumer is a
        BN -- ResNet v2's first pre-activation)."""
        assert self.bn and self.relu and Fn.native(x) and pool.is_max and self.training
        N = x.shape[0]
        P, Q, C = self.out_shape
        z = empty_act((N, P, Q, C), x.device)
        x = self._conv_fwd_stats(x, z)
        y = (empty_op if out_planes else empty_act)((N,) + tuple(pool.out_shape), x.device)
        amax = torch.empty((N,) + tuple(pool.out_shape), dtype=torch.uint8, device=x.device)
        acc_f, _, R = self._acc
        saved = Fn.bn_relu_maxpool_acc(z, *self._bn_params(), self.decay, self.eps, acc_f, R, self.sv_mean.data,
                                       self.sv_invstd.data, y, amax, *pool.k, *pool.s, pool.pads, shift=self._shift())
        self._saved = (x, z, None, saved, False)
        pool._saved = (z, y, amax)  # the argmax backward reads only shapes from x / y
        self._pool_fused = pool
        return y

    def backward_from_maxpool(self, dyp, pool: "Pool"):
        """Backward of forward_maxpool without the full-size BN output gradient: the BN backward
        reduce and apply gather it from the pool's gradient ``dyp`` through the saved argmax
        (bn.hip pool_gather), so the max-pool backward kernel and its conv-sized output (written
        once, read twice) are gone. Then the weight gradient; the stem needs no dx."""
        assert self._pool_fused is pool and not self.need_dx
        x, z, _, saved, _ = self._saved
        _, _, amax = pool._saved
        N = dyp.shape[0]
        H, W, C = self.out_shape
        P, Q, _ = pool.out_shape
        pt, _, pl, _ = pool.pads
        dz = empty_op((N, H, W, C), dyp.device)
        self._bn_backward_acc(dyp, None, z, saved, 2, dz, pool=(amax, [H, W, P, Q, pool.k[0], pool.s[0], pt, pl]))
        run_wgrad(self, dz, x)
        self._saved = None
        self._pool_fused = None
        pool._saved = None

    def _conv_fwd_stats(self, x, z):
        """GPU conv with the BN statistics in its epilogue; returns the tensor the weight
        gradient will read (the conv's GEMM input)."""
        acc_f, _, R = self._stat_bufs(x.shape[0], x.device)
        if Fn.planes_mode() and not Fn.is_planes(x):  # fp32 path: the GEMM (and wgrad) operand as planes
            x = Fn.to_planes(x)
        Fn.conv_forward(x, self.spec, self.pack.pack, self.w.data, z, stats=acc_f, stats_R=R,
                        stats_shift=self._shift())
        return x

    def _wgrad(self, dz, x):
        Fn.conv_wgrad(dz, x, self.spec, self.w.grad.view(dz.shape[-1], -1) if Fn.native(dz) else self.w.grad)

    # ------------------------------------------------------------------ backward
    def bwd_fuse_request(self) -> Optional[Fn.BNBwdFuse]:
        """BN-backward reduction of this layer, to be fused into the GEMM producing its dy."""
        if not (self.bn and FUSE_BN_BWD) or self._saved is None or self.relu6:
            return None  # (ReLU6: the GEMM epilogues have no upper clip; bn_bwd_reduce_acc runs)
        x, z, y, saved, had_res = self._saved
        if z.dtype == torch.float32 and not (Fn.planes_mode() and z.is_cuda):
            return None  # fp32 fusion runs on the plane GEMMs (conv_p3.hip) only
        mode = (1 if had_res else 2) if self.relu else 0
        self._pre_reduced = True
        _, acc_b, R = self._acc if self._acc is not None else (None, self.acc_b.data, STAT_R)
        return Fn.BNBwdFuse(z, y, saved, self.gamma.data, self.beta.data, mode, acc_b, R)

    def backward(self, dy, dx=None, accumulate: bool = False, want_gres: bool = False, dx_bn=None):
        """Returns (dx or None, gres or None). gres = gradient w.r.t. the residual input.
        ``dx_bn``: the ConvBN layer whose BN consumes dx; its backward reduction (and ReLU
        gating) is fused into this layer's data-grad GEMM."""
        x, z, y, saved, had_res = self._saved
        dev = dy.device
        N = dy.shape[0]
        P, Q, C = self.out_shape
        gres = None
        if self.bn and self._pre_reduced:
            # dy is already g = dy * mask and (GPU) acc_b holds sum(g), sum(g*xhat)
            self._pre_reduced = False
            dz = empty_op((N, P, Q, C), dev) if Fn.native(dy) else empty_act((N, P, Q, C), dev)
            if Fn.native(dy):
                self._bn_backward_acc(dy, None, z, saved, 0, dz, pre_reduced=True)
            else:
                self._bn_backward_ref(dy, y, z, saved, 0, dz)
            if want_gres:
                gres = dy
        elif self.bn:
            dz = empty_op((N, P, Q, C), dev) if Fn.native(dy) else empty_act((N, P, Q, C), dev)
            if want_gres:
                gres = empty_act((N, P, Q, C), dev)
            relu_mode = (1 if had_res else 2) if self.relu else 0
            if self.relu6:
                assert not had_res, "ReLU6 layers take no residual"
                relu_mode = 3
            if Fn.native(dy):
                self._bn_backward_acc(dy, y, z, saved, relu_mode, dz, gres)
            else:
                self._bn_backward_ref(dy, y, z, saved, relu_mode, dz, gres)
        else:
            if self.relu:
                if Fn.native(dy) and not (dy.is_contiguous() and y.is_contiguous()):
                    dy, y = dy.contiguous(), y.contiguous()  # concat-window views (GoogLeNet)
                dz = Fn.relu_backward(dy, y, empty_act((N, P, Q, C), dev))
            else:
                dz = dy if dy.is_contiguous() else dy.contiguous()
            if self.bias is not None:
                Fn.colsum(dz.reshape(-1, C), N * P * Q, C, self.bias.grad)
            if want_gres:
                gres = dz
            if Fn.planes_mode() and Fn.native(dz) and not Fn.is_planes(dz):
                dz = Fn.to_planes(dz)  # one split for the data- and the weight-gradient GEMM
        run_wgrad(self, dz, x)
        if self.need_dx:
            H, W, Cin = self.in_shape
            if dx is None:  # (a strided 1x1 data gradient writes its stride cells' gaps itself)
                dx = empty_act((N, H, W, Cin), dev)
                accumulate = False
            bnb = dx_bn.bwd_fuse_request() if dx_bn is not None else None
            Fn.conv_dgrad(dz, self.spec, self.pack.tr, self.w.data, dx, accumulate, bnb=bnb)
        self._saved = None
        return dx, gres

    def clear(self):
        self._saved = None
        self._pre_reduced = False


class DepthwiseConvBN(_BatchNorm):
    """depthwise conv 3x3 (stride 1 | 2, 'SAME') -> BatchNorm(train) -> ReLU6: the middle layer of a
    MobileNet-v2 bottleneck. One fp32 [C,3,3] kernel per channel, no GEMM: the GPU path is the
    stencil kernels of csrc/kernels/dwconv.hip on PLAIN activations (16-bit, or fp32 tensors on the
    fp32 path -- never Planes), with the BN statistics accumulated by the forward kernel; the BN
    apply then writes the next 1x1 GEMM's operand (Planes on the fp32 path) as ConvBN does. Backward:
    BN backward (ReLU6 mask recomputed from z) into a plain dz, the two-stage weight gradient
    (through run_wgrad: side-stream capable), the gather data gradient."""

    relu = True
    relu6 = True

    def __init__(self, ps: ParamStore, name: str, in_shape, stride: int = 1, eps: float = 1e-5, decay: float = 0.9):
        H, W, C = in_shape
        assert C % 8 == 0 and stride in (1, 2)
        self.name = name
        self.in_shape = in_shape
        self.stride = stride
        pt, pb, pl, pr = resolve_pads("SAME", H, W, 3, 3, stride, stride)
        assert pt in (0, 1) and pl in (0, 1)
        self.pads = (pt, pb, pl, pr)
        self.out_shape = ((H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1, C)
        self.eps = eps
        self.decay = decay
        self.w = ps.add(f"{name}/depthwise/kernel", (C, 3, 3), True, ps.variance_scaling(9))
        self._init_bn(ps, name, C)
        self._saved = None
        self._ws = None  # weight-gradient workspace [blocks][9][C], sized at the first backward
        self.training = True

    def flops(self, batch: int) -> int:
        P, Q, C = self.out_shape
        return 2 * batch * P * Q * C * 9

    def params(self):
        return [self.w, self.beta, self.gamma]

    def bwd_fuse_request(self):
        return None  # its BN backward reduction always runs in bn_bwd_reduce_acc

    def _conv(self, x, z, **kw):
        pt, _, pl, _ = self.pads
        return Fn.dwconv_forward(x, self.w.data, z, self.stride, pt, pl, **kw)

    def forward(self, x, out=None):
        if Fn.is_planes(x):  # (a producer that wrote the GEMM format: the stencil reads plain fp32)
            x = Fn.from_planes(x)
        N = x.shape[0]
        P, Q, C = self.out_shape
        dev = x.device
        z = empty_act((N, P, Q, C), dev)
        if not self.training:
            y = out if out is not None else empty_op((N, P, Q, C), dev)
            self._conv(x, z)
            self._saved = None
            return self._bn_inference(z, y)
        if Fn.native(x):
            y = out if out is not None else empty_op((N, P, Q, C), dev)
            acc_f, _, R = self._stat_bufs(N, dev)
            # statistics from the stencil kernel: replica = row block % R; in deterministic mode its
            # grid is capped at the R = det_replicas row blocks, so every slot receives one add
            self._conv(x, z, stats=acc_f, stats_R=R, stats_shift=self._shift())
            saved = self._bn_forward_acc(z, y)
        else:
            y = out if out is not None else empty_act((N, P, Q, C), dev)
            self._conv(x, z)
            saved = self._bn_forward_ref(z, y)
        self._saved = (x, z, y, saved)
        return y

    def _wgrad(self, dz, x):
        pt, _, pl, _ = self.pads
        if Fn.native(dz) and self._ws is None:
            self._ws = Fn.dwconv_wgrad_workspace(x.shape, dz.shape, dz.device)
        Fn.dwconv_wgrad(dz, x, self.w.grad, self.stride, pt, pl, ws=self._ws)

    def backward(self, dy, dx=None, accumulate: bool = False):
        """Returns dx. ``accumulate``: add into ``dx`` (an identity shortcut's gradient)."""
        x, z, y, saved = self._saved
        dev = dy.device
        N = dy.shape[0]
        P, Q, C = self.out_shape
        dz = empty_act((N, P, Q, C), dev)  # plain: the stencil kernels consume it
        if Fn.native(dy):  # (mode 3: the ReLU6 mask recomputed from z)
            self._bn_backward_acc(dy, None, z, saved, 3, dz)
        else:
            self._bn_backward_ref(dy, y, z, saved, 3, dz)
        run_wgrad(self, dz, x)
        H, W, _ = self.in_shape
        if dx is None:
            dx = empty_act((N, H, W, C), dev)
            accumulate = False
        pt, _, pl, _ = self.pads
        Fn.dwconv_dgrad(dz, self.w.data, dx, self.stride, pt, pl, accumulate)
        self._saved = None
        return dx

    def clear(self):
        self._saved = None


# Weight-gradient GEMMs on a side stream (set by the Trainer around a step, HCB_WGRAD_STREAM=1):
# layer i's dW GEMM forks off the main stream right after its dz exists and runs beside the data-
# gradient chain, filling the CUs the dgrad grid leaves idle (e.g. 196 tiles on 256 CUs); the
# Trainer joins before a segment's gradients are reduced / the optimizer runs. The operands are
# kept referenced until the join, so the caching allocator cannot hand their memory to a later
# main-stream tensor while the side stream still reads it.
WGRAD_SIDE = {"stream": None, "keep": []}


def run_wgrad(layer, dz, x):
    s = WGRAD_SIDE["stream"]
    if s is None or not Fn.native(dz):
        layer._wgrad(dz, x)
        return
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layer._wgrad(dz, x)
    WGRAD_SIDE["keep"].append((dz, x))


def wgrad_join():
    """The main stream waits for every weight-gradient GEMM issued on the side stream."""
    s = WGRAD_SIDE["stream"]
    if s is not None and WGRAD_SIDE["keep"]:
        torch.cuda.current_stream().wait_stream(s)
        WGRAD_SIDE["keep"].clear()


# GPU ResNet stem as a space-to-depth 4x4/1 GEMM (False: the direct padded 7x7/2 form)
STEM_S2D = True


# ResNet stem: the BN backward gathers dy from the max pool's gradient (ConvBN.backward_from_maxpool).
# Bitwise equal (tests/test_stem_pool_bwd_gpu.py). The per-pixel window gather (<= 4 argmax /
# gradient loads + index math per 8 channels) costs about what the removed round trip saves: bf16
# 0.5-0.7% slower (16-bit: the round trip is only 103 MB), fp32 +0.3% in round 5's A/B
# (profiles/r4sp_stem_pool_bwd_ab.txt, profiles/r5_stem_pool_bwd_fp32.txt). None = on for the fp32
# (planes) path only; HCB_FUSE_STEM_POOL_BWD=1 / 0 forces it.
_SPB = os.environ.get("HCB_FUSE_STEM_POOL_BWD")
FUSE_STEM_POOL_BWD = None if _SPB is None else _SPB == "1"


def fuse_stem_pool_bwd() -> bool:
    return FUSE_STEM_POOL_BWD if FUSE_STEM_POOL_BWD is not None else Fn.planes_mode()


class StemS2D(ConvBN):
    """The 7x7/2 'SAME_RESNET' stem conv (3 input channels, stored padded) computed on the GPU as
    a stride-1 4x4 conv over the 2x2 space-to-depth fold of the image (csrc/kernels/stem.hip):
    K = 256 instead of the padded direct form's 448. The fp32 master weight, its gradient, the
    BN and the CPU path are exactly those of the 7x7 layer; only the GEMM operands are folded."""

    PAD = 4  # X'(P) = x(2P + a - 4): the 3-pixel SAME_RESNET pad plus the fold's half step

    def __init__(self, ps: ParamStore, name: str, in_shape, cout: int, **kw):
        super().__init__(ps, name, in_shape, cout, 7, 7, 2, 2, "SAME_RESNET", **kw)
        assert self.spec.pt == 3 and self.spec.pl == 3 and not self.need_dx
        P, Q, _ = self.out_shape
        self.fold_shape = (P + 3, Q + 3, 16)
        # the GEMM of the 4x4 / stride-1 conv over the 16-channel fold, read as a 4x1 conv over ROW
        # WINDOWS of 64 channels (pixel w's window = the 16 channels of pixels w .. w+3, the input's
        # pixel stride staying 16; csrc/bindings.cpp x_span_bytes): K = 4 x 64 keeps the weight layout
        # [cout][r][s][16] = [cout][r][64], and every k-step reads one contiguous 64-channel row (the
        # kernels' channels-multiple-of-64 fast path) instead of a gather of 16-channel pieces of two
        # or four taps. pr = -3: the windows of the last three fold columns reach past the row and are
        # never an output's.
        self.fold_spec = ConvSpec(cin=64, cin_pad=64, cout=cout, kh=4, kw=1, sh=1, sw=1, pt=0, pl=0, pb=0, pr=-3)
        self._wfold = None
        self._wpack = None
        # the folded weight gradient [cout][256]: per-step scratch in the statistics buffer, so the
        # step-start clear zeroes it (no allocation + fill per step)
        self.dwfold = ps.add_stat(f"{name}/dw_fold", (cout, 256))

    def _folded_weight(self, dev):
        """The folded GEMM weight [cout][256]: the 16-bit pack, or on the fp32 path the hi pack of
        its three planes (mid / lo attached as the pack's ``hcb_lo``, ops.functional.lo_pack)."""
        from ..ops import _ext

        p3 = Fn.lo_pack(self.pack.pack) is not None  # this model's packs carry planes: the fp32 path
        if self._wfold is None or self._wfold.device != dev or (self._wfold.dim() == 3) != p3:
            if p3:
                self._wfold = torch.empty((3, self.spec.cout, 256), dtype=torch.bfloat16, device=dev)
                self._wpack = self._wfold[0]
                Fn.register_lo(self._wpack, self._wfold[1:].reshape(2, -1))
            else:
                self._wfold = torch.empty((self.spec.cout, 256), dtype=act_dtype(dev), device=dev)
                self._wpack = self._wfold
        _ext.ops().stem_wfold(self.w.data, self._wfold)
        return self._wpack

    def fold_input(self, x):
        """2x2 space-to-depth fold of the padded image; on the fp32 path the image is split into its
        bf16 planes first and the three planes are folded as one batch of 3N images."""
        from ..ops import _ext

        if Fn.is_planes(x) or (x.is_cuda and x.dtype == torch.float32):
            N = x.shape[0]
            xf = Fn.Planes.empty((N,) + self.fold_shape, x.device)
            if not Fn.is_planes(x) and x.is_contiguous():  # split while folding: one pass over the image
                _ext.ops().stem_s2d(x, xf.t, self.PAD)
                return xf
            xp = Fn.to_planes(x)
            _ext.ops().stem_s2d(xp.t.view((3 * N,) + tuple(xp.shape[1:])), xf.t.view((3 * N,) + self.fold_shape),
                                self.PAD)
            return xf
        xf = torch.empty((x.shape[0],) + self.fold_shape, dtype=x.dtype, device=x.device)
        _ext.ops().stem_s2d(x, xf, self.PAD)
        return xf

    def _conv_fwd_stats(self, x, z):
        xf = self.fold_input(x)
        acc_f, _, R = self._stat_bufs(x.shape[0], x.device)
        Fn.conv_forward(xf, self.fold_spec, self._folded_weight(x.device), self.w.data, z, stats=acc_f, stats_R=R,
                        stats_shift=self._shift())
        return xf

    def _wgrad(self, dz, x):
        if not Fn.native(dz):
            return super()._wgrad(dz, x)
        from ..ops import _ext

        if x.shape[1:] != self.fold_shape:  # direct-form training path (forward() not forward_maxpool)
            x = self.fold_input(x)
        dwf = self.dwfold.data.view(self.spec.cout, 256)
        Fn.conv_wgrad(dz, x, self.fold_spec, dwf)
        _ext.ops().stem_wgrad_unfold(dwf, self.w.grad)

    def forward(self, x, out=None, residual=None):
        if not Fn.native(x):
            return super().forward(x, out, residual)
        N = x.shape[0]
        P, Q, C = self.out_shape
        if not self.training and FUSE_INFER_BN:
            y = out if out is not None else empty_op((N, P, Q, C), x.device)
            Fn.conv_bn_inference(self.fold_input(x), self.fold_spec, self._folded_weight(x.device), self.w.data,
                                 *self._bn_params(), self.eps, y, self.relu, residual=residual)
            self._saved = None
            return y
        z = empty_act((N, P, Q, C), x.device)
        y = out if out is not None else empty_act((N, P, Q, C), x.device)
        if not self.training:
            xf = self.fold_input(x)
            Fn.conv_forward(xf, self.fold_spec, self._folded_weight(x.device), self.w.data, z)
            self._saved = None
            return self._bn_inference(z, y, residual)
        xf = self._conv_fwd_stats(x, z)
        self._saved = (xf, z, y, self._bn_forward_acc(z, y, residual), residual is not None)
        return y

    def tune_view(self):
        """The GEMM problem the autotuner must time for this layer (the folded one)."""
        from types import SimpleNamespace

        dev = self.w.data.device
        return SimpleNamespace(spec=self.fold_spec, in_shape=self.fold_shape, out_shape=self.out_shape,
                               need_dx=False, pack=SimpleNamespace(pack=self._folded_weight(dev), tr=None),
                               name=self.name)


class Pool(Layer):
    def __init__(self, name, in_shape, kh, kw, sh, sw, mode="VALID", is_max=True, incl_pad=False):
        H, W, C = in_shape
        self.name = name
        self.in_shape = in_shape
        self.k = (kh, kw)
        self.s = (sh, sw)
        self.pads = resolve_pads(mode, H, W, kh, kw, sh, sw)
        pt, pb, pl, pr = self.pads
        P = (H + pt + pb - kh) // sh + 1
        Q = (W + pl + pr - kw) // sw + 1
        self.out_shape = (P, Q, C)
        self.is_max = is_max
        self.incl_pad = incl_pad
        self._saved = None

    def forward(self, x, out=None):
        N = x.shape[0]
        if Fn.planes_mode() and Fn.native(x) and not Fn.is_planes(x) and (out is None or Fn.is_planes(out)):
            # fp32 path after a BN-free conv (the zoo): the fp32 map split into planes here, where the
            # consuming GEMM would split the pooled map anyway; the pool then runs on planes
            x = Fn.to_planes(x)
        if out is not None:
            y = out
        elif Fn.is_planes(x):  # fp32 path: the pooled tensor is the next GEMM's operand
            y = Fn.Planes.empty((N,) + self.out_shape, x.device)
        else:
            y = empty_act((N,) + self.out_shape, x.device)
        amax = None
        if self.is_max and Fn.native(x):
            amax = torch.empty((N,) + self.out_shape, dtype=torch.uint8, device=x.device)
        Fn.pool_forward(x, y, *self.k, *self.s, self.pads, self.is_max, self.incl_pad, argmax=amax)
        self._saved = (x, y, amax)
        return y

    def backward(self, dy, dx=None, accumulate=False):
        x, y, amax = self._saved
        if dx is None:
            dx = empty_act(x.shape, dy.device)
            accumulate = False
        Fn.pool_backward(dy, x, y, dx, *self.k, *self.s, self.pads, self.is_max, self.incl_pad, accumulate,
                         argmax=amax)
        self._saved = None
        return dx

    def clear(self):
        self._saved = None


class LRN(Layer):
    """Local response normalisation over the channels (tf_cnn_benchmarks ``cnn.lrn``, tf.nn.lrn): y = x *
    (bias + alpha * sum_{|j - d| <= depth_radius} x[j]^2)^(-beta), alpha not divided by the window size.
    No parameters; training and inference are one computation. On the GPU it is the pair of kernels of
    csrc/kernels/lrn.hip: 16-bit in / out, or on the fp32 path fp32 or Planes in and always Planes out (its
    consumers, a conv or a pool, take planes). The backward recomputes the scale from the saved input and
    writes a plain dx."""

    def __init__(self, name, in_shape, depth_radius: int, bias: float, alpha: float, beta: float):
        self.name = name
        self.in_shape = in_shape
        self.out_shape = in_shape
        self.r, self.bias, self.alpha, self.beta = int(depth_radius), float(bias), float(alpha), float(beta)
        self._saved = None

    def forward(self, x):
        if Fn.native(x) and not Fn.is_planes(x) and not x.is_contiguous():
            x = x.contiguous()  # (a concat-window view)
        shape = tuple(x.shape)
        y = empty_op(shape, x.device) if Fn.native(x) else torch.empty(shape, dtype=x.dtype, device=x.device)
        Fn.lrn_forward(x, y, self.r, self.bias, self.alpha, self.beta)
        self._saved = x
        return y

    def backward(self, dy):
        x = self._saved
        dx = empty_act(tuple(x.shape), dy.device)
        dy = dy if dy.is_contiguous() else dy.contiguous()
        Fn.lrn_backward(dy, x, dx, self.r, self.bias, self.alpha, self.beta)
        self._saved = None
        return dx

    def clear(self):
        self._saved = None


class BNReLU(_BatchNorm):
    """Standalone training-mode BatchNorm (+ ReLU) on an activation: the pre-activation of
    ResNet v2 blocks (tf_cnn_benchmarks ``bottleneck_block_v2``: preact = relu(batch_norm(x)))
    and its final BN. There is no producing GEMM epilogue to fuse the statistics into: on the GPU
    one reduction pass accumulates them (shifted sums into the R replicas, ``bn_stats_acc``) and
    the finalize-free apply writes the next GEMMs' operand (Planes on the fp32 path); the backward
    is the acc-replica reduce + apply, with the identity shortcut's gradient added in the apply
    (``backward(dy, add=)``)."""

    def __init__(self, ps: ParamStore, name: str, in_shape, relu: bool = True, eps: float = 1e-5,
                 decay: float = 0.9):
        self.name = name
        self.in_shape = in_shape
        self.out_shape = in_shape
        C = in_shape[2]
        self.relu = relu
        self.eps = eps
        self.decay = decay
        self._init_bn(ps, name, C)
        self._saved = None
        self.training = True

    def params(self):
        return [self.beta, self.gamma]

    def forward(self, x):
        if Fn.is_planes(x):  # (the fp32 path's pooled stem output when not produced in fp32)
            x = Fn.from_planes(x)
        if not self.training:
            return self._bn_inference(x, empty_act(tuple(x.shape), x.device))
        if Fn.native(x):
            acc_f, _, R = self._stat_bufs(x.shape[0], x.device)
            Fn.bn_stats_acc(x, acc_f, R, self._shift())
            y = empty_op(tuple(x.shape), x.device)
            saved = self._bn_forward_acc(x, y)
        else:
            y = empty_act(tuple(x.shape), x.device)
            saved = self._bn_forward_ref(x, y)
        self._saved = (x, y, saved)
        return y

    def backward(self, dy, add=None):
        """dx = BN'(dy) (+ ``add``, the identity shortcut's gradient, summed in the same pass)."""
        x, y, saved = self._saved
        dx = empty_act(tuple(x.shape), dy.device)
        dy = dy if dy.is_contiguous() else dy.contiguous()
        if Fn.native(dy):
            self._bn_backward_acc(dy, None, x, saved, 2 if self.relu else 0, dx, add=add)
        else:
            self._bn_backward_ref(dy, y, x, saved, 1 if self.relu else 0, dx)
            if add is not None:
                dx.add_(add)
        self._saved = None
        return dx

    def clear(self):
        self._saved = None


class Dropout(Layer):
    """tf_cnn_benchmarks ``cnn.dropout(keep_prob=0.5)`` after the hidden affine layers of
    AlexNet / VGG / OverFeat. Identity when ``keep == 1`` or in forward-only mode."""

    def __init__(self, name, in_shape, keep: float = 0.5, seed: int = 0):
        self.name = name
        self.in_shape = in_shape
        self.out_shape = in_shape
        self.keep = keep
        self.seed = seed
        self.training = True
        self._step = None
        self._mask = None

    def forward(self, x):
        if self.keep >= 1.0 or not self.training:
            self._mask = None
            return x
        if self._step is None or self._step.device != x.device:
            self._step = torch.zeros(1, dtype=torch.int64, device=x.device)
        y = torch.empty_like(x)
        if Fn.native(x):
            mask = torch.empty((x.numel() + 7) // 8, dtype=torch.uint8, device=x.device)
        else:
            mask = torch.empty(x.shape, dtype=torch.bool, device=x.device)
        Fn.dropout_forward(x, y, mask, self.keep, self.seed, self._step)
        self._step.add_(1)  # device-side: a replayed graph advances it too
        self._mask = mask
        return y

    def backward(self, dy):
        if self._mask is None:
            return dy
        dx = torch.empty_like(dy)
        Fn.dropout_backward(dy.contiguous(), self._mask, dx, self.keep)
        self._mask = None
        return dx

    def clear(self):
        self._mask = None


class PadShortcut(Layer):
    """The CIFAR ResNets' parameter-free ("plan A") shortcut: stride-``stride`` subsample, then a centred
    zero pad of the channels to ``cout`` (tf_cnn_benchmarks: apool(1, 1, s, s) 'VALID' + tf.pad). The
    forward writes the block input's format (16-bit, fp32, or Planes on the fp32 path), which is the
    format the block output's BN pass reads its residual in; the backward writes the whole plain dx the
    block's first data-gradient GEMM then accumulates into."""

    def __init__(self, name, in_shape, cout: int, stride: int):
        H, W, C = in_shape
        assert cout >= C and (cout - C) % 2 == 0 and stride in (1, 2)
        self.name = name
        self.in_shape = in_shape
        self.stride = stride
        self.out_shape = (-(-H // stride), -(-W // stride), cout)

    def forward(self, x):
        shape = (x.shape[0],) + tuple(self.out_shape)
        y = Fn.Planes.empty(shape, x.device) if Fn.is_planes(x) else torch.empty(shape, dtype=x.dtype, device=x.device)
        return Fn.shortcut_pad_forward(x, y, self.stride)

    def backward(self, g):
        dx = empty_act((g.shape[0],) + tuple(self.in_shape), g.device)
        return Fn.shortcut_pad_backward(g, dx, self.stride)


class GlobalAvgPool(Layer):
    def __init__(self, name, in_shape):
        self.name = name
        self.in_shape = in_shape
        self.out_shape = (1, 1, in_shape[2])

    def forward(self, x):
        N = x.shape[0]
        if Fn.is_planes(x):  # fp32 path: the pooled features feed the classifier GEMM as planes
            y = Fn.Planes.empty((N, self.in_shape[2]), x.device)
        else:
            y = torch.empty((N, self.in_shape[2]), dtype=x.dtype, device=x.device)
        return Fn.gap_forward(x, y)

    def backward(self, dy):
        N = dy.shape[0]
        dx = empty_act((N,) + tuple(self.in_shape), dy.device)
        Fn.gap_backward(dy, dx)
        return dx


class Logits(Layer):
    """Final affine layer: logits[B, ncls] (fp32, row stride padded to 8) = x W^T + b."""

    def __init__(self, ps: ParamStore, name, in_features: int, ncls: int, stddev: float = 0.01):
        self.name = name
        self.cin = in_features
        self.ncls = ncls
        self.ld = (ncls + 7) // 8 * 8
        self.spec = ConvSpec(cin=in_features, cin_pad=in_features, cout=ncls, kh=1, kw=1)
        self.w = ps.add(f"{name}/affine/weights", (ncls, 1, 1, in_features), True, ps.trunc_normal(stddev))
        self.b = ps.add(f"{name}/affine/biases", (ncls,), True, ParamStore.const(0.0))
        # dgrad operand uses the padded logits width as its reduction length
        kt = (self.ld + 63) // 64 * 64
        self.pack = ps.add_pack(self.w, ncls, 1, 1, in_features, self.spec.Kpad, kt, want_tr=True)
        self._x = None
        # fp32 copy of 16-bit dlogits (Trainer): the bias gradient's source -- only for the exact
        # dlogits tensor it was written with (dl32_src), never for another caller's dlogits
        self.dl32 = None
        self.dl32_src = None

    def forward(self, x):
        B = x.shape[0]
        x4 = x.view(B, 1, 1, self.cin)
        logits = torch.empty((B, self.ld), dtype=torch.float32, device=x.device)
        if Fn.native(x):
            Fn.conv_forward(x4, self.spec, self.pack.pack, None, logits.view(B, 1, 1, self.ld)[..., :self.ld],
                            bias=self.b.data)
        else:
            logits.zero_()
            logits[:, :self.ncls] = (x @ self.w.data.view(self.ncls, self.cin).t().to(x.dtype)
                                     + self.b.data.to(x.dtype)).float()
        self._x = x
        return logits

    def backward(self, dlogits):
        """dlogits: [B, ld] (bf16 on GPU, zero in the padding columns)."""
        x = self._x
        B = x.shape[0]
        if (self.dl32 is not None and dlogits is self.dl32_src and self.dl32.shape[0] == B and Fn.native(x)
                and dlogits.dtype != torch.float32):
            Fn._ext.ops().colsum(self.dl32, self.ld, B, self.ncls, self.b.grad)
        else:
            Fn.colsum(dlogits, B, self.ncls, self.b.grad)
        if Fn.native(x):  # 1x1 conv gradients over B pixels (fp32 path: Planes operands, conv_p3.hip)
            p3 = x.dtype == torch.float32
            dl = (Fn.to_planes(dlogits) if p3 else dlogits).view(B, 1, 1, self.ld)
            Fn.conv_wgrad(dl, x.view(B, 1, 1, self.cin), self._wgrad_spec(), self.w.grad.view(self.ncls, self.cin),
                          cfg=None if p3 else (2, 1))
            dx = torch.empty((B, self.cin), dtype=x.dtype, device=x.device)
            Fn.conv_dgrad(dl, self._dgrad_spec(), self.pack.tr, None, dx.view(B, 1, 1, self.cin), False,
                          cfg=None if p3 else (Fn.conv_plan(B, self.cin, self.ld)[0], 1))
        else:
            g = dlogits[:, :self.ncls]
            self.w.grad.view(self.ncls, self.cin).add_((g.t() @ x).float())
            dx = g @ self.w.data.view(self.ncls, self.cin).to(x.dtype)
        self._x = None
        return dx

    def _wgrad_spec(self):
        """dW[ncls, cin] = dlogits^T x as a 1x1 conv's weight gradient (dz rows of ld columns)."""
        return ConvSpec(cin=self.cin, cin_pad=self.cin, cout=self.ncls, kh=1, kw=1)

    def _dgrad_spec(self):
        """dx = dlogits W as a 1x1 conv's data gradient: the reduction runs over the padded logits
        width (the transposed pack's Kpad_t covers it)."""
        return ConvSpec(cin=self.cin, cin_pad=self.cin, cout=self.ld, kh=1, kw=1)

    def flops(self, batch):
        return 2 * batch * self.cin * self.ncls

    def params(self):
        return [self.w, self.b]


# ------------------------------------------------------------------------------ DenseNet
# DenseNet dense layers (BN -> ReLU -> conv 3x3 with k outputs) in one launch each (csrc/kernels/
# dense3x3.hip, Fn.dense_conv3x3_forward). False: bn_apply_acc writes the normalised operand and the
# existing conv GEMM (16 output columns) writes the slot, on the same layout -- the A/B partner
FUSE_DENSE = _env_on("HCB_FUSE_DENSE")
# The dense layers' weight gradient with BN and ReLU applied on the way in (csrc/kernels/dense3x3_wgrad.hip,
# Fn.dense_conv3x3_wgrad): no re-materialised operand, no scratch for it. False: bn_apply_acc writes the
# operand and conv_wgrad reads it back -- the A/B partner. Independent of FUSE_DENSE (profiles/densenet_wgrad.txt)
FUSE_DENSE_WGRAD = _env_on("HCB_FUSE_DENSE_WGRAD")
# The dense layers' data gradient with the ReLU and BatchNorm backward applied in registers (csrc/kernels/
# dense3x3_dgrad.hip, Fn.dense_conv3x3_dgrad): the gradient of the normalised operand is never stored, no scratch
# for it, no backward statistics accumulator. False: conv_dgrad writes it and bn_backward_acc reads it twice --
# the A/B partner. Independent of FUSE_DENSE and FUSE_DENSE_WGRAD. Default OFF (``HCB_FUSE_DENSE_DGRAD=1`` turns
# it on): the captured step measured no gain in fp32 and a loss in bf16 (profiles/densenet_dgrad.txt)
FUSE_DENSE_DGRAD = os.environ.get("HCB_FUSE_DENSE_DGRAD", "0") == "1"


def dense_channel_mask(c0: int, n: int, k: int) -> torch.Tensor:
    """True for the real channels of a dense block's buffer after n layers, False for the structural pads.

    Layout: the block owns ONE NHWC buffer of c0 + 16 n channels. Channels [0, c0) hold the block input (c0
    a multiple of 8); layer i reads channels [0, c0 + 16 i) and writes slot i = [c0 + 16 i, c0 + 16 i + 16) in
    place through the row stride -- no concat copy, forward or backward. The last 16 - k channels of a slot
    are pads. Why they stay zero without any masking in the step: a pad channel is 0 at every pixel (the
    producing kernel stores literal zeros), so its batch mean and variance are 0 and xhat = 0; its beta
    starts at 0 (gamma at 0 too), so every BN that reads it outputs 0, and ReLU's mask (y > 0) is closed.
    Hence, for the pad channel: dgamma = sum(g * xhat) = 0 and dbeta = sum(g) = 0 with g = dy * mask = 0, so
    gamma and beta never move; the BN's dx is scale * (g - mean(g) - xhat * mean(g * xhat)) = 0; every conv
    weight that multiplies it has dW = sum(dz * 0) = 0 and starts at 0, and weight decay and momentum keep
    a zero at zero; a slot's pad OUTPUT rows of the kernel have dz = 0 (nothing but zero weights reads
    them), so their dW is 0 as well. Parameter storage behind pads is bit-zero and stays so; parameter
    counts (logical_numel) and the L2 term are those of the real channels."""
    m = torch.ones(c0 + Fn.DENSE_SLOT * n, dtype=torch.bool)
    for i in range(n):
        m[c0 + Fn.DENSE_SLOT * i + k:c0 + Fn.DENSE_SLOT * (i + 1)] = False
    return m


def mask_param(p, keep: torch.Tensor, dim: int) -> None:
    """Zero ``p``'s initial value where ``keep`` (along ``dim``) is False and count only the kept part."""
    init, shape = p.init, [1] * len(p.shape)
    shape[dim] = -1

    def f(t):
        init(t)
        t.mul_(keep.view(shape).to(t.dtype))

    p.init = f
    p.logical_numel = p.logical_numel // p.shape[dim] * int(keep.sum())


class _DenseLayer:
    def __init__(self, ps: ParamStore, name: str, c_in: int, k: int, keep: torch.Tensor, eps: float):
        S = Fn.DENSE_SLOT
        self.c_in, self.slot = c_in, c_in
        self.spec = ConvSpec(cin=c_in, cin_pad=c_in, cout=S, kh=3, kw=3, pt=1, pl=1, pb=1, pr=1)
        self.w = ps.add(f"{name}/conv2d/kernel", (S, 3, 3, c_in), True, ps.trunc_normal(math.sqrt(2.0 / 9 / k)),
                        logical_numel=k * 9 * c_in)
        mask_param(self.w, keep, 3)
        mask_param(self.w, torch.arange(S) < k, 0)
        self.w.logical_numel = k * 9 * int(keep.sum())
        self.pack = ps.add_pack(self.w, S, 3, 3, c_in, self.spec.Kpad, self.spec.Kpad_t, want_tr=True)
        self.gamma = ps.add(f"{name}/batchnorm/gamma", (c_in,), False, ParamStore.const(1.0))
        self.beta = ps.add(f"{name}/batchnorm/beta", (c_in,), False, ParamStore.const(0.0))
        mask_param(self.gamma, keep, 0)
        mask_param(self.beta, keep, 0)
        self.rmean = ps.add_buffer(f"{name}/batchnorm/moving_mean", (c_in,), 0.0)
        self.rvar = ps.add_buffer(f"{name}/batchnorm/moving_variance", (c_in,), 1.0)
        self.acc_b = ps.add_stat(f"{name}/bn_acc_bwd", (STAT_R, 2, c_in))
        self.acc_s = ps.add_stat(f"{name}/slot_acc", (STAT_R, 2, S))  # the unfused conv's slot statistics
        self.sv_mean = ps.add_stat(f"{name}/bn_mean", (c_in,))
        self.sv_invstd = ps.add_stat(f"{name}/bn_invstd", (c_in,))

    def params(self):
        return [self.w, self.beta, self.gamma]


class DenseBlock(Layer):
    """A DenseNet block of ``n`` layers BN -> ReLU -> conv 3x3 (k outputs) -> concat on the padded
    in-place layout of ``dense_channel_mask``. The producer of the block input writes straight into
    ``input_view`` (no copy); ``forward`` returns the whole buffer [N, H, W, c0 + 16 n]. The buffer's batch
    statistics live in one accumulator (R replicas of [2][c_total]): the input's columns from bn_stats_acc,
    each slot's from the kernel that produced it, read by every later layer -- nothing is reduced twice.
    Backward, per layer, last to first: the weight gradient normalises its operand on the way into LDS
    (FUSE_DENSE_WGRAD: Fn.dense_conv3x3_wgrad, one workspace per block) -- or, switch off, the operand is
    re-materialised by bn_apply_acc into a scratch shared by the block and conv_wgrad reads it back. The data
    gradient, the ReLU mask and the BN backward run as one op that adds into the first c_in channels of the
    gradient buffer and never stores the operand's gradient (FUSE_DENSE_DGRAD: Fn.dense_conv3x3_dgrad, one
    workspace per block) -- or, switch off, the data-gradient GEMM runs with 16 output columns on the layer's
    slot of the gradient buffer into a scratch shared by the block, and the BN backward reads it back and adds
    into that same gradient buffer (bn_bwd_apply_acc's ``add``)."""

    def __init__(self, ps: ParamStore, name: str, in_shape, n: int, k: int = 12, eps: float = 1e-5,
                 decay: float = 0.9):
        H, W, c0 = in_shape
        S = Fn.DENSE_SLOT
        assert c0 % 8 == 0 and 1 <= k <= S, "dense block: C0 % 8, growth rate <= 16"
        self.name, self.in_shape, self.c0, self.n, self.k = name, in_shape, c0, n, k
        self.ctot = c0 + S * n
        self.out_shape = (H, W, self.ctot)
        self.eps, self.decay = eps, decay
        self.keep = dense_channel_mask(c0, n, k)
        self.subs = [_DenseLayer(ps, f"{name}/layer{i + 1}", c0 + S * i, k, self.keep[:c0 + S * i], eps)
                     for i in range(n)]
        self.acc = ps.add_stat(f"{name}/bn_acc", (STAT_R, 2, self.ctot))
        self.acc0 = ps.add_stat(f"{name}/bn_acc_in", (STAT_R, 2, c0))
        self.shift = ps.add_persist(f"{name}/bn_shift", (self.ctot,)) if BN_SHIFT else None
        self.training = True
        self._buf = self._st = self._ref = None

    def params(self):
        return [p for L in self.subs for p in L.params()]

    def flops(self, batch: int) -> int:
        H, W, _ = self.in_shape
        return sum(2 * batch * H * W * self.k * 9 * int(self.keep[:L.c_in].sum()) for L in self.subs)

    def input_view(self, N: int, dev):
        H, W, _ = self.in_shape
        self._buf = empty_act((N, H, W, self.ctot), dev)
        return self._buf[..., :self.c0]

    def _sh(self, a: int, b: int):
        return self.shift.data[a:b] if self.shift is not None else None

    # ------------------------------------------------------------------ forward
    def forward(self):
        buf = self._buf
        if not Fn.native(buf):
            return self._forward_ref(buf)
        N, H, W, _ = buf.shape
        S = Fn.DENSE_SLOT
        if not self.training:
            for L in self.subs:
                if FUSE_DENSE:
                    Fn.dense_conv3x3_forward(buf, L.c_in, L.slot, L.w.data[:self.k], L.gamma.data, L.beta.data, self.eps,
                                             running_mean=L.rmean.data, running_var=L.rvar.data, wpack=L.pack.pack)
                else:
                    op = empty_op((N, H, W, L.c_in), buf.device)
                    Fn.bn_inference(buf[..., :L.c_in], L.gamma.data, L.beta.data, L.rmean.data, L.rvar.data, self.eps,
                                    op, True)
                    Fn.conv_forward(op, L.spec, L.pack.pack, L.w.data, buf[..., L.slot:L.slot + S])
            return buf
        det = Fn.deterministic()
        R = Fn.det_replicas(N * H * W) if det else STAT_R
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=buf.device)  # noqa: E731
        acc, acc0 = (z(R, 2, self.ctot), z(R, 2, self.c0)) if det else (self.acc.data, self.acc0.data)
        Fn.bn_stats_acc(buf[..., :self.c0], acc0, R, self._sh(0, self.c0))
        acc[:, :, :self.c0].copy_(acc0)
        for L in self.subs:
            if FUSE_DENSE:
                Fn.dense_conv3x3_forward(buf, L.c_in, L.slot, L.w.data[:self.k], L.gamma.data, L.beta.data, self.eps,
                                         acc=acc, R=R, shift=self._sh(0, L.c_in), momentum=self.decay,
                                         running_mean=L.rmean.data, running_var=L.rvar.data, saved_mean=L.sv_mean.data,
                                         saved_invstd=L.sv_invstd.data, stats=acc, stats_R=R,
                                         stats_shift=self._sh(L.slot, L.slot + S), wpack=L.pack.pack)
            else:
                op = empty_op((N, H, W, L.c_in), buf.device)
                Fn.bn_forward_acc(buf[..., :L.c_in], L.gamma.data, L.beta.data, L.rmean.data, L.rvar.data, self.decay,
                                  self.eps, op, True, acc[:, :, :L.c_in].contiguous(), R, L.sv_mean.data,
                                  L.sv_invstd.data, shift=self._sh(0, L.c_in))
                acc_s = z(R, 2, S) if det else L.acc_s.data
                Fn.conv_forward(op, L.spec, L.pack.pack, L.w.data, buf[..., L.slot:L.slot + S], stats=acc_s, stats_R=R,
                                stats_shift=self._sh(L.slot, L.slot + S))
                acc[:, :, L.slot:L.slot + S].copy_(acc_s)
        self._st = (acc, R)
        return buf

    # ------------------------------------------------------------------ backward
    def backward(self, G):
        """``G``: the gradient of the whole buffer [N, H, W, c_total] (plain, contiguous), accumulated into
        in place; returns its first c0 channels, the gradient of the block input."""
        if self._ref is not None:
            return self._backward_ref(G)
        buf, (acc, R) = self._buf, self._st
        N, H, W, _ = buf.shape
        S, dev = Fn.DENSE_SLOT, buf.device
        cmax = self.subs[-1].c_in
        fuse, fuse_d = FUSE_DENSE_WGRAD, FUSE_DENSE_DGRAD
        if fuse_d:
            ws_d = Fn.dense_dgrad_workspace(buf.shape, [L.c_in for L in self.subs], buf.dtype, dev)
        else:
            da_all = empty_act((N, H, W, cmax), dev)
        if fuse:  # one workspace per block, sized for the layer that needs the most
            ws = Fn.dense_wgrad_workspace(buf.shape, [L.c_in for L in self.subs], buf.dtype, dev)
        else:
            op_all = empty_op((N, H, W, cmax), dev)
        for L in reversed(self.subs):
            c = L.c_in
            x, Gin = buf[..., :c], G[..., :c]
            dz = G[..., L.slot:L.slot + S]
            if fuse:
                Fn.dense_conv3x3_wgrad(buf, c, dz, L.gamma.data, L.beta.data, L.sv_mean.data, L.sv_invstd.data,
                                       L.w.grad.view(S, -1), self.k, ws=ws)
            else:
                op = op_all[..., :c]
                Fn.bn_forward_acc(x, L.gamma.data, L.beta.data, None, None, 1.0, self.eps, op, True,
                                  acc[:, :, :c].contiguous(), R, L.sv_mean.data, L.sv_invstd.data, shift=self._sh(0, c))
            if fuse_d:  # (no Planes of dz unless the unfused weight gradient wants them)
                if not fuse:
                    Fn.conv_wgrad(Fn.to_planes(dz) if Fn.planes_mode() else dz, op, L.spec, L.w.grad.view(S, -1))
                Fn.dense_conv3x3_dgrad(buf, c, dz, L.w.data, L.gamma.data, L.beta.data, L.sv_mean.data, L.sv_invstd.data,
                                       Gin, L.gamma.grad, L.beta.grad, self.k, ws=ws_d)
                continue
            da = da_all[..., :c]
            if Fn.planes_mode():
                dz = Fn.to_planes(dz)  # one split for both GEMMs
            if not fuse:
                Fn.conv_wgrad(dz, op, L.spec, L.w.grad.view(S, -1))
            Fn.conv_dgrad(dz, L.spec, L.pack.tr, L.w.data, da, False)
            acc_b = (torch.zeros((R, 2, c), dtype=torch.float32, device=dev) if Fn.deterministic() else L.acc_b.data)
            Fn.bn_backward_acc(da, None, x, Fn.BNSaved(L.sv_mean.data, L.sv_invstd.data), L.gamma.data, L.beta.data, 2,
                               L.gamma.grad, L.beta.grad, Gin, acc_b, R, add=Gin)
        if self.shift is not None:  # the next step's shift: this step's batch means (every reader is done)
            last = self.subs[-1]
            self.shift.data[:last.c_in].copy_(last.sv_mean.data)
        self._buf = self._st = None
        return G[..., :self.c0]

    # ------------------------------------------------------------------ PyTorch path (CPU, non-native dtypes)
    def _forward_ref(self, buf):
        S, M = Fn.DENSE_SLOT, buf.numel() // buf.shape[-1]
        if not self.training:
            for L in self.subs:
                Fn.dense_conv3x3_forward(buf, L.c_in, L.slot, L.w.data[:self.k], L.gamma.data, L.beta.data, self.eps,
                                         running_mean=L.rmean.data, running_var=L.rvar.data)
            return buf
        dt = buf.dtype
        with torch.enable_grad():
            x0 = buf[..., :self.c0].detach().clone().requires_grad_(True)
            leaves, cur = [], x0
            for L in self.subs:
                w, g, b = (t.data.detach().to(dt).requires_grad_(True) for t in (L.w, L.gamma, L.beta))
                leaves.append((w, g, b))
                mean, var = cur.mean((0, 1, 2)), cur.var((0, 1, 2), unbiased=False)
                with torch.no_grad():
                    L.rmean.data.mul_(self.decay).add_((1 - self.decay) * mean.detach().float())
                    L.rvar.data.mul_(self.decay).add_((1 - self.decay) * var.detach().float() * M / max(M - 1, 1))
                a = torch.relu((cur - mean) * torch.rsqrt(var + self.eps) * g + b)
                y = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
                cur = torch.cat([cur, y], 3)
        buf.copy_(cur.detach())
        self._ref = (x0, leaves, cur)
        return buf

    def _backward_ref(self, G):
        x0, leaves, out = self._ref
        flat = [x0] + [t for trip in leaves for t in trip]
        grads = torch.autograd.grad(out, flat, G.to(out.dtype))
        for L, i in zip(self.subs, range(1, len(flat), 3)):
            L.w.grad.add_(grads[i].float())
            L.gamma.grad.add_(grads[i + 1].float())
            L.beta.grad.add_(grads[i + 2].float())
        self._ref = self._buf = None
        return grads[0]

    def clear(self):
        self._buf = self._st = self._ref = None


# ------------------------------------------------------------------------------ CIFAR ResNet-v2
# The pre-activation conv of a v2 basic block -- conv3x3(stride)(relu(bn(x))) -- in one launch (csrc/kernels/
# preact3x3.hip, Fn.preact_conv3x3_forward) that also leaves the statistics of conv1's BatchNorm. False
# (``HCB_FUSE_PREACT=0``): BNReLU.forward writes the operand and ConvBN.forward's GEMM reads it back, existing
# kernels only -- the A/B partner. Default ON: resnet56_v2 at batch 128 trains 2.8 % faster in fp32 and in bf16
# (A/A 0.04 % / 0.2 %) and runs --forward_only 11 % faster in fp32. The 16-bit --forward_only step is 15 % SLOWER
# fused (the unfused conv1 is one GEMM with the BN in its epilogue), so it keeps the unfused chain whatever the
# switch says (profiles/resnet_cifar_v2.txt).
FUSE_PREACT = _env_on("HCB_FUSE_PREACT")

# The weight gradient of that conv from the block's RAW input, BatchNorm and ReLU applied on the way into LDS
# (csrc/kernels/preact3x3_wgrad.hip, Fn.preact_conv3x3_wgrad): the backward neither re-materialises the operand nor
# allocates the scratch for it. Takes effect only where the forward ran fused. False: bn_forward_acc writes the
# operand and conv_wgrad reads it back -- the A/B partner. Default OFF (``HCB_FUSE_PREACT_WGRAD=1`` turns it on): the
# captured resnet56_v2 step at batch 128 measured 4.4 % SLOWER in fp32 and 3.6 % slower in bf16 with it (A/A 0.01 % /
# 0.2 %): the op wins on the 32 x 32 and 16 x 16 stride-1 layers (2.0x .. 1.3x) and loses on the 64-column layers
# (0.55x at 8 x 8 x 64 in fp32), where its slab rule leaves few workgroups (profiles/resnet_cifar_v2_wgrad.txt).
FUSE_PREACT_WGRAD = os.environ.get("HCB_FUSE_PREACT_WGRAD", "0") == "1"

# 16-bit --forward_only: the WHOLE pre-activation basic block -- BN1, ReLU, conv1, BN2, ReLU, conv2 and the shortcut
# add -- in one launch (csrc/kernels/preact_block.hip, Fn.preact_block_inference; models/resnet_cifar.py takes it
# where Fn.preact_block_fits). False (``HCB_FUSE_PREACT_BLOCK=0``): bn_inference, conv_bn_inference and the conv with
# the residual add, three launches -- the A/B partner. Training, fp32 and the ImageNet ResNet-v2 never take it. Default ON: the captured
# resnet56_v2 --forward_only step at batch 128 runs 1.38x as fast in bf16 and 1.40x in fp16 with it (A/A 0.17 % /
# 0.03 %; profiles/resnet_cifar_v2_block.txt).
FUSE_PREACT_BLOCK = _env_on("HCB_FUSE_PREACT_BLOCK")

# 16-bit --forward_only MobileNet-v2: the WHOLE inverted-residual block -- 1x1 expand, BN + ReLU6, depthwise 3x3, BN +
# ReLU6, 1x1 projection, BN and the identity add -- in one launch with the expanded activations resident in LDS
# (csrc/kernels/mbconv_block.hip, Fn.mbconv_block_inference; models/mobilenet.py takes it where Fn.mbconv_block_fits).
# False: the expand GEMM, bn_inference, dwconv_forward, bn_inference and the projection GEMM, five launches -- the A/B
# partner. Training and fp32 never take it. Default OFF (``HCB_FUSE_MBCONV_BLOCK=1`` turns it on): see
# profiles/mobilenet_block.txt for the measurements behind the default.
FUSE_MBCONV_BLOCK = os.environ.get("HCB_FUSE_MBCONV_BLOCK", "0") == "1"


class _PreActConv1(ConvBN):
    """conv1 of a pre-activation block: a ConvBN whose weight gradient PreActConv.backward may redirect to the fused
    op on the block's raw input (``pre_wgrad``, set for one backward; None = ConvBN's own)."""

    pre_wgrad = None

    def _wgrad(self, dz, x):
        if self.pre_wgrad is None:
            return super()._wgrad(dz, x)
        self.pre_wgrad(dz, x)


class PreActConv:
    """``pre`` (the pre-activation BNReLU of the block input) and ``conv`` (conv1: 3x3 / stride + BN + ReLU) of a
    pre-activation basic block, run as one unit. With FUSE_PREACT, on native tensors of the kernel's shapes:
    training -- bn_stats_acc on x, then the fused op writes conv1's raw output and its statistics, and conv1's
    own BN + ReLU apply runs as in ConvBN; the backward re-materialises the operand with bn_apply_acc into
    ``scratch`` (a dict the model shares between its blocks and empties after each backward: one tensor per
    stage shape) and then runs conv1's and the pre-activation's existing backward kernels -- or, with
    FUSE_PREACT_WGRAD, conv1's weight gradient reads the raw input (Fn.preact_conv3x3_wgrad; ``scratch`` then holds
    only its workspace) and nothing is re-materialised. Forward-only, fp32: the
    fused op from the moving statistics, no re-materialisation. Otherwise ``pre.forward`` then ``conv.forward``."""

    def __init__(self, ps: ParamStore, name: str, in_shape, cout: int, stride: int, scratch: dict):
        self.pre = BNReLU(ps, f"{name}/preact", in_shape)
        self.conv = _PreActConv1(ps, f"{name}/conv1", in_shape, cout, 3, 3, stride, stride, "SAME")
        self.stride, self.scratch = stride, scratch
        self.out_shape = self.conv.out_shape
        self._fused = False

    def _fusable(self, x) -> bool:
        if not self.conv.training and x.dtype != torch.float32:
            return False  # (measured slower than bn_inference + conv_bn_inference: see FUSE_PREACT)
        return (FUSE_PREACT and Fn.native(x) and not Fn.is_planes(x) and x.shape[3] in Fn.PREACT_CHANNELS
                and self.out_shape[2] in Fn.PREACT_CHANNELS)

    def forward(self, x):
        pre, conv = self.pre, self.conv
        self._fused = self._fusable(x)
        if not self._fused:
            return conv.forward(pre.forward(x))
        N, dev = x.shape[0], x.device
        z = empty_act((N,) + tuple(self.out_shape), dev)
        if not conv.training:
            Fn.preact_conv3x3_forward(x, conv.w.data, pre.gamma.data, pre.beta.data, pre.eps, z, self.stride,
                                      running_mean=pre.rmean.data, running_var=pre.rvar.data, wpack=conv.pack.pack)
            return conv._bn_inference(z, empty_op(tuple(z.shape), dev))
        acc_x, _, Rx = pre._stat_bufs(N, dev)
        acc_z, _, Rz = conv._stat_bufs(N, dev)
        Fn.bn_stats_acc(x, acc_x, Rx, pre._shift())
        saved_x = Fn.preact_conv3x3_forward(x, conv.w.data, pre.gamma.data, pre.beta.data, pre.eps, z, self.stride,
                                            acc=acc_x, R=Rx, shift=pre._shift(), out_stats=acc_z, out_stats_R=Rz,
                                            out_stats_shift=conv._shift(), momentum=pre.decay,
                                            running_mean=pre.rmean.data, running_var=pre.rvar.data,
                                            saved_mean=pre.sv_mean.data, saved_invstd=pre.sv_invstd.data,
                                            wpack=conv.pack.pack)
        y = empty_op(tuple(z.shape), dev)
        conv._saved = (None, z, y, conv._bn_forward_acc(z, y), False)  # (the operand: re-materialised in backward)
        pre._saved = (x, None, saved_x)
        return y

    def _wgrad_fused(self, dz, x):
        """conv1's weight gradient from the raw block input ``x`` (called through run_wgrad: side-stream capable). The
        workspace is shared by the blocks of a stage through ``scratch``: every weight gradient of a step is ordered
        on one stream."""
        pre, conv = self.pre, self.conv
        nout = self.out_shape[2]
        key = ("preact_wgrad_ws", tuple(x.shape), nout, self.stride)
        ws = self.scratch.get(key)
        if ws is None:
            ws = self.scratch[key] = Fn.preact_wgrad_workspace(x.shape, x.shape[3], nout, self.stride, x.dtype, x.device)
        if WGRAD_SIDE["stream"] is not None:
            WGRAD_SIDE["keep"].append(ws)  # (the model empties ``scratch`` before the side stream is joined)
        dz = Fn.from_planes(dz)  # (fp32 path: conv1's BN backward wrote the data gradient's Planes)
        saved_x = pre._saved[2]
        Fn.preact_conv3x3_wgrad(x, x.shape[3], dz, pre.gamma.data, pre.beta.data, saved_x.mean, saved_x.invstd,
                                conv.w.grad.view(nout, -1), self.stride, ws=ws)

    def backward(self, d1, add):
        """``d1``: conv1's output gradient (gated and pre-reduced when conv2's data gradient fused conv1's BN
        backward); ``add``: the shortcut's gradient in x's layout, summed in the pre-activation BN's apply."""
        pre, conv = self.pre, self.conv
        if self._fused and FUSE_PREACT_WGRAD:
            x = pre._saved[0]
            conv._saved = (x,) + tuple(conv._saved[1:])  # (the raw input: what the fused weight gradient reads)
            conv.pre_wgrad = self._wgrad_fused
            da, _ = conv.backward(d1)
            conv.pre_wgrad = None
            return pre.backward(da, add=add)
        if self._fused:
            x, _, saved_x = pre._saved
            key = (tuple(x.shape), Fn.planes_mode())
            op = self.scratch.get(key)
            if op is None:
                op = self.scratch[key] = empty_op(tuple(x.shape), x.device)
            acc_x, _, Rx = pre._acc
            Fn.bn_forward_acc(x, pre.gamma.data, pre.beta.data, None, None, 1.0, pre.eps, op, True, acc_x, Rx,
                              saved_x.mean, saved_x.invstd, shift=pre._shift())
            conv._saved = (op,) + tuple(conv._saved[1:])
        da, _ = conv.backward(d1)
        return pre.backward(da, add=add)
