"""Local response normalisation (``Fn.lrn_forward`` / ``Fn.lrn_backward``, TF semantics) and the CIFAR-10
AlexNet built on it, on the CPU path: the definition against ``torch.nn.functional.local_response_norm`` and
its autograd in fp64, the host-side refusals, the model's parameter counts / shapes / gradients / learning-rate
schedule, and the driver's ``--model=alexnet --data_name=cifar10``."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN
from azure_hc_intel_tf_amd.bench.flags import parse_flags
from azure_hc_intel_tf_amd.models import CIFAR_MODELS, create_model, model_names
from azure_hc_intel_tf_amd.models.sequential import AlexNet, AlexNetCifar
from azure_hc_intel_tf_amd.nn.layers import LRN, ConvBN
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_LRN = (4, 1.0, 0.001 / 9.0, 0.75)


def torch_lrn(x_nhwc, r, bias, alpha, beta):
    """torch divides alpha by the window size; TF (and Fn.lrn_*) do not."""
    n = 2 * r + 1
    return F.local_response_norm(x_nhwc.permute(0, 3, 1, 2), n, alpha=alpha * n, beta=beta, k=bias).permute(0, 2, 3, 1)


# (C, r, bias, alpha, beta): every window clipped on both sides; a small window; 9 channel vectors; the
# model's layer; a radius only the CPU path takes
CASES = [(8, 4, 1.0, 1.0, 0.75), (16, 2, 2.0, 0.5, 0.5), (72, 4, 1.0, 1.0, 0.75), (64,) + MODEL_LRN,
         (24, 6, 1.5, 0.3, 0.6)]


@pytest.mark.parametrize("C,r,bias,alpha,beta", CASES)
def test_lrn_matches_torch_and_autograd_fp64(C, r, bias, alpha, beta):
    g = torch.Generator().manual_seed(C * 10 + r)
    x = torch.randn(2, 3, 5, C, dtype=torch.float64, generator=g).requires_grad_(True)
    dy = torch.randn(2, 3, 5, C, dtype=torch.float64, generator=g)
    ref = torch_lrn(x, r, bias, alpha, beta)
    (gref,) = torch.autograd.grad(ref, x, dy)
    y = Fn.lrn_forward(x.detach(), torch.full_like(dy, float("nan")), r, bias, alpha, beta)
    dx = Fn.lrn_backward(dy, x.detach(), torch.full_like(dy, float("nan")), r, bias, alpha, beta)
    ey, ed = (y - ref.detach()).abs().max().item(), (dx - gref).abs().max().item()
    print(f"C={C} r={r}: forward max err {ey:.2e}, backward max err {ed:.2e}")
    assert ey < 1e-12 and ed < 1e-12


def test_lrn_works_at_the_dtype_given():
    x = torch.randn(1, 2, 2, 16)
    y = Fn.lrn_forward(x, torch.empty_like(x), 2, 1.0, 0.5, 0.75)
    assert y.dtype == torch.float32
    assert torch.allclose(y.double(), torch_lrn(x.double(), 2, 1.0, 0.5, 0.75), rtol=1e-5, atol=1e-6)


def test_lrn_refusals_name_the_argument():
    x = torch.randn(1, 2, 2, 8)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    for kw, word in ((dict(bias=0.0), "bias"), (dict(bias=-1.0), "bias"), (dict(alpha=-0.1), "alpha"), (dict(r=0), "r")):
        args = dict(r=2, bias=1.0, alpha=1.0, beta=0.75)
        args.update(kw)
        with pytest.raises(ValueError, match=rf"\b{word}\b"):
            Fn.lrn_forward(x, y, **args)
        with pytest.raises(ValueError, match=rf"\b{word}\b"):
            Fn.lrn_backward(x, x, dx, **args)
    # the CPU path has no kernel limits: any radius, any C, views
    wide = torch.randn(1, 2, 2, 24)[..., :12]
    Fn.lrn_forward(wide, torch.empty(1, 2, 2, 12), 7, 1.0, 1.0, 0.75)


def test_lrn_layer_saves_x_and_clears():
    l = LRN("lrn", (3, 3, 16), *MODEL_LRN)
    assert l.out_shape == l.in_shape == (3, 3, 16) and not hasattr(l, "params")
    x = torch.randn(2, 3, 3, 16)
    y = l.forward(x)
    assert l._saved is x and tuple(y.shape) == tuple(x.shape)
    l.clear()
    assert l._saved is None
    l.forward(x)
    dx = l.backward(torch.ones_like(x))
    assert l._saved is None and tuple(dx.shape) == tuple(x.shape)


# ------------------------------------------------------------------ the model
def test_alexnet_cifar_parameter_counts_and_shapes():
    m = create_model("alexnet", data_name="cifar10", device="cpu")
    assert isinstance(m, AlexNetCifar) and m.name == "alexnet" and m.image_size == 32 and m.num_classes == 11
    assert m.default_batch_size == 128 and m.F32_NATIVE_OK
    assert m.num_params() == 1_756_619
    assert create_model("alexnet", data_name="cifar10", device="cpu", num_classes=10).num_params() == 1_756_426
    counts = {}
    for p in m.ps.params:
        counts[p.name.split("/")[0]] = counts.get(p.name.split("/")[0], 0) + p.logical_numel
    assert sorted(counts.values()) == sorted([4_864, 102_464, 1_573_248, 73_920, 2_123])
    assert [l.out_shape for l in m.seq] == [(32, 32, 64), (16, 16, 64), (16, 16, 64), (16, 16, 64), (16, 16, 64),
                                            (8, 8, 64), (1, 1, 4096), (1, 1, 384), (1, 1, 192)]
    assert [(l.r, l.bias, l.alpha, l.beta) for l in m.seq if isinstance(l, LRN)] == [MODEL_LRN, MODEL_LRN]
    x = torch.zeros(4, 32, 32, 3)
    for l in m.seq:
        x = l.forward(x)
        assert tuple(x.shape) == (4,) + tuple(l.out_shape), l.name
    assert tuple(m.fc.forward(x.reshape(4, -1)).shape) == (4, 16)  # 11 logits in a row padded to 16
    m.clear()
    # initial values: constant biases 0.0 / 0.1 / 0.1 / 0.1, truncated-normal kernels of stddev 0.05 / 0.04
    convs = [l for l in m.seq if isinstance(l, ConvBN)]
    assert [round(float(l.bias.data[0]), 6) for l in convs] == [0.0, 0.1, 0.1, 0.1]
    for l, std in zip(convs, (0.05, 0.05, 0.04, 0.04)):
        w = l.w.data
        assert float(w.abs().max()) <= 2 * std + 1e-7 and (w.numel() < 10000 or abs(float(w.std()) / (0.88 * std) - 1) < 0.05)


def test_registry_keeps_the_imagenet_alexnet():
    m = create_model("alexnet", device="cpu", image_size=99)
    assert type(m) is AlexNet and m.num_classes == 1001
    assert type(create_model("alexnet", data_name="imagenet", device="cpu", image_size=99)) is AlexNet
    assert model_names().count("alexnet") == 1 and "alexnet" not in CIFAR_MODELS and len(CIFAR_MODELS) == 5


def alexnet_cifar_ref(params, images_nhwc):
    """The model restated with torch.nn.functional ops on NCHW tensors (independent of the layer DSL)."""
    def same_pool(x):  # 3x3 / 2 'SAME' on an even size: one row / column of padding at the bottom / right
        return F.max_pool2d(F.pad(x, (0, 1, 0, 1), value=-float("inf")), 3, 2)

    def lrn(x):
        return F.local_response_norm(x, 9, alpha=0.001, beta=0.75, k=1.0)  # alpha / 9 per tap = TF's 0.001 / 9

    def p(i, kind, what):
        return params[f"v{i}_{kind}/conv2d/{what}"]

    x = images_nhwc.permute(0, 3, 1, 2)
    x = torch.relu(F.conv2d(x, p(0, "conv", "kernel").permute(0, 3, 1, 2), p(0, "conv", "bias"), padding=2))
    x = lrn(same_pool(x))
    x = torch.relu(F.conv2d(x, p(3, "conv", "kernel").permute(0, 3, 1, 2), p(3, "conv", "bias"), padding=2))
    x = same_pool(lrn(x))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)  # NHWC flatten order
    x = torch.relu(x @ p(7, "affine", "kernel").reshape(384, -1).t() + p(7, "affine", "bias"))
    x = torch.relu(x @ p(8, "affine", "kernel").reshape(192, -1).t() + p(8, "affine", "bias"))
    return x @ params["logits/affine/weights"].reshape(params["logits/affine/biases"].numel(), -1).t() + \
        params["logits/affine/biases"]


def test_alexnet_cifar_grads_match_autograd(monkeypatch):
    """One training step's gradients against fp64 autograd of the restated model, at the zoo's bound
    (tests/test_model_zoo_cpu.py: max error <= 1e-5 * max |reference| + 1e-9 per tensor)."""
    monkeypatch.setenv("HCB_CPU_DTYPE", "float64")
    torch.manual_seed(0)
    m = create_model("alexnet", data_name="cifar10", device="cpu")
    img, lab = synthetic_batch(m, 4)
    img = ((img - 127.0) / 60.0).double()
    params = {p.name: p.data.detach().clone().double().requires_grad_(True) for p in m.ps.params}
    loss = F.cross_entropy(alexnet_cifar_ref(params, img), lab)
    loss.backward()
    t = Trainer(m, 4, constant_lr(0.0), weight_decay=0.0)
    t._forward_backward(img, lab)
    assert torch.allclose(t.row_loss.mean().double(), loss.detach(), rtol=1e-6, atol=1e-7)
    for p in m.ps.params:
        r = params[p.name].grad
        err = (p.grad.double() - r).abs().max().item()
        scale = r.abs().max().item() + 1e-8
        print(f"{p.name}: max err {err:.2e} vs {scale:.2e}")
        assert scale > 1e-8, f"{p.name}: the reference gradient is zero"
        assert err <= 1e-5 * scale + 1e-9, f"{p.name}: max err {err} vs {scale}"


def test_alexnet_cifar_learning_rate_schedule():
    lr = AlexNetCifar.lr_schedule(128)
    assert lr(0) == 0.1 and lr(100 * 390 - 1) == 0.1
    assert lr(100 * 390) == pytest.approx(0.01, rel=1e-12) and lr(200 * 390) == pytest.approx(0.001, rel=1e-12)


# ------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_fake_cifar10", os.path.join(ROOT, "tools", "make_fake_cifar10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = tmp_path_factory.mktemp("cifar10_alexnet")
    mod.make(str(d), per_file=24, seed=5)
    return str(d)


def test_driver_builds_and_runs_the_cifar_alexnet(fake_dir):
    b = BenchmarkCNN(parse_flags(["--model=alexnet", "--data_name=cifar10", "--device=cpu"]))
    assert isinstance(b.model, AlexNetCifar) and b.model.image_size == 32 and b.model.num_classes == 11
    assert b.batch_size == 128
    assert b.trainer.lr_fn(100 * 390 - 1) == 0.1 and b.trainer.lr_fn(100 * 390) == pytest.approx(0.01)
    base = ["--model=alexnet", "--data_name=cifar10", "--device=cpu", "--batch_size=8", "--num_batches=2",
            "--num_warmup_batches=0", "--init_learning_rate=0.01"]
    s = BenchmarkCNN(parse_flags(base)).run()
    assert s["data"] == "cifar10-synthetic" and s["num_batches"] == 2 and np.isfinite(s["final_loss"])
    s = BenchmarkCNN(parse_flags(base + [f"--data_dir={fake_dir}"])).run()
    assert s["data"] == "cifar10-pickle" and s["num_batches"] == 2 and np.isfinite(s["final_loss"])


def test_driver_without_data_name_is_the_imagenet_alexnet_and_other_models_stay_refused():
    b = BenchmarkCNN(parse_flags(["--model=alexnet", "--device=cpu", "--batch_size=1"]))
    assert type(b.model) is AlexNet and b.model.image_size == 227 and b.model.num_classes == 1001
    assert b.data_name == "imagenet"
    with pytest.raises(ValueError, match="resnet20, resnet32, resnet44, resnet56, resnet110, trivial, alexnet"):
        BenchmarkCNN(parse_flags(["--model=vgg16", "--data_name=cifar10", "--device=cpu"]))
