"""CIFAR-10 pre-activation ResNets (resnet20_v2 .. resnet110_v2) on the CPU: gradients against an fp64 autograd
construction of the architecture, the parameter count against a plain torch.nn build, the driver's name rules,
and the CPU definition of Fn.preact_conv3x3_forward against BNReLU + ConvBN."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN
from azure_hc_intel_tf_amd.bench.flags import parse_flags
from azure_hc_intel_tf_amd.models import CIFAR_RESNETS_V2, create_model
from azure_hc_intel_tf_amd.nn.layers import BNReLU, ConvBN
from azure_hc_intel_tf_amd.nn.params import ParamStore
from azure_hc_intel_tf_amd.ops import functional as Fn
from azure_hc_intel_tf_amd.trainer import Trainer, constant_lr, synthetic_batch
from reference_models import conv_ref, convbn_ref, reference_grads


def resnet_cifar_v2_ref(model, images_nhwc, params):
    def bn_relu(layer, x):
        return torch.relu(F.batch_norm(x, None, None, params[layer.gamma.name], params[layer.beta.name], training=True,
                                       eps=layer.eps))

    x = convbn_ref(model.stem, images_nhwc.permute(0, 3, 1, 2), params)
    for b in model.blocks:
        sc = x
        if b.sc is not None:  # plan A on x: subsample, then a centred zero pad of the channels
            pad = (b.out_shape[2] - x.shape[1]) // 2
            sc = F.pad(x[:, :, ::b.sc.stride, ::b.sc.stride], (0, 0, 0, 0, pad, pad))
        x = conv_ref(b.c2, convbn_ref(b.c1, bn_relu(b.pre, x), params), params) + sc
    feat = bn_relu(model.post, x).mean(dim=(2, 3))
    return feat @ params[model.fc.w.name].view(model.fc.ncls, -1).t() + params[model.fc.b.name]


def test_grads_match_autograd(monkeypatch):
    monkeypatch.setenv("HCB_CPU_DTYPE", "float64")
    torch.manual_seed(0)
    m = create_model("resnet20_v2", data_name="cifar10", device="cpu", layer_counts=(1, 2, 1), image_size=16)
    img, lab = synthetic_batch(m, 4)
    img = ((img - 127.0) / 60.0).double()
    loss_ref, grads_ref, _ = reference_grads(m, img, lab, resnet_cifar_v2_ref)
    t = Trainer(m, 4, constant_lr(0.0), weight_decay=0.0)
    t._forward_backward(img, lab)
    assert torch.allclose(t.row_loss.mean().double(), loss_ref, rtol=1e-5, atol=1e-6)
    for p in m.ps.params:
        r = grads_ref[p.name]
        err = (p.grad - r).abs().max().item()
        scale = r.abs().max().item() + 1e-6
        assert err <= 1e-4 * scale + 1e-6, f"{p.name}: max err {err} vs scale {scale}"


def test_resnet20_v2_param_count():
    nn = torch.nn
    mods, c = [nn.Conv2d(3, 16, 3, bias=False), nn.BatchNorm2d(16)], 16
    for depth in (16, 32, 64):
        for _ in range(3):
            mods += [nn.BatchNorm2d(c), nn.Conv2d(c, depth, 3, bias=False), nn.BatchNorm2d(depth),
                     nn.Conv2d(depth, depth, 3, bias=False)]
            c = depth
    mods += [nn.BatchNorm2d(64), nn.Linear(64, 10)]
    want = sum(p.numel() for mod in mods for p in mod.parameters())
    assert want == 269_754
    assert create_model("resnet20_v2", data_name="cifar10", device="cpu", num_classes=10).num_params() == want


@pytest.mark.parametrize("name", CIFAR_RESNETS_V2)
def test_names_need_cifar10(name):
    base = ["--device=cpu", "--batch_size=2", f"--model={name}"]
    b = BenchmarkCNN(parse_flags(base + ["--data_name=cifar10"]))
    assert b.model.name == name and b.model.image_size == 32 and len(b.model.blocks) == (int(name[6:-3]) - 2) // 2
    with pytest.raises(ValueError, match="--data_name=cifar10"):
        BenchmarkCNN(parse_flags(base))


@pytest.mark.parametrize("c_in,cout,stride,hw", [(16, 16, 1, (6, 8)), (16, 32, 2, (8, 8)), (32, 64, 2, (5, 7))])
def test_cpu_definition_equals_bnrelu_convbn(c_in, cout, stride, hw):
    ps = ParamStore(seed=3)
    pre = BNReLU(ps, "pre", hw + (c_in,))
    conv = ConvBN(ps, "conv", hw + (c_in,), cout, 3, 3, stride, stride, "SAME")
    ps.finalize("cpu")
    pre.gamma.data.uniform_(0.5, 1.5)
    pre.beta.data.normal_(0.0, 0.3)
    x = torch.randn((3,) + hw + (c_in,)) + 2.0
    a = pre.forward(x)
    want = torch.empty((3,) + tuple(conv.out_shape))
    Fn.conv_forward(a, conv.spec, None, conv.w.data, want)
    M = x.numel() // c_in
    acc = torch.stack([x.reshape(M, c_in).sum(0), (x * x).reshape(M, c_in).sum(0)]).unsqueeze(0)
    got, stats = torch.zeros_like(want), torch.zeros(1, 2, cout)
    saved = Fn.preact_conv3x3_forward(x, conv.w.data, pre.gamma.data, pre.beta.data, pre.eps, got, stride, acc=acc,
                                      out_stats=stats, out_stats_R=1)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5)
    assert torch.allclose(saved.mean, pre._saved[2].mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(saved.invstd, pre._saved[2].invstd, rtol=1e-4)
    assert torch.allclose(stats[0, 0], want.reshape(-1, cout).sum(0), rtol=1e-4, atol=1e-4)
