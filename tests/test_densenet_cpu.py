"""The CPU path of Fn.dense_conv3x3_forward (the definition of the DenseNet dense-layer op) against the
formula written out in fp64: training form from the shifted statistic sums, inference form from the moving
statistics."""
import pytest
import torch
import torch.nn.functional as F

from azure_hc_intel_tf_amd.ops import functional as Fn

EPS = 1e-5


@pytest.mark.parametrize("training", [True, False], ids=["train", "inference"])
def test_dense_conv3x3_forward_cpu_is_the_formula(training):
    N, H, W, C, nout, slot, ldb, R = 2, 5, 7, 24, 12, 32, 56, 3
    M = N * H * W
    g = torch.Generator().manual_seed(0)
    buf = torch.randn(N, H, W, ldb, generator=g, dtype=torch.float64)
    before = buf.clone()
    w = torch.randn(nout, 3, 3, C, generator=g, dtype=torch.float64)
    gamma = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    x = buf[..., :C].clone()
    if training:
        mean, var = x.mean((0, 1, 2)), x.var((0, 1, 2), unbiased=False)
        shift = mean + 0.2
        d = x.reshape(M, C) - shift
        acc = torch.zeros(R, 2, ldb, dtype=torch.float64)
        acc[:, 0, :C], acc[:, 1, :C] = d.sum(0) / R, (d * d).sum(0) / R
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        kout = torch.randn(nout, generator=g, dtype=torch.float64)
        Fn.dense_conv3x3_forward(buf, C, slot, w, gamma, beta, EPS, acc=acc, R=R, shift=shift, momentum=0.9,
                                 running_mean=rm, running_var=rv, stats=acc, stats_R=R, stats_shift=kout)
        assert torch.allclose(rm, 0.1 * mean) and torch.allclose(rv, 0.9 + 0.1 * var * M / (M - 1))
    else:
        mean, var = torch.randn(C, generator=g, dtype=torch.float64), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
        Fn.dense_conv3x3_forward(buf, C, slot, w, gamma, beta, EPS, running_mean=mean, running_var=var)
    a = torch.relu((x - mean) * torch.rsqrt(var + EPS) * gamma + beta)
    ref = F.conv2d(a.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(buf[..., slot:slot + nout], ref, rtol=1e-10, atol=1e-10)
    assert not buf[..., slot + nout:slot + 16].any()
    assert torch.equal(buf[..., :slot], before[..., :slot]) and torch.equal(buf[..., slot + 16:], before[..., slot + 16:])
    if training:
        dy = ref.reshape(M, nout) - kout
        st = acc[:, :, slot:slot + nout].sum(0)
        assert torch.allclose(st[0], dy.sum(0)) and torch.allclose(st[1], (dy * dy).sum(0))


def _plain_densenet(n, k, ncls):
    """The same architecture from plain torch.nn modules, on the true channel counts."""
    nn = torch.nn
    mods, c = [nn.Conv2d(3, 16, 3, padding=1)], 16
    for b in range(3):
        for _ in range(n):
            mods += [nn.BatchNorm2d(c), nn.Conv2d(c, k, 3, padding=1, bias=False)]
            c += k
        mods += [nn.BatchNorm2d(c)] + ([nn.Conv2d(c, c, 1)] if b < 2 else [])
    return nn.ModuleList(mods + [nn.Linear(c, ncls)])


@pytest.mark.parametrize("name,n", [("densenet40_k12", 12), ("densenet100_k12", 32)])
@pytest.mark.parametrize("ncls", [10, 11])
def test_parameter_counts_are_those_of_the_true_channels(name, n, ncls):
    from azure_hc_intel_tf_amd.models import create_model

    m = create_model(name, data_name="cifar10", device="cpu", num_classes=ncls)
    assert m.num_params() == sum(p.numel() for p in _plain_densenet(n, 12, ncls).parameters())
    assert m.default_batch_size == 64 and m.lr_schedule(64)(0) == 0.1 and m.lr_schedule(64)(781 * 300) == 0.0001


def test_densenet_names_need_cifar10_and_k24_is_refused():
    from azure_hc_intel_tf_amd.bench.benchmark_cnn import check_dataset
    from azure_hc_intel_tf_amd.bench.flags import parse_flags
    from azure_hc_intel_tf_amd.models import create_model

    for name in ("densenet40_k12", "densenet100_k12"):
        with pytest.raises(ValueError, match="needs --data_name=cifar10"):
            check_dataset(parse_flags([f"--model={name}"]))
        assert check_dataset(parse_flags([f"--model={name}", "--data_name=cifar10"])) == "cifar10"
    for args in (["--model=densenet100_k24"], ["--model=densenet100_k24", "--data_name=cifar10"]):
        with pytest.raises(ValueError, match="C <= 2048"):
            check_dataset(parse_flags(args))
    with pytest.raises(ValueError, match="C <= 2048"):
        create_model("densenet100_k24", data_name="cifar10")
