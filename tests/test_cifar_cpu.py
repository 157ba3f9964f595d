"""CIFAR-10 on the CPU: the pickle reader, ``cifar_batch_reference`` against an independent numpy
construction, the loader's order / sharding / one-pass contract, the ResNet-20..110 shapes, parameter
count and learning-rate schedule, and the --data_name / --model refusals of the driver."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN
from azure_hc_intel_tf_amd.bench.flags import parse_flags
from azure_hc_intel_tf_amd.data import cifar10
from azure_hc_intel_tf_amd.data.cifar10 import Cifar10Loader, cifar_batch_reference, read_split
from azure_hc_intel_tf_amd.models import CIFAR_MODELS, create_model
from azure_hc_intel_tf_amd.models.resnet_cifar import cifar_lr_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_FILE = 24


def _tool():
    spec = importlib.util.spec_from_file_location("make_fake_cifar10", os.path.join(ROOT, "tools", "make_fake_cifar10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("cifar10")
    _tool().make(str(d), per_file=PER_FILE, seed=3)
    return str(d)


# ------------------------------------------------------------------ reader
def test_reader_round_trip(fake_dir, tmp_path):
    data, labels = read_split(fake_dir, train=True)
    assert data.shape == (5 * PER_FILE, 3, 32, 32) and data.dtype == np.uint8
    assert labels.shape == (5 * PER_FILE,) and labels.dtype == np.int64 and 0 <= labels.min() and labels.max() <= 9
    rng = np.random.default_rng(3)  # the tool's own stream: file by file, data then labels
    for i in range(5):
        want = rng.integers(0, 256, size=(PER_FILE, 3072), dtype=np.uint8)
        want_l = rng.integers(0, 10, size=PER_FILE)
        assert np.array_equal(data[i * PER_FILE:(i + 1) * PER_FILE].reshape(PER_FILE, 3072), want)
        assert np.array_equal(labels[i * PER_FILE:(i + 1) * PER_FILE], want_l)
    val, val_l = read_split(fake_dir, train=False)
    assert val.shape == (PER_FILE, 3, 32, 32) and val_l.shape == (PER_FILE,)
    # the standard archive layout: the files one level down
    sub = tmp_path / "cifar-10-batches-py"
    os.symlink(fake_dir, sub)
    assert np.array_equal(read_split(str(tmp_path), train=False)[0], val)


def test_reader_names_the_missing_or_malformed_file(fake_dir, tmp_path):
    import pickle
    import shutil

    with pytest.raises(FileNotFoundError, match="data_batch_1"):
        read_split(str(tmp_path), train=True)
    for f in os.listdir(fake_dir):
        if f != "data_batch_4":
            shutil.copy(os.path.join(fake_dir, f), tmp_path / f)
    with pytest.raises(FileNotFoundError, match="data_batch_4"):
        read_split(str(tmp_path), train=True)
    with open(tmp_path / "data_batch_4", "wb") as f:
        pickle.dump({b"data": np.zeros((3, 3071), dtype=np.uint8), b"labels": [0, 1, 2]}, f)
    with pytest.raises(ValueError, match="data_batch_4"):
        read_split(str(tmp_path), train=True)


# ------------------------------------------------------------------ reference
def _numpy_batch(data, labels, desc, cpad):
    """upstream's order, literally: zero pad to 40 x 40, crop, flip, HWC, then x / 127.5 - 1 in float64
    with the float32 constant."""
    sc = float(np.float32(1.0) / np.float32(127.5))
    out = np.zeros((len(desc), 32, 32, cpad))
    lab = np.full(len(desc), -1, dtype=np.int64)
    for b, (i, oy, ox, fl) in enumerate(desc):
        if i < 0:
            continue
        padded = np.pad(data[i], ((0, 0), (4, 4), (4, 4)))
        crop = padded[:, oy:oy + 32, ox:ox + 32]
        if fl:
            crop = crop[:, :, ::-1]
        out[b, :, :, :3] = crop.transpose(1, 2, 0).astype(np.float64) * sc - 1.0
        lab[b] = labels[i]
    return out, lab


DESC = [(0, 0, 0, 0), (1, 8, 8, 0), (2, 4, 4, 0), (3, 0, 8, 0), (4, 0, 0, 1), (5, 8, 8, 1), (6, 4, 4, 1), (7, 0, 8, 1),
        (-1, 4, 4, 0), (7, 8, 0, 1), (0, 3, 5, 1)]


@pytest.mark.parametrize("cpad", [3, 8, 16])
def test_reference_against_numpy_construction(cpad):
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, size=(8, 3, 32, 32), dtype=np.uint8)
    data[:, :, 0, :] = np.maximum(data[:, :, 0, :], 1)  # (no raw 0 on the border rows: a pad pixel is told apart)
    labels = rng.integers(0, 10, size=8)
    want, want_l = _numpy_batch(data, labels, DESC, cpad)
    out = torch.full((len(DESC), 32, 32, cpad), 7.0, dtype=torch.float64)
    got, got_l = cifar_batch_reference(torch.from_numpy(data), torch.from_numpy(labels), DESC, out, dtype=torch.float64)
    assert torch.equal(got, torch.from_numpy(want))
    assert torch.equal(got_l, torch.from_numpy(want_l))
    g = got.numpy()
    assert (g[0, :4, :, :3] == -1.0).all() and (g[0, :, :4, :3] == -1.0).all()      # offsets (0, 0): top / left pad
    assert (g[1, -4:, :, :3] == -1.0).all() and (g[1, :, -4:, :3] == -1.0).all()    # (8, 8): bottom / right pad
    assert (g[4, :, -4:, :3] == -1.0).all()                                       # (0, 0) flipped: the pad is right
    assert (g[2, :, :, :3] > -1.0).any() and np.array_equal(g[2, :, :, 0], data[2, 0] * float(np.float32(1 / 127.5)) - 1)
    assert (g[..., 3:] == 0).all()
    assert (g[8] == 0).all() and int(got_l[8]) == -1
    # the float32 CPU path: one rounding of the float64 value
    out32 = torch.empty((len(DESC), 32, 32, cpad), dtype=torch.float32)
    cifar_batch_reference(torch.from_numpy(data), torch.from_numpy(labels), DESC, out32)
    assert float((out32.double() - got).abs().max()) <= 2.0 ** -23


def test_reference_refuses_out_of_range_rows():
    data = torch.zeros((4, 3, 32, 32), dtype=torch.uint8)
    labels = torch.zeros(4, dtype=torch.int64)
    out = torch.empty((1, 32, 32, 8))
    for bad in [(4, 4, 4, 0), (-2, 4, 4, 0), (0, 9, 4, 0), (0, 4, -1, 0), (0, 4, 4, 2)]:
        with pytest.raises(ValueError):
            cifar_batch_reference(data, labels, [bad], out)


# ------------------------------------------------------------------ loader
def _drain(loader, n, B=8):
    img = torch.empty((B, 32, 32, 8))
    lab = torch.empty(B, dtype=torch.int64)
    out = []
    for _ in range(n):
        real = loader.next_into(img, lab)
        out.append((real, None if real == 0 else loader.last_desc.copy(), img.clone(), lab.clone()))
    return out


def test_loader_epoch_visits_each_index_once_and_ranks_partition(fake_dir):
    N = 5 * PER_FILE  # 120 = 15 batches of 8
    seen = []
    for rank in range(2):
        ld = Cifar10Loader(fake_dir, 8, "cpu", rank=rank, world=2, train=True, seed=5)
        share = N // 2
        batches = _drain(ld, -(-share // 8) * 2)  # two epochs' worth
        idx = np.concatenate([d[:, 0] for _, d, _, _ in batches])
        first, second = idx[:share], idx[share:2 * share]
        assert sorted(first) == sorted(second) == list(range(rank, N, 2))
        assert not np.array_equal(first, second) and not np.array_equal(first, np.arange(rank, N, 2))
        d = np.concatenate([d for _, d, _, _ in batches])
        assert d[:, 1:3].min() == 0 and d[:, 1:3].max() == 8 and set(d[:, 3]) == {0, 1}
        seen.append(set(first))
    assert seen[0] | seen[1] == set(range(N)) and not (seen[0] & seen[1])


def test_loader_one_pass_counts_and_padding(fake_dir):
    data, labels = read_split(fake_dir, train=False)
    ld = Cifar10Loader(fake_dir, 10, "cpu", train=False, loop=False)  # 24 images: 10, 10, 4
    got = _drain(ld, 5, B=10)
    assert [g[0] for g in got] == [10, 10, 4, 0, 0]
    d = np.concatenate([g[1] for g in got[:3]])
    assert list(d[:24, 0]) == list(range(24)) and (d[24:, 0] == -1).all()
    assert (d[:, 1:3] == 4).all() and (d[:, 3] == 0).all()  # the evaluation preprocessing
    last_img, last_lab = got[2][2], got[2][3]
    assert list(last_lab[:4]) == list(labels[20:24]) and (last_lab[4:] == -1).all()
    assert (last_img[4:] == 0).all()
    want = torch.from_numpy(data[20:24].transpose(0, 2, 3, 1).astype(np.float32)) * torch.tensor(1 / 127.5) - 1
    assert torch.equal(last_img[:4, :, :, :3], want)
    # training without distortions: shuffled, but the identity crop
    ld = Cifar10Loader(fake_dir, 8, "cpu", train=True, distort=False)
    d = np.concatenate([g[1] for g in _drain(ld, 3)])
    assert (d[:, 1:3] == 4).all() and (d[:, 3] == 0).all()


def test_loader_is_reproducible_per_seed_and_rank(fake_dir):
    def run(seed, rank):
        return _drain(Cifar10Loader(fake_dir, 8, "cpu", rank=rank, world=2, train=True, seed=seed), 4)

    a, b = run(11, 1), run(11, 1)
    for x, y in zip(a, b):
        assert np.array_equal(x[1], y[1]) and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])
    assert not np.array_equal(np.concatenate([x[1] for x in a]), np.concatenate([x[1] for x in run(12, 1)]))


# ------------------------------------------------------------------ models
def test_resnet20_parameter_count_and_stage_shapes():
    m = create_model("resnet20", device="cpu", num_classes=10)
    assert m.num_params() == 269722
    names = [p.name for p in m.ps.params]
    conv = sum(p.logical_numel for p in m.ps.params if p.name.endswith("conv2d/kernel"))
    bn = sum(p.logical_numel for p in m.ps.params if "/batchnorm/" in p.name)
    assert (conv, bn) == (267696, 1376) and len(names) == len(set(names))
    assert create_model("resnet20", device="cpu").num_params() == 269787  # the default: 11 classes
    assert m.image_size == 32 and m.default_batch_size == 128 and not m.stem.relu
    assert [b.out_shape for b in m.blocks] == [(32, 32, 16)] * 3 + [(16, 16, 32)] * 3 + [(8, 8, 64)] * 3
    assert [b.sc is not None for b in m.blocks] == [False, False, False, True, False, False, True, False, False]
    assert [b.c1.spec.sh for b in m.blocks] == [1, 1, 1, 2, 1, 1, 2, 1, 1]
    s2 = m.blocks[3].c1.spec  # TF 'SAME' on a stride-2 3x3 over 32 rows: all the padding at the end
    assert (s2.pt, s2.pb, s2.pl, s2.pr) == (0, 1, 0, 1)
    for name, n in zip(CIFAR_MODELS, (3, 5, 7, 9, 18)):
        assert len(create_model(name, device="cpu").blocks) == 3 * n
    small = create_model("resnet20", device="cpu", layer_counts=(1, 1, 1))
    assert [b.out_shape for b in small.blocks] == [(32, 32, 16), (16, 16, 32), (8, 8, 64)]


def test_learning_rate_schedule_batch_128():
    lr = cifar_lr_schedule(128)
    per = int(50000 / 128)  # 390
    assert per == 390
    for step, want in [(0, 0.1), (82 * per - 1, 0.1), (82 * per, 0.01), (123 * per - 1, 0.01), (123 * per, 0.001),
                       (300 * per - 1, 0.001), (300 * per, 0.0002), (10 ** 7, 0.0002)]:
        assert lr(step) == want, step
    b = BenchmarkCNN(parse_flags(["--device=cpu", "--model=resnet20", "--data_name=cifar10", "--batch_size=128",
                                  "--num_batches=1"]))
    assert b.trainer.lr_fn(82 * per - 1) == 0.1 and b.trainer.lr_fn(82 * per) == 0.01
    assert b.model.num_classes == 11 and b.batch_size == 128


def test_driver_dataset_and_model_refusals(fake_dir, capsys):
    base = ["--device=cpu", "--batch_size=4", "--num_batches=2", "--num_warmup_batches=0", "--display_every=1"]
    with pytest.raises(ValueError, match="resnet20, resnet32, resnet44, resnet56, resnet110, trivial"):
        BenchmarkCNN(parse_flags(base + ["--model=resnet50", "--data_name=cifar10"]))
    for flags in (["--model=resnet20"], ["--model=resnet110", "--data_name=imagenet"]):
        with pytest.raises(ValueError, match="--data_name=cifar10"):
            BenchmarkCNN(parse_flags(base + flags))
    with pytest.raises(ValueError, match="color_distortions"):
        BenchmarkCNN(parse_flags(base + ["--model=trivial", "--data_name=cifar10", "--color_distortions"]))
    with pytest.raises(ValueError, match="resize_method"):
        BenchmarkCNN(parse_flags(base + ["--model=trivial", "--data_name=cifar10", "--resize_method=area"]))
    with pytest.raises(ValueError, match="data_name"):
        BenchmarkCNN(parse_flags(base + ["--model=trivial", "--data_name=mnist"]))
    b = BenchmarkCNN(parse_flags(base + ["--model=trivial", "--data_name=cifar10", "--num_epochs=0.001"]))
    assert b.num_batches == 13 and b.model.image_size == 32 and b.model.num_classes == 11  # ceil(50 / 4)
    b = BenchmarkCNN(parse_flags(base + ["--model=trivial", "--data_name=cifar10", f"--data_dir={fake_dir}"]))
    b.print_info()
    s = b.run()
    out = capsys.readouterr().out
    assert "Dataset:     cifar10 (python pickles" in out and "Reading 5 CIFAR-10 pickles" in out
    assert s["data"] == "cifar10-pickle" and s["num_batches"] == 2 and np.isfinite(s["final_loss"])
    b = BenchmarkCNN(parse_flags(base + ["--model=trivial", "--data_name=cifar10"]))
    b.print_info()
    assert b.run()["data"] == "cifar10-synthetic" and "Dataset:     cifar10 (synthetic)" in capsys.readouterr().out
    # imagenet, named or not, is what it was
    b = BenchmarkCNN(parse_flags(base + ["--model=trivial", "--image_size=32"]))
    assert b.data_name == "imagenet" and b.model.num_classes == 1001 and b.epoch_images == 1281167


def test_cifar_pickles_evaluate_exactly_once_on_cpu(fake_dir):
    b = BenchmarkCNN(parse_flags(["--device=cpu", "--model=trivial", "--data_name=cifar10", f"--data_dir={fake_dir}",
                                  "--batch_size=10", "--eval", "--num_warmup_batches=0"]))
    assert b.run()["eval"]["examples"] == PER_FILE
