"""--gpu_jpeg_decode: parsing, the refusals, the run's echo and a two-step CPU run that reports the
decoded / declined counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from azure_hc_intel_tf_amd.bench.flags import parse_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fake_set(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_fake_imagenet

    d = tmp_path_factory.mktemp("fake_imagenet_jpeg")
    make_fake_imagenet.make(str(d), shards=2, per_shard=8, seed=5)
    return str(d)


def test_flag_parses_default_off():
    assert parse_flags([]).gpu_jpeg_decode is False
    assert parse_flags(["--gpu_jpeg_decode"]).gpu_jpeg_decode is True
    assert parse_flags(["--gpu_jpeg_decode=false"]).gpu_jpeg_decode is False


def test_refused_with_cifar10_by_name():
    from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN

    with pytest.raises(ValueError, match="gpu_jpeg_decode"):
        BenchmarkCNN(parse_flags(["--device=cpu", "--model=trivial", "--data_name=cifar10", "--gpu_jpeg_decode"]))


def test_ignored_with_a_note_without_data_dir(capsys):
    from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN

    b = BenchmarkCNN(parse_flags(["--device=cpu", "--model=trivial", "--gpu_jpeg_decode", "--batch_size=2"]))
    b.print_info()
    assert "--gpu_jpeg_decode ignored" in capsys.readouterr().out


def test_two_step_cpu_run_reports_counts(fake_set, tmp_path):
    out_json = str(tmp_path / "summary.json")
    cmd = [sys.executable, os.path.join(ROOT, "tf_cnn_benchmarks.py"), "--device=cpu", "--model=trivial",
           f"--data_dir={fake_set}", "--gpu_jpeg_decode", "--num_batches=2", "--num_warmup_batches=0",
           "--batch_size=2", f"--json_summary={out_json}"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "JPEG decode: host Huffman stage" in out.stdout  # the echo of the configuration
    assert "images on the GPU path, 0 declined to Pillow" in out.stdout
    with open(out_json) as f:
        s = json.load(f)
    assert s["jpeg_decode"]["gpu"] >= 4 and s["jpeg_decode"]["declined"] == 0


def test_loader_cpu_same_draws_and_fallback_mix(fake_set):
    """Flag on against off on the CPU path at 256 px, where every crop of the fake set (sides <= 500)
    keeps the reduction at 1: labels, windows and flips identical for a seed means identical inputs,
    because the r = 1 decode is bit-identical to Pillow's."""
    from azure_hc_intel_tf_amd.data.imagenet import ImageNetLoader

    outs = []
    for gpu_decode in (False, True):
        ld = ImageNetLoader(fake_set, 4, 256, 3, "cpu", seed=11, reader_threads=1, decode_threads=2, depth=1,
                            loop=False, gpu_decode=gpu_decode)  # one pass: the sample order depends on the seed alone
        img = torch.zeros(4, 256, 256, 3)
        lab = torch.zeros(4, dtype=torch.int64)
        assert ld.next_into(img, lab) == 4
        outs.append((img.clone(), lab.clone(), ld))
        ld.close()
    assert torch.equal(outs[0][1], outs[1][1])
    ld = outs[1][2]
    assert ld.gpu_decoded >= 4 and ld.gpu_declined == 0
    assert torch.equal(outs[0][0], outs[1][0])
