"""--eval and --eval_during_training_every_n_steps on the CPU path: the eval_metrics reference
against the numpy transcription (tests/eval_ref.py), the flags, the one-pass loader, and the
command line end to end (restore, accuracy line, JSON, untouched checkpoints, in-training passes
that leave training bitwise unchanged, two workers on gloo). All counts are compared exactly."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from eval_ref import eval_ref, make_case  # noqa: E402
from azure_hc_intel_tf_amd.bench.flags import parse_flags  # noqa: E402
from azure_hc_intel_tf_amd.ops import functional as Fn  # noqa: E402

CLI = os.path.join(ROOT, "tf_cnn_benchmarks.py")
ACC = re.compile(r"Accuracy @ 1 = ([0-9.]+) Accuracy @ 5 = ([0-9.]+) \[(\d+) examples\]")
SMALL = ["--device=cpu", "--model=trivial", "--batch_size=4", "--image_size=32", "--num_warmup_batches=1",
         "--display_every=1"]


# ------------------------------------------------------------------ the metric
@pytest.mark.parametrize("B,ncls", [(1, 3), (5, 10), (64, 1001), (70, 257)])
def test_cpu_metric_matches_transcription(B, ncls):
    lg, lab = make_case(B, ncls)
    assert lg.shape[1] == (ncls + 7) // 8 * 8 and (lg[:, ncls:] == np.float32(3e38)).all()
    c = torch.zeros(3, dtype=torch.int64)
    Fn.eval_metrics(torch.from_numpy(lg), torch.from_numpy(lab), ncls, c)
    assert tuple(c.tolist()) == eval_ref(lg, lab, ncls)


def test_edge_rows_of_the_semantics():
    """The planted rows of make_case, one by one (row order: tests/eval_ref.py)."""
    lg, lab = make_case(16, 10)
    want = {0: (1, 0, 0),   # label >= ncls
            1: (1, 1, 1),   # six equal maxima including the target
            2: (1, 0, 1),   # ties for ranks 5 and 6
            3: (1, 0, 0),   # five strictly above
            4: (1, 0, 0), 5: (1, 0, 0), 6: (1, 0, 0),  # NaN, +Inf, -Inf targets
            7: (1, 1, 1)}   # a NaN elsewhere does not count as greater
    for r, w in want.items():
        assert eval_ref(lg[r:r + 1], lab[r:r + 1], 10) == w, r
        c = torch.zeros(3, dtype=torch.int64)
        Fn.eval_metrics(torch.from_numpy(lg[r:r + 1]), torch.from_numpy(lab[r:r + 1]), 10, c)
        assert tuple(c.tolist()) == w, r
    pad = np.array([-1], dtype=np.int64)
    assert eval_ref(lg[:1], pad, 10) == (0, 0, 0)


def test_three_calls_accumulate():
    c = torch.zeros(3, dtype=torch.int64)
    want = np.zeros(3, dtype=np.int64)
    for seed in range(3):
        lg, lab = make_case(70, 257, seed=seed)
        Fn.eval_metrics(torch.from_numpy(lg), torch.from_numpy(lab), 257, c)
        want += eval_ref(lg, lab, 257)
    assert c.tolist() == want.tolist()


# ------------------------------------------------------------------ flags
def test_eval_flags():
    assert parse_flags(["--eval"]).eval is True and parse_flags(["--noeval"]).eval is False
    assert parse_flags(["--eval=true", "--train_dir=/x"]).eval is True and parse_flags([]).eval is False
    assert not parse_flags(["--eval"])._unknown
    with pytest.raises(ValueError, match="--eval.*--forward_only"):
        parse_flags(["--eval", "--forward_only"])
    p = parse_flags(["--eval_during_training_every_n_steps=3", "--num_eval_batches", "2", "--stop_at_top_1_accuracy=0.5"])
    assert (p.eval_during_training_every_n_steps, p.num_eval_batches, p.stop_at_top_1_accuracy) == (3, 2, 0.5)
    d = parse_flags([])
    assert (d.eval_during_training_every_n_steps, d.num_eval_batches, d.stop_at_top_1_accuracy) == (0, None, None)


def test_training_without_num_batches_still_runs_100():
    from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN

    p = parse_flags(["--device=cpu", "--model=trivial", "--image_size=32", "--batch_size=2"])
    assert p.num_batches == 100 and not p._num_batches_given
    assert parse_flags(["--num_batches=7"])._num_batches_given and parse_flags(["--num_epochs=1"])._num_batches_given
    b = BenchmarkCNN(p)
    assert b.num_batches == 100 and b.evaluator is None and not b._one_pass()


# ------------------------------------------------------------------ one-pass loader
@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    import make_fake_imagenet

    d = tmp_path_factory.mktemp("fake_imagenet_eval")
    make_fake_imagenet.make(str(d), shards=2, per_shard=8, subset="train", seed=1)
    make_fake_imagenet.make(str(d), shards=2, per_shard=5, subset="validation", seed=2)
    return str(d)


def _one_pass(fake_dir, rank=0, world=1, B=4):
    """(real-row counts per batch, [(label, image bytes)] of the real rows) of one pass."""
    from azure_hc_intel_tf_amd.data.imagenet import ImageNetLoader

    ld = ImageNetLoader(fake_dir, B, 32, 3, "cpu", rank=rank, world=world, train=False, seed=0, reader_threads=2,
                        decode_threads=2, depth=2, loop=False)
    img = torch.zeros(B, 32, 32, 3)
    lab = torch.zeros(B, dtype=torch.int64)
    counts, recs = [], []
    while True:
        n = ld.next_into(img, lab)
        if n == 0:
            break
        counts.append(n)
        assert (lab[:n] >= 1).all() and (lab[n:] == -1).all(), lab
        recs += [(int(lab[i]), img[i].numpy().tobytes()) for i in range(n)]
    assert ld.next_into(img, lab) == 0  # and again: exhausted stays exhausted
    ld.close()
    return counts, recs


def test_loader_one_pass_pads_and_ends(fake_dir):
    counts, recs = _one_pass(fake_dir)
    assert sum(counts) == 10 and all(c == 4 for c in counts[:-1]) and counts[-1] == 2
    assert len(set(recs)) == 10


def test_loader_one_pass_two_ranks_split_the_records(fake_dir):
    _, all_recs = _one_pass(fake_dir)
    c0, r0 = _one_pass(fake_dir, rank=0, world=2)
    c1, r1 = _one_pass(fake_dir, rank=1, world=2)
    assert sum(c0) + sum(c1) == 10
    assert len(set(r0 + r1)) == 10 and set(r0 + r1) == set(all_recs)


def test_looping_loader_is_unchanged(fake_dir):
    from azure_hc_intel_tf_amd.data.imagenet import ImageNetLoader

    ld = ImageNetLoader(fake_dir, 4, 32, 3, "cpu", train=False, seed=0, reader_threads=2, decode_threads=2, depth=2)
    img = torch.zeros(4, 32, 32, 3)
    lab = torch.zeros(4, dtype=torch.int64)
    for _ in range(5):  # 20 rows out of a 10-record split: it loops, every batch is full
        assert ld.next_into(img, lab) == 4 and (lab >= 1).all()
    ld.close()


# ------------------------------------------------------------------ command line
def _cli(args, timeout=300):
    return subprocess.run([sys.executable, CLI] + args, capture_output=True, text=True, timeout=timeout)


def _snapshot(d):
    return {f: (os.stat(os.path.join(d, f)).st_mtime_ns, open(os.path.join(d, f), "rb").read())
            for f in sorted(os.listdir(d))}


def test_cli_eval_end_to_end(fake_dir, tmp_path):
    ckpt = str(tmp_path / "ckpt")
    r = _cli(SMALL + ["--num_batches=3", f"--data_dir={fake_dir}", f"--train_dir={ckpt}"])
    assert r.returncode == 0, r.stdout + r.stderr
    before = _snapshot(ckpt)
    assert "model.ckpt-4.pt" in before
    js = tmp_path / "eval.json"
    r = _cli(SMALL + ["--eval", f"--data_dir={fake_dir}", f"--train_dir={ckpt}", f"--json_summary={js}"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Restored checkpoint at step 4" in r.stdout and "Mode:        evaluation" in r.stdout
    assert "Unrecognized flags" not in r.stdout
    m = ACC.search(r.stdout)
    assert m and int(m.group(3)) == 10, r.stdout
    assert r.stdout.index("Accuracy @ 1") < r.stdout.index("total images/sec")
    s = json.loads(js.read_text())
    assert s["eval"]["examples"] == 10 and s["eval"]["checkpoint_step"] == 4
    assert _snapshot(ckpt) == before, "--eval wrote to --train_dir"
    # the same records through the restored model, in process, counted by the transcription
    from azure_hc_intel_tf_amd.data.imagenet import ImageNetLoader
    from azure_hc_intel_tf_amd.models import create_model
    from azure_hc_intel_tf_amd.utils import checkpoint

    model = create_model("trivial", device=torch.device("cpu"), seed=1234, image_size=32)
    assert checkpoint.restore_latest(ckpt, model.ps) == 4
    model.set_training(False)
    ld = ImageNetLoader(fake_dir, 4, 32, model.image_channels, "cpu", train=False, seed=1234, reader_threads=2,
                        decode_threads=2, depth=2, loop=False)
    img = torch.zeros(model.input_shape(4))
    lab = torch.zeros(4, dtype=torch.int64)
    want = np.zeros(3, dtype=np.int64)
    while ld.next_into(img, lab):
        model.ps.repack()
        want += eval_ref(model.forward(img).float().numpy(), lab.numpy(), model.num_classes)
        model.clear()
    ld.close()
    assert want[0] == 10
    assert s["eval"]["top_1_accuracy"] == want[1] / 10 and s["eval"]["top_5_accuracy"] == want[2] / 10
    assert float(m.group(1)) == round(want[1] / 10, 4) and float(m.group(2)) == round(want[2] / 10, 4)


def test_cli_eval_without_checkpoint(tmp_path):
    empty = tmp_path / "empty"
    empty.mkdir()
    r = _cli(SMALL + ["--eval", "--num_batches=2", f"--train_dir={empty}"])
    assert r.returncode != 0 and "no checkpoint" in r.stdout + r.stderr
    assert not os.listdir(empty)
    # no --train_dir: the seeded initial weights, on synthetic data, num_batches batches
    r = _cli(SMALL + ["--eval", "--num_batches=2"])
    assert r.returncode == 0, r.stdout + r.stderr
    m = ACC.search(r.stdout)
    assert m and int(m.group(3)) == 8 and "initial weights" in r.stdout


def _load(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return {k: v for k, v in sd.items() if torch.is_tensor(v)}


def test_cli_in_training_eval_leaves_training_bitwise_unchanged(tmp_path):
    a, b, c = (str(tmp_path / n) for n in "abc")
    base = SMALL + ["--num_batches=6", "--optimizer=momentum"]
    ra = _cli(base + [f"--train_dir={a}", "--eval_during_training_every_n_steps=3", "--num_eval_batches=2"])
    rb = _cli(base + [f"--train_dir={b}"])
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout + ra.stderr + rb.stdout + rb.stderr
    lines = [l for l in ra.stdout.splitlines() if ACC.search(l)]
    assert len(lines) == 2 and lines[0].startswith("Step 3:") and lines[1].startswith("Step 6:"), ra.stdout
    assert all(int(ACC.search(l).group(3)) == 8 for l in lines)
    assert not ACC.search(rb.stdout)
    sa, sb = _load(os.path.join(a, "model.ckpt-7.pt")), _load(os.path.join(b, "model.ckpt-7.pt"))
    assert sa.keys() == sb.keys() and {"master", "momentum", "buffers"} <= sa.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{k} differs after in-training evaluation"
    # a reachable threshold ends training after the first pass, the final checkpoint still written
    rc = _cli(base + [f"--train_dir={c}", "--eval_during_training_every_n_steps=3", "--num_eval_batches=2",
                      "--stop_at_top_1_accuracy=0.0"])
    assert rc.returncode == 0, rc.stdout + rc.stderr
    assert len([l for l in rc.stdout.splitlines() if ACC.search(l)]) == 1 and "Stopping at step 3" in rc.stdout
    assert os.path.exists(os.path.join(c, "model.ckpt-4.pt")) and not os.path.exists(os.path.join(c, "model.ckpt-7.pt"))


# ------------------------------------------------------------------ two workers on gloo
def _eval_worker(hvd, argv=None):
    from azure_hc_intel_tf_amd.bench.benchmark_cnn import BenchmarkCNN, setup

    bench = BenchmarkCNN(setup(parse_flags(argv)))
    bench.run()


def test_two_workers_sum_their_counts(fake_dir, tmp_path):
    from test_hvd_dist import run

    one, two = tmp_path / "one.json", tmp_path / "two.json"
    argv = SMALL + ["--eval", f"--data_dir={fake_dir}", "--num_intra_threads=1"]
    r = _cli(argv + [f"--json_summary={one}"])
    assert r.returncode == 0, r.stdout + r.stderr
    run(2, functools.partial(_eval_worker, argv=argv + [f"--json_summary={two}"]))
    s1, s2 = json.loads(one.read_text())["eval"], json.loads(two.read_text())["eval"]
    assert s2["examples"] == 10 == s1["examples"]
    assert (s2["top_1_accuracy"], s2["top_5_accuracy"]) == (s1["top_1_accuracy"], s1["top_5_accuracy"])
    assert json.loads(two.read_text())["workers"] == 2
