"""Image distortions of the real-data path, CPU side: the definition of the ``preprocess_distort``
kernels (``preprocess_distort_reference``: resize methods and tf_cnn_benchmarks' distort_color)
checked against independent facts -- Python's ``colorsys``, ``preprocess_reference``, block means,
identities -- and the loader arguments, the prefetcher's ``distort`` switch and the flags."""
import colorsys
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from azure_hc_intel_tf_amd.data import tfrecord as T  # noqa: E402
from azure_hc_intel_tf_amd.data.imagenet import ImageNetLoader, decode_crop, preprocess_reference  # noqa: E402

F64 = torch.float64


def _ref():
    from azure_hc_intel_tf_amd.data import imagenet

    return imagenet


def _row(db=0.0, fs=1.0, dh=0.0, fc=1.0, ordering=-1, method=1):
    return [db, fs, dh, fc, ordering, method, 0, 0]


def _run(crop, row, S, flip=0, dtype=F64, scale=(1.0,) * 3, bias=(0.0,) * 3):
    """One image through the reference, returned in 0..255 units (scale 1, bias 0) as [S, S, 3]."""
    out = torch.empty(1, S, S, 8, dtype=dtype)
    _ref().preprocess_distort_reference([crop], [flip], np.array([row], dtype=np.float32), out, scale, bias,
                                        dtype=dtype)
    assert out[..., 3:].abs().max() == 0
    return out[0, :, :, :3]


@pytest.fixture(scope="module")
def img57():
    # 5 x 7, colourful, with a grey pixel, a black one, a white one and a two-channel tie
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    a[0, 0] = (90, 90, 90)
    a[0, 1] = (0, 0, 0)
    a[0, 2] = (255, 255, 255)
    a[0, 3] = (200, 200, 10)
    return a


def _colorsys_steps(x, db, fs, dh, fc, ordering):
    """distort_color with the standard library's HSV, pixel by pixel, in Python floats."""
    x = [[[c + db for c in px] for px in row] for row in x]

    def sat_hue(x):
        out = []
        for row in x:
            o = []
            for px in row:
                h, s, v = colorsys.rgb_to_hsv(*px)
                px = colorsys.hsv_to_rgb(h, min(max(s * fs, 0.0), 1.0), v)
                h, s, v = colorsys.rgb_to_hsv(*px)
                o.append(colorsys.hsv_to_rgb((h + dh) % 1.0, s, v))
            out.append(o)
        return out

    def contrast(x):
        n = len(x) * len(x[0])
        m = [sum(px[c] for row in x for px in row) / n for c in range(3)]
        return [[[(px[c] - m[c]) * fc + m[c] for c in range(3)] for px in row] for row in x]

    x = contrast(sat_hue(x)) if ordering == 0 else sat_hue(contrast(x))
    return [[[min(max(c, 0.0), 1.0) for c in px] for px in row] for row in x]


@pytest.mark.parametrize("ordering", [0, 1])
@pytest.mark.parametrize("prm", [(0.0, 0.6, 0.13, 1.3), (0.11, 1.5, -0.2, 0.5), (0.05, 0.5, 0.2, 1.5),
                                 (0.0, 1.0, 0.0, 1.0)])
def test_colour_steps_match_colorsys(img57, ordering, prm):
    # brightness deltas >= 0 here: colorsys divides by the maximum, which must stay positive (the black
    # pixel has s = 0 there and here); the reference's behaviour at max <= 0 is its own definition
    db, fs, dh, fc = (float(np.float32(p)) for p in prm)
    x = torch.from_numpy(img57).to(F64) / 255.0
    got = _ref().distort_color_reference(x, db, fs, dh, fc, ordering)
    want = torch.tensor(_colorsys_steps(x.tolist(), db, fs, dh, fc, ordering), dtype=F64)
    assert got.shape == (5, 7, 3) and (got - want).abs().max().item() < 1e-12
    # and through the whole reference, on a square image (nearest at out = in is the source)
    crop = np.concatenate([img57, img57[:2]], 0)
    got = _run(crop, _row(db, fs, dh, fc, ordering, 0), 7) / 255.0
    want = torch.tensor(_colorsys_steps((crop.astype(np.float64) / 255.0).tolist(), db, fs, dh, fc, ordering),
                        dtype=F64)
    assert (got - want).abs().max().item() < 1e-12


def test_no_colour_bilinear_is_preprocess_reference_exactly():
    rng = np.random.default_rng(0)
    crops = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in [(30, 40), (97, 301), (33, 33)]]
    flips = [0, 1, 1]
    want = torch.empty(3, 33, 33, 8)
    preprocess_reference(crops, flips, want)
    got = torch.empty(3, 33, 33, 8)
    _ref().preprocess_distort_reference(crops, flips, np.array([_row()] * 3, dtype=np.float32), got)
    assert torch.equal(got, want)
    # the colour stage with the neutral parameters (0, 1, 0, 1) is the identity up to rounding: the HSV
    # round trip and x / 255 * 255 are not bit-exact, so this half is compared in fp64
    want64 = torch.empty(3, 33, 33, 8, dtype=F64)
    _ref().preprocess_distort_reference(crops, flips, np.array([_row()] * 3, dtype=np.float32), want64, dtype=F64)
    for ordering in (0, 1):
        got64 = torch.empty(3, 33, 33, 8, dtype=F64)
        _ref().preprocess_distort_reference(crops, flips, np.array([_row(ordering=ordering)] * 3, dtype=np.float32),
                                            got64, dtype=F64)
        assert (got64 - want64).abs().max().item() < 1e-12
    assert (want64.float() - want).abs().max().item() < 2e-4  # fp32 against fp64 coordinates, as on the GPU


def test_hue_of_one_is_identity_and_zero_saturation_is_the_maximum(img57):
    S = 7
    crop = np.concatenate([img57, img57[:2]], 0)
    src = torch.from_numpy(crop).to(F64)
    for ordering in (0, 1):
        assert (_run(crop, _row(dh=1.0, ordering=ordering, method=0), S) - src).abs().max().item() < 1e-10
        grey = _run(crop, _row(fs=0.0, ordering=ordering, method=0), S)
        assert (grey - src.max(-1, keepdim=True).values.expand(-1, -1, 3)).abs().max().item() < 1e-10


def test_zero_contrast_is_the_channel_mean(img57):
    crop = np.concatenate([img57, img57[:2]], 0)
    mean = torch.from_numpy(crop).to(F64).mean(dim=(0, 1))
    got = _run(crop, _row(fc=0.0, ordering=0, method=0), 7)
    assert (got - mean.view(1, 1, 3)).abs().max().item() < 1e-10


def test_orderings_differ_on_a_colour_image(img57):
    crop = np.concatenate([img57, img57[:2]], 0)
    a = _run(crop, _row(0.05, 1.4, 0.1, 1.4, 0, 0), 7)
    b = _run(crop, _row(0.05, 1.4, 0.1, 1.4, 1, 0), 7)
    assert (a - b).abs().max().item() > 1.0  # in 0..255 units
    # ... and agree on a grey image, where saturation and hue do nothing
    g = np.repeat(crop[:, :, :1], 3, axis=2)
    a = _run(g, _row(0.05, 1.4, 0.1, 1.4, 0, 0), 7)
    b = _run(g, _row(0.05, 1.4, 0.1, 1.4, 1, 0), 7)
    assert (a - b).abs().max().item() < 1e-10


@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_nearest_and_bicubic_at_identity_size_return_the_source(dtype):
    rng = np.random.default_rng(3)
    crop = rng.integers(0, 256, size=(13, 13, 3), dtype=np.uint8)
    src = torch.from_numpy(crop).to(dtype)
    for method in (0, 2, 3, 1):
        assert torch.equal(_run(crop, _row(method=method), 13, dtype=dtype), src), method
        assert torch.equal(_run(crop, _row(method=method), 13, flip=1, dtype=dtype), src.flip(1)), method


def test_area_at_2x_is_the_block_mean_and_nearest_picks_the_corner():
    rng = np.random.default_rng(4)
    crop = rng.integers(0, 256, size=(12, 20, 3), dtype=np.uint8)
    crop = np.ascontiguousarray(crop[:, :12])  # 12 x 12 -> 6 x 6
    src = torch.from_numpy(crop).to(F64)
    block = src.view(6, 2, 6, 2, 3).mean(dim=(1, 3))
    assert (_run(crop, _row(method=3), 6) - block).abs().max().item() < 1e-12
    assert torch.equal(_run(crop, _row(method=0), 6), src[::2, ::2])
    # an uneven reduction keeps the total: area weights sum to one per output pixel
    r = rng.integers(0, 256, size=(7, 11, 3), dtype=np.uint8)
    got = _run(r, _row(method=3), 5)
    assert abs(got.mean().item() - float(r.mean())) < 1e-9
    # upscaling: every output interval lies inside one or two source pixels
    up = _run(r, _row(method=3), 23)
    assert up.min() >= r.min() - 1e-9 and up.max() <= r.max() + 1e-9


def test_bicubic_is_keys_cubic_convolution():
    """Against the kernel function written out once more, scalar: W(x) = (a+2)|x|^3 - (a+3)|x|^2 + 1 for
    |x| <= 1, a|x|^3 - 5a|x|^2 + 8a|x| - 4a for 1 < |x| < 2, a = -0.75, taps clamped to the edge."""
    def W(x, a=-0.75):
        x = abs(x)
        return (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1 if x <= 1 else a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a \
            if x < 2 else 0.0

    rng = np.random.default_rng(8)
    h, w, S = 9, 14, 11
    crop = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    for flip in (0, 1):
        got = _run(crop, _row(method=2), S, flip=flip)
        for y in range(S):
            for xo in range(S):
                x = S - 1 - xo if flip else xo
                sy, sx = y * h / S, x * w / S
                iy, ix = int(sy), int(sx)
                want = np.zeros(3)
                for ty in range(iy - 1, iy + 3):
                    for tx in range(ix - 1, ix + 3):
                        want += W(sy - ty) * W(sx - tx) * crop[min(max(ty, 0), h - 1), min(max(tx, 0), w - 1)]
                assert np.abs(got[y, xo].numpy() - want).max() < 1e-9, (y, xo)
    # the weights sum to one: a constant image stays constant
    const = np.full((h, w, 3), 201, dtype=np.uint8)
    assert (_run(const, _row(method=2), S) - 201).abs().max().item() < 1e-10


def test_reference_rejects_bad_rows():
    crop = np.zeros((4, 4, 3), dtype=np.uint8)
    for row in (_row(method=4), _row(ordering=2), _row(fs=-1.0), _row(db=float("nan")), [0, 1, 0, 1, -1, 1, 1, 0]):
        with pytest.raises(ValueError):
            _run(crop, row, 4)


# ------------------------------------------------------------------ loader, prefetcher, flags
@pytest.fixture(scope="module")
def fake_dir(tmp_path_factory):
    import make_fake_imagenet

    d = tmp_path_factory.mktemp("fake_imagenet_distort")
    make_fake_imagenet.make(str(d), shards=2, per_shard=8, subset="train", seed=5)
    return str(d)


def _batches(fake_dir, n, seed=3, **kw):
    """n batches of a CPU loader with one slot, with the queue items (crops, desc, params) beside them."""
    ld = ImageNetLoader(fake_dir, 4, 32, 3, "cpu", train=True, seed=seed, reader_threads=1, decode_threads=2, depth=1,
                        **kw)
    out = []
    for _ in range(n):
        item = ld.ready.get()  # depth=1: the producer cannot queue another one behind it
        assert item is not None, ld._err
        ld.ready.put(item)
        img = torch.zeros(4, 32, 32, 3)
        lab = torch.zeros(4, dtype=torch.int64)
        assert ld.next_into(img, lab) == 4
        out.append((img, lab, item))
    ld.close()
    return out


def test_loader_defaults_fill_the_same_batches_as_before(fake_dir):
    for img, lab, (slot, desc, labels, crops, real, prm) in _batches(fake_dir, 3):
        assert prm is None  # the preprocess_images / preprocess_reference path
        want = torch.zeros(4, 32, 32, 3)
        preprocess_reference(crops, [int(d[3]) for d in desc], want)
        assert torch.equal(img, want)
    flips = [int(d[3]) for _, _, it in _batches(fake_dir, 4) for d in it[1]]
    assert 0 < sum(flips) < len(flips)


def test_loader_colour_is_reproducible_and_draws_in_range(fake_dir):
    a = _batches(fake_dir, 3, color=True, resize_method="round_robin")
    b = _batches(fake_dir, 3, color=True, resize_method="round_robin")
    seen = []
    for (ia, la, ita), (ib, lb, itb) in zip(a, b):
        # the seed fixes the parameter stream, and a batch is a function of its crops, flips and parameters
        # (which records the shuffle pool hands out also depends on how far the reader threads have filled it)
        prm = ita[5]
        assert np.array_equal(prm, itb[5])
        for img, it in ((ia, ita), (ib, itb)):
            want = torch.zeros(4, 32, 32, 3)
            _ref().preprocess_distort_reference(it[3], [int(d[3]) for d in it[1]], it[5], want)
            assert torch.equal(img, want)
            plain = torch.zeros(4, 32, 32, 3)
            preprocess_reference(it[3], [int(d[3]) for d in it[1]], plain)
            assert not torch.equal(img, plain)
        assert prm.dtype == np.float32 and prm.shape == (4, 8)
        assert (np.abs(prm[:, 0]) <= 32.0 / 255.0 + 1e-7).all() and (np.abs(prm[:, 2]) <= 0.2 + 1e-7).all()
        assert ((prm[:, [1, 3]] >= 0.5) & (prm[:, [1, 3]] <= 1.5)).all()
        assert prm[:, 4].tolist() == [0, 1, 0, 1] and prm[:, 5].tolist() == [0, 1, 2, 3]
        assert (prm[:, 6:] == 0).all()
        assert ia.min() >= -1.0 and ia.max() <= 1.0 + 1e-6
        seen.append(prm[:, :4].copy())
    assert not np.array_equal(seen[0], seen[1])
    other = _batches(fake_dir, 1, seed=4, color=True)[0][2][5]
    assert not np.array_equal(other[:, :4], seen[0]) and other[:, 5].tolist() == [1] * 4
    # a fixed method without colour: no colour stage, that method in every row
    for img, _, it in _batches(fake_dir, 1, resize_method="area"):
        assert it[5][:, 4].tolist() == [-1] * 4 and it[5][:, 5].tolist() == [3] * 4
    with pytest.raises(ValueError):
        ImageNetLoader(fake_dir, 4, 32, 3, "cpu", resize_method="lanczos")


def test_distort_false_is_the_central_crop_without_flip(fake_dir):
    n = T.native()
    files = T.find_shards(fake_dir, "train")
    pf = n.Prefetcher(files, threads=1, shuffle_buffer=4, seed=2, train=True, loop=False, distort=False)
    got = pf.next(1000)
    pf.stop()
    assert len(got) == 16
    central = set()
    for jpeg, lab, win, flip, (H, W) in got:
        assert flip == 0 and tuple(win) == tuple(n.central_crop(H, W, 0.875))
        central.add(decode_crop(jpeg, tuple(win), (H, W), 32, 128).tobytes())
    # shuffled like training data: not the file order an eval reader (train=False) gives
    pf = n.Prefetcher(files, threads=1, shuffle_buffer=4, seed=2, train=False, loop=False)
    assert [s[1] for s in pf.next(1000)] != [s[1] for s in got]
    pf.stop()
    # the loader: every crop is one of the central crops, no flips, colour and method switched off
    for img, lab, (slot, desc, labels, crops, real, prm) in _batches(fake_dir, 3, distort=False, color=True,
                                                                      resize_method="bicubic"):
        assert prm is None and (desc[:, 3] == 0).all()
        assert all(c.tobytes() in central for c in crops)
    # evaluation loaders ignore all three arguments
    ld = ImageNetLoader(fake_dir, 4, 32, 3, "cpu", train=False, subset="train", distort=True, color=True,
                        resize_method="area", depth=1)
    assert not ld.distort_op and not ld.color and ld.resize_method == "bilinear"
    ld.close()


def test_flags_are_parsed():
    from azure_hc_intel_tf_amd.bench.flags import parse_flags

    p = parse_flags([])
    assert p.distortions is True and p.color_distortions is False and p.resize_method == "bilinear"
    p = parse_flags(["--distortions=false", "--resize_method=area", "--color_distortions"])
    assert p.distortions is False and p.color_distortions is True and p.resize_method == "area"
    assert p._unknown == []
    assert parse_flags(["--nodistortions"]).distortions is False
    for m in ("round_robin", "nearest", "bilinear", "bicubic", "area"):
        assert parse_flags([f"--resize_method={m}"]).resize_method == m
    with pytest.raises(SystemExit):
        parse_flags(["--resize_method=lanczos"])


def test_cli_two_cpu_steps_without_distortions(fake_dir):
    cmd = [sys.executable, os.path.join(ROOT, "tf_cnn_benchmarks.py"), "--device=cpu", "--model=trivial",
           "--batch_size=4", "--num_batches=2", "--num_warmup_batches=0", "--display_every=1",
           f"--data_dir={fake_dir}", "--data_name=imagenet", "--image_size=32", "--distortions=false",
           "--resize_method=area"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Distortions: none (central crop), resize=bilinear" in r.stdout and "total images/sec" in r.stdout
    assert "Unrecognized flags" not in r.stdout
