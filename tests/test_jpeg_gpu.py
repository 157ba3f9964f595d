"""The jpeg_idct / jpeg_crop_rgb HIP kernels against their definition (data/jpeg.py
jpeg_decode_reference), bitwise; the stage layout they leave for preprocess_images; the launches the
binding rejects; and ImageNetLoader(gpu_decode=True) against gpu_decode=False."""
import io
import os
import sys

import numpy as np
import pytest
import torch

import jpeg_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def _items():
    """(jpeg, window, r): every subsampling, grey, odd sizes; the whole image, the four corners and the
    MCU-crossing window at r = 1, odd-sized crops at r = 2. 33x31 at 4:2:0 has 3 x 2 MCUs, 100x77 enough
    blocks (91 luma) that a component spans several 32-block workgroups with a partial last one."""
    out = []
    cases = [(33, 31, False, "noise", s, 75) for s in C.SUBSAMPLINGS] + \
            [(17, 9, False, "gradient", "420", 5), (8, 8, False, "noise", "422", 100), (15, 15, True, "noise", "444", 75),
             (24, 24, True, "gradient", "444", 100), (100, 77, False, "noise", "420", 75)]
    for case in cases:
        h, w = case[0], case[1]
        jpeg = C.encode(*case)
        wins = [(0, 0, h, w)]
        if min(h, w) >= 9:
            ch, cw = h // 2 + 1, w // 2 + 1
            wins += [(0, 0, ch, cw), (0, w - cw, ch, cw), (h - ch, 0, ch, cw), (h - ch, w - cw, ch, cw),
                     (5, 5, min(13, h - 5), min(13, w - 5))]
        out += [(jpeg, win, 1) for win in wins]
        if min(h, w) >= 9:
            odd_h, odd_w = (h if h % 2 else h - 1), (w if w % 2 else w - 1)
            out += [(jpeg, (0, 0, odd_h, odd_w), 2), (jpeg, (h - odd_h, w - odd_w, odd_h, odd_w), 2)]
    return out


def _assemble(items, fallback=None):
    """Records packed back to back, the tables, the descriptors and the reference crops of a batch;
    ``fallback`` = (position, RGB crop): a Pillow-decoded image at that batch position, whose crop lies
    in the stage behind the kernel-written ones."""
    from azure_hc_intel_tf_amd.data import jpeg as J
    from azure_hc_intel_tf_amd.data.tfrecord import native

    B = len(items) + (1 if fallback else 0)
    headers, offsets, rs, refs, chunks = [None] * B, [0] * B, [1] * B, [None] * B, []
    pos = 0
    slots = [i for i in range(B) if not fallback or i != fallback[0]]
    for i, (jpeg, win, r) in zip(slots, items):
        buf = np.zeros(1 << 18, dtype=np.uint8)
        n = native().jpeg_entropy_decode(jpeg, win, buf)
        assert isinstance(n, int), n
        hdr, qt, coef = J.parse_record(buf[:n])
        headers[i], offsets[i], rs[i] = hdr, pos, r
        refs[i] = J.jpeg_decode_reference(coef, hdr, qt, r)
        chunks.append(buf[:(n + 15) // 16 * 16])
        pos += chunks[-1].size
    desc = np.zeros((B, 4), dtype=np.int64)
    off = 0
    for i in slots:
        desc[i] = (off, refs[i].shape[0], refs[i].shape[1], i % 2)
        off += (refs[i].size + 15) // 16 * 16
    gpu_bytes = off
    if fallback:
        i, crop = fallback
        refs[i] = crop
        desc[i] = (off, crop.shape[0], crop.shape[1], 1)
        off += (crop.size + 15) // 16 * 16
    segs, imgs, plane_bytes, groups = J.build_tables(headers, offsets, rs)
    return dict(coef=np.concatenate(chunks), segs=segs, imgs=imgs, desc=desc, refs=refs, plane_bytes=plane_bytes,
                stage_bytes=off, gpu_bytes=gpu_bytes, groups=groups)


def _run(b, fallback=None, fill=0x5A):
    """Both kernels over an assembled batch -> the stage as a numpy array. Scratch and stage start
    filled with a pattern: nothing may rely on zeroed memory."""
    from azure_hc_intel_tf_amd.ops import _ext

    coef = torch.from_numpy(b["coef"]).cuda()
    planes = torch.full((b["plane_bytes"] + 64,), fill, dtype=torch.uint8, device="cuda")
    stage = torch.full((b["stage_bytes"] + 64,), fill, dtype=torch.uint8, device="cuda")
    segs_h, imgs_h, desc_h = (torch.from_numpy(b[k]) for k in ("segs", "imgs", "desc"))
    if fallback is not None:  # the loader's upload of a Pillow-decoded crop behind the kernel-written ones
        i, crop = fallback
        o = int(b["desc"][i, 0])
        stage[o:o + crop.size] = torch.from_numpy(crop.reshape(-1)).cuda()
    _ext.ops().jpeg_idct(coef, segs_h.cuda(), segs_h, planes)
    _ext.ops().jpeg_crop_rgb(planes, imgs_h.cuda(), imgs_h, desc_h.cuda(), desc_h, stage)
    torch.cuda.synchronize()
    return stage, planes


@pytest.fixture(scope="module")
def mixed_batch():
    from PIL import Image

    crop = np.asarray(Image.open(io.BytesIO(C.encode(24, 24, False, "noise", "420", 75))).convert("RGB"))[3:20, 2:21]
    crop = np.ascontiguousarray(crop)
    fallback = (3, crop)
    b = _assemble(_items(), fallback)
    stage, planes = _run(b, fallback)
    return b, stage, fallback


def test_kernels_equal_the_definition_bitwise(mixed_batch):
    b, stage, fallback = mixed_batch
    assert b["groups"] > len(b["segs"])  # some segment spans more than one workgroup
    host = stage.cpu().numpy()
    bad = []
    for i, ref in enumerate(b["refs"]):
        o = int(b["desc"][i, 0])
        got = host[o:o + ref.size].reshape(ref.shape)
        if not np.array_equal(got, ref):
            bad.append((i, int(np.abs(got.astype(int) - ref.astype(int)).max())))
    assert not bad, f"(batch position, max abs diff) of the crops that differ: {bad}"
    # nothing written past the last crop or into the 16-byte padding between crops
    assert (host[b["stage_bytes"]:] == 0x5A).all()
    for i, ref in enumerate(b["refs"]):
        o = int(b["desc"][i, 0]) + ref.size
        assert (host[o:(o + 15) // 16 * 16] == 0x5A).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_stage_layout_feeds_preprocess_images(mixed_batch, dtype):
    from azure_hc_intel_tf_amd.data.imagenet import BIAS, SCALE, preprocess_reference
    from azure_hc_intel_tf_amd.ops import _ext

    b, stage, _ = mixed_batch
    B, S = len(b["refs"]), 32
    desc_h = torch.from_numpy(b["desc"])
    out = torch.full((B, S, S, 8), 7.0, dtype=dtype, device="cuda")
    _ext.ops().preprocess_images(stage, desc_h.cuda(), desc_h, out, list(SCALE), list(BIAS))
    ref = torch.empty(B, S, S, 8)
    preprocess_reference(b["refs"], [int(d[3]) for d in b["desc"]], ref)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < (1e-2 if dtype == torch.bfloat16 else 2e-4), err  # the bound of test_data_gpu.py


def _synthetic_record(coef_blocks, q):
    """A one-component record of a 1 x n block row around hand-made coefficients."""
    from azure_hc_intel_tf_amd.data import jpeg as J

    n = coef_blocks.shape[0]
    hdr = np.zeros(J.HDR_INTS, dtype=np.int32)
    hdr[:12] = (J.HDR_MAGIC, 1, 1, 1, 8, 8 * n, 0, 0, 8, 8 * n, 0, 0)
    hdr[12:18] = (0, 0, n, 1, 2, 0)
    hdr[30], hdr[31] = n, J.COEF_OFFSET + 128 * n
    qt = np.zeros((4, 64), dtype=np.uint16)
    qt[2] = q
    return np.concatenate([hdr.view(np.uint8), qt.reshape(-1).view(np.uint8), coef_blocks.reshape(-1).view(np.uint8)])


def test_clamp_paths_match_the_definition():
    """DC-only blocks, and blocks whose dequantised values sit at the int16 extremes (where the 32-bit
    arithmetic of the definition wraps), through both kernels."""
    from azure_hc_intel_tf_amd.data import jpeg as J

    rng = np.random.default_rng(3)
    blocks = np.zeros((40, 64), dtype=np.int16)
    blocks[0, 0], blocks[1, 0], blocks[2, 0], blocks[3, 0] = 80, -80, 4681, -4681  # x 7: up to +/- 32767
    blocks[4] = 4681
    blocks[5] = -4681
    blocks[6, ::2], blocks[6, 1::2] = 4681, -4681
    blocks[7:] = rng.choice(np.array([-4681, 4681, 0, 1, -1], dtype=np.int16), size=(33, 64))
    q = np.full(64, 7, dtype=np.uint16)
    rec = _synthetic_record(blocks, q)
    hdr, qt, coef = J.parse_record(rec)
    assert int(coef.astype(np.int32).max() * 7) == 32767 and int(coef.astype(np.int32).min() * 7) == -32767
    ref = J.jpeg_decode_reference(coef, hdr, qt, 1)
    assert (ref[:, 16:24] == 255).all() and (ref[:, 24:32] == 0).all()  # the two clamps
    segs, imgs, plane_bytes, groups = J.build_tables([hdr], [0], [1])
    desc = np.array([[0, 8, 8 * 40, 0]], dtype=np.int64)
    b = dict(coef=rec, segs=segs, imgs=imgs, desc=desc, plane_bytes=plane_bytes, stage_bytes=ref.size)
    stage, _ = _run(b)
    assert np.array_equal(stage.cpu().numpy()[:ref.size].reshape(ref.shape), ref)
    # the same at the 16-bit table's and the coefficients' extremes: +/- 32767 x 65535
    blocks2 = rng.choice(np.array([-32768, 32767, 0, 3], dtype=np.int16), size=(5, 64))
    rec2 = _synthetic_record(blocks2, np.full(64, 65535, dtype=np.uint16))
    hdr2, qt2, coef2 = J.parse_record(rec2)
    ref2 = J.jpeg_decode_reference(coef2, hdr2, qt2, 1)
    segs2, imgs2, pb2, _ = J.build_tables([hdr2], [0], [1])
    b2 = dict(coef=rec2, segs=segs2, imgs=imgs2, desc=np.array([[0, 8, 40, 0]], dtype=np.int64), plane_bytes=pb2,
              stage_bytes=ref2.size)
    stage2, _ = _run(b2)
    assert np.array_equal(stage2.cpu().numpy()[:ref2.size].reshape(ref2.shape), ref2)


def test_rejected_launches(mixed_batch):
    """Rows with an out-of-range window, offset or table index are refused by the binding, by name,
    before anything is launched."""
    from azure_hc_intel_tf_amd.ops import _ext

    b, _, _ = mixed_batch
    ops = _ext.ops()
    coef = torch.from_numpy(b["coef"]).cuda()
    planes = torch.zeros(b["plane_bytes"], dtype=torch.uint8, device="cuda")
    stage = torch.zeros(b["stage_bytes"], dtype=torch.uint8, device="cuda")
    segs_h, imgs_h, desc_h = (torch.from_numpy(b[k]) for k in ("segs", "imgs", "desc"))

    def idct(mut, match):
        bad = segs_h.clone()
        mut(bad)
        with pytest.raises(RuntimeError, match=match):
            ops.jpeg_idct(coef, bad.cuda(), bad, planes)

    def setv(r, c, v):
        def f(t):
            t[r, c] = v
        return f

    idct(setv(1, 4, 4), "quantisation table index of segment 1")
    idct(setv(1, 4, -1), "quantisation table index of segment 1")
    idct(setv(2, 1, 1 << 20), "outside")
    idct(setv(0, 2, b["coef"].size), "coefficients of segment 0 outside coef")
    idct(setv(0, 2, 8), "coefficients of segment 0 outside coef")
    idct(setv(3, 0, 1), "group prefix of segment 3")
    idct(setv(len(b["segs"]) - 1, 5, b["plane_bytes"]), "plane of segment")
    idct(setv(0, 3, b["coef"].size - 16), "record of segment 0 outside coef")
    with pytest.raises(RuntimeError, match="segs_host must be the CPU copy"):
        ops.jpeg_idct(coef, segs_h.cuda(), segs_h[:-1].contiguous(), planes)

    def crop(mut_imgs=None, mut_desc=None, match=""):
        bi, bd = imgs_h.clone(), desc_h.clone()
        if mut_imgs:
            mut_imgs(bi)
        if mut_desc:
            mut_desc(bd)
        with pytest.raises(RuntimeError, match=match):
            ops.jpeg_crop_rgb(planes, bi.cuda(), bi, bd.cuda(), bd, stage)

    crop(setv(0, 6, 1), None, "crop window of image 0 outside the image")      # y0 + h past the image
    crop(None, setv(0, 2, 64), "crop window of image 0 outside the image")     # wider than the image
    crop(setv(1, 9, 1), None, "block window of image 1 component 0 does not cover its crop")  # bx0 moved
    crop(setv(0, 11, 1), None, "block window of image 0 component 0 does not cover its crop")  # bw shrunk
    crop(setv(0, 14, 1), None, "block window of image 0 component 1 does not cover its crop")  # chroma margin
    crop(setv(0, 8, b["plane_bytes"]), None, "plane of image 0 component 0 outside planes")
    crop(setv(0, 1, 3), None, "reduction of image 0")
    crop(setv(0, 2, 4), None, "sampling factors of image 0")
    crop(setv(0, 0, 2), None, "component count of image 0")
    crop(None, setv(len(b["refs"]) - 1, 0, b["stage_bytes"]), "outside the staging buffer")


def test_loader_parity(tmp_path):
    """gpu_decode on against off, same seed, at 256 px where every crop of the fake set (sides <= 500)
    keeps the reduction at 1 on both paths: identical labels, windows and flips, images within the Pillow
    parity bound (recorded maximum 0, plus one grey level) carried through the bilinear resize -- a convex
    combination, so one level stays one level, 1 / 127.5 after the normalisation -- and no declines."""
    import make_fake_imagenet

    from azure_hc_intel_tf_amd.data.imagenet import ImageNetLoader

    make_fake_imagenet.make(str(tmp_path), shards=2, per_shard=16, seed=3)
    got = []
    for gpu_decode in (False, True):
        # one reader thread and one pass (loop=False): the shuffle pool holds the whole set before the first
        # draw, so the order of the samples is a function of the seed alone and not of thread timing
        ld = ImageNetLoader(str(tmp_path), 8, 256, 8, "cuda:0", seed=4, reader_threads=1, decode_threads=4, depth=2,
                            loop=False, gpu_decode=gpu_decode)
        img = torch.zeros(8, 256, 256, 8, dtype=torch.float32, device="cuda")
        lab = torch.zeros(8, dtype=torch.int64, device="cuda")
        batches = []
        for _ in range(3):
            assert ld.next_into(img, lab) == 8
            torch.cuda.synchronize()
            batches.append((img.cpu().clone(), lab.cpu().clone(), ld.dev_desc.cpu().clone()))
        got.append(batches)
        ld.close()
        if gpu_decode:
            assert ld.gpu_declined == 0 and ld.gpu_decoded >= 24
    for (i0, l0, d0), (i1, l1, d1) in zip(*got):
        assert torch.equal(l0, l1)
        assert torch.equal(d0[:, 1:], d1[:, 1:])  # crop sizes and flips (the offsets depend on the packing)
        err = (i0 - i1).abs().max().item()
        assert err <= 1.0 / 127.5 + 1e-6, err
