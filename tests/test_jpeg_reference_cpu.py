"""jpeg_decode_reference (data/jpeg.py), the definition of the jpeg_idct / jpeg_crop_rgb kernels:
a windowed decode equals the crop of the full decode bitwise, and the full decode against Pillow."""
import io
import os

import numpy as np
import pytest

import jpeg_cases as C
from azure_hc_intel_tf_amd.data import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.all_cases()


def _full(case):
    h, w = case[0], case[1]
    hdr, qt, coef = C.decode_record(C.encode(*case), (0, 0, h, w))
    return J.jpeg_decode_reference(coef, hdr, qt, 1)


@pytest.mark.parametrize("case", [c for _, c in CASES if c[5] == 75], ids=[i for i, c in CASES if c[5] == 75])
def test_crop_equals_window_bitwise(case):
    """The margin and border handling: the reference on a window's coefficients is the crop of the
    reference on the whole image, at r = 1 for every window and at r = 2 with odd crop sizes."""
    h, w = case[0], case[1]
    jpeg = C.encode(*case)
    full = _full(case)
    for name, (y, x, ch, cw) in C.windows(h, w):
        hdr, qt, coef = C.decode_record(jpeg, (y, x, ch, cw))
        got = J.jpeg_decode_reference(coef, hdr, qt, 1)
        assert got.shape == (ch, cw, 3) and np.array_equal(got, full[y:y + ch, x:x + cw]), name
    # r = 2, odd crop sizes: the 2 x 2 box mean (rounding half up) of the full decode's pixels
    def odd(n):  # the largest odd size <= n
        return n if n % 2 else n - 1

    for (y, x, ch, cw) in [(0, 0, odd(h), odd(w)), (1, 1, odd(h - 1), odd(w - 1)), (h // 2, w // 2, odd(h - h // 2), odd(w - w // 2))]:
        if ch < 3 or cw < 3:
            continue
        hdr, qt, coef = C.decode_record(jpeg, (y, x, ch, cw))
        got = J.jpeg_decode_reference(coef, hdr, qt, 2)
        oh, ow = ch // 2, cw // 2
        src = full[y:y + oh * 2, x:x + ow * 2].astype(np.int64).reshape(oh, 2, ow, 2, 3)
        assert got.shape == (oh, ow, 3) and np.array_equal(got, (src.sum(axis=(1, 3)) + 2) >> 2)


def _parity_figures():
    from PIL import Image

    worst, total, count, per = 0, 0, 0, []
    for cid, case in CASES:
        ref = _full(case).astype(np.int64)
        pil = np.asarray(Image.open(io.BytesIO(C.encode(*case))).convert("RGB")).astype(np.int64)
        d = np.abs(ref - pil)
        per.append((cid, int(d.max()), float(d.mean())))
        worst, total, count = max(worst, int(d.max())), total + int(d.sum()), count + d.size
    return worst, total / count, per


# Maximum absolute difference of the full r = 1 decode against Pillow (libjpeg-turbo's slow-integer
# IDCT, fancy upsampling and 16-bit-scaled colour tables) measured over the whole image set and recorded
# in profiles/jpeg_decode.txt: 0, mean 0 -- the decode is bit-identical.
RECORDED_MAX_ABS_DIFF = 0


def test_parity_with_pillow():
    """Full r = 1 decode against Image.open(...).convert("RGB") over the whole image set. The bound is
    the maximum recorded in profiles/jpeg_decode.txt plus one grey level; a maximum above 4 levels on
    any image would be a defect of the decoder, not a bound to record."""
    recorded = RECORDED_MAX_ABS_DIFF
    assert recorded <= 4, "a recorded maximum above 4 levels is a defect to find"
    worst, mean, per = _parity_figures()
    print(f"pillow parity r=1: max abs diff {worst}, mean abs diff {mean:.6f} over {len(per)} images")
    for cid, mx, _ in per:
        assert mx <= recorded + 1, f"{cid}: max abs diff {mx} against Pillow (recorded maximum {recorded})"


def test_draft_figure_r2_recorded_only():
    """r = 2 against Pillow's draft mode: two different filters (box mean of the full decode against a
    DCT-domain 4x4 IDCT), so the difference is printed for the record and not asserted."""
    from PIL import Image

    case = (33, 31, False, "gradient", "420", 75)
    jpeg = C.encode(*case)
    hdr, qt, coef = C.decode_record(jpeg, (0, 0, 32, 30))
    ref = J.jpeg_decode_reference(coef, hdr, qt, 2).astype(np.int64)
    img = Image.open(io.BytesIO(jpeg))
    img.draft("RGB", (15, 16))
    pil = np.asarray(img.convert("RGB")).astype(np.int64)[:16, :15]
    assert ref.shape == (16, 15, 3)
    d = np.abs(ref[:pil.shape[0], :pil.shape[1]] - pil)
    print(f"r=2 against Pillow draft (recorded only): max {int(d.max())}, mean {float(d.mean()):.3f}")


def test_idct_clamps_and_wraps_like_the_definition():
    """DC-only blocks are flat; extreme dequantised values clamp to 0 / 255."""
    q = np.ones(64, dtype=np.uint16)
    coef = np.zeros((4, 64), dtype=np.int16)
    coef[0, 0], coef[1, 0], coef[2, 0], coef[3, 0] = 80, -80, 32767, -32768
    out = J.idct_reference(coef, q)
    assert (out[0] == 138).all() and (out[1] == 118).all() and (out[2] == 255).all() and (out[3] == 0).all()


def test_reduction_rule_matches_decode_crop():
    for h, w, s in [(500, 375, 224), (448, 448, 224), (447, 900, 224), (4000, 3000, 224), (10, 10, 224), (1800, 1792, 224)]:
        r = 1
        while r < 8 and min(h, w) // (r * 2) >= s:
            r *= 2
        assert J.reduction(h, w, s) == r
    assert J.coef_budget(896) % 16 == 0 and J.coef_budget(896) >= 3 * 896 * 896
