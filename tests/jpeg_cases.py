"""Shared inputs of the JPEG decode tests: small JPEGs made at test time with Pillow's encoder from
seeded numpy arrays, and the crop windows every test uses. Nothing is read from disk."""
import functools
import io

import numpy as np

SIZES = [(8, 8), (17, 9), (33, 31), (24, 24)]  # (height, width), colour and grey
GREY_ONLY = [(15, 15)]
SUBSAMPLINGS = {"444": 0, "422": 1, "420": 2}  # Pillow's subsampling codes
QUALITIES = [5, 75, 100]
CONTENTS = ["gradient", "noise"]


def pixels(h, w, grey, content, seed=0):
    if content == "noise":
        rng = np.random.default_rng([seed, h, w, int(grey)])
        return rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    gy, gx = yy * 255 // max(h - 1, 1), xx * 255 // max(w - 1, 1)
    if grey:
        return ((gy + gx) // 2).astype(np.uint8)
    return np.stack([gy, gx, 255 - (gy + gx) // 2], axis=-1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def encode(h, w, grey, content, sub="444", quality=75, **save):
    from PIL import Image

    b = io.BytesIO()
    kw = dict(quality=quality, **save)
    if not grey:
        kw["subsampling"] = SUBSAMPLINGS[sub]
    Image.fromarray(pixels(h, w, grey, content)).save(b, "JPEG", **kw)
    return b.getvalue()


def all_cases():
    """(id, (h, w, grey, content, sub, quality)) of the issue's image set."""
    out = []
    for (h, w) in SIZES + GREY_ONLY:
        for grey in ((True,) if (h, w) in GREY_ONLY else (False, True)):
            for sub in (("444",) if grey else tuple(SUBSAMPLINGS)):
                for q in QUALITIES:
                    for content in CONTENTS:
                        cid = f"{h}x{w}-{'grey' if grey else sub}-q{q}-{content}"
                        out.append((cid, (h, w, grey, content, sub, q)))
    return out


def windows(h, w):
    """(name, (y, x, h, w)): the whole image, the last pixel of the last row, a window crossing an MCU
    boundary (of every sampling: 8 and 16 both lie inside it where the image is large enough) and one
    whose chroma margin falls outside the image (it starts at the origin / ends at the far corner)."""
    out = [("whole", (0, 0, h, w)), ("last-pixel", (h - 1, w - 1, 1, 1))]
    y0, x0 = min(5, h - 1), min(5, w - 1)
    out.append(("cross-mcu", (y0, x0, min(13, h - y0), min(13, w - x0))))
    out.append(("margin-outside-tl", (0, 0, max(1, h // 2), max(1, w // 2))))
    out.append(("margin-outside-br", (h // 2, w // 2, h - h // 2, w - w // 2)))
    return out


def decode_record(jpeg, win, capacity=1 << 20):
    """The native decoder's record for a window, parsed: (header, qtables, coefficients) or the
    decline string."""
    from azure_hc_intel_tf_amd.data import jpeg as J
    from azure_hc_intel_tf_amd.data.tfrecord import native

    buf = np.zeros(capacity, dtype=np.uint8)
    r = native().jpeg_entropy_decode(jpeg, tuple(int(v) for v in win), buf)
    if isinstance(r, str):
        return r
    return J.parse_record(buf[:r].copy())
