"""GPU JPEG decode (``--gpu_jpeg_decode``): the definition of its two kernels, and their tables.

The split. The host does only what is serial: ``jpeg_entropy_decode`` (csrc/data/jpeg.cpp) turns the
Huffman-coded scan into quantised DCT coefficients of the MCU-aligned block window a crop needs and
writes one record (layout: csrc/data/jpeg.h; ``parse_record`` here). The GPU does the rest in two
kernels (csrc/kernels/jpeg.hip): ``jpeg_idct`` (dequantise + 8x8 inverse DCT + level shift, one plane
per component) and ``jpeg_crop_rgb`` (chroma upsampling, YCbCr -> RGB, r x r box mean, packed crop).

``jpeg_decode_reference`` is the definition of both kernels in numpy integer arithmetic; the GPU
result equals it bitwise, and with ``--device=cpu`` it is the code that runs.

  IDCT          32-bit wrapping integer arithmetic, the separable Loeffler-Ligtenberg-Moschytz form
                with 13-bit constants (the "slow integer" IDCT): columns first, descaled by 11 bits
                with rounding, then rows, descaled by 18 bits with rounding, + 128, clamped to 0..255.
  upsampling    "fancy" triangle filter where a chroma axis is subsampled: weights 3/4 to the nearer
                and 1/4 to the farther chroma sample; one axis (3 a + b + {1, 2}) >> 2 with the bias
                alternating by output parity, both axes (3 (3 a + b) + (3 c + d) + {8, 7}) >> 4 with
                the bias alternating by output column. The neighbour is replicated at the image's
                true border only (the window carries one sample of margin inside the image).
  colour        R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
                B = Y + ((116130 Cb' + 32768) >> 16), Cb' = Cb - 128, Cr' = Cr - 128, clamped; grey
                images take R = G = B = Y.
  reduction     output pixel (i, j) = mean over the r x r full-resolution pixels from
                (y + i r, x + j r), per channel, (sum + r r / 2) >> log2(r r); the crop becomes
                (h // r, w // r). ``reduction`` gives r by decode_crop's rule.

``entropy_decode_python`` decodes the entropy stage slowly and independently (tests only).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

HDR_INTS = 32
HDR_MAGIC = 0x3147504A
QT_OFFSET = HDR_INTS * 4
COEF_OFFSET = QT_OFFSET + 4 * 64 * 2
IDCT_GROUP = 32  # blocks per workgroup of jpeg_idct: the unit of the segment table's prefix

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def coef_budget(max_side: int) -> int:
    """Bytes of one image's record the loader provides: 3 bytes per source pixel (int16 coefficients,
    1.5 samples per pixel at 4:2:0) of a max_side x max_side window. A larger window is declined."""
    return (COEF_OFFSET + 3 * max_side * max_side + 15) // 16 * 16


def reduction(h: int, w: int, out_size: int) -> int:
    """decode_crop's rule: double while the reduced crop keeps both sides >= out_size, at most 8."""
    r = 1
    while r < 8 and min(h, w) // (r * 2) >= out_size:
        r *= 2
    return r


def parse_record(buf) -> Tuple[Dict, np.ndarray, np.ndarray]:
    """One record written by jpeg_entropy_decode -> (header dict, qtables uint16 [4][64], coefficients
    int16 [nblocks][64]); the arrays are views of ``buf``."""
    buf = np.asarray(buf, dtype=np.uint8)
    h = buf[:QT_OFFSET].view(np.int32)
    if int(h[0]) != HDR_MAGIC:
        raise ValueError("not a jpeg_entropy_decode record")
    hdr = dict(ncomp=int(h[1]), hs=int(h[2]), vs=int(h[3]), H=int(h[4]), W=int(h[5]), cy=int(h[6]), cx=int(h[7]),
               ch=int(h[8]), cw=int(h[9]), oy=int(h[10]), ox=int(h[11]), nblocks=int(h[30]), nbytes=int(h[31]),
               comps=[dict(bx0=int(h[12 + 6 * c]), by0=int(h[13 + 6 * c]), bw=int(h[14 + 6 * c]), bh=int(h[15 + 6 * c]),
                           tq=int(h[16 + 6 * c]), first=int(h[17 + 6 * c])) for c in range(int(h[1]))])
    qt = buf[QT_OFFSET:COEF_OFFSET].view(np.uint16).reshape(4, 64)
    coef = buf[COEF_OFFSET:COEF_OFFSET + hdr["nblocks"] * 128].view(np.int16).reshape(-1, 64)
    return hdr, qt, coef


# ------------------------------------------------------------------------------------ the definition
_C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137,
          c1961=16069, c2053=16819, c2562=20995, c3072=25172)


def _idct_1d(v: List[np.ndarray], shift: int) -> List[np.ndarray]:
    """One pass over 8 int32 arrays (the elements of a column or a row), wrapping arithmetic."""
    i32 = np.int32
    K = {k: i32(c) for k, c in _C.items()}
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * K["c0541"]
    t2 = z1 - z3 * K["c1847"]
    t3 = z1 + z2 * K["c0765"]
    t0 = (v[0] + v[4]) << i32(13)
    t1 = (v[0] - v[4]) << i32(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * K["c1175"]
    t0 = t0 * K["c0298"]
    t1 = t1 * K["c2053"]
    t2 = t2 * K["c3072"]
    t3 = t3 * K["c1501"]
    z1 = -(z1 * K["c0899"])
    z2 = -(z2 * K["c2562"])
    z3 = -(z3 * K["c1961"]) + z5
    z4 = -(z4 * K["c0390"]) + z5
    t0 = t0 + z1 + z3
    t1 = t1 + z2 + z4
    t2 = t2 + z2 + z3
    t3 = t3 + z1 + z4
    rnd = i32(1 << (shift - 1))
    sh = i32(shift)
    return [(t10 + t3 + rnd) >> sh, (t11 + t2 + rnd) >> sh, (t12 + t1 + rnd) >> sh, (t13 + t0 + rnd) >> sh,
            (t13 - t0 + rnd) >> sh, (t12 - t1 + rnd) >> sh, (t11 - t2 + rnd) >> sh, (t10 - t3 + rnd) >> sh]


def idct_reference(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """``jpeg_idct``'s definition: coef int16 [n][64] (natural order), q uint16 [64] -> uint8 [n][8][8]."""
    with np.errstate(over="ignore"):
        x = (coef.astype(np.int32) * q.astype(np.int32)[None, :]).reshape(-1, 8, 8)  # [n][row][col]
        cols = _idct_1d([x[:, r, :] for r in range(8)], 11)  # down the columns: element r of every column
        ws = np.stack(cols, axis=1)
        rows = _idct_1d([ws[:, :, c] for c in range(8)], 18)  # along the rows
        out = np.stack(rows, axis=2) + np.int32(128)
    return np.clip(out, 0, 255).astype(np.uint8)


def _planes(coeffs: np.ndarray, header: Dict, qtables: np.ndarray) -> List[np.ndarray]:
    """IDCT of every component's window -> uint8 planes [bh * 8][bw * 8]."""
    planes = []
    for c in header["comps"]:
        n = c["bw"] * c["bh"]
        blk = idct_reference(coeffs[c["first"]:c["first"] + n], qtables[c["tq"]])
        planes.append(blk.reshape(c["bh"], c["bw"], 8, 8).transpose(0, 2, 1, 3).reshape(c["bh"] * 8, c["bw"] * 8))
    return planes


def _chroma(plane: np.ndarray, comp: Dict, Y: np.ndarray, X: np.ndarray, hs: int, vs: int, H: int, W: int) -> np.ndarray:
    """Upsampled chroma at the full-resolution pixels (Y[:, None], X[None, :]) as int32."""
    y0, x0 = comp["by0"] * 8, comp["bx0"] * 8

    def taps(P, f, n):  # nearer and farther sample along one axis, in plane coordinates
        if f == 1:
            return P, P
        c = P >> 1
        far = np.clip(np.where(P & 1, c + 1, c - 1), 0, (n + 1) // 2 - 1)
        return c, far

    ya, yb = taps(Y, vs, H)
    xa, xb = taps(X, hs, W)
    p = plane.astype(np.int32)

    def at(yy, xx):
        return p[(yy - y0)[:, None], (xx - x0)[None, :]]

    if hs == 1 and vs == 1:
        return at(ya, xa)
    if vs == 1:
        return (3 * at(ya, xa) + at(ya, xb) + np.where(X & 1, 2, 1)[None, :]) >> 2
    if hs == 1:
        return (3 * at(ya, xa) + at(yb, xa) + np.where(Y & 1, 2, 1)[:, None]) >> 2
    near = 3 * at(ya, xa) + at(yb, xa)
    far = 3 * at(ya, xb) + at(yb, xb)
    return (3 * near + far + np.where(X & 1, 7, 8)[None, :]) >> 4


def jpeg_decode_reference(coeffs: np.ndarray, header: Dict, qtables: np.ndarray, r: int = 1) -> np.ndarray:
    """Definition of ``jpeg_idct`` + ``jpeg_crop_rgb``: one record's coefficients int16 [nblocks][64],
    its header (``parse_record``) and quantisation tables -> the crop as RGB uint8 [ch // r][cw // r][3]."""
    if r not in (1, 2, 4, 8):
        raise ValueError(f"reduction {r}: 1 | 2 | 4 | 8")
    oh, ow = header["ch"] // r, header["cw"] // r
    if oh < 1 or ow < 1:
        raise ValueError(f"crop {header['ch']} x {header['cw']} is smaller than the reduction {r}")
    planes = _planes(coeffs, header, qtables)
    Y = header["cy"] + np.arange(oh * r)
    X = header["cx"] + np.arange(ow * r)
    c0 = header["comps"][0]
    lum = planes[0].astype(np.int32)[(Y - c0["by0"] * 8)[:, None], (X - c0["bx0"] * 8)[None, :]]
    if header["ncomp"] == 1:
        rgb = np.stack([lum, lum, lum], axis=-1)
    else:
        hs, vs, H, W = header["hs"], header["vs"], header["H"], header["W"]
        cb = _chroma(planes[1], header["comps"][1], Y, X, hs, vs, H, W) - 128
        cr = _chroma(planes[2], header["comps"][2], Y, X, hs, vs, H, W) - 128
        rgb = np.stack([lum + ((91881 * cr + 32768) >> 16), lum + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                        lum + ((116130 * cb + 32768) >> 16)], axis=-1)
        rgb = np.clip(rgb, 0, 255)
    if r > 1:
        rgb = (rgb.reshape(oh, r, ow, r, 3).sum(axis=(1, 3)) + (r * r) // 2) >> (2 * (r.bit_length() - 1))
    return np.ascontiguousarray(rgb.astype(np.uint8))


# ------------------------------------------------------------------------------------ kernel tables
SEG_COLS = 8   # jpeg_idct rows: group0, nblocks, coef byte offset, record byte offset, qtable, plane byte offset, 0, 0
IMG_COLS = 24  # jpeg_crop_rgb rows: ncomp (0: not a GPU image), r, hs, vs, H, W, y0, x0, then per component
#                (plane byte offset, bx0, by0, bw, bh), 0


def build_tables(headers: List[Optional[Dict]], record_offsets: List[int], rs: List[int]):
    """The device tables of one batch. headers[i] is None for an image that is not decoded on the GPU
    (a fallback crop or a padding row). Returns (segments int64 [nseg][8], images int64 [B][24], plane
    bytes needed, workgroups of jpeg_idct)."""
    segs, imgs = [], np.zeros((len(headers), IMG_COLS), dtype=np.int64)
    group, plane = 0, 0
    for i, h in enumerate(headers):
        if h is None:
            continue
        imgs[i, :8] = (h["ncomp"], rs[i], h["hs"], h["vs"], h["H"], h["W"], h["cy"], h["cx"])
        for c, comp in enumerate(h["comps"]):
            n = comp["bw"] * comp["bh"]
            segs.append((group, n, record_offsets[i] + COEF_OFFSET + comp["first"] * 128, record_offsets[i], comp["tq"],
                         plane, 0, 0))
            imgs[i, 8 + 5 * c:13 + 5 * c] = (plane, comp["bx0"], comp["by0"], comp["bw"], comp["bh"])
            group += (n + IDCT_GROUP - 1) // IDCT_GROUP
            plane += n * 64
    return np.array(segs, dtype=np.int64).reshape(-1, SEG_COLS), imgs, plane, group


# ------------------------------------------------------------------------------------ slow entropy decoder
class Declined(Exception):
    pass


def entropy_decode_python(data: bytes):
    """Independent, slow Huffman decode of a whole baseline JPEG (tests only). Returns a dict: H, W,
    ncomp, hs, vs, qtables uint16 [4][64] (natural order), tq per component, and per component the
    int16 coefficients [blocks_y][blocks_x][64] (natural order) of its full block grid."""
    d = data
    if d[:2] != b"\xff\xd8":
        raise Declined("not a JPEG")
    pos = 2
    qt = np.zeros((4, 64), dtype=np.uint16)
    tables = {}
    frame = None
    restart = 0
    while True:
        if d[pos] != 0xFF:
            raise Declined("marker expected")
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        ln = (d[pos] << 8) | d[pos + 1]
        seg = d[pos + 2:pos + ln]
        pos += ln
        if m in (0xC0, 0xC1):
            H, W, n = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = dict(H=H, W=W, comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c])
                                          for c in range(n)])
        elif m == 0xC2:
            raise Declined("progressive")
        elif m == 0xDB:
            o = 0
            while o < len(seg):
                pq, tq = seg[o] >> 4, seg[o] & 15
                for i in range(64):
                    qt[tq, ZIGZAG[i]] = ((seg[o + 1 + 2 * i] << 8) | seg[o + 2 + 2 * i]) if pq else seg[o + 1 + i]
                o += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                tc, th = seg[o] >> 4, seg[o] & 15
                counts = list(seg[o + 1:o + 17])
                vals = seg[o + 17:o + 17 + sum(counts)]
                codes, code, k = {}, 0, 0
                for ln_ in range(1, 17):
                    for _ in range(counts[ln_ - 1]):
                        codes[(ln_, code)] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                tables[(tc, th)] = codes
                o += 17 + sum(counts)
        elif m == 0xDD:
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            scan = [(seg[1 + 2 * c], seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            break
    comps = frame["comps"]
    n = len(comps)
    hs, vs = (comps[0][1], comps[0][2]) if n == 3 else (1, 1)
    H, W = frame["H"], frame["W"]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    fac = [(hs, vs)] + [(1, 1)] * (n - 1)
    out = [np.zeros((mcuy * fv, mcux * fh, 64), dtype=np.int16) for fh, fv in fac]

    # the entropy-coded bytes as one bit string per restart interval
    state = dict(pos=pos, bits="", at=0)

    def load_interval():
        p = state["pos"]
        chunk = bytearray()
        while True:
            b = d[p]
            if b == 0xFF:
                if d[p + 1] == 0:
                    chunk.append(0xFF)
                    p += 2
                    continue
                break
            chunk.append(b)
            p += 1
        while d[p] == 0xFF and d[p + 1] == 0xFF:
            p += 1
        state["pos"] = p + 2  # past the marker that ended the interval
        state["bits"] = "".join(f"{b:08b}" for b in chunk)
        state["at"] = 0

    def symbol(tab):
        bits, at = state["bits"], state["at"]
        code = 0
        for ln_ in range(1, 17):
            code = (code << 1) | int(bits[at + ln_ - 1])
            if (ln_, code) in tab:
                state["at"] = at + ln_
                return tab[(ln_, code)]
        raise Declined("bad code")

    def receive(s):
        if s == 0:
            return 0
        at = state["at"]
        v = int(state["bits"][at:at + s], 2)
        state["at"] = at + s
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1

    load_interval()
    pred = [0] * n
    for mcu in range(mcux * mcuy):
        if restart and mcu and mcu % restart == 0:
            load_interval()
            pred = [0] * n
        my, mx = divmod(mcu, mcux)
        for c in range(n):
            fh, fv = fac[c]
            dc, ac = tables[(0, scan[c][1])], tables[(1, scan[c][2])]
            for v in range(fv):
                for h in range(fh):
                    blk = out[c][my * fv + v, mx * fh + h]
                    pred[c] += receive(symbol(dc))
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = symbol(ac)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        blk[ZIGZAG[k]] = receive(s)
                        k += 1
    return dict(H=H, W=W, ncomp=n, hs=hs, vs=vs, qtables=qt, tq=[c[3] for c in comps], coeffs=out)


def expected_window(H: int, W: int, hs: int, vs: int, win: Tuple[int, int, int, int]) -> Tuple[int, int, int, int]:
    """The MCU window (mx0, my0, mx1, my1, inclusive) the decoder stores for a crop: the crop's
    pixels plus one chroma sample of margin on each subsampled axis, clipped to the image."""
    y, x, h, w = win

    def span(lo, ln_, f, full):
        if f == 2:
            c0 = max((lo >> 1) - 1, 0)
            c1 = min(((lo + ln_ - 1) >> 1) + 1, (full + 1) // 2 - 1)
        else:
            c0, c1 = lo, lo + ln_ - 1
        return c0 // 8, c1 // 8

    mx0, mx1 = span(x, w, hs, W)
    my0, my1 = span(y, h, vs, H)
    return mx0, my0, mx1, my1
