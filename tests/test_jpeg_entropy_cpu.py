"""The native baseline JPEG entropy decoder (csrc/data/jpeg.cpp) against the slow pure-Python Huffman
decoder of data/jpeg.py: coefficients and header fields, windowing, restart intervals, declines."""
import io

import numpy as np
import pytest

import jpeg_cases as C
from azure_hc_intel_tf_amd.data import jpeg as J


def _check_window(jpeg, win, slow):
    """One window of one image against the slow decode of the whole image."""
    rec = C.decode_record(jpeg, win)
    assert not isinstance(rec, str), rec
    hdr, qt, coef = rec
    H, W, hs, vs = slow["H"], slow["W"], slow["hs"], slow["vs"]
    assert (hdr["H"], hdr["W"], hdr["ncomp"], hdr["hs"], hdr["vs"]) == (H, W, slow["ncomp"], hs, vs)
    assert (hdr["cy"], hdr["cx"], hdr["ch"], hdr["cw"]) == tuple(win)
    mx0, my0, mx1, my1 = J.expected_window(H, W, hs, vs, win)
    nblocks = 0
    for c, comp in enumerate(hdr["comps"]):
        fh, fv = (hs, vs) if c == 0 else (1, 1)
        assert (comp["bx0"], comp["by0"], comp["bw"], comp["bh"]) == (mx0 * fh, my0 * fv, (mx1 - mx0 + 1) * fh,
                                                                      (my1 - my0 + 1) * fv)
        assert comp["tq"] == slow["tq"][c] and comp["first"] == nblocks
        n = comp["bw"] * comp["bh"]
        got = coef[nblocks:nblocks + n].reshape(comp["bh"], comp["bw"], 64)
        # the same blocks cut out of the full-image decode
        want = slow["coeffs"][c][comp["by0"]:comp["by0"] + comp["bh"], comp["bx0"]:comp["bx0"] + comp["bw"]]
        assert np.array_equal(got, want), f"component {c}"
        nblocks += n
    assert hdr["nblocks"] == nblocks == coef.shape[0]
    assert hdr["nbytes"] == J.COEF_OFFSET + 128 * nblocks
    assert (hdr["oy"], hdr["ox"]) == (win[0] - 8 * hdr["comps"][0]["by0"], win[1] - 8 * hdr["comps"][0]["bx0"])
    assert np.array_equal(qt, slow["qtables"])


@pytest.mark.parametrize("case", [c for _, c in C.all_cases()], ids=[i for i, _ in C.all_cases()])
def test_coefficients_and_header(case):
    jpeg = C.encode(*case)
    slow = J.entropy_decode_python(jpeg)
    for _, win in C.windows(case[0], case[1]):
        _check_window(jpeg, win, slow)


def test_windowed_equals_cut_from_full_decode():
    """A window's coefficients are the same blocks of the full-image record (native against native)."""
    jpeg = C.encode(33, 31, False, "noise", "420", 75)
    fh, fq, fc = C.decode_record(jpeg, (0, 0, 33, 31))
    for _, win in C.windows(33, 31):
        hdr, qt, coef = C.decode_record(jpeg, win)
        for c, comp in enumerate(hdr["comps"]):
            full = fh["comps"][c]
            grid = fc[full["first"]:full["first"] + full["bw"] * full["bh"]].reshape(full["bh"], full["bw"], 64)
            got = coef[comp["first"]:comp["first"] + comp["bw"] * comp["bh"]].reshape(comp["bh"], comp["bw"], 64)
            assert np.array_equal(got, grid[comp["by0"]:comp["by0"] + comp["bh"], comp["bx0"]:comp["bx0"] + comp["bw"]])


def _restart_kw():
    """Pillow's restart-marker save option, or None where the installed Pillow has none."""
    import PIL

    if tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (10, 1):
        return None
    return {"restart_marker_blocks": 2}


def test_restart_intervals():
    kw = _restart_kw()
    if kw is None:
        pytest.skip("the installed Pillow has no restart-marker save option (restart_marker_blocks needs >= 10.1)")
    for sub in C.SUBSAMPLINGS:
        jpeg = C.encode(33, 31, False, "noise", sub, 75, **kw)
        assert b"\xff\xdd" in jpeg and b"\xff\xd0" in jpeg, "the encoder wrote no restart markers"
        slow = J.entropy_decode_python(jpeg)
        for _, win in C.windows(33, 31):
            _check_window(jpeg, win, slow)


def test_16bit_dqt_and_comment_segments():
    """A DQT rewritten with 16-bit entries, fill bytes in front of a marker and a long COM segment decode
    to the same record."""
    jpeg = C.encode(17, 9, False, "noise", "420", 75)
    base = C.decode_record(jpeg, (0, 0, 17, 9))
    out, pos = bytearray(jpeg[:2]), 2
    while True:
        m, ln = jpeg[pos + 1], (jpeg[pos + 2] << 8) | jpeg[pos + 3]
        seg = jpeg[pos + 4:pos + 2 + ln]
        if m == 0xDB:
            new, o = bytearray(), 0
            while o < len(seg):
                assert seg[o] >> 4 == 0
                new.append(0x10 | (seg[o] & 15))
                for v in seg[o + 1:o + 65]:
                    new += bytes([0, v])
                o += 65
            out += b"\xff\xff\xff\xdb" + (len(new) + 2).to_bytes(2, "big") + new  # with two fill bytes
        else:
            out += jpeg[pos:pos + 2 + ln]
        if m == 0xE0:
            out += b"\xff\xfe" + (60000 + 2).to_bytes(2, "big") + bytes(60000)
        pos += 2 + ln
        if m == 0xDA:
            break
    out += jpeg[pos:]
    rec = C.decode_record(bytes(out), (0, 0, 17, 9))
    assert not isinstance(rec, str), rec
    assert rec[0] == base[0] and np.array_equal(rec[1], base[1]) and np.array_equal(rec[2], base[2])


def _declined(res):
    return isinstance(res, str) and res.startswith("declined: ") and len(res) > len("declined: ")


def test_declines_by_kind():
    from PIL import Image

    rgb = C.pixels(24, 24, False, "noise")
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", progressive=True)
    assert "progressive" in C.decode_record(b.getvalue(), (0, 0, 24, 24))
    b = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(b, "JPEG")
    res = C.decode_record(b.getvalue(), (0, 0, 24, 24))
    assert _declined(res) and "CMYK" in res
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "PNG")
    res = C.decode_record(b.getvalue(), (0, 0, 24, 24))
    assert _declined(res) and "not a JPEG" in res
    jpeg = C.encode(24, 24, False, "noise", "420", 75)
    assert _declined(C.decode_record(jpeg, (0, 0, 25, 24)))  # window outside the image
    assert "capacity" in C.decode_record(jpeg, (0, 0, 24, 24), capacity=J.COEF_OFFSET + 128 * 5)
    assert _declined(C.decode_record(b"", (0, 0, 1, 1)))


def test_every_prefix_truncation_declines():
    jpeg = C.encode(17, 9, False, "noise", "420", 75)
    assert not isinstance(C.decode_record(jpeg, (0, 0, 17, 9)), str)
    for n in range(len(jpeg)):
        res = C.decode_record(jpeg[:n], (0, 0, 17, 9), capacity=1 << 14)
        assert _declined(res), f"prefix of {n} / {len(jpeg)} bytes: {res if isinstance(res, str) else 'decoded'}"


def test_single_byte_corruptions_never_raise():
    """400 seeded single-byte corruptions. A corrupted byte can leave a stream that is still a valid
    JPEG (a changed coefficient, a byte of an APP0 payload), which no decoder can tell from an intact
    one, so the outcome is either a decline with a reason or a record whose header is consistent with
    the capacity it was given; an exception, a crash or a write outside the buffer is never one."""
    jpeg = C.encode(17, 9, False, "noise", "420", 75)
    rng = np.random.default_rng(7)
    from azure_hc_intel_tf_amd.data.tfrecord import native

    cap = 1 << 14
    declined = 0
    for _ in range(400):
        bad = bytearray(jpeg)
        bad[int(rng.integers(2, len(jpeg)))] ^= int(rng.integers(1, 256))
        buf = np.full(cap + 64, 0xA5, dtype=np.uint8)
        res = native().jpeg_entropy_decode(bytes(bad), (0, 0, 0, 0), buf[:cap])
        assert (buf[cap:] == 0xA5).all()
        if isinstance(res, str):
            assert _declined(res)
            declined += 1
        else:
            hdr, qt, coef = J.parse_record(buf[:res])
            assert J.COEF_OFFSET + 128 * hdr["nblocks"] == res == hdr["nbytes"] <= cap
            J.jpeg_decode_reference(coef, hdr, qt, 1)  # and the record is decodable
    assert declined > 50  # most corruptions of so small a file hit a table or break the scan
