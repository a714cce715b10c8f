"""JPEG encoder, host half (mx_det.jpeg.encode_coefs / encode_info / header; include/mx_det.h
mx_jpeg_encode_coefs, mx_jpeg_encode_info, mx_jpeg_write_header) against libjpeg-turbo itself (PIL's
encoder): byte equality, no tolerance anywhere.
  * round trip: PIL file -> decode_coefs -> encode_coefs == the file, byte for byte (4:2:0 / 4:2:2 /
    4:4:4, qualities 50..100, odd sizes, 9x5 and 1x1);
  * mx_jpeg_encode_info == jpeg.parse of a PIL file of the same size and settings (tables, geometry),
    and its header == the PIL file's header;
  * error paths: bad quality / subsampling, a short output buffer (guard bytes untouched), restarts.
Every image of a byte comparison holds a pure-noise band (large coefficients, ZRL, long codes), a flat
band (EOB-only blocks) and a 0/255 checkerboard patch; images too small for three bands (under 24 rows
or columns) hold what fits. The reference scan of every full-size image must contain FF 00, so the
byte-stuffing path is exercised."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

ROUND_TRIP = [  # (H, W, quality, PIL subsampling)
    (121, 163, 95, 2),
    (97, 131, 75, 1),
    (64, 80, 90, 0),
    (75, 93, 100, 2),
    (50, 66, 50, 2),
    (9, 5, 95, 2),
    (1, 1, 95, 2),
]


def band_image(H, W, seed):
    """uint8 [H, W, 3]: top third pure noise, middle third flat, bottom third a smooth synthetic scene
    with a 0/255 checkerboard patch (period 1) in its left part."""
    from mx_det.data import synth_image
    g = np.random.default_rng(seed)
    img = synth_image(seed, max(H, 32), max(W, 32))[:H, :W].copy()
    a, b = H // 3, 2 * H // 3
    img[:a] = g.integers(0, 256, (a, W, 3), dtype=np.uint8)
    img[a:b] = np.array([200, 40, 90], dtype=np.uint8)
    yy, xx = np.mgrid[b:H, 0:max(W // 2, 1)]
    img[b:H, :max(W // 2, 1)] = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]
    return img


def full_size(H, W):
    return H >= 24 and W >= 24


def pil_bytes(img, q, sub):
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=q, subsampling=sub)
    return b.getvalue()


def scan_of(data, info):
    return data[info.scan_off:-2]


@pytest.mark.parametrize("case", ROUND_TRIP, ids=lambda c: "%dx%d-q%d-s%d" % c)
def test_round_trip_is_byte_identical(case):
    from mx_det import jpeg
    H, W, q, sub = case
    data = pil_bytes(band_image(H, W, H + W), q, sub)
    info, coefs = jpeg.decode_coefs(data)
    if full_size(H, W):
        assert b"\xff\x00" in scan_of(data, info)
    assert jpeg.header(info) == data[:info.scan_off]
    assert jpeg.encode_coefs(info, coefs) == data


@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("q", [50, 75, 90, 95, 100])
def test_encode_info_matches_a_parsed_pil_file(q, sub):
    from mx_det import jpeg
    H, W = 75, 93
    data = pil_bytes(band_image(H, W, 1), q, sub)
    ref = jpeg.parse(data)
    got = jpeg.encode_info(W, H, q, sub)
    for f in ("width", "height", "ncomp", "hmax", "vmax", "mcux", "mcuy", "coef_total", "restart_interval", "scan_off"):
        assert getattr(got, f) == getattr(ref, f), f
    for f in ("h", "v", "tq", "bw", "bh", "dw", "dh", "coef_off", "cid", "td", "ta", "hdef"):
        assert list(getattr(got, f)) == list(getattr(ref, f)), f
    for t in (0, 1):
        assert list(got.qt[t]) == list(ref.qt[t]), ("qt", t)
    for t in (0, 1, 4, 5):
        assert list(got.hbits[t]) == list(ref.hbits[t]) and list(got.hval[t]) == list(ref.hval[t]), ("huffman", t)
    assert jpeg.header(got) == data[:ref.scan_off]


def test_quality_below_50_and_table_clamps():
    """jpeg_quality_scaling's other branch (5000 / q) and the 1..255 clamp of the scaled tables."""
    from mx_det import jpeg
    for q in (1, 10, 49):
        data = pil_bytes(band_image(40, 40, 2), q, 2)
        ref, got = jpeg.parse(data), jpeg.encode_info(40, 40, q, 2)
        for t in (0, 1):
            assert list(got.qt[t]) == list(ref.qt[t]), (q, t)


def _lib():
    from mx_det import _lib
    return _lib.load()


def test_bad_quality_and_subsampling_are_einval():
    from mx_det import jpeg
    from mx_det._lib import JpegInfo
    lib, info = _lib(), JpegInfo()
    for q in (0, 101, -3):
        assert lib.mx_jpeg_encode_info(64, 64, q, 2, ctypes.byref(info)) == -1
        assert b"quality" in lib.mx_last_error()
    for s in (1, 3, -1):
        assert lib.mx_jpeg_encode_info(64, 64, 95, s, ctypes.byref(info)) == -1
        assert b"subsampling" in lib.mx_last_error()
    assert lib.mx_jpeg_encode_info(0, 64, 95, 2, ctypes.byref(info)) == -1
    assert lib.mx_jpeg_encode_info(65536, 8, 95, 2, ctypes.byref(info)) == -2
    assert lib.mx_jpeg_encode_info(20000, 20000, 95, 2, ctypes.byref(info)) == -2
    with pytest.raises(ValueError):
        jpeg.encode_info(64, 64, 0, 2)
    with pytest.raises(jpeg.JpegUnsupported):
        jpeg.encode_info(65536, 8)


def test_short_buffer_is_einval_and_nothing_is_written_past_cap():
    from mx_det import jpeg
    lib = _lib()
    data = pil_bytes(band_image(50, 66, 3), 95, 2)
    info, coefs = jpeg.decode_coefs(data)
    need = len(scan_of(data, info))
    assert 0 < need <= lib.mx_jpeg_scan_bound(ctypes.byref(info))
    n = ctypes.c_int64(0)
    for cap in (0, 1, need // 2, need - 1):
        buf = np.full(need + 64, 0xA5, dtype=np.uint8)
        rc = lib.mx_jpeg_encode_coefs(ctypes.byref(info), coefs.ctypes.data, buf.ctypes.data, cap, ctypes.byref(n))
        assert rc == -1 and b"bytes required" in lib.mx_last_error(), cap
        assert n.value == need
        assert (buf[cap:] == 0xA5).all(), cap
        assert bytes(buf[:cap]) == scan_of(data, info)[:cap]
    buf = np.full(need + 64, 0xA5, dtype=np.uint8)
    assert lib.mx_jpeg_encode_coefs(ctypes.byref(info), coefs.ctypes.data, buf.ctypes.data, need, ctypes.byref(n)) == 0
    assert n.value == need and bytes(buf[:need]) == scan_of(data, info) and (buf[need:] == 0xA5).all()
    head = np.full(1024, 0xA5, dtype=np.uint8)
    rc = lib.mx_jpeg_write_header(ctypes.byref(info), head.ctypes.data, 100, ctypes.byref(n))
    assert rc == -1 and n.value == info.scan_off and (head[100:] == 0xA5).all()


def test_restart_interval_is_unsupported_and_bad_coefficients_are_refused():
    from mx_det import jpeg
    lib = _lib()
    data = pil_bytes(band_image(50, 66, 4), 90, 2)
    info, coefs = jpeg.decode_coefs(data)
    buf = np.zeros(int(lib.mx_jpeg_scan_bound(ctypes.byref(info))), dtype=np.uint8)
    n = ctypes.c_int64(0)
    info.restart_interval = 4
    assert lib.mx_jpeg_encode_coefs(ctypes.byref(info), coefs.ctypes.data, buf.ctypes.data, buf.size, ctypes.byref(n)) == -2
    with pytest.raises(jpeg.JpegUnsupported):
        jpeg.encode_coefs(info, coefs)
    info.restart_interval = 0
    bad = coefs.copy()
    bad[5] = -32768  # 16 magnitude bits: no AC code
    with pytest.raises(ValueError):
        jpeg.encode_coefs(info, bad)
    with pytest.raises(ValueError):
        jpeg.encode_coefs(info, coefs[:100])
