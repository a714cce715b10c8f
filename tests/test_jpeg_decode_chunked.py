"""The parallel JPEG entropy decoder on the host (no GPU needed): mx_jpeg_decode_coefs_chunked runs
the passes of mx_jpeg_entropy_decode serially over the walk both share (csrc/mx_jpeg_walk.h) and must
equal the sequential decoder mx_jpeg_decode_coefs, no tolerance, on the corpus of tests/jpeg_corpus.py
at the minimum and the default subsequence size; damaged streams set a status; the new entry points
validate their arguments before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (torch's HIP runtime first, as the package does)

import jpeg_corpus as jc

ST_CODE, ST_DC, ST_RUN, ST_SHORT, ST_RESTART = 1, 2, 4, 8, 16


def truncated(data):
    """Cut in the middle of the scan: no EOI, MCUs missing."""
    from mx_det import jpeg
    off = jpeg.parse(data).scan_off
    return data[:off + (len(data) - off) * 3 // 5]


def corrupted(data):
    """Sixteen scan bytes replaced by FF 00 pairs: 64 one-bits in a row, and no Huffman code is all ones."""
    from mx_det import jpeg
    off = jpeg.parse(data).scan_off
    mid = off + (len(data) - off) // 2
    return data[:mid] + b"\xff\x00" * 8 + data[mid + 16:]


def test_corpus_is_hard_enough():
    most_subseq, lane_straddles, chunk_straddles, shortest = jc.check_corpus()
    print("subsequences", most_subseq, "FF at a subsequence's end", lane_straddles, "FF 00 across a chunk",
          chunk_straddles, "shortest scan (bits)", shortest)


@pytest.mark.parametrize("subseq", [jc.SUBSEQ_MIN, jc.SUBSEQ_DEFAULT])
@pytest.mark.parametrize("i", range(len(jc.SPECS)), ids=jc.IDS)
def test_chunked_equals_sequential(i, subseq):
    from mx_det import jpeg
    info, ref = jc.reference(i)
    _, got, status = jpeg.decode_coefs_chunked(jc.jpeg_file(i), subseq)
    assert status == 0
    assert got.dtype == np.int16 and np.array_equal(got, ref)


def test_default_subsequence_size_is_the_setting():
    from mx_det import jpeg
    i = jc.IDS.index("noise-64x64-q100-444")
    _, ref = jc.reference(i)
    _, got, status = jpeg.decode_coefs_chunked(jc.jpeg_file(i))  # 0: the library setting
    assert status == 0 and np.array_equal(got, ref)


@pytest.mark.parametrize("subseq", [jc.SUBSEQ_MIN, jc.SUBSEQ_DEFAULT])
@pytest.mark.parametrize("name", ["noise-64x64-q100-444", "noise-250x131-q95-422-r7", "flat-64x64-q75-420"])
def test_truncated_file_sets_a_status(name, subseq):
    from mx_det import jpeg
    _, _, status = jpeg.decode_coefs_chunked(truncated(jc.jpeg_file(jc.IDS.index(name))), subseq)
    assert status & (ST_SHORT | ST_RESTART)


@pytest.mark.parametrize("subseq", [jc.SUBSEQ_MIN, jc.SUBSEQ_DEFAULT])
@pytest.mark.parametrize("name", ["noise-64x64-q100-444", "noise-64x64-q95-420-opt", "noise-64x64-q100-grey-r7"])
def test_corrupted_code_sets_a_status(name, subseq):
    from mx_det import jpeg
    data = corrupted(jc.jpeg_file(jc.IDS.index(name)))
    with pytest.raises(ValueError):
        jpeg.decode_coefs(data)
    _, _, status = jpeg.decode_coefs_chunked(data, subseq)
    assert status & ST_CODE


def test_missing_restart_marker_sets_a_status():
    from mx_det import jpeg
    data = jc.jpeg_file(jc.IDS.index("noise-64x64-q100-grey-r7"))
    off = jpeg.parse(data).scan_off
    at = data.index(b"\xff\xd3", off)
    _, _, status = jpeg.decode_coefs_chunked(data[:at] + data[at + 2:], jc.SUBSEQ_MIN)
    assert status & ST_RESTART


def test_setter_refuses_out_of_range_sizes():
    from mx_det import _lib, jpeg
    lib = _lib.load()
    try:
        for bad in (0, -64, jc.SUBSEQ_MIN - 1, 65537):
            assert lib.mx_jpeg_entropy_decode_set_subseq(bad) == -1
            assert b"mx_jpeg_entropy_decode_set_subseq" in lib.mx_last_error()
            with pytest.raises(ValueError):
                jpeg.set_subseq(bad)
        for ok in (jc.SUBSEQ_MIN, 65536, 1000):
            assert lib.mx_jpeg_entropy_decode_set_subseq(ok) == 0
        with pytest.raises(ValueError):
            jpeg.decode_coefs_chunked(jc.jpeg_file(0), 63)
    finally:
        assert lib.mx_jpeg_entropy_decode_set_subseq(jc.SUBSEQ_DEFAULT) == 0


def _aligned(nbytes, align=256):
    buf = np.zeros(nbytes + align, dtype=np.uint8)
    return buf, (buf.ctypes.data + align - 1) // align * align


def test_entry_points_validate_before_any_hip_call():
    """Host memory stands in for the device pointers: every call below returns before touching them."""
    from mx_det import _lib, jpeg
    lib = _lib.load()
    data = jc.jpeg_file(jc.IDS.index("noise-64x64-q95-420-opt"))
    info = jpeg.parse(data)
    n = len(data) - info.scan_off
    need = lib.mx_jpeg_entropy_decode_workspace(ctypes.byref(info), n)
    assert isinstance(need, int) and need > n and need % 256 == 0
    assert lib.mx_jpeg_entropy_decode_workspace(None, n) == 0
    assert lib.mx_jpeg_entropy_decode_workspace(ctypes.byref(info), 0) == 0
    keep, ws = _aligned(need)
    keep2, coefs = _aligned(info.coef_total * 2)
    keep3, scan = _aligned(n + 16)
    status = ctypes.c_int32(0)
    st = ctypes.addressof(status)

    def call(scan=scan + 1, n=n, info=info, ws=ws, ws_bytes=need, coefs=coefs, st=st):
        rc = lib.mx_jpeg_entropy_decode(scan, n, ctypes.byref(info) if info is not None else None, ws, ws_bytes, coefs,
                                        st, None)
        return rc, lib.mx_last_error()

    for kw in ({"scan": None}, {"info": None}, {"ws": None}, {"coefs": None}, {"st": None}):
        rc, msg = call(**kw)
        assert rc == -1 and b"null" in msg, kw
    for bad in (0, -5, 1 << 31):
        rc, msg = call(n=bad)
        assert rc == -1 and b"nbytes" in msg
    rc, msg = call(ws_bytes=need - 256)
    assert rc == -1 and b"workspace" in msg
    rc, msg = call(ws=ws + 64)
    assert rc == -1 and b"aligned" in msg
    rc, msg = call(coefs=coefs + 2)
    assert rc == -1 and b"aligned" in msg
    broken = jpeg.parse(data)
    broken.hbits[4 + broken.ta[0]][1] = 3  # three 1-bit codes
    rc, msg = call(info=broken)
    assert rc == -1 and b"Huffman" in msg
    geom = jpeg.parse(data)
    geom.coef_total += 64
    rc, msg = call(info=geom)
    assert rc == -1
    assert lib.mx_version() == 1
    del keep, keep2, keep3


def test_chunked_validates_its_arguments():
    from mx_det import _lib, jpeg
    lib = _lib.load()
    data = jc.jpeg_file(0)
    info = jpeg.parse(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(info.coef_total, dtype=np.int16)
    status = ctypes.c_int32(0)
    assert lib.mx_jpeg_decode_coefs_chunked(None, buf.size, ctypes.byref(info), 64, out.ctypes.data,
                                            ctypes.byref(status)) == -1
    assert lib.mx_jpeg_decode_coefs_chunked(buf.ctypes.data, buf.size, ctypes.byref(info), 64, out.ctypes.data, None) == -1
    assert lib.mx_jpeg_decode_coefs_chunked(buf.ctypes.data, info.scan_off, ctypes.byref(info), 64, out.ctypes.data,
                                            ctypes.byref(status)) == -1


def test_decode_refuses_an_unknown_entropy_mode():
    from mx_det import jpeg
    with pytest.raises(ValueError):
        jpeg.decode(jc.jpeg_file(0), "cpu", entropy="gpu")
