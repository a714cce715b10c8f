"""Device COCOeval entry points at the C-ABI boundary (no GPU needed): argument validation happens
before any HIP call, and the workspace size is defined for an empty evaluation."""
import ctypes

import torch  # noqa: F401  (torch's HIP runtime first, as the package does)

from mx_det import _lib


def _lib_handle():
    lib = _lib.load()
    for name in ("mx_coco_match", "mx_coco_accumulate", "mx_coco_accumulate_workspace"):
        assert hasattr(lib, name), name
    return lib


def test_match_rejects_negative_counts():
    lib = _lib_handle()
    none = [None] * 3
    # (ND, NG, S, A, T, max_g, max_d)
    for sizes in ((-1, 0, 0, 4, 10, 0, 0), (0, -1, 0, 4, 10, 0, 0), (0, 0, -1, 4, 10, 0, 0), (0, 0, 0, -1, 10, 0, 0),
                  (0, 0, 0, 4, -1, 0, 0), (0, 0, 0, 4, 10, -1, 0), (0, 0, 0, 4, 10, 0, -1)):
        nd, ng, s, a, t, mg, md = sizes
        rc = lib.mx_coco_match(*none, nd, None, None, None, None, None, ng, s, None, a, None, t, mg, md, None, None,
                               None, None)
        assert rc == -1, sizes
        assert b"mx_coco_match" in lib.mx_last_error() and b"bad sizes" in lib.mx_last_error()


def test_match_segment_bound_is_reported_not_truncated():
    lib = _lib_handle()
    big = 1 << 20  # GTs of one segment: above the kernel's per-segment limit
    rc = lib.mx_coco_match(None, None, None, 0, None, None, None, None, None, big, 1, None, 4, None, 10, big, 0, None,
                           None, None, None)
    assert rc == -2 and b"limit" in lib.mx_last_error()


def test_accumulate_rejects_negative_counts():
    lib = _lib_handle()
    # (S, ND, NG, K, A, T, M, R)
    for sizes in ((-1, 0, 0, 1, 4, 10, 3, 101), (0, -1, 0, 1, 4, 10, 3, 101), (0, 0, -1, 1, 4, 10, 3, 101),
                  (0, 0, 0, -1, 4, 10, 3, 101), (0, 0, 0, 1, -1, 10, 3, 101), (0, 0, 0, 1, 4, -1, 3, 101),
                  (0, 0, 0, 1, 4, 10, -1, 101), (0, 0, 0, 1, 4, 10, 3, -1)):
        s, nd, ng, k, a, t, m, r = sizes
        rc = lib.mx_coco_accumulate(None, None, None, None, None, None, s, nd, ng, None, None, k, a, t, None, m, None, r,
                                    None, None, None, None, 0, None)
        assert rc == -1, sizes
        assert b"mx_coco_accumulate" in lib.mx_last_error() and b"bad sizes" in lib.mx_last_error()


def test_accumulate_rejects_short_workspace_and_null_pointers():
    lib = _lib_handle()
    rc = lib.mx_coco_accumulate(None, None, None, None, None, None, 0, 1000, 0, None, None, 1, 4, 10, None, 3, None, 101,
                                None, None, None, None, 0, None)
    assert rc == -1 and b"workspace" in lib.mx_last_error()
    nws = lib.mx_coco_accumulate_workspace(0)
    rc = lib.mx_coco_accumulate(None, None, None, None, None, None, 0, 0, 0, None, None, 1, 4, 10, None, 3, None, 101,
                                None, None, None, None, nws, None)
    assert rc == -1 and b"null" in lib.mx_last_error()


def test_workspace_sizes():
    lib = _lib_handle()
    assert isinstance(lib.mx_coco_accumulate_workspace(0), int)
    assert 0 < lib.mx_coco_accumulate_workspace(0) <= 4096  # zero segments: a token allocation, not garbage
    n = 548 * 100 * 6
    assert 4 * n <= lib.mx_coco_accumulate_workspace(n) <= 4 * n + 4096  # one int32 rank per detection
    assert ctypes.sizeof(ctypes.c_size_t) == 8


def test_empty_evaluation_is_a_no_op_without_gpu():
    """Zero segments / zero categories: validated, then nothing is launched."""
    lib = _lib_handle()
    assert lib.mx_coco_match(None, None, None, 0, None, None, None, None, None, 0, 0, None, 4, None, 10, 0, 0, None,
                             None, None, None) == 0
    nws = lib.mx_coco_accumulate_workspace(0)
    assert lib.mx_coco_accumulate(None, None, None, None, None, None, 0, 0, 0, None, None, 0, 4, 10, None, 3, None, 101,
                                  None, None, None, None, nws, None) == 0
    assert lib.mx_version() == 1
