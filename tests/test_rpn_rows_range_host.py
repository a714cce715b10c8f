"""Host geometry of the rows forms of the RPN head backward (csrc/mx_rpn_rows.h: the grid of a rows-form
dgrad from a list's capacity, the block ranges of the listed-rows activation pass by binary search)
under AddressSanitizer and UBSan: the stand-alone tools/rpn_rows_range_check.cpp, compiled and run
here. No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    return None


def test_range_geometry_under_asan_ubsan(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rpn_rows_range_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "robust-object-detection_amd", "csrc"),
                           os.path.join(ROOT, "tools", "rpn_rows_range_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rpn_rows_range_check ok" in out.stdout


def test_rows_dgrad_support_query_without_gpu():
    """mx_conv2d_dgrad_x3_rows_supported decides from the shape and cfg alone: the headline tower dgrads
    (automatic tile, no split) have a rows form; a split-K pick, a narrow output or a stride do not."""
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(ROOT, "robust-object-detection_amd"))
    from mx_det import _lib
    lib = _lib.load()

    def sup(N, H, W, C, K, R, stride=1, cfg=None):
        pad = (R - 1) // 2
        Ho = (H + 2 * pad - R) // stride + 1
        Wo = (W + 2 * pad - R) // stride + 1
        s = _lib.ConvShape(N, H, W, C, K, R, R, Ho, Wo, stride, stride, pad, pad)
        return lib.mx_conv2d_dgrad_x3_rows_supported(ctypes.byref(s), cfg)

    assert sup(2, 200, 336, 256, 256, 3) == 1 and sup(2, 151, 168, 256, 256, 3) == 1
    unsplit = _lib.ConvCfg(128, 128, 1, 0, 3, 0, 0)
    assert sup(2, 13, 21, 32, 32, 3, cfg=unsplit) == 1 and sup(2, 13, 21, 256, 256, 3, cfg=unsplit) == 1
    assert sup(2, 13, 21, 256, 256, 3) == 0            # the default of a small map splits K
    assert sup(2, 200, 336, 256, 16, 1) == 0           # the 1x1 head dgrad: K = 16 has no buffer kernel
    assert sup(2, 200, 336, 256, 256, 3, stride=2) == 0
    assert sup(2, 200, 336, 256, 256, 3, cfg=_lib.ConvCfg(0, 0, 0, 3, 3, 0, 0)) == 0  # another ring layout
