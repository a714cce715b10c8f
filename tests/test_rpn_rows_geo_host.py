"""Host geometry of the row-sparse RPN backward (csrc/mx_rpn_rows.h: list capacities, bitmap
workspace, the K-step list capacities of the tile-list wgrad) under AddressSanitizer and UBSan: the
stand-alone tools/rpn_rows_geo_check.cpp, compiled and run here. No GPU, nothing loaded into Python."""
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


def test_geometry_under_asan_ubsan(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rpn_rows_geo_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "robust-object-detection_amd", "csrc"),
                           os.path.join(ROOT, "tools", "rpn_rows_geo_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rpn_rows_geo_check ok" in out.stdout


def test_capacity_matches_library():
    """The exported mx_rpn_rows_capacity is the header's rule."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "robust-object-detection_amd"))
    from mx_det import _lib
    lib = _lib.load()
    assert [lib.mx_rpn_rows_capacity(134400, 512, l) for l in range(3)] == [512, 4608, 12800]
    assert [lib.mx_rpn_rows_capacity(70, 7, l) for l in range(3)] == [7, 63, 70]
    assert lib.mx_rpn_rows_capacity(70, 7, 3) == -1
    assert [lib.mx_rpn_tiles_capacity(134400, 512, l) for l in range(3)] == [512, 3072, 4200]
    assert [lib.mx_rpn_tiles_capacity(70, 7, l) for l in range(3)] == [3, 3, 3]
    assert lib.mx_rpn_rows_workspace(134400) == 2 * ((134400 // 64 * 8 + 255) // 256 * 256)
