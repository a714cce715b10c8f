"""Which kernel every conv entry launches, as a recorded table: the return code and the eight
mx_conv_last_launch fields of each extern "C" conv entry, on zero-filled operands with MX_CONV_TUNE=0 and
the process defaults of test_gpu_conv_geometry's `fixed`, over the shapes of
test_conv_workspace_golden.py and four cfgs (NULL, 64x64 / 128x128 tiles unsplit, stages 3), compared for
equality with tests/golden/conv_launch_records.json.

The fixture is written by `python tests/test_gpu_conv_launch_golden.py --record` on an MI355X, on the
commit before the host launch layer of csrc/mx_conv.hip is changed; the kernels' values are pinned
elsewhere (test_gpu_conv_geometry.py), this file pins the dispatch. Every call is a valid launch (operands
and workspace of the sizes the entry documents; empty row / tile lists for the two rows entries) or is
refused by argument validation before any HIP call: a refused call is recorded as its return code alone
(the launch record is then an earlier call's).
"""
import ctypes
import functools
import json
import os

import pytest
import torch

from test_conv_cfg import _fd, _query
from test_conv_workspace_golden import SHAPES, _cfg_key, _shape_key
from test_gpu_conv_geometry import _shape, fixed, norm, out_hw  # noqa: F401 -- `fixed` is a fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_launch_records.json")
ENTRIES = ("mx_conv2d_fwd_ex", "mx_conv2d_dgrad_ex", "mx_conv2d_dgrad_bnb", "mx_conv2d_wgrad_ex", "mx_conv2d_fwd_x3",
           "mx_conv2d_dgrad_x3", "mx_conv2d_wgrad_x3", "mx_conv2d_wgrad_x3_rows", "mx_conv2d_dgrad_x3_rows")
DENSE_7X7 = (16, 7, 7, 256, 1024, 7, 1, 0)
assert DENSE_7X7 in SHAPES


def shapes_of(entry):
    return [c for c in SHAPES if not (entry.endswith("_rows") and c == DENSE_7X7)]


def cfgs():
    return [None, _fd((64, 64, 1, 0)), _fd((128, 128, 1, 0)), _fd((0, 0, 0, 3))]


@functools.lru_cache(maxsize=None)
def _zeros(c, dev):
    """Zero operands of a shape, one set for both number formats (an f32 buffer read as bf16 is zeros
    too): activations and gradients as f32, weights for two bf16 planes."""
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    z = functools.partial(torch.zeros, device=dev)
    return dict(x=z(N * H * W * C), y=z(N * Ho * Wo * K), w=z(2 * K * R * S * C, dtype=torch.bfloat16), dw=z(K * R * S * C),
                x2=z(N * H * W * C), x3=z(N * H * W * C), vec=z(C), part=z(2 * ((N * H * W + 63) // 64) * C),
                lst=torch.zeros(max(N * H * W, N * Ho * Wo), dtype=torch.int32, device=dev),
                cnt=torch.zeros(1, dtype=torch.int32, device=dev))


def run(entry, c, cfg, dev):
    """-> [rc] of a refused call, [rc, the eight launch-record fields] of a launched one."""
    from mx_det import _lib, conv as mc
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    t = _zeros(c, dev)
    p = lambda k: t[k].data_ptr()  # noqa: E731
    x3 = "_x3" in entry
    pass_ = 0 if "fwd" in entry else (1 if "dgrad" in entry else 2)
    n = 0 if entry == "mx_conv2d_dgrad_x3_rows" else _query(c, pass_, x3, cfg)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev) if n else None
    wsp = ws.data_ptr() if n else None
    s, st, mb = ctypes.byref(_shape(c)), mc._s(), (N * H * W + 63) // 64
    fn = getattr(_lib.load(), entry)
    if entry == "mx_conv2d_fwd_ex":
        rc = fn(s, p("x"), p("w"), None, None, 0, p("y"), 0, None, wsp, n, st, cfg)
    elif entry == "mx_conv2d_fwd_x3":
        rc = fn(s, p("x"), p("w"), None, None, 0, p("y"), None, wsp, n, st, cfg)
    elif entry == "mx_conv2d_dgrad_ex":
        rc = fn(s, p("y"), p("w"), None, p("x"), wsp, n, st, cfg)
    elif entry == "mx_conv2d_dgrad_bnb":
        rc = fn(s, p("y"), p("w"), None, p("x"), p("x2"), p("x3"), p("vec"), p("vec"), 1, p("part"), mb, wsp, n, st, cfg)
    elif entry == "mx_conv2d_dgrad_x3":
        rc = fn(s, p("y"), p("w"), None, p("x"), None, None, None, None, 0, None, 0, wsp, n, st, cfg)
    elif entry == "mx_conv2d_dgrad_x3_rows":
        rc = fn(s, p("y"), p("w"), None, p("x"), p("lst"), p("cnt"), N * H * W, st, cfg)
    elif entry == "mx_conv2d_wgrad_x3_rows":
        rc = fn(s, p("y"), p("x"), p("dw"), K, C, 1, p("lst"), p("cnt"), (N * Ho * Wo + 31) // 32, wsp, n, st, cfg)
    else:  # mx_conv2d_wgrad_ex, mx_conv2d_wgrad_x3
        rc = fn(s, p("y"), p("x"), p("dw"), K, C, 1, wsp, n, st, cfg)
    if rc:
        return [rc]
    out = (ctypes.c_int32 * 8)()
    _lib.call("mx_conv_last_launch", ctypes.cast(out, ctypes.c_void_p))
    return [rc] + list(out)


def records(entry, dev):
    out = {_shape_key(c): {_cfg_key(cfg): run(entry, c, cfg, dev) for cfg in cfgs()} for c in shapes_of(entry)}
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_launch_records_equal_the_recorded_ones(dev, fixed, entry):  # noqa: F811
    with open(GOLDEN) as f:
        want = json.load(f)[entry]
    assert any(len(r) == 9 for by_cfg in want.values() for r in by_cfg.values()), "the fixture holds no launch"
    got = records(entry, dev)
    assert sorted(got) == sorted(want), (entry, "shapes differ from the fixture's")
    for sk in got:
        assert sorted(got[sk]) == sorted(want[sk]), (entry, sk, "cfgs differ from the fixture's")
        for ck, r in got[sk].items():
            print(entry, sk, ck, r)
            assert r == want[sk][ck], (entry, sk, "cfg " + ck, r, want[sk][ck])


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_conv_launch_golden.py --record [path]")
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "robust-object-detection_amd")]
    os.environ["MX_CONV_TUNE"] = "0"
    from mx_det import _lib
    for name, args in (("mx_conv_set_variant", (7,)), ("mx_conv_set_loader", (1,)), ("mx_conv_set_wgrad_variant", (3,)),
                       ("mx_conv_set_wgrad_target", (0,)), ("mx_conv_set_tile", (0, 0)), ("mx_conv_set_max_splits", (0,)),
                       ("mx_conv_set_stages", (0,))):
        _lib.call(name, *args)
    device = torch.device("cuda:0")
    out = {e: records(e, device) for e in ENTRIES}
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", sum(len(v) for e in out for v in out[e].values()), "calls,",
          sum(len(r) == 9 for e in out for v in out[e].values() for r in v.values()), "of them launches")
