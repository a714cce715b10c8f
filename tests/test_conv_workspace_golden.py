"""The conv workspace sizes as a recorded table: mx_conv_workspace and mx_conv_workspace_x3, all three
passes, every tuner candidate cfg of test_conv_cfg._all_cfgs() plus a NULL cfg, over SHAPES, compared
for equality with tests/golden/conv_workspace.json.

The queries are host code; without a device the library sizes for 256 CUs, which is also an MI355X's
count, so one table holds with and without a GPU. The fixture is written by
`python tests/test_conv_workspace_golden.py --record`, on the commit before the host launch layer of
csrc/mx_conv.hip is changed: a size that moves afterwards is a changed split or tile decision (or a
changed tuner candidate list, which is re-recorded on purpose).
"""
import json
import os

import pytest

from test_conv_cfg import QUERY_SHAPES, _all_cfgs, _query
from test_gpu_conv_geometry import fixed  # noqa: F401 -- fixture: every process default at the library's own

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_workspace.json")
# (N, H, W, C, K, k, stride, pad)
SHAPES = QUERY_SHAPES + [
    (8, 56, 56, 64, 256, 1, 1, 0),   # 392 tiles: the big-grid tile-candidate branch of the bf16 geometry
    (1, 1, 9, 64, 64, 3, 2, 1),      # stride 2 on a one-row map: empty dgrad parity classes must not count
    (1, 12, 12, 64, 20, 1, 1, 0),    # Ncol % 8 != 0: forward is never split
]
QUERIES = ("mx_conv_workspace", "mx_conv_workspace_x3")
_CFG_FIELDS = ("tile_rows", "tile_cols", "max_splits", "stages", "wgrad_variant", "reserved", "wgrad_target")


def _cfg_key(cfg):
    return "null" if cfg is None else ",".join(str(getattr(cfg, f)) for f in _CFG_FIELDS)


def _shape_key(c):
    return ",".join(str(v) for v in c)


def _cfgs():
    out = {}
    for cfg in [None] + _all_cfgs():
        out.setdefault(_cfg_key(cfg), cfg)  # the fwd/dgrad and wgrad lists share the all-default cfg
    return out


def table():
    """{query: {shape: {pass: {cfg: bytes}}}} of the loaded library under its default process settings."""
    cfgs = _cfgs()
    return {q: {_shape_key(c): {str(p): {k: _query(c, p, q.endswith("_x3"), cfg) for k, cfg in cfgs.items()}
                                for p in (0, 1, 2)} for c in SHAPES} for q in QUERIES}


def check_not_vacuous(t):
    for q in QUERIES:
        for p in ("0", "1", "2"):
            assert any(max(t[q][s][p].values()) > 0 for s in t[q]), (q, p, "no split workspace in this pass")
        assert any(len(set(t[q][s][p].values())) > 1 for s in t[q] for p in t[q][s]), (q, "no cfg moves a size")


def test_workspace_table_equals_the_recorded_one(fixed):  # noqa: F811
    with open(GOLDEN) as f:
        want = json.load(f)
    check_not_vacuous(want)
    got = table()
    for q in QUERIES:
        assert sorted(got[q]) == sorted(want[q]), (q, "shapes differ from the fixture's")
        for s in got[q]:
            for p in got[q][s]:
                assert sorted(got[q][s][p]) == sorted(want[q][s][p]), (q, s, p, "cfgs differ from the fixture's")
                for k, v in got[q][s][p].items():
                    assert v == want[q][s][p][k], (q, s, "pass " + p, "cfg " + k, v, want[q][s][p][k])


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_conv_workspace_golden.py --record [path]")
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "robust-object-detection_amd")]
    os.environ["MX_CONV_TUNE"] = "0"
    from mx_det import _lib
    for name, args in (("mx_conv_set_variant", (7,)), ("mx_conv_set_loader", (1,)), ("mx_conv_set_wgrad_variant", (3,)),
                       ("mx_conv_set_wgrad_target", (0,)), ("mx_conv_set_tile", (0, 0)), ("mx_conv_set_max_splits", (0,)),
                       ("mx_conv_set_stages", (0,))):
        _lib.call(name, *args)
    out = table()
    check_not_vacuous(out)
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", sum(len(out[q][s][p]) for q in out for s in out[q] for p in out[q][s]), "sizes")
