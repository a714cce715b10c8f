"""Per-call conv launch settings (mx_conv_cfg): a cfg replaces the six values the tuner varies for
one call -- the workspace query and the launch that consumes the workspace get the same object --
and never reads or writes the process defaults behind mx_conv_set_*.

The host tests need no GPU (the workspace queries are host code; without a device they size for 256
CUs). The GPU tests call the C entries directly on the integer operands of
test_gpu_conv_geometry.py, so every comparison is an equality and the launch record
(mx_conv_last_launch) says which settings a launch really ran under.
"""
import ctypes
import threading

import pytest
import torch

from test_gpu_conv_geometry import _ops, _shape, _tup, on_device

# (N, H, W, C, K, k, stride, pad)
QUERY_SHAPES = [
    (1, 14, 14, 256, 256, 3, 1, 1),   # small grid: split-K on every pass
    (1, 14, 14, 256, 256, 3, 2, 1),   # its stride-2 form (four dgrad parity classes)
    (16, 7, 7, 256, 1024, 7, 1, 0),   # dense 7x7 on a 7x7 map (FC6 as a conv; wgrad as a 1x1 over R*S*C)
    (2, 20, 20, 64, 16, 1, 1, 0),     # narrow K = 16 1x1
]
GPU_CASE = (1, 16, 16, 32, 128, 3, 1, 1)


def _lib():
    from mx_det import _lib as lib
    return lib


def _fd(c):
    return _lib().ConvCfg(c[0], c[1], c[2], c[3], 3, 0, 0)


def _wg(c):
    return _lib().ConvCfg(0, 0, 0, 0, c[0], 0, c[1])


def _install(cfg):
    """The same six values through the process-wide setters."""
    lib = _lib()
    lib.call("mx_conv_set_tile", cfg.tile_rows, cfg.tile_cols)
    lib.call("mx_conv_set_max_splits", cfg.max_splits)
    lib.call("mx_conv_set_stages", cfg.stages)
    lib.call("mx_conv_set_wgrad_variant", cfg.wgrad_variant)
    lib.call("mx_conv_set_wgrad_target", cfg.wgrad_target)


def _query(c, pass_, x3, cfg):
    fn = _lib().load().mx_conv_workspace_x3 if x3 else _lib().load().mx_conv_workspace
    return fn(ctypes.byref(_shape(c)), pass_, cfg)


@pytest.fixture
def knobs(monkeypatch):
    """No per-shape tuner; the process defaults at the library's own values before and after."""
    monkeypatch.setenv("MX_CONV_TUNE", "0")
    default = _lib().ConvCfg(0, 0, 0, 0, 3, 0, 0)
    _install(default)
    try:
        yield
    finally:
        _install(default)


def _all_cfgs():
    from mx_det import conv as mc
    out = [_fd(c) for c in mc._FD_CANDS + mc._FD_CANDS_X3] + [_wg(c) for c in mc._WG_CANDS + mc._WG_CANDS_X3]
    # what the tuner hands the library for a candidate is exactly that struct
    for c in mc._FD_CANDS + mc._FD_CANDS_X3:
        assert bytes(mc._fd_cfg(c)) == bytes(_fd(c)), c
    for c in mc._WG_CANDS + mc._WG_CANDS_X3:
        assert bytes(mc._wg_cfg(c)) == bytes(_wg(c)), c
    assert mc._fd_cfg(None) is None and mc._wg_cfg(None) is None
    return out


def test_cfg_layout():
    """mx_conv_cfg: six int32 then one int64, 32 bytes."""
    C = _lib().ConvCfg
    assert ctypes.sizeof(C) == 32 and C.wgrad_target.offset == 24 and C.reserved.offset == 20
    assert [n for n, _ in C._fields_] == ["tile_rows", "tile_cols", "max_splits", "stages", "wgrad_variant",
                                          "reserved", "wgrad_target"]


def test_binding_takes_an_omitted_cfg_as_null(knobs):
    """From Python the trailing cfg may be left out (mx_det._lib): the same answer as an explicit NULL,
    here under a non-default process setting."""
    lib = _lib().load()
    _lib().call("mx_conv_set_max_splits", 2)
    for c in QUERY_SHAPES:
        s = _shape(c)
        for fn in (lib.mx_conv_workspace, lib.mx_conv_workspace_x3):
            for pass_ in (0, 1, 2):
                assert fn(ctypes.byref(s), pass_) == fn(ctypes.byref(s), pass_, None), (c, pass_)
    with pytest.raises(TypeError):
        lib.mx_conv_workspace(ctypes.byref(_shape(QUERY_SHAPES[0])))


def test_query_with_cfg_equals_setters_then_null(knobs):
    """Every tuner candidate, every pass, both query functions, four shapes: the size under a cfg is the
    size under the same values installed process-wide and a NULL cfg."""
    cfgs = _all_cfgs()
    sizes = {}
    for c in QUERY_SHAPES:
        for x3 in (False, True):
            for pass_ in (0, 1, 2):
                for i, cfg in enumerate(cfgs):
                    got = _query(c, pass_, x3, cfg)
                    _install(cfg)
                    want = _query(c, pass_, x3, None)
                    assert got == want, (c, x3, pass_, bytes(cfg).hex(), got, want)
                    sizes[(c, x3, pass_, i)] = got
    for pass_ in (0, 1, 2):  # not vacuous: every pass has split workspaces, and the settings move them
        per_query = [{v for (c, x, p, _), v in sizes.items() if (c, x, p) == (s, x3, pass_)}
                     for s in QUERY_SHAPES for x3 in (False, True)]
        assert any(max(v) > 0 for v in per_query), pass_
        assert any(len(v) > 1 for v in per_query), (pass_, per_query)


def test_cfg_query_leaves_no_state(knobs):
    """After a query under a cfg that changes the size, a NULL query returns the default size again and
    the process-wide variants are what they were."""
    lib = _lib().load()
    v0, w0 = lib.mx_conv_get_variant(), lib.mx_conv_get_wgrad_variant()
    small, narrow = QUERY_SHAPES[0], QUERY_SHAPES[3]  # 196 pixels are too few for a wgrad pixel split; 800 split
    for x3 in (False, True):
        for c, pass_, cfg in ((small, 0, _fd((0, 0, 1, 0))), (small, 1, _fd((128, 128, 1, 0))),
                              (narrow, 2, _wg((0, 2)))):
            d0 = _query(c, pass_, x3, None)
            assert d0 > 0 and _query(c, pass_, x3, cfg) != d0, (x3, pass_)
            assert _query(c, pass_, x3, None) == d0, (x3, pass_)
            assert (lib.mx_conv_get_variant(), lib.mx_conv_get_wgrad_variant()) == (v0, w0)


BAD = [("tile_rows", dict(tile_rows=96, tile_cols=128)), ("max_splits", dict(max_splits=17)),
       ("stages", dict(stages=2)), ("wgrad_variant", dict(wgrad_variant=6)), ("reserved", dict(reserved=1))]


@pytest.mark.parametrize("field,kw", BAD, ids=[b[0] for b in BAD])
def test_bad_cfg_is_rejected_before_any_device_call(knobs, field, kw):
    """MX_EINVAL with a message naming the field from the launch entries (null tensors: nothing is
    touched), 0 from the workspace queries."""
    L = _lib()
    lib = L.load()
    vals = dict(tile_rows=0, tile_cols=0, max_splits=0, stages=0, wgrad_variant=3, reserved=0, wgrad_target=0)
    vals.update(kw)
    cfg = L.ConvCfg(**vals)
    c = QUERY_SHAPES[0]
    s = _shape(c)
    rc = lib.mx_conv2d_fwd_ex(ctypes.byref(s), None, None, None, None, 0, None, 0, None, None, 0, None, cfg)
    assert rc == -1 and field.encode() in lib.mx_last_error(), (rc, lib.mx_last_error())
    rc = lib.mx_conv2d_wgrad_ex(ctypes.byref(s), None, None, None, c[4], c[3], 1, None, 0, None, cfg)
    assert rc == -1 and field.encode() in lib.mx_last_error(), (rc, lib.mx_last_error())
    for x3 in (False, True):
        for q, pass_ in ((c, 0), (c, 1), (QUERY_SHAPES[3], 2)):  # queries whose NULL answer is a split workspace
            assert _query(q, pass_, x3, None) > 0 and _query(q, pass_, x3, cfg) == 0, (x3, pass_)


# ---- GPU ------------------------------------------------------------------------------------------
def _ws(c, pass_, x3, cfg, dev):
    n = _query(c, pass_, x3, cfg)
    return (torch.empty(n, dtype=torch.uint8, device=dev) if n else None), n


def _fwd(c, dev, x3, cfg):
    """The fwd entry under `cfg` (workspace sized with the same object) -> (y f32, launch record)."""
    from mx_det import conv as mc
    d, dt, wk, _ = _ops(c, dev, x3)
    x = d["x"].to(dt)
    y = torch.full(d["z"].shape, float("nan"), device=dev)
    ws, n = _ws(c, 0, x3, cfg, dev)
    p, s = mc._p, _shape(c)
    if x3:
        _lib().call("mx_conv2d_fwd_x3", ctypes.byref(s), p(x), p(wk), None, None, 0, p(y), None, p(ws), n, mc._s(), cfg)
    else:
        _lib().call("mx_conv2d_fwd_ex", ctypes.byref(s), p(x), p(wk), None, None, 0, p(y), 0, None, p(ws), n, mc._s(),
                    cfg)
    return y, mc.last_launch()


def _dgrad(c, dev, x3, cfg):
    from mx_det import conv as mc
    d, dt, _, wt = _ops(c, dev, x3)
    dy = d["dy"].to(dt)
    dx = torch.full(d["dx"].shape, float("nan"), dtype=dt, device=dev)
    ws, n = _ws(c, 1, x3, cfg, dev)
    p, s = mc._p, _shape(c)
    if x3:
        _lib().call("mx_conv2d_dgrad_x3", ctypes.byref(s), p(dy), p(wt), None, p(dx), None, None, None, None, 0, None,
                    0, p(ws), n, mc._s(), cfg)
    else:
        _lib().call("mx_conv2d_dgrad_ex", ctypes.byref(s), p(dy), p(wt), None, p(dx), p(ws), n, mc._s(), cfg)
    return dx, mc.last_launch()


def _wgrad(c, dev, x3, cfg, no_ws=False):
    from mx_det import conv as mc
    d = on_device(c, dev)
    dt = torch.float32 if x3 else torch.bfloat16
    dy, x = d["dy"].to(dt), d["x"].to(dt)
    dw = torch.full(d["dw"].shape, float("nan"), device=dev)
    ws, n = (None, 0) if no_ws else _ws(c, 2, x3, cfg, dev)
    _lib().call("mx_conv2d_wgrad_x3" if x3 else "mx_conv2d_wgrad_ex", ctypes.byref(_shape(c)), mc._p(dy), mc._p(x),
                mc._p(dw), c[4], c[3], 1, mc._p(ws), n, mc._s(), cfg)
    return dw, mc.last_launch()


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
def test_cfg_beats_the_default_and_does_not_stick(dev, knobs, x3):
    """Process default tile 64x64, cfg tile 128x128: the cfg'd launch runs 128x128, the next NULL launch
    64x64 again, both exact; the same for dgrad, and for wgrad with wgrad_variant 0 against the default 3.
    (The bf16x3 wgrad has one 128x128 kernel for variants 0..3 -- kind 103 either way -- so there the
    128x256 block, variant 4 -> kind 104, shows the cfg as well.)"""
    c = GPU_CASE
    d = on_device(c, dev)
    dt = torch.float32 if x3 else torch.bfloat16
    _lib().call("mx_conv_set_tile", 64, 64)
    big = _fd((128, 128, 0, 0))
    for fn, want, pass_ in ((_fwd, d["z"], 0), (_dgrad, d["dx"].to(dt), 1)):
        out, rec = fn(c, dev, x3, big)
        assert (rec["pass_"], rec["bmt"], rec["bn"]) == (pass_, 128, 128), rec
        assert torch.equal(out, want), (fn.__name__, "cfg")
        out, rec = fn(c, dev, x3, None)
        assert (rec["pass_"], rec["bmt"], rec["bn"]) == (pass_, 64, 64), rec
        assert torch.equal(out, want), (fn.__name__, "NULL")
    dw, rec = _wgrad(c, dev, x3, _wg((0, 0)))
    assert (rec["pass_"], rec["kind"]) == (2, 103 if x3 else 0), rec
    assert torch.equal(dw, d["dw"])
    if x3:
        dw, rec = _wgrad(c, dev, x3, _wg((4, 0)))
        assert (rec["kind"], rec["bmt"], rec["bn"]) == (104, 128, 256), rec
        assert torch.equal(dw, d["dw"])
    dw, rec = _wgrad(c, dev, x3, None)
    assert (rec["pass_"], rec["kind"]) == (2, 103 if x3 else 3), rec
    assert torch.equal(dw, d["dw"])
    assert _lib().load().mx_conv_get_wgrad_variant() == 3


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
def test_failed_call_leaves_nothing_behind(dev, knobs, x3):
    """A wgrad whose cfg needs a split workspace, given none: rejected by argument validation (nothing
    launches); the next NULL launch runs the default geometry and is exact."""
    c = GPU_CASE
    d = on_device(c, dev)
    dw, before = _wgrad(c, dev, x3, None)
    assert torch.equal(dw, d["dw"])
    cfg = _wg((4, 1024) if x3 else (0, 1024))
    assert _query(c, 2, x3, cfg) > 0
    with pytest.raises(_lib().MxError, match="split workspace"):
        _wgrad(c, dev, x3, cfg, no_ws=True)
    dw, after = _wgrad(c, dev, x3, None)
    assert _tup(after) == _tup(before) and after["kind"] == (103 if x3 else 3), (before, after)
    assert torch.equal(dw, d["dw"])


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
def test_two_threads_with_different_cfgs(dev, knobs, x3):
    """Two threads, each on its own stream, 100 fwd launches each under its own cfg: every launch's
    thread-local record shows the thread's own tile, and both outputs are exact."""
    from mx_det import conv as mc
    c = GPU_CASE
    d, dt, wk, _ = _ops(c, dev, x3)
    x = d["x"].to(dt)
    torch.cuda.synchronize()
    errors = []

    def worker(name, cfg, tile):
        try:
            st = mc.dedicated_stream(dev, name)
            with torch.cuda.stream(st):
                y = torch.full(d["z"].shape, float("nan"), device=dev)
                ws, n = _ws(c, 0, x3, cfg, dev)
                p, s = mc._p, _shape(c)
                for i in range(100):
                    if x3:
                        _lib().call("mx_conv2d_fwd_x3", ctypes.byref(s), p(x), p(wk), None, None, 0, p(y), None, p(ws),
                                    n, mc._s(), cfg)
                    else:
                        _lib().call("mx_conv2d_fwd_ex", ctypes.byref(s), p(x), p(wk), None, None, 0, p(y), 0, None,
                                    p(ws), n, mc._s(), cfg)
                    rec = mc.last_launch()
                    assert (rec["bmt"], rec["bn"]) == tile, (name, i, rec)
                st.synchronize()
                assert torch.equal(y, d["z"]), name
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((name, e))

    ts = [threading.Thread(target=worker, args=("cfg_test_a", _fd((64, 64, 0, 0)), (64, 64))),
          threading.Thread(target=worker, args=("cfg_test_b", _fd((128, 128, 1, 0)), (128, 128)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
