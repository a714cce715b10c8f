"""The BatchNorm kernels of csrc/mx_bn.hip per channel and per element against the float64 references of
tests/bn_ref.py, at the edges of their launch geometry (tests/test_bn_ref_host.py pins the geometry tables
these shapes were chosen from). Integer operands: the sums of act 0 / 1 must be exact, everything else is
held to the rounding-count bounds written next to the predicates in bn_ref.py.

Every output lies between two NaN canary rows and is NaN-filled before the launch: every element must be
written and no canary touched. Every reduction runs twice on one fresh zero-filled workspace: the results are
bitwise equal and the arrival counters are zero afterwards. Only accepted argument combinations are ever
launched: K a positive multiple of 8, at most 4096."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {R.F32: torch.float32, R.BF16: torch.bfloat16}
MS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 960, 1024, 1088, 8128, 8192, 8193]
KS = [8, 56, 64, 72, 136]
# every M and every K at least twice
EDGES = sorted({(M, KS[(i + j) % 5]) for i, M in enumerate(MS) for j in (0, 2)})
WIDE = [(8193, 1024), (2100, 2048), (8193, 2048), (1088, 4096), (8193, 4096)]
ACT2 = [(M, K) for M in (1, 33, 65, 129, 257) for K in (8, 72, 136)] + [(8193, 72)]
FIN = [(mb, K) for mb in (1, 4, 5, 9, 33, 65, 97, 257, 2049) for K in (8, 72, 4096) if (mb, K) != (2049, 4096)]


def _call(name, *a):
    from mx_det import _lib
    return _lib.call(name, *a)


def _s():
    from mx_det import _lib
    return _lib.stream()


def _p(t):
    return None if t is None else t.data_ptr()


def _guarded(rows, K, dtype, dev):
    """(the whole NaN-filled allocation with its canary rows, the [rows][K] output inside it)."""
    assert K % 8 == 0
    full = torch.full((rows + 2, K), float("nan"), dtype=dtype, device=dev)
    return full, full[1:-1]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ws(nbytes, dev):
    assert nbytes >= 256
    return torch.zeros(nbytes, dtype=torch.uint8, device=dev)


def _f32(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _report(name, ratio):
    print(f"RATIO {name} {ratio:.4f}")


def _assert_legal(M, K):
    assert M > 0 and K > 0 and K % 8 == 0 and K <= 4096


# ---- mx_bn_bwd_reduce_ex ----------------------------------------------------------------------------

def _reduce(dev, d, p, M, K, act, dt, gamma=True):
    from mx_det import _lib
    _assert_legal(M, K)
    dy, y, x = (d[n].to(TD[dt]) for n in ("dy", "y", "x"))
    mean, invstd = _f32(p["mean"], dev), _f32(p["invstd"], dev)
    gm = _f32(p["gamma"], dev) if gamma else None
    wsb = _lib.load().mx_bn_bwd_workspace(M, K)
    ws = _ws(wsb, dev)
    runs = []
    for _ in range(2):
        sf, s = _guarded(2, K, torch.float32, dev)
        cf, c = _guarded(3, K, torch.float32, dev)
        _call("mx_bn_bwd_reduce_ex", _p(dy), _p(y) if act else None, _p(x), dt, M, K, act, _p(mean), _p(invstd),
              _p(gm), _p(ws), wsb, _p(s), _p(c), _s())
        runs.append((sf, cf, s, c))
    torch.cuda.synchronize()
    for sf, cf, _, _ in runs:
        R.check_canaries(sf, "sums")
        R.check_canaries(cf, "coef")
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "second launch on the workspace differs"
    assert int(ws[:256].sum()) == 0, "arrival counters not left zero"
    return runs[0][2], runs[0][3]


def _check_reduce(dev, M, K, acts, seed=21, gamma=True):
    d, p = R.data_operands(M, K, seed, dev), R.channel_params(K, seed)
    for act in acts:
        ref, mag = R.bwd_sums(d["dy"], d["y"], d["x"], p["mean"], p["invstd"], act)
        for dt in (R.BF16, R.F32):
            sums, coef = _reduce(dev, d, p, M, K, act, dt, gamma)
            tag = f"M={M} K={K} act={act} dtype={dt}"
            try:
                if act == 2:
                    _report(f"sums_bounded {tag}", R.check_sums_bounded(sums, ref, mag, M))
                else:
                    R.check_sums_exact(sums, ref, mag, M)
                _report(f"coef {tag}", R.check_coef(coef, sums, M, p["mean"], p["invstd"], p["gamma"] if gamma else None,
                                                    exact=act != 2 and R.is_pow2(M)))
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None


@pytest.mark.parametrize("M,K", EDGES + WIDE)
def test_bwd_reduce_exact_sums(dev, M, K):
    _check_reduce(dev, M, K, (0, 1))


@pytest.mark.parametrize("M,K", ACT2)
def test_bwd_reduce_leaky_bounded_sums(dev, M, K):
    _check_reduce(dev, M, K, (2,))


def test_bwd_reduce_without_gamma(dev):
    _check_reduce(dev, 129, 72, (1,), gamma=False)


# ---- mx_bn_bwd_apply_ex -----------------------------------------------------------------------------

def _apply_ex(dev, d, coef, M, K, act, dt, with_dres=True):
    _assert_legal(M, K)
    dy, y, x = (d[n].to(TD[dt]) for n in ("dy", "y", "x"))
    cf = _f32(coef, dev)
    xf, dx = _guarded(M, K, TD[dt], dev)
    rf, dres = _guarded(M, K, TD[dt], dev) if with_dres else (None, None)
    _call("mx_bn_bwd_apply_ex", _p(dy), _p(y) if act else None, _p(x), dt, M, K, act, _p(cf), _p(dx), _p(dres), _s())
    torch.cuda.synchronize()
    R.check_canaries(xf, "dx")
    if with_dres:
        R.check_canaries(rf, "dres")
    return dx, dres


@pytest.mark.parametrize("M,K", EDGES + WIDE)
def test_bwd_apply(dev, M, K):
    d, coef = R.data_operands(M, K, 22, dev), R.coef_params(K, 22)
    for act in (0, 1, 2):
        for dt in (R.BF16, R.F32):
            dx, dres = _apply_ex(dev, d, coef, M, K, act, dt)
            tag = f"M={M} K={K} act={act} dtype={dt}"
            try:
                ratio = R.check_bwd_apply(dx, dres, d["dy"], d["y"], d["x"], coef, act, dt)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
            if act == 2:
                _report(f"bwd_apply {tag}", ratio)


@pytest.mark.parametrize("act,dt", [(1, R.BF16), (2, R.F32)])
def test_bwd_apply_without_dres(dev, act, dt):
    M, K = 129, 72
    d, coef = R.data_operands(M, K, 23, dev), R.coef_params(K, 23)
    dx, _ = _apply_ex(dev, d, coef, M, K, act, dt, with_dres=False)
    R.check_bwd_apply(dx, None, d["dy"], d["y"], d["x"], coef, act, dt)
    dx2, _ = _apply_ex(dev, d, coef, M, K, act, dt)
    assert _same(dx, dx2)


# ---- mx_bn_bwd_finalize -----------------------------------------------------------------------------

@pytest.mark.parametrize("mb,K", FIN)
def test_bwd_finalize_from_partials(dev, mb, K):
    from mx_det import _lib
    _assert_legal(mb, K)
    rng = np.random.default_rng([31, mb, K])
    part = rng.integers(-100, 101, (2, mb, K)).astype(np.float32)
    p = R.channel_params(K, 31)
    partd, mean, invstd, gm = (_f32(a, dev) for a in (part, p["mean"], p["invstd"], p["gamma"]))
    wsb = _lib.load().mx_bn_finalize_workspace(mb, K)
    for M in sorted({mb * 64, mb * 64 - 63}):
        ws = _ws(wsb, dev)
        runs = []
        for _ in range(2):
            sf, s = _guarded(2, K, torch.float32, dev)
            cf, c = _guarded(3, K, torch.float32, dev)
            _call("mx_bn_bwd_finalize", _p(partd), mb, K, M, _p(mean), _p(invstd), _p(gm), _p(s), _p(c), _p(ws), wsb, _s())
            runs.append((sf, cf, s, c))
        torch.cuda.synchronize()
        for sf, cf, _, _ in runs:
            R.check_canaries(sf, "sums")
            R.check_canaries(cf, "coef")
        assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
        assert int(ws[:256].sum()) == 0
        R.check_partial_sums(runs[0][2], part)
        _report(f"bwd_finalize coef mb={mb} K={K} M={M}",
                R.check_coef(runs[0][3], runs[0][2], M, p["mean"], p["invstd"], p["gamma"], exact=R.is_pow2(M)))


# ---- mx_bn_finalize_ex / mx_bn_finalize ----------------------------------------------------------------

FIN_OUT = ("mean", "invstd", "scale", "shift")


def _finalize(dev, entry, stats, mb, K, count, gm, bt, rm0, rv0, ws=None):
    """One launch; the running stats are updated in place, so every launch gets its own copy inside its
    own canary rows. Returns (dict of [K] device tensors, the allocations to check)."""
    _assert_legal(mb, K)
    outs, fulls = {}, []
    for n in FIN_OUT + (("running_mean", "running_var") if rm0 is not None else ()):
        f, o = _guarded(1, K, torch.float32, dev)
        if n.startswith("running"):
            o.copy_(rm0 if n == "running_mean" else rv0)
        outs[n] = o[0]
        fulls.append((n, f))
    args = [_p(stats), mb, K, count, _p(gm), _p(bt), R.EPS, R.MOM, _p(outs.get("running_mean")),
            _p(outs.get("running_var"))] + [_p(outs[n]) for n in FIN_OUT]
    if entry == "mx_bn_finalize_ex":
        args += [_p(ws), ws.numel()]
    _call(entry, *args, _s())
    return outs, fulls


def _check_finalize_case(dev, mb, K, count, running, affine=True, seed=41):
    from mx_det import _lib
    p = R.channel_params(K, seed)
    stats = R.finalize_operands(mb, K, count, seed)
    rm0, rv0 = R.running_init(K, seed) if running else (None, None)
    gamma, beta = (p["gamma"], p["beta"]) if affine else (None, None)
    statsd, gm, bt, rmd, rvd = (_f32(a, dev) for a in (stats, gamma, beta, rm0, rv0))
    ws = _ws(_lib.load().mx_bn_finalize_workspace(mb, K), dev)
    runs = [_finalize(dev, "mx_bn_finalize_ex", statsd, mb, K, count, gm, bt, rmd, rvd, ws) for _ in range(2)]
    runs.append(_finalize(dev, "mx_bn_finalize", statsd, mb, K, count, gm, bt, rmd, rvd))
    torch.cuda.synchronize()
    assert int(ws[:256].sum()) == 0, "arrival counters not left zero"
    for outs, fulls in runs:
        for n, f in fulls:
            R.check_canaries(f, n)
        for n in outs:
            assert _same(outs[n], runs[0][0][n]), f"{n}: launches / entry points differ"
    got = {n: v.cpu().numpy() for n, v in runs[0][0].items()}
    tag = f"mb={mb} K={K} count={count} running={running} affine={affine}"
    try:
        _report(f"finalize shift {tag}", R.check_finalize(got, stats, count, gamma, beta, rm0, rv0))
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from None


@pytest.mark.parametrize("mb,K", FIN)
def test_finalize(dev, mb, K):
    pow2 = 1 << ((mb * 128).bit_length() - 1)
    for i, count in enumerate(sorted({mb * 128, mb * 128 - 127, pow2})):
        _check_finalize_case(dev, mb, K, count, running=True)
        if i == 0:
            _check_finalize_case(dev, mb, K, count, running=False)


def test_finalize_without_affine(dev):
    _check_finalize_case(dev, 5, 72, 513, running=True, affine=False)


# ---- mx_bn_apply --------------------------------------------------------------------------------------

APPLY_SHAPES = [(1, 8), (7, 24), (85, 24), (86, 24), (256, 264), (2049, 264), (2049, 2048), (4097, 2056), (524289, 8)]


@pytest.mark.parametrize("xd,yd", [(R.BF16, R.BF16), (R.F32, R.BF16), (R.F32, R.F32)])
@pytest.mark.parametrize("M,K", APPLY_SHAPES)
def test_apply(dev, M, K, xd, yd):
    _assert_legal(M, K)
    d, p = R.data_operands(M, K, 51, dev), R.channel_params(K, 51)
    x, res = d["x"].to(TD[xd]), d["res"].to(TD[yd])
    scale, shift = _f32(p["scale"], dev), _f32(p["shift"], dev)
    for act in (0, 1, 2):
        for r in (None, res):
            full, y = _guarded(M, K, TD[yd], dev)
            _call("mx_bn_apply", _p(x), xd, M, K, _p(scale), _p(shift), _p(r), act, _p(y), yd, _s())
            torch.cuda.synchronize()
            try:
                R.check_canaries(full, "y")
                R.check_apply(y, d["x"], p["scale"], p["shift"], None if r is None else d["res"], act, yd)
            except AssertionError as e:
                raise AssertionError(f"M={M} K={K} act={act} residual={r is not None}: {e}") from None


# ---- mx_act_bias_bwd ----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [3, 15, 35, 64, 72])
@pytest.mark.parametrize("M", [1, 65, 129, 8193])
def test_act_bias_bwd(dev, M, K):
    from mx_det import _lib
    K8 = (K + 7) // 8 * 8
    assert K8 <= 4096
    d = R.data_operands(M, K, 61, dev)
    wsb = _lib.load().mx_act_bias_bwd_workspace(M, K)
    for act in (0, 1, 2):
        g64 = d["dy"].double() * R.act_grad(d["y"], act)
        for dt, gdt in ((R.BF16, R.BF16), (R.F32, R.BF16), (R.F32, R.F32)):
            gy, y = d["dy"].to(TD[dt]).contiguous(), d["y"].to(TD[dt]).contiguous()
            ws = _ws(wsb, dev)
            runs = []
            for with_db in (True, True, False):
                gf, g = _guarded(M, K8, TD[gdt], dev)
                bf, db = _guarded(1, K8, torch.float32, dev)  # db [K] in a K8-wide row: its tail must stay NaN
                _call("mx_act_bias_bwd", _p(gy), _p(y) if act else None, dt, M, K, K8, act, _p(g), gdt,
                      _p(db) if with_db else None, _p(ws) if with_db else None, wsb if with_db else 0, _s())
                runs.append((gf, g, bf, db))
            torch.cuda.synchronize()
            tag = f"M={M} K={K} act={act} dtype={dt}->{gdt}"
            try:
                assert int(ws[:256].sum()) == 0, "arrival counters not left zero"
                gref = R.store_as(g64.float(), gdt).double()
                for i, (gf, g, bf, db) in enumerate(runs):
                    R.check_canaries(gf, "g")
                    R._raise("g", g[:, :K].double() != gref, g[:, :K].double(), gref)
                    assert int((g[:, K:] != 0).sum()) == 0, "padding columns not zero"
                    assert _same(g, runs[0][1]), "g differs between launches (db given / null)"
                    assert bool(torch.isnan(bf[0]).all() and torch.isnan(bf[2]).all() and torch.isnan(db[0, K:]).all())
                    if i == 2:
                        assert bool(torch.isnan(db).all()), "db written though null was passed"
                        continue
                    assert not bool(torch.isnan(db[0, :K]).any()), "db element not written"
                    assert _same(db, runs[0][3])
                    if act == 2:
                        R.check_sums_bounded(db[:, :K], g64.sum(0, keepdim=True), g64.abs().sum(0, keepdim=True), M)
                    else:
                        R.check_partial_sums(db[:, :K], g64[None], distinct=M > 1)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None


# ---- legacy mx_bn_bwd_reduce / mx_bn_bwd_apply ---------------------------------------------------------

@pytest.mark.parametrize("M", [64, 1024])
def test_legacy_entries_equal_the_hot_path(dev, M):
    """M a power of two: the legacy form's f32 sums * (1 / M) is exact, so its dx equals the hot path's."""
    K, act, dt = 72, 1, R.BF16
    d, p = R.data_operands(M, K, 71, dev), R.channel_params(K, 71)
    sums, coef = _reduce(dev, d, p, M, K, act, dt)
    dy, y, x = (d[n].to(TD[dt]) for n in ("dy", "y", "x"))
    mean, invstd, gm = (_f32(p[n], dev) for n in ("mean", "invstd", "gamma"))
    sf, s2 = _guarded(2, K, torch.float32, dev)
    _call("mx_bn_bwd_reduce", _p(dy), _p(y), _p(x), M, K, act, _p(mean), _p(invstd), _p(s2), _s())
    xf, dx2 = _guarded(M, K, TD[dt], dev)
    rf, dres2 = _guarded(M, K, TD[dt], dev)
    _call("mx_bn_bwd_apply", _p(dy), _p(y), _p(x), M, K, act, _p(mean), _p(invstd), _p(gm), _p(s2), _p(dx2), _p(dres2),
          _s())
    torch.cuda.synchronize()
    for f in (sf, xf, rf):
        R.check_canaries(f)
    assert _same(s2, sums)
    dx, dres = _apply_ex(dev, d, coef.cpu().numpy(), M, K, act, dt)
    assert _same(dx2, dx) and _same(dres2, dres)
