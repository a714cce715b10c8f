"""Everything about the BatchNorm kernel tests that needs no GPU: tests/bn_ref.py against torch float64
autograd, every predicate against deliberately wrong results built from the reference (the bounds are not
vacuous) and against the reference itself, the launch geometry read back from the library's workspace
functions against literal tables, and the argument rejections, which return before any HIP call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref as R  # noqa: E402


# ---- references against torch float64 autograd ----------------------------------------------------

@pytest.mark.parametrize("act", [0, 1, 2])
def test_reference_matches_torch_autograd(act):
    M, K = 200, 16
    d = R.data_operands(M, K, seed=3)
    p = R.channel_params(K, seed=3)
    x, dy = d["x"].double(), d["dy"].double()
    gamma, beta = torch.from_numpy(p["gamma"]).double(), torch.from_numpy(p["beta"]).double()
    rm0, rv0 = R.running_init(K, seed=3)
    # statistics through the partials path of the reference
    mb = (M + 127) // 128
    xp = F.pad(x, (0, 0, 0, mb * 128 - M)).view(mb, 128, K)
    stats = torch.stack([xp.sum(1), (xp * xp).sum(1)]).numpy()
    fin = R.finalize_ref(stats, M, p["gamma"], p["beta"], rm0, rv0)
    # torch
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.from_numpy(rm0).double(), torch.from_numpy(rv0).double()
    out = F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=R.MOM, eps=R.EPS)
    yr = F.relu(out) if act == 1 else F.leaky_relu(out, R.SLOPE) if act == 2 else out
    yr.backward(dy)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(torch.from_numpy(fin["running_mean"]), rm, **tol)
    torch.testing.assert_close(torch.from_numpy(fin["running_var"]), rv, **tol)
    torch.testing.assert_close(torch.from_numpy(fin["scale"] * x.numpy() + fin["shift"]), out.detach(), **tol)
    mean, invstd = fin["mean"], fin["invstd"]
    sums, _ = R.bwd_sums(dy, yr.detach(), x, mean, invstd, act)
    torch.testing.assert_close(sums[0], br.grad, **tol)
    torch.testing.assert_close(sums[1], gr.grad, **tol)
    coef, _, _ = R.bwd_coef(sums, M, mean, invstd, p["gamma"])
    g, _ = R.bwd_terms(dy, yr.detach(), x, mean, invstd, act)
    torch.testing.assert_close(R.bwd_dx(g, x, coef), xr.grad, **tol)


# ---- predicates: pass on the reference, raise on every mutant ----------------------------------------

def _bwd_case(M, K, act, seed=5):
    d, p = R.data_operands(M, K, seed), R.channel_params(K, seed)
    sums, mag = R.bwd_sums(d["dy"], d["y"], d["x"], p["mean"], p["invstd"], act)
    return d, p, sums, mag


def _check_sums(act, got, ref, mag, M):
    (R.check_sums_exact if act != 2 else R.check_sums_bounded)(got, ref, mag, M)


def _roll(a, n):
    return torch.roll(a, n, -1) if isinstance(a, torch.Tensor) else np.roll(a, n, -1)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,K", [(65, 72), (129, 136), (64, 136)])
def test_sums_predicates_reject_mutants(M, K, act):
    d, p, ref, mag = _bwd_case(M, K, act)
    dev = ref.float()                       # a correct device result: the reference cast to f32
    _check_sums(act, dev, ref, mag, M)
    mutants = {"roll 8": _roll(dev, 8), "roll 64": _roll(dev, 64)}
    mutants["last row dropped"] = R.bwd_sums(d["dy"][:-1], d["y"][:-1], d["x"][:-1], p["mean"], p["invstd"], act)[0].float()
    if act:
        mutants["mask y >= 0"] = R.bwd_sums(d["dy"], d["y"], d["x"], p["mean"], p["invstd"], act, strict=False)[0].float()
    if act == 2:
        mutants["slope 0.25"] = R.bwd_sums(d["dy"], d["y"], d["x"], p["mean"], p["invstd"], act, slope=0.25)[0].float()
    mean2, inv2 = p["mean"].copy(), p["invstd"].copy()
    n = min(64, K - 64)
    mean2[64:64 + n], inv2[64:64 + n] = p["mean"][:n], p["invstd"][:n]
    mutants["chunk 0 statistics in chunk 1"] = R.bwd_sums(d["dy"], d["y"], d["x"], mean2, inv2, act)[0].float()
    for name, m in mutants.items():
        assert not torch.equal(m, dev), name
        with pytest.raises(AssertionError):
            _check_sums(act, m, ref, mag, M)
            pytest.fail(f"mutant passed: {name}")


def test_sums_exact_premise_is_checked():
    d, p, ref, mag = _bwd_case(65, 72, 1)
    with pytest.raises(AssertionError, match="premise"):
        R.check_sums_exact(ref.float(), ref, mag * 4096, 65)
    with pytest.raises(AssertionError, match="premise"):
        R.check_sums_exact(ref.float(), ref, mag, 8194)


@pytest.mark.parametrize("M,K,act,gamma", [(64, 72, 1, True), (65, 72, 1, True), (129, 136, 2, True), (65, 136, 0, False),
                                           (1, 72, 2, True)])
def test_coef_predicate_rejects_mutants(M, K, act, gamma):
    d, p, ref, mag = _bwd_case(M, K, act)
    gm = p["gamma"] if gamma else None
    sums = ref.float()
    exact = act != 2 and R.is_pow2(M)
    coef = R.bwd_coef(sums, M, p["mean"], p["invstd"], gm)[0].float()
    R.check_coef(coef, sums, M, p["mean"], p["invstd"], gm, exact)
    up = lambda v, k: torch.where(v != 0, v * (1 + k * 2.0 ** -23), torch.full_like(v, 1e-6))
    mutants = {"roll 8": _roll(coef, 8), "roll 64": _roll(coef, 64),
               "mean over M + 1": R.bwd_coef(sums, M + 1, p["mean"], p["invstd"], gm)[0].float(),
               "b off by 16 ulp": torch.stack([coef[0], up(coef[1], 16), coef[2]]),
               "a off by 1 ulp": torch.stack([up(coef[0], 1), coef[1], coef[2]]),
               "c without the mean term": R.bwd_coef(sums, M, np.zeros_like(p["mean"]), p["invstd"], gm)[0].float()}
    if gamma:
        mutants["gamma ignored"] = R.bwd_coef(sums, M, p["mean"], p["invstd"], None)[0].float()
    if exact:
        mutants["b off by 1 ulp"] = torch.stack([coef[0], up(coef[1], 1), coef[2]])
    for name, m in mutants.items():
        with pytest.raises(AssertionError):
            R.check_coef(m, sums, M, p["mean"], p["invstd"], gm, exact)
            pytest.fail(f"mutant passed: {name}")


def _emulate_bwd_apply(d, coef, act, dtype, slope=R.SLOPE, strict=True):
    """The kernel's arithmetic with its f32 roundings: g = f32(dy * act'), dx = f32(f32(A*g + B*x) + C)."""
    c = torch.from_numpy(coef).double()
    g = (d["dy"].double() * R.act_grad(d["y"], act, slope, strict)).float().double()
    dx = ((c[0] * g + c[1] * d["x"].double()).float().double() + c[2]).float()
    return R.store_as(dx, dtype), R.store_as(g.float(), dtype)


@pytest.mark.parametrize("dtype", [R.F32, R.BF16])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,K", [(65, 72), (33, 136)])
def test_bwd_apply_predicate_rejects_mutants(M, K, act, dtype):
    d, coef = R.data_operands(M, K, 7), R.coef_params(K, 7)
    dx, dres = _emulate_bwd_apply(d, coef, act, dtype)
    args = (d["dy"], d["y"], d["x"], coef, act, dtype)
    R.check_bwd_apply(dx, dres, *args)
    R.check_bwd_apply(dx, None, *args)
    mutants = {"roll 8": _emulate_bwd_apply(d, np.roll(coef, 8, -1), act, dtype),
               "roll 64": _emulate_bwd_apply(d, np.roll(coef, 64, -1), act, dtype),
               "dres = dy": (dx, d["dy"] + (0 if act else 1))}
    if act:
        mutants["mask y >= 0"] = _emulate_bwd_apply(d, coef, act, dtype, strict=False)
    if act == 2:
        mutants["slope 0.25"] = _emulate_bwd_apply(d, coef, act, dtype, slope=0.25)
        if dtype == R.BF16:  # a bf16 store that truncates instead of rounding to nearest even
            g32 = (d["dy"].double() * R.act_grad(d["y"], 2)).float()
            trunc = (g32.view(torch.int32) & -65536).view(torch.float32)
            mutants["bf16 by truncation"] = (dx, trunc)
    for name, (mx, mr) in mutants.items():
        with pytest.raises(AssertionError):
            R.check_bwd_apply(mx, mr, *args)
            pytest.fail(f"mutant passed: {name}")


@pytest.mark.parametrize("xd,yd", [(R.BF16, R.BF16), (R.F32, R.BF16), (R.F32, R.F32)])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("res", [False, True])
def test_apply_predicate_rejects_mutants(xd, yd, act, res):
    M, K = 86, 136
    d, p = R.data_operands(M, K, 9), R.channel_params(K, 9)
    r = d["res"] if res else None
    dev = R.store_as(R.apply_ref(d["x"], p["scale"], p["shift"], r, act), yd)
    R.check_apply(dev, d["x"], p["scale"], p["shift"], r, act, yd)
    mk = lambda sc, sh, rr=r, a=act, **kw: R.store_as(R.apply_ref(d["x"], sc, sh, rr, a, **kw), yd)
    mutants = {"roll 8": mk(np.roll(p["scale"], 8), np.roll(p["shift"], 8)),
               "roll 64": mk(np.roll(p["scale"], 64), np.roll(p["shift"], 64)),
               "other activation": mk(p["scale"], p["shift"], a=(act + 1) % 3),
               "residual flipped": mk(p["scale"], p["shift"], rr=None if res else d["res"])}
    if act == 2:
        mutants["slope 0.25"] = mk(p["scale"], p["shift"], slope=0.25)
    for name, m in mutants.items():
        with pytest.raises(AssertionError):
            R.check_apply(m, d["x"], p["scale"], p["shift"], r, act, yd)
            pytest.fail(f"mutant passed: {name}")


def _fin_dev(ref, running):
    names = ["mean", "invstd", "scale", "shift"] + (["running_mean", "running_var"] if running else [])
    return {n: ref[n].astype(np.float32) for n in names}


@pytest.mark.parametrize("mb,K,count", [(2, 72, 256), (5, 136, 513), (1, 72, 1), (3, 136, 384)])
def test_finalize_predicate_rejects_mutants(mb, K, count):
    p = R.channel_params(K, 11)
    stats = R.finalize_operands(mb, K, count, 11)
    rm0, rv0 = R.running_init(K, 11)
    ref = R.finalize_ref(stats, count, p["gamma"], p["beta"], rm0, rv0)
    dev = _fin_dev(ref, True)
    args = (stats, count, p["gamma"], p["beta"], rm0, rv0)
    R.check_finalize(dev, *args)
    R.check_finalize(_fin_dev(R.finalize_ref(stats, count, None, None), False), stats, count, None, None)
    mutants = {}
    if count > 1:
        mutants["biased running_var"] = _fin_dev(R.finalize_ref(*args, unbiased=False), True)
    if mb > 1:
        mutants["last block dropped"] = _fin_dev(R.finalize_ref(stats[:, :-1], *args[1:]), True)
    for sh in (8, 64):
        mutants[f"roll {sh}"] = _fin_dev(R.finalize_ref(np.roll(stats, sh, -1), *args[1:]), True)
    s2 = stats.copy()
    n = min(64, K - 64)
    s2[:, :, 64:64 + n] = stats[:, :, :n]
    mutants["chunk 0 partials in chunk 1"] = _fin_dev(R.finalize_ref(s2, *args[1:]), True)
    mutants["momentum 0.2"] = _fin_dev(R.finalize_ref(*args, mom=0.2), True)
    mutants["eps 1e-3"] = _fin_dev(R.finalize_ref(*args, eps=1e-3), True)
    for n_ in ("mean", "invstd", "scale", "running_mean", "running_var"):
        m = dict(dev)
        m[n_] = dev[n_] + 2 * np.spacing(np.abs(dev[n_])) + np.float32(1e-30)
        mutants[f"{n_} off by 2 ulp"] = m
    m = dict(dev)
    m["shift"] = dev["shift"] + np.float32(32 * R.U) * (np.abs(p["beta"]) + np.abs(dev["mean"] * dev["scale"]) + 1)
    mutants["shift off by 32 u"] = m
    for name, m in mutants.items():
        with pytest.raises(AssertionError):
            R.check_finalize(m, *args)
            pytest.fail(f"mutant passed: {name}")


def test_partial_sums_predicate_rejects_mutants():
    part = np.random.default_rng(13).integers(-100, 101, (2, 5, 136)).astype(np.float32)
    dev = part.astype(np.float64).sum(1).astype(np.float32)
    R.check_partial_sums(dev, part)
    bump = dev.copy()
    bump[1, 135] += 1
    for m in (np.roll(dev, 8, -1), np.roll(dev, 64, -1), part[:, :-1].sum(1), dev[::-1].copy(), bump):
        with pytest.raises(AssertionError):
            R.check_partial_sums(m, part)
    with pytest.raises(AssertionError, match="premise"):
        R.check_partial_sums(dev, part + 0.5)


def test_canary_predicate():
    full = torch.full((5, 16), float("nan"))
    full[1:-1] = 1.0
    for dt in (torch.float32, torch.bfloat16):
        R.check_canaries(full.to(dt))
    left = full.clone()
    left[3, 15] = float("nan")               # one output element left at its canary value
    over = full.clone()
    over[4, 0] = 0.0                          # a store past the end
    under = full.clone()
    under[0, 15] = 2.0
    for m in (left, over, under):
        with pytest.raises(AssertionError):
            R.check_canaries(m)


def test_operands_are_exact_in_bf16_and_cover_the_edges():
    d, p = R.data_operands(129, 136, 1), R.channel_params(136, 1)
    for v in d.values():
        assert torch.equal(v.bfloat16().float(), v)
    for v in list(p.values()) + [R.coef_params(136, 1)]:
        t = torch.from_numpy(v)
        assert torch.equal(t.bfloat16().float(), t)
    assert bool((d["y"] == 0).any()) and bool((d["y"] > 0).any()) and bool((d["y"] < 0).any())
    for name in ("mean", "invstd", "gamma", "scale"):  # not periodic in 8 or in 64
        assert not np.array_equal(np.roll(p[name], 8), p[name]) and not np.array_equal(np.roll(p[name], 64), p[name])
    st = R.finalize_operands(3, 72, 257, 1)
    assert st.shape == (2, 3, 72) and st[0, 2, 71] == 3 and st[1, 2, 71] == 9


# ---- launch geometry, read back from the library ------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from mx_det import _lib
    return _lib.load()


RB_SMALL_K = {1: 1, 31: 1, 32: 1, 33: 1, 63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 3, 257: 5, 960: 15, 1024: 16,
              1088: 17, 2100: 33, 8128: 127, 8191: 128, 8192: 128, 8193: 127}
RB_WIDE = {(8193, 1024): 64, (2100, 2048): 32, (8193, 2048): 32, (1088, 4096): 16, (8193, 4096): 16}
RS_TABLE = {1: 1, 2: 1, 4: 1, 5: 1, 9: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3, 97: 4, 256: 8, 257: 9, 2047: 64,
            2048: 64, 2049: 64}
ACT_RB = {1: 1, 65: 2, 129: 3, 8193: 127}


def _rb(lib, M, K):
    ws = lib.mx_bn_bwd_workspace(M, K)
    assert (ws - 256) % (8 * K) == 0
    return (ws - 256) // (8 * K)


def test_bwd_reduce_geometry_table(lib):
    """Row blocks of mx_bn_bwd_reduce_ex. A retune that moves a threshold fails here, with the shapes of
    tests/test_gpu_bn_channels.py to revisit, instead of silently dropping their coverage."""
    for K in (8, 56, 64, 72, 136):
        got = {M: _rb(lib, M, K) for M in RB_SMALL_K}
        assert got == RB_SMALL_K, (K, {M: (got[M], RB_SMALL_K[M]) for M in got if got[M] != RB_SMALL_K[M]})
    got = {mk: _rb(lib, *mk) for mk in RB_WIDE}
    assert got == RB_WIDE
    # rows per block = cdiv(M, RB): 65 rows and a 3-row last block; 2, 3 and 5 passes of the 128-row loop
    cdiv = lambda a, b: -(-a // b)
    assert cdiv(8193, 127) == 65 and 8193 - 126 * 65 == 3
    assert [cdiv(8193, RB_WIDE[(8193, K)]) for K in (1024, 2048, 4096)] == [129, 257, 513]


def test_finalize_geometry_table(lib):
    for K in (8, 72, 4096):
        got = {}
        for mb in RS_TABLE:
            ws = lib.mx_bn_finalize_workspace(mb, K)
            assert (ws - 256) % (16 * K) == 0
            got[mb] = (ws - 256) // (16 * K)
        assert got == RS_TABLE, (K, got)
    # 2049 blocks in 64 slices of 33: 62 full slices, a 3-block slice and one empty slice
    assert -(-2049 // 64) == 33 and 2049 - 62 * 33 == 3


def test_act_bias_geometry_table(lib):
    for K in (3, 15, 35, 64, 72):
        got = {}
        for M in ACT_RB:
            ws = lib.mx_act_bias_bwd_workspace(M, K)
            assert (ws - 256) % (4 * K) == 0
            got[M] = (ws - 256) // (4 * K)
        assert got == ACT_RB, (K, got)


# ---- rejections: before any HIP call --------------------------------------------------------------------
# Every call passes NULL data pointers and no workspace, and the streaming entries M = 0, so that a call
# whose check had gone would still return without launching anything.

def _rejected(lib, name, args, msg):
    rc = getattr(lib, name)(*args)
    err = lib.mx_last_error().decode()
    assert rc == -1 and msg in err, (name, args, rc, err)


N = None


@pytest.mark.parametrize("M,K,act,msg", [(64, 12, 0, "positive multiple of 8"), (64, 0, 0, "positive multiple of 8"),
                                         (0, 8, 0, "M > 0"), (64, 8, 3, "act 0/1/2"), (64, 8, -1, "act 0/1/2"),
                                         (64, 8, 1, "y required"), (64, 8, 2, "y required"),
                                         (64, 4104, 0, "bn_bwd_reduce: K > 4096")])
def test_bwd_reduce_rejections(lib, M, K, act, msg):
    for dt in (R.F32, R.BF16):
        _rejected(lib, "mx_bn_bwd_reduce_ex", (N, N, N, dt, M, K, act, N, N, N, N, 0, N, N, N), msg)


def test_bwd_reduce_rejects_a_missing_workspace(lib):
    _rejected(lib, "mx_bn_bwd_reduce_ex", (N, N, N, R.BF16, 64, 8, 0, N, N, N, N, 0, N, N, N), "workspace of 320 bytes")


@pytest.mark.parametrize("K,act,msg", [(12, 0, "positive multiple of 8"), (0, 0, "positive multiple of 8"),
                                       (8, 3, "act 0/1/2"), (8, 1, "y required"), (8, 2, "y required")])
def test_bwd_apply_rejections(lib, K, act, msg):
    _rejected(lib, "mx_bn_bwd_apply_ex", (N, N, N, R.BF16, 0, K, act, N, N, N, N), msg)


def test_apply_rejections(lib):
    _rejected(lib, "mx_bn_apply", (N, R.F32, 0, 12, N, N, N, 0, N, R.F32, N), "K % 8")
    _rejected(lib, "mx_bn_apply", (N, R.BF16, 0, 8, N, N, N, 0, N, R.F32, N), "bf16 input with f32 output")
    _rejected(lib, "mx_bn_apply", (N, 2, 0, 8, N, N, N, 0, N, R.F32, N), "bad dtype")


def test_finalize_rejections(lib):
    fin = lambda K, rm, rv: (N, 1, K, 128, N, N, 1e-5, 0.1, rm, rv, N, N, N, N, N, 0, N)
    _rejected(lib, "mx_bn_finalize_ex", fin(4104, N, N), "bn_finalize: K > 4096")
    _rejected(lib, "mx_bn_finalize_ex", fin(8, N, N), "workspace of 384 bytes")
    _rejected(lib, "mx_bn_finalize_ex", (N, 0, 8, 128, N, N, 1e-5, 0.1, N, N, N, N, N, N, N, 0, N), "bad sizes")
    _rejected(lib, "mx_bn_bwd_finalize", (N, 1, 4104, 64, N, N, N, N, N, N, 0, N), "bn_bwd_finalize: K > 4096")
    _rejected(lib, "mx_bn_bwd_finalize", (N, 1, 8, 0, N, N, N, N, N, N, 0, N), "bad sizes")
    # only one of running_mean / running_var: the one pointer is a real host buffer of K floats (never
    # dereferenced), and K = 4104 so that the next check would reject the call as well
    buf = (ctypes.c_float * 4104)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    _rejected(lib, "mx_bn_finalize_ex", fin(4104, p, N), "both be given or both null")
    _rejected(lib, "mx_bn_finalize_ex", fin(4104, N, p), "both be given or both null")
