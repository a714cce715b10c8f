"""float64 restatement of the train-mode BatchNorm kernels (csrc/mx_bn.hip), written from the formulas in that
file's header and in include/mx_det.h (a helper, not a test): seeded small-alphabet operands, the references,
and the assertion predicates of tests/test_bn_ref_host.py (CPU, mutants) and tests/test_gpu_bn_channels.py.

Operands are exact in bf16 and in f32, so the column sums of act 0 / 1 are exact in f32 under any summation
order and any FMA contraction; everything else is held to a bound counted in roundings, u = 2^-24. Every
check is per channel or per element, never a norm. Arguments may be numpy arrays or torch tensors (torch
for bf16); a predicate computes on the device of the result it is given and raises AssertionError."""
import numpy as np
import torch

U = 2.0 ** -24
SLOPE = float(np.float32(0.2))   # leaky-relu slope as the kernels hold it
MOM = float(np.float32(0.1))
EPS = float(np.float32(1e-5))
F32, BF16 = 0, 1                 # MX_F32 / MX_BF16
MAX_EXACT_ROWS = 8193


def t64(a, device=None):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.detach()
    return a.to(device=device if device is not None else a.device, dtype=torch.float64)


def _dev(a):
    return a.device if isinstance(a, torch.Tensor) else torch.device("cpu")


def is_pow2(n):
    return n > 0 and (n & (n - 1)) == 0


# ---- operands -------------------------------------------------------------------------------------

def channel_params(K, seed):
    """Per-channel parameters, a seeded non-periodic function of k (float32 numpy arrays)."""
    rng = np.random.default_rng([seed, K, 77])
    pick = lambda vals: np.asarray(vals, np.float32)[rng.integers(0, len(vals), K)]
    return dict(mean=pick([-1, 0, 1]), invstd=pick([0.5, 1, 2]), gamma=pick([0.5, 1, 2]),
                beta=rng.integers(-3, 4, K).astype(np.float32), scale=pick([0.25, 0.5, 1, 2]),
                shift=rng.integers(-3, 4, K).astype(np.float32))


def coef_params(K, seed):
    """Backward-apply coefficients chosen by the test: A, B, C [3][K] float32."""
    rng = np.random.default_rng([seed, K, 78])
    A = np.asarray([0.5, 1, 2], np.float32)[rng.integers(0, 3, K)]
    B = np.asarray([-0.25, 0, 0.5], np.float32)[rng.integers(0, 3, K)]
    C = (rng.integers(-6, 7, K) * 0.5).astype(np.float32)
    return np.stack([A, B, C])


def data_operands(M, K, seed, device="cpu"):
    """x in -4..4, dy and res in -2..2, y in {-1, 0, 1}: float32 [M][K] tensors on `device`. Row 0 holds
    y == 0 under a non-zero dy in every even channel, so a mask y >= 0 moves those column sums."""
    g = torch.Generator(device=device).manual_seed(seed * 1000003 + M * 4099 + K)
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (M, K), generator=g, device=device, dtype=torch.int32).float()
    x, dy, res, y = ri(-4, 4), ri(-2, 2), ri(-2, 2), ri(-1, 1)
    y[0, ::2] = 0
    dy[0, ::2] = 1 + (torch.arange(0, K, 2, device=device) // 2 % 2).float()
    return dict(x=x, dy=dy, y=y, res=res)


def finalize_operands(mb, K, count, seed):
    """Integer-valued conv-epilogue partials stats [2][mb][K] (float32 numpy) of `count` rows in 128-row
    blocks: block sums of z and z^2 with |mean| <= 4 and variance >= 5 per channel, the columns told apart
    by a per-channel offset; the last channel is the constant 3 (variance exactly 0)."""
    assert 0 < count <= mb * 128
    rng = np.random.default_rng([seed, mb, K, count])
    nb = np.clip(count - 128 * np.arange(mb), 0, 128).astype(np.int64)[:, None]
    s = rng.integers(-nb, nb + 1, (mb, K))
    q = 6 * nb + rng.integers(0, nb + 1, (mb, K))
    q += (q - s) & 1                                   # sum z^2 and sum z have one parity
    o = rng.integers(-3, 4, K)[None, :]                # z + o: mean moves, variance stays
    q = q + 2 * o * s + o * o * nb
    s = s + o * nb
    s[:, K - 1], q[:, K - 1] = 3 * nb[:, 0], 9 * nb[:, 0]
    return np.stack([s, q]).astype(np.float32)


def running_init(K, seed):
    rng = np.random.default_rng([seed, K, 79])
    return rng.integers(-3, 4, K).astype(np.float32), np.asarray([0.5, 1, 2], np.float32)[rng.integers(0, 3, K)]


# ---- references (float64) -------------------------------------------------------------------------

def act_grad(y, act, slope=SLOPE, strict=True):
    y = t64(y)
    if act == 0:
        return torch.ones_like(y)
    pos = (y > 0) if strict else (y >= 0)
    return torch.where(pos, torch.ones_like(y), torch.full_like(y, 0.0 if act == 1 else slope))


def bwd_terms(dy, y, x, mean, invstd, act, slope=SLOPE, strict=True):
    """g = dy * act'(y) and g * xhat, xhat = (x - mean) * invstd, [M][K] float64."""
    d = _dev(dy)
    g = t64(dy) * act_grad(y if act else dy, act, slope, strict)
    return g, g * ((t64(x) - t64(mean, d)) * t64(invstd, d))


def bwd_sums(dy, y, x, mean, invstd, act, **kw):
    """(sums [2][K] = (sum g, sum g*xhat), the column sums of |g| and |g*xhat|)."""
    g, gx = bwd_terms(dy, y, x, mean, invstd, act, **kw)
    return torch.stack([g.sum(0), gx.sum(0)]), torch.stack([g.abs().sum(0), gx.abs().sum(0)])


def bwd_coef(sums, M, mean, invstd, gamma):
    """coef [3][K] of dx = a*g + b*x + c, and (mg, t = mean*invstd*mgx) for the bound on c."""
    sums = t64(sums)
    d = sums.device
    mean, invstd = t64(mean, d), t64(invstd, d)
    a = invstd if gamma is None else t64(gamma, d) * invstd
    mg, mgx = sums[0] / M, sums[1] / M
    t = mean * invstd * mgx
    return torch.stack([a, -a * invstd * mgx, -a * (mg - t)]), mg, t


def bwd_dx(g, x, coef):
    coef = t64(coef, _dev(g))
    return coef[0] * g + coef[1] * t64(x) + coef[2]


def finalize_ref(stats, count, gamma, beta, rm=None, rv=None, eps=EPS, mom=MOM, unbiased=True):
    """numpy float64: mean, var (biased), invstd, scale, shift, running_mean, running_var. A single row
    (count == 1) has no unbiased variance; the kernel then keeps the biased one, and so does this."""
    st = np.asarray(stats, np.float64)
    s, q = st[0].sum(0), st[1].sum(0)
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    K = mean.shape[0]
    g = np.ones(K) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(K) if beta is None else np.asarray(beta, np.float64)
    out = dict(mean=mean, var=var, invstd=invstd, scale=g * invstd, shift=b - mean * g * invstd)
    if rm is not None:
        unb = var * count / (count - 1) if (unbiased and count > 1) else var
        out["running_mean"] = (1.0 - mom) * np.asarray(rm, np.float64) + mom * mean
        out["running_var"] = (1.0 - mom) * np.asarray(rv, np.float64) + mom * unb
    return out


def apply_ref(x, scale, shift, res, act, slope=SLOPE):
    """act(x*scale + shift (+ res)) as the float32 value the kernel holds before it stores: the
    pre-activation is exact on these operands, leaky relu is one rounding of slope * z."""
    d = _dev(x)
    z = t64(x) * t64(scale, d) + t64(shift, d)
    if res is not None:
        z = z + t64(res)
    assert bool((z.float().double() == z).all()), "premise: exact pre-activation"
    if act == 1:
        z = torch.where(z > 0, z, 0.0)
    elif act == 2:
        z = torch.where(z > 0, z, slope * z)
    return z.float()


def store_as(v32, dtype):
    """The stored value of a float32 result: itself, or its round-to-nearest-even bf16."""
    return v32.to(torch.bfloat16).float() if dtype == BF16 else v32


# ---- predicates -----------------------------------------------------------------------------------

def _raise(name, bad, *cols):
    bad = bad.reshape(-1) if isinstance(bad, torch.Tensor) else torch.from_numpy(np.asarray(bad)).reshape(-1)
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad)[0])
        vals = ", ".join(f"{float((c if isinstance(c, torch.Tensor) else torch.as_tensor(c)).reshape(-1)[i]):.9g}"
                         for c in cols)
        raise AssertionError(f"{name}: {n} of {bad.numel()} wrong, first at flat index {i}: ({vals})")


def check_canaries(full, name="output"):
    """full [rows + 2][K], allocated NaN-filled with one canary row before and after the output: both
    canary rows are still NaN and every element between them was written."""
    full = full if isinstance(full, torch.Tensor) else torch.from_numpy(np.asarray(full))
    f = full.float()
    _raise(f"{name}: canary row overwritten", ~torch.isnan(torch.stack([f[0], f[-1]])))
    _raise(f"{name}: element not written", torch.isnan(f[1:-1]))


def check_distinct(ref, K):
    """Premise: moving the channels by 8 or by 64 changes the reference."""
    ref = t64(ref)
    for sh in (8, 64):
        if K > sh:
            assert not torch.equal(torch.roll(ref, sh, -1), ref), f"premise: columns distinct under a shift of {sh}"


def check_sums_exact(got, ref, mag, M):
    """act 0 / 1. g is an integer, g*xhat a multiple of 0.5; with M <= 8193 the column sums of the
    magnitudes stay below 2^18, so every partial sum, in any order, is exact in f32: equality."""
    got = t64(got)
    ref, mag = t64(ref, got.device), t64(mag, got.device)
    assert M <= MAX_EXACT_ROWS and float(mag.max()) < 2.0 ** 18, "premise: sums below 2^18"
    assert bool(((2 * ref) == torch.round(2 * ref)).all()), "premise: half-integer sums"
    check_distinct(ref, ref.shape[-1])
    _raise("sums (exact)", got != ref, got, ref)


def check_partial_sums(got, part, distinct=True):
    """Column sums [W][K] of integer-valued partials part [W][mb][K] (mx_bn_bwd_finalize, the db of
    mx_act_bias_bwd on integer operands): below 2^24 every order is exact, equality. distinct=False drops
    the premise that the columns differ (a single row of a relu gradient may be all zero)."""
    got = t64(got)
    part = t64(part, got.device)
    ref, mag = part.sum(1), part.abs().sum(1)
    assert bool((part == torch.round(part)).all()) and float(mag.max()) < 2.0 ** 24, "premise: integer partials"
    if distinct:
        check_distinct(ref, ref.shape[-1])
    _raise("sums of partials (exact)", got != ref, got, ref)


def check_sums_bounded(got, ref, mag, M):
    """act 2 (dy * 0.2f is inexact): |got - ref| <= (M + 2) u sum|t| + u |ref|, the order-independent
    forward bound of a sum of M f32 terms, one rounding per product and the final cast. Returns the largest
    |error| / bound."""
    got = t64(got)
    ref, mag = t64(ref, got.device), t64(mag, got.device)
    check_distinct(ref, ref.shape[-1])
    err, bound = (got - ref).abs(), (M + 2) * U * mag + U * ref.abs()
    _raise("sums (bounded)", ~(err <= bound), got, ref, bound)
    return float((err / bound.clamp_min(1e-300)).max())


def check_coef(coef, sums, M, mean, invstd, gamma, exact):
    """coef against the f64 formulas evaluated at the device's own sums. coef[0] = gamma*invstd is a product
    of powers of two: equal. b and c each see at most 4 f32 roundings (the two means, the product or the
    difference, the cast of a non-f32 f64 sum); doubled: |b' - b| <= 8u|b|, |c' - c| <= 8u|a|(|mg| + |t|),
    absolute because c cancels. exact (M a power of two, half-integer sums): the means and their
    difference are f32 numbers, nothing rounds, equality. Returns the largest |error| / bound."""
    coef = t64(coef)
    ref, mg, t = bwd_coef(t64(sums, coef.device), M, mean, invstd, gamma)
    _raise("coef[0] = gamma*invstd", coef[0] != ref[0], coef[0], ref[0])
    if exact:
        assert is_pow2(M), "premise: M a power of two"
        for v in (mg, t, mg - t, ref[1], ref[2]):
            assert bool((v.float().double() == v).all()), "premise: dyadic means"
        _raise("coef[1] (exact)", coef[1] != ref[1], coef[1], ref[1])
        _raise("coef[2] (exact)", coef[2] != ref[2], coef[2], ref[2])
        return 0.0
    eb, bb = (coef[1] - ref[1]).abs(), 8 * U * ref[1].abs()
    ec, bc = (coef[2] - ref[2]).abs(), 8 * U * ref[0].abs() * (mg.abs() + t.abs())
    _raise("coef[1]", ~(eb <= bb), coef[1], ref[1], bb)
    _raise("coef[2]", ~(ec <= bc), coef[2], ref[2], bc)
    return max(float((eb / bb.clamp_min(1e-300)).max()), float((ec / bc.clamp_min(1e-300)).max()))


def check_bwd_apply(dx, dres, dy, y, x, coef, act, dtype):
    """mx_bn_bwd_apply_ex with coefficients A in {.5, 1, 2}, B in {-.25, 0, .5}, C in halves, |C| <= 3.
    act 0 / 1: dx and dres are multiples of 1/8 below 2^5, exact in f32 and bf16: equality. act 2: dres is the
    stored form of float32(0.2f * dy); where B = C = 0, dx is the stored form of A * float32(0.2f * dy);
    elsewhere |dx' - dx| <= 4u(|A g| + |B x| + |C|) (one rounding each for g, the first sum, the second
    sum; 4 allows the second-order terms), plus 2^-8 |dx| for a bf16 store. dres may be None. Returns the
    largest |error| / bound of the bounded elements."""
    dx = t64(dx)
    d = dx.device
    coef = t64(coef, d)
    A, B, C = coef[0], coef[1], coef[2]
    xx = t64(x)
    g = t64(dy) * act_grad(y if act else dy, act)
    worst = 0.0
    if act != 2:
        ref = A * g + B * xx + C
        assert bool(((8 * ref) == torch.round(8 * ref)).all()) and float(ref.abs().max()) < 32, "premise: eighths"
        _raise("dx (exact)", dx != ref, dx, ref)
        gref = g
    else:
        g32 = g.float().double()            # the kernel's g: one f32 rounding of the f64-exact product
        gref = store_as(g32.float(), dtype).double()
        plain = ((B == 0) & (C == 0)).expand_as(dx)
        ref0 = store_as((A * g32).float(), dtype).double()
        _raise("dx (act 2, B = C = 0)", plain & (dx != ref0), dx, ref0)
        ref = A * g + B * xx + C
        bound = 4 * U * ((A * g).abs() + (B * xx).abs() + C.abs().expand_as(dx))
        if dtype == BF16:
            bound = bound + 2.0 ** -8 * ref.abs()
        err = (dx - ref).abs()
        _raise("dx (act 2)", ~plain & ~(err <= bound), dx, ref, bound)
        worst = float(torch.where(plain, 0.0, err / bound.clamp_min(1e-300)).max())
    if dres is not None:
        dres = t64(dres)
        _raise("dres", dres != gref, dres, gref)
    return worst


def check_apply(got, x, scale, shift, res, act, ydtype):
    """mx_bn_apply: equal to the f32 value (f32 output) or to its round-to-nearest-even bf16."""
    got = t64(got)
    ref = store_as(apply_ref(x, scale, shift, res, act), ydtype).double()
    _raise("bn_apply", got != ref, got, ref)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def check_finalize(got, stats, count, gamma, beta, rm0=None, rv0=None):
    """got: dict of float32 numpy arrays mean, invstd, scale, shift (and running_mean, running_var when
    rm0 / rv0 are given). The partials are integer-valued f32, so s and q are exact in f64; with variance
    >= 1 (or exactly 0) and |mean| <= 4 the cancellation in q/count - mean^2 costs < 1e-13 relative, far
    below an f32 ulp. mean, invstd, running stats and scale (gamma a power of two) are within 1 f32 ulp of
    the f64 formula rounded to f32; mean is equal when count is a power of two; a zero-variance channel's
    invstd is float32(1/sqrt(float64(float32(1e-5)))); |shift' - shift| <= 8u(|beta| + |mean*scale|):
    casts of mean and invstd, the product and the difference are 4 roundings, doubled."""
    st = np.asarray(stats, np.float64)
    assert np.array_equal(st, np.rint(st)) and np.abs(st).max() < 2.0 ** 24, "premise: integer partials"
    ref = finalize_ref(stats, count, gamma, beta, rm0, rv0)
    assert np.all((ref["var"] >= 1.0) | (ref["var"] == 0.0)) and np.abs(ref["mean"]).max() <= 4.0, "premise: variance"
    if gamma is not None:
        m, _ = np.frexp(np.asarray(gamma, np.float64))
        assert np.all(m == 0.5), "premise: gamma a power of two"
    check_distinct(ref["mean"], ref["mean"].shape[0])
    names = ["mean", "invstd", "scale"] + (["running_mean", "running_var"] if rm0 is not None else [])
    for n in names:
        r32 = ref[n].astype(np.float32)
        g = np.asarray(got[n], np.float32)
        _raise(f"{n} (1 ulp)", ~(np.abs(g.astype(np.float64) - r32) <= _ulp32(r32)), g, r32)
    if is_pow2(count):
        _raise("mean (count a power of two)", np.asarray(got["mean"], np.float64) != ref["mean"], got["mean"], ref["mean"])
    zero = ref["var"] == 0.0
    const = np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5))))
    _raise("invstd (variance 0)", zero & (np.asarray(got["invstd"], np.float32) != const), got["invstd"],
           np.full_like(ref["invstd"], const))
    b = np.zeros_like(ref["mean"]) if beta is None else np.asarray(beta, np.float64)
    err = np.abs(np.asarray(got["shift"], np.float64) - ref["shift"])
    bound = 8 * U * (np.abs(b) + np.abs(ref["mean"] * ref["scale"]))
    _raise("shift", ~(err <= bound), got["shift"], ref["shift"], bound)
    return float((err / np.maximum(bound, 1e-300)).max())
