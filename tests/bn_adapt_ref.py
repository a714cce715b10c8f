"""float64 restatement of test-time BatchNorm adaptation (mx_bn_finalize_adapt, csrc/mx_bn.hip; formulas in
include/mx_det.h and mx_det/adapt.py) and its assertion predicate (a helper, not a test). The method is
tests/bn_ref.py's: integer-valued partials whose column sums are exact, per-channel comparison, bounds
counted in roundings (u = 2^-24 for f32 results, U64 = 2^-53 for the f64 state), never chosen."""
import numpy as np

import bn_ref
from bn_ref import EPS, U, _raise, _ulp32

U64 = 2.0 ** -53


# ---- the restatement, one function per step -------------------------------------------------------

def batch_stats(stats, count):
    """(m_b, v_b): mean and biased variance of `count` rows from the partials [2][mb][K]."""
    st = np.asarray(stats, np.float64)
    m = st[0].sum(0) / count
    return m, np.maximum(st[1].sum(0) / count - m * m, 0.0)


def stream_merge(state, m_b, v_b, count):
    """Chan's merge of a batch into state [3][K] = (rows, mean, M2); returns the new state."""
    rows, mean, M2 = np.asarray(state, np.float64)
    d = m_b - mean
    rows1 = rows + count
    return np.stack([rows1, mean + d * count / rows1, M2 + v_b * count + d * d * rows * count / rows1])


def target_of(state):
    return state[1], state[2] / state[0]


def blend(m_t, v_t, n, prior, src_mean, src_var):
    """Schneider et al. eq. 1 with the prior and n in images."""
    a = prior / (prior + n)
    return (a * np.asarray(src_mean, np.float64) + (1.0 - a) * m_t,
            a * np.asarray(src_var, np.float64) + (1.0 - a) * v_t)


def outputs(mu, var, gamma, beta, eps=EPS):
    K = mu.shape[0]
    g = np.ones(K) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(K) if beta is None else np.asarray(beta, np.float64)
    invstd = 1.0 / np.sqrt(var + eps)
    return dict(mean=mu, var=var, invstd=invstd, scale=g * invstd, shift=b - mu * g * invstd)


def adapt_ref(stats, count, gamma, beta, src_mean, src_var, prior, n, state0=None):
    """The whole of section 1: (outputs dict, new state or None)."""
    m_b, v_b = batch_stats(stats, count)
    state = None
    if state0 is not None:
        state = stream_merge(state0, m_b, v_b, count)
        m_b, v_b = target_of(state)
    mu, var = blend(m_b, v_b, n, prior, src_mean, src_var)
    return outputs(mu, var, gamma, beta), state


# ---- counted f64 bounds of one merge --------------------------------------------------------------

def batch_var_err(stats, count):
    """|error| of the f64 v_b: the division (u q/count), the rounding of m_b squared through (2u m_b^2),
    the square (u m_b^2) and the difference (u v_b)."""
    st = np.asarray(stats, np.float64)
    m, v = batch_stats(stats, count)
    return U64 * (st[1].sum(0) / count + 3.0 * m * m + v)


def merge_err(state0, m_b, v_b, count, e_v, e_mean0=0.0):
    """(e_mean, e_M2) of one merge whose inputs carry |mean error| <= e_mean0 and |v_b error| <= e_v.
    mean' = mean + d*count/rows': m_b, d, the product, the quotient and the sum are 5 roundings, each at
    most U64 (|mean| + |m_b|) since count/rows' <= 1, and the incoming error passes with a factor <= 1.
    M2' = M2 + v_b*count + d^2*rows*count/rows' (all terms >= 0): e_v*count, one rounding of v_b*count, the
    error of d (e_d = U64(|m_b| + |d|) + e_mean0) through the square, 4 roundings of the products and the
    quotient of the last term T, 2 roundings of the sums. Every count is doubled (second-order terms and a
    compiler's choice of fused multiply-adds), as tests/bn_ref.py does."""
    rows, mean, M2 = np.asarray(state0, np.float64)
    d = m_b - mean
    rows1 = rows + count
    f = rows * count / rows1
    T = d * d * f
    e_d = U64 * (np.abs(m_b) + np.abs(d)) + e_mean0
    e_mean = 2 * 5 * U64 * (np.abs(mean) + np.abs(m_b)) + e_mean0
    e_M2 = 2 * (e_v * count + U64 * v_b * count + (2 * e_d * np.abs(d) + e_d * e_d) * f + 4 * U64 * T
                + 2 * U64 * (M2 + v_b * count + T))
    return e_mean, e_M2


# ---- the predicate --------------------------------------------------------------------------------

def _premises(stats, gamma, src_mean, src_var, prior, n):
    st = np.asarray(stats, np.float64)
    assert np.array_equal(st, np.rint(st)) and np.abs(st).max() < 2.0 ** 24, "premise: integer partials"
    sm, sv = np.asarray(src_mean, np.float64), np.asarray(src_var, np.float64)
    assert np.array_equal(sm, np.rint(sm)) and np.abs(sm).max() <= 3 and np.all(np.isin(sv, (0.5, 1.0, 2.0))), \
        "premise: source statistics from bn_ref.running_init"
    if gamma is not None:
        m, _ = np.frexp(np.asarray(gamma, np.float64))
        assert np.all(m == 0.5), "premise: gamma a power of two"
    assert n > 0 and prior in (0, n, 3 * n), "premise: prior in {0, n, 3n} (a in {0, 1/2, 3/4}, exact)"


def check_adapt(got, stats, count, gamma, beta, src_mean, src_var, prior, n, state0=None, got_state=None):
    """got: dict of float32 numpy arrays mean, var, scale, shift written by one mx_bn_finalize_adapt launch;
    state0 / got_state: the f64 state [3][K] before / after it (stream mode), else None.

    Premises (asserted): integer-valued partials (bn_ref.finalize_operands: s and q exact in f64, variance
    >= 5 or exactly 0, |mean| <= 4), source statistics from bn_ref.running_init (integers, variances in
    {1/2, 1, 2}), gamma a power of two, prior in {0, n, 3n} so that a and 1 - a are exact and a*src, (1-a)*m_t
    round nowhere.

    State, against the restated merge of state0: rows' equal (integers below 2^53); mean' and M2' within
    merge_err (counted there, in U64 = 2^-53).

    Outputs, against the restatement (in stream mode evaluated at the restated state): every f64 error
    above is far below an f32 ulp where nothing cancels, so var and scale (gamma a power of two) are
    within 1 f32 ulp of the f64 formula rounded to f32 -- var terms are all >= 0. The mean blend can
    cancel, so mean is within 1 f32 ulp plus the absolute f64 error 16 U64 (|a src_mean| + (1-a)(|mean0| +
    |m_b|)): m_b, the 5 roundings of the merge and the sum of the blend are 7, doubled. A channel whose
    blended variance is exactly 0 has var == 0 and scale == gamma * float32(1/sqrt(float64(float32(1e-5)))).
    |shift' - shift| <= 8u(|beta| + |mean*scale|): the casts of mean and invstd, the product and the
    difference are 4 f32 roundings, doubled (bn_ref.check_finalize's count; the tail is the same code).
    Returns the largest |shift error| / bound."""
    _premises(stats, gamma, src_mean, src_var, prior, n)
    m_b, v_b = batch_stats(stats, count)
    assert np.all((v_b >= 1.0) | (v_b == 0.0)) and np.abs(m_b).max() <= 4.0, "premise: variance"
    ref, state = adapt_ref(stats, count, gamma, beta, src_mean, src_var, prior, n, state0)
    bn_ref.check_distinct(ref["mean"], ref["mean"].shape[0])
    mean0 = 0.0
    if state0 is not None:
        gs = np.asarray(got_state, np.float64)
        assert gs.shape == state.shape
        e_mean, e_M2 = merge_err(state0, m_b, v_b, count, batch_var_err(stats, count))
        _raise("state rows (exact)", gs[0] != state[0], gs[0], state[0])
        _raise("state mean", ~(np.abs(gs[1] - state[1]) <= e_mean), gs[1], state[1], e_mean)
        _raise("state M2", ~(np.abs(gs[2] - state[2]) <= e_M2), gs[2], state[2], e_M2)
        mean0 = np.abs(np.asarray(state0, np.float64)[1])
    a = prior / (prior + n)
    slack = {"mean": 16 * U64 * (np.abs(a * np.asarray(src_mean, np.float64)) + (1 - a) * (mean0 + np.abs(m_b)))}
    for name in ("mean", "var", "scale"):
        r32 = ref[name].astype(np.float32)
        g = np.asarray(got[name], np.float32)
        _raise(f"{name} (1 ulp)", ~(np.abs(g.astype(np.float64) - r32) <= _ulp32(r32) + slack.get(name, 0.0)), g, r32)
    zero = ref["var"] == 0.0
    const = np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5))))
    gm = np.ones_like(const) if gamma is None else np.asarray(gamma, np.float32)
    _raise("var (exactly 0)", zero & (np.asarray(got["var"], np.float32) != 0), got["var"], ref["var"])
    _raise("scale (variance 0)", zero & (np.asarray(got["scale"], np.float32) != gm * const), got["scale"],
           np.broadcast_to(gm * const, zero.shape))
    b = np.zeros_like(ref["mean"]) if beta is None else np.asarray(beta, np.float64)
    err = np.abs(np.asarray(got["shift"], np.float64) - ref["shift"])
    bound = 8 * U * (np.abs(b) + np.abs(ref["mean"] * ref["scale"]))
    _raise("shift", ~(err <= bound), got["shift"], ref["shift"], bound)
    return float((err / np.maximum(bound, 1e-300)).max())


def as_got(out):
    """The f32 arrays a launch would write, from a restated outputs dict (for the host tests)."""
    return {k: out[k].astype(np.float32) for k in ("mean", "var", "scale", "shift")}
