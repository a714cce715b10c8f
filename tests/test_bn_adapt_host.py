"""Everything about test-time BatchNorm adaptation that needs no GPU: the streaming merge of
tests/bn_adapt_ref.py against the one-shot statistics of the concatenated partials, its predicate against
deliberately wrong results built from the restatement (the bounds are not vacuous) and against the
restatement itself, the argument rejections of mx_bn_finalize_adapt (they return before any HIP call), the
MX_BN_ADAPT parser and the adapter's marks on a model that is never run."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_adapt_ref as A  # noqa: E402
import bn_ref as R  # noqa: E402

K, SEED = 72, 61
BATCHES = [(5, 513, 2), (9, 1100, 3), (3, 257, 1)]  # (mblocks, rows, images) of three different forwards


def _operands():
    p = R.channel_params(K, SEED)
    sm, sv = R.running_init(K, SEED)
    stats = [R.finalize_operands(mb, K, count, SEED + i) for i, (mb, count, _) in enumerate(BATCHES)]
    return p, sm, sv, stats


def test_merge_of_three_batches_equals_the_one_shot_statistics():
    """Chan's merge, restated, against mean / biased variance of all rows at once. The bound is the sum of
    the three merges' counted errors (bn_adapt_ref.merge_err, the mean error of one merge fed to the next)
    plus the one-shot side's own: u|m| for its mean, batch_var_err for its variance."""
    _, _, _, stats = _operands()
    state = np.zeros((3, K))
    e_mean = e_M2 = 0.0
    for st, (_, count, _) in zip(stats, BATCHES):
        m_b, v_b = A.batch_stats(st, count)
        em, eM = A.merge_err(state, m_b, v_b, count, A.batch_var_err(st, count), e_mean)
        e_mean, e_M2 = em, e_M2 + eM
        state = A.stream_merge(state, m_b, v_b, count)
    rows = sum(c for _, c, _ in BATCHES)
    allst = np.concatenate(stats, axis=1)
    m1, v1 = A.batch_stats(allst, rows)
    m_t, v_t = A.target_of(state)
    assert np.array_equal(state[0], np.full(K, float(rows)))
    assert float(np.abs(m1).max()) > 0.5 and float(v1[:-1].min()) >= 5.0  # the comparison is of real numbers
    R._raise("merged mean", ~(np.abs(m_t - m1) <= e_mean + A.U64 * np.abs(m1)), m_t, m1)
    bound_v = e_M2 / rows + A.U64 * v_t + A.batch_var_err(allst, rows)
    R._raise("merged variance", ~(np.abs(v_t - v1) <= bound_v), v_t, v1, bound_v)
    # the batches differ in mean, so the between-batch term carries weight: the pooled within-batch
    # variance alone is far from the one-shot variance in some channel
    within = sum(A.batch_stats(s, c)[1] * c for s, (_, c, _) in zip(stats, BATCHES)) / rows
    assert float(np.abs(within - v1).max()) > 0.1


def _stream(mutant=None, prior_of=lambda n: n):
    """Three forwards in stream mode through the restatement; yields the check_adapt arguments of each, with
    `mutant` applied to the outputs (and the state) a correct kernel would have written."""
    p, sm, sv, stats = _operands()
    state, n = np.zeros((3, K)), 0
    for st, (_, count, b) in zip(stats, BATCHES):
        n += b
        prior = prior_of(n)
        out, new = A.adapt_ref(st, count, p["gamma"], p["beta"], sm, sv, prior, n, state)
        got, got_state = A.as_got(out), new
        if mutant is not None:
            got, got_state = mutant(st, count, b, n, prior, state, new, p, sm, sv)
        yield dict(got=got, stats=st, count=count, gamma=p["gamma"], beta=p["beta"], src_mean=sm, src_var=sv,
                   prior=prior, n=n, state0=state, got_state=got_state)
        state = new


def _outs(mu, var, p):
    return A.as_got(A.outputs(mu, var, p["gamma"], p["beta"]))


def m_unbiased(st, count, b, n, prior, s0, s1, p, sm, sv):
    m_b, v_b = A.batch_stats(st, count)
    new = A.stream_merge(s0, m_b, v_b * count / (count - 1), count)
    return _outs(*A.blend(*A.target_of(new), n, prior, sm, sv), p), new


def m_prior_in_rows(st, count, b, n, prior, s0, s1, p, sm, sv):
    return _outs(*A.blend(*A.target_of(s1), s1[0][0], prior, sm, sv), p), s1


def m_no_between_term(st, count, b, n, prior, s0, s1, p, sm, sv):
    m_b, v_b = A.batch_stats(st, count)
    new = np.stack([s1[0], s1[1], s0[2] + v_b * count])
    return _outs(*A.blend(*A.target_of(new), n, prior, sm, sv), p), new


def m_blend_invstd(st, count, b, n, prior, s0, s1, p, sm, sv):
    m_t, v_t = A.target_of(s1)
    a = prior / (prior + n)
    invstd = a / np.sqrt(sv + R.EPS) + (1 - a) / np.sqrt(v_t + R.EPS)
    mu, _ = A.blend(m_t, v_t, n, prior, sm, sv)
    return _outs(mu, 1.0 / (invstd * invstd) - R.EPS, p), s1


def m_swapped(st, count, b, n, prior, s0, s1, p, sm, sv):
    m_t, v_t = A.target_of(s1)
    a = 1.0 - prior / (prior + n)
    return _outs(a * sm + (1 - a) * m_t, a * sv + (1 - a) * v_t, p), s1


def m_n_not_accumulated(st, count, b, n, prior, s0, s1, p, sm, sv):
    return _outs(*A.blend(*A.target_of(s1), b, prior, sm, sv), p), s1


def test_predicate_accepts_the_restatement():
    for prior_of in (lambda n: 0, lambda n: n, lambda n: 3 * n):
        for kw in _stream(prior_of=prior_of):
            A.check_adapt(**kw)
    p, sm, sv, stats = _operands()  # batch mode, with and without the affine
    mb, count, b = BATCHES[0]
    for gamma, beta in ((p["gamma"], p["beta"]), (None, None)):
        for prior in (0, 3 * b):
            out, _ = A.adapt_ref(stats[0], count, gamma, beta, sm, sv, prior, b)
            A.check_adapt(A.as_got(out), stats[0], count, gamma, beta, sm, sv, prior, b)


@pytest.mark.parametrize("mutant", [m_unbiased, m_prior_in_rows, m_no_between_term, m_blend_invstd, m_swapped,
                                    m_n_not_accumulated], ids=lambda f: f.__name__)
def test_predicate_rejects_mutant(mutant):
    """Each wrong formula, run through the three forwards at P = 3n (a = 3/4: every term of the blend carries
    weight and source and target are told apart), is rejected at some forward."""
    rejected = 0
    for kw in _stream(mutant, prior_of=lambda n: 3 * n):
        try:
            A.check_adapt(**kw)
        except AssertionError as e:
            assert "premise" not in str(e), e
            rejected += 1
    assert rejected, f"{mutant.__name__} passed the predicate"


def test_predicate_rejects_a_prior_outside_its_premise():
    kw = next(iter(_stream()))
    kw["prior"] = 5
    with pytest.raises(AssertionError, match="premise"):
        A.check_adapt(**kw)


# ---- argument rejections (before any HIP call) ----------------------------------------------------

def _lib():
    from mx_det import _lib as L
    return L


def test_argument_errors_without_gpu():
    L = _lib()
    lib = L.load()
    need = lib.mx_bn_finalize_workspace(5, 72)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)  # never dereferenced: every call below is rejected first
    ok = dict(stats=p, mb=5, K=72, count=513, gamma=None, beta=None, eps=1e-5, sm=p, sv=p, prior=16.0, n=1.0, state=None,
              mean=p, var=p, scale=p, shift=p, ws=p, wsb=need, stream=None)
    cases = [(dict(prior=-1.0), b"prior < 0"), (dict(prior=0.0, n=0.0), b"prior + n_images <= 0"),
             (dict(sm=None), b"source mean"), (dict(sv=None), b"source mean"), (dict(K=4104), b"K > 4096"),
             (dict(wsb=need - 1), b"workspace"), (dict(ws=None), b"workspace"), (dict(count=0), b"bad sizes"),
             (dict(prior=float("nan")), b"prior < 0")]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = getattr(lib, "mx_bn_finalize_adapt")(*a.values())
        assert rc < 0 and msg in lib.mx_last_error(), (change, rc, lib.mx_last_error())


# ---- the environment switch and the adapter's marks -----------------------------------------------

def test_parse_env():
    from mx_det import adapt
    assert adapt.parse_env("") is None and adapt.parse_env(None) is None
    assert adapt.parse_env("stream:16") == ("stream", 16.0)
    assert adapt.parse_env("batch:0") == ("batch", 0.0)
    assert adapt.parse_env("stream") == ("stream", 16.0) and adapt.parse_env("batch") == ("batch", 16.0)
    for bad in ("on", "stream:x", "1"):
        with pytest.raises(ValueError):
            adapt.parse_env(bad)


def _block():
    from mx_det import conv as mc
    return torch.nn.Sequential(mc.Conv2d(8, 16, 3, padding=1, bias=False), mc.BatchNorm2d(16))


def test_adapter_marks_modules_without_touching_their_state():
    from mx_det import adapt
    from mx_det import conv as mc
    blk = _block().eval()
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    ad = adapt.BNAdapter(blk, mode="stream", prior=16, scope=None)
    assert mc.bn_adapting(blk[1]) is None
    with ad:
        assert mc.bn_adapting(blk[1]) is ad.layers[0][1] and not blk[1].training
        import copy
        assert mc.bn_adapting(copy.deepcopy(blk)[1]) is None  # a copy of an adapted model is not adapted
    assert mc.bn_adapting(blk[1]) is None and "_mx_adapt" not in blk[1].__dict__
    after = blk.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert ad.images_seen == 0
    with pytest.raises(RuntimeError):
        ad.freeze()  # nothing to keep yet
    with pytest.raises(RuntimeError, match="no backward"):  # no autograd through an adapted layer
        mc._no_grad_inputs(torch.zeros(1, 4, 4, 8, requires_grad=True), blk[0], blk[1])
    with torch.no_grad():
        mc._no_grad_inputs(torch.zeros(1, 4, 4, 8, requires_grad=True), blk[0], blk[1])
    with pytest.raises(ValueError):
        adapt.BNAdapter(blk, mode="online", scope=None)
    with pytest.raises(ValueError):
        adapt.BNAdapter(blk, prior=-1, scope=None)


def test_scope_and_backend_errors():
    from mx_det import adapt, frcnn
    from oracle.cpu_backend import CpuBackend
    m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None).eval()
    with pytest.raises(ValueError, match="padded RoI rows"):
        adapt.BNAdapter(m, scope=("box_head",))
    with pytest.raises(ValueError):
        adapt.BNAdapter(m, scope=("rpn",))
    ad = adapt.BNAdapter(m)
    assert len(ad.layers) == 61
    box = {id(b) for b in m.roi_heads.box_head.modules()}
    assert not any(id(b) in box for b, _ in ad.layers)
    m.set_backend(CpuBackend())
    with pytest.raises(NotImplementedError):
        ad.enable()
    assert not ad.enabled
