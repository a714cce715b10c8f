"""mx_bn_finalize_adapt (csrc/mx_bn.hip) per channel against the float64 restatement of
tests/bn_adapt_ref.py, at the edges of its launch geometry: the block counts cross fin_slices (1 slice up
to 32 blocks, then ceil(mb / 32), capped at 64), K = 72 has a partial second 64-channel chunk, K = 4096 is
the chunk limit. Integer partials (bn_ref.finalize_operands: every channel its own values, the last one
constant), a row count that is no multiple of 128, bounds counted in bn_adapt_ref.check_adapt.

Every output lies between two NaN canary rows. Only accepted argument combinations are launched; the
rejected ones return before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_adapt_ref as A  # noqa: E402
import bn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(mb, K) for mb in (1, 5, 33, 65, 257, 2049) for K in (8, 72, 4096) if (mb, K) != (2049, 4096)]
OUT = ("mean", "var", "scale", "shift")
SEED = 43


def _L():
    from mx_det import _lib
    return _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _f32(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ws(mb, K, dev):
    n = _L().load().mx_bn_finalize_workspace(mb, K)
    assert n >= 256
    return torch.zeros(n, dtype=torch.uint8, device=dev)


def _count(mb):
    c = mb * 128 - 37 if mb > 1 else 91
    assert c % 128 and 0 < c <= mb * 128 and c > (mb - 1) * 128
    return c


class Case:
    """One layer's operands on the device, built once per shape."""

    def __init__(self, dev, mb, K, count=None, seed=SEED, affine=True):
        assert mb > 0 and 0 < K <= 4096 and K % 8 == 0
        self.dev, self.mb, self.K, self.count = dev, mb, K, _count(mb) if count is None else count
        p = R.channel_params(K, seed)
        self.gamma, self.beta = (p["gamma"], p["beta"]) if affine else (None, None)
        self.sm, self.sv = R.running_init(K, seed)
        self.stats = R.finalize_operands(mb, K, self.count, seed)
        self.d = {n: _f32(getattr(self, n), dev) for n in ("stats", "gamma", "beta", "sm", "sv")}
        self.keep = {n: (None if t is None else t.clone()) for n, t in self.d.items()}

    def launch(self, prior, n, state=None, ws=None, expect_ok=True, **override):
        """One launch into fresh NaN-filled outputs inside canary rows. Returns (outs, fulls, rc)."""
        fulls = {k: torch.full((3, self.K), float("nan"), dtype=torch.float32, device=self.dev) for k in OUT}
        outs = {k: f[1] for k, f in fulls.items()}
        ws = _ws(self.mb, self.K, self.dev) if ws is None else ws
        a = dict(stats=_p(self.d["stats"]), mb=self.mb, K=self.K, count=self.count, gamma=_p(self.d["gamma"]),
                 beta=_p(self.d["beta"]), eps=R.EPS, sm=_p(self.d["sm"]), sv=_p(self.d["sv"]), prior=float(prior),
                 n=float(n), state=_p(state), mean=_p(outs["mean"]), var=_p(outs["var"]), scale=_p(outs["scale"]),
                 shift=_p(outs["shift"]), ws=_p(ws), wsb=ws.numel(), stream=_L().stream())
        a.update(override)
        if expect_ok:
            _L().call("mx_bn_finalize_adapt", *a.values())
            return outs, fulls, 0
        return outs, fulls, _L().load().mx_bn_finalize_adapt(*a.values())

    def check(self, outs, fulls, prior, n, state0=None, state=None):
        for k, f in fulls.items():
            R.check_canaries(f, k)
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        tag = f"mb={self.mb} K={self.K} count={self.count} prior={prior} n={n} stream={state0 is not None}"
        try:
            r = A.check_adapt(got, self.stats, self.count, self.gamma, self.beta, self.sm, self.sv, prior, n,
                              state0, None if state is None else state.cpu().numpy())
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from None
        print(f"RATIO adapt shift {tag} {r:.4f}")

    def unchanged(self):
        """Case 4: the source statistics, the affine and the partials are bitwise what they were."""
        for n, t in self.d.items():
            assert t is None or _same(t, self.keep[n]), f"{n} was written"


@pytest.mark.parametrize("mb,K", SHAPES)
def test_batch_mode(dev, mb, K):
    """Cases 1, 2, 4, 5, 6 at one shape: P = 0 and P = 3n through check_adapt, twice each on one scratch
    zeroed once (same bits as on a fresh scratch, counters left zero); at P = 0 mean / scale / shift are
    bit-equal to mx_bn_finalize_ex on the same partials and var is within 1 ulp of what its invstd implies."""
    c = Case(dev, mb, K)
    n = 2
    shared = _ws(mb, K, dev)
    for prior in (0, 3 * n):
        fresh = c.launch(prior, n)
        again = [c.launch(prior, n, ws=shared) for _ in range(2)]
        torch.cuda.synchronize()
        c.check(fresh[0], fresh[1], prior, n)
        for outs, fulls, _ in again:
            for k in OUT:
                R.check_canaries(fulls[k], k)
                assert _same(outs[k], fresh[0][k]), f"{k}: a launch on the reused scratch differs (prior {prior})"
        assert int(shared[:256].sum()) == 0, "arrival counters not left zero"
        if prior == 0:
            at0 = fresh[0]
    # case 2: the two ends of the blend against the train-mode finalize
    t = {k: torch.full((K,), float("nan"), dtype=torch.float32, device=dev) for k in ("mean", "invstd", "scale", "shift")}
    ws = _ws(mb, K, dev)
    _L().call("mx_bn_finalize_ex", _p(c.d["stats"]), mb, K, c.count, _p(c.d["gamma"]), _p(c.d["beta"]), R.EPS, R.MOM,
              None, None, _p(t["mean"]), _p(t["invstd"]), _p(t["scale"]), _p(t["shift"]), _p(ws), ws.numel(), _L().stream())
    torch.cuda.synchronize()
    for k in ("mean", "scale", "shift"):
        assert _same(at0[k], t[k]), f"{k}: P = 0 differs from mx_bn_finalize_ex"
    # var_out is the f32 rounding of the f64 variance v whose image f32(1/sqrt(v + eps)) is the train-mode
    # invstd, so v lies within 1 ulp of var_out; 1/sqrt is monotone and so is rounding: the invstd lies
    # between the images of var_out + 1 ulp and var_out - 1 ulp
    inv = t["invstd"].cpu().numpy()
    var = at0["var"].cpu().numpy()
    ulp = np.spacing(np.abs(var)).astype(np.float64)
    img = lambda v: (1.0 / np.sqrt(v + np.float64(np.float32(R.EPS)))).astype(np.float32)
    lo, hi = img(var.astype(np.float64) + ulp), img(var.astype(np.float64) - ulp)
    R._raise("var within 1 ulp of the value mx_bn_finalize_ex's invstd implies", ~((lo <= inv) & (inv <= hi)), var, inv,
             lo, hi)
    c.unchanged()


def test_batch_mode_without_affine(dev):
    c = Case(dev, 5, 72, affine=False)
    for prior in (0, 6):
        outs, fulls, _ = c.launch(prior, 2)
        torch.cuda.synchronize()
        c.check(outs, fulls, prior, 2)


@pytest.mark.parametrize("K", [8, 72, 4096])
def test_stream_mode(dev, K):
    """Case 3: three launches with different (mb, count) on one state at P = n; outputs and state after each."""
    state = torch.zeros((3, K), dtype=torch.float64, device=dev)
    n = 0
    for i, (mb, b) in enumerate(((33, 2), (5, 1), (257, 3))):
        c = Case(dev, mb, K, seed=SEED + i)
        n += b
        s0 = state.cpu().numpy()
        outs, fulls, _ = c.launch(n, n, state=state)
        torch.cuda.synchronize()
        c.check(outs, fulls, n, n, s0, state)
        c.unchanged()
    assert np.array_equal(state[0].cpu().numpy(), np.full(K, float(sum(_count(mb) for mb in (33, 5, 257)))))


def test_argument_errors_leave_the_outputs_untouched(dev):
    """Case 7: every rejected call returns nonzero and writes nothing (outputs still NaN, state still zero)."""
    c = Case(dev, 5, 72)
    state = torch.zeros((3, 72), dtype=torch.float64, device=dev)
    small = torch.zeros(_L().load().mx_bn_finalize_workspace(5, 72) - 8, dtype=torch.uint8, device=dev)
    bad = [dict(prior=-1.0), dict(prior=0.0, n=0.0), dict(sm=None), dict(sv=None), dict(K=4104),
           dict(ws=small)]  # launch() passes the scratch's own size: 8 bytes short
    for change in bad:
        rest = {k: v for k, v in change.items() if k not in ("prior", "n")}
        outs, fulls, rc = c.launch(change.get("prior", 16.0), change.get("n", 2.0), state=state, expect_ok=False, **rest)
        torch.cuda.synchronize()
        assert rc != 0 and _L().load().mx_last_error(), change
        for k in OUT:
            assert bool(torch.isnan(fulls[k]).all()), (change, k)
        assert not bool(state.any()), change
    c.unchanged()
