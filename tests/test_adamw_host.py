"""AdamW without a GPU: the argument checks of mx_adamw_step / mx_adamw_pack_build / mx_adamw_pack_step
(MX_EINVAL with a message before any HIP call -- with no device any HIP call would fail as MX_EHIP),
the host-only plan build against mx_sgd_pack_build's tiling for the job list of test_gpu_adamw.py, and
mx_det.optim.AdamW on CPU parameters (torch's own implementation: bit-identical, state_dict
interchangeable with torch.optim.AdamW in both directions)."""
import ctypes

import pytest
import torch

import adamw_cases as ac

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from mx_det import _lib
    return _lib.load()


def _err(lib):
    return lib.mx_last_error().decode()


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-4)


def test_adamw_step_argument_errors(lib):
    P, G, M, V = (_ptrs([0x1000 * (i + 1), 0x1000 * (i + 5)]) for i in range(4))
    N, S = _i64([16, 7]), _i64([1, 3])

    def call(p=P, g=G, m=M, v=V, n=N, s=S, count=2, hyper=HYPER):
        return lib.mx_adamw_step(p, g, m, v, n, s, count, *hyper, None)

    assert call(p=None) == EINVAL and "bad tensor lists" in _err(lib)
    assert call(s=None) == EINVAL and "bad tensor lists" in _err(lib)
    assert call(count=-1) == EINVAL and "bad tensor lists" in _err(lib)
    assert call(n=_i64([16, 0])) == EINVAL and "tensor 1 empty or null" in _err(lib)
    assert call(g=_ptrs([0x1000, None])) == EINVAL and "tensor 1 empty or null" in _err(lib)
    assert call(s=_i64([1, 0])) == EINVAL and "step 0" in _err(lib)
    assert call(hyper=(1e-3, 1.0, 0.999, 1e-8, 0.0)) == EINVAL and "betas" in _err(lib)
    assert call(hyper=(1e-3, 0.9, -0.1, 1e-8, 0.0)) == EINVAL and "betas" in _err(lib)
    assert call(hyper=(1e-3, 0.9, 0.999, -1e-8, 0.0)) == EINVAL and "eps" in _err(lib)
    assert call(count=0) == 0  # nothing to do, no launch


def _jobs(split):
    """(params as (address, numel, pack index), pack descriptors) for adamw_cases with made-up device
    addresses: the builds are host-only and never dereference them."""
    from mx_det.conv import PackDesc
    addr = 0x10000000
    params, descs = [], []
    for shp, st, pd in ac.CONVS:
        K, C, R, S = shp
        n = ac.numel(shp)
        cp, kp = ac.ceil8(C), ac.ceil8(K)
        fus = R * S <= 49
        if fus:
            descs.append(PackDesc(addr, addr + 0x100000, addr + 0x200000, C, K, cp, kp, R, S, st[0], st[1], pd[0], pd[1],
                                  2 if split else 0))
        params.append((addr, n, len(descs) - 1 if fus else -1))
        addr += 0x1000000
    for shp in ac.PLAIN:
        params.append((addr, ac.numel(shp), -1))
        addr += 0x1000000
    return params, (PackDesc * len(descs))(*descs)


def _build_adamw(lib, params, descs, plan_bytes=None, reserved=0):
    n = len(params)
    prm = (ac.AdamwParam * n)(*[ac.AdamwParam(a, a + 0x400000, a + 0x800000, ne, pk, reserved) for a, ne, pk in params])
    nb = lib.mx_adamw_pack_plan_bytes(n)
    buf = (ctypes.c_uint8 * nb)()
    blocks, lds = ctypes.c_int64(-1), ctypes.c_size_t(0)
    rc = lib.mx_adamw_pack_build(prm, n, descs, buf, nb if plan_bytes is None else plan_bytes, ctypes.byref(blocks),
                                 ctypes.byref(lds))
    return rc, blocks.value, lds.value


@pytest.mark.parametrize("split", [False, True])
def test_adamw_pack_build_matches_sgd_tiling(lib, split):
    """Host-only (this machine has no device: a device call would fail), and the same tiling as
    mx_sgd_pack_build for the same tensors and packs, nothing hard-coded."""
    params, descs = _jobs(split)
    rc, blocks, lds = _build_adamw(lib, params, descs)
    assert rc == 0, _err(lib)
    n = len(params)
    prm = (ac.SgdParam * n)(*[ac.SgdParam(a, a + 0x400000, ne, 0, pk) for a, ne, pk in params])
    nb = lib.mx_sgd_pack_plan_bytes(n)
    buf = (ctypes.c_uint8 * nb)()
    sb, sl = ctypes.c_int64(-1), ctypes.c_size_t(0)
    assert lib.mx_sgd_pack_build(prm, n, descs, buf, nb, ctypes.byref(sb), ctypes.byref(sl)) == 0, _err(lib)
    assert blocks == sb.value and blocks > n
    assert lds == sl.value and lds > 0


def test_adamw_pack_build_argument_errors(lib):
    params, descs = _jobs(True)
    assert lib.mx_adamw_pack_plan_bytes(0) == 0 and lib.mx_adamw_pack_plan_bytes(len(params)) > 0
    rc, _, _ = _build_adamw(lib, params, descs, plan_bytes=lib.mx_adamw_pack_plan_bytes(len(params)) - 1)
    assert rc == EINVAL and "plan buffer too small" in _err(lib)
    rc, _, _ = _build_adamw(lib, params, descs, reserved=1)
    assert rc == EINVAL and "reserved" in _err(lib)
    blocks, lds = ctypes.c_int64(0), ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * 64)()
    assert lib.mx_adamw_pack_build(None, 3, descs, buf, 64, ctypes.byref(blocks), ctypes.byref(lds)) == EINVAL
    assert "bad lists" in _err(lib)
    rc, _, _ = _build_adamw(lib, [(params[0][0], 0, -1)], None)
    assert rc == EINVAL and "empty or null" in _err(lib)
    rc, _, _ = _build_adamw(lib, [(params[0][0], params[0][1], 0)], None)
    assert rc == EINVAL and "without pack list" in _err(lib)
    # the 81-tap weight as a fused pack
    from mx_det.conv import PackDesc
    a = 0x10000000
    d81 = (PackDesc * 1)(PackDesc(a, a + 0x100000, a + 0x200000, 8, 8, 8, 8, 9, 9, 1, 1, 4, 4, 0))
    rc, _, _ = _build_adamw(lib, [(a, 8 * 8 * 81, 0)], d81)
    assert rc == EINVAL and "81 taps" in _err(lib)


def test_adamw_pack_step_argument_errors(lib):
    def call(plan=0x1000, grads=0x2000, n=3, blocks=5, lds=1024, step=1, hyper=HYPER):
        return lib.mx_adamw_pack_step(plan, grads, n, blocks, lds, step, *hyper, None)

    assert call(plan=None) == EINVAL and "bad plan" in _err(lib)
    assert call(grads=None) == EINVAL and "bad plan" in _err(lib)
    assert call(blocks=0) == EINVAL and "bad plan" in _err(lib)
    assert call(lds=1 << 20) == EINVAL and "bad plan" in _err(lib)
    assert call(step=0) == EINVAL and "step 0" in _err(lib)
    assert call(hyper=(1e-3, -0.5, 0.999, 1e-8, 0.0)) == EINVAL and "betas" in _err(lib)
    assert call(hyper=(1e-3, 0.9, 1.0, 1e-8, 0.0)) == EINVAL and "betas" in _err(lib)
    assert call(hyper=(1e-3, 0.9, 0.999, -1.0, 0.0)) == EINVAL and "eps" in _err(lib)


def _cpu_params():
    shapes = [s for s, _, _ in ac.CONVS[:3]] + ac.PLAIN
    return [torch.nn.Parameter(ac.initial(torch, s, i)) for i, s in enumerate(shapes)]


def _set_grads(ps, step):
    for i, p in enumerate(ps):
        p.grad = ac.gradient(torch, tuple(p.shape), step, i)


def _same_state(oa, a, ob, b):
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        sa, sb = oa.state[p], ob.state[q]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device and torch.equal(sa[k], sb[k]), k


def test_adamw_cpu_parameters_are_torchs_bits():
    from mx_det.optim import AdamW
    a, b = _cpu_params(), _cpu_params()
    oa = AdamW(a, lr=1e-3, weight_decay=1e-4)
    ob = torch.optim.AdamW(b, lr=1e-3, weight_decay=1e-4)
    assert isinstance(oa, torch.optim.AdamW) and oa.defaults == ob.defaults
    for step in range(5):
        _set_grads(a, step)
        _set_grads(b, step)
        oa.step()
        ob.step()
        _same_state(oa, a, ob, b)
    assert float(oa.state[a[0]]["step"]) == 5.0


def test_adamw_state_dict_round_trips_both_ways():
    from mx_det.optim import AdamW
    for first, second in ((AdamW, torch.optim.AdamW), (torch.optim.AdamW, AdamW)):
        a, b, r = _cpu_params(), _cpu_params(), _cpu_params()
        oa = first(a, lr=1e-3, weight_decay=1e-4)
        orf = torch.optim.AdamW(r, lr=1e-3, weight_decay=1e-4)  # uninterrupted reference run
        for step in range(2):
            _set_grads(a, step)
            _set_grads(r, step)
            oa.step()
            orf.step()
        ob = second(b, lr=5e-4, weight_decay=0.0)
        ob.load_state_dict(oa.state_dict())
        assert ob.param_groups[0]["lr"] == 1e-3 and ob.param_groups[0]["weight_decay"] == 1e-4
        with torch.no_grad():
            for p, q in zip(a, b):
                q.copy_(p)
        for step in range(2, 4):
            _set_grads(b, step)
            _set_grads(r, step)
            ob.step()
            orf.step()
        _same_state(ob, b, orf, r)
        sd = ob.state_dict()
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
