"""mx_det.optim.AdamW on the device (mx_adamw_step, mx_adamw_pack_step) over the parameter set of
tests/adamw_cases.py: 12 steps, a cosine schedule stepping lr every 3 steps, one parameter without a
grad at step 2 (its step number diverges from then on), load_state_dict(state_dict()) at step 8.

1. against torch.optim.AdamW on the same device, every step: rtol 1e-6, atol 1e-7 (the tolerance of
   test_sgd_matches_torch; an f32 restatement of the rule with single-rounded ops uses <= 11 % of it).
2. against the same run in f64 on the CPU: per tensor max|p_kernel - p_f64| <= 2 * err_torch + 2 ulp_f32(max|p|),
   err_torch being torch's f32 CPU run in the same test (2: another equally valid rounding order; the
   ulp floor: tensors where torch happens to land exactly).
3. the fused path equals the plain path bit for bit after every step (parameters, exp_avg, exp_avg_sq),
4. and its packed operands are what a fresh WeightPacker + refresh() writes from the updated weights.
5. version counters, the amsgrad fall-back (torch's bits), differing step numbers under a packer.
6. the U-Net training loop of test_unet_train_steps_decrease_loss with this optimizer.
"""
import functools
import math

import pytest
import torch

import adamw_cases as ac

pytestmark = pytest.mark.gpu

SHAPES = [s for s, _, _ in ac.CONVS] + ac.PLAIN
HYPER = dict(lr=1e-3, weight_decay=1e-4)


@functools.lru_cache(maxsize=None)
def _grads():
    """[step][tensor] CPU f32, computed once and never modified."""
    return [[ac.gradient(torch, s, step, i) for i, s in enumerate(SHAPES)] for step in range(ac.STEPS)]


def _params(device, dtype=torch.float32):
    return [torch.nn.Parameter(ac.initial(torch, s, i).to(device=device, dtype=dtype)) for i, s in enumerate(SHAPES)]


def _set_grads(ps, step, skip):
    for i, (p, g) in enumerate(zip(ps, _grads()[step])):
        if skip and step == 2 and i == ac.NO_GRAD_AT_STEP2:
            p.grad = None
        elif i == ac.MISALIGNED and p.is_cuda:
            buf = torch.empty(g.numel() + 1, dtype=p.dtype, device=p.device)
            buf[1:].copy_(g)
            p.grad = buf[1:]  # starts 4 bytes into its storage
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = g.to(device=p.device, dtype=p.dtype)


def _run(opt, ps, after=None, skip=True):
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4, eta_min=1e-6)
    for step in range(ac.STEPS):
        if step == 8:
            opt.load_state_dict(opt.state_dict())
        _set_grads(ps, step, skip)
        opt.step()
        if (step + 1) % 3 == 0:
            sched.step()
        if after is not None:
            after(step)
    assert abs(opt.param_groups[0]["lr"] - 1e-6) < 1e-12  # the schedule ran to its end


def _snapshot(opt, ps):
    out = []
    for p in ps:
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])))
    return out


@functools.lru_cache(maxsize=None)
def _cpu_finals():
    """Final parameters of torch.optim.AdamW on the CPU in f32 and in f64 (the f32 inputs widened)."""
    out = []
    for dt in (torch.float32, torch.float64):
        ps = _params("cpu", dt)
        _run(torch.optim.AdamW(ps, **HYPER), ps)
        out.append([p.detach().clone() for p in ps])
    return out


def _calls(monkeypatch):
    """Names of the libmx_det entries mx_det.optim and mx_det.conv call from here on."""
    from mx_det import _lib, conv as mc
    names = []
    orig = _lib.call

    def call(name, *a):
        names.append(name)
        return orig(name, *a)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(mc, "call", call)
    return names


def _packer(ps, split):
    from mx_det import conv as mc
    pk = mc.WeightPacker()
    for p, (_, st, pd) in zip(ps, ac.CONVS):
        pk.register(p, st, pd, True, split=split)
    return pk


def test_adamw_matches_torch_every_step(dev, monkeypatch):
    from mx_det import conv as mc
    from mx_det.optim import AdamW
    assert mc.get_packer() is None
    names = _calls(monkeypatch)
    a, b = _params(dev), _params(dev)
    oa, ob = AdamW(a, **HYPER), torch.optim.AdamW(b, **HYPER)
    snaps = []
    _run(oa, a, after=lambda step: snaps.append(_snapshot(oa, a)))
    assert set(names) == {"mx_adamw_step"} and len(names) == ac.STEPS
    steps = iter(snaps)

    def check(step):
        for i, ((p, m, v, n), q) in enumerate(zip(next(steps), b)):
            st = ob.state[q]
            assert n == float(st["step"]), (step, i)
            for x, y, what in ((p, q, "p"), (m, st["exp_avg"], "exp_avg"), (v, st["exp_avg_sq"], "exp_avg_sq")):
                assert torch.allclose(x, y, rtol=1e-6, atol=1e-7), (step, i, what, (x - y).abs().max().item())
    _run(ob, b, after=check)
    assert float(oa.state[a[ac.NO_GRAD_AT_STEP2]]["step"]) == ac.STEPS - 1
    # the state is torch's layout: it loads into torch.optim.AdamW as it is
    oc = torch.optim.AdamW(_params(dev), **HYPER)
    oc.load_state_dict(oa.state_dict())
    assert not oc.state[oc.param_groups[0]["params"][0]]["step"].is_cuda


def _ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


def test_adamw_error_against_f64(dev):
    from mx_det.optim import AdamW
    p32, p64 = _cpu_finals()
    ps = _params(dev)
    _run(AdamW(ps, **HYPER), ps)
    bad = []
    for i, (p, t, r) in enumerate(zip(ps, p32, p64)):
        ek = (p.detach().cpu().double() - r).abs().max().item()
        et = (t.double() - r).abs().max().item()
        floor = _ulp(r.abs().max().item())
        print(f"adamw f64 error tensor {i} {tuple(p.shape)}: kernel {ek:.3e} torch {et:.3e} "
              f"ratio {ek / et if et else float('inf'):.3f} ulp {floor:.3e}")
        if not ek <= 2 * et + 2 * floor:
            bad.append((i, ek, et, floor))
    assert not bad, bad


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("split", [False, True])
def test_adamw_fused_equals_plain_bitwise(dev, monkeypatch, split, skip):
    """skip: the run above (steps 0 and 1 fused, the plain path once the step numbers differ);
    not skip: every parameter has a grad at every step, so all 12 steps are fused."""
    from mx_det import conv as mc, optim
    names = _calls(monkeypatch)
    runs = []
    try:
        for fused in (1, 0):
            monkeypatch.setattr(optim, "_ADAMW_PACK", fused)
            ps = _params(dev)
            pk = _packer(ps, split)
            mc.set_packer(pk)
            pk.refresh()
            opt = optim.AdamW(ps, **HYPER)
            snaps = []
            del names[:]

            def after(step):
                pk.refresh()
                snaps.append(_snapshot(opt, ps))
            _run(opt, ps, after=after, skip=skip)
            nf = names.count("mx_adamw_pack_step")
            assert nf == ((2 if skip else ac.STEPS) if fused else 0), names
            assert names.count("mx_adamw_step") == ac.STEPS - nf
            runs.append(snaps)
    finally:
        mc.set_packer(None)
    for step, (sa, sb) in enumerate(zip(*runs)):
        for i, (x, y) in enumerate(zip(sa, sb)):
            assert x[3] == y[3]
            for u, w, what in zip(x[:3], y[:3], ("p", "exp_avg", "exp_avg_sq")):
                assert torch.equal(u, w), (step, i, what)


@pytest.mark.parametrize("split", [False, True])
def test_adamw_fused_operands_are_the_packs(dev, monkeypatch, split):
    from mx_det import conv as mc, optim
    monkeypatch.setattr(optim, "_ADAMW_PACK", 1)
    names = _calls(monkeypatch)
    ps = _params(dev)
    pk = _packer(ps, split)
    fus = [k for k in pk.order if pk.entries[k].w.shape[2] * pk.entries[k].w.shape[3] <= 49]
    assert len(fus) == len(ac.CONVS) - 1 and len(pk.order) == len(ac.CONVS)
    opt = optim.AdamW(ps, **HYPER)

    def after(step):
        clones = [p.detach().clone() for p in ps[:len(ac.CONVS)]]
        fresh = _packer(clones, split)
        fresh.refresh()
        for k, kf in zip(pk.order, fresh.order):
            e, f = pk.entries[k], fresh.entries[kf]
            if k not in fus:  # 81 taps: a plain block of the launch, repacked by the next refresh()
                assert e.version != e.w._version
                continue
            assert e.version == e.w._version, (step, tuple(e.w.shape))
            assert torch.equal(e.wk, f.wk) and torch.equal(e.wt, f.wt), (step, tuple(e.w.shape))
            K, C, R, S = e.w.shape
            assert not e.wk[..., C:].any()  # zero-padded input channels
            if e.stride == (1, 1):  # [planes][Cpad][R][S][Kpad]
                wt = e.wt.view(-1, e.cp, R, S, e.kp)
                assert not wt[..., K:].any() and not wt[:, C:].any()
        del names[:]
        pk.refresh()
        assert names == ["mx_conv_pack_batched"] and pk._plan_key == tuple(k for k in pk.order if k not in fus)
        del names[:]
    try:
        mc.set_packer(pk)
        pk.refresh()
        del names[:]
        _run(opt, ps, after=after, skip=False)
    finally:
        mc.set_packer(None)


def test_adamw_versions_and_fallbacks(dev, monkeypatch):
    from mx_det import conv as mc, optim
    names = _calls(monkeypatch)
    # version counters move on every step, on both kernel paths
    for split, packed in ((False, False), (True, True)):
        ps = _params(dev)
        opt = optim.AdamW(ps, **HYPER)
        try:
            if packed:
                pk = _packer(ps, split)
                mc.set_packer(pk)
                pk.refresh()
            for step in range(3):
                before = [p._version for p in ps]
                _set_grads(ps, step, False)
                opt.step()
                assert all(p._version > v for p, v in zip(ps, before))
                sv = [opt.state[p]["exp_avg"]._version for p in ps]
            assert all(v > 0 for v in sv)
            assert names[-1] == ("mx_adamw_pack_step" if packed else "mx_adamw_step")
        finally:
            mc.set_packer(None)
    # amsgrad: torch's own implementation, torch's bits
    del names[:]
    a, b = _params(dev), _params(dev)
    oa, ob = optim.AdamW(a, amsgrad=True, **HYPER), torch.optim.AdamW(b, amsgrad=True, **HYPER)
    for step in range(3):
        _set_grads(a, step, True)
        _set_grads(b, step, True)
        oa.step()
        ob.step()
    assert not names
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"):
            assert torch.equal(oa.state[p][k], ob.state[q][k]), k
    # differing step numbers under a packer: the plain path, and refresh() repacks
    ps = _params(dev)
    pk = _packer(ps, True)
    opt = optim.AdamW(ps, **HYPER)
    try:
        mc.set_packer(pk)
        pk.refresh()
        for step, want in ((1, "mx_adamw_pack_step"), (2, "mx_adamw_step"), (3, "mx_adamw_step")):
            _set_grads(ps, step, True)
            del names[:]
            opt.step()
            assert [n for n in names if n != "mx_adamw_pack_build"] == [want], (step, names)
            dirty = [k for k in pk.order if pk.entries[k].version != pk.entries[k].w._version]
            assert len(dirty) == (1 if step == 1 else len(ac.CONVS))  # fused: only the 81-tap weight
            pk.refresh()
            fresh = _packer([p.detach().clone() for p in ps[:len(ac.CONVS)]], True)
            fresh.refresh()
            for k, kf in zip(pk.order, fresh.order):
                assert torch.equal(pk.entries[k].wk, fresh.entries[kf].wk)
                assert torch.equal(pk.entries[k].wt, fresh.entries[kf].wt)
    finally:
        mc.set_packer(None)


def test_unet_train_steps_decrease_loss_adamw(dev):
    """The loop of test_gpu_unet_train.py::test_unet_train_steps_decrease_loss with mx_det.optim.AdamW
    (the fused path: the model's WeightPacker is current from the first forward on)."""
    from mx_det import conv as mc
    from mx_det.optim import AdamW
    from mx_det.restoration import CombinedLoss
    from mx_det.unet import RestorationUNet
    torch.manual_seed(3)
    m = RestorationUNet(channels=(8, 16, 32, 64), precision="f32")
    with torch.no_grad():  # non-trivial BN affine and ConvTranspose biases
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.2, 0.2)
            if isinstance(mod, torch.nn.ConvTranspose2d):
                mod.bias.uniform_(-0.1, 0.1)
    m = m.to(dev).train()
    try:
        opt = AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
        g = torch.Generator().manual_seed(2)
        clean = torch.rand(8, 3, 64, 64, generator=g).to(dev)
        corrupted = (clean + 0.1 * torch.randn(8, 3, 64, 64, generator=g).to(dev)).clamp(0, 1)
        crit = CombinedLoss(0.3)
        losses = []
        for _ in range(8):
            loss = crit(m(corrupted), clean)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        pk = mc.get_packer()
        assert pk is not None and all(pk.entries[k].version == pk.entries[k].w._version for k in pk.order)
        assert losses[-1] < 0.8 * losses[0], losses
    finally:
        mc.set_packer(None)
