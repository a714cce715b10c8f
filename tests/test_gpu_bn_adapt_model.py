"""Test-time BatchNorm adaptation (mx_det.adapt.BNAdapter) from conv_bn up to the evaluation runner, on tiny
inputs with seeded random weights, f32 precision unless a test says otherwise. The kernel's arithmetic is
pinned per channel in tests/test_gpu_bn_adapt.py; here: which kernels run (bit-equalities with the train-mode
forward and with plain eval), one layer per element against f64, state handling (stream, freeze, reset), the
scope, and the plumbing."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_adapt_ref as A  # noqa: E402
import bn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _sd_bytes(model):
    return {k: v.detach().cpu().numpy().tobytes() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def model(dev):
    """One detector for the module: random seeded weights, non-trivial BN affine and running statistics."""
    from mx_det import frcnn
    from mx_det.backend import HipBackend
    torch.manual_seed(5)
    m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    m.roi_heads.box_predictor = frcnn.FastRCNNPredictor(m.roi_heads.box_predictor.cls_score.in_features, 7)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for mod in m.modules():
            if hasattr(mod, "running_mean"):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    m.transform.min_size, m.transform.max_size = 128, 192
    return m.to(dev).eval().set_backend(HipBackend("f32"))


@pytest.fixture(autouse=True)
def _no_stale_packer():
    from mx_det import conv as mc
    mc.set_packer(None)
    yield
    mc.set_packer(None)


def _x(dev, seed=0, n=2, h=64, w=96, dtype=torch.float32):
    """A normalised image batch as the transform hands it to the stem: NHWC, RGB padded to 8 channels."""
    x = torch.zeros(n, h, w, 8)
    x[..., :3] = torch.randn(n, h, w, 3, generator=torch.Generator().manual_seed(seed))
    return x.to(dev, dtype)


def _backbone(m, x):
    with torch.no_grad():
        out = m.backbone(x, m.be)
    torch.cuda.synchronize()
    return out


def test_batch_mode_at_prior_0_is_the_train_mode_forward(dev, model):
    """1. The same conv, statistics and apply kernels as train-mode BN (the fused stem included): every FPN
    level bit-equal to a deep copy in .train() under no_grad -- and the adapted model's buffers untouched."""
    from mx_det.adapt import BNAdapter
    x = _x(dev)
    before = _sd_bytes(model)
    with BNAdapter(model, mode="batch", prior=0):
        got = _backbone(model, x)
    twin = copy.deepcopy(model).train()
    ref = _backbone(twin, x)
    assert list(got) == list(ref) and len(got) == 5
    for k in got:
        assert _same(got[k], ref[k]), f"level {k} differs from the train-mode forward"
    assert _sd_bytes(model) == before
    plain = _backbone(model, x)
    assert not _same(plain["0"], got["0"])  # the adapter did change the forward


def test_inert_when_off(dev, model):
    """2. Construct, enable, run, disable: eval outputs bit-equal to a model that never had an adapter, and
    state_dict() byte-equal to its copy from before (running statistics and num_batches_tracked included)."""
    from mx_det.adapt import BNAdapter
    x = _x(dev, 1)
    never = _backbone(copy.deepcopy(model), x)
    before = _sd_bytes(model)
    assert any(k.endswith("num_batches_tracked") for k in before)
    ad = BNAdapter(model, mode="stream", prior=16)
    ad.enable()
    on = _backbone(model, x)
    ad.disable()
    assert ad.images_seen == 2 and not ad.enabled
    after = _backbone(model, x)
    for k in never:
        assert _same(after[k], never[k]), f"level {k} differs after the adapter was disabled"
    assert not _same(on["0"], never["0"])
    assert _sd_bytes(model) == before and not model.backbone.body.bn1.training


def test_one_layer_against_f64(dev):
    """3. Conv2d + BatchNorm2d through conv.conv_bn in stream mode (P = 16) over two different batches; the
    conv output z is read back (the same launch, repeated) and the statistics, the blend and the apply
    restated in f64 from it, per element.

    bn_ref.check_apply is an equality: its operands make x*scale + shift exact. Here scale is not dyadic and
    the statistics come from f32 partials, so the bound is derived, each count doubled as bn_ref does:
      partials  a block's column sums of z and z^2 over at most Rb rows, in f32, any order:
                e_m = Rb u mean|z|,  e_q = (Rb + 1) u mean z^2 (one more rounding for the square),
                e_v = e_q + 2|m_b| e_m + e_m^2; merged over the forwards by their row weights, the
                between-batch term adding w1 w2 (2|d| (e_m1 + e_m2) + (e_m1 + e_m2)^2)
      blend     e_mu = (1-a) e_mt, e_var = (1-a) e_vt
      scale     gamma*f32(invstd): e_s = |gamma| invstd e_var / (2 (var + eps - e_var)) + 2u|scale|
      shift     beta - f32(mu)*scale: e_h = |scale| e_mu + |mu| e_s + 2u|mu scale| + u|shift|
      apply     z*scale + shift in f32, relu (1-Lipschitz): |z| e_s + e_h + u|z scale| + u|y|"""
    from mx_det import conv as mc
    from mx_det.adapt import BNAdapter
    torch.manual_seed(9)
    C, K, P = 16, 72, 16
    blk = torch.nn.Sequential(mc.Conv2d(C, K, 3, padding=1, bias=False), mc.BatchNorm2d(K)).to(dev).eval()
    conv, bn = blk[0], blk[1]
    g = torch.Generator().manual_seed(10)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(K, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(K, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
    gamma, beta = bn.weight.detach().double().cpu().numpy(), bn.bias.detach().double().cpu().numpy()
    sm, sv = bn.running_mean.double().cpu().numpy(), bn.running_var.double().cpu().numpy()
    eps, u = float(np.float32(bn.eps)), R.U
    ad = BNAdapter(blk, mode="stream", prior=P, scope=None)
    state, n, seen = np.zeros((3, K)), 0, []
    for i, shape in enumerate(((2, 20, 24, C), (1, 17, 19, C))):
        x = (torch.randn(shape, generator=g) + 0.3 * i).to(dev)
        with torch.no_grad(), ad:
            y = mc.conv_bn(x, conv, bn, mc.ACT_RELU)
            wk, _ = mc.operands(conv.weight, C, conv.stride, conv.padding, K, False, split=True)
            z, st = mc.conv_fwd(x, wk, conv.stride, conv.padding, stats=True, cin=C)
        torch.cuda.synchronize()
        z64 = z.double().cpu().numpy().reshape(-1, K)
        M = z64.shape[0]
        per = -(-M // st.shape[1])
        Rb = 64 * -(-per // 64)  # rows per partial block, rounded up to the 64-row tile
        m_b, v_b = z64.mean(0), z64.var(0)
        e_m = Rb * u * np.abs(z64).mean(0)
        e_v = (Rb + 1) * u * (z64 * z64).mean(0) + 2 * np.abs(m_b) * e_m + e_m * e_m
        seen.append((M, m_b, e_m, e_v))
        state = A.stream_merge(state, m_b, v_b, M)
        n += shape[0]
        m_t, v_t = A.target_of(state)
        rows = sum(s[0] for s in seen)
        e_mt = sum(s[0] * s[2] for s in seen) / rows
        e_vt = sum(s[0] * s[3] for s in seen) / rows
        if len(seen) == 2:
            w12 = seen[0][0] * seen[1][0] / rows ** 2
            es = seen[0][2] + seen[1][2]
            e_vt = e_vt + w12 * (2 * np.abs(seen[1][1] - seen[0][1]) * es + es * es)
        a = P / (P + n)
        mu, var = A.blend(m_t, v_t, n, P, sm, sv)
        o = A.outputs(mu, var, gamma, beta, eps)
        e_mu, e_var = (1 - a) * e_mt, (1 - a) * e_vt
        assert np.all(e_var < 1e-3 * (var + eps))
        e_s = np.abs(gamma) * o["invstd"] * e_var / (2 * (var + eps - e_var)) + 2 * u * np.abs(o["scale"])
        e_h = np.abs(o["scale"]) * e_mu + np.abs(mu) * e_s + 2 * u * np.abs(mu * o["scale"]) + u * np.abs(o["shift"])
        pre = z64 * o["scale"] + o["shift"]
        ref = np.maximum(pre, 0.0)
        bound = 2 * (np.abs(z64) * e_s + e_h + u * np.abs(z64 * o["scale"]) + u * np.abs(pre))
        got = y.double().cpu().numpy().reshape(-1, K)
        err = np.abs(got - ref)
        print(f"RATIO adapt apply forward {i}: {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        R._raise(f"conv_bn under adaptation, forward {i}", ~(err <= bound), got, ref, bound)
        assert float(np.abs(ref).max()) > 1.0 and float(bound.max()) < 1e-3 * float(np.abs(ref).max())  # not vacuous
    assert ad.images_seen == 3
    assert np.array_equal(ad.states()[0][0].cpu().numpy(), np.full(K, float(sum(s[0] for s in seen))))


def test_stream_fed_one_batch_twice_equals_batch_mode(dev, model):
    """4. P = 0, the same batch twice: d = 0 on the second merge and the doubled M2 over the doubled rows is
    the batch variance, so the stem's second output is batch mode's, bit for bit."""
    from mx_det.adapt import BNAdapter
    x = _x(dev, 2)
    body, be = model.backbone.body, model.be
    with torch.no_grad():
        with BNAdapter(model, mode="batch", prior=0):
            ref = body.stem(x, be)
        with BNAdapter(model, mode="stream", prior=0) as ad:
            first = body.stem(x, be)
            second = body.stem(x, be)
    torch.cuda.synchronize()
    assert _same(first, ref) and _same(second, ref)
    st = ad.states()[0].cpu().numpy()
    assert ad.images_seen == 4 and np.array_equal(st[0], np.full(64, 2.0 * 2 * 32 * 48))


FREEZE_BAR = 1e-5   # tests/test_gpu_x3.py lines 186 and 281: one f32 conv (+ BN, + epilogue) against f64
FREEZE_PATH = 51    # convs on the longest path from the image to any FPN level: stem 1, 16 bottlenecks x 3
#                     (the downsample conv runs beside them), the top lateral conv, the level's output conv


def test_freeze(dev, model, monkeypatch):
    """5. After freeze(): every state tensor bitwise unchanged by further forwards, two runs on one input
    bit-equal, and the frozen (folded) form agrees with the online (unfolded) form.

    The tolerance is that of ONE conv: tests/test_gpu_x3.py holds one f32 conv (+ BN, + epilogue) to a relative
    L2 error of 1e-5 against f64 (its lines 186 and 281). It is applied where it is defined: each of the 61
    adapted layers, frozen, on the very input its online form saw in the online forward (recorded there), must
    be within 1e-5 of the online output. Measured on an MI355X: at most 7.4e-6 per layer, each form at most
    6.5e-6 from an f64 restatement of the layer.

    The features at the end of the chain cannot be held to the tolerance of one conv: the two forms split
    different weights into bf16 hi / lo planes (w * scale against w), so their errors are independent in every
    layer, and a level's longest path has 51 convs. To first order the per-layer relative differences add, so
    the features are held to 51 x 1e-5 (measured: 1.1e-4 to 1.9e-4, the same at 64 x 96, 128 x 192 and
    256 x 384). The bound is far from vacuous: the same forward on the running statistics is more than ten
    times further away, which is asserted. The stem runs unfused here so that it is recorded like
    every other layer; the fused stem is covered by the train-mode and stream tests above."""
    from mx_det import conv as mc
    from mx_det.adapt import BNAdapter
    monkeypatch.setenv("MX_STEM_FUSED", "0")
    xa, xb = _x(dev, 3), _x(dev, 4)
    plain = _backbone(model, xb)
    seen, real = [], mc.adapt_conv_bn

    def recording(x, conv, bn, act, residual, ad):
        y = real(x, conv, bn, act, residual, ad)
        if not ad.frozen:
            seen.append((x, conv, bn, act, residual, ad, y))
        return y

    def rel(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm()).item()

    with BNAdapter(model, mode="stream", prior=16) as ad:
        _backbone(model, xa)
        monkeypatch.setattr(mc, "adapt_conv_bn", recording)
        online = _backbone(model, xb)
        monkeypatch.setattr(mc, "adapt_conv_bn", real)
        assert len(seen) == len(ad.layers) == 61
        # the statistics the online forward of xb used already include xb: freezing now keeps exactly them
        ad.freeze()
        assert ad.frozen and ad.images_seen == 4
        states = [s.clone() for s in ad.states()]
        f1 = _backbone(model, xb)
        f2 = _backbone(model, xb)
        assert ad.images_seen == 4
        for s, t in zip(states, ad.states()):
            assert torch.equal(s.view(torch.int64), t.view(torch.int64))
        worst = 0.0
        with torch.no_grad():
            for x, conv, bn, act, residual, rec, y in seen:
                assert rec.frozen
                r = rel(mc.conv_bn(x, conv, bn, act, residual), y)
                worst = max(worst, r)
                assert r < FREEZE_BAR, (tuple(x.shape), tuple(conv.weight.shape), r)
        print(f"RATIO frozen vs online, worst of 61 layers on the same input: {worst:.3e}")
        for k in f1:
            assert _same(f1[k], f2[k])
            r = rel(f1[k], online[k])
            print(f"RATIO frozen vs online level {k}: {r:.3e}")
            assert r < FREEZE_PATH * FREEZE_BAR, (k, r)
            # frozen runs on the adapter's statistics, not on the running ones
            assert rel(plain[k], online[k]) > 10 * FREEZE_PATH * FREEZE_BAR, (k, rel(plain[k], online[k]))


def test_reset(dev, model):
    """6. reset() zeroes every state and images_seen, and unfreezes."""
    from mx_det.adapt import BNAdapter
    with BNAdapter(model, mode="stream", prior=16) as ad:
        _backbone(model, _x(dev, 5))
        ad.freeze()
        assert ad.images_seen == 2 and all(bool(s.any()) for s in ad.states())
        ad.reset()
        torch.cuda.synchronize()
        assert ad.images_seen == 0 and not ad.frozen
        assert all(s is not None and not bool(s.any()) for s in ad.states())
        _backbone(model, _x(dev, 5))
        assert ad.images_seen == 2


def test_scope(dev, model):
    """7. Default scope: the box head's output for fixed RoI features is bit-equal with and without the
    adapter, and its BatchNorms carry no mark; scope "box_head" is refused with the reason."""
    from mx_det.adapt import BNAdapter
    from mx_det import conv as mc
    feat = torch.randn(6, 7, 7, 256, generator=torch.Generator().manual_seed(7)).to(dev)
    head = model.roi_heads.box_head
    with torch.no_grad():
        ref = head(feat, model.be)
        with BNAdapter(model, mode="batch", prior=0) as ad:
            got = head(feat, model.be)
            assert all(mc.bn_adapting(b) is None for b in head.modules() if isinstance(b, mc.BatchNorm2d))
            assert mc.bn_adapting(model.backbone.fpn.inner_blocks[0][1]) is not None
    torch.cuda.synchronize()
    assert _same(got, ref) and len(ad.layers) == 61
    with pytest.raises(ValueError, match="dead rows"):
        BNAdapter(model, scope=("box_head",))
    with pytest.raises(ValueError, match="dead rows"):
        BNAdapter(model, scope=("backbone", "box_head"))


def _well_formed(outs, n):
    assert len(outs) == n
    for o in outs:
        assert set(o) == {"boxes", "scores", "labels"}
        k = o["scores"].shape[0]
        assert o["boxes"].shape == (k, 4) and o["labels"].shape == (k,) and k <= 100
        assert bool(torch.isfinite(o["boxes"].float()).all()) and bool(torch.isfinite(o["scores"].float()).all())
        assert bool(((o["labels"] >= 1) & (o["labels"] < 7)).all())
        assert bool((o["boxes"][:, 2] >= o["boxes"][:, 0]).all()) and bool((o["boxes"][:, 3] >= o["boxes"][:, 1]).all())


@pytest.mark.parametrize("route", ["unfused", "fused", "bf16"])
def test_end_to_end(dev, model, monkeypatch, route):
    """8. model(images) in eval under the adapter: well-formed detections through the unfused tail, the
    fused one (MX_FUSED_DETECTIONS=1) and bf16 precision; the model's state is untouched."""
    from mx_det.adapt import BNAdapter
    from mx_det.backend import HipBackend
    from mx_det.data import synth_batch
    monkeypatch.setenv("MX_FUSED_DETECTIONS", "1" if route == "fused" else "0")
    m = copy.deepcopy(model).set_backend(HipBackend("bf16" if route == "bf16" else "f32"))
    with torch.no_grad():  # a detection tail that keeps some boxes on random weights
        m.roi_heads.box_predictor.cls_score.weight.mul_(20.0)
    before = _sd_bytes(m)
    imgs, _ = synth_batch(40, 2, H=128, W=160, device=dev)
    with torch.no_grad(), BNAdapter(m, mode="stream", prior=16) as ad:
        outs = m(list(imgs))
        outs2 = m(list(imgs))
    torch.cuda.synchronize()
    _well_formed(outs, 2)
    _well_formed(outs2, 2)
    assert ad.images_seen == 4 and _sd_bytes(m) == before


def test_engine_and_scripts(dev, model, tmp_path, monkeypatch):
    """9. eval_frcnn_variant with an adapter over two synthetic variants: the state is reset between them
    (the stem's rows = that variant's images x its rows per image) and the adapter disabled afterwards. With
    MX_BN_ADAPT unset scripts.eval_all writes byte for byte what the previous logic writes (restated here);
    with MX_BN_ADAPT=stream:16 it adds the <name>_BNAdapt entries beside unchanged unadapted ones."""
    from mx_det import engine
    from mx_det.adapt import BNAdapter
    from mx_det.data import write_coco_split
    from scripts import eval_all
    monkeypatch.delenv("MX_BN_ADAPT", raising=False)
    monkeypatch.delenv("MX_BN_ADAPT_FREEZE_AFTER", raising=False)
    ts = tmp_path / "testsets"
    sizes = {"Test_Clean": (96, 128), "Test_Noise": (80, 144)}
    for i, (v, (h, w)) in enumerate(sizes.items()):
        write_coco_split(ts / v, "val", 100 + 10 * i, 4, h, w, mean_boxes=4)
    ad = BNAdapter(model, mode="stream", prior=16)
    stem = ad.layers[0]
    assert stem[0] is model.backbone.body.bn1
    for v, (h, w) in sizes.items():
        img_dir, ann = eval_all.variant_paths(ts, v)
        res = engine.eval_frcnn_variant(model, img_dir, ann, dev, adapter=ad)
        assert set(res) == {"mAP50_95", "mAP50", "per_class_ap50"} and not ad.enabled
        il, _ = model.transform([torch.zeros(h, w, 3, dtype=torch.uint8, device=dev)], None, model.be)
        H, W = il.tensors.shape[1:3]
        per_image = ((H + 6 - 7) // 2 + 1) * ((W + 6 - 7) // 2 + 1)
        rows = stem[1].state[0].cpu().numpy()
        assert ad.images_seen == 4 and np.array_equal(rows, np.full(64, 4.0 * per_image)), (v, rows[0], per_image)
    # freeze_after: frozen from the third image on, two images merged
    img_dir, ann = eval_all.variant_paths(ts, "Test_Noise")
    engine.eval_frcnn_variant(model, img_dir, ann, dev, adapter=ad, freeze_after=2)
    assert ad.frozen and ad.images_seen == 2 and not ad.enabled

    # the scripts: one checkpoint, the two variants, a small transform for speed
    ck = tmp_path / "best.pth"
    torch.save({"model": model.state_dict()}, ck)
    load = engine.load_frcnn_checkpoint

    def load_small(path, d):
        m = load(path, d)
        m.transform.min_size, m.transform.max_size = 128, 192
        return m

    monkeypatch.setattr(eval_all, "load_frcnn_checkpoint", load_small)
    monkeypatch.setattr(eval_all, "VARIANTS", list(sizes))
    monkeypatch.setattr(eval_all, "COCO_TESTSET_ROOT", ts)
    monkeypatch.setattr(eval_all, "CKPTS", {"FasterRCNN": ck})
    monkeypatch.setattr(eval_all, "OUT_DIR", tmp_path / "off")
    eval_all.main()
    # the previous logic: one entry per checkpoint, eval_frcnn_variant per variant, json.dump(indent=2)
    m = load_small(ck, dev)
    parent = {"FasterRCNN": {v: engine.eval_frcnn_variant(m, *eval_all.variant_paths(ts, v), dev) for v in sizes}}
    want = json.dumps(parent, indent=2, ensure_ascii=False).encode("utf-8")
    off_json = (tmp_path / "off/eval_results.json").read_bytes()
    off_csv = (tmp_path / "off/eval_results.csv").read_bytes()
    assert off_json == want
    monkeypatch.setenv("MX_BN_ADAPT", "stream:16")
    monkeypatch.setattr(eval_all, "OUT_DIR", tmp_path / "on")
    eval_all.main()
    on = json.load(open(tmp_path / "on/eval_results.json"))
    assert list(on) == ["FasterRCNN", "FasterRCNN_BNAdapt"]
    assert on["FasterRCNN"] == parent["FasterRCNN"]
    assert set(on["FasterRCNN_BNAdapt"]) == set(sizes)
    assert all(set(r) == {"mAP50_95", "mAP50", "per_class_ap50"} for r in on["FasterRCNN_BNAdapt"].values())
    rows = (tmp_path / "on/eval_results.csv").read_text().splitlines()
    assert [r.split(",")[0] for r in rows[1:5]] == ["FasterRCNN", "FasterRCNN", "FasterRCNN_BNAdapt", "FasterRCNN_BNAdapt"]
    assert [r for r in rows if r.startswith("FasterRCNN,")] == [r for r in off_csv.decode().splitlines()
                                                                 if r.startswith("FasterRCNN,")]
