"""The restoration gate, the parts that need no GPU (include/mx_det.h mx_degradation_stats_u8 and
mx_restore_finish_gated; mx_det.gate; tests/gate_ref.py):
  * the entries are bound, the two structs have the declared layout, and every bad argument is refused
    before any launch, with a message;
  * the numpy restatement: a flat image, a 3 x 3 image worked by hand, rule order and the default;
  * MX_RESTORE_GATE parses (off, auto, a good file, a bad file);
  * with the variable unset the scripts build what they built before the gate existed (restated here);
  * fit_rules puts its thresholds between the classes and raises when they overlap;
  * the condition behind the GPU verdict test, on the CPU: the 24 content images get the expected verdicts
    under the oracle's level-3 noise, blur and low-res."""
import ctypes
import json

import numpy as np
import pytest

import gate_ref as ref

FAKE = 0x10000000  # a device address that is never dereferenced: every case below is refused first


def _lib():
    from mx_det import _lib
    return _lib


def _call(descs, rules=(), default=0, stats=FAKE + (1 << 24), verdict=FAKE + (2 << 24), nrules=None):
    """(rc, message) of mx_degradation_stats_u8 on lists of field dicts / rule tuples."""
    L = _lib()
    lib = L.load()
    arr = (L.GateDesc * max(len(descs), 1))()
    for d, f in zip(arr, descs):
        for k, v in f.items():
            setattr(d, k, v)
    rarr = (L.GateRule * max(len(rules), 1))()
    for d, r in zip(rarr, rules):
        d.i, d.j, d.a, d.b, d.verdict = r
    rc = lib.mx_degradation_stats_u8(arr, len(descs), rarr, len(rules) if nrules is None else nrules, default, stats,
                                     verdict, None)
    return rc, lib.mx_last_error().decode()


def desc(**kw):
    d = dict(src=FAKE, H=20, W=30, bgr=0)
    d.update(kw)
    return d


GOOD_RULE = (1, 0, 10, 383, 0)


def test_entries_are_bound():
    L = _lib()
    names = {"mx_degradation_stats_u8", "mx_degradation_stats_tile", "mx_restore_finish_gated"}
    assert names <= set(L.declared_symbols())
    lib = L.load()
    assert all(hasattr(lib, n) for n in names)
    # a pointer, H, W, bgr (padded to the pointer's alignment); five int32
    assert ctypes.sizeof(L.GateDesc) == 24
    assert (L.GateDesc.src.offset, L.GateDesc.H.offset, L.GateDesc.W.offset, L.GateDesc.bgr.offset) == (0, 8, 12, 16)
    assert ctypes.sizeof(L.GateRule) == 20
    assert [getattr(L.GateRule, f).offset for f in ("i", "j", "a", "b", "verdict")] == [0, 4, 8, 12, 16]
    tile = (ctypes.c_int32 * 2)()
    assert lib.mx_degradation_stats_tile(tile) == 0
    assert tile[0] >= 1 and tile[1] >= 1
    assert lib.mx_degradation_stats_tile(None) == -1
    assert "null output" in lib.mx_last_error().decode()
    from mx_det import ops
    assert ops.degradation_stats_tile() == (tile[0], tile[1])


def test_an_empty_batch_returns_zero():
    assert _call([])[0] == 0
    assert _call([], stats=None, verdict=None)[0] == 0
    assert _call([], rules=[GOOD_RULE])[0] == 0


@pytest.mark.parametrize("fields, word", [
    (dict(src=None), "null image"),
    (dict(H=2), "bad size"),
    (dict(W=2), "bad size"),
    (dict(H=0), "bad size"),
    (dict(W=-5), "bad size"),
    (dict(H=4097, W=4096), "bad size"),      # H * W = 2^24 + 4096
    (dict(H=3, W=5592406), "bad size"),      # 3 * 5592406 = 2^24 + 2
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_bad_images_are_refused_before_any_launch(fields, word):
    """No GPU is needed: the refusal comes before the first HIP call. The bad image is the last of three."""
    rc, msg = _call([desc(), desc(H=4096, W=4096), desc(**fields)], rules=[GOOD_RULE])
    assert rc == -1, (rc, msg)
    assert "mx_degradation_stats_u8" in msg and "image 2" in msg and word in msg, msg


@pytest.mark.parametrize("rule, word", [
    ((8, 0, 1, 1, 0), "sum index"),
    ((-1, 0, 1, 1, 0), "sum index"),
    ((0, 8, 1, 1, 1), "sum index"),
    ((0, -1, 1, 1, 1), "sum index"),
    ((1, 0, 65536, 1, 0), "coefficient"),
    ((1, 0, -1, 1, 0), "coefficient"),
    ((1, 0, 1, 65536, 0), "coefficient"),
    ((1, 0, 1, -1, 0), "coefficient"),
    ((1, 0, 1, 1, 2), "verdict"),
    ((1, 0, 1, 1, -1), "verdict"),
], ids=str)
def test_bad_rules_are_refused_before_any_launch(rule, word):
    rc, msg = _call([desc()], rules=[GOOD_RULE, rule])
    assert rc == -1 and "mx_degradation_stats_u8" in msg and "rule 1" in msg and word in msg, msg


def test_other_bad_arguments_are_refused():
    L = _lib()
    lib = L.load()
    rc, msg = _call([desc()], rules=[GOOD_RULE] * 9)
    assert rc == -1 and "9 rules" in msg, msg
    rc, msg = _call([desc()], rules=[GOOD_RULE] * 8, default=1, stats=None)
    assert rc == -1 and "null stats or verdict" in msg, msg
    rc, msg = _call([desc()], verdict=None)
    assert rc == -1 and "null stats or verdict" in msg, msg
    for bad in (2, -1):
        rc, msg = _call([desc()], default=bad)
        assert rc == -1 and "default verdict" in msg, msg
    rc, msg = _call([desc()], nrules=-1)
    assert rc == -1 and "rules" in msg, msg
    rc = lib.mx_degradation_stats_u8(None, 1, None, 0, 0, FAKE, FAKE, None)
    assert rc == -1 and "descriptor" in lib.mx_last_error().decode()
    rc = lib.mx_degradation_stats_u8((L.GateDesc * 1)(), 1, None, 1, 0, FAKE, FAKE, None)
    assert rc == -1 and "null rule array" in lib.mx_last_error().decode()
    # the pass-through entry: bad sizes and null pointers, before any launch
    assert lib.mx_restore_finish_gated(FAKE, 1, 16, 16, FAKE, 17, 16, FAKE, FAKE, None) == -1
    assert "bad sizes" in lib.mx_last_error().decode()
    assert lib.mx_restore_finish_gated(FAKE, 1, 16, 16, FAKE, 16, 16, None, FAKE, None) == -1
    assert "null pointer" in lib.mx_last_error().decode()
    assert lib.mx_restore_finish_gated(None, 0, 16, 16, None, 16, 16, None, None, None) == 0  # nothing to do


# ---------------------------------------------------------------------------------------------
def test_a_flat_image_gives_n_and_seven_zeros():
    for h, w, bgr in ((3, 3, False), (7, 12, True), (40, 33, False)):
        img = np.full((h, w, 3), 137, np.uint8)
        assert ref.stats(img, bgr) == [(h - 2) * (w - 2), 0, 0, 0, 0, 0, 0, 0]


def test_a_3x3_image_by_hand():
    # grey pixels, so Y = (256 v + 128) >> 8 = v:   10 20 30 / 40 50 70 / 5 100 200
    y = np.array([[10, 20, 30], [40, 50, 70], [5, 100, 200]], np.uint8)
    img = np.repeat(y[..., None], 3, axis=2)
    assert np.array_equal(ref.luma(img), y)
    # corners 10 + 30 + 5 + 200 = 245; edges 20 + 100 + 40 + 70 = 230; |245 - 460 + 200| = 15
    # dx = 70 - 40 = 30, dy = 100 - 20 = 80, dxx = 70 - 100 + 40 = 10, dyy = 100 - 100 + 20 = 20
    assert ref.stats(img) == [1, 15, 900, 6400, 100, 400, 7300, 500]
    # luma weights: R 77, G 150, B 29 of 256, rounded; bgr swaps R and B
    px = np.zeros((3, 3, 3), np.uint8)
    px[1, 1] = (255, 0, 0)
    assert ref.luma(px)[1, 1] == (77 * 255 + 128) >> 8 and ref.luma(px, bgr=True)[1, 1] == (29 * 255 + 128) >> 8
    px[1, 1] = (255, 255, 255)
    assert ref.luma(px)[1, 1] == 255


def test_decide_honours_rule_order_and_the_default():
    from mx_det import gate
    row = [100, 5000, 10, 30, 1, 1, 40, 2]
    first = [(1, 0, 1, 40, 0), (3, 2, 1, 2, 1)]  # both fire: IMM > 40 N, DY2 > 2 DX2
    for decide in (ref.decide, gate.decide):
        assert decide(row, first, 1) == 0
        assert decide(row, first[::-1], 0) == 1
        assert decide(row, [(1, 0, 1, 50, 0)], 1) == 1   # 5000 > 5000 is false: the default
        assert decide(row, [(1, 0, 1, 50, 0)], 0) == 0
        assert decide(row, [], 1) == 1 and decide(row, [], 0) == 0
        assert decide(row, [(0, 0, 0, 0, 1)], 0) == 0    # 0 > 0 never fires
    assert gate.STAT_NAMES == ("N", "IMM", "DX2", "DY2", "DXX2", "DYY2", "G2", "H2")
    assert gate.DEFAULT_VERDICT == 0
    assert [tuple(r)[:5] for r in gate.DEFAULT_RULES] == [(1, 0, 10, 383, 0), (6, 7, 35, 100, 1), (3, 2, 2, 5, 1),
                                                        (2, 3, 2, 5, 1)]
    assert [r.name for r in gate.DEFAULT_RULES] == ["noise", "lowres", "blur-h", "blur-v"]
    f = gate.features([1000, 38300, 100, 250, 10, 25, 350, 35])
    assert abs(f["sigma"] - 1.2533 * 38.3 / 6) < 1e-9 and f["anisotropy"] == 2.5 and f["hf"] == 0.1
    assert len(gate.features([[4, 0, 0, 0, 0, 0, 0, 0]] * 2)) == 2
    for bad in ([(8, 0, 1, 1, 0)], [(0, 0, 65536, 1, 0)], [(0, 0, 1, 1, 2)], [gate.DEFAULT_RULES[0]] * 9):
        with pytest.raises(ValueError):
            gate.check_rules(bad)
    with pytest.raises(ValueError):
        gate.GatedRestorer(None, mode="maybe")


def test_restore_gate_variable_parses(monkeypatch, tmp_path):
    from mx_det import gate
    monkeypatch.delenv("MX_RESTORE_GATE", raising=False)
    assert gate.env_gate() is None and gate.from_env(None) is None
    for off in ("", "0", " 0 "):
        monkeypatch.setenv("MX_RESTORE_GATE", off)
        assert gate.env_gate() is None
    monkeypatch.setenv("MX_RESTORE_GATE", "auto")
    assert gate.env_gate() == (gate.DEFAULT_RULES, 0)
    g = gate.from_env(None, mode="skip")
    assert isinstance(g, gate.GatedRestorer) and g.mode == "skip" and g.rules == gate.DEFAULT_RULES
    good = tmp_path / "gate.json"
    rules = (gate.Rule(1, 0, 7, 300, 0, "noise"), gate.Rule(6, 7, 3, 10, 1, "lowres"))
    gate.save_rules(good, rules, 1)
    monkeypatch.setenv("MX_RESTORE_GATE", str(good))
    assert gate.env_gate() == (rules, 1)
    doc = json.loads(good.read_text())
    assert doc["rules"][0] == {"name": "noise", "lhs": "IMM", "a": 7, "rhs": "N", "b": 300, "verdict": 0}
    bad = tmp_path / "bad.json"
    for text in ("not json", "{}", json.dumps({"rules": [{"lhs": "XYZ", "rhs": "N", "a": 1, "b": 1, "verdict": 0}]}),
                 json.dumps({"rules": [{"lhs": "IMM", "rhs": "N", "a": 70000, "b": 1, "verdict": 0}]}),
                 json.dumps({"rules": [{"lhs": "IMM", "rhs": "N", "a": 1, "b": 1, "verdict": 3}]}),
                 json.dumps({"default_verdict": 2, "rules": []})):
        bad.write_text(text)
        monkeypatch.setenv("MX_RESTORE_GATE", str(bad))
        with pytest.raises(ValueError, match="bad gate rules file"):
            gate.env_gate()
    monkeypatch.setenv("MX_RESTORE_GATE", str(tmp_path / "missing.json"))
    with pytest.raises(ValueError, match="bad gate rules file"):
        gate.env_gate()


class _Unet:
    def to(self, dev):
        return self

    def eval(self):
        return self


def test_with_the_gate_unset_the_scripts_build_what_they_built(monkeypatch, tmp_path):
    """eval_restored and restore_testsets before the gate, restated: the variant lists, the output names,
    the restorer handed on as it is, Test_Clean left alone, the plain _RestoredLoader around a U-Net."""
    from mx_det import engine, gate
    from scripts import eval_all, eval_restored, restore_testsets
    for name in ("MX_RESTORE_GATE", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(name, raising=False)
    four = ["Test_Clean", "Test_Noise", "Test_Blur", "Test_LowRes"]
    assert eval_all.all_variants() == four and restore_testsets.variants_to_restore() == four[1:]
    assert str(restore_testsets.COCO_OUT_ROOT) == "data/testsets/coco6_restored"
    assert eval_restored.results_name(False) == "eval_restored_results.json"
    assert eval_restored.results_name(True) == "eval_restored_results_fused.json"
    assert eval_restored.results_name(True, gated=True) == "eval_restored_results_gated.json"

    unet, calls, saved = _Unet(), [], []
    monkeypatch.setattr(eval_all, "init_device", lambda: ("dev", 1, 0))
    monkeypatch.setattr(eval_restored, "load_unet", lambda dev: unet)
    monkeypatch.setattr(eval_all, "save_json", lambda results, path: saved.append(str(path)))
    monkeypatch.setattr(eval_all, "eval_model", lambda *a, **kw: calls.append((a, kw)) or {})
    monkeypatch.setattr(eval_restored, "OUT_DIR", tmp_path)
    for on, root, out in (("0", eval_restored.RESTORED_ROOT, "eval_restored_results.json"),
                          ("1", eval_restored.CORRUPTED_ROOT, "eval_restored_results_fused.json")):
        monkeypatch.setenv("MX_RESTORE_ON_DEVICE", on)
        calls.clear(), saved.clear()
        eval_restored.main()
        ck = eval_restored.CKPTS["FasterRCNN"]
        assert calls == [(("FasterRCNN", ck, "dev"), dict(root=root, restorer=unet if on == "1" else None))]
        assert saved == [str(tmp_path / out)]
    # the gate on: a GatedRestorer in select mode, every variant, the two gated files
    monkeypatch.setenv("MX_RESTORE_GATE", "auto")
    calls.clear(), saved.clear()
    eval_restored.main()
    (a, kw), = calls
    assert isinstance(kw["restorer"], gate.GatedRestorer) and kw["restorer"].mode == "select" and kw["restorer"].unet is unet
    assert kw["restore_clean"] is True and kw["counts"] == {} and kw["root"] == eval_restored.CORRUPTED_ROOT
    assert saved == [str(tmp_path / "eval_restored_results_gated.json"), str(tmp_path / "restore_gate_counts.json")]
    monkeypatch.setenv("MX_RESTORE_ON_DEVICE", "0")  # the gate needs the device path: ignored without it
    calls.clear(), saved.clear()
    eval_restored.main()
    assert calls[0][1] == dict(root=eval_restored.RESTORED_ROOT, restorer=None)
    monkeypatch.delenv("MX_RESTORE_GATE")

    # eval_model: Test_Clean keeps no restorer unless restore_clean says so
    monkeypatch.undo()
    for name in ("MX_RESTORE_GATE", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(name, raising=False)
    seen = []
    monkeypatch.setattr(eval_all, "load_frcnn_checkpoint", lambda ck, dev: object())
    monkeypatch.setattr(eval_all, "eval_frcnn_variant",
                        lambda model, img_dir, ann, dev, restorer=None: seen.append(restorer) or {"mAP50": 0.0, "mAP50_95": 0.0})
    monkeypatch.setattr(eval_all.torch.cuda, "empty_cache", lambda: None)
    eval_all.eval_model("m", "ck", "dev", restorer=unet)
    assert seen == [None, unet, unet, unet]
    seen.clear()

    class Counting(_Unet):
        n = 0

        def take_counts(self):
            self.n += 1
            return {"restored": self.n, "passed": 0}

    c, counts = Counting(), {}
    eval_all.eval_model("m", "ck", "dev", restorer=c, restore_clean=True, counts=counts)
    assert seen == [c] * 4 and counts == {v: {"restored": k + 1, "passed": 0} for k, v in enumerate(four)}

    # the loader class around a plain U-Net is the one it was
    made = []
    monkeypatch.setattr(engine, "_RestoredLoader", lambda loader, r, dev: made.append(r) or loader)
    monkeypatch.setattr(engine, "evaluate", lambda *a, **k: {})
    monkeypatch.setattr(engine, "DeviceJpegLoader", lambda loader, dev: loader)
    import mx_det.dataset as dataset
    monkeypatch.setattr(dataset, "COCODetectionDataset", lambda *a, **k: [0, 1])
    engine.eval_frcnn_variant(None, "imgs", "ann", "cpu", restorer=unet)
    engine.eval_frcnn_variant(None, "imgs", "ann", "cpu")
    assert made == [unet]


def test_restore_testsets_main_with_and_without_the_gate(monkeypatch):
    from mx_det import gate
    from scripts import eval_restored, restore_testsets
    for name in ("MX_RESTORE_GATE", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(name, raising=False)
    unet, calls = _Unet(), []
    monkeypatch.setattr(restore_testsets, "init_device", lambda: ("dev", 1, 0))
    monkeypatch.setattr(eval_restored, "load_unet", lambda dev: unet)
    monkeypatch.setattr(restore_testsets, "restore_variant", lambda *a, **kw: calls.append((a, kw)))
    monkeypatch.setattr(restore_testsets, "COCO_TESTSET_ROOT", restore_testsets.Path("/nonexistent/coco6"))
    restore_testsets.main()
    assert calls == [((unet, v, "dev"), {}) for v in ("Test_Noise", "Test_Blur", "Test_LowRes")]
    calls.clear()
    monkeypatch.setenv("MX_RESTORE_GATE", "auto")
    restore_testsets.main()
    assert [a[1] for a, _ in calls] == ["Test_Clean", "Test_Noise", "Test_Blur", "Test_LowRes"]
    assert all(isinstance(a[0], gate.GatedRestorer) and a[0].mode == "skip" and a[0].unet is unet for a, _ in calls)
    assert all(kw == dict(dst_root=restore_testsets.COCO_GATED_ROOT) for _, kw in calls)
    assert str(restore_testsets.COCO_GATED_ROOT) == "data/testsets/coco6_gated"


# ---------------------------------------------------------------------------------------------
def _stats_row(n, sigma, ani, hf):
    from mx_det import gate
    imm, dx = int(sigma / gate.SIGMA_SCALE * n), 100000
    dy = int(dx * ani)
    g = dx + dy
    h = int(g * hf)
    return [n, imm, dx, dy, h // 2, h - h // 2, g, h]


def test_fit_rules_thresholds_lie_between_the_classes():
    from mx_det import gate
    table = {"clean": [_stats_row(1000, 1.45, 0.85, 0.98), _stats_row(1000, 5.84, 1.37, 1.26)],
             "noise": [_stats_row(1000, 9.7, 0.88, 1.43), _stats_row(1000, 12.3, 1.19, 2.07)],
             "blur": [_stats_row(1000, 0.34, 3.8, 0.52), _stats_row(1000, 0.75, 7.1, 0.87)],
             "lowres": [_stats_row(1000, 0.26, 0.88, 0.135), _stats_row(1000, 0.55, 1.36, 0.23)]}
    rules, default = gate.fit_rules(table)
    assert default == 0 and [r.name for r in rules] == ["noise", "lowres", "blur-h", "blur-v"]
    assert [(r.i, r.j, r.verdict) for r in rules] == [(1, 0, 0), (6, 7, 1), (3, 2, 1), (2, 3, 1)]
    noise, lowres, blur_h, blur_v = rules
    sigma = noise.b / noise.a * gate.SIGMA_SCALE
    assert 5.84 < sigma < 9.7 and abs(sigma - (5.84 * 9.7) ** 0.5) < 0.05    # the midpoint in log space
    hf = lowres.a / lowres.b
    assert 0.23 < hf < 0.52 and abs(hf - (0.23 * 0.52) ** 0.5) < 0.005
    ani = blur_h.b / blur_h.a
    assert 1.37 < ani < 3.8 and abs(ani - (1.37 * 3.8) ** 0.5) < 0.02
    assert (blur_v.a, blur_v.b) == (blur_h.a, blur_h.b)
    for name, rows in table.items():
        assert [gate.decide(r, rules, default) for r in rows] == [gate.CONDITION_VERDICTS[name]] * 2
    # an extra condition labelled pass may overlap noise (both pass), not blur
    table["night"] = [_stats_row(1000, 11.0, 1.0, 1.5)]
    assert gate.fit_rules(table)[0] == rules
    with pytest.raises(ValueError, match="noise"):
        gate.fit_rules(table, labels={"night": 1})
    table["night"] = [_stats_row(1000, 3.0, 4.0, 1.0)]
    with pytest.raises(ValueError, match="blur"):
        gate.fit_rules(table)
    assert gate.fit_rules(table, labels={"night": 1})[0] == rules


@pytest.mark.parametrize("cond, row", [
    ("noise", (1000, 5.0, 1.0, 1.5)),     # sigma inside clean's range
    ("lowres", (1000, 0.4, 1.0, 0.6)),    # hf inside blur's range
    ("blur", (1000, 0.5, 1.3, 0.7)),      # anisotropy inside clean's range
    ("clean", (1000, 2.0, 0.2, 1.0)),     # 1 / anisotropy = 5: the mirrored blur rule would fire on clean
])
def test_fit_rules_raises_on_overlap(cond, row):
    from mx_det import gate
    table = {"clean": [_stats_row(1000, 1.45, 0.85, 0.98), _stats_row(1000, 5.84, 1.37, 1.26)],
             "noise": [_stats_row(1000, 9.7, 0.88, 1.43)], "blur": [_stats_row(1000, 0.34, 3.8, 0.52)],
             "lowres": [_stats_row(1000, 0.26, 0.88, 0.135)]}
    gate.fit_rules(table)
    table[cond].append(_stats_row(*row))
    with pytest.raises(ValueError, match="overlap"):
        gate.fit_rules(table)
    with pytest.raises(ValueError, match="no rows"):
        gate.fit_rules({k: v for k, v in table.items() if k != "blur"})


def test_fit_script_conditions_and_labels(monkeypatch):
    from scripts import fit_restore_gate as f
    for name in ("MX_EXTRA_VARIANTS", "MX_SEVERITIES", "MX_GATE_LABELS"):
        monkeypatch.delenv(name, raising=False)
    base = [("clean", None, 3), ("noise", "noise", 3), ("blur", "blur", 3), ("lowres", "lowres", 3)]
    assert f.conditions() == base and f.labels(base) == {}
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "jpeg,haze")
    monkeypatch.setenv("MX_SEVERITIES", "1,3")
    conds = f.conditions()
    assert conds == base + [("jpeg", "jpeg", 3), ("haze", "haze", 3), ("noise-s1", "noise", 1), ("blur-s1", "blur", 1),
                            ("lowres-s1", "lowres", 1), ("jpeg-s1", "jpeg", 1), ("haze-s1", "haze", 1)]
    # other levels follow their kind, other kinds pass unless mapped
    assert f.labels(conds) == {"jpeg": 0, "haze": 0, "noise-s1": 0, "blur-s1": 1, "lowres-s1": 1, "jpeg-s1": 0, "haze-s1": 0}
    assert f.labels(conds, "jpeg=1, haze-s1=1")["jpeg"] == 1 and f.labels(conds, "jpeg=1, haze-s1=1")["haze-s1"] == 1
    for bad in ("fog=1", "jpeg=2", "noise=1", "jpeg"):
        with pytest.raises(ValueError, match="MX_GATE_LABELS"):
            f.labels(conds, bad)
    files = [f"{k:03d}.jpg" for k in range(10)]
    assert f.pick(files[::-1], 20) == files and f.pick(files, 5) == files[::2] and f.pick(files, 10) == files
    assert str(f.OUT_PATH) == "experiments/restoration/gate.json"


def test_content_verdicts_on_the_cpu():
    """The 24 cases of the GPU verdict test, with the oracle's restatements of the level-3 corruptions
    (noise sigma 15 from a fixed field, the 1 x 9 motion blur, x0.5 INTER_AREA down and INTER_LINEAR up)."""
    from mx_det import gate
    from oracle import oracle as orc
    imgs = ref.content_images()
    assert len(imgs) == 6 and all(im.shape == (192, 256, 3) and im.dtype == np.uint8 for im in imgs)
    rng = np.random.default_rng(7)
    got, want = [], []
    for im in imgs:
        noise = rng.normal(0, 15, im.shape).astype(np.float32)
        conds = (("clean", im, 0), ("noise", orc.noise_u8(im, noise), 0), ("blur", orc.blur_u8(im), 1),
                 ("lowres", orc.lowres_u8(im, 0.5), 1))
        for name, x, verdict in conds:
            row = ref.stats(x)
            assert gate.decide(row, gate.DEFAULT_RULES, gate.DEFAULT_VERDICT) == ref.decide(row, gate.DEFAULT_RULES, 0)
            got.append(ref.decide(row, gate.DEFAULT_RULES, gate.DEFAULT_VERDICT))
            want.append(verdict)
    assert len(got) == 24 and got == want
