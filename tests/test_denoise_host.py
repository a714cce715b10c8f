"""The non-local-means denoiser, the parts that need no GPU (include/mx_det.h mx_denoise_nlm_u8; mx_det.denoise;
tests/denoise_ref.py):
  * the entries are bound, the descriptor has the declared layout, every bad argument is refused before any
    launch with a message, and an empty batch returns;
  * the weight table: the library's, the restatement's literals and round(4096 * exp(-i / 16)) are the same;
  * denoise.params equals a hand-computed case and honours the rule and the verdict;
  * the restatement: 3 x 3 images worked by hand, a constant image is a fixed point;
  * quality: on the six content images under sigma 15 noise the noise rule fires on every noisy image and on
    no clean one, and the blind denoiser gains at least 3 dB PSNR on each;
  * MX_RESTORE_DENOISE parses, is refused without the gate, and with it unset the scripts build what they
    built before."""
import ctypes
import math

import numpy as np
import pytest

import denoise_ref as ref
import gate_ref

FAKE = 0x10000000  # device addresses that are never dereferenced: every case below is refused first
STATS, VERDICT, APPLIED = FAKE + (8 << 24), FAKE + (9 << 24), FAKE + (10 << 24)


def _lib():
    from mx_det import _lib
    return _lib


def desc(k=0, **kw):
    d = dict(src=FAKE + (2 * k << 24), dst=FAKE + (2 * k + 1 << 24), H=20, W=30, bgr=0, sigma_q8=2560)
    d.update(kw)
    return d


def _call(descs, stats=STATS, verdict=None, a=10, b=383, k16=6, applied=APPLIED):
    """(rc, message) of mx_denoise_nlm_u8 on a list of field dicts."""
    L = _lib()
    lib = L.load()
    arr = (L.NlmDesc * max(len(descs), 1))()
    for d, f in zip(arr, descs):
        for k, v in f.items():
            setattr(d, k, v)
    rc = lib.mx_denoise_nlm_u8(arr, len(descs), stats, verdict, a, b, k16, applied, None)
    return rc, lib.mx_last_error().decode()


def test_entries_are_bound():
    L = _lib()
    names = {"mx_denoise_nlm_u8", "mx_denoise_nlm_tile", "mx_denoise_nlm_lut"}
    assert names <= set(L.declared_symbols())
    lib = L.load()
    assert all(hasattr(lib, n) for n in names)
    # two pointers, then H, W, bgr, sigma_q8
    assert ctypes.sizeof(L.NlmDesc) == 32
    assert [getattr(L.NlmDesc, f).offset for f in ("src", "dst", "H", "W", "bgr", "sigma_q8")] == [0, 8, 16, 20, 24, 28]
    tile = (ctypes.c_int32 * 2)()
    assert lib.mx_denoise_nlm_tile(tile) == 0 and tile[0] >= 1 and tile[1] >= 1
    assert lib.mx_denoise_nlm_tile(None) == -1 and "null output" in lib.mx_last_error().decode()
    assert lib.mx_denoise_nlm_lut(None) == -1 and "null output" in lib.mx_last_error().decode()
    from mx_det import ops
    assert ops.denoise_nlm_tile() == (tile[0], tile[1])


def test_an_empty_batch_returns_zero():
    assert _call([])[0] == 0
    assert _call([], stats=None, applied=None)[0] == 0
    L = _lib()
    assert L.load().mx_denoise_nlm_u8(None, 0, None, None, 10, 383, 6, None, None) == 0


@pytest.mark.parametrize("fields, word", [
    (dict(src=None), "null image"),
    (dict(dst=None), "null image"),
    (dict(H=0), "bad size"),
    (dict(W=0), "bad size"),
    (dict(W=-5), "bad size"),
    (dict(H=4097, W=4096), "bad size"),      # H * W = 2^24 + 4096
    (dict(H=1, W=(1 << 24) + 1), "bad size"),
    (dict(sigma_q8=-1), "sigma_q8"),
    (dict(sigma_q8=65536), "sigma_q8"),
    (dict(sigma_q8=0, H=2), "no stats"),     # a blind image needs the gate's sums, which need 3 x 3
    (dict(sigma_q8=0, W=2), "no stats"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_bad_images_are_refused_before_any_launch(fields, word):
    """No GPU is needed: the refusal comes before the first HIP call. The bad image is the last of three."""
    rc, msg = _call([desc(0), desc(1, H=1, W=1), desc(2, **fields)])
    assert rc == -1, (rc, msg)
    assert "mx_denoise_nlm_u8" in msg and "image 2" in msg and word in msg, msg


def test_other_bad_arguments_are_refused():
    L = _lib()
    lib = L.load()
    rc, msg = _call([desc(0), desc(1, sigma_q8=0)], stats=None)
    assert rc == -1 and "image 1" in msg and "without stats" in msg, msg
    for k16 in (0, 65, -1):
        rc, msg = _call([desc()], k16=k16)
        assert rc == -1 and "k16" in msg, msg
    for a, b in ((-1, 1), (65536, 1), (1, -1), (1, 65536)):
        rc, msg = _call([desc()], a=a, b=b)
        assert rc == -1 and "rule coefficient" in msg, msg
    rc = lib.mx_denoise_nlm_u8(None, 1, STATS, None, 10, 383, 6, APPLIED, None)
    assert rc == -1 and "descriptor" in lib.mx_last_error().decode()
    rc = lib.mx_denoise_nlm_u8(None, -1, STATS, None, 10, 383, 6, APPLIED, None)
    assert rc == -1 and "descriptor" in lib.mx_last_error().decode()


@pytest.mark.parametrize("src, dst, h, w", [
    (FAKE, FAKE, 20, 30),                       # in place
    (FAKE, FAKE + 20 * 30 * 3 - 1, 20, 30),     # the last byte of src
    (FAKE + 20 * 30 * 3 - 1, FAKE, 20, 30),     # the last byte of dst
    (FAKE, FAKE + 1, 1, 1),
])
def test_overlap_of_dst_and_src_is_refused(src, dst, h, w):
    rc, msg = _call([desc(1), desc(0, src=src, dst=dst, H=h, W=w)])
    assert rc == -1 and "image 1" in msg and "overlaps" in msg, msg


def test_overlap_with_another_images_src_is_refused():
    a = desc(0)
    rc, msg = _call([a, desc(1, dst=a["src"] + 100)])
    assert rc == -1 and "image 1: dst overlaps the src of image 0" in msg, msg


def test_the_three_tables_are_the_same():
    from mx_det import ops
    lut = ops.denoise_nlm_lut()
    assert len(lut) == 128 and lut == list(ref.LUT)
    assert lut == [int(round(4096 * math.exp(-i / 16))) for i in range(128)]
    assert lut[0] == 4096 and lut[127] == 1 and all(a >= b for a, b in zip(lut, lut[1:]))


# ---------------------------------------------------------------------------------------------
def test_params_by_hand():
    from mx_det import denoise
    # N = 1000, IMM = 48000: a = (48000 << 8) / 1000 = 12288 (48 grey levels in 1/256); s8 = 12288 * 13689 >> 16
    # = 168210432 >> 16 = 2566 (10.02 grey levels); T0 = 50 * 2566^2 >> 16 = 329217800 >> 16 = 5023;
    # D = 25 * 36 * 2566^2 >> 24 = 5925920400 >> 24 = 353; Q = 16777216 / 353 = 47527
    row = [1000, 48000, 0, 0, 0, 0, 0, 0]
    assert 12288 * 13689 == 168210432 and 2566 * 2566 == 6584356
    want = (True, 2566, 5023, 353, 47527)
    assert denoise.params(row) == want == ref.params(row)
    # the rule: 10 * IMM > 383 * N; 38300 is the boundary and does not fire
    assert denoise.params([1000, 38300] + [0] * 6)[0] is False and denoise.params([1000, 38301] + [0] * 6)[0] is True
    assert denoise.params(row, rule=(1, 48))[0] is False and denoise.params(row, rule=(1, 47))[0] is True
    assert denoise.params(row, rule=(0, 0))[0] is False
    # the verdict: anything but 0 leaves the image alone; the numbers stay
    assert denoise.params(row, verdict=1) == (False,) + want[1:] == ref.params(row, verdict=1)
    assert denoise.params(row, verdict=0) == want
    # an explicit sigma: no stats, no rule
    assert denoise.params(None, sigma_q8=1) == (True, 1, 0, 1, 1 << 24) == ref.params(None, sigma_q8=1)
    assert denoise.params([1000, 0] + [0] * 6, 64, sigma_q8=65535) == (True, 65535, 3276700, 26213600, 0)
    assert denoise.params(None, 64, sigma_q8=65535, verdict=1)[0] is False
    assert denoise.params(row, k16=16)[3] == (25 * 256 * 6584356) >> 24
    # a flat blind image: s8 = 0, D = 1
    assert denoise.params([1000, 0] + [0] * 6) == (False, 0, 0, 1, 1 << 24)
    for bad in (dict(k16=0), dict(k16=65), dict(rule=(-1, 1)), dict(rule=(1, 65536)), dict(sigma_q8=65536), dict(sigma_q8=-1)):
        with pytest.raises(ValueError):
            denoise.params(row, **bad)
    for k in range(8):  # the restatement and the module agree on other rows
        r = [997 + k, 5000 * (k + 1) + 13] + [0] * 6
        assert denoise.params(r, k16=1 + 9 * k) == ref.params(r, k16=1 + 9 * k)


def grey(y):
    return np.repeat(np.asarray(y, np.uint8)[..., None], 3, axis=2)


def test_3x3_images_by_hand():
    # (a) sigma_q8 = 65535, k16 = 64: Q = 0, every weight is 4096, the output is the mean over the 11 x 11
    # window with clamped coordinates. Around the centre of a 3 x 3 image rows and columns 0, 1, 2 are hit
    # 5, 1, 5 times; around a corner 6, 1, 4 times.
    y = np.array([[10, 20, 30], [40, 50, 70], [5, 100, 200]], np.int64)
    out, wsum = ref.nlm(grey(y), 65535, 64, want_wsum=True)
    assert (wsum == 121 * 4096).all()
    m = np.array([5, 1, 5])
    centre = int((m[:, None] * m[None, :] * y).sum())   # rows: 5*10 + 20 + 5*30, 5*40 + 50 + 5*70, 5*5 + 100 + 5*200
    assert centre == 5 * 220 + 600 + 5 * 1125 == 7325
    assert out[1, 1].tolist() == [(7325 + 60) // 121] * 3 == [61] * 3
    c = np.array([6, 1, 4])
    corner = int((c[:, None] * c[None, :] * y).sum())
    assert corner == 6 * 200 + 570 + 4 * 930 == 5490
    assert out[0, 0].tolist() == [(5490 + 60) // 121] * 3 == [45] * 3
    # channels are averaged separately, luma only guides
    img = grey(y)
    img[..., 2] = 255 - img[..., 2]
    out = ref.nlm(img, 65535, 64)
    assert out[1, 1].tolist() == [61, 61, (121 * 255 - 7325 + 60) // 121]
    # (b) sigma_q8 = 1: T0 = 0, D = 1, Q = 2^24, idx = min(16 d, 128): only d < 8 weighs anything. Columns a, b, b
    # with |a - b| = 100: the rows are equal, so d depends on dx alone, and no other column profile equals a
    # pixel's own: the weights are 4096 for dx = 0 (eleven dy) and 0 elsewhere. The edge stays as it is.
    edge = grey([[50, 150, 150]] * 3)
    out, wsum = ref.nlm(edge, 1, want_wsum=True)
    assert np.array_equal(out, edge) and (wsum == 11 * 4096).all()
    # (c) the same with |a - b| = 1: the profiles of column 0 (a a a b b), of its left neighbour by clamping
    # (a a a a b) and of column 1 (a a b b b) differ in one place: d = 5 rows * 1 = 5, idx = 80, w = LUT[80] = 28
    edge1 = grey([[100, 101, 101]] * 3)
    _, wsum = ref.nlm(edge1, 1, want_wsum=True)
    assert ref.LUT[80] == 28 and (wsum[:, 0] == 11 * (4096 + 28 + 28)).all()


def test_a_constant_image_is_a_fixed_point():
    for h, w, v, s8, k16 in ((1, 1, 0, 1, 1), (3, 5, 255, 65535, 6), (12, 9, 137, 2560, 6), (4, 30, 1, 300, 64)):
        img = np.full((h, w, 3), v, np.uint8)
        img[..., 1] = 255 - v
        out, wsum = ref.nlm(img, s8, k16, want_wsum=True)
        assert np.array_equal(out, img) and (wsum == 121 * 4096).all()


def test_quality_on_the_content_images():
    """Blind parameters, k16 = 6, noise sigma 15 per channel. The prototype of this definition gained
    3.76-7.5 dB; a restatement that lands elsewhere has drifted from the definition."""
    from mx_det import gate
    clean = gate_ref.content_images()
    assert len(clean) == 6 and clean[0].shape == (192, 256, 3)
    gains = []
    for i, im in enumerate(clean):
        noisy = np.clip(np.rint(im + np.random.default_rng(500 + i).normal(0, 15, im.shape)), 0, 255).astype(np.uint8)
        row_c, row_n = gate_ref.stats(im), gate_ref.stats(noisy)
        assert ref.params(row_c)[0] is False and ref.params(row_n)[0] is True
        assert gate.decide(row_n, gate.DEFAULT_RULES[:1], 1) == 0 and gate.decide(row_c, gate.DEFAULT_RULES[:1], 1) == 1
        assert 256 < ref.params(row_c)[1] < 512 and 2432 < ref.params(row_n)[1] < 2688   # sigma 1-2 and 9.5-10.5
        out, applied = ref.denoise(noisy, row_n)
        assert applied == 1
        same, zero = ref.denoise(im, row_c)
        assert zero == 0 and np.array_equal(same, im)
        gains.append(ref.psnr(out, im) - ref.psnr(noisy, im))
    print("PSNR gains (dB):", [round(g, 2) for g in gains])
    assert min(gains) >= 3.0, gains


# ---------------------------------------------------------------------------------------------
def test_restore_denoise_variable_parses(monkeypatch):
    from mx_det import denoise
    monkeypatch.delenv("MX_RESTORE_DENOISE", raising=False)
    assert denoise.env_denoise() is None
    for off in ("", "0", " 0 "):
        monkeypatch.setenv("MX_RESTORE_DENOISE", off)
        assert denoise.env_denoise() is None
    monkeypatch.setenv("MX_RESTORE_DENOISE", "nlm")
    d = denoise.env_denoise()
    assert isinstance(d, denoise.NLMDenoiser) and (d.k16, d.rule, d.bgr) == (6, (10, 383), False)
    monkeypatch.setenv("MX_RESTORE_DENOISE", " nlm:9 ")
    assert denoise.env_denoise().k16 == 9
    assert denoise.env_denoise("nlm:64").k16 == 64
    for bad in ("1", "auto", "nlm:", "nlm:0", "nlm:65", "nlm:x", "nlm:-3", "nlm:6:1", "bm3d", "NLM"):
        with pytest.raises(ValueError, match="MX_RESTORE_DENOISE"):
            denoise.env_denoise(bad)
    for bad in (dict(k16=0), dict(k16=6.0), dict(rule=(1, 70000)), dict(rule=(True, 1))):
        with pytest.raises(ValueError):
            denoise.NLMDenoiser(**bad)


class _Unet:
    def to(self, dev):
        return self

    def eval(self):
        return self


def _no_models(monkeypatch, tmp_path):
    from scripts import eval_all, eval_restored
    unet, calls, saved, loaded = _Unet(), [], [], []
    monkeypatch.setattr(eval_all, "init_device", lambda: ("dev", 1, 0))
    monkeypatch.setattr(eval_restored, "load_unet", lambda dev: loaded.append(dev) or unet)
    monkeypatch.setattr(eval_all, "save_json", lambda results, path: saved.append(str(path)))
    monkeypatch.setattr(eval_all, "eval_model", lambda *a, **kw: calls.append((a, kw)) or {})
    monkeypatch.setattr(eval_restored, "OUT_DIR", tmp_path)
    return unet, calls, saved, loaded


def test_eval_restored_with_and_without_the_denoiser(monkeypatch, tmp_path):
    from mx_det import denoise, gate
    from scripts import eval_restored
    for name in ("MX_RESTORE_GATE", "MX_RESTORE_DENOISE", "MX_EXTRA_VARIANTS", "MX_SEVERITIES", "MX_BN_ADAPT"):
        monkeypatch.delenv(name, raising=False)
    assert eval_restored.results_name(False) == "eval_restored_results.json"
    assert eval_restored.results_name(True) == "eval_restored_results_fused.json"
    assert eval_restored.results_name(True, True) == "eval_restored_results_gated.json"
    assert eval_restored.results_name(True, True, False) == "eval_restored_results_gated.json"
    assert eval_restored.results_name(True, True, True) == "eval_restored_results_gated_nlm.json"
    assert eval_restored.results_name(True, gated=True, denoised=True) == "eval_restored_results_gated_nlm.json"
    unet, calls, saved, loaded = _no_models(monkeypatch, tmp_path)
    ck = eval_restored.CKPTS["FasterRCNN"]
    # unset: the objects, roots and file names of before
    for on, root, out in (("0", eval_restored.RESTORED_ROOT, "eval_restored_results.json"),
                          ("1", eval_restored.CORRUPTED_ROOT, "eval_restored_results_fused.json")):
        monkeypatch.setenv("MX_RESTORE_ON_DEVICE", on)
        calls.clear(), saved.clear()
        eval_restored.main()
        assert calls == [(("FasterRCNN", ck, "dev"), dict(root=root, restorer=unet if on == "1" else None))]
        assert saved == [str(tmp_path / out)]
    monkeypatch.setenv("MX_RESTORE_GATE", "auto")
    calls.clear(), saved.clear()
    eval_restored.main()
    (a, kw), = calls
    assert isinstance(kw["restorer"], gate.GatedRestorer) and kw["restorer"].denoiser is None
    assert kw["restorer"].take_counts() == {"restored": 0, "passed": 0}
    assert saved == [str(tmp_path / "eval_restored_results_gated.json"), str(tmp_path / "restore_gate_counts.json")]
    # on: a select-mode gate with the denoiser, the _nlm results file
    monkeypatch.setenv("MX_RESTORE_DENOISE", "nlm:8")
    calls.clear(), saved.clear()
    eval_restored.main()
    (a, kw), = calls
    r = kw["restorer"]
    assert isinstance(r, gate.GatedRestorer) and r.mode == "select" and r.unet is unet
    assert isinstance(r.denoiser, denoise.NLMDenoiser) and r.denoiser.k16 == 8
    assert r.take_counts() == {"restored": 0, "passed": 0, "denoised": 0}
    assert kw["restore_clean"] is True and kw["counts"] == {} and kw["root"] == eval_restored.CORRUPTED_ROOT
    assert saved == [str(tmp_path / "eval_restored_results_gated_nlm.json"), str(tmp_path / "restore_gate_counts.json")]
    # refused before any model loads: without the gate, without the device path, or misspelt
    for gate_v, on, dn in (("0", "1", "nlm"), (None, "1", "nlm"), ("auto", "0", "nlm"), ("auto", "1", "nlmeans")):
        if gate_v is None:
            monkeypatch.delenv("MX_RESTORE_GATE")
        else:
            monkeypatch.setenv("MX_RESTORE_GATE", gate_v)
        monkeypatch.setenv("MX_RESTORE_ON_DEVICE", on)
        monkeypatch.setenv("MX_RESTORE_DENOISE", dn)
        calls.clear(), loaded.clear()
        with pytest.raises(ValueError, match="MX_RESTORE_DENOISE"):
            eval_restored.main()
        assert not calls and not loaded


def test_restore_testsets_with_and_without_the_denoiser(monkeypatch):
    from mx_det import denoise, gate
    from scripts import eval_restored, restore_testsets
    for name in ("MX_RESTORE_GATE", "MX_RESTORE_DENOISE", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(name, raising=False)
    unet, calls, loaded = _Unet(), [], []
    monkeypatch.setattr(restore_testsets, "init_device", lambda: ("dev", 1, 0))
    monkeypatch.setattr(eval_restored, "load_unet", lambda dev: loaded.append(dev) or unet)
    monkeypatch.setattr(restore_testsets, "restore_variant", lambda *a, **kw: calls.append((a, kw)))
    monkeypatch.setattr(restore_testsets, "COCO_TESTSET_ROOT", restore_testsets.Path("/nonexistent/coco6"))
    three = ("Test_Noise", "Test_Blur", "Test_LowRes")
    restore_testsets.main()
    assert calls == [((unet, v, "dev"), {}) for v in three]
    calls.clear()
    monkeypatch.setenv("MX_RESTORE_GATE", "auto")
    restore_testsets.main()
    assert all(a[0].denoiser is None and kw == dict(dst_root=restore_testsets.COCO_GATED_ROOT) for a, kw in calls)
    calls.clear()
    monkeypatch.setenv("MX_RESTORE_DENOISE", "nlm")
    restore_testsets.main()
    assert [a[1] for a, _ in calls] == ["Test_Clean"] + list(three)
    assert all(isinstance(a[0], gate.GatedRestorer) and a[0].mode == "skip" and isinstance(a[0].denoiser, denoise.NLMDenoiser)
               for a, _ in calls)
    assert all(kw == dict(dst_root=restore_testsets.COCO_GATED_NLM_ROOT) for _, kw in calls)
    assert str(restore_testsets.COCO_GATED_NLM_ROOT) == "data/testsets/coco6_gated_nlm"
    assert str(restore_testsets.COCO_GATED_ROOT) == "data/testsets/coco6_gated"
    monkeypatch.delenv("MX_RESTORE_GATE")
    calls.clear(), loaded.clear()
    with pytest.raises(ValueError, match="MX_RESTORE_DENOISE"):
        restore_testsets.main()
    assert not calls and not loaded


def test_gated_restorer_counts_without_a_device():
    from mx_det import denoise, gate
    g = gate.GatedRestorer(None, mode="skip")
    g.count([1, 0, 0])
    assert g.take_counts() == {"restored": 1, "passed": 2}
    d = gate.GatedRestorer(None, mode="skip", denoiser=denoise.NLMDenoiser())
    d.count([1, 0, 0, 0], [0, 1, 1, 0])
    assert (d.restored, d.denoised, d.passed) == (1, 2, 1)
    assert d.take_counts() == {"restored": 1, "passed": 1, "denoised": 2}
    assert d.take_counts() == {"restored": 0, "passed": 0, "denoised": 0}
    # the host restatement of the device's decision, as skip mode uses it
    noisy, clean = [1000, 48000] + [0] * 6, [1000, 7000] + [0] * 6
    assert d._denoise_decisions([noisy, clean, noisy], [0, 0, 1]) == [1, 0, 0]
    with pytest.raises(ValueError, match="bgr"):
        gate.GatedRestorer(None, bgr=True, denoiser=denoise.NLMDenoiser())
