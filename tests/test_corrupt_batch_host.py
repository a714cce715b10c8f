"""Severity levels and the batched corruption entry, the parts that need no GPU (include/mx_det.h
mx_corrupt_batch_u8; mx_det.augment SEVERITY / env_severities / severity_variants; the `severities`
parameter of RandomCorruptionGPU and RestorationBatcher):
  * the entry is bound, and refuses every bad descriptor before any launch, with a message;
  * level 3 of every severity row is the module's reference constant;
  * MX_SEVERITIES parsing; the variant names the scripts share;
  * with the device ops stubbed out, the classes at the default severities consume exactly the `random`
    stream of the classes as they stood (restated here), and one more draw per corrupted image otherwise."""
import ctypes
import random

import numpy as np
import pytest
import torch

FAKE = 0x10000000  # a device address that is never dereferenced: every case below is refused first


def _lib():
    from mx_det import _lib
    return _lib


def _call(descs, taps=(), noise=None):
    """(rc, message) of mx_corrupt_batch_u8 on a list of field dicts."""
    L = _lib()
    lib = L.load()
    arr = (L.CorruptDesc * max(len(descs), 1))()
    for d, f in zip(arr, descs):
        for k, v in f.items():
            setattr(d, k, v)
    t = (ctypes.c_float * max(len(taps), 1))(*taps)
    rc = lib.mx_corrupt_batch_u8(arr, len(descs), t, len(taps) // 3, noise, None)
    return rc, lib.mx_last_error().decode()


def desc(**kw):
    d = dict(src=FAKE, dst=FAKE + (1 << 20), H=20, W=30, op=0, sigma=0.0, seed=0, tap_off=0, ntaps=0, nh=0, nw=0)
    d.update(kw)
    return d


def test_entry_is_bound():
    L = _lib()
    assert {"mx_corrupt_batch_u8", "mx_corrupt_batch_tile"} <= set(L.declared_symbols())
    lib = L.load()
    assert hasattr(lib, "mx_corrupt_batch_u8") and hasattr(lib, "mx_corrupt_batch_tile")
    assert ctypes.sizeof(L.CorruptDesc) == 56
    tile = (ctypes.c_int32 * 2)()
    assert lib.mx_corrupt_batch_tile(tile) == 0
    assert tile[0] >= 1 and tile[1] >= 1
    assert _call([])[0] == 0  # an empty batch launches nothing


@pytest.mark.parametrize("fields, taps, word", [
    (dict(op=4), (), "bad op"),
    (dict(op=-1), (), "bad op"),
    (dict(op=3, nh=21, nw=15), (), "low-res size"),
    (dict(op=3, nh=10, nw=0), (), "low-res size"),
    (dict(op=3, nh=10, nw=31), (), "low-res size"),
    (dict(op=2, tap_off=0, ntaps=129), (0.0, 0.0, 1.0) * 129, "128"),
    (dict(op=2, tap_off=0, ntaps=2), (0.0, 0.0, 0.5, 0.0, 16.0, 0.5), "reach"),
    (dict(op=2, tap_off=0, ntaps=2), (-16.0, 0.0, 0.5, 0.0, 1.0, 0.5), "reach"),
    (dict(op=2, tap_off=1, ntaps=2), (0.0, 0.0, 0.5, 0.0, 1.0, 0.5), "outside the table"),
    (dict(op=2, dst=FAKE, ntaps=1), (0.0, 0.0, 1.0), "in place"),
    (dict(op=3, dst=FAKE, nh=10, nw=15), (), "in place"),
    (dict(op=1, dst=FAKE + 7), (), "overlap"),
    (dict(op=0, dst=FAKE - 20 * 30 * 3 + 1), (), "overlap"),
    (dict(op=1, H=0), (), "bad size"),
    (dict(op=1, src=None), (), "null image"),
], ids=lambda v: None)
def test_bad_descriptors_are_refused_before_any_launch(fields, taps, word):
    """No GPU is needed: the refusal comes before the first HIP call. The bad image is the last of three,
    so nothing of the batch may have been launched when it is found."""
    good = [desc(op=0, src=FAKE + (4 << 20), dst=FAKE + (5 << 20)), desc(op=1, src=FAKE + (6 << 20), dst=FAKE + (6 << 20))]
    rc, msg = _call(good + [desc(**fields)], taps)
    assert rc == -1, (rc, msg)
    assert "mx_corrupt_batch_u8" in msg and word in msg, msg


def test_outputs_that_meet_another_image_are_refused():
    a = desc(op=1, src=FAKE, dst=FAKE + (1 << 20))
    rc, msg = _call([a, desc(op=1, src=FAKE + (2 << 20), dst=FAKE + (1 << 20) + 5)])
    assert rc == -1 and "overlap" in msg, msg
    rc, msg = _call([a, desc(op=1, src=FAKE + (1 << 20), dst=FAKE + (3 << 20))])
    assert rc == -1 and "overlaps input" in msg, msg


def test_level_three_is_the_reference_setting():
    from mx_det import augment as A, ops
    assert A.SEVERITY_LEVELS == (1, 2, 3, 4, 5) and A.DEFAULT_SEVERITIES == (3,)
    assert set(A.SEVERITY) == set(A.KINDS)
    assert all(len(row) == 5 for row in A.SEVERITY.values())
    assert A.severity_value("noise", 3) == A.NOISE_SIGMA
    assert A.severity_value("blur", 3) == A.BLUR_KERNEL
    assert A.severity_value("lowres", 3) == A.DOWNSCALE_FACTOR
    assert A.severity_value("jpeg", 3) == A.JPEG_QUALITY
    assert A.SEVERITY["noise"] == (5, 10, 15, 25, 40)
    assert A.SEVERITY["blur"] == (5, 7, 9, 13, 17)
    assert A.SEVERITY["lowres"] == (0.75, 0.625, 0.5, 0.375, 0.25)
    assert A.SEVERITY["jpeg"] == (25, 18, 15, 10, 7)
    assert A.severity_spec("noise", 5) == (ops.CORRUPT_NOISE, 40.0)
    assert A.severity_spec("lowres", 1) == (ops.CORRUPT_LOWRES, 0.75)
    assert A.severity_spec("jpeg", 4) == (ops.CORRUPT_JPEG, 10)
    op, taps = A.severity_spec("blur", 3)
    assert op == ops.CORRUPT_BLUR
    assert taps == A.kernel_taps(A.motion_blur_kernel(A.BLUR_KERNEL, A.BLUR_ANGLE_DEG))
    assert [(dy, dx) for dy, dx, _ in A.severity_spec("blur", 5).param] == [(0, x) for x in range(-8, 9)]
    for bad in (("fog", 3), ("noise", 0), ("noise", 6)):
        with pytest.raises(ValueError):
            A.severity_spec(*bad)


def test_env_severities(monkeypatch):
    from mx_det import augment as A
    monkeypatch.delenv("MX_SEVERITIES", raising=False)
    assert A.env_severities() == (3,)
    monkeypatch.setenv("MX_SEVERITIES", "")
    assert A.env_severities() == (3,)
    monkeypatch.setenv("MX_SEVERITIES", " 1, 3 ,5,")
    assert A.env_severities() == (1, 3, 5)
    assert A.env_severities("2") == (2,)
    assert A.env_severities([4, 5]) == (4, 5)
    assert A.env_severities(1) == (1,)
    for bad in ("0", "6", "1,x", "mild", "2.5", [0], [1.5], []):
        with pytest.raises(ValueError):
            A.env_severities(bad)
    monkeypatch.setenv("MX_SEVERITIES", "7")
    with pytest.raises(ValueError):
        A.env_severities()


def test_severity_variants(monkeypatch):
    from mx_det import augment as A
    monkeypatch.delenv("MX_SEVERITIES", raising=False)
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    assert A.severity_variants() == []
    assert A.severity_variants("3") == []
    got = A.severity_variants("5,1,3,1")
    assert [v[0] for v in got] == ["Test_Noise_s1", "Test_Noise_s5", "Test_Blur_s1", "Test_Blur_s5",
                                   "Test_LowRes_s1", "Test_LowRes_s5"]
    assert [v[1] for v in got] == ["Noise-s1", "Noise-s5", "Blur-s1", "Blur-s5", "LowRes-s1", "LowRes-s5"]
    assert [v[2:] for v in got] == [("noise", 1), ("noise", 5), ("blur", 1), ("blur", 5), ("lowres", 1), ("lowres", 5)]
    assert not any(v[0].endswith("_s3") for v in A.severity_variants("1,2,3,4,5"))
    assert len(A.severity_variants("1,2,3,4,5")) == 12
    monkeypatch.setenv("MX_SEVERITIES", "2")
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "jpeg")
    assert A.severity_variants()[-1] == ("Test_JPEG_s2", "JPEG-s2", "jpeg", 2)
    assert [v[0] for v in A.severity_variants()] == ["Test_Noise_s2", "Test_Blur_s2", "Test_LowRes_s2", "Test_JPEG_s2"]


def test_scripts_enumerate_the_severity_sets(monkeypatch):
    """After the reference's four and the MX_EXTRA_VARIANTS sets; nothing new without the variable."""
    from scripts import eval_all, restore_testsets
    monkeypatch.delenv("MX_SEVERITIES", raising=False)
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    assert eval_all.all_variants() == eval_all.VARIANTS
    assert restore_testsets.variants_to_restore() == restore_testsets.VARIANTS_TO_RESTORE
    monkeypatch.setenv("MX_SEVERITIES", "1,3")
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "jpeg")
    assert eval_all.all_variants() == eval_all.VARIANTS + ["Test_JPEG", "Test_Noise_s1", "Test_Blur_s1",
                                                          "Test_LowRes_s1", "Test_JPEG_s1"]
    assert [eval_all.short(v) for v in eval_all.all_variants()] == [
        "Clean", "Noise", "Blur", "LowRes", "JPEG", "Noise-s1", "Blur-s1", "LowRes-s1", "JPEG-s1"]
    assert restore_testsets.variants_to_restore() == ["Test_Noise", "Test_Blur", "Test_LowRes", "Test_JPEG",
                                                      "Test_Noise_s1", "Test_Blur_s1", "Test_LowRes_s1", "Test_JPEG_s1"]


class Calls:
    """Stands in for the device ops: records the calls, returns its input."""

    def __init__(self, monkeypatch):
        from mx_det import ops
        self.log = []
        monkeypatch.setattr(ops, "corrupt_u8", self.corrupt_u8)
        monkeypatch.setattr(ops, "corrupt_batch_u8", self.corrupt_batch_u8)

    def corrupt_u8(self, images, codes, **kw):
        self.log.append(("corrupt_u8", list(codes), kw))
        return images

    def corrupt_batch_u8(self, images, specs, **kw):
        self.log.append(("corrupt_batch_u8", list(specs), kw))
        return images


def gpu_class_before(img, p, kinds):
    """RandomCorruptionGPU.__call__ before `severities`: its draws from `random`."""
    if random.random() > p:
        return None
    kind = random.choice(["noise", "blur", "lowres"]) if kinds == ("noise", "blur", "lowres") else random.choice(list(kinds))
    return kind, random.getrandbits(63)


@pytest.mark.parametrize("kinds", [("noise", "blur", "lowres"), ("noise", "jpeg")], ids=["default", "jpeg"])
def test_random_corruption_gpu_draws(monkeypatch, kinds):
    from mx_det import augment as A, ops
    calls = Calls(monkeypatch)
    img = torch.zeros((4, 5, 3), dtype=torch.uint8)
    N = 40
    # default severities: the stream and the calls of the class as it stood
    random.seed(7)
    want = [gpu_class_before(img, 0.5, kinds) for _ in range(N)]
    want_state = random.getstate()
    aug = A.RandomCorruptionGPU(p=0.5, kinds=kinds)
    assert aug.severities == (3,)
    random.seed(7)
    for _ in range(N):
        aug(img)
    assert random.getstate() == want_state
    hits = [w for w in want if w is not None]
    assert 0 < len(hits) < N
    assert [c[0] for c in calls.log] == ["corrupt_u8"] * len(hits)
    for (_, codes, kw), (kind, seed) in zip(calls.log, hits):
        assert codes == [A.RandomCorruptionGPU.CODES[kind]]
        assert kw == dict(sigma=A.NOISE_SIGMA, seed=seed, factor=A.DOWNSCALE_FACTOR, quality=A.JPEG_QUALITY,
                          subsampling=A.JPEG_SUBSAMPLING)
    # other severities: one more draw (the level) per corrupted image, after its kind
    levels = (1, 2, 4)
    calls.log.clear()
    random.seed(7)
    want = []
    for _ in range(N):
        if random.random() > 0.5:
            continue
        kind = random.choice(["noise", "blur", "lowres"]) if kinds == A.DEFAULT_KINDS else random.choice(list(kinds))
        level = random.choice(levels)
        want.append((kind, level, random.getrandbits(63)))
    want_state = random.getstate()
    aug = A.RandomCorruptionGPU(p=0.5, kinds=kinds, severities=levels)
    random.seed(7)
    for _ in range(N):
        aug(img)
    assert random.getstate() == want_state
    assert [c[0] for c in calls.log] == ["corrupt_batch_u8"] * len(want)
    for (_, specs, kw), (kind, level, seed) in zip(calls.log, want):
        assert specs == [A.severity_spec(kind, level)] and kw["seed"] == seed
    # a single level other than 3 still draws it
    random.seed(7)
    A.RandomCorruptionGPU(p=1.0, kinds=kinds, severities=(5,))(img)
    got = random.getstate()
    random.seed(7)
    random.random(); A._choice(kinds); random.choice((5,)); random.getrandbits(63)  # noqa: E702
    assert got == random.getstate()
    with pytest.raises(ValueError):
        A.RandomCorruptionGPU(severities=(0,))
    with pytest.raises(ValueError):
        A.RandomCorruptionGPU(severities=())
    assert ops.CORRUPT_JPEG == 4


def test_random_corruption_gpu_batch(monkeypatch):
    """batch(imgs): keep draw, kind, level per frame in order, one seed draw, one call."""
    from mx_det import augment as A
    calls = Calls(monkeypatch)
    imgs = [torch.full((3 + i, 4, 3), i, dtype=torch.uint8) for i in range(9)]
    levels = (1, 5)
    random.seed(3)
    picks = {}
    for i in range(len(imgs)):
        if random.random() > 0.5:
            continue
        kind = random.choice(["noise", "blur", "lowres"])
        picks[i] = A.severity_spec(kind, random.choice(levels))
    seed = random.getrandbits(63)
    want_state = random.getstate()
    assert 0 < len(picks) < len(imgs)
    random.seed(3)
    out = A.RandomCorruptionGPU(p=0.5, severities=levels).batch(imgs)
    assert random.getstate() == want_state
    assert len(calls.log) == 1 and calls.log[0][0] == "corrupt_batch_u8"
    assert calls.log[0][1] == list(picks.values()) and calls.log[0][2]["seed"] == seed
    assert len(out) == len(imgs)
    for i, (o, im) in enumerate(zip(out, imgs)):
        assert o is im  # the stub returns its inputs: kept and corrupted frames both stay in their slots


def batcher_before(B, kinds, NOISE=1, BLUR=2, LOWRES=3):
    """RestorationBatcher.__call__ before `severities`: its draws from `random`."""
    codes = {"noise": 1, "blur": 2, "lowres": 3, "jpeg": 4}
    if kinds == ("noise", "blur", "lowres"):
        c = [random.choice((NOISE, BLUR, LOWRES)) for _ in range(B)]
    else:
        c = [codes[random.choice(list(kinds))] for _ in range(B)]
    return c, random.getrandbits(62)


@pytest.mark.parametrize("kinds", [("noise", "blur", "lowres"), ("blur", "jpeg", "noise")], ids=["default", "jpeg"])
def test_restoration_batcher_draws(monkeypatch, kinds):
    from mx_det import augment as A
    from mx_det.restoration import RestorationBatcher
    calls = Calls(monkeypatch)
    x = torch.from_numpy(np.arange(6 * 4 * 4 * 3, dtype=np.uint8).reshape(6, 4, 4, 3))
    random.seed(11)
    want = [batcher_before(6, kinds) for _ in range(5)]
    want_state = random.getstate()
    bt = RestorationBatcher(torch.device("cpu"), kinds=kinds)
    random.seed(11)
    for _ in range(5):
        cor, clean = bt(x)
        assert cor.shape == (6, 3, 4, 4) and torch.equal(cor, clean)
    assert random.getstate() == want_state
    assert [c[0] for c in calls.log] == ["corrupt_u8"] * 5
    for (_, codes, kw), (c, seed) in zip(calls.log, want):
        assert codes == c
        assert kw == dict(seed=seed, quality=A.JPEG_QUALITY, subsampling=A.JPEG_SUBSAMPLING)
    # other severities: kind then level per patch, then the seed; one batched call
    levels = (1, 2, 3, 4, 5)
    calls.log.clear()
    random.seed(11)
    specs = []
    for _ in range(6):
        kind = random.choice(["noise", "blur", "lowres"]) if kinds == A.DEFAULT_KINDS else random.choice(list(kinds))
        specs.append(A.severity_spec(kind, random.choice(levels)))
    seed = random.getrandbits(62)
    want_state = random.getstate()
    random.seed(11)
    RestorationBatcher(torch.device("cpu"), kinds=kinds, severities=levels)(x)
    assert random.getstate() == want_state
    assert len(calls.log) == 1 and calls.log[0][0] == "corrupt_batch_u8"
    assert calls.log[0][1] == specs and calls.log[0][2]["seed"] == seed
