"""Night, haze and rain, the parts that need no GPU (include/mx_det.h mx_weather_batch_u8; mx_det.augment
WEATHER_KINDS; tests/weather_ref.py):
  * the entries are bound, and every bad descriptor is refused before any launch, with a message;
  * the numpy restatement: Philox's known answers, haze alpha within [lo, hi], rain without heads is the
    identity;
  * the new names parse in MX_CORRUPTIONS / MX_EXTRA_VARIANTS / MX_SEVERITIES, `fog` is still refused;
  * with the variables unset, the kinds, the variant lists and the `random` draws of RandomCorruptionGPU
    and RestorationBatcher are the ones before the kinds existed (restated here), and the scripts
    enumerate the Test_Night / Test_Haze / Test_Rain sets only when asked."""
import ctypes
import random

import numpy as np
import pytest
import torch

import weather_ref as ref

FAKE = 0x10000000  # a device address that is never dereferenced: every case below is refused first
NIGHT, HAZE, RAIN = 1, 2, 3  # mx_weather_desc.op


def _lib():
    from mx_det import _lib
    return _lib


def _call(descs, noise=None):
    """(rc, message) of mx_weather_batch_u8 on a list of field dicts."""
    L = _lib()
    lib = L.load()
    arr = (L.WeatherDesc * max(len(descs), 1))()
    for d, f in zip(arr, descs):
        for k, v in f.items():
            setattr(d, k, v)
    rc = lib.mx_weather_batch_u8(arr, len(descs), noise, None)
    return rc, lib.mx_last_error().decode()


def desc(**kw):
    """A good descriptor of each op's parameters (level 3), 20 x 30, out of place; kw overrides."""
    d = dict(src=FAKE, dst=FAKE + (1 << 20), H=20, W=30, op=NIGHT, seed=5, gain=0.3, shot=0.25, read2=16.0,
             lo=19661, hi=42598, air=235, thr=393, len=17, slant=2, fade=15, beta=150)
    d.update(kw)
    return d


def test_entries_are_bound():
    L = _lib()
    assert {"mx_weather_batch_u8", "mx_weather_batch_tile"} <= set(L.declared_symbols())
    lib = L.load()
    assert hasattr(lib, "mx_weather_batch_u8") and hasattr(lib, "mx_weather_batch_tile")
    # 2 pointers, H, W, op, gain, the 8-byte seed, shot, read2, and 8 int32 parameters
    assert ctypes.sizeof(L.WeatherDesc) == 80
    assert L.WeatherDesc.seed.offset == 32 and L.WeatherDesc.beta.offset == 76
    tile = (ctypes.c_int32 * 2)()
    assert lib.mx_weather_batch_tile(tile) == 0
    assert (tile[0], tile[1]) == (16, 80)
    assert lib.mx_weather_batch_tile(None) == -1
    assert _call([])[0] == 0  # an empty batch launches nothing
    rc, msg = L.load().mx_weather_batch_u8(None, 1, None, None), L.load().mx_last_error().decode()
    assert rc == -1 and "descriptor" in msg


@pytest.mark.parametrize("fields, word", [
    (dict(op=0), "bad op"),
    (dict(op=4), "bad op"),
    (dict(op=-1), "bad op"),
    (dict(src=None), "null image"),
    (dict(dst=None), "null image"),
    (dict(H=0), "bad size"),
    (dict(W=0), "bad size"),
    (dict(H=32769), "bad size"),
    (dict(W=32769), "bad size"),
    (dict(dst=FAKE + 7), "src and dst overlap"),
    (dict(op=HAZE, dst=FAKE - 20 * 30 * 3 + 1), "src and dst overlap"),
    (dict(op=NIGHT, gain=-0.5), "night parameters"),
    (dict(op=NIGHT, shot=float("nan")), "night parameters"),
    (dict(op=NIGHT, shot=-1.0), "night parameters"),
    (dict(op=NIGHT, read2=float("inf")), "night parameters"),
    (dict(op=NIGHT, read2=-4.0), "night parameters"),
    (dict(op=HAZE, lo=-1), "haze parameters"),
    (dict(op=HAZE, lo=30000, hi=29999), "haze parameters"),
    (dict(op=HAZE, hi=65536), "haze parameters"),
    (dict(op=HAZE, air=256), "haze parameters"),
    (dict(op=HAZE, air=-1), "haze parameters"),
    (dict(op=RAIN, thr=-1), "rain parameters"),
    (dict(op=RAIN, thr=65536), "rain parameters"),
    (dict(op=RAIN, len=0), "rain parameters"),
    (dict(op=RAIN, len=33, fade=0), "rain parameters"),
    (dict(op=RAIN, slant=9), "rain parameters"),
    (dict(op=RAIN, slant=-9), "rain parameters"),
    (dict(op=RAIN, fade=-1), "rain parameters"),
    (dict(op=RAIN, len=17, fade=16), "rain parameters"),  # (len - 1) * fade = 256
    (dict(op=RAIN, beta=257), "rain parameters"),
    (dict(op=RAIN, beta=-1), "rain parameters"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_bad_descriptors_are_refused_before_any_launch(fields, word):
    """No GPU is needed: the refusal comes before the first HIP call. The bad image is the last of four,
    so nothing of the batch may have been launched when it is found; the three before it are good, each
    of them in place, which every op allows."""
    good = [desc(op=op, src=FAKE + ((4 + op) << 20), dst=FAKE + ((4 + op) << 20)) for op in (NIGHT, HAZE, RAIN)]
    rc, msg = _call(good + [desc(**fields)])
    assert rc == -1, (rc, msg)
    assert "mx_weather_batch_u8" in msg and "image 3" in msg and word in msg, msg


def test_outputs_that_meet_another_image_are_refused():
    a = desc(op=HAZE, src=FAKE, dst=FAKE + (1 << 20))
    rc, msg = _call([a, desc(op=RAIN, src=FAKE + (2 << 20), dst=FAKE + (1 << 20) + 5)])
    assert rc == -1 and "outputs 0 and 1 overlap" in msg, msg
    rc, msg = _call([a, desc(op=NIGHT, src=FAKE + (1 << 20), dst=FAKE + (3 << 20))])
    assert rc == -1 and "output 0 overlaps input 1" in msg, msg
    # an image in place meets itself only: the refusal names the next image's clash with it
    b = desc(op=RAIN, src=FAKE + (2 << 20), dst=FAKE + (2 << 20))
    rc, msg = _call([b, desc(op=NIGHT, src=FAKE + (2 << 20) + 100, dst=FAKE + (5 << 20))])
    assert rc == -1 and "output 0 overlaps input 1" in msg, msg


def test_philox_known_answers():
    """Random123's known answers for philox4x32-10: counter and key all zero, counter and key all ones."""
    ref.check_known_answers()
    assert [int(v) for v in ref.philox(0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert [int(v) for v in ref.philox(ones, ones, ones, ones, 2 ** 64 - 1)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6,
                                                                                0x6D5451FD]
    # arrays broadcast, element by element the scalar result
    got = ref.philox(np.array([0, ones]), np.array([0, ones]), np.array([0, ones]), np.array([0, ones]), 0)
    assert int(got[0][0]) == 0x6627E8D5 and got[0].dtype == np.uint32


def test_restatement_invariants():
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (300, 90, 3), dtype=np.uint8)
    # haze: alpha within [lo, hi] and not constant; lo == hi is a uniform blend; alpha 0 is the identity
    for lo, hi in ((6554, 22938), (32768, 58982), (0, 65535)):
        a = ref.haze_alpha(300, 530, lo, hi, seed=77)
        assert a.min() >= lo and a.max() <= hi and a.min() < a.max()
    assert (ref.haze_alpha(40, 50, 1234, 1234, seed=1) == 1234).all()
    assert np.array_equal(ref.haze(img, 0, 0, 235, seed=3), img)
    want = ((img.astype(np.int64) * 32768 + 235 * 32768 + 32768) >> 16).astype(np.uint8)
    assert np.array_equal(ref.haze(img, 32768, 32768, 235, seed=3), want)
    # rain: no heads (thr 0) or no weight (beta 0) is the identity; every head lightens, nothing darkens
    assert np.array_equal(ref.rain(img, 0, 17, 2, 15, 150, seed=9), img)
    assert np.array_equal(ref.rain(img, 393, 17, 2, 15, 0, seed=9), img)
    out = ref.rain(img, 393, 17, 2, 15, 150, seed=9)
    assert (out >= img).all() and (out > img).any()
    R = ref.rain_strength(64, 64, 65535, 5, 0, 10, seed=2)  # thr 65535: all heads but 1 in 65536
    assert R.max() == 256 and (R == 256).mean() > 0.99
    # the seed matters, and the same seed repeats
    assert not np.array_equal(ref.rain(img, 393, 17, 2, 15, 150, seed=10), out)
    assert np.array_equal(ref.rain(img, 393, 17, 2, 15, 150, seed=9), out)
    # night with a zero field is the dimmed image, truncated
    z = np.zeros(img.shape, np.float32)
    assert np.array_equal(ref.night(img, 0.5, 0.25, 16.0, z), (img.astype(np.float32) * np.float32(0.5)).astype(np.uint8))


def test_severity_rows_and_specs():
    from mx_det import augment as A, ops
    assert (ops.CORRUPT_NIGHT, ops.CORRUPT_HAZE, ops.CORRUPT_RAIN) == (5, 6, 7)
    assert A.WEATHER_KINDS == ("night", "haze", "rain")
    assert A.KINDS == ("noise", "blur", "lowres", "jpeg", "night", "haze", "rain")
    assert A.DEFAULT_KINDS == ("noise", "blur", "lowres")
    assert A.SEVERITY["night"] == ((0.6, 0.1, 2), (0.45, 0.15, 3), (0.3, 0.25, 4), (0.2, 0.4, 6), (0.12, 0.6, 8))
    assert A.SEVERITY["haze"] == ((0.10, 0.35), (0.20, 0.50), (0.30, 0.65), (0.40, 0.78), (0.50, 0.90))
    assert A.SEVERITY["rain"] == ((131, 9, 110), (262, 13, 130), (393, 17, 150), (590, 23, 170), (786, 31, 190))
    assert A.severity_spec("night", 3) == (ops.CORRUPT_NIGHT, (0.3, 0.25, 16.0))
    assert A.severity_spec("night", 5) == (ops.CORRUPT_NIGHT, (0.12, 0.6, 64.0))
    assert A.severity_spec("haze", 1) == (ops.CORRUPT_HAZE, (6554, 22938, 235))
    assert A.severity_spec("haze", 5) == (ops.CORRUPT_HAZE, (32768, 58982, 235))
    assert A.severity_spec("rain", 1) == (ops.CORRUPT_RAIN, (131, 9, 2, 28, 110))
    assert A.severity_spec("rain", 5) == (ops.CORRUPT_RAIN, (786, 31, 2, 8, 190))
    for kind in A.WEATHER_KINDS:
        for level in A.SEVERITY_LEVELS:
            sp = A.severity_spec(kind, level)
            if kind == "rain":  # within the entry's ranges
                thr, length, slant, fade, beta = sp.param
                assert (length - 1) * fade < 256 and 1 <= length <= 32 and 0 <= beta <= 256
            if kind == "haze":
                assert 0 <= sp.param[0] <= sp.param[1] <= 65535
        with pytest.raises(ValueError):
            A.severity_spec(kind, 0)
        with pytest.raises(ValueError):
            A.severity_spec(kind, 6)
    assert A.RandomCorruptionGPU.CODES["night"] == 5 and A.RandomCorruptionGPU.CODES["rain"] == 7
    assert A.KIND_VARIANTS["haze"] == ("Test_Haze", "Haze") and A.KIND_VARIANTS["jpeg"] == ("Test_JPEG", "JPEG")
    assert A.KIND_VARIANTS["noise"] == ("Test_Noise", "Noise")


def test_fog_is_still_refused(monkeypatch):
    from mx_det import augment as A
    from mx_det.restoration import RestorationBatcher
    from scripts import build_corrupted_testsets as b
    from scripts import eval_all
    monkeypatch.setenv("MX_CORRUPTIONS", "noise,fog")
    with pytest.raises(ValueError):
        A.env_kinds()
    for cls in (A.RandomCorruption, A.RandomCorruptionGPU):
        with pytest.raises(ValueError):
            cls(kinds=("fog",))
        with pytest.raises(ValueError):
            cls(kinds=("night", "fog"))
    with pytest.raises(ValueError):
        RestorationBatcher(torch.device("cpu"), kinds=("fog",))
    with pytest.raises(ValueError):
        A.severity_spec("fog", 3)
    for bad in ("jpeg,fog", "fog", "night,fog", "Night", "noise"):
        monkeypatch.setenv("MX_EXTRA_VARIANTS", bad)
        with pytest.raises(ValueError):
            A.env_extra_variants()
        with pytest.raises(ValueError):
            b.variants()
        with pytest.raises(ValueError):
            eval_all.all_variants()


def test_the_new_names_parse(monkeypatch):
    from mx_det import augment as A
    monkeypatch.setenv("MX_CORRUPTIONS", "noise, night ,haze,rain")
    assert A.env_kinds() == ("noise", "night", "haze", "rain")
    assert A.env_kinds("rain") == ("rain",)
    assert A.env_kinds(["haze", "jpeg"]) == ("haze", "jpeg")
    assert A.RandomCorruption(kinds=("night",)).kinds == ("night",)
    assert A.RandomCorruptionGPU(kinds=A.KINDS).kinds == A.KINDS
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "rain, night")
    assert A.env_extra_variants() == [("Test_Rain", "Rain"), ("Test_Night", "Night")]
    assert A.env_extra_variants("jpeg,haze,haze") == [("Test_JPEG", "JPEG"), ("Test_Haze", "Haze")]
    monkeypatch.setenv("MX_SEVERITIES", "1,3")
    assert A.severity_variants()[-2:] == [("Test_Rain_s1", "Rain-s1", "rain", 1), ("Test_Night_s1", "Night-s1", "night", 1)]
    monkeypatch.delenv("MX_EXTRA_VARIANTS")
    assert [v[0] for v in A.severity_variants()] == ["Test_Noise_s1", "Test_Blur_s1", "Test_LowRes_s1"]


def test_unset_variables_give_the_values_as_they_stood(monkeypatch):
    from mx_det import augment as A
    from scripts import build_corrupted_testsets as b
    from scripts import eval_all, eval_restored, restore_testsets
    for name in ("MX_CORRUPTIONS", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(name, raising=False)
    four = ["Test_Clean", "Test_Noise", "Test_Blur", "Test_LowRes"]
    assert A.env_kinds() == ("noise", "blur", "lowres")
    assert A.env_extra_variants() == [] and A.severity_variants() == [] and A.env_severities() == (3,)
    assert eval_all.all_variants() == four and b.variants() == four and eval_restored.VARIANTS == four
    assert restore_testsets.variants_to_restore() == four[1:]


def test_scripts_enumerate_the_weather_sets_only_when_asked(monkeypatch):
    from scripts import build_corrupted_testsets as b
    from scripts import eval_all, restore_testsets
    monkeypatch.delenv("MX_SEVERITIES", raising=False)
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    weather = ("Night", "Haze", "Rain")
    for vs in (eval_all.all_variants(), b.variants(), restore_testsets.variants_to_restore()):
        assert not any(k in v for v in vs for k in weather)
    monkeypatch.setenv("MX_SEVERITIES", "2,5")  # levels alone add no weather set
    for vs in (eval_all.all_variants(), b.variants(), restore_testsets.variants_to_restore()):
        assert not any(k in v for v in vs for k in weather)
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "night,haze,rain")
    monkeypatch.setenv("MX_SEVERITIES", "3")
    sets = ["Test_Night", "Test_Haze", "Test_Rain"]
    assert eval_all.all_variants() == eval_all.VARIANTS + sets == b.variants()
    assert restore_testsets.variants_to_restore() == restore_testsets.VARIANTS_TO_RESTORE + sets
    monkeypatch.setenv("MX_SEVERITIES", "1,3")
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "haze,rain")
    assert b.variants() == b.VARIANTS + ["Test_Haze", "Test_Rain", "Test_Noise_s1", "Test_Blur_s1", "Test_LowRes_s1",
                                         "Test_Haze_s1", "Test_Rain_s1"] == eval_all.all_variants()
    assert [eval_all.short(v) for v in eval_all.all_variants()] == [
        "Clean", "Noise", "Blur", "LowRes", "Haze", "Rain", "Noise-s1", "Blur-s1", "LowRes-s1", "Haze-s1", "Rain-s1"]
    assert restore_testsets.variants_to_restore()[-2:] == ["Test_Haze_s1", "Test_Rain_s1"]
    # the builder's seeds: fixed by SEED and the index, distinct per image
    assert b.weather_seed(0) == 42 << 32 and b.weather_seed(7) == (42 << 32) + 7


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


def test_default_kinds_consume_the_draws_as_they_stood(monkeypatch):
    """RandomCorruptionGPU and RestorationBatcher at their defaults, against their decision rules before
    the weather kinds, restated: the same calls, the same seeds, the same state of `random`."""
    from mx_det import augment as A
    from mx_det.restoration import RestorationBatcher
    calls = Calls(monkeypatch)
    img = torch.zeros((4, 5, 3), dtype=torch.uint8)
    random.seed(21)
    want = []
    for _ in range(40):
        if random.random() > 0.5:
            continue
        want.append(({"noise": 1, "blur": 2, "lowres": 3}[random.choice(["noise", "blur", "lowres"])], random.getrandbits(63)))
    want_state = random.getstate()
    aug = A.RandomCorruptionGPU(p=0.5)
    random.seed(21)
    for _ in range(40):
        aug(img)
    assert random.getstate() == want_state
    assert [(c[0], c[1], c[2]["seed"]) for c in calls.log] == [("corrupt_u8", [code], seed) for code, seed in want]
    assert len({c[1][0] for c in calls.log}) == 3
    # the batcher
    calls.log.clear()
    x = torch.zeros((6, 4, 4, 3), dtype=torch.uint8)
    random.seed(22)
    want = []
    for _ in range(4):
        codes = [random.choice((1, 2, 3)) for _ in range(6)]
        want.append((codes, random.getrandbits(62)))
    want_state = random.getstate()
    bt = RestorationBatcher(torch.device("cpu"))
    random.seed(22)
    for _ in range(4):
        bt(x)
    assert random.getstate() == want_state
    assert [(c[0], c[1], c[2]) for c in calls.log] == [
        ("corrupt_u8", codes, dict(seed=seed, quality=A.JPEG_QUALITY, subsampling=A.JPEG_SUBSAMPLING)) for codes, seed in want]


@pytest.mark.parametrize("levels", [(3,), (1, 4)], ids=["default-level", "levels"])
def test_weather_kinds_draw_keep_kind_level_seed(monkeypatch, levels):
    """With a weather kind among them: keep draw, a uniform choice of the kinds, the level only when the
    severities are not the default, then the seed; a weather draw is a corrupt_batch_u8 call."""
    from mx_det import augment as A
    from mx_det.restoration import RestorationBatcher
    calls = Calls(monkeypatch)
    kinds = ("noise", "night", "haze", "rain")
    img = torch.zeros((4, 5, 3), dtype=torch.uint8)
    random.seed(31)
    want = []
    for _ in range(40):
        if random.random() > 0.5:
            continue
        kind = random.choice(list(kinds))
        level = 3 if levels == (3,) else random.choice(levels)
        want.append((kind, level, random.getrandbits(63)))
    want_state = random.getstate()
    aug = A.RandomCorruptionGPU(p=0.5, kinds=kinds, severities=levels)
    random.seed(31)
    for _ in range(40):
        aug(img)
    assert random.getstate() == want_state
    assert len(calls.log) == len(want) and {w[0] for w in want} == set(kinds)
    for (name, arg, kw), (kind, level, seed) in zip(calls.log, want):
        assert kw["seed"] == seed
        if levels == (3,) and kind == "noise":
            assert name == "corrupt_u8" and arg == [1]
        else:
            assert name == "corrupt_batch_u8" and arg == [A.severity_spec(kind, level)]
    # batch(): the same rule per frame, one seed, one call
    calls.log.clear()
    random.seed(32)
    picks = []
    for _ in range(9):
        if random.random() > 0.5:
            continue
        kind = random.choice(list(kinds))
        picks.append(A.severity_spec(kind, random.choice(levels)))
    seed = random.getrandbits(63)
    want_state = random.getstate()
    random.seed(32)
    A.RandomCorruptionGPU(p=0.5, kinds=kinds, severities=levels).batch([img] * 9)
    assert random.getstate() == want_state
    assert len(calls.log) == 1 and calls.log[0][0] == "corrupt_batch_u8"
    assert calls.log[0][1] == picks and calls.log[0][2]["seed"] == seed
    # the batcher: kind (then level) per patch, then the seed; one corrupt_batch_u8 call
    calls.log.clear()
    x = torch.zeros((6, 4, 4, 3), dtype=torch.uint8)
    random.seed(33)
    specs = []
    for _ in range(6):
        kind = random.choice(list(kinds))
        specs.append(A.severity_spec(kind, 3 if levels == (3,) else random.choice(levels)))
    seed = random.getrandbits(62)
    want_state = random.getstate()
    random.seed(33)
    cor, clean = RestorationBatcher(torch.device("cpu"), kinds=kinds, severities=levels)(x)
    assert random.getstate() == want_state and cor.shape == (6, 3, 4, 4)
    assert len(calls.log) == 1 and calls.log[0][0] == "corrupt_batch_u8"
    assert calls.log[0][1] == specs and calls.log[0][2]["seed"] == seed


def test_host_chooser_reaches_the_weather_kinds(monkeypatch):
    from mx_det import augment as A
    seen = []
    monkeypatch.setattr(A, "apply_night", lambda img, level=3, seed=None: seen.append(("night", level)))
    monkeypatch.setattr(A, "apply_haze", lambda img, level=3, seed=None: seen.append(("haze", level)))
    monkeypatch.setattr(A, "apply_rain", lambda img, level=3, seed=None: seen.append(("rain", level)))
    for kind in A.WEATHER_KINDS:
        A._apply_random_corruption(None, kinds=(kind,))
    assert seen == [("night", 3), ("haze", 3), ("rain", 3)]
