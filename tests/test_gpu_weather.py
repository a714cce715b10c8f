"""Night, haze and rain on the device (include/mx_det.h mx_weather_batch_u8; mx_det.ops.weather_batch_u8,
ops.corrupt_batch_u8; mx_det.augment) against the numpy restatement of their definitions
(tests/weather_ref.py). Every comparison but one is equality:
  * each op at sizes around the 16 x 80 output tile and across a 256-cell column and row of the haze
    lattice; all five levels; rain at both extreme slants and the longest streak;
  * 17 frames of different sizes and mixed ops in one call (two chunks), image by image against the call
    for that image alone; in place; the seed rule;
  * ops.corrupt_batch_u8 with all seven kinds in one batch, image by image against its own single call;
  * the Python layer: apply_night / apply_haze / apply_rain, RandomCorruptionGPU.batch, the builder.
The exception is night from the device generator, whose normals cannot be matched bit for bit: its sample
mean and variance are compared with the restatement's under a numpy normal field, within six standard
errors."""
import functools
import random

import numpy as np
import pytest
import torch

import weather_ref as ref

pytestmark = pytest.mark.gpu

STEP = 0x9E3779B97F4A7C15
M64 = 2 ** 64 - 1
# 1 x 1; one exact tile; one past it both ways; several tiles; across a 256-cell column; across a 256-cell
# row with a row start that is no multiple of 4
SIZES = ((1, 1), (16, 80), (17, 81), (33, 161), (40, 257), (300, 90))


@functools.lru_cache(maxsize=None)
def image(H, W, salt=0):
    """Uniform random bytes; computed once, read-only."""
    img = np.random.default_rng(1000003 * salt + 4099 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def field(H, W, salt=0):
    """A standard normal f32 field like image(H, W); computed once, read-only."""
    f = np.random.default_rng(7 + 1000003 * salt + 4099 * H + W).standard_normal((H, W, 3)).astype(np.float32)
    f.setflags(write=False)
    return f


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def same(got, want, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:6].tolist(), got[tuple(bad[:6].T)], want[tuple(bad[:6].T)])


def spec(kind, level):
    from mx_det import augment as A
    return A.severity_spec(kind, level)


def test_tile():
    from mx_det import ops
    assert ops.weather_batch_tile() == (16, 80) == ops.corrupt_batch_tile()


@pytest.mark.parametrize("params", [(0.3, 0.25, 16.0), (1.5, 0.5, 9.0), (0.0, 0.0, 0.0)], ids=["level3", "bright", "zero"])
def test_night_with_an_explicit_field_equals_the_restatement(dev, params):
    """`bright` clips at 255 and, with the field's negative tail on dark pixels, at 0."""
    from mx_det import ops
    imgs = [image(h, w) for h, w in SIZES]
    fields = [field(h, w) for h, w in SIZES]
    got = ops.weather_batch_u8([to_dev(im, dev) for im in imgs], [(ops.CORRUPT_NIGHT, params)] * len(imgs), seed=1,
                               noise=[to_dev(f, dev) for f in fields])
    for im, f, g in zip(imgs, fields, got):
        want = ref.night(im, *params, f)
        same(g, want, im.shape)
    if params[0] == 1.5:
        big = ref.night(imgs[-1], *params, fields[-1])
        assert (big == 255).any() and (big == 0).any()


@pytest.mark.parametrize("kind", ["haze", "rain"])
def test_haze_and_rain_equal_the_restatement(dev, kind):
    from mx_det import ops
    sp = spec(kind, 3)
    imgs = [image(h, w) for h, w in SIZES]
    seed = 0xFEDCBA9876543210
    got = ops.weather_batch_u8([to_dev(im, dev) for im in imgs], [sp] * len(imgs), seed=seed)
    for b, (im, g) in enumerate(zip(imgs, got)):
        want = ref.apply(im, sp, (seed + STEP * b) & M64)
        same(g, want, (kind, im.shape))
    assert (got[-1].cpu().numpy() != imgs[-1]).any()


@pytest.mark.parametrize("kind", ["night", "haze", "rain"])
def test_all_five_levels(dev, kind):
    from mx_det import ops
    im, f = image(33, 161, salt=2), field(33, 161, salt=2)
    x = torch.stack([to_dev(im, dev)] * 5)
    specs = [spec(kind, lv) for lv in (1, 2, 3, 4, 5)]
    noise = torch.stack([to_dev(f, dev)] * 5) if kind == "night" else None
    got = ops.weather_batch_u8(x, specs, seed=99, noise=noise)
    assert got.shape == x.shape and got.dtype == torch.uint8
    outs = []
    for b, sp in enumerate(specs):
        want = ref.apply(im, sp, (99 + STEP * b) & M64, f)
        same(got[b], want, (kind, b + 1))
        outs.append(want)
    assert all((outs[b] != outs[b + 1]).any() for b in range(4))


@pytest.mark.parametrize("slant", [-8, 0, 8])
def test_rain_at_the_longest_streak_and_extreme_slants(dev, slant):
    """len 32 at slant +-8 reaches 31 columns to one side of the tile and 31 rows below it."""
    from mx_det import ops
    sp = (ops.CORRUPT_RAIN, (786, 32, slant, 8, 256))
    hw = ((33, 161), (16, 80), (5, 3))
    imgs = [image(h, w, salt=3) for h, w in hw]
    got = ops.weather_batch_u8([to_dev(im, dev) for im in imgs], [sp] * len(imgs), seed=4242)
    for b, (im, g) in enumerate(zip(imgs, got)):
        same(g, ref.apply(im, sp, (4242 + STEP * b) & M64), (slant, im.shape))


def seventeen(dev):
    """17 frames, all of different sizes, the three ops in turn at rotating levels: two chunks."""
    from mx_det import ops
    hw = [(1 + 7 * b % 40, 1 + 23 * b % 170) for b in range(17)]
    assert len(set(hw)) == 17
    kinds = ("night", "haze", "rain")
    specs = [spec(kinds[b % 3], 1 + b % 5) for b in range(17)]
    assert {int(s.op) for s in specs} == {ops.CORRUPT_NIGHT, ops.CORRUPT_HAZE, ops.CORRUPT_RAIN}
    return [image(h, w, salt=5) for h, w in hw], specs


def test_seventeen_frames_in_one_call_equal_each_alone(dev):
    from mx_det import ops
    imgs, specs = seventeen(dev)
    xs = [to_dev(im, dev) for im in imgs]
    fields = [field(*im.shape[:2], salt=5) for im in imgs]
    seed = 31337
    got = ops.weather_batch_u8(xs, specs, seed=seed, noise=[to_dev(f, dev) for f in fields])
    assert isinstance(got, list) and [g.shape for g in got] == [x.shape for x in xs]
    for b, (x, sp, f) in enumerate(zip(xs, specs, fields)):
        sb = (seed + STEP * b) & M64
        same(got[b], ops.weather_batch_u8([x], [sp], seed=sb, noise=[to_dev(f, dev)])[0], b)
        same(got[b], ref.apply(imgs[b], sp, sb, f), b)
    # from the device generator: image b is the single call with seed + STEP * b, and the same seed repeats
    got = ops.weather_batch_u8(xs, specs, seed=seed)
    again = ops.weather_batch_u8(xs, specs, seed=seed)
    other = ops.weather_batch_u8(xs, specs, seed=seed + 1)
    for b, (x, sp) in enumerate(zip(xs, specs)):
        same(got[b], again[b], b)
        same(got[b], ops.weather_batch_u8([x], [sp], seed=(seed + STEP * b) & M64)[0], b)
    assert sum(bool((g != o).any()) for g, o in zip(got, other)) >= 15  # all but the tiniest frames differ


def test_in_place_equals_out_of_place(dev):
    from mx_det import ops
    x = torch.stack([to_dev(image(34, 162, salt=6 + b), dev) for b in range(6)])
    specs = [spec(k, lv) for k, lv in (("night", 2), ("haze", 2), ("rain", 2), ("night", 5), ("haze", 5), ("rain", 5))]
    want = ops.weather_batch_u8(x, specs, seed=8)
    assert all((want[b] != x[b]).any() for b in range(6))
    y = x.clone()
    assert ops.weather_batch_u8(y, specs, seed=8, out=y) is y
    same(y, want)
    frames = [x[b].clone() for b in range(6)]
    got = ops.weather_batch_u8(frames, specs, seed=8, out=frames)
    assert all(g is f for g, f in zip(got, frames))
    for b in range(6):
        same(frames[b], want[b], b)
    out = torch.full_like(x, 0xA5)
    assert ops.weather_batch_u8(x, specs, seed=8, out=out) is out
    same(out, want)
    # outputs that meet another image are refused, and nothing is written
    with pytest.raises(RuntimeError, match="overlap"):
        ops.weather_batch_u8([x[0], x[1]], specs[:2], out=[y[2], y[2]])
    same(y, want)
    with pytest.raises(RuntimeError, match="night, haze or rain"):
        ops.weather_batch_u8(x[:1], [(ops.CORRUPT_NOISE, 5.0)])


def test_night_from_the_device_generator(dev):
    """A constant 64 x 64 image (v = 200) at level 3: d = 60, s = sqrt(0.25 * 60 + 16). The device's
    normals are Box-Muller over Philox in f32 and cannot be matched bit for bit; the output's sample mean
    and variance are compared with those of the restatement under a numpy normal field of the same size.
    Both are samples of n = 64 * 64 * 3 independent values of one distribution with variance var (the
    truncation to uint8 included): the difference of two sample means has standard error sqrt(2 var / n),
    the difference of two sample variances of a near-normal variable sqrt(2 * 2 var^2 / (n - 1)). The
    bound is six of those."""
    from mx_det import ops
    img = np.full((64, 64, 3), 200, dtype=np.uint8)
    sp = spec("night", 3)
    want = ref.night(img, *sp.param, np.random.default_rng(2024).standard_normal(img.shape)).astype(np.float64)
    got = ops.weather_batch_u8([to_dev(img, dev)], [sp], seed=20240607)[0].cpu().numpy().astype(np.float64)
    n = img.size
    var = want.var(ddof=1)
    assert 25.0 < var < 40.0  # s^2 = 31 plus the truncation's 1/12
    se_mean, se_var = np.sqrt(2 * var / n), np.sqrt(4 * var * var / (n - 1))
    print(f"night generator: mean {got.mean():.4f} vs {want.mean():.4f} (6 se = {6 * se_mean:.4f}), "
          f"var {got.var(ddof=1):.4f} vs {var:.4f} (6 se = {6 * se_var:.4f})")
    assert abs(got.mean() - want.mean()) <= 6 * se_mean
    assert abs(got.var(ddof=1) - var) <= 6 * se_var


def test_corrupt_batch_with_all_seven_kinds(dev):
    """Each image gets the bits of its own single call, with and without an explicit noise field (noise and
    night read their own slices of it)."""
    from mx_det import augment as A, ops
    kinds = ("noise", "blur", "lowres", "jpeg", "night", "haze", "rain", "haze", "noise")
    levels = (2, 4, 3, 1, 4, 2, 5, 3, 5)
    x = torch.stack([to_dev(image(34, 162, salt=30 + b), dev) for b in range(len(kinds))])
    specs = [A.severity_spec(k, lv) for k, lv in zip(kinds, levels)]
    seed = 0x1234567890ABCDEF

    def alone(b, noise=None):
        sb = (seed + STEP * b) & M64
        if kinds[b] in A.WEATHER_KINDS:
            return ops.weather_batch_u8(x[b:b + 1], [specs[b]], seed=sb, noise=noise)[0]
        return ops.corrupt_batch_u8(x[b:b + 1], [specs[b]], seed=sb, noise=noise)[0]

    got = ops.corrupt_batch_u8(x, specs, seed=seed)
    assert got.shape == x.shape
    for b in range(len(kinds)):
        same(got[b], alone(b), (b, kinds[b]))
        assert (got[b] != x[b]).any()
    same(got[5], ref.apply(image(34, 162, salt=35), specs[5], (seed + STEP * 5) & M64), "haze")
    fields = torch.stack([to_dev(field(34, 162, salt=30 + b), dev) for b in range(len(kinds))])
    fields[0] *= 10.0
    got = ops.corrupt_batch_u8(x, specs, seed=seed, noise=fields)
    for b in range(len(kinds)):
        same(got[b], alone(b, fields[b:b + 1]), (b, kinds[b], "field"))
    same(got[4], ref.night(image(34, 162, salt=34), *specs[4].param, field(34, 162, salt=34)), "night")
    # frames of several sizes, as a list, weather kinds only and mixed
    hw = ((20, 33), (61, 87), (16, 80), (35, 200))
    xs = [to_dev(image(h, w, salt=40), dev) for h, w in hw]
    for ks in (("rain", "night", "haze", "rain"), ("blur", "rain", "lowres", "night")):
        sps = [A.severity_spec(k, 3) for k in ks]
        got = ops.corrupt_batch_u8(xs, sps, seed=77)
        for b, (xb, sp, k) in enumerate(zip(xs, sps, ks)):
            fn = ops.weather_batch_u8 if k in A.WEATHER_KINDS else ops.corrupt_batch_u8
            same(got[b], fn([xb], [sp], seed=(77 + STEP * b) & M64)[0], (ks, b))


@pytest.mark.parametrize("level", [2, 4])
def test_apply_functions_and_the_batch_class(dev, level):
    from mx_det import augment as A, ops
    img = np.array(image(61, 87, salt=50))
    same(A.apply_haze(img, level, seed=123), ref.apply(img, spec("haze", level), 123), "haze")
    same(A.apply_rain(img, level, seed=456), ref.apply(img, spec("rain", level), 456), "rain")
    night = A.apply_night(img, level, seed=789)
    assert night.shape == img.shape and night.dtype == np.uint8 and night.mean() < img.mean()
    same(night, A.apply_night(img, level, seed=789), "night repeats")
    random.seed(5)
    want_seed = random.getrandbits(63)
    random.seed(5)
    same(A.apply_rain(img, level), ref.apply(img, spec("rain", level), want_seed), "seed=None")
    # RandomCorruptionGPU.batch: every frame corrupted (p = 1), the draws restated
    frames = [to_dev(image(20 + 3 * i, 50 + 11 * i, salt=51), dev) for i in range(5)]
    levels = (level, 3)
    random.seed(60)
    draws = []
    for _ in frames:
        random.random()
        kind = random.choice(list(A.WEATHER_KINDS))
        draws.append((kind, random.choice(levels)))
    seed = random.getrandbits(63)
    random.seed(60)
    out = A.RandomCorruptionGPU(p=1.0, kinds=A.WEATHER_KINDS, severities=levels).batch(frames)
    for b, ((kind, lv), f, o) in enumerate(zip(draws, frames, out)):
        sb = (seed + STEP * b) & M64
        if kind == "night":
            same(o, ops.weather_batch_u8([f], [spec(kind, lv)], seed=sb)[0], (b, kind))
        else:
            same(o, ref.apply(f.cpu().numpy(), spec(kind, lv), sb), (b, kind))
    # a single frame through __call__ at the default severities: level 3
    random.seed(61)
    random.random()
    kind = random.choice(["haze", "rain"])
    seed = random.getrandbits(63)
    random.seed(61)
    got = A.RandomCorruptionGPU(p=1.0, kinds=("haze", "rain"))(frames[0])
    same(got, ref.apply(frames[0].cpu().numpy(), spec(kind, 3), seed), kind)


def test_builder_writes_the_weather_sets(dev, tmp_path, monkeypatch):
    """Test_Haze / Test_Rain after the reference's four, which keep their bytes; each image seeded by its
    index in the sorted listing, so a second build writes the same files."""
    from PIL import Image
    from mx_det.data import write_coco_split
    from scripts import build_corrupted_testsets as b
    for name in ("MX_JPEG_ENCODE", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(name, raising=False)
    src = tmp_path / "src"
    write_coco_split(src, "val", 0, 3, H=48, W=100)
    b.set_seed(b.SEED)
    b.build_coco_testsets(src, tmp_path / "plain")
    written = {}
    orig = b._write_bgr

    def spy(path, img):  # keep the pre-encode pixels
        written[str(path)] = img.cpu().numpy()
        orig(path, img)
    monkeypatch.setattr(b, "_write_bgr", spy)
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "haze,rain")
    b.set_seed(b.SEED)
    b.build_coco_testsets(src, tmp_path / "wx")
    plain, wx = tmp_path / "plain" / "coco6", tmp_path / "wx" / "coco6"
    assert sorted(p.name for p in plain.iterdir()) == sorted(b.VARIANTS)
    assert sorted(p.name for p in wx.iterdir()) == sorted(b.VARIANTS + ["Test_Haze", "Test_Rain"])
    for v in b.VARIANTS:
        for p in sorted((plain / v / "images" / "val").glob("*.jpg")):
            assert p.read_bytes() == (wx / v / "images" / "val" / p.name).read_bytes(), (v, p.name)
    names = sorted(p.name for p in (src / "images" / "val").glob("*.*"))
    assert len(names) == 3
    for i, n in enumerate(names):
        with Image.open(src / "images" / "val" / n) as im:
            bgr = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])
        for v, kind in (("Test_Haze", "haze"), ("Test_Rain", "rain")):
            same(written[str(wx / v / "images" / "val" / n)], ref.apply(bgr, spec(kind, 3), b.weather_seed(i)), (v, n))
    first = {p.name: p.read_bytes() for p in (wx / "Test_Rain" / "images" / "val").glob("*.jpg")}
    b.set_seed(b.SEED)
    b.build_coco_testsets(src, tmp_path / "wx2")
    for p in (tmp_path / "wx2" / "coco6" / "Test_Rain" / "images" / "val").glob("*.jpg"):
        assert p.read_bytes() == first[p.name], p.name
