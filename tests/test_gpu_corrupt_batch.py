"""The batched corruption launch (include/mx_det.h mx_corrupt_batch_u8; mx_det.ops.corrupt_batch_u8) and
the severity levels built on it (mx_det.augment, RestorationBatcher, the test-set builder). Every
comparison is equality:
  * each op against the exact-arithmetic oracle (oracle/) at sizes around the kernel's output tile
    (mx_corrupt_batch_tile: rows R, columns C): heights {1, 3, R-1, R, R+1, 2R+1} x widths {1, 2, C-1, C,
    C+1, 2C+1} and 61 x 87, all frames of one case in one call (a list of frames of different sizes);
  * a mixed batch, image by image, against the existing one-parameter-set entries (ops.corrupt_u8,
    ops.filter2d_u8, ops.corrupt_jpeg_u8) called for that image alone;
  * in place, `out=`, stream order behind a delayed producer;
  * the Python layer: RestorationBatcher with severities, the builder's Test_<Kind>_s<L> sets, eval_all's
    names."""
import csv
import functools
import io
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

STEP = 0x9E3779B97F4A7C15
M64 = 2 ** 64 - 1


@functools.lru_cache(maxsize=None)
def tile():
    from mx_det import ops
    return ops.corrupt_batch_tile()


@functools.lru_cache(maxsize=None)
def sizes():
    R, C = tile()
    return tuple((h, w) for h in (1, 3, R - 1, R, R + 1, 2 * R + 1) for w in (1, 2, C - 1, C, C + 1, 2 * C + 1)) + ((61, 87),)


@functools.lru_cache(maxsize=None)
def image(H, W, salt=0):
    """Uniform random bytes (every neighbour differs, both clip ends occur); computed once, read-only."""
    img = np.random.default_rng(1000003 * salt + 4099 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def to_dev(img, dev):
    return torch.from_numpy(np.array(img)).to(dev)


def same(got, ref, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    ref = ref.cpu().numpy() if torch.is_tensor(ref) else ref
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:6].tolist(), got[tuple(bad[:6].T)], ref[tuple(bad[:6].T)])


def test_noise_with_an_explicit_field_equals_the_oracle(dev):
    from mx_det import ops
    from oracle import oracle as orc
    rng = np.random.default_rng(5)
    imgs = [image(h, w) for h, w in sizes()]
    fields = [rng.normal(0, 40, im.shape).astype(np.float32) for im in imgs]
    got = ops.corrupt_batch_u8([to_dev(im, dev) for im in imgs], [(ops.CORRUPT_NOISE, 40.0)] * len(imgs),
                               noise=[torch.from_numpy(f).to(dev) for f in fields])
    for im, f, g in zip(imgs, fields, got):
        same(g, orc.noise_u8(im, f), im.shape)


@pytest.mark.parametrize("k, angle", [(5, 0), (9, 0), (17, 0), (13, 45), (5, -20), (11, 135)])
def test_blur_equals_the_oracle(dev, k, angle):
    """The sizes include H = 3 under k = 17 (repeated reflection) and W = 1."""
    from mx_det import ops
    from oracle import oracle as orc
    taps = [tuple(float(v) for v in row) for row in orc.kernel_taps(orc.motion_blur_kernel(k, angle))]
    imgs = [image(h, w) for h, w in sizes()]
    got = ops.corrupt_batch_u8([to_dev(im, dev) for im in imgs], [(ops.CORRUPT_BLUR, taps)] * len(imgs))
    for im, g in zip(imgs, got):
        same(g, orc.motion_blur_u8(im, k, angle), im.shape)


@pytest.mark.parametrize("factor", [0.75, 0.625, 0.5, 0.375, 0.25, 0.3, 0.9])
def test_lowres_equals_the_oracle(dev, factor):
    """Beyond the tile sizes: even frames that take the exact-x2 path with a non-empty scalar tail, odd
    frames at 0.5 (the general path; 61 x 87 and the odd tile sizes), 2 x 2 at 0.25 (nh = nw = 1)."""
    from mx_det import ops
    from oracle import oracle as orc
    hw = list(sizes()) + [(64, 162), (80, 132), (2, 2)]
    if factor == 0.5:
        assert (162 // 2 * 3) % 48 and (132 // 2 * 3) % 48  # the scalar tails are not empty
    imgs = [image(h, w) for h, w in hw]
    got = ops.corrupt_batch_u8([to_dev(im, dev) for im in imgs], [(ops.CORRUPT_LOWRES, factor)] * len(imgs))
    for im, g in zip(imgs, got):
        same(g, orc.lowres_u8(im, factor), im.shape)


def mixed_batch(dev):
    """B = 8 at 34 x 162 (even: factor 0.5 takes the exact-x2 path with a tail): every op and identity,
    eight parameter sets."""
    from mx_det import augment as A, ops
    x = torch.from_numpy(np.stack([image(34, 162, salt=b + 1) for b in range(8)])).to(dev)
    t5 = A.kernel_taps(A.motion_blur_kernel(5, 0))
    t13 = A.kernel_taps(A.motion_blur_kernel(13, 45))
    specs = [(ops.CORRUPT_NONE,), (ops.CORRUPT_NOISE, 5.0), (ops.CORRUPT_NOISE, 40.0), (ops.CORRUPT_BLUR, t5),
             (ops.CORRUPT_BLUR, t13), (ops.CORRUPT_LOWRES, 0.5), (ops.CORRUPT_LOWRES, 0.25), (ops.CORRUPT_LOWRES, 0.9)]
    return x, specs


def alone(x, b, spec, seed):
    """Image b of batch x under `spec` by the existing entries, called for that parameter set alone."""
    from mx_det import ops
    B = x.shape[0]
    op = spec[0]
    if op == ops.CORRUPT_NONE:
        return x[b]
    if op == ops.CORRUPT_NOISE:
        return ops.corrupt_u8(x, [op] * B, sigma=spec[1], seed=seed)[b]
    if op == ops.CORRUPT_BLUR:
        return ops.filter2d_u8(x[b:b + 1], spec[1])[0]
    if op == ops.CORRUPT_LOWRES:
        return ops.corrupt_u8(x, [op] * B, factor=spec[1], seed=seed)[b]
    return ops.corrupt_jpeg_u8(x[b:b + 1], int(spec[1]))[0]


def test_mixed_batch_equals_each_image_alone(dev):
    from mx_det import ops
    x, specs = mixed_batch(dev)
    seed = 0x1234567890ABCDEF
    got = ops.corrupt_batch_u8(x, specs, seed=seed)
    assert got.shape == x.shape and got.dtype == torch.uint8
    for b, sp in enumerate(specs):
        same(got[b], alone(x, b, sp, seed), (b, sp[0]))
    assert all((got[b] != x[b]).any() for b in range(1, 8))
    # the same batch with JPEG among them
    specs[0], specs[4] = (ops.CORRUPT_JPEG, 25), ops.CorruptSpec(ops.CORRUPT_JPEG, 7)
    got = ops.corrupt_batch_u8(x, specs, seed=seed)
    for b, sp in enumerate(specs):
        same(got[b], alone(x, b, sp, seed), (b, sp[0]))


def test_frames_of_four_sizes_in_one_call(dev):
    from mx_det import augment as A, ops
    R, C = tile()
    hw = [(R + 1, 2 * C + 1), (61, 87), (2 * R, C), (3, C - 1)]
    xs = [to_dev(image(h, w, salt=9), dev) for h, w in hw]
    specs = [(ops.CORRUPT_NOISE, 25.0), (ops.CORRUPT_BLUR, A.kernel_taps(A.motion_blur_kernel(7, 0))),
             (ops.CORRUPT_LOWRES, 0.5), (ops.CORRUPT_NOISE, 10.0)]
    got = ops.corrupt_batch_u8(xs, specs, seed=77)
    assert isinstance(got, list) and [g.shape for g in got] == [x.shape for x in xs]
    for b, (x, sp) in enumerate(zip(xs, specs)):
        one = ops.corrupt_batch_u8([x], [sp], seed=(77 + STEP * b) & M64)[0]
        same(got[b], one, b)
        same(got[b], alone(x[None], 0, sp, (77 + STEP * b) & M64), b)
    # JPEG frames of two sizes: one corrupt_jpeg_u8 call per size group
    js = [to_dev(image(24, 40, salt=1), dev), to_dev(image(9, 5), dev), to_dev(image(24, 40, salt=2), dev)]
    qs = [15, 50, 7]
    got = ops.corrupt_batch_u8(js, [(ops.CORRUPT_JPEG, q) for q in qs])
    for x, q, g in zip(js, qs, got):
        same(g, ops.corrupt_jpeg_u8(x[None], q)[0])


def test_in_place_and_out(dev):
    from mx_det import ops
    x, specs = mixed_batch(dev)
    want = ops.corrupt_batch_u8(x, specs, seed=3)
    # noise and identity in place
    y = x[:3].clone()
    assert ops.corrupt_batch_u8(y, specs[:3], seed=3, out=y) is y
    same(y, want[:3])
    frames = [x[b].clone() for b in range(3)]
    got = ops.corrupt_batch_u8(frames, specs[:3], seed=3, out=frames)
    assert all(g is f for g, f in zip(got, frames))
    for b in range(3):
        same(frames[b], want[b])
    # out= is honoured, and rows with op 0 are copied
    out = torch.full_like(x, 0xA5)
    assert ops.corrupt_batch_u8(x, specs, seed=3, out=out) is out
    same(out, want)
    same(out[0], x[0])
    # blur and low-res refuse to run in place
    for b in (3, 5):
        y = x[b:b + 1].clone()
        with pytest.raises(RuntimeError, match="in place"):
            ops.corrupt_batch_u8(y, specs[b:b + 1], out=y)
        same(y, x[b:b + 1])


def test_stream_order_behind_a_delayed_producer(dev):
    """On the framework's own weight-gradient stream (no new stream from torch's pool), as the JPEG
    corruption's test does."""
    from _stream_delay import spin
    from mx_det import conv, ops
    src, specs = mixed_batch(dev)
    want = ops.corrupt_batch_u8(src, specs, seed=21).cpu().numpy()
    x = torch.zeros_like(src)
    torch.cuda.synchronize()
    side = conv.wgrad_stream(dev)
    with torch.cuda.stream(side):
        spin(20.0)
        x.copy_(src)  # the late producer
        out = ops.corrupt_batch_u8(x, specs, seed=21)
    torch.cuda.current_stream().wait_stream(side)
    same(out, want)


@pytest.mark.parametrize("kinds", [("noise", "blur", "lowres"), ("noise", "blur", "lowres", "jpeg")], ids=["default", "jpeg"])
def test_restoration_batcher_with_severities(dev, kinds):
    """Per patch exactly the pixels of its drawn (kind, level), computed alone by the existing entries."""
    from mx_det import augment as A
    from mx_det.restoration import RestorationBatcher
    clean = torch.from_numpy(np.stack([image(96, 96, salt=20 + b) for b in range(8)]))
    levels = (1, 2, 3, 4, 5)
    random.seed(1234)
    draws = []
    for _ in range(8):
        kind = A._choice(kinds)
        draws.append((kind, random.choice(levels)))
    seed = random.getrandbits(62)
    random.seed(1234)
    cor, tgt = RestorationBatcher(dev, kinds=kinds, severities=levels)(clean)
    x = clean.to(dev)
    f32 = lambda t: t.permute(2, 0, 1).float().div_(255.0)  # noqa: E731
    assert len({d for d in draws}) > 3
    for b, (kind, level) in enumerate(draws):
        sp = A.severity_spec(kind, level)
        same(cor[b], f32(alone(x, b, (sp.op, sp.param), seed)), (b, kind, level))
        same(tgt[b], f32(x[b]))


def test_restoration_batcher_default_is_the_call_as_it_stood(dev, monkeypatch):
    from mx_det import augment as A, ops
    from mx_det.restoration import RestorationBatcher
    monkeypatch.delenv("MX_SEVERITIES", raising=False)
    clean = torch.from_numpy(np.stack([image(48, 48, salt=40 + b) for b in range(6)]))
    random.seed(99)
    codes = [random.choice((ops.CORRUPT_NOISE, ops.CORRUPT_BLUR, ops.CORRUPT_LOWRES)) for _ in range(6)]
    want = ops.corrupt_u8(clean.to(dev), codes, seed=random.getrandbits(62), quality=15, subsampling=2)
    state = random.getstate()
    random.seed(99)
    cor, _ = RestorationBatcher(dev, severities=A.env_severities())(clean)  # unset: (3,), as the scripts pass it
    assert random.getstate() == state
    same(cor, want.permute(0, 3, 1, 2).float().div_(255.0))


def q95(rgb):
    """The pixels read back from rgb saved as JPEG at quality 95."""
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=95)
    buf.seek(0)
    with Image.open(buf) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8).copy()


def test_builder_writes_the_severity_sets(dev, tmp_path, monkeypatch):
    from mx_det.data import write_coco_split
    from oracle import oracle as orc
    from scripts import build_corrupted_testsets as b
    monkeypatch.delenv("MX_JPEG_ENCODE", raising=False)
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    monkeypatch.delenv("MX_SEVERITIES", raising=False)
    src = tmp_path / "src"
    write_coco_split(src, "val", 0, 3, H=96, W=134)
    b.set_seed(b.SEED)
    b.build_coco_testsets(src, tmp_path / "plain")
    written = {}
    orig = b._write_bgr

    def spy(path, img):  # keep the pre-encode pixels
        written[str(path)] = img.cpu().numpy()
        orig(path, img)
    monkeypatch.setattr(b, "_write_bgr", spy)
    monkeypatch.setenv("MX_SEVERITIES", "1,3,5")
    b.set_seed(b.SEED)
    b.build_coco_testsets(src, tmp_path / "sev")
    plain, sev = tmp_path / "plain" / "coco6", tmp_path / "sev" / "coco6"
    assert sorted(p.name for p in plain.iterdir()) == sorted(b.VARIANTS)
    assert sorted(p.name for p in sev.iterdir()) == sorted(
        b.VARIANTS + [f"Test_{k}_s{lv}" for k in ("Noise", "Blur", "LowRes") for lv in (1, 5)])
    for v in b.VARIANTS:  # the four reference sets, the noise stream included: the same bytes
        files = sorted((plain / v / "images" / "val").glob("*.jpg"))
        assert len(files) == 3
        for p in files:
            assert p.read_bytes() == (sev / v / "images" / "val" / p.name).read_bytes(), (v, p.name)
    assert (sev / "Test_Blur_s1" / "annotations" / "instances_val.json").exists()
    names = [p.name for p in (src / "images" / "val").glob("*.*")]  # the builder's order
    bgr = {}
    for n in names:
        with Image.open(src / "images" / "val" / n) as im:
            bgr[n] = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])
    for n in names:
        for lv, f in ((1, 0.75), (5, 0.25)):
            want = orc.lowres_u8(bgr[n], f)
            p = sev / f"Test_LowRes_s{lv}" / "images" / "val" / n
            same(written[str(p)], want, (n, lv))
            with Image.open(p) as im:
                same(np.asarray(im.convert("RGB"), dtype=np.uint8), q95(want[..., ::-1]), (n, lv))
        for lv, k in ((1, 5), (5, 17)):
            same(written[str(sev / f"Test_Blur_s{lv}" / "images" / "val" / n)], orc.motion_blur_u8(bgr[n], k, 0.0), (n, lv))
    # the severity noise sets continue the one np.random stream behind Test_Noise
    rng = np.random.RandomState(b.SEED)
    for lv, sigma in ((3, 15), (1, 5), (5, 40)):
        for n in names:
            field = rng.normal(0, sigma, bgr[n].shape).astype(np.float32)
            v = "Test_Noise" if lv == 3 else f"Test_Noise_s{lv}"
            same(written[str(sev / v / "images" / "val" / n)], orc.noise_u8(bgr[n], field), (n, lv))


def test_eval_all_names_the_severity_sets(tmp_path, monkeypatch):
    from scripts import eval_all
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    monkeypatch.setenv("MX_SEVERITIES", "1,3,5")
    vs = eval_all.all_variants()
    assert vs == eval_all.VARIANTS + ["Test_Noise_s1", "Test_Noise_s5", "Test_Blur_s1", "Test_Blur_s5",
                                      "Test_LowRes_s1", "Test_LowRes_s5"]
    res = {"FasterRCNN": {v: {"mAP50": 0.5, "mAP50_95": 0.25, "per_class_ap50": {}} for v in vs}}
    eval_all.save_csv(res, tmp_path / "r.csv")
    rows = list(csv.reader(open(tmp_path / "r.csv")))
    assert rows[0] == ["Model", "Metric", "Clean", "Noise", "Blur", "LowRes", "Noise-s1", "Noise-s5", "Blur-s1",
                       "Blur-s5", "LowRes-s1", "LowRes-s5"]
    assert len(rows[1]) == 2 + len(vs)
