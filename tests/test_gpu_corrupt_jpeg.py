"""JPEG compression as a corruption (include/mx_det.h mx_corrupt_jpeg_u8; mx_det.ops.corrupt_jpeg_u8 /
corrupt_u8 code CORRUPT_JPEG; mx_det.augment; the test-set builder) against libjpeg-turbo itself: the
pixels PIL reads back from the file PIL saves. Every comparison is equality.
  * geometry x quality x subsampling, RGB and BGR; every quality 1..100 in one batch (the in-kernel
    quantisation tables); a mixed batch whose quality-0 rows keep a sentinel;
  * the same pixels as the existing stages (jpeg.forward -> mx_jpeg_reconstruct): a difference there is
    the fusion's, not the arithmetic's;
  * stream order behind a delayed producer on a side stream;
  * ops.corrupt_u8 with and without the new code; the augmentation classes; the builder's Test_JPEG.
Images: tests/test_jpeg_encode.py band_image (noise band, flat band, checkerboard patch)."""
import ctypes
import functools
import io
import json
import random

import numpy as np
import pytest
import torch
from PIL import Image

from test_jpeg_encode import band_image

pytestmark = pytest.mark.gpu

SIZES = [  # (H, W)
    (1, 1),
    (9, 5),      # luma dummy row, replicate-mode chroma
    (16, 3),
    (8, 9),      # chroma row replicated after downsampling
    (24, 40),
    (17, 130),   # three 64-pixel strips, a partial last strip, odd height
    (121, 163),
]
QUALITIES = (5, 15, 50, 95, 100)
BGR_SIZES = ((9, 5), (121, 163))


@functools.lru_cache(maxsize=None)
def image(H, W):
    img = band_image(H, W, 7 * H + W)
    img.setflags(write=False)
    return img


def pil_round_trip(img, q, sub):
    """Image.open(BytesIO(save(img, "JPEG", quality=q, subsampling=sub))).convert("RGB")"""
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(b, format="JPEG", quality=q, subsampling=sub)
    b.seek(0)
    with Image.open(b) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def reference(H, W, q, sub, bgr=False):
    """PIL's round trip of image(H, W); with bgr the array is read as BGR on both sides. Computed once,
    shared, read-only."""
    img = image(H, W)
    ref = pil_round_trip(img[..., ::-1], q, sub)[..., ::-1] if bgr else pil_round_trip(img, q, sub)
    ref = np.ascontiguousarray(ref)
    ref.setflags(write=False)
    return ref


def same(got, ref):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = np.argwhere(got != ref)
    assert bad.shape[0] == 0, (bad.shape[0], bad[:6].tolist(), got[tuple(bad[:6].T)], ref[tuple(bad[:6].T)])


@pytest.mark.parametrize("sub", [2, 0], ids=["s2", "s0"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_equals_pil_round_trip(dev, size, sub):
    from mx_det import ops
    H, W = size
    x = torch.from_numpy(image(H, W).copy()).to(dev)[None]
    for q in QUALITIES:
        same(ops.corrupt_jpeg_u8(x, q, subsampling=sub)[0], reference(H, W, q, sub))
        if size in BGR_SIZES:
            same(ops.corrupt_jpeg_u8(x, q, subsampling=sub, bgr=True)[0], reference(H, W, q, sub, True))


def test_every_quality_in_one_batch(dev):
    from mx_det import ops
    img = image(24, 40)
    x = torch.from_numpy(img.copy()).to(dev)[None].repeat(100, 1, 1, 1)
    got = ops.corrupt_jpeg_u8(x, list(range(1, 101))).cpu().numpy()
    for q in range(1, 101):
        same(got[q - 1], reference(24, 40, q, 2))


def test_mixed_batch_leaves_quality_zero_rows_alone(dev):
    from mx_det import ops
    g = np.random.default_rng(3)
    imgs = np.stack([band_image(40, 72, 50 + i) for i in range(5)])
    imgs[1:] = np.roll(imgs[1:], 3, axis=2)
    imgs[4] = g.integers(0, 256, imgs[4].shape, dtype=np.uint8)
    x = torch.from_numpy(imgs).to(dev)
    qs = [15, 0, 90, 0, 1]
    out = torch.full_like(x, 0xA5)
    assert ops.corrupt_jpeg_u8(x, qs, out=out) is out
    got = out.cpu().numpy()
    for b, q in enumerate(qs):
        if q == 0:
            assert (got[b] == 0xA5).all()
        else:
            same(got[b], ops.corrupt_jpeg_u8(x[b:b + 1], q)[0].cpu().numpy())
            same(got[b], pil_round_trip(imgs[b], q, 2))
    # without `out`, a quality-0 row is the input
    same(ops.corrupt_jpeg_u8(x, qs)[1], imgs[1])


@pytest.mark.parametrize("sub", [2, 0], ids=["s2", "s0"])
def test_equals_the_separate_stages(dev, sub):
    from mx_det import jpeg, ops
    x = torch.from_numpy(image(121, 163).copy()).to(dev)
    info = jpeg.encode_info(163, 121, 15, sub)
    staged = jpeg._reconstruct(info, jpeg.forward(x, info), dev, False)
    same(ops.corrupt_jpeg_u8(x[None], 15, subsampling=sub)[0], staged.cpu().numpy())


def test_stream_order_behind_a_delayed_producer(dev):
    """The side stream is the framework's own weight-gradient stream (a HIP stream the process keeps
    anyway), not a new one from torch's pool: the streams and hardware queues the later tests see stay
    the ones they saw without this test."""
    from _stream_delay import spin
    from mx_det import conv, ops
    img = image(121, 163)
    want = reference(121, 163, 15, 2)
    src = torch.from_numpy(img.copy()).to(dev)[None]
    x = torch.zeros_like(src)
    torch.cuda.synchronize()
    side = conv.wgrad_stream(dev)
    with torch.cuda.stream(side):
        spin(20.0)
        x.copy_(src)  # the late producer
        out = ops.corrupt_jpeg_u8(x, 15)
    torch.cuda.current_stream().wait_stream(side)
    same(out[0], want)


def test_corrupt_u8_with_the_jpeg_code(dev):
    from mx_det import ops
    imgs = np.stack([band_image(40, 72, 80 + i) for i in range(5)])
    x = torch.from_numpy(imgs).to(dev)
    N, B, L, J = ops.CORRUPT_NOISE, ops.CORRUPT_BLUR, ops.CORRUPT_LOWRES, ops.CORRUPT_JPEG
    assert J == 4
    plain = ops.corrupt_u8(x, [N, 0, B, 0, L], seed=11).cpu().numpy()
    mixed = ops.corrupt_u8(x, [N, J, B, J, L], seed=11).cpu().numpy()
    for b in (0, 2, 4):
        same(mixed[b], plain[b])
    for b in (1, 3):
        same(plain[b], imgs[b])
        same(mixed[b], pil_round_trip(imgs[b], 15, 2))
    other = ops.corrupt_u8(x, [J, J, 0, 0, 0], quality=60, subsampling=0, bgr=True).cpu().numpy()
    same(other[1], pil_round_trip(imgs[1][..., ::-1], 60, 0)[..., ::-1])


def test_corrupt_u8_without_the_jpeg_code_is_unchanged(dev):
    """The single mx_corrupt_u8 call corrupt_u8 made before CORRUPT_JPEG existed, restated."""
    from mx_det import _lib, ops
    x = torch.from_numpy(np.stack([band_image(33, 50, 90 + i) for i in range(4)])).to(dev)
    codes = [ops.CORRUPT_NOISE, ops.CORRUPT_BLUR, ops.CORRUPT_LOWRES, ops.CORRUPT_NONE]
    B, H, W, C = x.shape
    want = torch.empty_like(x)
    tmp = torch.empty((B, max(1, int(H * 0.5)), max(1, int(W * 0.5)), C), dtype=torch.uint8, device=dev)
    _lib.call("mx_corrupt_u8", x.data_ptr(), B, H, W, C, (ctypes.c_int32 * B)(*codes), 15.0, ctypes.c_uint64(5), None,
              0.5, tmp.data_ptr(), want.data_ptr(), _lib.stream())
    same(ops.corrupt_u8(x, codes, seed=5), want.cpu().numpy())


def test_apply_jpeg_is_pil_on_a_bgr_array(dev):
    from mx_det import augment
    assert (augment.JPEG_QUALITY, augment.JPEG_SUBSAMPLING) == (15, 2)
    bgr = np.ascontiguousarray(image(121, 163)[..., ::-1])
    got = augment.apply_jpeg(bgr, augment.JPEG_QUALITY)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    same(got, reference(121, 163, 15, 2)[..., ::-1])


def test_random_corruption_gpu_draws_jpeg(dev):
    from mx_det import augment
    x = torch.from_numpy(image(24, 40).copy()).to(dev)
    aug = augment.RandomCorruptionGPU(p=1.0, kinds=("noise", "jpeg"))
    random.seed(5)
    hits = 0
    for _ in range(12):
        state = random.getstate()
        out = aug(x)
        random.setstate(state)
        random.random()  # the keep draw
        if random.choice(["noise", "jpeg"]) == "jpeg":
            hits += 1
            same(out, reference(24, 40, 15, 2))
        random.getrandbits(63)
    assert hits > 0
    # the PIL transform hands over the BGR view of the RGB image and says so: the same pixels
    random.seed(1)
    got = np.asarray(augment.RandomCorruption(p=1.0, kinds=("jpeg",))(Image.fromarray(image(24, 40))))
    same(got, reference(24, 40, 15, 2))
    with pytest.raises(ValueError):
        augment.RandomCorruptionGPU(kinds=("noise", "fog"))


def test_default_kinds_are_the_class_as_it_stood(dev):
    """RandomCorruptionGPU before `kinds`, restated: same outputs, same state of `random` after 20 calls."""
    from mx_det import augment, ops

    def before(img, p=0.5):
        if random.random() > p:
            return img
        code = {"noise": ops.CORRUPT_NOISE, "blur": ops.CORRUPT_BLUR,
                "lowres": ops.CORRUPT_LOWRES}[random.choice(["noise", "blur", "lowres"])]
        return ops.corrupt_u8(img[None], [code], sigma=15, seed=random.getrandbits(63), factor=0.5)[0]

    x = torch.from_numpy(image(24, 40).copy()).to(dev)
    random.seed(9)
    want = [before(x).cpu().numpy() for _ in range(20)]
    want_state = random.getstate()
    aug = augment.RandomCorruptionGPU(p=0.5)
    random.seed(9)
    got = [aug(x).cpu().numpy() for _ in range(20)]
    assert random.getstate() == want_state
    assert any((w != image(24, 40)).any() for w in want)
    for g, w in zip(got, want):
        same(g, w)


def _src(root, n=3):
    from mx_det.data import synth_image
    for kind in ("yolo6", "coco6"):
        d = root / kind / "images" / "val"
        d.mkdir(parents=True)
        for i in range(n):
            Image.fromarray(synth_image(i, 40, 56)).save(d / f"{i:03d}.jpg", quality=95)
    lbl = root / "yolo6" / "labels" / "val"
    lbl.mkdir(parents=True)
    for i in range(n):
        (lbl / f"{i:03d}.txt").write_text("0 0.5 0.5 0.1 0.1\n")
    (root / "coco6" / "annotations").mkdir(parents=True)
    json.dump({"images": [], "annotations": [], "categories": []},
              open(root / "coco6/annotations/instances_val.json", "w"))


def test_builder_writes_test_jpeg(dev, tmp_path, monkeypatch):
    from scripts import build_corrupted_testsets as b
    monkeypatch.delenv("MX_JPEG_ENCODE", raising=False)
    _src(tmp_path / "src")
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    b.main(tmp_path / "src/yolo6", tmp_path / "src/coco6", tmp_path / "plain")
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "jpeg")
    b.main(tmp_path / "src/yolo6", tmp_path / "src/coco6", tmp_path / "extra")
    plain = sorted(p.relative_to(tmp_path / "plain") for p in (tmp_path / "plain").rglob("*") if p.is_file())
    extra = sorted(p.relative_to(tmp_path / "extra") for p in (tmp_path / "extra").rglob("*") if p.is_file())
    assert not any("Test_JPEG" in f.parts for f in plain)
    assert [f for f in extra if "Test_JPEG" not in f.parts] == plain
    for f in plain:  # the reference's four variants, the noise stream included
        if f.name != "data.yaml":  # data.yaml names its own root
            assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "extra" / f).read_bytes(), f
    for kind in ("yolo6", "coco6"):
        files = sorted((tmp_path / "extra" / kind / "Test_JPEG" / "images" / "val").glob("*.jpg"))
        assert len(files) == 3
        for p in files:
            with Image.open(tmp_path / "src" / kind / "images" / "val" / p.name) as im:
                src = np.asarray(im.convert("RGB"), dtype=np.uint8)
            buf = io.BytesIO()
            Image.fromarray(pil_round_trip(src, 15, 2)).save(buf, format="JPEG", quality=95)
            assert p.read_bytes() == buf.getvalue(), p
    assert (tmp_path / "extra/coco6/Test_JPEG/annotations/instances_val.json").exists()
    assert (tmp_path / "extra/yolo6/Test_JPEG/labels/val/000.txt").exists()
