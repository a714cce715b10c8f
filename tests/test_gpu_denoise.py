"""The non-local-means denoiser on the device (csrc/mx_denoise.hip; mx_det.denoise; tests/denoise_ref.py is the
numpy restatement): the arithmetic is unsigned integers, so every comparison is byte equality.
  * sizes at the tile's edges (one pixel, one tile exactly, one more row and column, more than two tiles each
    way) and images smaller than the halo, where the clamp hits both sides at once;
  * widths whose row pitch is no multiple of 4, and views at odd byte offsets of one buffer;
  * a 17-image list of mixed sizes (it crosses the 16-image chunk), bgr on and off;
  * the saturating inputs: a 0 / 255 checkerboard at sigma_q8 = 1 (D = 1, the largest Q and t * Q), constant
    255 at a large sigma (the largest sum w * X), sigma_q8 = 65535 with k16 = 64 (Q = 0: the clamped 11 x 11
    box mean);
  * blind calls from device stats produced in the same stream with no synchronisation in between, the rule,
    the verdict array and `applied`;
  * two calls into the same buffers agree; a captured and replayed call equals the eager one;
  * GatedRestorer with a denoiser: select and skip return the same bytes and counts, select leaves the host
    ahead of the device, and eval_frcnn_variant runs behind it."""
import numpy as np
import pytest
import torch

import denoise_ref as ref
import gate_ref

pytestmark = pytest.mark.gpu


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rand_img(h, w, salt):
    return np.random.default_rng(3000 + salt).integers(0, 256, (h, w, 3), dtype=np.uint8)


def soft_img(h, w, salt, sigma=12.0):
    """Piecewise-smooth content under noise: the candidates' weights spread over the whole table."""
    rng = np.random.default_rng(4000 + salt)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3), np.float64)
    img[:] = rng.integers(40, 200, 3)
    img += (0.9 * xx + 0.6 * yy)[..., None]
    for _ in range(4):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = rng.integers(20, 236, 3)
    img += rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def tile():
    from mx_det import ops
    return ops.denoise_nlm_tile()


def check(imgs, dev, sigma_q8, k16=6, bgr=False):
    """One explicit-sigma call on a list of numpy images against the restatement; returns the outputs."""
    from mx_det import ops
    q8 = sigma_q8 if isinstance(sigma_q8, (list, tuple)) else [sigma_q8] * len(imgs)
    xs = [to_dev(im, dev) for im in imgs]
    outs, applied = ops.denoise_nlm_u8(xs, sigma=[q / 256.0 for q in q8], k16=k16, bgr=bgr)
    assert applied.dtype == torch.int32 and applied.cpu().tolist() == [1] * len(imgs)
    for b, (im, x, o, q) in enumerate(zip(imgs, xs, outs, q8)):
        assert torch.equal(x.cpu(), torch.from_numpy(im)), "the input changed"
        want = ref.nlm(im, q, k16, bgr)
        got = o.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (b, im.shape, q, int((got != want).sum()))
    return outs


def edge_sizes():
    tr, tc = tile()
    return [(1, 1), (1, tc), (tr, 1), (tr, tc), (tr + 1, tc + 1), (2 * tr + 3, 2 * tc + 3)]


SMALL = [(2, 3), (7, 7), (5, 40)]


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
def test_sizes_at_the_tile_edges_and_below_the_halo(dev, bgr):
    sizes = edge_sizes() + SMALL
    imgs = [soft_img(h, w, k) for k, (h, w) in enumerate(sizes)]
    outs = check(imgs, dev, 2560, bgr=bgr)  # sigma 10
    assert any(not np.array_equal(o.cpu().numpy(), im) for o, im in zip(outs, imgs)), "nothing was denoised"
    # random bytes under a wide filter: the distances are large, the weights still spread
    check([rand_img(h, w, 20 + k) for k, (h, w) in enumerate(sizes)], dev, 80 * 256, k16=24, bgr=bgr)


@pytest.mark.parametrize("w", [5, 67, 69, 70, 71])
def test_odd_row_pitches(dev, w):
    """3 * W % 4 != 0: the rows start at different bytes of their 16-byte vectors."""
    from mx_det import ops
    assert (3 * w) % 4 != 0
    check([soft_img(35, w, w), soft_img(4, w, w + 1)], dev, 2560)
    # views at odd byte offsets of one buffer: the first and last vectors of an image are partial
    h = 21
    base = soft_img(h, w, w + 2)
    want = ref.nlm(base, 2560)
    n = 3 * h * w
    src, dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev), torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    for o in (1, 7, 18, 63):
        src.fill_(0)
        src[o:o + n] = to_dev(base.reshape(-1), dev)
        dst.fill_(9)
        ops.denoise_nlm_u8([src[o:o + n].view(h, w, 3)], sigma=10.0, out=[dst[64 - o:64 - o + n].view(h, w, 3)])
        assert np.array_equal(dst[64 - o:64 - o + n].view(h, w, 3).cpu().numpy(), want), o
        got = dst.cpu().numpy()
        assert (got[:64 - o] == 9).all() and (got[64 - o + n:] == 9).all(), "bytes outside the output changed"


def test_a_list_that_crosses_the_chunk(dev):
    tr, tc = tile()
    sizes = [(1 + 3 * k, 2 + 7 * k) for k in range(12)] + [(tr, tc), (tr + 5, 7), (9, 2 * tc + 9), (40, 40), (1, 1)]
    assert len(sizes) == 17
    imgs = [soft_img(h, w, 40 + k) for k, (h, w) in enumerate(sizes)]
    q8 = [1536 + 256 * k for k in range(17)]  # sigma 6 .. 22: one per image
    check(imgs, dev, q8)
    check(imgs, dev, q8, k16=9, bgr=True)
    # a [B,H,W,3] tensor of 17 is the same call
    from mx_det import ops
    x = np.stack([soft_img(13, 29, 80 + k) for k in range(17)])
    out, applied = ops.denoise_nlm_u8(to_dev(x, dev), sigma=9.0)
    assert tuple(out.shape) == x.shape and applied.cpu().tolist() == [1] * 17
    assert all(np.array_equal(o, ref.nlm(im, 2304)) for o, im in zip(out.cpu().numpy(), x))
    # nothing in, nothing out
    o0, a0 = ops.denoise_nlm_u8(to_dev(x, dev)[:0], sigma=9.0)
    assert tuple(o0.shape) == (0, 13, 29, 3) and tuple(a0.shape) == (0,)


def box_mean(img):
    """The clamped 11 x 11 mean, rounded: what every weight 4096 gives."""
    x = np.pad(img.astype(np.int64), ((5, 5), (5, 5), (0, 0)), mode="edge")
    h, w = img.shape[:2]
    s = sum(x[dy:dy + h, dx:dx + w] for dy in range(11) for dx in range(11))
    return ((4096 * s + (121 * 4096 >> 1)) // (121 * 4096)).astype(np.uint8)


def test_saturating_inputs(dev):
    tr, tc = tile()
    h, w = tr + 9, tc + 7
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    assert ref.params(None, 6, sigma_q8=1)[2:] == (0, 1, 1 << 24)       # T0 = 0, D = 1, the largest Q
    out, wsum = ref.nlm(checker, 1, want_wsum=True)
    assert np.array_equal(out, checker) and int(wsum[h // 2, w // 2]) == 61 * 4096  # the 61 same-parity candidates
    check([checker], dev, 1)
    white = np.full((h, w, 3), 255, np.uint8)                          # the largest sum w * X = 121 * 4096 * 255
    assert np.array_equal(check([white], dev, 65535)[0].cpu().numpy(), white)
    assert ref.params(None, 64, sigma_q8=65535)[4] == 0                 # Q = 0: every weight 4096
    imgs = [rand_img(h, w, 7), rand_img(3, 4, 8)]
    outs = check(imgs, dev, 65535, k16=64)
    assert all(np.array_equal(o.cpu().numpy(), box_mean(im)) for o, im in zip(outs, imgs))


def noisy_content(count, h, w, seed):
    clean = gate_ref.content_images(count, h, w, seed=seed)
    return clean, [np.clip(np.rint(im + np.random.default_rng(500 + i).normal(0, 15, im.shape)), 0, 255).astype(np.uint8)
                   for i, im in enumerate(clean)]


def test_blind_from_device_stats_in_one_stream(dev):
    """Stats and the denoiser back to back, nothing read in between: the kernel takes sigma and the apply
    decision from the device sums."""
    from mx_det import ops
    clean, noisy = noisy_content(3, 45, 83, seed=9)
    imgs = [noisy[0], clean[0], noisy[1], clean[1], noisy[2], clean[2]]
    xs = [to_dev(im, dev) for im in imgs]
    stats, verdict = ops.degradation_stats_u8(xs)
    outs, applied = ops.denoise_nlm_u8(xs, stats=stats)
    rows = [gate_ref.stats(im) for im in imgs]
    assert stats.cpu().tolist() == rows
    want = [ref.denoise(im, row) for im, row in zip(imgs, rows)]
    assert [a for _, a in want] == [1, 0, 1, 0, 1, 0] == applied.cpu().tolist()
    for k, (o, (w, a), im) in enumerate(zip(outs, want, imgs)):
        assert np.array_equal(o.cpu().numpy(), w), k
        assert a or np.array_equal(o.cpu().numpy(), im)
    # another rule and strength: rule (1, 0) fires on every image with IMM > 0
    outs, applied = ops.denoise_nlm_u8(xs, stats=stats, rule=(1, 0), k16=10)
    assert applied.cpu().tolist() == [1] * 6
    for o, im, row in zip(outs, imgs, rows):
        assert np.array_equal(o.cpu().numpy(), ref.denoise(im, row, k16=10, rule=(1, 0))[0])
    # a rule that never fires: copies
    outs, applied = ops.denoise_nlm_u8(xs, stats=stats, rule=(0, 1))
    assert applied.cpu().tolist() == [0] * 6 and all(torch.equal(o, x) for o, x in zip(outs, xs))
    # blind and explicit images in one call
    outs, applied = ops.denoise_nlm_u8(xs[:3], stats=stats[:3].contiguous(), sigma=[None, 7.5, None])
    assert applied.cpu().tolist() == [1, 1, 1]
    assert np.array_equal(outs[1].cpu().numpy(), ref.nlm(imgs[1], 1920))
    assert np.array_equal(outs[2].cpu().numpy(), want[2][0])


def test_an_image_with_verdict_one_is_left_alone(dev):
    from mx_det import ops
    _, noisy = noisy_content(3, 33, 70, seed=10)
    xs = [to_dev(im, dev) for im in noisy]
    stats, _ = ops.degradation_stats_u8(xs)
    verdict = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
    outs, applied = ops.denoise_nlm_u8(xs, stats=stats, verdict=verdict)
    assert applied.cpu().tolist() == [1, 0, 1]
    rows = stats.cpu().tolist()
    for k, (o, im) in enumerate(zip(outs, noisy)):
        want, a = ref.denoise(im, rows[k], verdict=[0, 1, 0][k])
        assert a == [1, 0, 1][k] and np.array_equal(o.cpu().numpy(), want), k
    assert torch.equal(outs[1], xs[1]) and not torch.equal(outs[0], xs[0])
    # the verdict holds for an explicit sigma too
    outs, applied = ops.denoise_nlm_u8(xs, verdict=verdict, sigma=10.0)
    assert applied.cpu().tolist() == [1, 0, 1] and torch.equal(outs[1], xs[1])


def test_two_calls_and_a_replayed_capture_agree(dev):
    from mx_det import conv, ops
    sizes = edge_sizes() + SMALL + [(20, 30)] * 9
    assert len(sizes) > 16
    xs = [to_dev(soft_img(h, w, 70 + k), dev) for k, (h, w) in enumerate(sizes)]
    sig =[10.0] * len(xs)
    out = [torch.full_like(x, 7) for x in xs]
    o1, a1 = ops.denoise_nlm_u8(xs, sigma=sig, out=out)
    assert all(p is q for p, q in zip(o1, out))
    first = [o.clone() for o in out]
    ops.denoise_nlm_u8(xs, sigma=sig, out=out)  # the same buffers, not cleared in between
    assert all(torch.equal(p, q) for p, q in zip(out, first))
    side = conv.capture_stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with conv.capture_guard(), torch.cuda.graph(g, stream=side):
        _, a2 = ops.denoise_nlm_u8(xs, sigma=sig, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(3)
        a2.fill_(-1)
        g.replay()
        torch.cuda.synchronize(dev)
        assert all(torch.equal(p, q) for p, q in zip(out, first)) and torch.equal(a2, a1)


def test_overlap_is_refused_on_the_device_path(dev):
    from mx_det import _lib, ops
    x = to_dev(soft_img(20, 30, 1), dev)
    with pytest.raises(_lib.MxError, match="overlaps"):
        ops.denoise_nlm_u8([x], sigma=5.0, out=[x])


# ---------------------------------------------------------------------------------------------
_UNET = {}


def small_unet(dev):
    """The golden small U-Net (tests/golden/unet_small.npz) on the device, built once."""
    if "m" not in _UNET:
        from mx_det.unet import RestorationUNet
        d = np.load("tests/golden/unet_small.npz")
        m = RestorationUNet(channels=(8, 16, 32, 64), precision="f32")
        m.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")})
        _UNET["m"] = m.eval().to(dev)
    return _UNET["m"]


def gate_mix(dev):
    """Five images of two sizes: blurred (restore), clean (pass), noisy (denoise), and two more of those."""
    from mx_det import augment as A, ops
    clean_a, noisy_a = noisy_content(3, 48, 80, seed=5)
    clean_b, noisy_b = noisy_content(2, 37, 53, seed=6)
    blur = A.severity_spec("blur", 3)
    return [ops.corrupt_batch_u8([to_dev(clean_a[0], dev)], [blur])[0], to_dev(clean_a[1], dev), to_dev(noisy_a[2], dev),
            to_dev(noisy_b[0], dev), to_dev(clean_b[1], dev)]


KINDS = ["restored", "passed", "denoised", "denoised", "passed"]
COUNTS = {"restored": 1, "passed": 2, "denoised": 2}


def test_gated_restorer_with_a_denoiser_modes_agree(dev):
    from mx_det import denoise, gate
    m = small_unet(dev)
    xs = gate_mix(dev)
    dn = denoise.NLMDenoiser()
    sel, skp = gate.GatedRestorer(m, mode="select", denoiser=dn), gate.GatedRestorer(m, mode="skip", denoiser=dn)
    o1, o2 = sel.restore_u8(xs), skp.restore_u8(xs)
    for k, (x, p, q) in enumerate(zip(xs, o1, o2)):
        assert torch.equal(p, q), k
        im = x.cpu().numpy()
        want = {"restored": lambda: m.restore_u8(x[None])[0].cpu().numpy(), "passed": lambda: im,
                "denoised": lambda: ref.denoise(im, gate_ref.stats(im))[0]}[KINDS[k]]()
        assert np.array_equal(p.cpu().numpy(), want), (k, KINDS[k])
        assert (KINDS[k] == "passed") == torch.equal(p, x), k
    assert sel.take_counts() == COUNTS == skp.take_counts()
    assert sel.take_counts() == {"restored": 0, "passed": 0, "denoised": 0}
    # a batch tensor
    x = torch.stack([xs[1], xs[2]])
    a, b = sel.restore_u8(x), skp.restore_u8(x)
    assert torch.equal(a, b) and torch.equal(a[0], x[0]) and torch.equal(a[1], o1[2])
    assert sel.take_counts() == {"restored": 0, "passed": 1, "denoised": 1} == skp.take_counts()
    # without a denoiser: what it was
    plain = gate.GatedRestorer(m, mode="select")
    out = plain.restore_u8(xs)
    assert torch.equal(out[2], xs[2]) and plain.take_counts() == {"restored": 1, "passed": 4}


def test_select_mode_with_a_denoiser_does_not_wait_for_the_device(dev):
    """With the stream held back by a busy kernel (tests/_stream_delay.spin), select mode returns while that
    kernel still runs: the host waited neither for a verdict nor for the sums the denoiser reads."""
    from _stream_delay import spin
    from mx_det import denoise, gate
    m = small_unet(dev)
    xs = gate_mix(dev)
    sel = gate.GatedRestorer(m, mode="select", denoiser=denoise.NLMDenoiser())
    want = [t.clone() for t in sel.restore_u8(xs)]  # warm: kernels loaded, workspaces cached
    sel.take_counts()
    torch.cuda.synchronize(dev)
    assert spin(400.0)
    held = torch.cuda.current_stream(dev).record_event()
    out = sel.restore_u8(xs)
    still_running = not held.query()
    torch.cuda.synchronize(dev)
    assert still_running, "restore_u8 in select mode waited for the device"
    assert all(torch.equal(p, q) for p, q in zip(out, want))
    assert sel.take_counts() == COUNTS


def test_restore_testsets_writes_the_denoised_images(dev, tmp_path, monkeypatch):
    """restore_variant behind a gate in skip mode with a denoiser: a noisy image is the denoiser's output,
    encoded; a passed one is the source file, byte for byte."""
    from PIL import Image
    from mx_det import denoise, gate, jpeg
    from scripts import restore_testsets as rt
    for name in ("MX_JPEG_ENCODE", "MX_JPEG_DECODE"):
        monkeypatch.delenv(name, raising=False)
    src = tmp_path / "in" / "Test_X"
    (src / "images" / "val").mkdir(parents=True)
    (src / "annotations").mkdir()
    (src / "annotations" / "instances_val.json").write_text("{}")
    xs = gate_mix(dev)
    for k, x in enumerate((xs[2], xs[1])):  # noisy, clean
        Image.fromarray(x.cpu().numpy()).save(src / "images" / "val" / f"{k}.jpg", quality=95)
    g = gate.GatedRestorer(small_unet(dev), mode="skip", denoiser=denoise.NLMDenoiser())
    rt.restore_variant(g, "Test_X", dev, src_root=tmp_path / "in", dst_root=tmp_path / "out")
    assert g.take_counts() == {"restored": 0, "passed": 1, "denoised": 1}
    out = tmp_path / "out" / "Test_X" / "images" / "val"
    assert (out / "1.jpg").read_bytes() == (src / "images" / "val" / "1.jpg").read_bytes()
    noisy = rt.read_rgb(src / "images" / "val" / "0.jpg", dev).cpu().numpy()
    den, applied = ref.denoise(noisy, gate_ref.stats(noisy))
    assert applied == 1
    want = tmp_path / "want.jpg"
    jpeg.write_file(want, to_dev(den, dev), quality=95)
    assert (out / "0.jpg").read_bytes() == want.read_bytes()


def test_eval_behind_a_gated_restorer_with_a_denoiser(dev, tmp_path, monkeypatch):
    from mx_det import denoise, engine, gate
    from mx_det.data import write_coco_split
    for name in ("MX_DEVICE_JPEG",):
        monkeypatch.delenv(name, raising=False)
    write_coco_split(tmp_path, "val", 0, 4, H=64, W=96, mean_boxes=3)
    model = engine.build_frcnn(7).to(dev).eval()
    g = gate.GatedRestorer(small_unet(dev), mode="select", denoiser=denoise.NLMDenoiser(rule=(1, 0)))
    res = engine.eval_frcnn_variant(model, str(tmp_path / "images" / "val"), str(tmp_path / "annotations" / "instances_val.json"),
                                    dev, restorer=g)
    assert {"mAP50", "mAP50_95"} <= set(res)
    counts = g.take_counts()
    assert set(counts) == {"restored", "passed", "denoised"} and sum(counts.values()) == 4 and min(counts.values()) >= 0
    assert counts["denoised"] == 4 - counts["restored"]  # rule (1, 0): every image the U-Net leaves alone
