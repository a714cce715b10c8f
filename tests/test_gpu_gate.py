"""The restoration gate on the device (csrc/mx_gate.hip; mx_det.gate; tests/gate_ref.py is the numpy
restatement): the eight sums are exact integers, so every comparison is equality.
  * stats equal the restatement at the tile's edges (one interior pixel, one tile exactly, one more row and
    column than a tile, more than one tile each way), at widths whose row pitch is no multiple of 4, for a
    17-image list of mixed sizes (it crosses the 16-image chunk), with bgr on and off, on random bytes and
    on the two saturating 512 x 512 patterns at which a narrow accumulator would overflow;
  * the device verdict equals decide() under the default rules, under eight rules with coefficients 65535,
    and under no rule with default 1; two calls into the same buffers agree; a captured and replayed call
    agrees with the eager one;
  * the 24 content images, corrupted on the device at level 3, get the expected verdicts;
  * mx_restore_finish_gated picks per image between restore_u8's bytes and the input's;
  * GatedRestorer: select and skip return the same bytes and counts, select leaves the host ahead of the
    device (no synchronisation), and eval_frcnn_variant runs behind a gated restorer."""
import numpy as np
import pytest
import torch

import gate_ref as ref

pytestmark = pytest.mark.gpu


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rand_img(h, w, salt):
    return np.random.default_rng(1000 + salt).integers(0, 256, (h, w, 3), dtype=np.uint8)


def tile():
    from mx_det import ops
    return ops.degradation_stats_tile()


def check(imgs, dev, rules=None, default=0, bgr=False, out=None):
    """Device stats and verdicts of a list of numpy images against the restatement; returns them."""
    from mx_det import gate, ops
    rules = gate.DEFAULT_RULES if rules is None else rules
    stats, verdict = ops.degradation_stats_u8([to_dev(im, dev) for im in imgs], rules, default, bgr=bgr, out=out)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (len(imgs), 8)
    assert verdict.dtype == torch.int32 and tuple(verdict.shape) == (len(imgs),)
    got, gv = stats.cpu().tolist(), verdict.cpu().tolist()
    for b, im in enumerate(imgs):
        want = ref.stats(im, bgr)
        assert got[b] == want, (b, im.shape, got[b], want)
        assert gv[b] == ref.decide(want, rules, default), (b, im.shape, gv[b])
    return stats, verdict


def edge_sizes():
    tr, tc = tile()
    return [(3, 3), (3, tc + 2), (tr + 2, 3), (tr + 2, tc + 2), (tr + 1, tc + 1), (tr + 3, tc + 3), (2 * tr + 2, 2 * tc + 3)]


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
def test_stats_at_the_tile_edges(dev, bgr):
    sizes = edge_sizes()
    assert any((3 * w) % 4 for _, w in sizes)
    check([rand_img(h, w, k) for k, (h, w) in enumerate(sizes)], dev, bgr=bgr)


@pytest.mark.parametrize("w", [5, 131, 133, 134, 135])
def test_odd_row_pitches(dev, w):
    """3 * W % 4 != 0: the rows start at different bytes of their 16-byte vectors."""
    assert (3 * w) % 4 != 0
    imgs = [rand_img(37, w, w), rand_img(4, w, w + 1)]
    check(imgs, dev)
    # views at odd byte offsets of one buffer: the first and last vectors of an image are partial
    flat = to_dev(np.random.default_rng(w).integers(0, 256, 3 * 37 * w + 64, dtype=np.uint8), dev)
    from mx_det import ops
    views = [flat[o:o + 3 * 37 * w].view(37, w, 3) for o in (1, 7, 18, 63)]
    stats, _ = ops.degradation_stats_u8(views)
    for v, row in zip(views, stats.cpu().tolist()):
        assert row == ref.stats(v.cpu().numpy())


def test_a_list_that_crosses_the_chunk(dev):
    tr, tc = tile()
    sizes = [(3 + 5 * k, 4 + 13 * k) for k in range(12)] + [(tr + 2, tc + 2), (tr + 5, 7), (9, 2 * tc + 9), (64, 64), (3, 3)]
    assert len(sizes) == 17
    imgs = [rand_img(h, w, 40 + k) for k, (h, w) in enumerate(sizes)]
    check(imgs, dev)
    check(imgs, dev, bgr=True)
    # a [B,H,W,3] tensor of 17 is the same call
    from mx_det import ops
    x = to_dev(np.stack([rand_img(21, 29, 80 + k) for k in range(17)]), dev)
    stats, verdict = ops.degradation_stats_u8(x)
    assert stats.cpu().tolist() == [ref.stats(im) for im in x.cpu().numpy()]
    # nothing in, nothing out
    s0, v0 = ops.degradation_stats_u8(x[:0])
    assert tuple(s0.shape) == (0, 8) and tuple(v0.shape) == (0,)


def saturating():
    yy, xx = np.mgrid[0:512, 0:512]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)           # maximises |IMM| = 2040, DXX, DYY = 510
    steps = (((yy >> 1) + (xx >> 1)) & 1) * 255                   # 0,0,255,255 each way: DX, DY = 255
    return [np.repeat(p.astype(np.uint8)[..., None], 3, axis=2) for p in (checker, steps)]


def test_saturating_patterns(dev):
    checker, steps = saturating()
    n = 510 * 510
    assert ref.stats(checker)[:2] == [n, 2040 * n] and ref.stats(checker)[4] == 510 * 510 * n
    assert ref.stats(steps)[2] == 255 * 255 * n and ref.stats(steps)[3] == 255 * 255 * n
    check([checker, steps], dev)


def test_verdicts_under_other_rule_lists(dev):
    from mx_det import gate
    imgs = [rand_img(h, w, 60 + k) for k, (h, w) in enumerate(edge_sizes())] + saturating()
    imgs.append(np.full((20, 31, 3), 90, np.uint8))  # flat: nothing fires
    check(imgs, dev, gate.DEFAULT_RULES, 0)
    big = 65535
    eight = [(1, 7, big, big, 0), (4, 5, big, big - 1, 1), (2, 3, big, big, 0), (3, 2, big - 1, big, 1), (6, 7, 1, big, 0),
             (0, 1, big, 1, 1), (5, 4, big, big, 0), (7, 6, big, 0, 1)]
    _, v = check(imgs, dev, eight, 0)
    assert len(set(v.cpu().tolist())) == 2  # both verdicts occur
    check(imgs, dev, eight[::-1], 1)
    _, v = check(imgs, dev, (), 1)
    assert v.cpu().tolist() == [1] * len(imgs)
    _, v = check(imgs, dev, (), 0)
    assert v.cpu().tolist() == [0] * len(imgs)


def test_two_calls_and_a_replayed_capture_agree(dev):
    from mx_det import ops
    imgs = [rand_img(h, w, 70 + k) for k, (h, w) in enumerate(edge_sizes())] + [rand_img(50, 70, 99 + k) for k in range(11)]
    assert len(imgs) > 16
    xs = [to_dev(im, dev) for im in imgs]
    out = (torch.full((len(xs), 8), -7, dtype=torch.int64, device=dev), torch.full((len(xs),), -7, dtype=torch.int32, device=dev))
    s1, v1 = check(imgs, dev, out=out)
    assert s1 is out[0] and v1 is out[1]
    first = (s1.clone(), v1.clone())
    check(imgs, dev, out=out)  # the same buffers, not cleared in between
    assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])
    # one stream, no branches: captured on the framework's capture stream, as its own graphs are, and
    # replayed on the main stream; the outputs are poisoned before each replay
    from mx_det import conv
    side = conv.capture_stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with conv.capture_guard(), torch.cuda.graph(g, stream=side):
        ops.degradation_stats_u8(xs, out=out)
    for _ in range(2):
        out[0].fill_(-1)
        out[1].fill_(-1)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])


def test_content_verdicts_on_the_device(dev):
    """The 24 cases of test_gate_host.py's CPU check, corrupted on the device at level 3 (noise from the
    device generator), under DEFAULT_RULES: clean 0, noise 0, blur 1, lowres 1."""
    from mx_det import augment as A, gate, ops
    clean = [to_dev(im, dev) for im in ref.content_images()]
    assert len(clean) == 6
    want = {"clean": 0, "noise": 0, "blur": 1, "lowres": 1}
    xs, expect = [], []
    for kind, verdict in want.items():
        xs += clean if kind == "clean" else ops.corrupt_batch_u8(clean, [A.severity_spec(kind, 3)] * 6, seed=11)
        expect += [verdict] * 6
    stats, verdict = ops.degradation_stats_u8(xs)
    rows = stats.cpu().tolist()
    for x, row in zip(xs, rows):
        assert row == ref.stats(x.cpu().numpy())
    print([(round(f["sigma"], 2), round(f["anisotropy"], 2), round(f["hf"], 3)) for f in gate.features(rows)])
    assert len(expect) == 24 and verdict.cpu().tolist() == expect


def test_fit_script_measures_fits_and_writes(dev, tmp_path, monkeypatch):
    """scripts.fit_restore_gate on the content images written as JPEGs: the fitted rules classify every
    measured row, the file loads back, and MX_RESTORE_GATE takes it."""
    from PIL import Image
    from mx_det import gate
    from scripts import fit_restore_gate as f
    for name in ("MX_EXTRA_VARIANTS", "MX_SEVERITIES", "MX_GATE_LABELS", "MX_JPEG_DECODE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(f, "init_device", lambda: (dev, 1, 0))
    for k, im in enumerate(ref.content_images()):
        Image.fromarray(im).save(tmp_path / f"{k}.jpg", quality=95)
    table = f.measure([f.restore_testsets.read_rgb(p, dev) for p in sorted(tmp_path.glob("*.jpg"))], f.conditions(), 7)
    assert sorted(table) == ["blur", "clean", "lowres", "noise"] and all(len(v) == 6 for v in table.values())
    rules, default = f.main(train_dir=tmp_path, out_path=tmp_path / "out" / "gate.json", count=6)
    assert gate.load_rules(tmp_path / "out" / "gate.json") == (rules, default)
    assert gate.env_gate(str(tmp_path / "out" / "gate.json")) == (rules, default)
    for name, rows in table.items():
        assert [gate.decide(r, rules, default) for r in rows] == [gate.CONDITION_VERDICTS[name]] * 6, name
    with pytest.raises(FileNotFoundError):
        f.main(train_dir=tmp_path / "none", out_path=tmp_path / "x.json", count=6)


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


def test_restore_finish_gated(dev):
    m = small_unet(dev)
    x = to_dev(np.stack([rand_img(37, 53, 120), rand_img(37, 53, 121)]), dev)
    full = m.restore_u8(x)
    assert not torch.equal(full, x)
    verdict = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    got = m.restore_u8(x, verdict=verdict)
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], x[1])
    assert torch.equal(m.restore_u8(x, verdict=torch.ones(2, dtype=torch.int32, device=dev)), full)
    assert torch.equal(m.restore_u8(x, verdict=torch.zeros(2, dtype=torch.int32, device=dev)), x)
    y = to_dev(rand_img(48, 64, 122), dev)[None]  # no padding: Hp == H, Wp == W
    assert torch.equal(m.restore_u8(y, verdict=torch.ones(1, dtype=torch.int32, device=dev)), m.restore_u8(y))
    with pytest.raises(RuntimeError):
        m.restore_u8(x, verdict=torch.ones(2, dtype=torch.int64, device=dev))


def gate_mix(dev):
    """Four images of two sizes: content blurred (restore), content clean (pass), and the same again."""
    from mx_det import augment as A, ops
    a, b = (to_dev(im, dev) for im in ref.content_images(2, 48, 80, seed=5))
    c, d = (to_dev(im, dev) for im in ref.content_images(2, 37, 53, seed=6))
    blur = A.severity_spec("blur", 3)
    return [ops.corrupt_batch_u8([a], [blur])[0], b, c, ops.corrupt_batch_u8([d], [blur])[0]]


def test_gated_restorer_modes_agree(dev):
    from mx_det import gate
    m = small_unet(dev)
    xs = gate_mix(dev)
    want = [1, 0, 0, 1]
    sel, skp = gate.GatedRestorer(m, mode="select"), gate.GatedRestorer(m, mode="skip")
    assert sel.decide_u8(xs) == want
    o1, o2 = sel.restore_u8(xs), skp.restore_u8(xs)
    for k, (x, p, q) in enumerate(zip(xs, o1, o2)):
        assert torch.equal(p, q), k
        assert torch.equal(p, m.restore_u8(x[None])[0] if want[k] else x), k
        assert p.data_ptr() != x.data_ptr()
    assert (sel.restored, sel.passed) == (2, 2) == (skp.restored, skp.passed)
    # a batch tensor, every mode; the counts add up and take_counts() starts again
    x = torch.stack([xs[0], xs[1]])
    assert torch.equal(sel.restore_u8(x), skp.restore_u8(x))
    assert torch.equal(sel.restore_u8(x)[1], x[1])
    assert sel.take_counts() == {"restored": 4, "passed": 4} and skp.take_counts() == {"restored": 3, "passed": 3}
    assert sel.take_counts() == {"restored": 0, "passed": 0}
    # other rules: restore everything / nothing
    every = gate.GatedRestorer(m, rules=(), default=1)
    assert torch.equal(every.restore_u8(x), m.restore_u8(x)) and every.take_counts() == {"restored": 2, "passed": 0}
    none = gate.GatedRestorer(m, rules=(), default=0, mode="skip")
    assert torch.equal(none.restore_u8(x), x) and none.take_counts() == {"restored": 0, "passed": 2}


def test_select_mode_does_not_wait_for_the_device(dev):
    """With the stream held back by a busy kernel (tests/_stream_delay.spin), select mode returns while that
    kernel still runs: the host never waited for a verdict. The result is right once the stream drains."""
    from _stream_delay import spin
    from mx_det import gate
    m = small_unet(dev)
    xs = gate_mix(dev)
    sel = gate.GatedRestorer(m, mode="select")
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
    assert sel.take_counts() == {"restored": 2, "passed": 2}


def test_restore_testsets_copies_the_passed_files(dev, tmp_path, monkeypatch):
    """restore_variant behind a gate in skip mode: a passed image is the source file, byte for byte; a flagged
    one is the U-Net's output, encoded."""
    from PIL import Image
    from mx_det import gate, jpeg
    from scripts import restore_testsets as rt
    for name in ("MX_JPEG_ENCODE", "MX_JPEG_DECODE"):
        monkeypatch.delenv(name, raising=False)
    src = tmp_path / "in" / "Test_X"
    (src / "images" / "val").mkdir(parents=True)
    (src / "annotations").mkdir()
    (src / "annotations" / "instances_val.json").write_text("{}")
    for k, x in enumerate(gate_mix(dev)[:2]):  # blurred, clean
        Image.fromarray(x.cpu().numpy()).save(src / "images" / "val" / f"{k}.jpg", quality=95)
    m = small_unet(dev)
    g = gate.GatedRestorer(m, mode="skip")
    rt.restore_variant(g, "Test_X", dev, src_root=tmp_path / "in", dst_root=tmp_path / "out")
    assert g.take_counts() == {"restored": 1, "passed": 1}
    out = tmp_path / "out" / "Test_X" / "images" / "val"
    assert (out / "1.jpg").read_bytes() == (src / "images" / "val" / "1.jpg").read_bytes()
    blurred = rt.read_rgb(src / "images" / "val" / "0.jpg", dev)
    want = tmp_path / "want.jpg"
    jpeg.write_file(want, m.restore_u8(blurred[None])[0], quality=95)
    assert (out / "0.jpg").read_bytes() == want.read_bytes()
    assert (tmp_path / "out" / "Test_X" / "annotations" / "instances_val.json").read_text() == "{}"


def test_eval_behind_a_gated_restorer(dev, tmp_path, monkeypatch):
    from mx_det import engine, gate
    from mx_det.data import write_coco_split
    for name in ("MX_DEVICE_JPEG",):
        monkeypatch.delenv(name, raising=False)
    write_coco_split(tmp_path, "val", 0, 4, H=64, W=96, mean_boxes=3)
    model = engine.build_frcnn(7).to(dev).eval()
    g = gate.GatedRestorer(small_unet(dev), mode="select")
    res = engine.eval_frcnn_variant(model, str(tmp_path / "images" / "val"), str(tmp_path / "annotations" / "instances_val.json"),
                                    dev, restorer=g)
    assert {"mAP50", "mAP50_95"} <= set(res)
    counts = g.take_counts()
    assert counts["restored"] + counts["passed"] == 4 and min(counts.values()) >= 0
