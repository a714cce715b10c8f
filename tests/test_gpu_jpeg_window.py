"""mx_jpeg_reconstruct_window on the device: every window equals the same slice of the full decode
(jpeg.decode, itself pinned to libjpeg-turbo by tests/test_jpeg.py), bit for bit, flipped or not; for
one file of each sampling PIL's own decode, sliced, is a second oracle. The cases sit where the window
path can differ from the full one: windows and tiles that end inside the image (the chroma neighbour
is then real data from the halo block) against windows that end on the image's edge (the clamp),
frames whose chroma takes the replicating upsampler (downsampled width <= 2), partially filled MCUs
at the right and bottom edges, and MCU / tile boundaries. Every test counts its cases."""
import functools
import io
import random

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_corpus as jc

pytestmark = pytest.mark.gpu


def _spec(h, w, sampling, content=None):
    return next(i for i, s in enumerate(jc.SPECS)
                if (s[1], s[2], s[5]) == (h, w, sampling) and content in (None, s[0]))


@functools.lru_cache(maxsize=None)
def _small(n):
    """n x n 4:2:0 noise: downsampled width 2, the replicating upsampler."""
    return jc.pil_jpeg(jc.noise(n, n, 40 + n), 95, "420")


def _data(key):
    return _small(key[1]) if isinstance(key, tuple) else jc.jpeg_file(key)


_frames = {}


def _frame(key, dev, bgr=False):
    """(info, device coefficients, full decode) of a file: computed once, read-only."""
    from mx_det import jpeg
    if (key, bgr) not in _frames:
        data = _data(key)
        info, coefs = jpeg.decode_coefs(data)
        _frames[(key, bgr)] = (info, torch.from_numpy(coefs.copy()).to(dev), jpeg.decode(data, dev, bgr=bgr))
    return _frames[(key, bgr)]


def _run(key, dev, cases, bgr=False):
    """cases: (x0, y0, w, h, hflip). Returns how many were checked."""
    from mx_det import jpeg
    info, coefs, full = _frame(key, dev, bgr)
    n = 0
    for x0, y0, w, h, flip in cases:
        got = jpeg.reconstruct_window(info, coefs, (x0, y0, w, h), hflip=flip, bgr=bgr)
        ref = full[y0:y0 + h, x0:x0 + w]
        ref = ref.flip(1) if flip else ref
        assert got.shape == ref.shape and got.dtype == torch.uint8
        if not torch.equal(got, ref):
            bad = (got != ref).any(2).nonzero()
            raise AssertionError(f"file {key} window {(x0, y0, w, h)} hflip {flip} bgr {bgr}: {bad.shape[0]} pixels "
                                 f"differ, first at (row, col) {bad[0].tolist()}")
        n += 1
    return n


def _every_origin(H, W, sizes=(1, 2, 9)):
    """Every origin with the sizes clipped to the frame; every third case also flipped."""
    cases, k = [], 0
    for y0 in range(H):
        for x0 in range(W):
            for s in sizes:
                cases.append((x0, y0, min(s, W - x0), min(s, H - y0), False))
                if k % 3 == 0:
                    cases.append((x0, y0, min(s, W - x0), min(s, H - y0), True))
                k += 1
    return cases


SMALL = [(8, 8, "444"), (8, 8, "grey"), (17, 13, "420"), (17, 13, "422"), (17, 13, "444")]


@pytest.mark.parametrize("h,w,sampling", SMALL, ids=["%dx%d-%s" % s for s in SMALL])
def test_small_frames_every_origin(dev, h, w, sampling):
    cases = _every_origin(h, w)
    assert len(cases) == h * w * 3 + h * w  # a third of the h * w * 3 windows twice
    assert _run(_spec(h, w, sampling), dev, cases) == len(cases)


def test_small_frame_bgr(dev):
    cases = _every_origin(17, 13)
    assert _run(_spec(17, 13, "420"), dev, cases, bgr=True) == 17 * 13 * 4


def _all_windows(H, W):
    return [(x0, y0, w, h, (x0 + y0 + w + h) % 2 == 1)
            for y0 in range(H) for x0 in range(W) for h in range(1, H - y0 + 1) for w in range(1, W - x0 + 1)]


NONFANCY = [_spec(1, 1, "420"), _spec(1, 1, "grey"), ("small", 3), ("small", 4)]


@pytest.mark.parametrize("key", NONFANCY, ids=["1x1-420", "1x1-grey", "3x3-420", "4x4-420"])
def test_replicating_upsampler_all_windows(dev, key):
    from mx_det import jpeg
    info = jpeg.parse(_data(key))
    if info.ncomp == 3:
        assert info.dw[1] <= 2 and info.hmax == 2  # the frame does take the non-fancy path
    n = info.width
    cases = _all_windows(info.height, info.width)
    assert len(cases) == (n * (n + 1) // 2) ** 2
    assert _run(key, dev, cases) == len(cases)


def _edge_cases(H, W, seed):
    cases = [(0, 0, W, H)]
    for s in (1, 17):  # the four corners
        cases += [(0, 0, s, s), (W - s, 0, s, s), (0, H - s, s, s), (W - s, H - s, s, s)]
    cases += [(15, 40, 2, 30), (15, 0, 2, H), (20, 15, 60, 2), (0, 15, W, 2)]  # astride an MCU boundary
    cases += [(31, 31, 2, 2), (32, 32, 1, 1), (31, 0, 1, H), (0, 31, W, 1)]  # astride / beside a tile boundary
    cases += [(W - 5, H - 7, 5, 7), (W - 33, 3, 33, 20), (3, H - 33, 20, 33), (W - 1, 0, 1, H), (0, H - 1, W, 1)]
    cases += [(97, 130, min(64, W - 97), min(64, H - 130))]
    rng = random.Random(seed)
    for _ in range(50):
        w, h = rng.randint(1, W), rng.randint(1, H)
        cases.append((rng.randint(0, W - w), rng.randint(0, H - h), w, h))
    return [c + (k % 2 == 1,) for k, c in enumerate(cases)]


LARGE = [(250, 131, "420", None), (250, 131, "422", None), (250, 131, "444", None), (250, 131, "grey", "synth"),
         (256, 256, "420", "noise")]


@pytest.mark.parametrize("h,w,sampling,content", LARGE, ids=["%dx%d-%s" % s[:3] for s in LARGE])
def test_large_frames_edges_and_random_windows(dev, h, w, sampling, content):
    key = _spec(h, w, sampling, content)
    info = _frame(key, dev)[0]
    assert (info.height, info.width) == (h, w)
    cases = _edge_cases(h, w, seed=1000 + key)
    assert len(cases) == 1 + 8 + 4 + 4 + 5 + 1 + 50
    assert _run(key, dev, cases) == len(cases)


@pytest.mark.parametrize("sampling", ["420", "422", "444", "grey"])
def test_against_pil(dev, sampling):
    """The second oracle: PIL's decode of the file, sliced."""
    from mx_det import jpeg
    key = _spec(250, 131, sampling, "synth" if sampling == "grey" else None)
    info, coefs, _ = _frame(key, dev)
    pil = torch.from_numpy(np.asarray(Image.open(io.BytesIO(jc.jpeg_file(key))).convert("RGB")).copy())
    n = 0
    for x0, y0, w, h, flip in _edge_cases(250, 131, seed=7)[:30]:
        got = jpeg.reconstruct_window(info, coefs, (x0, y0, w, h), hflip=flip).cpu()
        ref = pil[y0:y0 + h, x0:x0 + w]
        assert torch.equal(got, ref.flip(1) if flip else ref), (sampling, x0, y0, w, h, flip)
        n += 1
    assert n == 30


def test_slot_write_touches_nothing_else(dev):
    from mx_det import jpeg
    key = _spec(250, 131, "420")
    info, coefs, full = _frame(key, dev)
    n = 0
    for flip in (False, True):
        # a whole slot of a batch
        batch = torch.full((3, 20, 20, 3), 0xA5, dtype=torch.uint8, device=dev)
        ret = jpeg.reconstruct_window(info, coefs, (37, 101, 20, 20), hflip=flip, out=batch[1])
        assert ret.data_ptr() == batch[1].data_ptr()
        ref = full[101:121, 37:57]
        assert torch.equal(batch[1], ref.flip(1) if flip else ref)
        assert bool((batch[0] == 0xA5).all()) and bool((batch[2] == 0xA5).all())
        # a row-strided view: the left 12 columns of a slot
        batch = torch.full((3, 20, 20, 3), 0xA5, dtype=torch.uint8, device=dev)
        view = batch[1][:, :12]
        assert not view.is_contiguous()
        jpeg.reconstruct_window(info, coefs, (119, 230, 12, 20), hflip=flip, out=view)
        ref = full[230:250, 119:131]
        assert torch.equal(batch[1][:, :12], ref.flip(1) if flip else ref)
        assert bool((batch[1][:, 12:] == 0xA5).all())
        assert bool((batch[0] == 0xA5).all()) and bool((batch[2] == 0xA5).all())
        n += 2
    assert n == 4
    with pytest.raises(ValueError):
        jpeg.reconstruct_window(info, coefs, (0, 0, 12, 20), out=batch[1][:, :12, :2])
    with pytest.raises(ValueError):
        jpeg.reconstruct_window(info, coefs, (0, 0, 10, 20), out=batch[1][:, ::2])  # pixels not 3 bytes apart


def test_decode_window(dev):
    from mx_det import jpeg
    # plain, optimised tables, restart intervals (1 block, 7 blocks: no multiple of an MCU row)
    keys = [_spec(250, 131, "420"), _spec(250, 131, "444"), _spec(250, 131, "422"), _spec(64, 64, "420", "synth")]
    assert [jc.SPECS[k][7] for k in keys] == [0, 2, 7, 7]
    n = 0
    for key in keys:
        full = _frame(key, dev)[2]
        H, W = full.shape[:2]
        for entropy in ("device", "host"):
            for box, flip in [((W // 3, H // 4, W // 2, H // 2), False), ((W - 9, H - 11, 9, 11), True)]:
                got = jpeg.decode_window(jc.jpeg_file(key), dev, box, hflip=flip, entropy=entropy)
                x0, y0, w, h = box
                ref = full[y0:y0 + h, x0:x0 + w]
                assert torch.equal(got, ref.flip(1) if flip else ref), (key, entropy, box)
                n += 1
    assert n == 16
    with pytest.raises(ValueError):
        jpeg.decode_window(jc.jpeg_file(keys[0]), dev, (0, 0, 1, 1), entropy="gpu")
