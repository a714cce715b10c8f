"""Host side of the windowed JPEG reconstruct and the device patch loader (no GPU needed):
restoration.draw_crop against RestorationDataset.crop, jpeg.window_cover (mx_jpeg_window_cover, the
function the kernel calls per tile) against a brute-force restatement of the upsampler's taps, and the
argument guards of both entry points, which answer before any HIP call."""
import ctypes
import random

import numpy as np
import pytest

import jpeg_corpus as jc

PATCH = 64


# ------------------------------------------------------------------------------------------ draw_crop
def _apply(img, x0, y0, flip, s=PATCH):
    p = img[y0:y0 + s, x0:x0 + s]
    return np.ascontiguousarray(p[:, ::-1] if flip else p)


def test_draw_crop_matches_dataset_crop(tmp_path):
    from mx_det.restoration import RestorationDataset, draw_crop
    ds = RestorationDataset(tmp_path, PATCH, is_train=True)
    imgs = [np.random.default_rng(n).integers(0, 256, (h, w, 3), dtype=np.uint8)
            for n, (h, w) in enumerate([(64, 64), (65, 90), (300, 280)])]
    for k in range(5):
        for img in imgs:  # one size at a time
            random.seed(k)
            rng = random.Random(k)
            assert np.array_equal(ds.crop(img), _apply(img, *draw_crop(rng, *img.shape[:2], PATCH, True)))
        # a sequence of mixed sizes, then the generators' next draws
        random.seed(k)
        rng = random.Random(k)
        for img in imgs + imgs[::-1] + imgs:
            assert np.array_equal(ds.crop(img), _apply(img, *draw_crop(rng, *img.shape[:2], PATCH, True)))
        assert random.random() == rng.random()
        assert random.getrandbits(64) == rng.getrandbits(64)


def test_draw_crop_validation_draws_nothing(tmp_path):
    from mx_det.restoration import RestorationDataset, draw_crop
    ds = RestorationDataset(tmp_path, PATCH, is_train=False)
    rng = random.Random(3)
    state = rng.getstate()
    for h, w in [(64, 64), (65, 90), (300, 280)]:
        img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        x0, y0, flip = draw_crop(rng, h, w, PATCH, False)
        assert (x0, y0, flip) == ((w - PATCH) // 2, (h - PATCH) // 2, False)
        assert np.array_equal(ds.crop(img), _apply(img, x0, y0, flip))
    assert rng.getstate() == state


# --------------------------------------------------------------------------------------- window_cover
def _spec(h, w, sampling):
    return next(i for i, s in enumerate(jc.SPECS) if (s[1], s[2], s[5]) == (h, w, sampling))


def _taps(info, x, y):
    """(component, sample row, sample column) of everything output pixel (x, y) reads: the luma sample
    and the taps of chroma() in csrc/mx_jpeg.hip (jdsample.c), restated."""
    out = [(0, y, x)]
    if info.ncomp == 1:
        return out
    hs, vs, dw, dh = info.hmax // info.h[1], info.vmax // info.v[1], info.dw[1], info.dh[1]
    if hs == 1 and vs == 1:
        rows, cols = [y], [x]
    elif dw <= 2:  # replicate
        rows, cols = [y // vs], [x // hs]
    else:
        cx = x >> 1
        cols = [cx]
        if x % 2 == 0 and cx != 0:
            cols.append(cx - 1)
        if x % 2 == 1 and cx != dw - 1:
            cols.append(cx + 1)
        if vs == 1:
            rows = [y]
        else:
            r0 = y >> 1
            r1 = min(max(r0 + 1 if y % 2 else r0 - 1, 0), dh - 1)
            rows = [r0, r1]
    return out + [(c, r, q) for c in (1, 2) for r in rows for q in cols]


def _check_cover(info, box):
    from mx_det import jpeg
    x0, y0, w, h = box
    cover = jpeg.window_cover(info, box)
    assert cover.shape == (3, 4) and cover.dtype == np.int32
    blocks = {(c, r >> 3, q >> 3) for y in range(y0, y0 + h) for x in range(x0, x0 + w) for c, r, q in _taps(info, x, y)}
    for c in range(3):
        mine = [(by, bx) for cc, by, bx in blocks if cc == c]
        if not mine:
            assert c > 0 and info.ncomp == 1 and not cover[c].any(), (box, c, cover)
            continue
        bx0, by0, bx1, by1 = (int(v) for v in cover[c])
        assert 0 <= bx0 < bx1 <= info.bw[c] and 0 <= by0 < by1 <= info.bh[c], (box, c, cover)
        # inside the cover, and every edge of it attained
        assert min(bx for _, bx in mine) == bx0 and max(bx for _, bx in mine) == bx1 - 1, (box, c, cover)
        assert min(by for by, _ in mine) == by0 and max(by for by, _ in mine) == by1 - 1, (box, c, cover)


@pytest.mark.parametrize("sampling", ["420", "422", "444"])
def test_window_cover_small_frames_every_origin(sampling):
    from mx_det import jpeg
    info = jpeg.parse(jc.jpeg_file(_spec(17, 13, sampling)))
    H, W = info.height, info.width
    assert (H, W) == (17, 13)
    n = 0
    for y0 in range(H):
        for x0 in range(W):
            for s in (1, 2, 9):
                _check_cover(info, (x0, y0, min(s, W - x0), min(s, H - y0)))
                n += 1
    assert n == 17 * 13 * 3


@pytest.mark.parametrize("sampling", ["420", "422", "grey"])
def test_window_cover_random_windows(sampling):
    from mx_det import jpeg
    info = jpeg.parse(jc.jpeg_file(_spec(250, 131, sampling)))
    H, W = info.height, info.width
    assert (H, W) == (250, 131)
    rng = random.Random(250131)
    _check_cover(info, (0, 0, W, 1))
    _check_cover(info, (W - 1, 0, 1, H))
    for _ in range(200):
        w, h = rng.randint(1, 48), rng.randint(1, 48)
        _check_cover(info, (rng.randint(0, W - w), rng.randint(0, H - h), w, h))


# --------------------------------------------------------------------------------------------- guards
def test_window_guards_without_gpu():
    """Validation happens before any HIP call and before any pointer is read: MX_EINVAL with a message."""
    from mx_det import _lib, jpeg
    lib = _lib.load()
    info = jpeg.parse(jc.jpeg_file(_spec(17, 13, "420")))
    fake = 1 << 20  # never dereferenced
    cover = np.zeros((3, 4), dtype=np.int32)

    def recon(x0, y0, w, h, row_bytes, inf=info, coefs=fake, out=fake):
        return lib.mx_jpeg_reconstruct_window(coefs, ctypes.byref(inf), x0, y0, w, h, 0, 0, out, row_bytes, None)

    for args, word in [((10, 0, 4, 4, 12), b"outside"), ((0, 14, 4, 4, 12), b"outside"), ((-1, 0, 4, 4, 12), b"outside"),
                       ((0, 0, 0, 4, 12), b"empty"), ((0, 0, 4, 0, 12), b"empty"), ((0, 0, 4, 4, 11), b"out_row_bytes")]:
        assert recon(*args) == -1, args
        assert word in lib.mx_last_error(), (args, lib.mx_last_error())
    assert recon(0, 0, 4, 4, 12, coefs=None) == -1 and b"null" in lib.mx_last_error()
    assert recon(0, 0, 4, 4, 12, out=None) == -1 and b"null" in lib.mx_last_error()
    assert recon(0, 0, 4, 4, 12, inf=_lib.JpegInfo()) == -1 and lib.mx_last_error()  # never parsed
    assert lib.mx_jpeg_window_cover(ctypes.byref(info), 10, 0, 4, 4, cover.ctypes.data) == -1
    assert b"outside" in lib.mx_last_error()
    assert lib.mx_jpeg_window_cover(ctypes.byref(info), 0, 0, 0, 1, cover.ctypes.data) == -1
    assert lib.mx_jpeg_window_cover(ctypes.byref(info), 0, 0, 1, 1, None) == -1
    with pytest.raises(ValueError):
        jpeg.window_cover(info, (0, 0, 14, 1))
    assert lib.mx_jpeg_window_cover(ctypes.byref(info), 0, 0, 13, 17, cover.ctypes.data) == 0
