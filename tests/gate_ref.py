"""numpy restatement of mx_degradation_stats_u8, written from its definition in include/mx_det.h (a helper,
not a test): the int64 luma, the eight sums over the interior pixels, and the verdict of a rule list in
Python ints. Plus the content generator of the verdict tests."""
import numpy as np

N, IMM, DX2, DY2, DXX2, DYY2, G2, H2 = range(8)


def luma(img, bgr=False):
    """Y = (77 R + 150 G + 29 B + 128) >> 8 of a uint8 [H, W, 3] array, int64."""
    v = np.asarray(img).astype(np.int64)
    r, g, b = (v[..., 2], v[..., 1], v[..., 0]) if bgr else (v[..., 0], v[..., 1], v[..., 2])
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def stats(img, bgr=False):
    """[N, IMM, DX2, DY2, DXX2, DYY2, G2, H2] as Python ints."""
    y = luma(img, bgr)
    h, w = y.shape
    assert h >= 3 and w >= 3
    c = y[1:-1, 1:-1]
    up, down, left, right = y[:-2, 1:-1], y[2:, 1:-1], y[1:-1, :-2], y[1:-1, 2:]
    corners = y[:-2, :-2] + y[:-2, 2:] + y[2:, :-2] + y[2:, 2:]
    imm = np.abs(corners - 2 * (up + down + left + right) + 4 * c)
    assert int(imm.max()) <= 2040
    dx2 = int(((right - left) ** 2).sum())
    dy2 = int(((down - up) ** 2).sum())
    dxx2 = int(((right - 2 * c + left) ** 2).sum())
    dyy2 = int(((down - 2 * c + up) ** 2).sum())
    return [(h - 2) * (w - 2), int(imm.sum()), dx2, dy2, dxx2, dyy2, dx2 + dy2, dxx2 + dyy2]


def decide(row, rules, default):
    """The first rule (i, j, a, b, verdict, ...) with a * row[i] > b * row[j] gives the verdict."""
    row = [int(v) for v in row]
    for r in rules:
        i, j, a, b, verdict = (int(v) for v in tuple(r)[:5])
        if a * row[i] > b * row[j]:
            return verdict
    return int(default)


def content_images(count=6, h=192, w=256, seed=2024):
    """The piecewise-smooth test content: a constant colour, 40 random filled rectangles, a 10-grey-level
    sinusoid in x and y, sigma = 2 grain; uint8 [h, w, 3], a fixed seed."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(count):
        img = np.empty((h, w, 3), np.float64)
        img[:] = rng.integers(60, 200, 3)
        for _ in range(40):
            y0, x0 = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 8))
            hh, ww = int(rng.integers(8, h // 2)), int(rng.integers(8, w // 2))
            img[y0:y0 + hh, x0:x0 + ww] = rng.integers(20, 236, 3)
        px, py = rng.uniform(40, 120, 2)
        img += (10.0 * np.sin(2 * np.pi * xx / px + rng.uniform(0, 6)) * np.sin(2 * np.pi * yy / py + rng.uniform(0, 6)))[..., None]
        img += rng.normal(0.0, 2.0, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out
