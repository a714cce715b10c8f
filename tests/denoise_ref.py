"""numpy restatement of mx_denoise_nlm_u8, written from its definition in include/mx_det.h (a helper, not a
test): the per-image parameters in Python ints, then per candidate offset the squared luma differences on the
clamped image, their 5 x 5 box sums by cumulative sums, the table lookup and the weighted channel sums, all in
int64. About 0.1 s for 96 x 128."""
import numpy as np

import gate_ref

P, S = 2, 5
# round(4096 * exp(-i / 16)), i = 0..127: the literals of csrc/mx_nlm_lut.h
LUT = (
    4096, 3848, 3615, 3396, 3190, 2997, 2815, 2645, 2484, 2334, 2192, 2060, 1935, 1818, 1707, 1604,
    1507, 1416, 1330, 1249, 1174, 1102, 1036, 973, 914, 859, 807, 758, 712, 669, 628, 590,
    554, 521, 489, 460, 432, 406, 381, 358, 336, 316, 297, 279, 262, 246, 231, 217,
    204, 192, 180, 169, 159, 149, 140, 132, 124, 116, 109, 103, 96, 90, 85, 80,
    75, 70, 66, 62, 58, 55, 52, 48, 46, 43, 40, 38, 35, 33, 31, 29,
    28, 26, 24, 23, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 12, 11,
    10, 10, 9, 8, 8, 7, 7, 7, 6, 6, 5, 5, 5, 5, 4, 4,
    4, 4, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 1,
)


def tdq(s8, k16):
    """(T0, D, Q) of a luma sigma s8 / 256."""
    d = max((25 * k16 * k16 * s8 * s8) >> 24, 1)
    return (50 * s8 * s8) >> 16, d, (1 << 24) // d


def params(stats_row=None, k16=6, rule=(10, 383), sigma_q8=0, verdict=None):
    """(apply, s8, T0, D, Q) in Python ints."""
    if sigma_q8:
        apply, s8 = True, int(sigma_q8)
    else:
        n, imm = int(stats_row[0]), int(stats_row[1])
        apply = rule[0] * imm > rule[1] * n
        s8 = (((imm << 8) // n) * 13689) >> 16
    if verdict is not None and verdict != 0:
        apply = False
    return (apply, s8) + tdq(s8, k16)


def nlm(img, s8, k16=6, bgr=False, want_wsum=False):
    """The denoised image (uint8 [H, W, 3]) of a uint8 [H, W, 3] array at luma sigma s8 / 256; with want_wsum
    also Wsum per pixel (int64 [H, W])."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    t0, _, q = tdq(int(s8), k16)
    y = np.pad(gate_ref.luma(img, bgr), P + S, mode="edge")          # clamped coordinates -(P+S) .. +(P+S)
    x = np.pad(img.astype(np.int64), ((S, S), (S, S), (0, 0)), mode="edge")
    lut = np.array(LUT + (0,), np.int64)
    hh, ww = h + 2 * P, w + 2 * P                                       # the pixels a patch of the image touches
    centre = y[S:S + hh, S:S + ww]
    wsum = np.zeros((h, w), np.int64)
    acc = np.zeros((h, w, 3), np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            e = (centre - y[S + dy:S + dy + hh, S + dx:S + dx + ww]) ** 2
            c = np.zeros((hh + 1, ww + 1), np.int64)
            c[1:, 1:] = e.cumsum(0).cumsum(1)
            k = 2 * P + 1
            d = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]    # [h, w]: the 5 x 5 box sum
            assert int(d.max()) < 1 << 21
            t = np.maximum(d - t0, 0)
            assert int(t.max()) * q < 1 << 45
            wgt = lut[np.minimum((t * q) >> 20, 128)]
            wsum += wgt
            acc += wgt[..., None] * x[S + dy:S + dy + h, S + dx:S + dx + w]
    assert int(wsum.min()) >= 4096 and int(acc.max()) < 1 << 27
    out = ((acc + (wsum >> 1)[..., None]) // wsum[..., None]).astype(np.uint8)
    return (out, wsum) if want_wsum else out


def denoise(img, stats_row=None, k16=6, rule=(10, 383), sigma_q8=0, verdict=None, bgr=False):
    """(out, applied) of one image under mx_denoise_nlm_u8's per-image rules."""
    apply, s8, _, _, _ = params(stats_row, k16, rule, sigma_q8, verdict)
    if not apply:
        return np.array(img, copy=True), 0
    return nlm(img, s8, k16, bgr), 1


def psnr(a, b):
    mse = float(((np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)) ** 2).mean())
    return 10.0 * np.log10(255.0 ** 2 / mse)
