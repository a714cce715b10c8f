"""Exact-integer checks of the implicit-GEMM conv kernels at launch-geometry boundaries and on the
big grids of the production dispatch.

Operands are small integers (x, dy, residual in -2..2, w in {-1, 1}, bias in -3..3): exact in bf16 and
in the bf16x3 hi plane (lo = 0), and with |x|max * |w|max * Kdim < 2^24 every partial sum of any
order is an exact f32. The result then depends on no tile, split count, K-tile order or kernel
variant, and every comparison with torch's float64 CPU conv is an equality:
  f32 outputs == ref, bf16 outputs == bf16(ref) (one rounding of an exact value on either side),
  the BN statistics sum row (summed over blocks in float64) == the reference column sums,
  bias / residual / ReLU epilogues exact, LeakyReLU == where(z > 0, z, z * 0.2f) in f32.
The sum-of-squares row keeps the bar of test_gpu_conv.py / test_gpu_x3.py. The BN-backward partials
of the dgrad epilogue are taken with an integer mean and invstd = 0.5, which makes them exact too;
they are held to test_gpu_x3.py's bar (rtol 1e-5, atol 1e-4).

Each case asserts through mx_conv_last_launch that it took the path it was written for (block tile,
split count, buffer or per-lane loader, kernel kind): the expected records are literal tables worked
out from make_geo / launch_igemm at 256 CUs, so a retune that moves a threshold fails here with a
message instead of silently dropping the coverage.

Cases are (N, H, W, C, K, k, stride, pad), or (N, H, W, C, K, R, S, stride_h, stride_w, pad_h, pad_w)
for the asymmetric family.

Two-plane operand families (bf16x3 only). With integers both lo planes of the bf16x3 split are zero
and two of its three MFMAs per K-step (a_lo * b_hi, a_hi * b_lo) multiply by zero. A "two-plane" value
is v = a + b * 2^-10 with a a nonzero integer, |a| <= 2 (activations, gradients) or |a| = 1 (weights),
and b in {-1, 0, 1}: the RNE split of mx_common.h gives hi = bf16(v) = a and lo = bf16(v - hi) =
b * 2^-10, so hi + lo = v exactly and about two thirds of the lo plane is nonzero. The kernels never form
lo * lo, so every product they do form is a multiple of 2^-10, and with sum |terms| * 2^10 < 2^24 over a
reduction (asserted on the CPU per case, pass and family from convs of the planes' absolute values)
every partial sum of any order, tile, split count or kernel variant is an exact f32: the comparisons
stay equalities. Bias and residuals stay integers. Three families, each with its own float64 reference:
  "alo"   A operand two-plane, B integers (fwd: x two-plane, w = +-1; dgrad: dy two-plane, w = +-1;
          wgrad: dy two-plane, x integers). Expected: the exact conv. B_lo = 0, so this pins the
          a_lo * b_hi MFMA alone: the A-lo half-tile in LDS, its ring halves and its masking.
  "blo"   A integers, B two-plane (fwd: w two-plane; dgrad: w two-plane; wgrad: x two-plane).
          Expected: the exact conv. Pins a_hi * b_lo alone, and the weight lo plane in the KRSC and
          the dgrad parity-class layouts.
  "both"  both two-plane. Expected: conv(a, b) - conv(a_lo, b_lo) in float64, the planes taken on
          the host with .bfloat16(): no fourth term, no doubled term, and the RNE split itself.
The BN sum row is compared by equality where 64 * max|z| * 2^10 < 2^24 holds for the case (a 64-row
partial is then exact), else at test_gpu_x3.py's bar (1e-5 of the largest column sum of |z|).
Deliberately left to the integer family: the bf16 path (it cannot hold these values) and the wgrad of
the big grids (family A reduces over up to 128,000 pixels, past the bound with 2^-10 steps).
"""
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

# ---- shape families -------------------------------------------------------------------------------
# A. big grids of the default dispatch (variant 7, loader 1). fwd pick / dgrad pick at 256 CUs:
FAMILY_A = [
    (2, 128, 192, 256, 256, 1, 1, 0),   # 128x128, 768 tiles, unsplit / the same
    (1, 128, 160, 32, 384, 1, 1, 0),    # 128x256, 320 tiles / dgrad narrow (Ncol 32): 128x64, 160 -> 64x64
    (2, 160, 168, 64, 64, 3, 1, 1),     # 128x64 narrow, 420 tiles / the same
    (2, 200, 320, 128, 128, 1, 1, 0),   # 64x128, 2000 tiles / the same
    # C % 32 != 0: per-lane loader; 800 narrow 128-row tiles, nk = 16 -> launch_kind picks 4 (BK64x2):
    # 2 rounds at 2 blocks per CU (x 2/3) against 2 rounds at 3
    (2, 200, 256, 112, 64, 3, 1, 1),
]
# fwd (bmt, bn, splits, tiles, buf, kind) and dgrad record of FAMILY_A
A_FWD = {
    FAMILY_A[0]: (128, 128, 1, 768, 1, 3),
    FAMILY_A[1]: (128, 256, 1, 320, 1, 3),
    FAMILY_A[2]: (128, 64, 1, 420, 1, 3),
    FAMILY_A[3]: (64, 128, 1, 2000, 1, 3),
    FAMILY_A[4]: (128, 64, 1, 800, 0, 4),
}
A_DGRAD = {
    FAMILY_A[0]: (128, 128, 1, 768, 1, 3),
    FAMILY_A[1]: (64, 64, 1, 320, 1, 3),     # Ncol = 32 -> narrow; 160 128-row tiles -> 64-row tiles; nk = 6
    FAMILY_A[2]: (128, 64, 1, 420, 1, 3),
    FAMILY_A[3]: (64, 128, 1, 2000, 1, 3),
    FAMILY_A[4]: (128, 128, 1, 800, 1, 3),   # Ncol = 112 < 128: no candidate applies, the 128x128 default stays
}

# B. tile and K-loop boundaries: 1x1, N = 1, H = 1, W = M; C = 64 (fwd: one 64-wide K-tile, buffer
# loader; dgrad: Ncol = 64 narrow, Kdim = K on either side of % 32). Pairwise M x K:
B_MK = [(1, 1, m, 64, k, 1, 1, 0) for m, k in [
    (63, 8), (64, 56), (65, 64), (127, 72), (128, 120), (129, 128), (193, 136), (63, 248), (64, 256), (65, 264),
    (127, 64), (128, 128), (129, 256), (193, 72), (193, 264), (64, 136), (128, 8), (63, 120)]]
B_FWD_ONLY = [(1, 1, m, 64, k, 1, 1, 0) for m, k in [(65, 1), (127, 7), (129, 9), (193, 65), (64, 129)]]
# C % 32 / Kdim % 32 loader switch: 3x3 pad 1 on a 5x6 map, two M (N = 2, 5) x two K, pairwise
B_C_LOADER = [(n, 5, 6, c, k, 3, 1, 1) for c in (8, 24, 32, 40, 72) for n, k in ((2, 64), (5, 136))]
# nk 7/8 and 15/16 in 64- and 32-wide K-tiles (split on / off, kt_per_split remainders): M = 200
B_C_KLOOP = [(1, 1, 200, c, 128, 1, 1, 0) for c in (440, 448, 456, 504, 512, 520, 1016, 1024, 1032)]
# fwd (bmt, bn, splits, tiles, buf, kind)
B_FWD = {
    (1, 1, 63, 64, 8, 1, 1, 0): (64, 64, 1, 1, 1, 3),
    (1, 1, 64, 64, 56, 1, 1, 0): (64, 64, 1, 1, 1, 3),
    (1, 1, 65, 64, 64, 1, 1, 0): (64, 64, 1, 2, 1, 3),
    (1, 1, 127, 64, 72, 1, 1, 0): (64, 128, 1, 2, 1, 3),
    (1, 1, 128, 64, 120, 1, 1, 0): (64, 128, 1, 2, 1, 3),
    (1, 1, 129, 64, 128, 1, 1, 0): (64, 128, 1, 3, 1, 3),
    (1, 1, 193, 64, 136, 1, 1, 0): (64, 128, 1, 8, 1, 3),
    (1, 1, 63, 64, 248, 1, 1, 0): (64, 128, 1, 2, 1, 3),
    (1, 1, 64, 64, 256, 1, 1, 0): (64, 128, 1, 2, 1, 3),
    (1, 1, 65, 64, 264, 1, 1, 0): (64, 128, 1, 6, 1, 3),
    (1, 1, 127, 64, 64, 1, 1, 0): (64, 64, 1, 2, 1, 3),
    (1, 1, 128, 64, 128, 1, 1, 0): (64, 128, 1, 2, 1, 3),
    (1, 1, 129, 64, 256, 1, 1, 0): (64, 128, 1, 6, 1, 3),
    (1, 1, 193, 64, 72, 1, 1, 0): (64, 128, 1, 4, 1, 3),
    (1, 1, 193, 64, 264, 1, 1, 0): (64, 128, 1, 12, 1, 3),
    (1, 1, 64, 64, 136, 1, 1, 0): (64, 128, 1, 2, 1, 3),
    (1, 1, 128, 64, 8, 1, 1, 0): (64, 64, 1, 2, 1, 3),
    (1, 1, 63, 64, 120, 1, 1, 0): (64, 128, 1, 1, 1, 3),
}

# C. spatial edges, C = K = 64 and C = K = 32
_SMALL_MAPS = [(1, 1), (1, 2), (2, 3), (3, 2), (1, 9), (9, 1)]
C_SMALL = [(2, h, w, ck, ck, 3, st, 1) for ck in (64, 32) for st in (1, 2) for h, w in _SMALL_MAPS]
C_STEM = [(2, 5, 4, 8, 64, 7, 2, 3)]
C_1X1_S2 = [(2, h, w, ck, ck, 1, 2, 0) for ck in (64, 32) for h, w in ((1, 1), (1, 2), (2, 1))]
# stride 2 over even / odd x even / odd H, W from {1, 2, 3, 4, 15, 16}, pairwise
C_S2_PARITY = [(2, h, w, ck, ck, 3, 2, 1) for h, w, ck in [
    (1, 16, 64), (2, 15, 32), (3, 4, 64), (4, 3, 32), (15, 2, 64), (16, 1, 32), (15, 15, 32), (16, 16, 64),
    (2, 2, 64), (3, 3, 32), (15, 16, 64), (16, 15, 32), (4, 1, 64), (1, 3, 32),
    # 128 channels: the non-empty classes reach 8 K-tiles of 64, so the bf16 split-K sizing runs too
    (1, 16, 128), (16, 1, 128)]]
# wgrad pixel walk: output maps of 2, 31, 32, 33, 35, 63, 64, 65 pixels (3x3 pad 1, stride 1)
C_WGRAD_MAPS = [(1, 2), (1, 31), (4, 8), (3, 11), (5, 7), (7, 9), (8, 8), (5, 13)]
C_WGRAD = [(n, h, w, 64, 64, 3, 1, 1) for h, w in C_WGRAD_MAPS for n in (1, 5)]

# D. asymmetric geometry on a 9x14 map, C = K = 64, N = 2: (N, H, W, C, K, R, S, sh, sw, ph, pw)
FAMILY_D = (
    [(2, 9, 14, 64, 64, 3, 3, sh, sw, 1, 1) for sh, sw in ((1, 2), (2, 1))]
    + [(2, 9, 14, 64, 64, r, 3, 1, 1, ph, pw) for r in (3, 5) for ph, pw in ((0, 1), (1, 0), (2, 1))]
    + [(2, 9, 14, 64, 64, r, s, 1, 1, r // 2, s // 2) for r, s in ((1, 3), (3, 1), (1, 7), (7, 1))]
    + [(2, 9, 14, 64, 64, 5, 3, 2, 1, 2, 1), (2, 9, 14, 64, 64, 3, 3, 1, 2, 0, 1)]
)

BOUNDARY_SIX = [B_MK[5], B_MK[9], B_C_LOADER[3], B_C_KLOOP[8], C_S2_PARITY[6], C_WGRAD[2]]
ALL_CASES = (FAMILY_A + B_MK + B_FWD_ONLY + B_C_LOADER + B_C_KLOOP + C_SMALL + C_STEM + C_1X1_S2 + C_S2_PARITY
             + C_WGRAD + FAMILY_D)
# two-plane families (module docstring): "alo" and "blo" on LO_AB (and on FAMILY_A's fwd / dgrad, C_WGRAD's
# wgrad), "both" on LO_BOTH (and on C_WGRAD's wgrad)
LO_AB = B_MK + B_FWD_ONLY + B_C_LOADER + B_C_KLOOP + C_SMALL + C_STEM + C_1X1_S2 + C_S2_PARITY + FAMILY_D
LO_BOTH = BOUNDARY_SIX + FAMILY_D
# the stem kernel (mx_conv2d_stem_x3): (N, H, W, cin, stride, pad), 7x7 -> 64 on cin real channels padded to 8
STEM_CASES = [(2, 33, 41, 3, 2, 3), (1, 23, 19, 4, 1, 2)]


def norm(c):
    if len(c) == 8:
        N, H, W, C, K, k, st, pd = c
        return (N, H, W, C, K, k, k, st, st, pd, pd)
    assert len(c) == 11
    return tuple(c)


def out_hw(c):
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    return (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1


# ---- integer operands and the float64 reference ---------------------------------------------------
X_MAX, W_MAX, DY_MAX = 2, 1, 2
FAMILIES = ("alo", "blo", "both")   # two-plane operand families (module docstring); "int" is the integer one
LO_STEP = 2.0 ** -10


def two_plane(g, shape, amax):
    """a + b * 2^-10 as f32 (12 significant bits: exact), a nonzero in -amax..amax, b in {-1, 0, 1}."""
    i = torch.randint(0, 6 * amax, shape, generator=g, dtype=torch.int32)   # one draw: (|a|, sign, b)
    a = (i // 6 + 1) * (i % 2 * 2 - 1)
    b = i // 2 % 3 - 1
    v = a.double() + b.double() * LO_STEP
    assert torch.equal(v.float().double(), v)
    return v.float()


def planes(v):
    """The RNE bf16 hi / lo planes of an f32 tensor (mx_common.h's split2), as float64."""
    v = v.float()
    hi = v.bfloat16().float()
    return hi.double(), (v - hi).bfloat16().double()


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def conv_fns(c):
    """float64 CPU fwd(x, w) -> NHWC z, dgrad(dy, w) -> NHWC dx, wgrad(dy, x) -> KCRS dw of a case's geometry
    (NHWC activations, KCRS weights; channel and batch counts are the operands')."""
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)

    def fwd(x, w):
        return F.conv2d(_nchw(x), w.double(), None, (sh, sw), (ph, pw)).permute(0, 2, 3, 1).contiguous()

    def dgrad(dy, w):
        shp = (dy.shape[0], w.shape[1], H, W)
        dx = torch.nn.grad.conv2d_input(shp, w.double(), _nchw(dy), (sh, sw), (ph, pw))
        return dx.permute(0, 2, 3, 1).contiguous()

    def wgrad(dy, x):
        shp = (dy.shape[3], x.shape[3], R, S)
        return torch.nn.grad.conv2d_weight(_nchw(x), shp, _nchw(dy), (sh, sw), (ph, pw)).contiguous()
    return {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad}


def three_products(conv, a, b):
    """What the bf16x3 kernels compute from f32 operands a, b in exact arithmetic: a_hi b_hi + a_lo b_hi
    + a_hi b_lo = conv(a, b) - conv(a_lo, b_lo) (hi + lo = operand, asserted), in float64."""
    (ah, al), (bh, bl) = planes(a), planes(b)
    assert torch.equal(ah + al, a.double()) and torch.equal(bh + bl, b.double())
    r = conv(a, b)
    if al.any() and bl.any():
        r = r - conv(al, bl)
    assert torch.equal(r.float().double(), r), "the reference is not representable in f32"
    return r


def lo_passes(c):
    """The passes a case runs with two-plane operands: no dgrad / wgrad entry for K % 8 != 0, and the
    wgrad of the big grids stays with the integer family (module docstring)."""
    if norm(c)[4] % 8:
        return ("fwd",)
    return ("fwd", "dgrad") if c in FAMILY_A else ("fwd", "dgrad", "wgrad")


@functools.lru_cache(maxsize=None)
def _operand_sets(c):
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    r = reference(c)
    g = torch.Generator().manual_seed(zlib.crc32(repr((norm(c), "two-plane")).encode()))
    ints = (r["x"].float(), r["w"].float(), r["dy"].float())
    return ints, (two_plane(g, (N, H, W, C), X_MAX), two_plane(g, (K, C, R, S), W_MAX),
                  two_plane(g, (N, Ho, Wo, K), DY_MAX))


def lo_operands(c, fam):
    """(a, b) f32 operands per pass of a two-plane family: fwd (x, w), dgrad (dy, w), wgrad (dy, x).
    The integer operands are the integer family's, the two-plane ones have a seed of their own."""
    (x1, w1, dy1), (x2, w2, dy2) = _operand_sets(c)
    return {"alo": {"fwd": (x2, w1), "dgrad": (dy2, w1), "wgrad": (dy2, x1)},
            "blo": {"fwd": (x1, w2), "dgrad": (dy1, w2), "wgrad": (dy1, x2)},
            "both": {"fwd": (x2, w2), "dgrad": (dy2, w2), "wgrad": (dy2, x2)}}[fam]


def _lo_reference(c, fam):
    r = reference(c)
    ops, conv = lo_operands(c, fam), conv_fns(c)
    out = {"b": r["b"], "ry": r["ry"], "rx": r["rx"], "x": ops["fwd"][0], "w": ops["fwd"][1], "dy": ops["dgrad"][0],
           "xw": ops["wgrad"][1]}
    assert ops["dgrad"][1] is ops["fwd"][1] and ops["wgrad"][0] is ops["dgrad"][0]
    for p, name in (("fwd", "z"), ("dgrad", "dx"), ("wgrad", "dw")):
        if p in lo_passes(c):
            out[name] = three_products(conv[p], *ops[p]).float()
    # a 64-row BN partial of multiples of 2^-10 is exact when this holds
    out["sum_exact"] = 64 * out["z"].abs().max().item() * 2 ** 10 < 2 ** 24
    return out


def reference(c, fam="int"):
    return _reference(c, fam)   # one cache entry per (case, family), however the family is passed


@functools.lru_cache(maxsize=None)
def _reference(c, fam):
    """Seeded integer operands (int8, NHWC) and torch's float64 CPU conv / input gradient / weight
    gradient on them, kept as float32 (exact: every magnitude is asserted below 2^24). fam: a
    two-plane family instead (f32 operands; "xw" is the x of the wgrad, "sum_exact" whether the BN
    sum row is an equality)."""
    if fam != "int":
        return _lo_reference(c, fam)
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    g = torch.Generator().manual_seed(zlib.crc32(repr(norm(c)).encode()))
    nz = torch.tensor([-2, -1, 1, 2], dtype=torch.int8)
    x = torch.randint(-X_MAX, X_MAX + 1, (N, H, W, C), generator=g, dtype=torch.int8)  # a fifth are zeros
    w = (torch.randint(0, 2, (K, C, R, S), generator=g, dtype=torch.int8) * 2 - 1)
    b = torch.randint(-3, 4, (K,), generator=g, dtype=torch.int8)
    dy = nz[torch.randint(0, 4, (N, Ho, Wo, K), generator=g)]
    ry = nz[torch.randint(0, 4, (N, Ho, Wo, K), generator=g)]  # residual of the forward epilogue
    rx = nz[torch.randint(0, 4, (N, H, W, C), generator=g)]    # residual of the dgrad epilogue
    xn, wd, dyn = x.double().permute(0, 3, 1, 2), w.double(), dy.double().permute(0, 3, 1, 2)
    z = F.conv2d(xn, wd, None, (sh, sw), (ph, pw)).permute(0, 2, 3, 1).contiguous()
    dx = torch.nn.grad.conv2d_input(xn.shape, wd, dyn, (sh, sw), (ph, pw)).permute(0, 2, 3, 1).contiguous()
    dw = torch.nn.grad.conv2d_weight(xn, wd.shape, dyn, (sh, sw), (ph, pw)).contiguous()
    assert z.shape == (N, Ho, Wo, K) and dx.shape == (N, H, W, C) and dw.shape == (K, C, R, S)
    mags = {"z": z.abs().max().item(), "dx": dx.abs().max().item(), "dw": dw.abs().max().item(),
            "zcol64": 64 * z.abs().max().item()}
    assert max(mags.values()) + 8 < 2 ** 24, mags
    return {"x": x, "w": w, "b": b, "dy": dy, "ry": ry, "rx": rx, "z": z.float(), "dx": dx.float(), "dw": dw.float(),
            "mags": mags, "xw": x, "sum_exact": True}


def on_device(c, dev, fam="int"):
    return _on_device(c, dev, fam)


@functools.lru_cache(maxsize=None)
def _on_device(c, dev, fam):
    r = reference(c, fam)
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in r.items()}


def lo_runs():
    """(case, family, passes) of every launch set the two-plane tests below make (their parametrize lists)."""
    runs = [(c, fam) for c in LO_AB + FAMILY_A for fam in ("alo", "blo")]
    runs += [(c, "both") for c in LO_BOTH]
    runs += [(c, fam) for c in C_WGRAD for fam in FAMILIES]
    return [(c, fam, lo_passes(c)) for c, fam in dict.fromkeys(runs)]


def lo_evidence(conv, count, a, b):
    """CPU evidence for one pass of a two-plane case, reduction by `conv` of operands a, b:
    bound  max over outputs of sum |terms| of the three products, from convs of the planes' absolute values
    share  of the outputs that receive a term (count > 0), the share whose reference changes when the lo
           planes are zeroed
    mean_len  mean number of terms of those outputs."""
    (ah, al), (bh, bl) = planes(a), planes(b)
    for hi, lo in ((ah, al), (bh, bl)):   # the plane contract
        assert torch.equal(hi, hi.round()) and ((lo == 0) | (lo.abs() == LO_STEP)).all()
    assert torch.equal(ah + al, a.double()) and torch.equal(bh + bl, b.double())

    def cz(u, v):  # a zero plane contributes nothing
        return conv(u, v) if u.any() and v.any() else 0.0
    bound = (conv(ah.abs() + al.abs(), bh.abs()) + cz(ah.abs(), bl.abs())).max().item()
    differs = (cz(al, bh) + cz(ah, bl)) != 0
    sup = (count > 0).expand_as(differs)
    return {"bound": bound, "share": differs[sup].double().mean().item(), "mean_len": count[count > 0].mean().item(),
            "unsupported_differ": bool(differs[~sup].any())}


def term_counts(c):
    """Per pass, the number of terms each output element receives (broadcastable to the output)."""
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    conv, k1 = conv_fns(c), torch.ones(1, 1, R, S)
    return {"fwd": conv["fwd"](torch.ones(1, H, W, 1), k1) * C,
            "dgrad": conv["dgrad"](torch.ones(1, Ho, Wo, 1), k1) * K,
            "wgrad": conv["wgrad"](torch.ones(1, Ho, Wo, 1), torch.ones(1, H, W, 1)) * N}


def assert_lo_evidence(tag, conv, count, a, b):
    """The exactness bound and the teeth of one two-plane pass (see lo_evidence)."""
    e = lo_evidence(conv, count, a, b)
    assert (e["bound"] + 8) * 2 ** 10 < 2 ** 24, (tag, e)   # + 8: the integer bias and residual of the epilogues
    assert not e["unsupported_differ"], (tag, e)
    if e["mean_len"] >= 8:
        assert e["share"] >= 0.5, (tag, e)
    else:
        assert e["share"] > 0, (tag, e)
    return e


def exactness_bounds(c):
    """The issue's bounds: |x|max |w|max Kdim < 2^24 (fwd), the dgrad and wgrad analogues."""
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    return {"fwd": X_MAX * W_MAX * R * S * C + 3 + DY_MAX, "dgrad": DY_MAX * W_MAX * R * S * K + DY_MAX,
            "wgrad": DY_MAX * X_MAX * N * Ho * Wo}


def test_table_shapes_and_exactness_bounds():
    """CPU only: every listed shape has a positive output map, satisfies the exactness bounds (so that
    any f32 summation order is exact) and its float64 reference stays below 2^24 in magnitude."""
    assert len(set(ALL_CASES)) == len(ALL_CASES)
    for c in ALL_CASES:
        N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
        Ho, Wo = out_hw(c)
        assert Ho > 0 and Wo > 0, c
        assert C % 8 == 0, c
        for name, v in exactness_bounds(c).items():
            assert v < 2 ** 24, (c, name, v)
    for c in ALL_CASES:
        m = reference(c)["mags"]  # reference() asserts the magnitudes
        b = exactness_bounds(c)
        assert m["z"] <= b["fwd"] and m["dx"] <= b["dgrad"] and m["dw"] <= b["wgrad"], (c, m, b)
    for t in (A_FWD, A_DGRAD):
        assert set(t) == set(FAMILY_A)
    assert set(B_FWD) == set(B_MK)


@functools.lru_cache(maxsize=None)
def stem_reference(sc, fam):
    """Operands (x zero-padded to 8 channels, w on the cin real ones, integer bias) and the float64
    three-product conv of a stem case in a two-plane family."""
    N, H, W, cin, st, pd = sc
    c = (N, H, W, cin, 64, 7, st, pd)
    g = torch.Generator().manual_seed(zlib.crc32(repr((sc, "stem")).encode()))
    x1 = torch.randint(-X_MAX, X_MAX + 1, (N, H, W, cin), generator=g).float()
    w1 = (torch.randint(0, 2, (64, cin, 7, 7), generator=g) * 2 - 1).float()
    b = torch.randint(-3, 4, (64,), generator=g).float()
    x2, w2 = two_plane(g, (N, H, W, cin), X_MAX), two_plane(g, (64, cin, 7, 7), W_MAX)
    x, w = {"alo": (x2, w1), "blo": (x1, w2), "both": (x2, w2)}[fam]
    z = three_products(conv_fns(c)["fwd"], x, w).float()
    xp = torch.zeros(N, H, W, 8)
    xp[..., :cin] = x
    return {"c": c, "x": xp, "xr": x, "w": w, "b": b, "z": z,
            "sum_exact": 64 * z.abs().max().item() * 2 ** 10 < 2 ** 24}


def test_two_plane_values():
    """CPU only: the plane contract of the two-plane values under the host's RNE split (the one
    test_split_pack_planes pins for the device pack): hi = a, lo = b * 2^-10, hi + lo = v, about two
    thirds of the lo plane nonzero; and three_products is the three-product sum, term by term."""
    g = torch.Generator().manual_seed(0)
    for amax in (W_MAX, X_MAX):
        v = two_plane(g, (4096,), amax)
        hi, lo = planes(v)
        assert torch.equal(hi, hi.round()) and hi.abs().min() >= 1 and hi.abs().max() == amax
        assert set((lo / LO_STEP).unique().tolist()) == {-1.0, 0.0, 1.0}
        assert torch.equal(hi + lo, v.double())
        assert 0.6 < (lo != 0).double().mean().item() < 0.73
    for s in (1.0, -1.0, 2.0, -2.0):      # every (a, b) pair, the RNE ties-free neighbours of a power of two included
        for b in (-1, 0, 1):
            hi, lo = planes(torch.tensor([s + b * LO_STEP]))
            assert hi.item() == s and lo.item() == b * LO_STEP, (s, b, hi, lo)
    c = BOUNDARY_SIX[2]
    for p, (a, b) in lo_operands(c, "both").items():
        conv = conv_fns(c)[p]
        (ah, al), (bh, bl) = planes(a), planes(b)
        assert torch.equal(three_products(conv, a, b), conv(ah, bh) + conv(al, bh) + conv(ah, bl)), p


def test_two_plane_bounds_and_teeth():
    """CPU only, for every case, pass and family the two-plane tests run (lo_runs, the stem cases):
    the plane contract of the operands, sum |terms| * 2^10 < 2^24 from convs of the planes' absolute
    values (any f32 summation order is then exact), the float64 reference round-trips through f32
    (three_products asserts it), and the teeth: of the outputs that receive a term, at least half
    differ from the reference with the lo planes zeroed where the mean reduction has 8 terms or more,
    and some do elsewhere (wgrad on 1- and 2-pixel maps)."""
    runs = lo_runs()
    # C_WGRAD[2] is one of BOUNDARY_SIX
    assert len(runs) == 2 * (len(LO_AB) + len(FAMILY_A)) + len(LO_BOTH) + 3 * len(C_WGRAD) - 1
    shares = {}
    for c, fam, passes in runs:
        reference(c, fam)   # asserts that the float64 results are representable in f32
        ops, conv, count = lo_operands(c, fam), conv_fns(c), term_counts(c)
        for p in passes:
            e = assert_lo_evidence((c, fam, p), conv[p], count[p], *ops[p])
            shares.setdefault((p, e["mean_len"] >= 8), []).append(e["share"])
    for sc in STEM_CASES:
        for fam in FAMILIES:
            r = stem_reference(sc, fam)
            e = assert_lo_evidence((sc, fam), conv_fns(r["c"])["fwd"], term_counts(r["c"])["fwd"], r["xr"], r["w"])
            assert e["mean_len"] >= 8
    assert all((p, True) in shares for p in ("fwd", "dgrad", "wgrad")) and ("wgrad", False) in shares, sorted(shares)


def test_workspace_sizes_on_host():
    """CPU only (mx_conv_workspace* are host code): every listed shape and pass gets a size that is a
    whole number of f32 slabs, stride-2 shapes with empty parity classes (H or W of 1) included."""
    for c in ALL_CASES:
        N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
        Ho, Wo = out_hw(c)
        for x3 in (False, True):
            assert _ws_bytes(c, 0, x3) % (4 * N * Ho * Wo * K) == 0, c
            if K % 8 == 0:
                b = _ws_bytes(c, 1, x3)
                assert b % (4 * C) == 0 and (sh > 1 or sw > 1 or b % (4 * N * H * W * C) == 0), c
                assert _ws_bytes(c, 2, x3) % (4 * K * R * S * C) == 0, c


# ---- launch helpers -------------------------------------------------------------------------------
def _ops(c, dev, x3, fam="int"):
    """Device operands of a case in the path's dtype and its packed weights."""
    from mx_det import conv as mc
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    assert x3 or fam == "int", "two-plane values need the bf16x3 path"
    d = on_device(c, dev, fam)
    dt = torch.float32 if x3 else torch.bfloat16
    wk, wt = mc.pack_weight(d["w"].float(), C, (sh, sw), (ph, pw), kpad=K, dgrad=K % 8 == 0, split=x3)
    return d, dt, wk, wt


def _rec():
    from mx_det import conv as mc
    return mc.last_launch()


def _tup(r):
    return (r["bmt"], r["bn"], r["splits"], r["tiles"], r["buf"], r["kind"])


def _shape(c):
    from mx_det import _lib
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    Ho, Wo = out_hw(c)
    return _lib.ConvShape(N, H, W, C, K, R, S, Ho, Wo, sh, sw, ph, pw)


def _ws_bytes(c, pass_, x3):
    from mx_det import _lib
    fn = _lib.load().mx_conv_workspace_x3 if x3 else _lib.load().mx_conv_workspace
    return fn(ctypes.byref(_shape(c)), pass_)


def check_fwd(c, dev, x3, expect=None, raw_record=True, fam="int"):
    """fwd with bias + BN statistics (f32 out), bias + residual + ReLU (bf16 out on the bf16 path),
    residual + LeakyReLU; returns the launch record of the first."""
    from mx_det import conv as mc
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    d, dt, wk, _ = _ops(c, dev, x3, fam)
    x, z, b = d["x"].to(dt), d["z"], d["b"].float()
    y, stats = mc.conv_fwd(x, wk, (sh, sw), (ph, pw), bias=b, out_dtype=torch.float32, stats=True)
    rec = _rec()
    assert rec["pass_"] == 0 and rec["launches"] == 1, rec
    if expect is not None:
        assert _tup(rec) == expect, (c, "fwd launch record", _tup(rec), "expected", expect)
    if raw_record:  # the split count launched is the one the workspace was sized for
        M = z.numel() // K
        assert _ws_bytes(c, 0, x3) == (4 * rec["splits"] * M * K if rec["splits"] > 1 else 0), (c, rec)
    assert y.dtype == torch.float32 and torch.equal(y, z + b), (c, "fwd f32")
    zz = z.reshape(-1, K).double()
    s = stats.double().sum(1)
    if d["sum_exact"]:
        assert torch.equal(s[0], zz.sum(0)), (c, "BN sum row")
    else:  # two-plane z too large for exact 64-row partials: test_gpu_x3.py's bar
        torch.testing.assert_close(s[0], zz.sum(0), rtol=0, atol=1e-5 * zz.abs().sum(0).max().item())
    sq = (zz * zz).sum(0)
    if x3:
        torch.testing.assert_close(s[1], sq, rtol=0, atol=1e-5 * sq.max().item())
    else:
        tol = 2e-5 * X_MAX * W_MAX * C * R * S
        torch.testing.assert_close(s[1], sq, rtol=1e-4, atol=tol * tol * 10 + 1e-3)
    if K % 8:
        yb = mc.conv_fwd(x, wk, (sh, sw), (ph, pw), bias=b, act=mc.ACT_RELU)
        assert torch.equal(yb, (z + b).clamp_min(0).to(dt)), (c, "fwd relu")
        return rec
    ry = d["ry"].to(dt)
    yb = mc.conv_fwd(x, wk, (sh, sw), (ph, pw), bias=b, residual=ry, act=mc.ACT_RELU)
    assert yb.dtype == dt and torch.equal(yb, (z + b + ry.float()).clamp_min(0).to(dt)), (c, "fwd residual relu")
    v = z + ry.float()
    yl = mc.conv_fwd(x, wk, (sh, sw), (ph, pw), residual=ry, act=mc.ACT_LEAKY, out_dtype=torch.float32)
    assert torch.equal(yl, torch.where(v > 0, v, v * 0.2)), (c, "fwd leaky")
    return rec


def _dgrad_raw(c, dev, x3, dy, wt, residual, bnb=None):
    """The dgrad entry on a NaN-filled dx (an element no class writes shows); returns (dx, part)."""
    from mx_det import _lib, conv as mc
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    s = _shape(c)
    dx = torch.full((N, H, W, C), float("nan"), dtype=dy.dtype, device=dev)
    wsb = _ws_bytes(c, 1, x3)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    p = mc._p
    mb = (N * H * W + 63) // 64
    part = torch.full((2, mb, C), float("nan"), device=dev) if bnb else None
    by, bz, bm, bi = bnb if bnb else (None, None, None, None)
    if x3:
        _lib.call("mx_conv2d_dgrad_x3", ctypes.byref(s), p(dy), p(wt), p(residual), p(dx), p(by), p(bz), p(bm), p(bi),
                  1 if bnb else 0, p(part), mb, p(ws), wsb, mc._s())
    elif bnb:
        _lib.call("mx_conv2d_dgrad_bnb", ctypes.byref(s), p(dy), p(wt), p(residual), p(dx), p(by), p(bz), p(bm), p(bi),
                  1, p(part), mb, p(ws), wsb, mc._s())
    elif residual is None:
        _lib.call("mx_conv2d_dgrad_t", ctypes.byref(s), p(dy), p(wt), p(dx), p(ws), wsb, mc._s())
    else:
        _lib.call("mx_conv2d_dgrad_ex", ctypes.byref(s), p(dy), p(wt), p(residual), p(dx), p(ws), wsb, mc._s())
    return dx, part


def check_dgrad(c, dev, x3, expect=None, fam="int"):
    """dgrad_t and dgrad_ex (+ residual) into NaN-filled outputs; returns the last launch record."""
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    d, dt, _, wt = _ops(c, dev, x3, fam)
    dy, rx = d["dy"].to(dt), d["rx"].to(dt)
    dx, _ = _dgrad_raw(c, dev, x3, dy, wt, None)
    rec = _rec()
    assert rec["pass_"] == 1, rec
    # one launch per non-empty stride-parity class; an empty class has no rows to write
    assert rec["launches"] == min(sh, H) * min(sw, W), (c, rec)
    if expect is not None:
        assert _tup(rec) == expect, (c, "dgrad launch record", _tup(rec), "expected", expect)
    if sh == 1 and sw == 1:
        assert _ws_bytes(c, 1, x3) == (4 * rec["splits"] * N * H * W * C if rec["splits"] > 1 else 0), (c, rec)
    assert torch.equal(dx, d["dx"].to(dt)), (c, "dgrad")
    dx, _ = _dgrad_raw(c, dev, x3, dy, wt, rx)
    assert torch.equal(dx, (d["dx"] + rx.float()).to(dt)), (c, "dgrad + residual")
    return rec


def check_wgrad(c, dev, x3, fam="int"):
    from mx_det import conv as mc
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    assert x3 or fam == "int"
    d = on_device(c, dev, fam)
    dt = torch.float32 if x3 else torch.bfloat16
    dw = mc.conv_wgrad(d["dy"].to(dt), d["xw"].to(dt), K, R, S, (sh, sw), (ph, pw))
    rec = _rec()
    assert rec["pass_"] == 2, rec
    assert (_ws_bytes(c, 2, x3) > 0) == (rec["splits"] > 1), (c, rec)
    assert torch.equal(dw, d["dw"]), (c, "wgrad", rec)
    return rec


@pytest.fixture
def fixed(monkeypatch):
    """The library's own dispatch: no per-shape tuner, every knob at its default (and restored)."""
    from mx_det import _lib
    monkeypatch.setenv("MX_CONV_TUNE", "0")
    old, oldw = _lib.load().mx_conv_get_variant(), _lib.load().mx_conv_get_wgrad_variant()

    def defaults():
        _lib.call("mx_conv_set_variant", 7)
        _lib.call("mx_conv_set_loader", 1)
        _lib.call("mx_conv_set_wgrad_variant", 3)
        _lib.call("mx_conv_set_wgrad_target", 0)
        _lib.call("mx_conv_set_tile", 0, 0)
        _lib.call("mx_conv_set_max_splits", 0)
        _lib.call("mx_conv_set_stages", 0)
    defaults()
    try:
        yield _lib
    finally:
        defaults()
        _lib.call("mx_conv_set_variant", old)
        _lib.call("mx_conv_set_wgrad_variant", oldw)


def _all_passes(c, dev, x3, fwd_expect=None, dgrad_expect=None, fam="int"):
    K = norm(c)[4]
    recs = {"fwd": check_fwd(c, dev, x3, fwd_expect, fam=fam)}
    if K % 8 == 0:
        recs["dgrad"] = check_dgrad(c, dev, x3, dgrad_expect, fam=fam)
        if fam == "int" or "wgrad" in lo_passes(c):
            recs["wgrad"] = check_wgrad(c, dev, x3, fam)
    return recs


# ---- A. big grids ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", FAMILY_A)
def test_big_grid_bf16(dev, fixed, c):
    """Default dispatch of the bf16 path on the grids the full-size step selects: the tile pick is
    asserted, then fwd (f32 / bf16 out, bias, residual, ReLU, LeakyReLU, stats), dgrad_t / dgrad_ex
    and wgrad are exact."""
    assert torch.cuda.get_device_properties(dev).multi_processor_count == 256, "the picks are for 256 CUs"
    recs = _all_passes(c, dev, False, A_FWD[c], A_DGRAD[c])
    assert recs["wgrad"]["buf"] == 1 and recs["wgrad"]["kind"] == 3, recs["wgrad"]


@pytest.mark.gpu
def test_big_grid_picks_cover_every_tile(dev, fixed):
    """Across family A each unsplit big-grid tile of make_geo's candidate loop is launched: 128x256,
    128x128, 128x64 and 64x128 on >= 320 tiles, and launch_kind's BK64x2 choice."""
    from mx_det import conv as mc
    seen = set()
    for c in FAMILY_A:
        N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
        d, dt, wk, _ = _ops(c, dev, False)
        mc.conv_fwd(d["x"].to(dt), wk, (sh, sw), (ph, pw))
        r = _rec()
        if r["splits"] == 1 and r["tiles"] >= 320:
            seen.add((r["bmt"], r["bn"]))
        if r["kind"] == 4:
            seen.add("kind4")
    assert seen >= {(128, 256), (128, 128), (128, 64), (64, 128), "kind4"}, seen


@pytest.mark.gpu
@pytest.mark.parametrize("c", FAMILY_A)
def test_big_grid_x3(dev, fixed, c):
    """The same grids through the bf16x3 entries (128x128 / 128x64 tiles at two rounds and more)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    recs = _all_passes(c, dev, True)
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    M = N * out_hw(c)[0] * out_hw(c)[1]
    t128 = -(-M // 128) * -(-K // (64 if K <= 64 else 128))
    assert recs["fwd"]["bmt"] == (128 if t128 >= 2 * cus else 64) and recs["fwd"]["splits"] == 1, recs["fwd"]
    assert recs["fwd"]["kind"] == 100 and recs["wgrad"]["kind"] == 103


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
def test_big_grid_dgrad_bn_partials(dev, fixed, x3):
    """dgrad with the BN-backward epilogue on the 128x64 narrow big grid: dx stays exact and the
    per-64-row partials of g = dx * act'(y) and g * (z - mean) * invstd (integer mean, invstd 0.5:
    exact products) meet test_gpu_x3.py's bar."""
    c = FAMILY_A[2]
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    d, dt, _, wt = _ops(c, dev, x3)
    g = torch.Generator().manual_seed(5)
    zb = torch.randint(-3, 4, (N, H, W, C), generator=g).float()
    yb = (zb + 1).clamp_min(0)
    mean = torch.randint(-1, 2, (C,), generator=g).float()
    invstd = torch.full((C,), 0.5)
    bnb = tuple(t.to(dev) for t in (yb.to(dt), zb.to(dt), mean, invstd))
    dx, part = _dgrad_raw(c, dev, x3, d["dy"].to(dt), wt, d["rx"].to(dt), bnb)
    ref = (d["dx"] + d["rx"].float()).to(dt)
    assert torch.equal(dx, ref)
    gg = ref.double().reshape(-1, C) * (yb.to(dev).reshape(-1, C) > 0).double()
    xh = (zb.to(dev).reshape(-1, C).double() - mean.to(dev).double()) * 0.5
    rows = torch.arange(gg.shape[0], device=dev) // 64
    mb = part.shape[1]
    s0 = torch.zeros(mb, C, dtype=torch.float64, device=dev).index_add_(0, rows, gg)
    s1 = torch.zeros(mb, C, dtype=torch.float64, device=dev).index_add_(0, rows, gg * xh)
    torch.testing.assert_close(part[0].double(), s0, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(part[1].double(), s1, rtol=1e-5, atol=1e-4)


# ---- B. tile and K-loop boundaries ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("c", B_MK)
def test_tile_boundaries(dev, fixed, x3, c, fam="int"):
    """M around 64 / 128 rows x Ncol around 64 (narrow), 128 and 256."""
    recs = _all_passes(c, dev, x3, None if x3 else B_FWD[c], fam=fam)
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    if not x3:  # dgrad: Ncol = 64 narrow, Kdim = K: the buffer loader exactly when K % 32 == 0
        assert recs["dgrad"]["bn"] == 64 and recs["dgrad"]["buf"] == int(K % 32 == 0), recs["dgrad"]
        assert recs["dgrad"]["kind"] == (3 if K % 32 == 0 else 8), recs["dgrad"]


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("c", B_FWD_ONLY)
def test_odd_output_channels_fwd(dev, fixed, x3, c, fam="int"):
    """K % 8 != 0 (no residual, no split-K, scalar epilogue stores)."""
    rec = check_fwd(c, dev, x3, fam=fam)
    assert rec["splits"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("c", B_C_LOADER)
def test_loader_switch_on_channels(dev, fixed, x3, c, fam="int"):
    """C % 32 and Kdim % 32 select the buffer-descriptor or the per-lane loader (3x3 on a 5x6 map)."""
    recs = _all_passes(c, dev, x3, fam=fam)
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    assert recs["fwd"]["buf"] == int(C % 32 == 0), recs["fwd"]
    assert recs["dgrad"]["buf"] == int(K % 32 == 0), recs["dgrad"]
    if not x3:
        assert recs["fwd"]["kind"] == (3 if C % 32 == 0 else 8), recs["fwd"]


# fwd splits launched at C = 440 .. 1032 (4 tiles of 64x128: min(nk / 4, 16) once nk >= 8 64-wide K-tiles)
B_KLOOP_SPLITS = {440: 1, 448: 1, 456: 2, 504: 2, 512: 2, 520: 2, 1016: 4, 1024: 4, 1032: 4}


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("c", B_C_KLOOP)
def test_k_loop_boundaries(dev, fixed, x3, c, fam="int"):
    """nk 7 / 8 (split-K off / on) and 15 / 16 in 64- and 32-wide K-tiles, with kt_per_split remainders."""
    recs = _all_passes(c, dev, x3, fam=fam)
    C = norm(c)[3]
    f = recs["fwd"]
    assert (f["bmt"], f["bn"], f["tiles"]) == (64, 128, 4), f
    assert f["buf"] == int(C % 32 == 0), f
    if x3:  # 32-wide K-tiles: nk = ceil(C / 32) >= 8 everywhere here
        nk = -(-C // 32)
        sp = min(160, nk // 4, 16)
        assert f["splits"] == -(-nk // -(-nk // sp)), f
    else:
        assert f["splits"] == B_KLOOP_SPLITS[C], f


# ---- C. spatial edges -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("c", C_SMALL + C_STEM + C_1X1_S2 + C_S2_PARITY)
def test_spatial_edges(dev, fixed, x3, c, fam="int"):
    """Maps smaller than the filter, single rows / columns, stride-2 parity classes that are empty
    (H = 1 or W = 1: skipped on the host, dx still fully written) or of unequal shape."""
    _all_passes(c, dev, x3, fam=fam)


@pytest.mark.gpu
@pytest.mark.parametrize("wv", [0, 1, 2, 3, 103, 104, 105])
@pytest.mark.parametrize("c", C_WGRAD)
def test_wgrad_pixel_walk(dev, fixed, wv, c, fam="int"):
    """Every wgrad kernel on output maps of 2 .. 65 pixels, one and five images: the buffer kernel
    (variant 3) runs from 32 pixels per map on and hands smaller maps to the register kernel."""
    x3 = wv >= 100
    fixed.call("mx_conv_set_wgrad_variant", wv % 100)
    rec = check_wgrad(c, dev, x3, fam)
    px = out_hw(c)[0] * out_hw(c)[1]
    if x3:
        assert rec["kind"] == wv, rec
    elif wv == 3:
        assert (rec["kind"], rec["buf"]) == ((3, 1) if px >= 32 else (0, 0)), (px, rec)
    else:
        assert (rec["kind"], rec["buf"]) == (wv, 0), rec


# ---- D. asymmetric geometry -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("c", FAMILY_D)
def test_asymmetric_geometry(dev, fixed, x3, c, fam="int"):
    """stride_h != stride_w, pad_h != pad_w, R != S: fwd, dgrad and wgrad on both paths."""
    _all_passes(c, dev, x3, fam=fam)


# ---- tuner candidates -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(13))
@pytest.mark.parametrize("c", FAMILY_A + BOUNDARY_SIX)
def test_tuner_candidates_exact(dev, monkeypatch, ci, c):
    """Every launch configuration of the per-shape tuner (_FD_CANDS, _WG_CANDS and their bf16x3
    lists) on the big grids and on six boundary shapes: as the only candidate, it is what runs."""
    from mx_det import conv as mc
    fd, wg = mc._FD_CANDS[ci % len(mc._FD_CANDS)], mc._WG_CANDS[ci % len(mc._WG_CANDS)]
    fd3, wg3 = mc._FD_CANDS_X3[ci % len(mc._FD_CANDS_X3)], mc._WG_CANDS_X3[ci % len(mc._WG_CANDS_X3)]
    monkeypatch.setenv("MX_CONV_TUNE", "1")
    monkeypatch.setattr(mc, "_tune_cache", {})
    monkeypatch.setattr(mc, "_FD_CANDS", (fd,))
    monkeypatch.setattr(mc, "_WG_CANDS", (wg,))
    monkeypatch.setattr(mc, "_FD_CANDS_X3", (fd3,))
    monkeypatch.setattr(mc, "_WG_CANDS_X3", (wg3,))
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    for x3, f, g in ((False, fd, wg), (True, fd3, wg3)):
        rec = check_fwd(c, dev, x3, raw_record=False)
        if f[0]:  # a forced block tile is the one launched (bf16 kernels cap the rows at 128)
            assert rec["bmt"] in (min(f[0], 128), f[0]) and rec["bn"] == min(f[1], 128 if x3 else 256), (f, rec)
        if f[2]:
            assert rec["splits"] <= f[2], (f, rec)
        d, dt, _, wt = _ops(c, dev, x3)
        dx = mc.conv_dgrad(d["dy"].to(dt), wt, (N, H, W, C), R, S, (sh, sw), (ph, pw), residual=d["rx"].to(dt))
        assert torch.equal(dx, (d["dx"] + d["rx"].float()).to(dt)), (c, "dgrad", f)
        dw = mc.conv_wgrad(d["dy"].to(dt), d["x"].to(dt), K, R, S, (sh, sw), (ph, pw))
        rec = _rec()
        assert torch.equal(dw, d["dw"]), (c, "wgrad", g, rec)
        px = out_hw(c)[0] * out_hw(c)[1]
        want = 100 + g[0] if x3 else (0 if g[0] == 3 and px < 32 and px > 1 else g[0])
        assert rec["kind"] == want, (g, rec)


# ---- two-plane operand families (bf16x3 only) -----------------------------------------------------
# The launches above with nonzero lo planes (module docstring): each test runs the body of its integer
# counterpart, launch-record assertions included, on a two-plane family's operands and reference.
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", B_MK)
def test_tile_boundaries_lo(dev, fixed, fam, c):
    test_tile_boundaries(dev, fixed, True, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", B_FWD_ONLY)
def test_odd_output_channels_fwd_lo(dev, fixed, fam, c):
    test_odd_output_channels_fwd(dev, fixed, True, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", B_C_LOADER)
def test_loader_switch_on_channels_lo(dev, fixed, fam, c):
    test_loader_switch_on_channels(dev, fixed, True, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", B_C_KLOOP)
def test_k_loop_boundaries_lo(dev, fixed, fam, c):
    test_k_loop_boundaries(dev, fixed, True, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", C_SMALL + C_STEM + C_1X1_S2 + C_S2_PARITY)
def test_spatial_edges_lo(dev, fixed, fam, c):
    test_spatial_edges(dev, fixed, True, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", FAMILY_D)
def test_asymmetric_geometry_lo(dev, fixed, fam, c):
    test_asymmetric_geometry(dev, fixed, True, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("c", LO_BOTH)
def test_both_planes(dev, fixed, c):
    """Both operands two-plane on the six boundary shapes and the asymmetric family: the result is
    conv(a, b) - conv(a_lo, b_lo), the three products and no other, under the RNE split."""
    _all_passes(c, dev, True, fam="both")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("wv", [103, 104, 105])
@pytest.mark.parametrize("c", C_WGRAD)
def test_wgrad_pixel_walk_lo(dev, fixed, wv, c, fam):
    """The bf16x3 wgrad kernels, the wide blocks (104, 105) included, on maps of 2 .. 65 pixels."""
    test_wgrad_pixel_walk(dev, fixed, wv, c, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["alo", "blo"])
@pytest.mark.parametrize("c", FAMILY_A)
def test_big_grid_x3_lo(dev, fixed, fam, c):
    """fwd and dgrad of the big grids (test_big_grid_x3's tile assertions). Their wgrad reduces over up
    to 128,000 pixels, past the exactness bound with 2^-10 steps: it stays with the integer family."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    recs = _all_passes(c, dev, True, fam=fam)
    assert set(recs) == {"fwd", "dgrad"}
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    M = N * out_hw(c)[0] * out_hw(c)[1]
    t128 = -(-M // 128) * -(-K // (64 if K <= 64 else 128))
    assert recs["fwd"]["bmt"] == (128 if t128 >= 2 * cus else 64) and recs["fwd"]["splits"] == 1, recs["fwd"]
    assert recs["fwd"]["kind"] == 100


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(13))
@pytest.mark.parametrize("c", BOUNDARY_SIX)
def test_tuner_candidates_exact_lo(dev, monkeypatch, ci, c):
    """Every bf16x3 launch configuration of the per-shape tuner as the only candidate, both operands
    two-plane, on the six boundary shapes (test_tuner_candidates_exact's bf16x3 half)."""
    from mx_det import conv as mc
    f, g = mc._FD_CANDS_X3[ci % len(mc._FD_CANDS_X3)], mc._WG_CANDS_X3[ci % len(mc._WG_CANDS_X3)]
    monkeypatch.setenv("MX_CONV_TUNE", "1")
    monkeypatch.setattr(mc, "_tune_cache", {})
    monkeypatch.setattr(mc, "_FD_CANDS_X3", (f,))
    monkeypatch.setattr(mc, "_WG_CANDS_X3", (g,))
    N, H, W, C, K, R, S, sh, sw, ph, pw = norm(c)
    rec = check_fwd(c, dev, True, raw_record=False, fam="both")
    if f[0]:
        assert rec["bmt"] in (min(f[0], 128), f[0]) and rec["bn"] == min(f[1], 128), (f, rec)
    if f[2]:
        assert rec["splits"] <= f[2], (f, rec)
    d, dt, _, wt = _ops(c, dev, True, "both")
    dx = mc.conv_dgrad(d["dy"], wt, (N, H, W, C), R, S, (sh, sw), (ph, pw), residual=d["rx"].to(dt))
    assert torch.equal(dx, d["dx"] + d["rx"].float()), (c, "dgrad", f)
    dw = mc.conv_wgrad(d["dy"], d["xw"], K, R, S, (sh, sw), (ph, pw))
    rec = _rec()
    assert torch.equal(dw, d["dw"]), (c, "wgrad", g, rec)
    assert rec["kind"] == 100 + g[0], (g, rec)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("sc", STEM_CASES)
def test_stem_kernel_exact(dev, fixed, monkeypatch, sc, fam):
    """mx_conv2d_stem_x3 (its own walk of K: 7 filter rows of 8 taps x 4 channels) with bias, ReLU and
    statistics on two-plane operands: equal to float64, and to the generic bf16x3 kernels on the same
    packed operands."""
    from mx_det import conv as mc
    N, H, W, cin, st, pd = sc
    r = stem_reference(sc, fam)
    x, b, z = r["x"].to(dev), r["b"].to(dev), r["z"].to(dev)
    wk, _ = mc.pack_weight(r["w"].to(dev), 8, (st, st), (pd, pd), split=True)
    monkeypatch.setenv("MX_STEM_KERNEL", "1")
    y, stats = mc.conv_fwd(x, wk, (st, st), (pd, pd), bias=b, act=mc.ACT_RELU, stats=True, cin=cin)
    assert torch.equal(y, (z + b).clamp_min(0)), (sc, fam, "stem kernel")
    zz = z.reshape(-1, 64).double()
    s, sq = stats.double().sum(1), (zz * zz).sum(0)
    if r["sum_exact"]:
        assert torch.equal(s[0], zz.sum(0)), (sc, fam, "BN sum row")
    else:
        torch.testing.assert_close(s[0], zz.sum(0), rtol=0, atol=1e-5 * zz.abs().sum(0).max().item())
    torch.testing.assert_close(s[1], sq, rtol=0, atol=1e-5 * sq.max().item())
    monkeypatch.setenv("MX_STEM_KERNEL", "0")
    y0 = mc.conv_fwd(x, wk, (st, st), (pd, pd), bias=b, act=mc.ACT_RELU, cin=cin)
    assert torch.equal(y0, (z + b).clamp_min(0)) and torch.equal(y, y0), (sc, fam, "generic kernels")
