"""Corruption augmentation (drop-in for scripts/augmentations.py) executed by the HIP kernels.

Same constants and call surface as the reference (augmentations.py:14-98):
  NOISE_SIGMA = 15, BLUR_KERNEL = 9, BLUR_ANGLE_DEG = 0, DOWNSCALE_FACTOR = 0.5
  apply_noise / apply_motion_blur (any kernel size and angle) / apply_lowres on HxWx3 uint8 numpy
  arrays, _apply_random_corruption, RandomCorruption(p) as a PIL transform that corrupts the BGR view
  of the RGB image like the reference (augmentations.py:72-74), patch_ultralytics_augmentations().
apply_noise draws its field with np.random.normal(0, sigma, shape) exactly like the reference, so a
seeded numpy stream reproduces the reference output bit for bit; the add/clip/truncate runs on
device. RandomCorruptionGPU is the training-loop form: uint8 HWC device tensors in and out, the noise
field from the on-device Philox generator, never leaving HBM.
SEVERITY gives every corruption five levels (level 3 = the constants above); severity_spec / env_severities
/ severity_variants and the `severities` parameter of RandomCorruptionGPU put them to use through
ops.corrupt_batch_u8 (one launch for a batch with its own kind and strength per image). Opt-in: with the
default (3,) every call and every random draw is the one without it.
Night, haze and rain (WEATHER_KINDS; this project's own definitions, include/mx_det.h) are three more
opt-in kinds with five levels each: apply_night / apply_haze / apply_rain on numpy images, and the names
in MX_CORRUPTIONS / MX_EXTRA_VARIANTS; they run through ops.weather_batch_u8 / ops.corrupt_batch_u8.
"""
import random

import numpy as np
import torch

from . import ops

NOISE_SIGMA = 15
BLUR_KERNEL = 9
BLUR_ANGLE_DEG = 0
DOWNSCALE_FACTOR = 0.5
JPEG_QUALITY = 15  # ImageNet-C's middle severity of its JPEG corruption; a constant of this project
JPEG_SUBSAMPLING = 2  # 4:2:0, PIL's default for that quality

DEFAULT_KINDS = ("noise", "blur", "lowres")  # the reference's corruptions
WEATHER_KINDS = ("night", "haze", "rain")  # mx_weather_batch_u8's ops
KINDS = DEFAULT_KINDS + ("jpeg",) + WEATHER_KINDS


def check_kinds(kinds):
    """kinds as a tuple; ValueError for an empty choice or a name that is no corruption."""
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in KINDS]
    if bad or not kinds:
        raise ValueError(f"corruption kinds must be a non-empty choice of {', '.join(KINDS)}; got {list(kinds)}")
    return kinds


def env_kinds(value=None):
    """The corruption kinds of a training run: `value`, or MX_CORRUPTIONS, a comma-separated list
    (default noise,blur,lowres)."""
    import os
    value = os.environ.get("MX_CORRUPTIONS", "") if value is None else value
    if isinstance(value, str):
        value = [k.strip() for k in value.split(",") if k.strip()] or DEFAULT_KINDS
    return check_kinds(value)


EXTRA_VARIANTS = {"jpeg": ("Test_JPEG", "JPEG"), "night": ("Test_Night", "Night"), "haze": ("Test_Haze", "Haze"),
                  "rain": ("Test_Rain", "Rain")}  # name -> (test-set variant, its short name)


def env_extra_variants(value=None):
    """Test-set variants beyond the reference's four, as [(variant, short name)]: `value`, or
    MX_EXTRA_VARIANTS, a comma-separated list (default empty; the names are jpeg, night, haze, rain)."""
    import os
    value = os.environ.get("MX_EXTRA_VARIANTS", "") if value is None else value
    names = [k.strip() for k in value.split(",") if k.strip()] if isinstance(value, str) else list(value)
    bad = [k for k in names if k not in EXTRA_VARIANTS]
    if bad:
        raise ValueError(f"MX_EXTRA_VARIANTS names {', '.join(EXTRA_VARIANTS)} only; got {bad}")
    return [EXTRA_VARIANTS[k] for k in dict.fromkeys(names)]


# Severity levels 1..5 of every corruption; constants of this project. Level 3 is the reference's
# setting in every row it has one for (NOISE_SIGMA, BLUR_KERNEL, DOWNSCALE_FACTOR, JPEG_QUALITY); the JPEG row
# is ImageNet-C's five qualities. Night, haze and rain are this project's own ops and rows.
SEVERITY_LEVELS = (1, 2, 3, 4, 5)
DEFAULT_SEVERITIES = (3,)
SEVERITY = {
    "noise": (5, 10, 15, 25, 40),                    # sigma
    "blur": (5, 7, 9, 13, 17),                       # kernel size k, at BLUR_ANGLE_DEG
    "lowres": (0.75, 0.625, 0.5, 0.375, 0.25),       # down-scale factor
    "jpeg": (25, 18, 15, 10, 7),                     # quality
    "night": ((0.6, 0.1, 2), (0.45, 0.15, 3), (0.3, 0.25, 4), (0.2, 0.4, 6), (0.12, 0.6, 8)),  # gain, shot, read
    "haze": ((0.10, 0.35), (0.20, 0.50), (0.30, 0.65), (0.40, 0.78), (0.50, 0.90)),            # alpha lo, hi
    "rain": ((131, 9, 110), (262, 13, 130), (393, 17, 150), (590, 23, 170), (786, 31, 190)),   # thr, len, beta
}
HAZE_AIR = 235    # the airlight every haze level blends towards
RAIN_SLANT = 2    # columns per 8 rows of streak; fade = 256 // len
KIND_VARIANTS = {"noise": ("Test_Noise", "Noise"), "blur": ("Test_Blur", "Blur"), "lowres": ("Test_LowRes", "LowRes"),
                 **EXTRA_VARIANTS}  # kind -> (its level-3 test-set variant, short name)


def check_severities(levels):
    """levels as a tuple of ints; ValueError for an empty choice or a level outside 1..5."""
    try:
        out = tuple(int(v) for v in levels)
        bad = [v for v, o in zip(levels, out) if o not in SEVERITY_LEVELS or float(v) != o]
    except (TypeError, ValueError):
        out, bad = (), [levels]
    if bad or not out:
        raise ValueError(f"severities must be a non-empty choice of the levels 1..5; got {levels!r}")
    return out


def env_severities(value=None):
    """The severity levels of a run: `value`, or MX_SEVERITIES, a comma-separated list of levels 1..5
    (default 3, the reference's setting: every call and every random draw as without the switch)."""
    import os
    value = os.environ.get("MX_SEVERITIES", "") if value is None else value
    if isinstance(value, str):
        value = [k.strip() for k in value.split(",") if k.strip()] or DEFAULT_SEVERITIES
    elif isinstance(value, int):
        value = [value]
    return check_severities(value)


def severity_value(kind, level):
    """The strength of `kind` at `level`: sigma, kernel size, down-scale factor or JPEG quality; the
    SEVERITY row's tuple for night, haze and rain."""
    if kind not in SEVERITY or level not in SEVERITY_LEVELS:
        raise ValueError(f"no severity {level!r} of corruption {kind!r}")
    return SEVERITY[kind][level - 1]


_TAPS = {}


def _blur_taps(k, angle_deg=BLUR_ANGLE_DEG):
    if (k, angle_deg) not in _TAPS:
        _TAPS[(k, angle_deg)] = kernel_taps(motion_blur_kernel(k, angle_deg))
    return _TAPS[(k, angle_deg)]


def severity_spec(kind, level):
    """The ops.corrupt_batch_u8 spec of `kind` at `level`."""
    v = severity_value(kind, level)
    if kind == "noise":
        return ops.CorruptSpec(ops.CORRUPT_NOISE, float(v))
    if kind == "blur":
        return ops.CorruptSpec(ops.CORRUPT_BLUR, _blur_taps(v))
    if kind == "lowres":
        return ops.CorruptSpec(ops.CORRUPT_LOWRES, float(v))
    if kind == "night":
        gain, shot, read = v
        return ops.CorruptSpec(ops.CORRUPT_NIGHT, (float(gain), float(shot), float(read * read)))
    if kind == "haze":
        return ops.CorruptSpec(ops.CORRUPT_HAZE, (round(v[0] * 65536), round(v[1] * 65536), HAZE_AIR))
    if kind == "rain":
        thr, length, beta = v
        return ops.CorruptSpec(ops.CORRUPT_RAIN, (thr, length, RAIN_SLANT, 256 // length, beta))
    return ops.CorruptSpec(ops.CORRUPT_JPEG, int(v))


def severity_variants(severities=None, extra=None):
    """The test sets MX_SEVERITIES adds, as [(variant, short name, kind, level)]: for every corrupted
    variant that is built anyway (the reference's Noise / Blur / LowRes, then the MX_EXTRA_VARIANTS
    ones) and every level other than 3, ascending, Test_<Kind>_s<L> / <Kind>-s<L>. Level 3 is the plain
    Test_<Kind>, so there is no _s3 set. `severities` / `extra`: as env_severities / env_extra_variants."""
    levels = sorted(set(env_severities(severities)) - {3})
    built = [KIND_VARIANTS[k] for k in DEFAULT_KINDS] + env_extra_variants(extra)
    kinds = {v: k for k, v in KIND_VARIANTS.items()}
    return [(f"{var}_s{lv}", f"{short}-s{lv}", kinds[(var, short)], lv) for var, short in built for lv in levels]


def _choice(kinds):
    """The reference's draw for its three kinds (the same call, so the same `random` stream), a uniform
    choice of the given ones otherwise."""
    return random.choice(["noise", "blur", "lowres"]) if tuple(kinds) == DEFAULT_KINDS else random.choice(list(kinds))


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("mx_det corruption ops run on the GPU (HIP); no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _run(img, op, **kw):
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8))[None].to(_dev())
    return ops.corrupt_u8(t, [op], **kw)[0].cpu().numpy()


def apply_noise(img_bgr: np.ndarray, sigma: float) -> np.ndarray:
    noise = np.random.normal(0, sigma, img_bgr.shape).astype(np.float32)
    return _run(img_bgr, ops.CORRUPT_NOISE, noise=torch.from_numpy(noise)[None].to(_dev()))


def motion_blur_kernel(k: int, angle_deg: float) -> np.ndarray:
    """_motion_blur_kernel (augmentations.py:21-27) restated without OpenCV: the centre row of ones,
    rotated by cv2.getRotationMatrix2D((k/2 - 0.5, k/2 - 0.5), angle, 1) through cv2.warpAffine's
    INTER_LINEAR / BORDER_CONSTANT path (OpenCV imgwarp.cpp: the matrix inverted in double, source
    coordinates in 1/32-pixel fixed point -- AB_BITS 10, INTER_BITS 5, round_delta 16 -- and the f32
    bilinear table (1-ay)(1-ax), (1-ay)ax, ay(1-ax), ay*ax summed in tap order), then / (sum + 1e-8)
    in f32 (numpy 2 scalar rules). Host-side: k*k values."""
    f32 = np.float32
    src = np.zeros((k, k), f32)
    src[k // 2, :] = 1.0
    cx = cy = k / 2 - 0.5
    a = np.deg2rad(angle_deg)
    alpha, beta = float(np.cos(a)), float(np.sin(a))
    M = [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0], M[1], M[3], M[4] = A11, M[1] * -D, M[3] * -D, A22
    M[2], M[5] = -M[0] * M[2] - M[1] * M[5], -M[3] * M[2] - M[4] * M[5]
    rnd = lambda v: int(np.rint(v))  # noqa: E731  (cvRound: half to even)
    out = np.zeros((k, k), f32)

    def tap(yy, xx):
        return src[yy, xx] if 0 <= yy < k and 0 <= xx < k else f32(0)
    for y in range(k):
        X0 = rnd((M[1] * y + M[2]) * 1024) + 16
        Y0 = rnd((M[4] * y + M[5]) * 1024) + 16
        for x in range(k):
            X = (X0 + rnd(M[0] * x * 1024)) >> 5
            Y = (Y0 + rnd(M[3] * x * 1024)) >> 5
            sx, sy = X >> 5, Y >> 5
            ax, ay = f32(X & 31) * f32(1 / 32), f32(Y & 31) * f32(1 / 32)
            w = (f32(1) - ay) * (f32(1) - ax), (f32(1) - ay) * ax, ay * (f32(1) - ax), ay * ax
            if sx >= k or sx + 1 < 0 or sy >= k or sy + 1 < 0:
                continue
            v = tap(sy, sx) * w[0] + tap(sy, sx + 1) * w[1]
            v = v + tap(sy + 1, sx) * w[2]
            out[y, x] = v + tap(sy + 1, sx + 1) * w[3]
    return out / (out.sum() + f32(1e-8))


def kernel_taps(kernel: np.ndarray):
    """Non-zero coefficients of a k x k kernel in row-major order (OpenCV preprocess2DKernel) as
    (dy, dx, coef) relative to the centre anchor."""
    k = kernel.shape[0]
    ys, xs = np.nonzero(kernel)
    return [(int(y) - k // 2, int(x) - k // 2, float(kernel[y, x])) for y, x in zip(ys, xs)]


_DEFAULT_TAPS = None


def apply_motion_blur(img_bgr: np.ndarray, k: int, angle_deg: float) -> np.ndarray:
    global _DEFAULT_TAPS
    taps = kernel_taps(motion_blur_kernel(k, angle_deg))
    if _DEFAULT_TAPS is None:
        _DEFAULT_TAPS = kernel_taps(motion_blur_kernel(BLUR_KERNEL, BLUR_ANGLE_DEG))
    if taps == _DEFAULT_TAPS:  # the reference setting: the fused 1x9 row kernel (same arithmetic)
        return _run(img_bgr, ops.CORRUPT_BLUR)
    t = torch.from_numpy(np.ascontiguousarray(img_bgr, dtype=np.uint8))[None].to(_dev())
    return ops.filter2d_u8(t, taps)[0].cpu().numpy()


def apply_lowres(img_bgr: np.ndarray, factor: float) -> np.ndarray:
    return _run(img_bgr, ops.CORRUPT_LOWRES, factor=float(factor))


def apply_jpeg(img_bgr: np.ndarray, quality: int) -> np.ndarray:
    """The BGR pixels a decoder reads back from img_bgr saved as JPEG at `quality` (4:2:0)."""
    t = torch.from_numpy(np.ascontiguousarray(img_bgr, dtype=np.uint8))[None].to(_dev())
    return ops.corrupt_jpeg_u8(t, int(quality), JPEG_SUBSAMPLING, bgr=True)[0].cpu().numpy()


def _apply_weather(img_bgr, kind, level, seed):
    t = torch.from_numpy(np.ascontiguousarray(img_bgr, dtype=np.uint8)).to(_dev())
    seed = random.getrandbits(63) if seed is None else int(seed)
    return ops.weather_batch_u8([t], [severity_spec(kind, level)], seed=seed)[0].cpu().numpy()


def apply_night(img_bgr: np.ndarray, level: int = 3, seed=None) -> np.ndarray:
    """Low light at SEVERITY["night"][level - 1]: the image dimmed by `gain`, plus signal-dependent
    (shot) and constant (read) sensor noise from the device generator. seed None: random.getrandbits(63)."""
    return _apply_weather(img_bgr, "night", level, seed)


def apply_haze(img_bgr: np.ndarray, level: int = 3, seed=None) -> np.ndarray:
    """Haze at SEVERITY["haze"][level - 1]: a blend towards HAZE_AIR by a smooth four-octave field
    between the row's two alphas. seed None: random.getrandbits(63)."""
    return _apply_weather(img_bgr, "haze", level, seed)


def apply_rain(img_bgr: np.ndarray, level: int = 3, seed=None) -> np.ndarray:
    """Rain at SEVERITY["rain"][level - 1]: slanted, fading streaks below hashed drop heads, lightening
    the pixels they cover. seed None: random.getrandbits(63)."""
    return _apply_weather(img_bgr, "rain", level, seed)


def _apply_random_corruption(img_bgr: np.ndarray, kinds=DEFAULT_KINDS) -> np.ndarray:
    choice = _choice(kinds)
    if choice == "noise":
        return apply_noise(img_bgr, NOISE_SIGMA)
    if choice == "blur":
        return apply_motion_blur(img_bgr, BLUR_KERNEL, BLUR_ANGLE_DEG)
    if choice == "jpeg":
        return apply_jpeg(img_bgr, JPEG_QUALITY)
    if choice in WEATHER_KINDS:
        return {"night": apply_night, "haze": apply_haze, "rain": apply_rain}[choice](img_bgr)
    return apply_lowres(img_bgr, DOWNSCALE_FACTOR)


class RandomCorruption:
    """PIL transform: with probability p apply one random corruption (augmentations.py:60-74), drawn
    from `kinds` (the reference's three by default; "jpeg", "night", "haze" and "rain" may join them)."""

    def __init__(self, p: float = 0.5, kinds=DEFAULT_KINDS):
        self.p = p
        self.kinds = check_kinds(kinds)

    def __call__(self, img):
        from PIL import Image
        if random.random() > self.p:
            return img
        bgr = np.ascontiguousarray(np.asarray(img)[..., ::-1])  # cv2.cvtColor(RGB2BGR)
        out = _apply_random_corruption(bgr, self.kinds)
        return Image.fromarray(np.ascontiguousarray(out[..., ::-1]))  # BGR2RGB


class RandomCorruptionGPU:
    """Device form for uint8 HWC tensors: same decision rule (keep with prob 1-p, else a uniform choice
    of `kinds`: noise / blur / lowres by default) drawn from Python's `random` like the reference; noise
    from Philox. The images are RGB here, so a "jpeg" draw compresses them as RGB.
    severities: the levels a corrupted image draws from, random.choice(severities) after its kind. The
    default (3,) draws nothing more and makes exactly the calls the class made before the parameter;
    anything else goes through ops.corrupt_batch_u8, and batch(imgs) corrupts a list of frames of any
    sizes in one call. A "night", "haze" or "rain" draw goes through ops.corrupt_batch_u8 at any severities
    (level 3, without a level draw, at the default ones)."""

    CODES = {"noise": ops.CORRUPT_NOISE, "blur": ops.CORRUPT_BLUR, "lowres": ops.CORRUPT_LOWRES,
             "jpeg": ops.CORRUPT_JPEG, "night": ops.CORRUPT_NIGHT, "haze": ops.CORRUPT_HAZE,
             "rain": ops.CORRUPT_RAIN}

    def __init__(self, p: float = 0.5, kinds=DEFAULT_KINDS, severities=DEFAULT_SEVERITIES):
        self.p = p
        self.kinds = check_kinds(kinds)
        self.severities = check_severities(severities)

    def __call__(self, img):
        if random.random() > self.p:
            return img
        kind = _choice(self.kinds)
        if self.severities == DEFAULT_SEVERITIES and kind not in WEATHER_KINDS:
            return ops.corrupt_u8(img[None], [self.CODES[kind]], sigma=NOISE_SIGMA, seed=random.getrandbits(63),
                                  factor=DOWNSCALE_FACTOR, quality=JPEG_QUALITY, subsampling=JPEG_SUBSAMPLING)[0]
        level = 3 if self.severities == DEFAULT_SEVERITIES else random.choice(self.severities)
        spec = severity_spec(kind, level)
        return ops.corrupt_batch_u8([img], [spec], seed=random.getrandbits(63), subsampling=JPEG_SUBSAMPLING)[0]

    def batch(self, imgs):
        """The decision rule per frame, in order (keep draw, then kind, then level), one seed draw for
        the call, and one ops.corrupt_batch_u8 call for the frames that are corrupted; the others are
        returned as they are."""
        picks = {}
        for i in range(len(imgs)):
            if random.random() > self.p:
                continue
            kind = _choice(self.kinds)
            picks[i] = severity_spec(kind, random.choice(self.severities))
        seed = random.getrandbits(63)
        out = list(imgs)
        if picks:
            got = ops.corrupt_batch_u8([imgs[i] for i in picks], list(picks.values()), seed=seed,
                                       subsampling=JPEG_SUBSAMPLING)
            for i, g in zip(picks, got):
                out[i] = g
        return out


def patch_ultralytics_augmentations():
    """augmentations.py:78-98: wrap Ultralytics' Albumentations.__call__ with a p=0.5 corruption of
    labels["img"] (BGR uint8). Ultralytics itself is not installed here (SURVEY.md §8f 'next')."""
    from ultralytics.data import augment as _augment

    orig = _augment.Albumentations.__call__

    def _patched(self, labels):
        if random.random() < 0.5:
            labels["img"] = _apply_random_corruption(labels["img"])
        return orig(self, labels)

    _augment.Albumentations.__call__ = _patched
    print("[augmentations] Ultralytics Albumentations patched with corruption augmentations")
