"""The blind non-local-means denoiser: the pixel branch for the images the gate's noise rule recognises.

ops.denoise_nlm_u8 (mx_denoise_nlm_u8, csrc/mx_denoise.hip) denoises every image of a batch in one device
launch; a blind image takes its strength from the sums mx_degradation_stats_u8 left on the device, so nothing
is read back. This module holds what needs no device: the host restatement of the per-image parameters
(params, as gate.decide is for verdicts), NLMDenoiser, which holds the settings and calls the op, and the
MX_RESTORE_DENOISE switch.

It is edge-preserving and not learned: no checkpoint, no training data. On six synthetic images with sigma 15
noise it gains 3.8-7.5 dB PSNR ("Non-local-means denoiser"); its effect on mAP is unmeasured for
want of a trained checkpoint.
"""
import os

from . import gate

DEFAULT_K16 = 6                 # h = 6 / 16 = 0.375 sigma
DEFAULT_RULE = (10, 383)        # the gate's noise rule: 10 * IMM > 383 * N
SIGMA_MUL = 13689               # 1.2533 / 6 in 1 / 65536: Immerkaer's scale
MAX_COEF = 65535


def check(k16, rule):
    """(k16, (a, b)) checked against mx_denoise_nlm_u8's bounds (ValueError)."""
    if not isinstance(k16, int) or isinstance(k16, bool) or not 1 <= k16 <= 64:
        raise ValueError(f"denoiser k16 {k16!r} must be an integer in 1..64")
    a, b = rule
    for v in (a, b):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= MAX_COEF:
            raise ValueError(f"denoiser rule {rule!r}: coefficients must be integers in 0..{MAX_COEF}")
    return k16, (a, b)


def params(stats_row, k16=DEFAULT_K16, rule=DEFAULT_RULE, sigma_q8=0, verdict=None):
    """The device's per-image parameters in Python ints: (apply, s8, T0, D, Q) as include/mx_det.h defines
    them. sigma_q8 in 1..65535: s8 = sigma_q8 and the image is denoised (stats_row may be None); 0: blind,
    from stats_row = [N, IMM, ...]. verdict: the gate's verdict of the image, if a verdict array goes with the
    call; anything but 0 leaves the image alone."""
    k16, (a, b) = check(k16, rule)
    if not 0 <= int(sigma_q8) <= 65535:
        raise ValueError(f"sigma_q8 {sigma_q8!r} outside 0..65535")
    if sigma_q8:
        apply, s8 = True, int(sigma_q8)
    else:
        row = [int(v) for v in (stats_row.tolist() if hasattr(stats_row, "tolist") else stats_row)]
        n, imm = row[gate.N], row[gate.IMM]
        if n < 1:
            raise ValueError("a blind image needs stats with N >= 1")
        apply = a * imm > b * n
        s8 = (((imm << 8) // n) * SIGMA_MUL) >> 16
    if verdict is not None and int(verdict) != 0:
        apply = False
    t0 = (50 * s8 * s8) >> 16
    d = max((25 * k16 * k16 * s8 * s8) >> 24, 1)
    return bool(apply), s8, t0, d, (1 << 24) // d


class NLMDenoiser:
    """Holds k16 and the rule; denoise_u8 is one ops.denoise_nlm_u8 call."""

    def __init__(self, k16=DEFAULT_K16, rule=DEFAULT_RULE, bgr=False):
        self.k16, self.rule = check(k16, tuple(rule))
        self.bgr = bool(bgr)

    def denoise_u8(self, images, stats=None, verdict=None, sigma=None, out=None):
        """(out, applied) of ops.denoise_nlm_u8 under this denoiser's settings: blind from `stats` (and left
        alone where `verdict` is not 0) unless `sigma` is given."""
        from . import ops
        return ops.denoise_nlm_u8(images, stats=stats, verdict=verdict, sigma=sigma, k16=self.k16, rule=self.rule,
                                  bgr=self.bgr, out=out)


def env_denoise(value=None):
    """MX_RESTORE_DENOISE: unset, empty or 0 -> None (off); nlm or nlm:<k16> -> an NLMDenoiser; anything else
    raises ValueError here, at start-up."""
    value = os.environ.get("MX_RESTORE_DENOISE", "") if value is None else value
    value = value.strip()
    if value in ("", "0"):
        return None
    name, sep, arg = value.partition(":")
    if name != "nlm" or (sep and not arg.strip().isdigit()):
        raise ValueError(f"MX_RESTORE_DENOISE={value!r}: expected 0, nlm or nlm:<k16>")
    try:
        return NLMDenoiser(int(arg) if sep else DEFAULT_K16)
    except ValueError as e:
        raise ValueError(f"MX_RESTORE_DENOISE={value!r}: {e}") from e
