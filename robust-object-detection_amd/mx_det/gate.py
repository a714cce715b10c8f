"""The blind restoration gate: look at an image, decide whether the U-Net should touch it.

ops.degradation_stats_u8 (mx_degradation_stats_u8, csrc/mx_gate.hip) gives eight exact integer sums of the
luma per image and, on the device, the verdict of a rule list over them: 1 = restore, 0 = pass through. This
module holds what needs no device: the names, the rules as data (DEFAULT_RULES, JSON files, fit_rules), the
host restatement of the verdict (decide), and GatedRestorer, which wraps a RestorationUNet.

The default thresholds come from a CPU sketch on ten images ("Restoration gate"): the gate's
accuracy on VisDrone and the mAP of the gated strategy are unmeasured. scripts/fit_restore_gate.py refits
them on real data; MX_RESTORE_GATE=<file> loads the result.
"""
import collections
import fractions
import json
import math
import os

STAT_NAMES = ("N", "IMM", "DX2", "DY2", "DXX2", "DYY2", "G2", "H2")
N, IMM, DX2, DY2, DXX2, DYY2, G2, H2 = range(8)
MAX_RULES = 8
MAX_COEF = 65535
SIGMA_SCALE = 1.2533 / 6.0  # Immerkaer: sigma = sqrt(pi / 2) / 6 * mean |mask response|

# fires when a * stats[i] > b * stats[j]; the first rule that fires gives the verdict
Rule = collections.namedtuple("Rule", "i j a b verdict name", defaults=("",))

DEFAULT_RULES = (
    Rule(IMM, N, 10, 383, 0, "noise"),    # sigma > 8: the U-Net hurts on noise, do not restore
    Rule(G2, H2, 35, 100, 1, "lowres"),   # H2 / G2 < 0.35
    Rule(DY2, DX2, 2, 5, 1, "blur-h"),    # DY2 / DX2 > 2.5: horizontal blur
    Rule(DX2, DY2, 2, 5, 1, "blur-v"),    # DX2 / DY2 > 2.5: vertical blur
)
DEFAULT_VERDICT = 0
CONDITION_VERDICTS = {"clean": 0, "noise": 0, "blur": 1, "lowres": 1}  # fit_rules' labels; others pass


def check_rules(rules, default=DEFAULT_VERDICT):
    """The rules as a tuple of Rule, checked against mx_degradation_stats_u8's bounds (ValueError)."""
    out = []
    for r in rules:
        r = Rule(*r)
        vals = (r.i, r.j, r.a, r.b, r.verdict)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
            raise ValueError(f"gate rule {r}: i, j, a, b and verdict must be integers")
        if not (0 <= r.i < 8 and 0 <= r.j < 8):
            raise ValueError(f"gate rule {r}: sum index outside 0..7")
        if not (0 <= r.a <= MAX_COEF and 0 <= r.b <= MAX_COEF):
            raise ValueError(f"gate rule {r}: coefficient outside 0..{MAX_COEF}")
        if r.verdict not in (0, 1):
            raise ValueError(f"gate rule {r}: verdict must be 0 or 1")
        out.append(r)
    if len(out) > MAX_RULES:
        raise ValueError(f"{len(out)} gate rules, at most {MAX_RULES}")
    if default not in (0, 1) or isinstance(default, bool):
        raise ValueError(f"default verdict {default!r} must be 0 or 1")
    return tuple(out)


def _row(stats_row):
    row = [int(v) for v in (stats_row.tolist() if hasattr(stats_row, "tolist") else stats_row)]
    if len(row) != 8:
        raise ValueError("a stats row has 8 sums")
    return row


def decide(stats_row, rules=DEFAULT_RULES, default=DEFAULT_VERDICT):
    """The device's verdict for one stats row, in Python ints: the first rule with
    a * stats[i] > b * stats[j], else default."""
    row = _row(stats_row)
    for r in rules:
        r = Rule(*r)
        if r.a * row[r.i] > r.b * row[r.j]:
            return int(r.verdict)
    return int(default)


def _ratio(x, y):
    return x / y if y else (math.inf if x else math.nan)


def features(stats):
    """The three quantities the default rules threshold, as floats, for reports only: one dict for one
    row, a list of dicts for rows. sigma is Immerkaer's noise estimate, anisotropy DY2 / DX2, hf H2 / G2."""
    rows = stats.tolist() if hasattr(stats, "tolist") else list(stats)
    if rows and isinstance(rows[0], (list, tuple)) or not rows:
        return [features(r) for r in rows]
    row = _row(rows)
    return {"sigma": SIGMA_SCALE * _ratio(row[IMM], row[N]), "anisotropy": _ratio(row[DY2], row[DX2]),
            "hf": _ratio(row[H2], row[G2])}


def save_rules(path, rules=DEFAULT_RULES, default=DEFAULT_VERDICT):
    rules = check_rules(rules, default)
    doc = {"default_verdict": int(default),
           "rules": [{"name": r.name, "lhs": STAT_NAMES[r.i], "a": r.a, "rhs": STAT_NAMES[r.j], "b": r.b,
                      "verdict": r.verdict} for r in rules]}
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=2)
        f.write("\n")


def load_rules(path):
    """(rules, default) of a file save_rules wrote: a * lhs > b * rhs gives verdict. ValueError on anything
    else."""
    try:
        with open(path, encoding="utf-8") as f:
            doc = json.load(f)
        rules = [Rule(STAT_NAMES.index(r["lhs"]), STAT_NAMES.index(r["rhs"]), r["a"], r["b"], r["verdict"],
                      str(r.get("name", ""))) for r in doc["rules"]]
        default = doc.get("default_verdict", DEFAULT_VERDICT)
    except (OSError, KeyError, TypeError, AttributeError, json.JSONDecodeError, ValueError) as e:
        raise ValueError(f"bad gate rules file {path}: {e}") from e
    try:
        return check_rules(rules, default), default
    except ValueError as e:
        raise ValueError(f"bad gate rules file {path}: {e}") from e


def env_gate(value=None):
    """MX_RESTORE_GATE: unset, empty or 0 -> None (off); auto -> (DEFAULT_RULES, DEFAULT_VERDICT); anything
    else is the path of a rules JSON (a bad file raises ValueError here, at start-up)."""
    value = os.environ.get("MX_RESTORE_GATE", "") if value is None else value
    value = value.strip()
    if value in ("", "0"):
        return None
    if value == "auto":
        return DEFAULT_RULES, DEFAULT_VERDICT
    return load_rules(value)


# ---------------------------------------------------------------------------------------------
def _quantile(vals, q):
    v = sorted(vals)
    pos = q * (len(v) - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (pos - lo)


def _as_ratio(t):
    """t > 0 as num / den with both in 1..MAX_COEF."""
    for limit in (1000, 100, 10, 1):
        f = fractions.Fraction(t).limit_denominator(limit)
        if 0 < f.numerator <= MAX_COEF:
            return f.numerator, f.denominator
    raise ValueError(f"threshold {t} has no ratio of coefficients in 1..{MAX_COEF}")


def _split(name, above, below, q):
    """The threshold between the classes that must lie above it and those that must lie below: the
    midpoint, in log space, of the nearest quantiles. ValueError when they overlap."""
    if not all(above.values()) or not any(below.values()):
        raise ValueError(f"gate rule {name}: a class without a usable row")
    lo_edge = min(_quantile(v, q) for v in above.values())
    hi_edge = max(_quantile(v, 1.0 - q) for v in below.values() if v)
    if not (hi_edge < lo_edge):
        raise ValueError(f"gate rule {name}: the classes overlap ({sorted(above)} from {lo_edge:.4g}, "
                         f"{sorted(below)} up to {hi_edge:.4g})")
    if math.isinf(lo_edge):
        raise ValueError(f"gate rule {name}: no finite value in {sorted(above)}")
    return math.exp(0.5 * (math.log(max(hi_edge, 1e-9)) + math.log(lo_edge)))


def fit_rules(table, labels=None, quantile=0.0):
    """Refit the thresholds of the four default rule shapes. table: condition name -> list of stats rows;
    it must hold clean, noise, blur and lowres, and may hold more (haze-s2, ...). labels: condition ->
    verdict for the extra conditions (default 0, pass). Each rule separates its own condition from the
    other three and from every extra condition with another verdict than the rule's; its threshold is
    the midpoint, in log space, between the nearest `quantile` / 1 - `quantile` quantiles of the two
    sides (0: the extremes). blur-v mirrors blur-h. Returns (rules, default); ValueError when two sides
    overlap."""
    verdicts = dict(CONDITION_VERDICTS)
    for k, v in (labels or {}).items():
        if k in CONDITION_VERDICTS and v != CONDITION_VERDICTS[k]:
            raise ValueError(f"the verdict of {k} is fixed")
        verdicts[k] = int(v)
    for need in CONDITION_VERDICTS:
        if not table.get(need):
            raise ValueError(f"fit_rules: no rows for {need}")
    # per condition, the three quantities in the direction their rule fires in (nan: a flat image, which
    # fires nothing)
    feats = {k: [_row(r) for r in rows] for k, rows in table.items() if rows}

    def vals(k, num, den, scale=1.0):
        v = [scale * _ratio(r[num], r[den]) for r in feats[k]]
        return [x for x in v if not math.isnan(x)]

    def others(own, verdict):
        return [k for k in feats if k != own and (k in CONDITION_VERDICTS or verdicts.get(k, 0) != verdict)]

    # noise: sigma above the others; the rule compares IMM / N = sigma / SIGMA_SCALE
    sig = _split("noise", {"noise": vals("noise", IMM, N, SIGMA_SCALE)},
                 {k: vals(k, IMM, N, SIGMA_SCALE) for k in others("noise", 0)}, quantile)
    nb, na = _as_ratio(sig / SIGMA_SCALE)  # na * IMM > nb * N
    # lowres: H2 / G2 below the others, so G2 / H2 above them
    inv = _split("lowres", {"lowres": vals("lowres", G2, H2)}, {k: vals(k, G2, H2) for k in others("lowres", 1)}, quantile)
    lb, la = _as_ratio(inv)  # la * G2 > lb * H2
    # blur: DY2 / DX2 above the others, and above their DX2 / DY2 too (the mirrored rule must not fire)
    below = {k: vals(k, DY2, DX2) for k in others("blur", 1)}
    below.update({k + " (mirrored)": vals(k, DX2, DY2) for k in others("blur", 1)})
    ani = _split("blur", {"blur": vals("blur", DY2, DX2)}, below, quantile)
    bb, ba = _as_ratio(ani)  # ba * DY2 > bb * DX2
    rules = (Rule(IMM, N, na, nb, 0, "noise"), Rule(G2, H2, la, lb, 1, "lowres"), Rule(DY2, DX2, ba, bb, 1, "blur-h"),
             Rule(DX2, DY2, ba, bb, 1, "blur-v"))
    return check_rules(rules, DEFAULT_VERDICT), DEFAULT_VERDICT


# ---------------------------------------------------------------------------------------------
class GatedRestorer:
    """A RestorationUNet behind the gate: restore_u8 restores the images whose verdict is 1 and passes the
    others through unchanged. It stands wherever the U-Net's restore_u8 does (engine.eval_frcnn_variant).
      mode "select": stats and verdicts, the U-Net on every image, mx_restore_finish_gated picks per image
        on the device; no host synchronisation (the counts stay on the device until they are read).
      mode "skip": the verdicts are read once, the U-Net runs on the flagged images only, the others are
        copied. The same bytes as "select".
    denoiser (a denoise.NLMDenoiser, or None): the pixel branch for noise. An image the U-Net leaves alone
    (verdict 0) and the denoiser's rule recognises as noisy is denoised, blind, from the gate's own sums
    (mx_denoise_nlm_u8): in select mode the stats and verdicts go to it on the device after the U-Net's
    selection and the host still never waits; skip mode makes the same decisions from its one read-back.
    restored / denoised / passed count the images of each kind since the last take_counts(); without a
    denoiser nothing changes and take_counts() has its two keys."""

    def __init__(self, unet, rules=DEFAULT_RULES, default=DEFAULT_VERDICT, mode="select", bgr=False, denoiser=None):
        if mode not in ("select", "skip"):
            raise ValueError(f"GatedRestorer mode {mode!r}: select or skip")
        self.unet, self.mode, self.bgr = unet, mode, bool(bgr)
        self.rules, self.default = check_rules(rules, default), int(default)
        if denoiser is not None and bool(denoiser.bgr) != self.bgr:
            raise ValueError("GatedRestorer: the denoiser's bgr differs from the gate's")
        self.denoiser = denoiser
        self._seen = 0
        self._restored = 0      # host part (skip mode)
        self._restored_dev = None  # device part (select mode): an int64 scalar, summed without a sync
        self._denoised = 0
        self._denoised_dev = None

    # -- counts
    @property
    def restored(self):
        dev = int(self._restored_dev.item()) if self._restored_dev is not None else 0
        return self._restored + dev

    @property
    def denoised(self):
        dev = int(self._denoised_dev.item()) if self._denoised_dev is not None else 0
        return self._denoised + dev

    @property
    def passed(self):
        return self._seen - self.restored - (self.denoised if self.denoiser is not None else 0)

    def take_counts(self):
        """{"restored", "passed"} since the last call (with a denoiser: and "denoised", which passed then
        excludes), and start again from zero."""
        out = {"restored": self.restored, "passed": self.passed}
        if self.denoiser is not None:
            out["denoised"] = self.denoised
        self._seen, self._restored, self._restored_dev = 0, 0, None
        self._denoised, self._denoised_dev = 0, None
        return out

    # -- verdicts
    def verdicts(self, images):
        """(stats int64 [B, 8], verdict int32 [B]) on the device for a [B,H,W,3] tensor or a list."""
        from . import ops
        return ops.degradation_stats_u8(images, self.rules, self.default, bgr=self.bgr)

    def decide_u8(self, images):
        """The verdicts as a list of ints (one read-back)."""
        return [int(v) for v in self.verdicts(images)[1].tolist()]

    def _denoise_decisions(self, rows, verdicts):
        """The device's apply decision per image, restated on the host (denoise.params)."""
        from . import denoise
        d = self.denoiser
        return [int(denoise.params(row, d.k16, d.rule, verdict=v)[0]) for row, v in zip(rows, verdicts)]

    def decide_both_u8(self, images):
        """(stats, verdicts, denoise) with one read-back: the device stats, the verdicts as ints and, per image,
        1 when the denoiser would take it (all 0 without a denoiser)."""
        import torch
        stats, verdict = self.verdicts(images)
        rows = torch.cat([stats, verdict[:, None].to(torch.int64)], 1).tolist()
        v = [int(r[8]) for r in rows]
        dn = self._denoise_decisions([r[:8] for r in rows], v) if self.denoiser is not None else [0] * len(v)
        return stats, v, dn

    def count(self, verdicts, denoised=()):
        """Count images decided outside restore_u8 (scripts that copy passed files themselves)."""
        verdicts = [int(v) for v in verdicts]
        self._seen += len(verdicts)
        self._restored += sum(verdicts)
        self._denoised += sum(int(v) for v in denoised)

    # -- restore
    def restore_u8(self, img_u8):
        """uint8 [B,H,W,3] -> uint8 [B,H,W,3], or a list of uint8 [H,W,3] of any sizes -> a list."""
        import torch
        batched = torch.is_tensor(img_u8)
        xs = img_u8 if batched else list(img_u8)
        if len(xs) == 0:
            return img_u8 if batched else []
        if self.denoiser is not None and self.mode == "skip":
            return self._restore_skip_denoise(xs, batched)
        stats, verdict = self.verdicts(xs)
        if self.mode == "select":
            self._seen += len(xs)
            s = verdict.sum(dtype=torch.int64)
            self._restored_dev = s if self._restored_dev is None else self._restored_dev + s
            if batched:
                out = self.unet.restore_u8(xs, verdict=verdict)
            else:
                out = [self.unet.restore_u8(im[None], verdict=verdict[b:b + 1])[0] for b, im in enumerate(xs)]
            if self.denoiser is not None:  # the U-Net's images are copied, the noisy ones denoised: one launch
                out, applied = self.denoiser.denoise_u8(out, stats=stats, verdict=verdict)
                s = applied.sum(dtype=torch.int64)
                self._denoised_dev = s if self._denoised_dev is None else self._denoised_dev + s
            return out
        v = [int(k) for k in verdict.tolist()]
        self.count(v)
        if batched:
            out = xs.clone()
            idx = [b for b, k in enumerate(v) if k]
            if idx:
                sel = torch.tensor(idx, device=xs.device)
                out[sel] = self.unet.restore_u8(xs[sel])
            return out
        return [self.unet.restore_u8(im[None])[0] if k else im.clone() for im, k in zip(xs, v)]

    def _restore_skip_denoise(self, xs, batched):
        """Skip mode with a denoiser: the U-Net on the flagged images, the denoiser (blind, from the device
        stats of exactly those images) on the noisy ones, copies of the rest."""
        import torch
        stats, v, dn = self.decide_both_u8(xs)
        self.count(v, dn)
        outs = [self.unet.restore_u8(im[None])[0] if k else (None if d else im.clone()) for im, k, d in zip(xs, v, dn)]
        idx = [b for b, d in enumerate(dn) if d]
        if idx:
            sel = torch.tensor(idx, device=stats.device)
            got, _ = self.denoiser.denoise_u8([xs[b] for b in idx], stats=stats.index_select(0, sel).contiguous())
            for b, g in zip(idx, got):
                outs[b] = g
        return torch.stack(outs) if batched else outs


def from_env(unet, mode="select", value=None, denoiser=None):
    """The GatedRestorer MX_RESTORE_GATE asks for, or None when the gate is off."""
    g = env_gate(value)
    return None if g is None else GatedRestorer(unet, g[0], g[1], mode=mode, denoiser=denoiser)
