"""Fit the restoration gate's thresholds on real images — `python -m scripts.fit_restore_gate`.

The default rules of mx_det.gate come from a CPU sketch on ten images; this script replaces their thresholds
with ones fitted on the training images. Each image (MX_GATE_FIT_IMAGES of them, default 500, evenly spaced
over the sorted listing of data/processed/visdrone_coco6/images/train) is decoded on the device, corrupted
there under every condition (ops.corrupt_batch_u8, Philox noise seeded by the image's index) and measured
by the statistics kernel (ops.degradation_stats_u8), sixteen images per launch. Conditions: clean, noise,
blur and lowres at level 3, then the MX_EXTRA_VARIANTS kinds at level 3 (named jpeg, night, ...), then, under
MX_SEVERITIES, every kind at the other levels (named noise-s1, ...). Labels: noise passes, blur and lowres
are restored, their other levels follow their kind, every other kind passes unless MX_GATE_LABELS maps it
(for example MX_GATE_LABELS=jpeg=1,haze-s1=0).
gate.fit_rules keeps the four rule shapes and puts each threshold at the midpoint, in log space, between the
classes it separates; it raises when two of them overlap. The rules go to experiments/restoration/gate.json
(MX_RESTORE_GATE takes that path), the feature ranges per condition are printed with the verdicts the
fitted rules give.
"""
import os
from pathlib import Path

from mx_det import augment, gate, ops
from mx_det.engine import init_device
from scripts import restore_testsets

TRAIN_IMG_DIR = Path("data/processed/visdrone_coco6/images/train")
OUT_PATH = Path("experiments/restoration/gate.json")
SEED = 42
BATCH = 16


def conditions():
    """[(name, kind or None, level)]: clean and the three default kinds at level 3, the MX_EXTRA_VARIANTS
    kinds at level 3, then the MX_SEVERITIES levels of all of them."""
    kinds = {v: k for k, v in augment.KIND_VARIANTS.items()}
    extra = [kinds[v] for v in augment.env_extra_variants()]
    out = [("clean", None, 3)] + [(k, k, 3) for k in list(augment.DEFAULT_KINDS) + extra]
    return out + [(f"{kind}-s{level}", kind, level) for _, _, kind, level in augment.severity_variants()]


def labels(conds, value=None):
    """condition name -> verdict for the conditions beyond the four that fit_rules fixes."""
    out = {name: gate.CONDITION_VERDICTS.get(kind, 0) for name, kind, _ in conds if name not in gate.CONDITION_VERDICTS}
    value = os.environ.get("MX_GATE_LABELS", "") if value is None else value
    for item in (s.strip() for s in value.split(",") if s.strip()):
        name, _, v = item.partition("=")
        if name.strip() not in out or v.strip() not in ("0", "1"):
            raise ValueError(f"MX_GATE_LABELS: {item!r} is not <condition>=0|1 with a condition of {sorted(out)}")
        out[name.strip()] = int(v)
    return out


def pick(files, count):
    """`count` files evenly spaced over the sorted listing (all of them when there are fewer)."""
    files = sorted(files)
    if count >= len(files):
        return files
    return [files[i * len(files) // count] for i in range(count)]


def measure(images, conds, seed):
    """condition name -> stats rows (lists of 8 ints) for a list of uint8 [H,W,3] device images."""
    table = {}
    for name, kind, level in conds:
        xs = images
        if kind is not None:
            xs = ops.corrupt_batch_u8(images, [augment.severity_spec(kind, level)] * len(images), seed=seed)
        table[name] = ops.degradation_stats_u8(xs, rules=(), default=0)[0].tolist()
    return table


def report(table, rules, default):
    for name, rows in table.items():
        f = gate.features(rows)
        v = [gate.decide(r, rules, default) for r in rows]
        rng = "  ".join(f"{k} {min(x[k] for x in f):.3g}..{max(x[k] for x in f):.3g}" for k in ("sigma", "anisotropy", "hf"))
        print(f"  {name:12s} n={len(rows):5d}  {rng}  restored {sum(v)} passed {len(v) - sum(v)}", flush=True)


def main(train_dir=TRAIN_IMG_DIR, out_path=OUT_PATH, count=None):
    dev, _, _ = init_device()
    conds = conditions()
    lab = labels(conds)
    count = int(os.environ.get("MX_GATE_FIT_IMAGES", 500)) if count is None else count
    files = pick(Path(train_dir).glob("*.jpg"), count)
    if not files:
        raise FileNotFoundError(f"no training images under {train_dir}")
    table = {name: [] for name, _, _ in conds}
    for i in range(0, len(files), BATCH):
        images = [restore_testsets.read_rgb(p, dev) for p in files[i:i + BATCH]]
        for name, rows in measure(images, conds, (SEED << 32) + i).items():
            table[name] += rows
    rules, default = gate.fit_rules(table, labels=lab)
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    gate.save_rules(out_path, rules, default)
    print(f"gate rules fitted on {len(files)} images -> {Path(out_path).resolve()}")
    for r in rules:
        print(f"  {r.name:8s} {r.a} * {gate.STAT_NAMES[r.i]} > {r.b} * {gate.STAT_NAMES[r.j]} -> {r.verdict}")
    report(table, rules, default)
    return rules, default


if __name__ == "__main__":
    main()
