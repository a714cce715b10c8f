"""Evaluate Faster R-CNN checkpoints on the Clean / Noise / Blur / LowRes test sets —
`python -m scripts.eval_all`.

FRCNN branch of the reference's eval_all.py (:79-156, :198-213) on MI355X; the Ultralytics RT-DETR /
YOLO branches are outside this build's scope and are reported as skipped.
Outputs keep the reference schema: experiments/eval_results.json ({model: {variant: {mAP50_95, mAP50,
per_class_ap50}}}) and experiments/eval_results.csv. torchrun shards the images per rank.
MX_EXTRA_VARIANTS=jpeg adds the Test_JPEG set (column JPEG) after the reference's four, and night / haze /
rain the Test_Night / Test_Haze / Test_Rain sets (columns Night, Haze, Rain); MX_SEVERITIES
(levels 1..5, default 3) adds the Test_<Kind>_s<L> sets after those (columns Noise-s1 and so on).
MX_BN_ADAPT=<mode>[:<prior>] (batch or stream; prior in images, default 16; unset: off) evaluates every
checkpoint a second time under test-time BatchNorm adaptation (mx_det.adapt) and adds it as
<name>_BNAdapt next to the unadapted entry, in the same schema; MX_BN_ADAPT_FREEZE_AFTER=<images>
freezes the stream-mode statistics after that many images of each variant.
MX_TTA=flip[:<vote_iou>] (default 0.8; unset: off) evaluates every checkpoint once more under flip test-time
augmentation with box voting (mx_det.tta) and adds it as <name>_TTA, in the same schema; the plain and the
_BNAdapt passes of the same run stay single-view.
"""
import csv
import json
import os
import time
from pathlib import Path

import torch

from mx_det import adapt as bn_adapt
from mx_det import tta as mx_tta
from mx_det.augment import EXTRA_VARIANTS, env_extra_variants, severity_variants
from mx_det.engine import dist_info, eval_frcnn_variant, init_device, load_frcnn_checkpoint

VARIANTS = ["Test_Clean", "Test_Noise", "Test_Blur", "Test_LowRes"]
SHORT = {"Test_Clean": "Clean", "Test_Noise": "Noise", "Test_Blur": "Blur", "Test_LowRes": "LowRes"}
CLASS_NAMES = ["pedestrian", "car", "van", "truck", "bus", "motor"]
COCO_TESTSET_ROOT = Path("data/testsets/coco6")
CKPTS = {
    "FasterRCNN": Path("experiments/frcnn/baseline_clean/best.pth"),
    "FasterRCNN_aug": Path("experiments/frcnn/augmented/best.pth"),
}
MODEL_ORDER = ["FasterRCNN", "FasterRCNN_aug", "RT-DETR-L", "RT-DETR-L_aug", "YOLOv8m", "YOLOv8m_aug"]
BASELINE_PAIRS = [("FasterRCNN", "FasterRCNN_aug"), ("RT-DETR-L", "RT-DETR-L_aug"), ("YOLOv8m", "YOLOv8m_aug")]
OUT_DIR = Path("experiments")


def all_variants():
    """The reference's four variants, then those MX_EXTRA_VARIANTS names, then the MX_SEVERITIES sets."""
    return VARIANTS + [v for v, _ in env_extra_variants()] + [v[0] for v in severity_variants()]


def short(v):
    if v in SHORT:
        return SHORT[v]
    base, _, level = v.rpartition("_s")  # Test_<Kind>_s<L> -> <Kind>-s<L>
    names = dict(SHORT, **dict(EXTRA_VARIANTS.values()))
    return f"{names[base]}-s{level}" if base in names and level.isdigit() else names[v]


def variant_paths(root, v):
    return str(root / v / "images" / "val"), str(root / v / "annotations" / "instances_val.json")


ADAPT_SUFFIX = "_BNAdapt"
TTA_SUFFIX = "_TTA"


def eval_model(name, ckpt, dev, root=None, restorer=None, variants=None, restore_clean=False, counts=None, adapt=None,
               tta=None):
    """restore_clean: apply `restorer` to Test_Clean as well (a blind mx_det.gate.GatedRestorer decides per
    image, so the directory name no longer does). counts: a dict that receives the restorer's
    take_counts() per variant (this rank's shard). adapt: (mode, prior) of a mx_det.adapt.BNAdapter for the
    model, reset at the start of every variant (None: the running statistics, as the reference). tta: an
    mx_det.tta.TTA the model evaluates under (None: one view)."""
    rank = dist_info()[1]
    root = COCO_TESTSET_ROOT if root is None else root
    variants = all_variants() if variants is None else variants
    if rank == 0:
        print("=" * 60 + f"\n  {name}  (COCOeval bbox)\n" + "=" * 60, flush=True)
    model = load_frcnn_checkpoint(ckpt, dev)
    if tta is not None:
        model.tta = tta
    kw = {} if adapt is None else dict(adapter=bn_adapt.BNAdapter(model, mode=adapt[0], prior=adapt[1]))
    res = {}
    for v in variants:
        img_dir, ann = variant_paths(root, v)
        m = eval_frcnn_variant(model, img_dir, ann, dev, restorer=restorer if restore_clean or v != "Test_Clean" else None,
                               **kw)
        if counts is not None and restorer is not None:
            counts[v] = restorer.take_counts()
        if rank == 0:
            res[v] = m
            print(f"  [{short(v)}] mAP50={m['mAP50']:.4f}  mAP50-95={m['mAP50_95']:.4f}", flush=True)
    del model
    torch.cuda.empty_cache()
    return res


def save_json(all_results, path):
    with open(path, "w", encoding="utf-8") as f:
        json.dump(all_results, f, indent=2, ensure_ascii=False)
    print(f"\nJSON saved: {Path(path).resolve()}")


def save_csv(all_results, path, variants=None, pairs=None):
    variants = all_variants() if variants is None else variants
    pairs = BASELINE_PAIRS if pairs is None else pairs
    models = [m for base in MODEL_ORDER for m in (base, base + ADAPT_SUFFIX, base + TTA_SUFFIX)
              if m in all_results]
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(["Model", "Metric"] + [short(v) for v in variants])
        for m in models:
            w.writerow([m, "mAP@50"] + [f"{all_results[m][v]['mAP50']:.4f}" for v in variants])
            w.writerow([m, "mAP@50-95"] + [f"{all_results[m][v]['mAP50_95']:.4f}" for v in variants])
        w.writerow([])
        w.writerow(["Model", "Metric"] + [short(v) for v in variants[1:]])
        for m in models:
            clean = all_results[m]["Test_Clean"]["mAP50"]
            w.writerow([m, "Deg%_mAP50"] + [f"{((all_results[m][v]['mAP50'] - clean) / clean * 100 if clean > 0 else 0.0):.1f}%"
                                            for v in variants[1:]])
        w.writerow([])
        w.writerow(["Model", "Metric"] + [short(v) for v in variants])
        for base, aug in pairs:
            if base in all_results and aug in all_results:
                w.writerow([base, "Aug-Base_mAP50"] + [f"{all_results[aug][v]['mAP50'] - all_results[base][v]['mAP50']:+.4f}"
                                                       for v in variants])
    print(f"CSV  saved: {Path(path).resolve()}")


def main():
    dev, world, rank = init_device()
    adapt = bn_adapt.parse_env(os.environ.get("MX_BN_ADAPT", ""))  # a bad value raises before any model loads
    tta = mx_tta.parse_env(os.environ.get("MX_TTA", ""))  # likewise
    t0 = time.time()
    all_results = {}
    for name, ck in CKPTS.items():
        r = eval_model(name, ck, dev)
        if rank == 0:
            all_results[name] = r
        if adapt is not None:
            r = eval_model(name + ADAPT_SUFFIX, ck, dev, adapt=adapt)
            if rank == 0:
                all_results[name + ADAPT_SUFFIX] = r
        if tta is not None:
            r = eval_model(name + TTA_SUFFIX, ck, dev, tta=tta)
            if rank == 0:
                all_results[name + TTA_SUFFIX] = r
    if rank == 0:
        print("\n  RT-DETR-L / YOLOv8m: Ultralytics branches not part of this build (skipped)")
        print(f"\nTotal evaluation time: {(time.time() - t0) / 60:.1f} min")
        OUT_DIR.mkdir(parents=True, exist_ok=True)
        save_json(all_results, OUT_DIR / "eval_results.json")
        save_csv(all_results, OUT_DIR / "eval_results.csv")
    return all_results


if __name__ == "__main__":
    main()
