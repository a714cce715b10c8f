"""Demo inference: side-by-side Baseline vs Augmented detections on corrupted images —
`python -m scripts.demo_inference`.

FRCNN branch of the reference's demo_inference.py on MI355X. For each selected image one JPEG under
experiments/demo/:  [Clean + ground truth]  [Blur + baseline]  [Blur + augmented]
with the reference's constants, image selection and file names (FRCNN_img<id>_gt<n>_base<n>_aug<n>.jpg).
Everything between the files runs on the device: JPEG decode (mx_det.jpeg), both checkpoints' eval forward
with the fused detection tail's padded outputs left where they are (FasterRCNN.detect_padded), frames, label
plates, text and title bars in one launch (mx_det.draw.Overlay), the three panels resized to height 480 and
laid side by side in one launch (mx_det.draw.compose), and the JPEG encoder (quality 92, as cv2.imwrite's
IMWRITE_JPEG_QUALITY). Per image only `drawn` (the detection counts of the file name) and the finished scan
come back. The text is the project's 5x7 bitmap font, not cv2's Hershey strokes: the pictures show the
same boxes, labels and scores, not the same pixels, as the reference's. The Ultralytics RT-DETR / YOLO
branches are outside this build's scope and are reported as skipped, as eval_all does.

MX_DEMO_EXTRA=tta,bnadapt appends one more panel per named strategy, each the augmented checkpoint once
more on the blurred image: under flip test-time augmentation with box voting (mx_det.tta.TTA()) and under
test-time BatchNorm adaptation (mx_det.adapt.BNAdapter(mode="batch")).
"""
import json
import os
from pathlib import Path

import numpy as np
import torch

from mx_det import adapt as bn_adapt
from mx_det import draw, jpeg
from mx_det import tta as mx_tta
from mx_det.draw import CLASS_COLORS, CLASS_NAMES, select_images  # noqa: F401  (the reference's names)
from mx_det.engine import init_device, load_frcnn_checkpoint

COCO_TESTSET_ROOT = Path("data/testsets/coco6")
CKPTS = {
    "FasterRCNN": Path("experiments/frcnn/baseline_clean/best.pth"),
    "FasterRCNN_aug": Path("experiments/frcnn/augmented/best.pth"),
}
OUT_DIR = Path("experiments/demo")
CONF_THRESHOLD = 0.35
N_SAMPLES = 5
SEED = 42
VIS_CONDITIONS = ["Test_Clean", "Test_Blur"]
TARGET_H = 480
JPEG_QUALITY = 92
EXTRAS = {"tta": "TTA", "bnadapt": "BNAdapt"}  # MX_DEMO_EXTRA name -> title suffix


def parse_extra(value):
    """MX_DEMO_EXTRA -> the strategy names in the order given, each once; a bad name raises ValueError."""
    names = [v.strip().lower() for v in (value or "").split(",") if v.strip()]
    bad = [v for v in names if v not in EXTRAS]
    if bad or len(set(names)) != len(names):
        raise ValueError(f"MX_DEMO_EXTRA: a comma-separated list of {sorted(EXTRAS)}, each at most once, got {value!r}")
    return names


def read_image(path, dev):
    """uint8 [H, W, 3] RGB on the device, or None when the file is missing (the reference skips such images)."""
    if not os.path.exists(path):
        return None
    with open(path, "rb") as f:
        data = f.read()
    try:
        return jpeg.decode(data, dev, entropy=jpeg.env_entropy())
    except (jpeg.JpegUnsupported, ValueError):  # progressive, CMYK, ...: PIL on the host, as the reference decodes
        import io
        from PIL import Image
        return torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()).to(dev)


def ground_truth(anns):
    """demo_inference.py:216-222: xywh -> xyxy of the annotations with w > 0 and h > 0."""
    boxes, labels = [], []
    for a in anns:
        x, y, w, h = a["bbox"]
        if w > 0 and h > 0:
            boxes.append([x, y, x + w, y + h])
            labels.append(a["category_id"])
    return boxes, labels


def detect(model, image, strategy=None):
    """The padded device detections of one RGB image under a strategy of MX_DEMO_EXTRA (None: plain)."""
    with torch.no_grad():
        if strategy == "tta":
            model.tta = mx_tta.TTA()
            try:
                return model.detect_padded([image])
            finally:
                model.tta = None
        if strategy == "bnadapt":
            with bn_adapt.BNAdapter(model, mode="batch"):
                return model.detect_padded([image])
        return model.detect_padded([image])


def generate_comparison(img_ids, model_pair, model_name, ann_clean, dev, extras=()):
    base_model, aug_model = model_pair
    clean_dir = COCO_TESTSET_ROOT / "Test_Clean" / "images" / "val"
    blur_dir = COCO_TESTSET_ROOT / "Test_Blur" / "images" / "val"
    with open(ann_clean, encoding="utf-8") as f:
        ds = json.load(f)
    info = {im["id"]: im for im in ds["images"]}
    anns = {}
    for a in ds["annotations"]:
        anns.setdefault(a["image_id"], []).append(a)
    overlay = draw.Overlay(CLASS_NAMES, CLASS_COLORS, conf_thr=CONF_THRESHOLD)
    written = []
    for img_id in img_ids:
        fname = info[img_id]["file_name"]
        clean, blur = read_image(clean_dir / fname, dev), read_image(blur_dir / fname, dev)
        if clean is None or blur is None:
            continue
        gt_boxes, gt_labels = ground_truth(anns.get(img_id, []))
        runs = [(f"Blur + {model_name} (Baseline)", base_model, None), (f"Blur + {model_name} (Augmented)", aug_model, None)]
        runs += [(f"Blur + {model_name} (Augmented, {EXTRAS[e]})", aug_model, e) for e in extras]
        dets = [detect(m, blur, s) for _, m, s in runs]
        # the reference draws on cv2's BGR images and hands them to cv2.imwrite
        clean_bgr, blur_bgr = clean.flip(2).contiguous(), blur.flip(2).contiguous()
        gtb = torch.tensor(gt_boxes, dtype=torch.float32).reshape(-1, 4).to(dev)
        gtl = torch.tensor(gt_labels, dtype=torch.int64).to(dev)
        counts = torch.cat([torch.tensor([len(gt_boxes)], dtype=torch.int32).to(dev)] + [d[3] for d in dets])
        panels, drawn = overlay.batch([clean_bgr] + [blur_bgr] * len(runs), [gtb] + [d[0][0] for d in dets],
                                      [gtl] + [d[2][0] for d in dets], [None] + [d[1][0] for d in dets], counts,
                                      ["Clean (Ground Truth)"] + [t for t, _, _ in runs])
        combined = draw.compose(panels, TARGET_H)
        drawn = drawn.tolist()  # the one read-back besides the finished file: the counts in its name
        if min(drawn) < 0:
            raise RuntimeError("detection NMS: a class segment exceeded max_seg (num_keep < 0)")
        n_gt, n_base, n_aug = len(gt_boxes), drawn[1], drawn[2]
        out_path = OUT_DIR / f"{model_name}_img{img_id:04d}_gt{n_gt}_base{n_base}_aug{n_aug}.jpg"
        jpeg.write_file(out_path, combined, quality=JPEG_QUALITY, bgr=True)
        written.append(out_path)
        print(f"  Saved: {out_path.name}  (GT={n_gt}, Base={n_base}, Aug={n_aug})", flush=True)
    return written


def main():
    extras = parse_extra(os.environ.get("MX_DEMO_EXTRA", ""))  # a bad value raises before any model loads
    dev, _, _ = init_device()
    print(f"Device: {dev}")
    print("Generating demo inference comparisons ...\n")
    ann_clean = str(COCO_TESTSET_ROOT / "Test_Clean" / "annotations" / "instances_val.json")
    img_ids = select_images(ann_clean, N_SAMPLES, SEED)
    print(f"Selected {len(img_ids)} images: {img_ids}\n")
    OUT_DIR.mkdir(parents=True, exist_ok=True)

    print("=" * 50 + "\n  Faster R-CNN: Baseline vs Augmented\n" + "=" * 50)
    base = load_frcnn_checkpoint(CKPTS["FasterRCNN"], dev)
    aug = load_frcnn_checkpoint(CKPTS["FasterRCNN_aug"], dev)
    written = generate_comparison(img_ids, (base, aug), "FRCNN", ann_clean, dev, extras)
    del base, aug
    torch.cuda.empty_cache()

    print("\n  RT-DETR-L / YOLOv8m: Ultralytics branches not part of this build (skipped)")
    print(f"\nAll demo images saved to: {OUT_DIR.resolve()}")
    return written


if __name__ == "__main__":
    main()
