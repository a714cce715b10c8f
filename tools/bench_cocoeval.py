"""COCOeval timing: the host evaluator (mx_det.coco.COCOeval evaluate + accumulate) against the device
path (mx_det.coco_device.DeviceCOCOeval evaluate + accumulate: sorts, segment tables, mx_coco_match,
mx_coco_accumulate and the copy of precision / recall / scores to the host) on a seeded synthetic
set the size of a VisDrone val split: 548 images, 6 classes, about 55 GT and 100 detections an image.

time.perf_counter around a synchronised region, after one warm-up of the device path; the host
evaluator runs once (it is seconds of Python), the device path `--reps` times (median, min..max).
The two results must be bit-identical before a time is reported.

    python tools/bench_cocoeval.py [--images 548] [--reps 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mx_det.coco import COCO, COCOeval  # noqa: E402
from mx_det.coco_device import DeviceCOCOeval  # noqa: E402


def synth(n_img, n_cls, seed=0):
    """(COCO gt, per-image (id, xyxy f32, score f32, label i64)): small objects on a 1360x765 frame,
    detections mostly near a GT of their class, a few crowd regions."""
    rng = np.random.default_rng(seed)
    anns, dets, aid = [], [], 1
    for img in range(1, n_img + 1):
        g = int(rng.integers(35, 76))
        xy = rng.uniform(0, [1300, 700], (g, 2))
        wh = rng.uniform(6, 120, (g, 2))
        cls = rng.integers(1, n_cls + 1, g)
        for j in range(g):
            b = [float(v) for v in (*xy[j], *wh[j])]
            anns.append({"id": aid, "image_id": img, "category_id": int(cls[j]), "bbox": b, "area": b[2] * b[3],
                         "iscrowd": int(rng.random() < 0.02)})
            aid += 1
        d = 100
        src = rng.integers(0, g, d)
        near = rng.random(d) < 0.7
        bxy = np.where(near[:, None], xy[src] + rng.normal(0, 4, (d, 2)), rng.uniform(0, [1300, 700], (d, 2)))
        bwh = np.where(near[:, None], np.maximum(wh[src] + rng.normal(0, 5, (d, 2)), 2), rng.uniform(6, 120, (d, 2)))
        lab = np.where(rng.random(d) < 0.9, cls[src], rng.integers(1, n_cls + 1, d))
        boxes = np.concatenate([bxy, bxy + bwh], 1).astype(np.float32)
        dets.append((img, boxes, rng.random(d).astype(np.float32), lab.astype(np.int64)))
    gt = COCO({"images": [{"id": i} for i in range(1, n_img + 1)], "annotations": anns,
               "categories": [{"id": c, "name": f"c{c}"} for c in range(1, n_cls + 1)]})
    return gt, dets


def host_results(dets):
    """The result dicts of engine.evaluate's host loop."""
    res = []
    for img, boxes, scores, labels in dets:
        for (x1, y1, x2, y2), sc, lb in zip(boxes.tolist(), scores.tolist(), labels.tolist()):
            res.append({"image_id": img, "category_id": int(lb), "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(sc)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=548)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cocoeval: no GPU")
    dev = torch.device("cuda:0")
    gt, dets = synth(args.images, args.classes)
    dev_dets = [(img, torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), torch.from_numpy(lb).to(dev))
                for img, b, s, lb in dets]

    def device_run():
        ev = DeviceCOCOeval(gt, dev)
        for d in dev_dets:
            ev.add(*d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev.accumulate()  # ends with the results on the host
        torch.cuda.synchronize()
        return ev, t1 - t0, time.perf_counter() - t1

    device_run()  # warm-up: code objects, torch's sort / unique workspaces
    runs = [device_run() for _ in range(args.reps)]
    dev_ev = runs[-1][0]

    hev = COCOeval(gt, gt.loadRes(host_results(dets)), "bbox")
    t0 = time.perf_counter()
    hev.evaluate()
    t1 = time.perf_counter()
    hev.accumulate()
    t2 = time.perf_counter()
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(hev.eval[name], dev_ev.eval[name]), f"{name} differs from the host evaluator"

    tot = [e + a for _, e, a in runs]
    row = {"images": args.images, "classes": args.classes, "gt": len(gt.dataset["annotations"]),
           "detections": sum(len(d[2]) for d in dets), "reps": args.reps,
           "host_evaluate_s": t1 - t0, "host_accumulate_s": t2 - t1, "host_total_s": t2 - t0,
           "device_evaluate_ms": statistics.median(e for _, e, _ in runs) * 1e3,
           "device_accumulate_ms": statistics.median(a for _, _, a in runs) * 1e3,
           "device_total_ms": statistics.median(tot) * 1e3, "device_total_min_ms": min(tot) * 1e3,
           "device_total_max_ms": max(tot) * 1e3, "bit_identical": True}
    row["ratio"] = row["host_total_s"] * 1e3 / row["device_total_ms"]
    print(json.dumps(row), flush=True)
    print(f"\nhost   evaluate {row['host_evaluate_s']:.2f} s + accumulate {row['host_accumulate_s']:.2f} s = "
          f"{row['host_total_s']:.2f} s")
    print(f"device evaluate {row['device_evaluate_ms']:.1f} ms + accumulate {row['device_accumulate_ms']:.1f} ms = "
          f"{row['device_total_ms']:.1f} ms ({row['device_total_min_ms']:.1f}..{row['device_total_max_ms']:.1f}), "
          f"{row['ratio']:.0f}x, results bit-identical")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
