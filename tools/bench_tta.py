"""What flip test-time augmentation (mx_det.tta.TTA) costs on the device, in one session on one GPU.

Forward: the detector's eval forward, model(images) on 1 x 800 x 1333 with the fused detection tail on,
through three routes that alternate inside every round:

  plain    one view (today's fused eval)
  tta      model.tta = TTA(): the image and its mirror through the trunk, folded, one NMS, box voting
  plain-2  plain again, last in every round: its distance from `plain` is the drift of the measurement

Tail: on the doubled candidates of that tta forward (its recorded box-head outputs, after
detection_candidates and the grouped NMS), the back half alone:

  select       ops.detection_select on the folded candidates (no voting)
  fold+vote    ops.detection_views_fold + ops.detection_select_vote

A route's time is the device-event time of `--reps` calls back to back divided down to one call; a round
yields one time per route; the tables show the median of the rounds and their min..max. Every route is
warmed up first. Random seeded weights: nearly every candidate passes the score threshold, so the tail
works on far more live candidates (shown) than a trained detector leaves it.

    python tools/bench_tta.py [--rounds 7] [--reps 10] [--precision f32] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import torch  # noqa: E402

from mx_det import frcnn, ops  # noqa: E402
from mx_det.backend import HipBackend  # noqa: E402
from mx_det.data import synth_batch  # noqa: E402
from mx_det.tta import TTA  # noqa: E402


class Recorder:
    """The HIP backend with the latest detections_postprocess_views call kept."""

    def __init__(self, be):
        self._be, self.last = be, None

    def __getattr__(self, k):
        return getattr(self._be, k)

    def detections_postprocess_views(self, *a, **kw):
        self.last = (a, kw)
        return self._be.detections_postprocess_views(*a, **kw)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per call


def rounds(fns, n, reps):
    for fn in fns.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {r: [] for r in fns}
    for _ in range(n):
        for r, fn in fns.items():
            ms[r].append(timed(fn, reps))
    return {r: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for r, v in ms.items()}


def table(title, res, base):
    print(f"\n| {title} | ms per call: median (min..max) | vs {base} |")
    print("|---|---|---|")
    b = res[base]["median_ms"]
    for r, v in res.items():
        d = "" if r == base else f"{v['median_ms'] - b:+.3f} ms (x{v['median_ms'] / b:.2f})"
        print(f"| {r} | {v['median_ms']:.3f} ({v['min_ms']:.3f}..{v['max_ms']:.3f}) | {d} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--vote-iou", type=float, default=0.8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta: no GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    model.roi_heads.box_predictor = frcnn.FastRCNNPredictor(model.roi_heads.box_predictor.cls_score.in_features, 7)
    rec = Recorder(HipBackend(args.precision))
    model = model.to(dev).eval().set_backend(rec)
    model.roi_heads.fused_detections = True
    imgs = list(synth_batch(0, 1, H=800, W=1333, device=dev)[0])
    tta = TTA(vote_iou=args.vote_iou)
    kept = {}

    def forward(route):
        def run():
            model.tta = tta if route == "tta" else None
            with torch.no_grad():
                kept[route] = model(imgs)
        return run

    fwd = rounds({r: forward(r) for r in ("plain", "tta", "plain-2")}, args.rounds, args.reps)
    for r in fwd:
        fwd[r]["detections"] = int(kept[r][0]["scores"].shape[0])

    # the tail alone, on the candidates of the recorded tta forward
    (logits, reg, rois, img, hw, N, V, flips, thr, nms_thr, D, vote_iou), kw = rec.last
    C, P = logits.shape[1], logits.shape[0] // (V * N)
    scores, boxes, labels, grp = ops.detection_candidates(logits, reg, rois, img, hw.repeat(V, 1), V * N, thr)
    fboxes, fgrp = ops.detection_views_fold(boxes, grp, hw, V, N, P, C, flips)
    keep, nk = ops.batched_nms_grouped(fboxes, scores, labels, fgrp, N, C, nms_thr, V * max(P, 1000))
    ratios = kw.get("ratios")
    tail = rounds({
        "select": lambda: ops.detection_select(keep, nk, fboxes, scores, labels, fgrp, N, D, ratios),
        "fold+vote": lambda: (ops.detection_views_fold(boxes, grp, hw, V, N, P, C, flips),
                              ops.detection_select_vote(keep, nk, fboxes, scores, labels, fgrp, V, N, P, C, D, vote_iou,
                                                        ratios)),
    }, args.rounds, args.reps * 10)
    res = {"shape": [1, 800, 1333], "precision": args.precision, "rounds": args.rounds, "reps": args.reps,
           "vote_iou": vote_iou, "forward": fwd, "tail": tail,
           "candidates": {"slots": int(scores.shape[0]), "live": int((fgrp < N).sum()), "survivors": int(nk)}}
    print(json.dumps(res), flush=True)
    table("forward", fwd, "plain")
    table("tail", tail, "select")
    print(f"\ncandidates: {res['candidates']}; detections: " + ", ".join(f"{r} {v['detections']}" for r, v in fwd.items()))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
