"""Detection-postprocess micro-benchmark at the eval shape (N = 2 images, 1000 proposal rows per image,
C = 7): the per-image torch tail (RoIHeads.postprocess_detections + GeneralizedRCNNTransform.postprocess,
two compactions and one NMS count read back per image) against the fused device tail
(ops.detections_postprocess + the one counts.tolist() the model does per batch), on the same seeded
random inputs. Both are timed from the host's point of view (they end in a host read) with HIP events
and a wall clock, alternating in rounds after a warm-up; prints every round, the medians and the spread,
and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import torch  # noqa: E402

from mx_det import frcnn, ops  # noqa: E402
from mx_det.backend import HipBackend  # noqa: E402


def inputs(N, per, C, bg_bias, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    R = N * per
    sizes, original = [(800, 1333), (800, 1201)][:N] + [(800, 1333)] * max(0, N - 2), [(480, 800)] * N
    ctr = torch.rand(R, 2, generator=g) * torch.tensor([1333., 800.])
    wh = torch.rand(R, 2, generator=g) * 120 + 4
    rois = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    logits = torch.randn(R, C, generator=g) * 2
    logits[:, 0] += bg_bias  # a detector's rows are mostly background
    reg = torch.randn(R, 4 * C, generator=g) * 0.5
    return logits.to(dev), reg.to(dev), rois.to(dev), sizes, original


def timed(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3, (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--bg-bias", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_postprocess: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    N, per, C = a.images, a.rows, a.classes
    be = HipBackend("f32")
    heads = frcnn.RoIHeads(None, None)
    tf = frcnn.GeneralizedRCNNTransform()
    logits, reg, rois, sizes, original = inputs(N, per, C, a.bg_bias, dev)
    props = list(rois.split(per))
    img = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(per)
    hw = torch.tensor(sizes, dtype=torch.float32).to(dev)
    ratios = (torch.tensor(original, dtype=torch.float32) / torch.tensor(sizes, dtype=torch.float32)).to(dev)
    D = heads.detections_per_img

    def present():
        return tf.postprocess(heads.postprocess_detections(logits, reg, props, sizes, be), sizes, original)

    def fused():
        ob, osc, ol, counts = ops.detections_postprocess(logits, reg, rois, img, hw, N, heads.score_thresh,
                                                         heads.nms_thresh, D, ratios=ratios, max_seg=per)
        return [{"boxes": ob[i, :c], "labels": ol[i, :c], "scores": osc[i, :c]} for i, c in enumerate(counts.tolist())]

    # same detections (torch's softmax may differ from the kernel's in the last bit)
    p, f = present(), fused()
    for x, y in zip(p, f):
        same = x["labels"].shape == y["labels"].shape and bool((x["labels"] == y["labels"]).all())
        ds = float((x["scores"] - y["scores"]).abs().max()) if same and x["scores"].numel() else float("nan")
        db = float((x["boxes"] - y["boxes"]).abs().max()) if same and x["boxes"].numel() else float("nan")
        print(f"detections {x['labels'].shape[0]} / {y['labels'].shape[0]} same labels {same} "
              f"max |dscore| {ds:.2e} max |dbox| {db:.2e}")
    for _ in range(3):  # warm-up of both shapes
        timed(present, a.reps)
        timed(fused, a.reps)
    rows = {"present": [], "fused": []}
    for r in range(a.rounds):
        for name, fn in (("present", present), ("fused", fused)):
            ev, wall = timed(fn, a.reps)
            rows[name].append((ev, wall))
            print(f"round {r} {name:8s} events {ev:8.1f} us/call   wall {wall:8.1f} us/call", flush=True)
    out = {"shape": {"images": N, "rows_per_image": per, "classes": C, "bg_bias": a.bg_bias}, "reps": a.reps,
           "rounds": a.rounds}
    for name, v in rows.items():
        ev = [x[0] for x in v]
        out[name] = {"events_us_median": statistics.median(ev), "events_us_min": min(ev), "events_us_max": max(ev),
                     "wall_us_median": statistics.median(x[1] for x in v)}
        print(f"{name:8s} median {out[name]['events_us_median']:.1f} us (min {min(ev):.1f}, max {max(ev):.1f})")
    out["speedup_events_median"] = out["present"]["events_us_median"] / out["fused"]["events_us_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
