"""What test-time BatchNorm adaptation (mx_det.adapt.BNAdapter) costs on the device: the detector's eval
forward, model(images) on 1 x 800 x 1333 with the fused detection tail on (MX_FUSED_DETECTIONS=1), through
five routes:

  off      no adapter: BatchNorm folded into the convs (today's eval)
  batch    adapter, mode "batch"  (conv with statistics -> mx_bn_finalize_adapt -> mx_bn_apply, 61 layers)
  stream   adapter, mode "stream" (the same launches, plus the f64 state per layer)
  frozen   adapter, mode "stream" after freeze(): the folded convs with the adapter's statistics
  off-2    off again, last in every round: its distance from `off` is the drift of the measurement

The routes alternate inside every round. A route's time is the device-event time of `--reps` forwards back
to back (each ends in the detections, nothing is read back between them), divided down to one forward; a
round yields one time per route; the table shows the median of the rounds and their min..max, and the
difference of each median from `off`. Every route is warmed up first (code objects, conv tuning, scratch).
Random seeded weights: the forward's cost does not depend on what the detector has learnt, except through
the number of detections kept (shown). Kernel-level sums come from a profiler run of their own:

    python tools/bench_bn_adapt.py [--rounds 7] [--reps 10] [--precision f32] [--json out.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_bn_adapt.py --rounds 1 --reps 5 --routes stream
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import torch  # noqa: E402

from mx_det import frcnn  # noqa: E402
from mx_det.adapt import BNAdapter  # noqa: E402
from mx_det.backend import HipBackend  # noqa: E402
from mx_det.data import synth_batch  # noqa: E402

ROUTES = ("off", "batch", "stream", "frozen", "off-2")


def build(dev, precision):
    torch.manual_seed(0)
    m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    m.roi_heads.box_predictor = frcnn.FastRCNNPredictor(m.roi_heads.box_predictor.cls_score.in_features, 7)
    return m.to(dev).eval().set_backend(HipBackend(precision))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--routes", default=",".join(ROUTES), help="comma-separated subset (a profiler run takes one)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_adapt: no GPU")
    routes = tuple(r for r in args.routes.split(",") if r)
    if not routes or any(r not in ROUTES for r in routes):
        raise SystemExit(f"bench_bn_adapt: --routes takes names among {ROUTES}")
    os.environ["MX_FUSED_DETECTIONS"] = "1"
    dev = torch.device("cuda:0")
    model = build(dev, args.precision)
    imgs = list(synth_batch(0, 1, H=800, W=1333, device=dev)[0])
    adapters = {"batch": BNAdapter(model, mode="batch", prior=16), "stream": BNAdapter(model, mode="stream", prior=16),
                "frozen": BNAdapter(model, mode="stream", prior=16)}
    kept = {}

    def forward(route):
        ad = adapters.get(route)

        def run():
            with torch.no_grad():
                if ad is None:
                    out = model(imgs)
                else:
                    with ad:
                        out = model(imgs)
            kept[route] = out
        return run

    fns = {r: forward(r) for r in routes}
    if "frozen" in fns:  # statistics of 4 forwards, then frozen for good
        for _ in range(4):
            fns["frozen"]()
        adapters["frozen"].freeze()
    for fn in fns.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {r: [] for r in routes}
    for _ in range(args.rounds):
        for r, fn in fns.items():
            ms[r].append(timed(fn, args.reps))
    res = {"shape": [1, 800, 1333], "precision": args.precision, "rounds": args.rounds, "reps": args.reps, "routes": {}}
    for r in routes:
        o = kept[r][0]
        res["routes"][r] = {"median_ms": statistics.median(ms[r]), "min_ms": min(ms[r]), "max_ms": max(ms[r]),
                            "detections": int(o["scores"].shape[0])}
    print(json.dumps(res), flush=True)
    base = res["routes"].get("off", {}).get("median_ms")
    print("\n| route | ms per forward: median (min..max) | vs off | detections |")
    print("|---|---|---|---|")
    for r in routes:
        v = res["routes"][r]
        d = "" if base is None or r == "off" else f"{v['median_ms'] - base:+.3f} ms ({(v['median_ms'] / base - 1) * 100:+.1f} %)"
        print(f"| {r} | {v['median_ms']:.3f} ({v['min_ms']:.3f}..{v['max_ms']:.3f}) | {d} | {v['detections']} |")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
