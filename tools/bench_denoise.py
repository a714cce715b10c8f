"""Device time of one mx_denoise_nlm_u8 call beside the two things it stands next to, the U-Net forward
(RestorationUNet.restore_u8, the reference's channel widths, random weights) and mx_degradation_stats_u8, at
the same shapes in one session: 1 x 800 x 1333 and 8 x 256 x 256, once with every image denoised and once with
every image passed. Warm caches, device events on the stream around `inner` back-to-back calls, the median
over `reps` such windows. Prints one JSON line per shape and a table; --out writes both to a file.

    python tools/bench_denoise.py --out profiles/denoise_nlm_cost.txt
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "robust-object-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mx_det import ops  # noqa: E402
from mx_det.unet import RestorationUNet  # noqa: E402

SHAPES = (("1x800x1333", (1, 800, 1333)), ("8x256x256", (8, 256, 256)))


def timed(fn, reps, inner, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def content(b, h, w, seed):
    """Piecewise-smooth content under sigma 15 noise (the recipe of tests/gate_ref.content_images): the noise
    rule fires, and the candidates' weights spread over the table as they do on a noisy photograph."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(b):
        img = np.empty((h, w, 3), np.float64)
        img[:] = rng.integers(60, 200, 3)
        for _ in range(40):
            y0, x0 = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 8))
            img[y0:y0 + int(rng.integers(8, h // 2)), x0:x0 + int(rng.integers(8, w // 2))] = rng.integers(20, 236, 3)
        img += (10.0 * np.sin(2 * np.pi * xx / 77.0) * np.sin(2 * np.pi * yy / 53.0))[..., None]
        img += rng.normal(0.0, 15.0, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return np.stack(out)


ROUTES = (("nlm_every_image_denoised", "mx_denoise_nlm_u8, blind, every image denoised"),
          ("nlm_every_image_passed", "mx_denoise_nlm_u8, blind, every image passed (copied)"),
          ("degradation_stats", "mx_degradation_stats_u8"),
          ("unet_restore_u8", "RestorationUNet.restore_u8"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    unet = RestorationUNet(channels=(32, 64, 128, 256)).to(dev).eval()
    lines = []
    table = ["| shape | call | ms per call: median (min..max) |", "|---|---|---|"]
    for name, (b, h, w) in SHAPES:
        x = torch.from_numpy(content(b, h, w, 1)).to(dev)
        out = torch.empty_like(x)
        stats, verdict = ops.degradation_stats_u8(x)
        so = (torch.empty_like(stats), torch.empty_like(verdict))
        _, applied = ops.denoise_nlm_u8(x, stats=stats, out=out)
        _, passed = ops.denoise_nlm_u8(x, stats=stats, rule=(0, 1), out=out)
        assert applied.cpu().tolist() == [1] * b and passed.cpu().tolist() == [0] * b
        r = {"shape": [b, h, w], "reps": args.reps, "inner": args.inner,
             "sigma": [round(v[1] / v[0] * 1.2533 / 6, 2) for v in stats.cpu().tolist()]}
        r["nlm_every_image_denoised"] = timed(lambda: ops.denoise_nlm_u8(x, stats=stats, out=out), args.reps, args.inner)
        r["nlm_every_image_passed"] = timed(lambda: ops.denoise_nlm_u8(x, stats=stats, rule=(0, 1), out=out), args.reps, args.inner)
        r["degradation_stats"] = timed(lambda: ops.degradation_stats_u8(x, out=so), args.reps, args.inner)
        with torch.no_grad():
            r["unet_restore_u8"] = timed(lambda: unet.restore_u8(x), args.reps, max(1, args.inner // 4))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        for key, label in ROUTES:
            t = r[key]
            table.append(f"| {name} | {label} | {t['median_ms']:.4f} ({t['min_ms']:.4f}..{t['max_ms']:.4f}) |")
    print("\n".join(table))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    main()
