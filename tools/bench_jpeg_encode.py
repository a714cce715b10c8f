"""JPEG encode micro-benchmark: the device encoder (mx_det.jpeg.encode, bytes on the host at the end)
against the path it replaces in the test-set writers (.cpu() + PIL save(quality=95)), and the device
entropy coder against the host one (entropy="host"), per image, at 1360x765 and 2000x1500.

Host clock around work that ends with the bytes on the host (every path synchronises itself). The
three paths alternate inside every repeat; a round is `--reps` repeats and yields one median per path;
the table shows the median of the round medians and their min..max (the run-to-run spread). Stage
times (pixel stage, entropy passes) are device-event times of the kernels alone.

    python tools/bench_jpeg_encode.py [--rounds 7] [--reps 15] [--json out.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from mx_det import _lib, jpeg  # noqa: E402
from mx_det.data import synth_image  # noqa: E402

SIZES = [(765, 1360), (1500, 2000)]  # (H, W)


def image(H, W):
    """A scene-like image with sensor-like noise (sigma 8): the kind of picture the writers encode."""
    g = np.random.default_rng(0)
    img = synth_image(0, H, W).astype(np.float32) + g.normal(0, 8, (H, W, 3)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def pil_path(dev_img):
    b = io.BytesIO()
    Image.fromarray(dev_img.cpu().numpy()).save(b, format="JPEG", quality=95)
    return b.getvalue()


def stage_times(dev_img, reps):
    """Device-event time per call (us) of the pixel stage and of the entropy passes."""
    H, W = dev_img.shape[:2]
    info = jpeg.encode_info(W, H, 95, 2)
    lib = _lib.load()
    ws = torch.empty(lib.mx_jpeg_entropy_workspace(ctypes.byref(info)), dtype=torch.uint8, device=dev_img.device)
    cap = int(lib.mx_jpeg_scan_bound(ctypes.byref(info)))
    out = torch.empty(cap, dtype=torch.uint8, device=dev_img.device)
    n = torch.empty(1, dtype=torch.int64, device=dev_img.device)
    coefs = jpeg.forward(dev_img, info)

    def fwd():
        jpeg.forward(dev_img, info)

    def ent():
        _lib.call("mx_jpeg_entropy", coefs.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), out.data_ptr(),
                  cap, n.data_ptr(), _lib.stream())

    res = {}
    for name, fn in (("forward_us", fwd), ("entropy_us", ent)):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[name] = a.elapsed_time(b) / reps * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode: no GPU")
    dev = torch.device("cuda:0")
    paths = {
        "device": lambda t: jpeg.encode(t, 95),
        "host_entropy": lambda t: jpeg.encode(t, 95, entropy="host"),
        "cpu_pil": pil_path,
    }
    results = []
    for H, W in SIZES:
        t = torch.from_numpy(image(H, W)).to(dev)
        ref = pil_path(t)
        for name, fn in paths.items():  # warm-up + the bytes must be PIL's
            for _ in range(3):
                got = fn(t)
            assert got == ref, name
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):
            ms = {k: [] for k in paths}
            for _ in range(args.reps):
                for name, fn in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(t)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            for k in paths:
                rounds[k].append(statistics.median(ms[k]))
        row = {"H": H, "W": W, "file_bytes": len(ref), "rounds": args.rounds, "reps": args.reps}
        for k in paths:
            row[k] = {"median_ms": statistics.median(rounds[k]), "min_ms": min(rounds[k]), "max_ms": max(rounds[k])}
        row.update(stage_times(t, 50))
        results.append(row)
        print(json.dumps(row), flush=True)
    print("\n| image | file | device encode | host entropy | .cpu() + PIL | pixel stage | entropy passes |")
    print("|---|---|---|---|---|---|---|")
    for r in results:
        f = lambda d: f"{d['median_ms']:.2f} ms ({d['min_ms']:.2f}..{d['max_ms']:.2f})"  # noqa: E731
        print(f"| {r['W']}x{r['H']} | {r['file_bytes'] / 1e3:.0f} kB | {f(r['device'])} | {f(r['host_entropy'])} | "
              f"{f(r['cpu_pil'])} | {r['forward_us']:.0f} us | {r['entropy_us']:.0f} us |")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
