"""JPEG decode micro-benchmark: the scan decoded on the device (mx_det.jpeg.decode(entropy="device"):
file bytes up, mx_jpeg_entropy_decode, mx_jpeg_reconstruct, one read of the status word) against the
default path (host mx_jpeg_decode_coefs into pinned memory + coefficient copy + mx_jpeg_reconstruct)
and against PIL (Image.open().convert("RGB") + copy of the pixels), per image, on the images of
tools/bench_jpeg_encode.py saved by PIL at quality 95 (4:2:0), and at 1333x800.

Host clock around work that ends with the pixels on the device (every path is followed by a device
synchronisation). The three paths alternate inside every repeat; a round is `--reps` repeats and
yields one median per path; the table shows the median of the round medians and their min..max (the
run-to-run spread). "entropy passes" is the device-event time of mx_jpeg_entropy_decode's launches
alone, "host entropy" the host clock of mx_jpeg_decode_coefs alone; the last columns are the bytes
each path copies to the device. --subseq lists subsequence sizes to time the entropy passes at.

    python tools/bench_jpeg_decode.py [--rounds 7] [--reps 15] [--subseq 256,512,1024,2048] [--json out.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd"), os.path.join(ROOT, "tools")]

import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from bench_jpeg_encode import SIZES, image  # noqa: E402
from mx_det import _lib, jpeg  # noqa: E402

DECODE_SIZES = SIZES + [(800, 1333)]


def pil_path(data, dev):
    return torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()).to(dev)


def entropy_times(data, dev, reps, sizes):
    """Device-event time per call (us) of the entropy passes at every subsequence size, and the host
    clock (ms) of the sequential host decoder."""
    info = jpeg.parse(data)
    lib = _lib.load()
    scan = torch.from_numpy(np.frombuffer(data, dtype=np.uint8)[info.scan_off:].copy()).to(dev)
    coefs = torch.empty(info.coef_total, dtype=torch.int16, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ref = torch.from_numpy(jpeg.decode_coefs(data, info)[1]).to(dev)
    res = {}
    for s in sizes:
        jpeg.set_subseq(s)
        ws = torch.empty(lib.mx_jpeg_entropy_decode_workspace(ctypes.byref(info), scan.numel()), dtype=torch.uint8,
                         device=dev)

        def ent():
            _lib.call("mx_jpeg_entropy_decode", scan.data_ptr(), scan.numel(), ctypes.byref(info), ws.data_ptr(),
                      ws.numel(), coefs.data_ptr(), status.data_ptr(), _lib.stream())

        ent()
        assert int(status.item()) == 0 and torch.equal(coefs, ref)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            ent()
        b.record()
        torch.cuda.synchronize()
        res[str(s)] = a.elapsed_time(b) / reps * 1e3
    jpeg.set_subseq(512)
    pinned = torch.empty(info.coef_total, dtype=torch.int16, pin_memory=True)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        jpeg.decode_coefs(data, info, out=pinned)
        ms.append((time.perf_counter() - t0) * 1e3)
    return res, statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--subseq", default="512")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode: no GPU")
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in args.subseq.split(",")]
    paths = {
        "host": lambda d: jpeg.decode(d, dev, entropy="host"),
        "device": lambda d: jpeg.decode(d, dev, entropy="device"),
        "cpu_pil": lambda d: pil_path(d, dev),
    }
    results = []
    for H, W in DECODE_SIZES:
        b = io.BytesIO()
        Image.fromarray(image(H, W)).save(b, format="JPEG", quality=95)
        data = b.getvalue()
        ref = pil_path(data, dev)
        for name, fn in paths.items():  # warm-up + the pixels must be PIL's
            for _ in range(3):
                got = fn(data)
            assert torch.equal(got, ref), name
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):
            ms = {k: [] for k in paths}
            for _ in range(args.reps):
                for name, fn in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(data)
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            for k in paths:
                rounds[k].append(statistics.median(ms[k]))
        info = jpeg.parse(data)
        row = {"H": H, "W": W, "file_bytes": len(data), "coef_bytes": int(info.coef_total) * 2, "rounds": args.rounds,
               "reps": args.reps}
        for k in paths:
            row[k] = {"median_ms": statistics.median(rounds[k]), "min_ms": min(rounds[k]), "max_ms": max(rounds[k])}
        row["entropy_us"], row["host_entropy_ms"] = entropy_times(data, dev, 30, sizes)
        results.append(row)
        print(json.dumps(row), flush=True)
    print("\n| image | host entropy + copy + reconstruct | device entropy + reconstruct | PIL + copy | host entropy alone | "
          "entropy passes | bytes up: host | device |")
    print("|---|---|---|---|---|---|---|---|")
    for r in results:
        f = lambda d: f"{d['median_ms']:.2f} ms ({d['min_ms']:.2f}..{d['max_ms']:.2f})"  # noqa: E731
        ent = ", ".join(f"{v:.0f} us (S={k})" for k, v in r["entropy_us"].items())
        print(f"| {r['W']}x{r['H']} | {f(r['host'])} | {f(r['device'])} | {f(r['cpu_pil'])} | {r['host_entropy_ms']:.2f} ms | "
              f"{ent} | {r['coef_bytes'] / 1e3:.0f} kB | {r['file_bytes'] / 1e3:.0f} kB |")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
