"""Patch-loader benchmark of U-Net restoration training (scripts/train_restoration.py), three parts:

(a) kernel   device-event time of mx_jpeg_reconstruct_window for a 256x256 window at an unaligned
             origin of a 1920x1080 frame against mx_jpeg_reconstruct of the same coefficients (the
             whole frame; workspace and output allocated outside the timed loop). The two alternate
             inside every repeat, `--calls` calls between two events.
(b) loader   patches/s of one epoch of each loader alone, ending with the batches in HBM and a device
             synchronisation: the host path (DataLoader over RestorationDataset: PIL decode, crop, pinned
             copy) and restoration.DevicePatchLoader with MX_JPEG_DECODE=host and =device.
(c) step     wall time per restoration.train_epoch step (batch 8, 256x256, f32 U-Net, mx AdamW) with
             each of the three loaders, DevicePatchLoader.wait_s per step, and the same step on patches
             resident in HBM (a list of device batches: what bench.py --mode unet_train times).

Frames: data.synth_image written by PIL at quality 95, 4:2:0, in the VisDrone sizes 1360x765,
1920x1080 and 2000x1500 (`--files` of them, the sizes in turn), in a temporary directory. Every figure
is the median of `--repeats` repeats after one warm-up pass, with max - min as the spread; the
variants of a part alternate inside a repeat. Needs a GPU.

    python tools/bench_patch_loader.py [--files 48] [--repeats 5] [--calls 200] [--parts abc] [--workers 4]\
                                         [--json out.json]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import torch  # noqa: E402
from PIL import Image  # noqa: E402

from mx_det import _lib, jpeg  # noqa: E402
from mx_det import optim as mx_optim  # noqa: E402
from mx_det.data import synth_image  # noqa: E402
from mx_det.restoration import (CombinedLoss, DevicePatchLoader, RestorationBatcher, RestorationDataset,  # noqa: E402
                                collate_u8, train_epoch)
from mx_det.unet import RestorationUNet  # noqa: E402

SIZES = [(765, 1360), (1080, 1920), (1500, 2000)]  # H, W
PATCH, BATCH = 256, 8


def summary(xs):
    return {"median": statistics.median(xs), "spread": max(xs) - min(xs), "n": len(xs)}


def write_frames(root, n):
    for i in range(n):
        H, W = SIZES[i % len(SIZES)]
        Image.fromarray(synth_image(i, H, W)).save(os.path.join(root, f"{i:05d}.jpg"), quality=95)


def kernel_part(dev, repeats, calls):
    import io
    b = io.BytesIO()
    Image.fromarray(synth_image(1, 1080, 1920)).save(b, format="JPEG", quality=95)
    info, coefs = jpeg.decode_coefs(b.getvalue())
    coefs = torch.from_numpy(coefs).to(dev)
    box = (333, 217, PATCH, PATCH)
    ws = torch.empty(_lib.load().mx_jpeg_workspace(ctypes.byref(info)), dtype=torch.uint8, device=dev)
    full = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((PATCH, PATCH, 3), dtype=torch.uint8, device=dev)

    def run_full():
        _lib.call("mx_jpeg_reconstruct", coefs.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), full.data_ptr(),
                  0, _lib.stream())

    def run_window():
        jpeg.reconstruct_window(info, coefs, box, out=out)

    fns = {"window_256x256": run_window, "full_1920x1080": run_full}
    for fn in fns.values():  # warm-up
        for _ in range(10):
            fn()
    assert torch.equal(out, full[box[1]:box[1] + PATCH, box[0]:box[0] + PATCH])
    us = {k: [] for k in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            e.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(e) / calls * 1e3)
    cover = jpeg.window_cover(info, box)
    blocks = sum(int((c[2] - c[0]) * (c[3] - c[1])) for c in cover)
    return {"box": box, "calls": calls, "window_cover_blocks": blocks, "frame_blocks": int(info.coef_total) // 64,
            "us_per_call": {k: summary(v) for k, v in us.items()}}


def make_loaders(root, dev, workers=4):
    host = torch.utils.data.DataLoader(RestorationDataset(root, PATCH, is_train=True), batch_size=BATCH, shuffle=True,
                                       num_workers=0, pin_memory=True, drop_last=True, collate_fn=collate_u8)
    device = DevicePatchLoader(root, PATCH, BATCH, True, dev, shuffle=True, drop_last=True, workers=workers)
    return {"host_dataloader": (host, None), "device_loader_host_entropy": (device, "host"),
            "device_loader_device_entropy": (device, "device")}


def use(entropy):
    if entropy is not None:
        os.environ["MX_JPEG_DECODE"] = entropy


def loader_part(root, dev, repeats, workers):
    loaders = make_loaders(root, dev, workers)

    def epoch(loader):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for batch in loader:
            n += batch.to(dev, non_blocking=True).shape[0]
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    rate = {k: [] for k in loaders}
    for rep in range(repeats + 1):  # the first pass warms up
        for name, (loader, entropy) in loaders.items():
            use(entropy)
            r = epoch(loader)
            if rep:
                rate[name].append(r)
    return {"patches_per_s": {k: summary(v) for k, v in rate.items()},
            "host_fallbacks": loaders["device_loader_host_entropy"][0].host_fallbacks}


def step_part(root, dev, repeats, workers):
    torch.manual_seed(42)
    model = RestorationUNet(channels=(32, 64, 128, 256)).to(dev)
    opt = mx_optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    crit, batcher = CombinedLoss(0.3), RestorationBatcher(dev)
    loaders = make_loaders(root, dev, workers)
    steps = len(loaders["host_dataloader"][0])
    use("host")
    resident = [b.clone() for b in loaders["device_loader_host_entropy"][0]]
    loaders["resident_in_hbm"] = (resident, None)
    ms, wait = {k: [] for k in loaders}, {k: [] for k in loaders if k.startswith("device")}
    for rep in range(repeats + 1):
        for name, (loader, entropy) in loaders.items():
            use(entropy)
            w0 = getattr(loader, "wait_s", 0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_epoch(model, loader, batcher, opt, crit, log_every=1 << 30, epoch=rep)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                ms[name].append(dt / steps * 1e3)
                if name in wait:
                    wait[name].append((loader.wait_s - w0) / steps * 1e3)
    return {"steps_per_epoch": steps, "ms_per_step": {k: summary(v) for k, v in ms.items()},
            "wait_ms_per_step": {k: summary(v) for k, v in wait.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--workers", type=int, default=4, help="DevicePatchLoader's host worker threads")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_loader: no GPU")
    if args.repeats < 3:
        raise SystemExit("bench_patch_loader: at least three repeats")
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    random.seed(42)
    res = {"device": torch.cuda.get_device_name(0), "files": args.files, "repeats": args.repeats,
           "sizes": [f"{w}x{h}" for h, w in SIZES], "patch": PATCH, "batch": BATCH, "workers": args.workers}
    if "a" in args.parts:
        res["kernel"] = kernel_part(dev, args.repeats, args.calls)
        print(json.dumps({"kernel": res["kernel"]}), flush=True)
    if "b" in args.parts or "c" in args.parts:
        with tempfile.TemporaryDirectory() as root:
            write_frames(root, args.files)
            if "b" in args.parts:
                res["loader"] = loader_part(root, dev, args.repeats, args.workers)
                print(json.dumps({"loader": res["loader"]}), flush=True)
            if "c" in args.parts:
                res["step"] = step_part(root, dev, args.repeats, args.workers)
                print(json.dumps({"step": res["step"]}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
