"""Optimizer step of the restoration U-Net (RestorationUNet((32, 64, 128, 256)), f32 mode) with
synthetic gradients: time per optimizer step INCLUDING the following WeightPacker.refresh() (the
operand pack the next forward needs), for

    torch   torch.optim.AdamW (foreach) + refresh         -- what the training script ran before
    plain   mx_det.optim.AdamW, MX_ADAMW_PACK=0 (mx_adamw_step) + refresh
    fused   mx_det.optim.AdamW (mx_adamw_pack_step; refresh finds nothing to do)

    python tools/bench_adamw.py [--steps 50] [--warmup 10] [--repeats 3] [--launches]

Per configuration and repeat: device time per step from events around `steps` steps after `warmup`
steps (the stream is otherwise idle, so this is max(host, device) per step), and the host wall time of
the step() call alone. Prints one JSON line per configuration with every repeat and the spread.
--launches: also count the device kernels of one step + refresh with torch.profiler.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import torch  # noqa: E402

from mx_det import conv as mc  # noqa: E402
from mx_det import optim  # noqa: E402
from mx_det.unet import RestorationUNet  # noqa: E402

CONFIGS = ("torch", "plain", "fused")


def make_opt(kind, params):
    optim._ADAMW_PACK = 1 if kind == "fused" else 0
    cls = torch.optim.AdamW if kind == "torch" else optim.AdamW
    return cls(params, lr=1e-3, weight_decay=1e-4)


def measure(kind, params, pk, steps, warmup):
    opt = make_opt(kind, params)

    def one():
        t = time.perf_counter()
        opt.step()
        dt = time.perf_counter() - t
        pk.refresh()
        return dt

    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = 0.0
    a.record()
    for _ in range(steps):
        host += one()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps, host * 1e6 / steps, opt


def launches(opt, pk):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        opt.step()
        pk.refresh()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
             and not e.name.lower().startswith(("memcpy", "memset"))]
    return len(names), sorted(set(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = RestorationUNet(channels=(32, 64, 128, 256), precision="f32").to(dev).train()
    m._prepare()  # registers every conv weight with the model's WeightPacker and makes it current
    pk = mc.get_packer()
    params = list(m.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    res = {k: {"device_us": [], "host_us": []} for k in CONFIGS}
    last = {}
    for _ in range(args.repeats):
        for kind in CONFIGS:
            d, h, last[kind] = measure(kind, params, pk, args.steps, args.warmup)
            res[kind]["device_us"].append(round(d, 1))
            res[kind]["host_us"].append(round(h, 1))
    for kind in CONFIGS:
        r = res[kind]
        out = {"config": kind, "tensors": len(params), "parameters": sum(p.numel() for p in params),
               "steps": args.steps, "warmup": args.warmup, **r,
               "device_us_median": sorted(r["device_us"])[len(r["device_us"]) // 2],
               "device_us_spread": round(max(r["device_us"]) - min(r["device_us"]), 1),
               "host_us_median": sorted(r["host_us"])[len(r["host_us"]) // 2]}
        print(json.dumps(out), flush=True)
    for kind in CONFIGS if args.launches else ():
        optim._ADAMW_PACK = 1 if kind == "fused" else 0
        n, names = launches(last[kind], pk)
        print(json.dumps({"config": kind, "launches_per_step": n, "kernels": names}), flush=True)


if __name__ == "__main__":
    main()
