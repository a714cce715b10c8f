"""What the device overlay renderer and panel composer (mx_det.draw, csrc/mx_draw.hip) cost, in one session
on one GPU, at the demo's working size: 1080 x 1920 frames with D = 100 random VisDrone-sized boxes.

  overlay   one mx_draw_batch_u8 launch for one frame with a 40-row title bar (Overlay.batch's launch
            alone: descriptors prepared once). Bytes = source read + output written.
  compose   one mx_panels_compose_u8 launch, three such panels into 480 x ... . Bytes = sources + canvas.
  host      the path a user has without these kernels: boxes, labels, scores and the frame to the host,
            tests/draw_ref.py's numpy painter, the pixels back to the device (wall clock, few repeats).

Device routes are timed with device events around one launch, `--reps` launches per round after a
warm-up: warm (back to back, the frame may sit in the 256 MiB last-level cache) and cold (a 512 MiB
buffer is rewritten before every launch, outside the timed window). The table shows the median of all
launches and min..max, µs, and the fraction of the HBM peak (8.0 TB/s spec) the bytes over the median make.

    python tools/bench_draw.py [--rounds 5] [--reps 20] [--host-reps 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mx_det import _lib, draw  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, spec
H, W, D, BAR, TARGET_H = 1080, 1920, 100, 40, 480


def boxes_like_visdrone(rng, n):
    """Small objects of an aerial frame: 12..120 pixels wide, 12..90 high, anywhere in the frame."""
    w, h = rng.uniform(12, 120, n), rng.uniform(12, 90, n)
    x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
    return np.stack([x, y, x + w, y + h], 1).astype(np.float32)


def timed(fn, reps, flush=None):
    out = []
    for _ in range(reps):
        if flush is not None:
            flush.add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)  # µs
    return out


def summary(us, nbytes):
    med = statistics.median(us)
    return {"median_us": med, "min_us": min(us), "max_us": max(us), "bytes": nbytes,
            "hbm_fraction": nbytes / (med * 1e-6) / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_draw: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    boxes = torch.from_numpy(boxes_like_visdrone(rng, D)).to(dev)
    labels = torch.from_numpy(rng.integers(1, 7, D)).to(dev)
    scores = torch.from_numpy(np.sort(rng.uniform(0.36, 1.0, D).astype(np.float32))[::-1].copy()).to(dev)
    count = torch.tensor([D], dtype=torch.int32).to(dev)
    ov = draw.Overlay()
    title = "Blur + FRCNN (Augmented)"
    panels, drawn = ov.batch([frame], [boxes], [labels], [scores], count, [title])
    assert int(drawn[0]) == D
    panel = panels[0]

    # the overlay launch alone: Overlay.batch's descriptor, prepared once
    desc = (_lib.DrawDesc * 1)()
    d = desc[0]
    d.src, d.dst, d.boxes, d.labels, d.scores, d.count = (frame.data_ptr(), panel.data_ptr(), boxes.data_ptr(),
                                                           labels.data_ptr(), scores.data_ptr(), count.data_ptr())
    d.H, d.W, d.D, d.bar, d.title_len, d.title = H, W, D, BAR, len(title), title.encode()
    stream = _lib.stream()

    def overlay():
        _lib.call("mx_draw_batch_u8", desc, 1, ov._names_c, len(ov.names), ov._colors_c, len(ov.colors), ov.conf_thr,
                  ov.label_scale, ov.title_scale, drawn.data_ptr(), stream)

    three = [panel, panel.clone(), panel.clone()]
    dws = draw.panel_widths([tuple(p.shape[:2]) for p in three], TARGET_H)
    canvas = draw.compose(three, TARGET_H)
    pdesc = (_lib.PanelDesc * 3)()
    for q, p, dw in zip(pdesc, three, dws):
        q.src, q.h, q.w, q.dw = p.data_ptr(), p.shape[0], p.shape[1], dw

    def compose():
        _lib.call("mx_panels_compose_u8", pdesc, 3, TARGET_H, canvas.data_ptr(), stream)

    routes = {"overlay": (overlay, frame.numel() + panel.numel()),
              "compose": (compose, sum(p.numel() for p in three) + canvas.numel())}
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    res = {"shape": [H, W], "D": D, "bar": BAR, "target_h": TARGET_H, "canvas": list(canvas.shape), "rounds": args.rounds,
           "reps": args.reps}
    for name, (fn, nbytes) in routes.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        warm, cold = [], []
        for _ in range(args.rounds):  # the two modes alternate
            warm += timed(fn, args.reps)
            cold += timed(fn, args.reps, flush)
        res[name] = {"warm": summary(warm, nbytes), "cold": summary(cold, nbytes)}

    # the host path: detections and frame down, numpy painter, pixels up
    import draw_ref
    glyphs = draw_ref.font()
    names = [draw.CLASS_NAMES[k] for k in range(1, 7)]
    colors = [draw.CLASS_COLORS[k] for k in range(1, 7)]
    host = []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b, lab, sc, src = boxes.cpu().numpy(), labels.cpu().numpy(), scores.cpu().numpy(), frame.cpu().numpy()
        out, n = draw_ref.paint(src, b, lab, sc, D, names, colors, ov.conf_thr, title=title, bar=BAR, glyphs=glyphs)
        up = torch.from_numpy(out).to(dev)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    assert torch.equal(up, panel) and n == D  # the two paths draw the same pixels
    res["host"] = {"median_us": statistics.median(host), "min_us": min(host), "max_us": max(host)}

    print(json.dumps(res), flush=True)
    print("\n| route | µs per launch: median (min..max) | bytes | fraction of 8.0 TB/s |")
    print("|---|---|---|---|")
    for name in routes:
        for mode in ("warm", "cold"):
            v = res[name][mode]
            print(f"| {name}, {mode} | {v['median_us']:.1f} ({v['min_us']:.1f}..{v['max_us']:.1f}) | {v['bytes']} | "
                  f"{v['hbm_fraction']:.3f} |")
    v = res["host"]
    print(f"| host path (copy down, numpy painter, copy up) | {v['median_us']:.0f} ({v['min_us']:.0f}..{v['max_us']:.0f}) | | |")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
