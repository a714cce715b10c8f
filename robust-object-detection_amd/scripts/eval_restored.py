"""Evaluate the baseline Faster R-CNN on U-Net-restored test sets — `python -m scripts.eval_restored`.

Reference: eval_restored.py (FRCNN branch :60-113, :164-184) reads JPEGs written by restore_testsets.py.
Default (MX_RESTORE_ON_DEVICE=0): the reference's pipeline -- pre-restored JPEGs from
data/testsets/coco6_restored (written by `python -m scripts.restore_testsets`, which runs the U-Net
on the device in the reference's fp32 precision and re-encodes JPEG like restore_testsets.py:101),
results in experiments/eval_restored_results.json (reference schema).
MX_RESTORE_ON_DEVICE=1: the fused MI355X pipeline of the north star -- each corrupted test image is
restored by the HIP U-Net on the GPU (reflect pad, /255, U-Net, *255, clip, truncate, crop) and fed
straight to detection, no host round trip and no JPEG re-encode. That skips the reference's JPEG
round trip, so its mAP is not the reference's number: it goes to
experiments/eval_restored_results_fused.json instead.
MX_RESTORE_GATE (with MX_RESTORE_ON_DEVICE=1; unset or 0: off, auto: mx_det.gate.DEFAULT_RULES, else the path
of a rules JSON such as scripts.fit_restore_gate writes): the blind gate in front of the U-Net. Every image
of every variant, Test_Clean included, gets its degradation statistics on the device and is restored or
passed through by their verdict (mx_det.gate.GatedRestorer, mode select: no host synchronisation). Results
go to experiments/eval_restored_results_gated.json (reference schema), the per-variant restored / passed
counts to experiments/restore_gate_counts.json.
MX_RESTORE_DENOISE (nlm or nlm:<k16>; unset or 0: off; needs the gate and MX_RESTORE_ON_DEVICE=1, otherwise
ValueError before any model loads): the images the gate's noise rule recognises, which the U-Net leaves alone,
go through the blind non-local-means denoiser (mx_det.denoise; one more device launch per batch, still no host
synchronisation). Results go to experiments/eval_restored_results_gated_nlm.json (reference schema), and the
counts file gains the denoised counts. The denoiser's effect on mAP is unmeasured.
MX_EXTRA_VARIANTS=jpeg evaluates the restored Test_JPEG set too, MX_SEVERITIES the restored
Test_<Kind>_s<L> sets (eval_all.all_variants()).
MX_BN_ADAPT=<mode>[:<prior>] adds a <name>_BNAdapt entry per checkpoint: the same run with test-time BatchNorm
adaptation of the detector (mx_det.adapt; the U-Net's BatchNorm stays folded), as in eval_all.
"""
import os
from pathlib import Path

import torch

from mx_det import adapt as bn_adapt
from mx_det import denoise, gate
from mx_det.unet import RestorationUNet
from scripts import eval_all

VARIANTS = eval_all.VARIANTS
CORRUPTED_ROOT = Path("data/testsets/coco6")
RESTORED_ROOT = Path("data/testsets/coco6_restored")
UNET_CKPT = Path("experiments/restoration/best.pth")
CKPTS = {"FasterRCNN": Path("experiments/frcnn/baseline_clean/best.pth")}
OUT_DIR = Path("experiments")


def load_unet(dev, ckpt=None):
    ckpt = UNET_CKPT if ckpt is None else ckpt
    unet = RestorationUNet(channels=(32, 64, 128, 256))
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    unet.load_state_dict(sd.get("model", sd))
    return unet.to(dev).eval()


def results_name(on_device, gated=False, denoised=False):
    if on_device and gated:
        return "eval_restored_results_gated_nlm.json" if denoised else "eval_restored_results_gated.json"
    return "eval_restored_results_fused.json" if on_device else "eval_restored_results.json"


def main():
    dev, world, rank = eval_all.init_device()
    on_device = os.environ.get("MX_RESTORE_ON_DEVICE", "0") != "0"
    adapt = bn_adapt.parse_env(os.environ.get("MX_BN_ADAPT", ""))
    rules = gate.env_gate() if on_device else None  # a bad rules file raises here, before any model loads
    denoiser = denoise.env_denoise()  # and so does a bad MX_RESTORE_DENOISE
    if denoiser is not None and rules is None:
        raise ValueError("MX_RESTORE_DENOISE needs the gate (MX_RESTORE_GATE) and MX_RESTORE_ON_DEVICE=1")
    restorer = load_unet(dev) if on_device else None
    root = CORRUPTED_ROOT if on_device else RESTORED_ROOT
    results, counts = {}, {}
    kw = {}
    if rules is not None:
        restorer = gate.GatedRestorer(restorer, rules[0], rules[1], mode="select", denoiser=denoiser)
        kw = dict(restore_clean=True)
    for name, ck in CKPTS.items():
        if rules is not None:
            kw["counts"] = counts.setdefault(name, {})
        r = eval_all.eval_model(name, ck, dev, root=root, restorer=restorer, **kw)
        if rank == 0:
            results[name] = r
        if adapt is not None:
            aname = name + eval_all.ADAPT_SUFFIX
            if rules is not None:
                kw["counts"] = counts.setdefault(aname, {})
            r = eval_all.eval_model(aname, ck, dev, root=root, restorer=restorer, adapt=adapt, **kw)
            if rank == 0:
                results[aname] = r
    if rank == 0:
        OUT_DIR.mkdir(parents=True, exist_ok=True)
        eval_all.save_json(results, OUT_DIR / results_name(on_device, rules is not None, denoiser is not None))
        if rules is not None:
            eval_all.save_json(counts, OUT_DIR / "restore_gate_counts.json")
    return results


if __name__ == "__main__":
    main()
