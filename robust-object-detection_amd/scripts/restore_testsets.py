"""Write U-Net-restored copies of the corrupted COCO test sets — `python -m scripts.restore_testsets`.

Reference restore_testsets.py:82-159: Noise / Blur / LowRes images restored, annotations copied, Clean
copied unchanged; JPEG output. Here the restoration runs on the GPU (mx_det.unet.restore_u8), and so
do the JPEG decode (mx_det.jpeg.read_file; PIL for the files it does not handle) and the quality-95
encode (mx_det.jpeg.write_file), both bit-identical to libjpeg-turbo: pixels never visit the host.
MX_JPEG_ENCODE=host encodes with PIL instead; MX_JPEG_DECODE=device decodes the scan on the device
too (the default decodes it on the host). The fused eval path (eval_restored.py) skips this step.
MX_EXTRA_VARIANTS=jpeg restores Test_JPEG as well (night, haze, rain: Test_Night, Test_Haze, Test_Rain),
MX_SEVERITIES the Test_<Kind>_s<L> sets.
MX_RESTORE_GATE (unset or 0: off, auto, or a rules JSON; mx_det.gate): the blind gate decides per image. An
image it passes is copied as a file (shutil.copy2: no JPEG round trip), one it flags is restored and encoded
as above; Test_Clean goes through the gate like the others. Output goes to data/testsets/coco6_gated, the
per-variant restored / passed counts are printed.
MX_RESTORE_DENOISE (nlm or nlm:<k16>; needs the gate, otherwise ValueError before any model loads): an image
the gate's noise rule recognises goes through the blind non-local-means denoiser (mx_det.denoise) and is
encoded and written; passed files are copied as before. Output goes to data/testsets/coco6_gated_nlm.
"""
import os
import shutil
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from scripts import eval_restored
from mx_det import denoise, gate, jpeg
from mx_det.augment import env_extra_variants, severity_variants
from mx_det.engine import init_device

COCO_TESTSET_ROOT = Path("data/testsets/coco6")
COCO_OUT_ROOT = Path("data/testsets/coco6_restored")
COCO_GATED_ROOT = Path("data/testsets/coco6_gated")
COCO_GATED_NLM_ROOT = Path("data/testsets/coco6_gated_nlm")
VARIANTS_TO_RESTORE = ["Test_Noise", "Test_Blur", "Test_LowRes"]


def variants_to_restore():
    """The reference's three corrupted variants, then those MX_EXTRA_VARIANTS names, then the
    MX_SEVERITIES sets."""
    return VARIANTS_TO_RESTORE + [v for v, _ in env_extra_variants()] + [v[0] for v in severity_variants()]


def read_rgb(path, dev):
    """Image.open(path).convert("RGB") as a uint8 [H, W, 3] tensor on `dev`."""
    try:
        return jpeg.read_file(path, dev)
    except (jpeg.JpegUnsupported, ValueError):
        with Image.open(path) as im:
            return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy()).to(dev)


def write_rgb(path, img):
    """Image.fromarray(img).save(path, quality=95) of a uint8 [H, W, 3] device tensor."""
    if os.environ.get("MX_JPEG_ENCODE", "device") == "host":
        Image.fromarray(img.cpu().numpy()).save(path, quality=95)
    else:
        jpeg.write_file(path, img, quality=95)


def restore_variant(unet, variant, dev, src_root=None, dst_root=None):
    """unet: a RestorationUNet, or a gate.GatedRestorer (mode skip) that decides per image."""
    gated = isinstance(unet, gate.GatedRestorer)
    src_root = COCO_TESTSET_ROOT if src_root is None else src_root
    dst_root = COCO_OUT_ROOT if dst_root is None else dst_root
    src_img, dst_img = src_root / variant / "images" / "val", dst_root / variant / "images" / "val"
    src_ann, dst_ann = src_root / variant / "annotations", dst_root / variant / "annotations"
    dst_img.mkdir(parents=True, exist_ok=True)
    dst_ann.mkdir(parents=True, exist_ok=True)
    for f in src_ann.glob("*.json"):
        shutil.copy2(f, dst_ann / f.name)
    files = sorted(src_img.glob("*.jpg"))
    for i, p in enumerate(files):
        img = read_rgb(p, dev)[None]
        verdict, noisy = 1, 0
        if gated and unet.denoiser is not None:
            stats, (verdict,), (noisy,) = unet.decide_both_u8(img)
            unet.count([verdict], [noisy])
        elif gated:  # skip mode, with the file itself as the passed image's copy
            verdict = unet.decide_u8(img)[0]
            unet.count([verdict])
        if verdict:
            write_rgb(dst_img / p.name, (unet.unet if gated else unet).restore_u8(img)[0])
        elif noisy:
            write_rgb(dst_img / p.name, unet.denoiser.denoise_u8(img, stats=stats)[0][0])
        else:
            shutil.copy2(p, dst_img / p.name)
        if (i + 1) % 100 == 0 or i + 1 == len(files):
            print(f"    COCO {variant}: {i + 1}/{len(files)}", flush=True)


def main():
    dev, _, _ = init_device()
    rules = gate.env_gate()  # a bad rules file raises here
    denoiser = denoise.env_denoise()  # and a bad MX_RESTORE_DENOISE here
    if denoiser is not None and rules is None:
        raise ValueError("MX_RESTORE_DENOISE needs the gate (MX_RESTORE_GATE)")
    unet = eval_restored.load_unet(dev)
    if rules is not None:
        gated = gate.GatedRestorer(unet, rules[0], rules[1], mode="skip", denoiser=denoiser)
        dst_root = COCO_GATED_ROOT if denoiser is None else COCO_GATED_NLM_ROOT
        for v in ["Test_Clean"] + variants_to_restore():
            restore_variant(gated, v, dev, dst_root=dst_root)
            print(f"    gate {v}: {gated.take_counts()}", flush=True)
        return
    for v in variants_to_restore():
        restore_variant(unet, v, dev)
    clean_src, clean_dst = COCO_TESTSET_ROOT / "Test_Clean", COCO_OUT_ROOT / "Test_Clean"
    if clean_src.exists() and not clean_dst.exists():
        shutil.copytree(clean_src, clean_dst)


if __name__ == "__main__":
    main()
