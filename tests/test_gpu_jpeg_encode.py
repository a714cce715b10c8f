"""JPEG encoder on the device (mx_det.jpeg.forward / encode / write_file; include/mx_det.h
mx_jpeg_forward, mx_jpeg_entropy) against libjpeg-turbo itself (PIL's encoder): equality, no tolerance.
  * coefficient stage: mx_jpeg_forward == decode_coefs(PIL's file of the same pixels), dummy blocks
    included, RGB and BGR input;
  * full encode: encode(img, q, s) == PIL's bytes with the device and with the host entropy coder;
  * scripts.build_corrupted_testsets writes the same trees with MX_JPEG_ENCODE=host (PIL) and without;
  * scripts.restore_testsets' read / write helpers == PIL's encode of PIL's decode.
Images: tests/test_jpeg_encode.py band_image (noise band, flat band, checkerboard patch); the
reference scan of every image large enough to hold the three must contain FF 00."""
import functools
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

from test_jpeg_encode import band_image, full_size, pil_bytes

pytestmark = pytest.mark.gpu

CASES = [  # (H, W, quality, PIL subsampling)
    (1, 1, 95, 2),      # smallest image
    (9, 5, 95, 2),      # luma dummy row
    (16, 3, 95, 2),
    (8, 9, 95, 2),      # chroma rows replicated after downsampling
    (24, 40, 95, 2),
    (50, 66, 50, 2),
    (121, 163, 95, 2),  # odd block counts, right dummy column, three 64-pixel strips
    (64, 80, 90, 0),
    (75, 93, 100, 2),
    (200, 311, 95, 2),  # more than 256 blocks: several workgroups in the entropy passes
]
IDS = ["%dx%d-q%d-s%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def reference(i):
    """(pixels, PIL's file) of case i; computed once, shared, read-only."""
    H, W, q, sub = CASES[i]
    img = band_image(H, W, 100 + i)
    img.setflags(write=False)
    return img, pil_bytes(img, q, sub)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward_coefficients_match_libjpeg(dev, i):
    from mx_det import jpeg
    H, W, q, sub = CASES[i]
    img, data = reference(i)
    ref_info, ref = jpeg.decode_coefs(data)
    info = jpeg.encode_info(W, H, q, sub)
    assert info.coef_total == ref_info.coef_total
    got = jpeg.forward(torch.from_numpy(img.copy()).to(dev), info).cpu().numpy()
    assert got.dtype == np.int16
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])
    if i == 6:  # BGR input, same coefficients
        bgr = torch.from_numpy(np.ascontiguousarray(img[..., ::-1])).to(dev)
        assert np.array_equal(jpeg.forward(bgr, info, bgr=True).cpu().numpy(), ref)


@pytest.mark.parametrize("entropy", ["device", "host"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_encode_is_byte_identical_to_libjpeg(dev, i, entropy):
    from mx_det import jpeg
    H, W, q, sub = CASES[i]
    img, data = reference(i)
    if full_size(H, W):
        assert b"\xff\x00" in data[jpeg.parse(data).scan_off:-2]
    got = jpeg.encode(torch.from_numpy(img.copy()).to(dev), q, sub, entropy=entropy)
    assert isinstance(got, bytes)
    assert len(got) == len(data) and got == data, (len(got), len(data))
    bgr = torch.from_numpy(np.ascontiguousarray(img[..., ::-1])).to(dev)
    assert jpeg.encode(bgr, q, sub, bgr=True, entropy=entropy) == data


@pytest.mark.parametrize("grey", [False, True], ids=["422", "grey"])
def test_entropy_coder_on_a_parsed_file(dev, grey):
    """mx_jpeg_entropy with the tables and geometry of a parsed file (4:2:2, 4 blocks per MCU; grey, one
    component) == the file's scan."""
    import ctypes
    from mx_det import _lib, jpeg
    if grey:
        b = io.BytesIO()
        Image.fromarray(band_image(97, 131, 7)).convert("L").save(b, format="JPEG", quality=75)
        data = b.getvalue()
    else:
        data = pil_bytes(band_image(97, 131, 7), 75, 1)
    info, coefs = jpeg.decode_coefs(data)
    lib = _lib.load()
    ws = torch.empty(lib.mx_jpeg_entropy_workspace(ctypes.byref(info)), dtype=torch.uint8, device=dev)
    cap = int(lib.mx_jpeg_scan_bound(ctypes.byref(info)))
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    cd = torch.from_numpy(coefs).to(dev)
    _lib.call("mx_jpeg_entropy", cd.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), out.data_ptr(), cap,
              n.data_ptr(), _lib.stream())
    scan = data[info.scan_off:-2]
    assert int(n.item()) == len(scan)
    assert out[:len(scan)].cpu().numpy().tobytes() == scan
    # a short out_cap: the length is still reported, nothing is written at or past the capacity
    small = len(scan) // 2
    out.fill_(0xA5)
    _lib.call("mx_jpeg_entropy", cd.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), out.data_ptr(), small,
              n.data_ptr(), _lib.stream())
    host = out.cpu().numpy()
    assert int(n.item()) == len(scan) and host[:small].tobytes() == scan[:small] and (host[small:] == 0xA5).all()
    # a coefficient without a code: -1
    cd[5] = -32768
    _lib.call("mx_jpeg_entropy", cd.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), out.data_ptr(), cap,
              n.data_ptr(), _lib.stream())
    assert int(n.item()) == -1


def test_encode_refuses_what_it_does_not_handle(dev):
    from mx_det import jpeg
    img = torch.zeros((16, 16, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        jpeg.encode(img[..., 0])                      # grey
    with pytest.raises(ValueError):
        jpeg.encode(img, subsampling=1)               # 4:2:2 pixel input
    with pytest.raises(ValueError):
        jpeg.encode(img.float())                      # not uint8
    with pytest.raises(ValueError):
        jpeg.encode(img, quality=0)
    with pytest.raises(ValueError):
        jpeg.encode(img, entropy="nowhere")


def _src(root, n=2):
    from mx_det.data import synth_image
    for kind in ("yolo6", "coco6"):
        d = root / kind / "images" / "val"
        d.mkdir(parents=True)
        for i in range(n):
            Image.fromarray(synth_image(i, 90 + 2 * i, 120 + 3 * i)).save(d / f"{i:03d}.jpg", quality=95)
    lbl = root / "yolo6" / "labels" / "val"
    lbl.mkdir(parents=True)
    for i in range(n):
        (lbl / f"{i:03d}.txt").write_text("0 0.5 0.5 0.1 0.1\n")
    (root / "coco6" / "annotations").mkdir(parents=True)
    json.dump({"images": [], "annotations": [], "categories": []},
              open(root / "coco6/annotations/instances_val.json", "w"))


def test_builder_writes_the_same_trees_with_either_encoder(dev, tmp_path, monkeypatch):
    from mx_det import jpeg
    from scripts import build_corrupted_testsets as b
    _src(tmp_path / "src")
    calls = []
    orig = jpeg.encode
    monkeypatch.setattr(jpeg, "encode", lambda *a, **k: calls.append(1) or orig(*a, **k))
    monkeypatch.setenv("MX_JPEG_ENCODE", "host")
    b.main(tmp_path / "src/yolo6", tmp_path / "src/coco6", tmp_path / "host")
    assert not calls
    monkeypatch.setenv("MX_JPEG_ENCODE", "device")
    b.main(tmp_path / "src/yolo6", tmp_path / "src/coco6", tmp_path / "device")
    assert len(calls) == 2 * 4 * 2  # every image of every variant of both layouts went through the device encoder
    monkeypatch.delenv("MX_JPEG_ENCODE")
    b.main(tmp_path / "src/yolo6", tmp_path / "src/coco6", tmp_path / "default")
    for other in ("device", "default"):
        files = sorted(p.relative_to(tmp_path / "host") for p in (tmp_path / "host").rglob("*") if p.is_file())
        assert files == sorted(p.relative_to(tmp_path / other) for p in (tmp_path / other).rglob("*") if p.is_file())
        assert sum(f.suffix == ".jpg" for f in files) == 16
        for f in files:
            if f.name != "data.yaml":  # data.yaml names its own root
                assert (tmp_path / "host" / f).read_bytes() == (tmp_path / other / f).read_bytes(), (other, f)


def test_restore_writer_matches_pil(dev, tmp_path, monkeypatch):
    from scripts import restore_testsets as r
    monkeypatch.delenv("MX_JPEG_ENCODE", raising=False)
    src = tmp_path / "in.jpg"
    src.write_bytes(pil_bytes(band_image(75, 93, 9), 95, 2))
    img = r.read_rgb(src, dev)
    assert img.is_cuda and img.dtype == torch.uint8
    pil = np.asarray(Image.open(src).convert("RGB"))
    assert np.array_equal(img.cpu().numpy(), pil)
    r.write_rgb(tmp_path / "out.jpg", img)
    buf = io.BytesIO()
    Image.fromarray(pil).save(buf, format="JPEG", quality=95)
    assert (tmp_path / "out.jpg").read_bytes() == buf.getvalue()
    png = tmp_path / "in.png"  # not a JPEG: PIL reads it
    Image.fromarray(pil).save(png)
    assert np.array_equal(r.read_rgb(png, dev).cpu().numpy(), pil)
