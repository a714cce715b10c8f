"""JPEG entropy decoding on the device (mx_det.jpeg.decode_coefs_device / decode(entropy="device");
include/mx_det.h mx_jpeg_entropy_decode) against the sequential host decoder and libjpeg-turbo (PIL):
equality, no tolerance, on the corpus of tests/jpeg_corpus.py at the minimum and the default
subsequence size; damaged files come out as the host path gives them; the loaders and the offline
scripts' reader give the same tensors under MX_JPEG_DECODE=device as without it."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_corpus as jc
from test_jpeg_decode_chunked import corrupted, truncated

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[jc.SUBSEQ_MIN, jc.SUBSEQ_DEFAULT], ids=["s64", "s512"])
def subseq(request):
    from mx_det import jpeg
    jpeg.set_subseq(request.param)
    yield request.param
    jpeg.set_subseq(jc.SUBSEQ_DEFAULT)


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_corpus_is_hard_enough():
    jc.check_corpus()


@pytest.mark.parametrize("i", range(len(jc.SPECS)), ids=jc.IDS)
def test_device_equals_sequential(dev, i, subseq):
    from mx_det import jpeg
    _, ref = jc.reference(i)
    info, coefs, status = jpeg.decode_coefs_device(jc.jpeg_file(i), dev)
    assert coefs.dtype == torch.int16 and coefs.device.type == "cuda" and status.dtype == torch.int32
    assert int(status.item()) == 0
    got = coefs.cpu().numpy()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])


@pytest.mark.parametrize("offset", [1, 7, 13])
@pytest.mark.parametrize("name", ["noise-1x1-q75-420", "noise-64x64-q100-grey-r7", "noise-256x256-q100-444"])
def test_scan_at_an_odd_device_offset(dev, name, offset, subseq):
    from mx_det import jpeg
    i = jc.IDS.index(name)
    info, ref = jc.reference(i)
    host = torch.from_numpy(np.frombuffer(jc.jpeg_file(i), dtype=np.uint8).copy())
    coefs, status = jpeg.entropy_stage(info, host, dev, offset=offset)
    assert int(status.item()) == 0
    assert np.array_equal(coefs.cpu().numpy(), ref)


@pytest.mark.parametrize("i", range(len(jc.SPECS)), ids=jc.IDS)
def test_decode_equals_pil(dev, i):
    from mx_det import jpeg
    data = jc.jpeg_file(i)
    ref = pil_rgb(data)
    assert np.array_equal(jpeg.decode(data, dev, entropy="device").cpu().numpy(), ref)
    assert np.array_equal(jpeg.decode(data, dev, bgr=True, entropy="device").cpu().numpy(), ref[..., ::-1])


def test_decode_refuses_an_unknown_entropy_mode(dev):
    from mx_det import jpeg
    with pytest.raises(ValueError):
        jpeg.decode(jc.jpeg_file(0), dev, entropy="gpu")


@pytest.mark.parametrize("name", ["noise-64x64-q100-444", "noise-250x131-q95-422-r7", "flat-64x64-q75-420"])
def test_truncated_file_decodes_as_on_the_host(dev, name, subseq):
    from mx_det import jpeg
    data = truncated(jc.jpeg_file(jc.IDS.index(name)))
    _, _, status = jpeg.decode_coefs_device(data, dev)
    assert int(status.item()) != 0
    assert torch.equal(jpeg.decode(data, dev, entropy="device"), jpeg.decode(data, dev, entropy="host"))


@pytest.mark.parametrize("name", ["noise-64x64-q100-444", "noise-64x64-q95-420-opt", "noise-64x64-q100-grey-r7"])
def test_corrupted_code_raises_as_on_the_host(dev, name, subseq):
    from mx_det import jpeg
    data = corrupted(jc.jpeg_file(jc.IDS.index(name)))
    _, _, status = jpeg.decode_coefs_device(data, dev)
    assert int(status.item()) & 1
    with pytest.raises(ValueError):
        jpeg.decode(data, dev, entropy="host")
    with pytest.raises(ValueError):
        jpeg.decode(data, dev, entropy="device")


def small_files():
    """Four 64x48 files, the third truncated."""
    files = [jc.pil_jpeg(jc.CONTENT[c](48, 64, 40 + k), q, s, opt, rst)
             for k, (c, q, s, opt, rst) in enumerate([("noise", 95, "420", False, 0), ("synth", 75, "444", True, 0),
                                                      ("noise", 100, "422", False, 3), ("flat", 95, "grey", False, 0)])]
    files[2] = truncated(files[2])
    return files


def batches(files):
    def target(k):
        return {"boxes": torch.tensor([[1.0, 2.0, 30.0 + k, 40.0]]), "labels": torch.tensor([k + 1]),
                "image_id": torch.tensor([k])}
    arrays = [np.frombuffer(f, dtype=np.uint8) for f in files]
    return [(arrays[:2], [target(0), target(1)]), (arrays[2:], [target(2), target(3)])]


@pytest.mark.parametrize("which", ["DeviceJpegLoader", "PrefetchJpegLoader"])
def test_loaders_under_the_switch(dev, which, monkeypatch):
    from mx_det import engine, jpeg
    files = small_files()
    host = [jpeg.decode(f, dev, entropy="host").cpu() for f in files]

    def run():
        loader = getattr(engine, which)(batches(files), dev)
        out = []
        for images, targets in loader:
            torch.cuda.synchronize()
            out += [(im.cpu(), {k: torch.as_tensor(v).cpu() for k, v in t.items()}) for im, t in zip(images, targets)]
        return out

    monkeypatch.delenv("MX_JPEG_DECODE", raising=False)
    plain = run()
    monkeypatch.setenv("MX_JPEG_DECODE", "device")
    switched = run()
    assert len(plain) == len(switched) == 4
    for k, ((a, ta), (b, tb)) in enumerate(zip(plain, switched)):
        assert torch.equal(a, host[k]) and torch.equal(b, host[k]), k
        assert sorted(ta) == sorted(tb) and all(torch.equal(ta[key], tb[key]) for key in ta)
    monkeypatch.setenv("MX_JPEG_DECODE", "somewhere")
    with pytest.raises(ValueError):
        jpeg.env_entropy()


def test_restore_testsets_reader_under_the_switch(dev, tmp_path, monkeypatch):
    from scripts import restore_testsets as r
    files = small_files()
    for k, f in enumerate(files):
        (tmp_path / f"{k}.jpg").write_bytes(f)
    monkeypatch.delenv("MX_JPEG_DECODE", raising=False)
    plain = [r.read_rgb(tmp_path / f"{k}.jpg", dev).cpu() for k in range(4)]
    monkeypatch.setenv("MX_JPEG_DECODE", "device")
    switched = [r.read_rgb(tmp_path / f"{k}.jpg", dev).cpu() for k in range(4)]
    for k in (0, 1, 3):
        assert np.array_equal(plain[k].numpy(), pil_rgb(files[k]))
    assert all(torch.equal(a, b) for a, b in zip(plain, switched))
