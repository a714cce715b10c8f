"""restoration.DevicePatchLoader: the device patch loader of U-Net training yields, bit for bit, the
patches the host path (RestorationDataset: PIL decode, resize up, crop, flip) crops for the same
draws -- with the entropy decode on the host and on the device, through the per-file host fallback
and no further than it, across the loader stream's hand-off when that stream is late, and from
scripts.train_restoration with MX_PATCH_LOADER=device."""
import json
import random
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_corpus as jc
from _stream_delay import delayed, delayed_call

pytestmark = pytest.mark.gpu

PATCH = 64
# (width, height, coding): 6 and 7 are smaller than the patch on a side (the reference resizes them
# up), 8 is progressive (the parser refuses it): those three take the host path, the rest the device's
FILES = [(300, 280, "420"), (64, 64, "420"), (257, 65, "422"), (131, 250, "grey"), (90, 70, "444"), (50, 90, "420"),
         (120, 40, "420"), (200, 200, "progressive"), (300, 280, "restart")]
ON_DEVICE = 6


@pytest.fixture(scope="module")
def img_dir(tmp_path_factory):
    from mx_det.data import synth_image
    d = tmp_path_factory.mktemp("patches")
    for k, (w, h, coding) in enumerate(FILES):
        img = synth_image(100 + k, h, w)
        path = d / f"{k + 1:02d}.jpg"
        if coding == "progressive":
            Image.fromarray(img).save(path, quality=90, progressive=True)
        elif coding == "restart":
            path.write_bytes(jc.pil_jpeg(img, 95, "420", restart=5))
        else:
            path.write_bytes(jc.pil_jpeg(img, 95, coding))
    return d


def _host_patches(img_dir, is_train, seed=None):
    """The host path's patches [N, S, S, 3], in file order (the module-level random stream seeded)."""
    from mx_det.restoration import RestorationDataset
    ds = RestorationDataset(img_dir, PATCH, is_train=is_train)
    if seed is not None:
        random.seed(seed)
    return torch.stack([ds[i] for i in range(len(ds))])


def _count_windows(monkeypatch):
    from mx_det import jpeg
    real, calls = jpeg.reconstruct_window, []

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(jpeg, "reconstruct_window", counted)
    return calls


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_train_patches_equal_host_crops(dev, img_dir, monkeypatch, entropy):
    from mx_det.restoration import DevicePatchLoader
    monkeypatch.setenv("MX_JPEG_DECODE", entropy)
    ref = _host_patches(img_dir, True, seed=7)
    calls = _count_windows(monkeypatch)
    loader = DevicePatchLoader(img_dir, PATCH, 4, True, dev, shuffle=False, drop_last=False, workers=3,
                               rng=random.Random(7))
    got = list(loader)
    assert [tuple(b.shape) for b in got] == [(4, PATCH, PATCH, 3), (4, PATCH, PATCH, 3), (1, PATCH, PATCH, 3)]
    assert all(b.dtype == torch.uint8 and b.device.type == "cuda" for b in got)
    got = torch.cat(got).cpu()
    same = [bool(torch.equal(got[i], ref[i])) for i in range(len(FILES))]
    assert all(same), same
    # the two small frames and the progressive one took the host path, and nothing else did
    assert loader.host_fallbacks == len(FILES) - ON_DEVICE == 3
    assert len(calls) == ON_DEVICE
    assert loader.wait_s >= 0.0


def test_validation_centre_crops_and_length(dev, img_dir):
    from mx_det.restoration import DevicePatchLoader, RestorationDataset, collate_u8
    ref = _host_patches(img_dir, False)
    for drop_last in (False, True):
        host = torch.utils.data.DataLoader(RestorationDataset(img_dir, PATCH, is_train=False), batch_size=4,
                                           shuffle=False, drop_last=drop_last, collate_fn=collate_u8)
        loader = DevicePatchLoader(img_dir, PATCH, 4, False, dev, shuffle=False, drop_last=drop_last)
        got = list(loader)
        assert len(loader) == len(host) == len(got) == (2 if drop_last else 3)
        assert [b.shape[0] for b in got] == ([4, 4] if drop_last else [4, 4, 1])
        got = torch.cat(got).cpu()
        assert torch.equal(got, ref[:got.shape[0]])
        # a second pass over the same loader gives the same batches
        assert torch.equal(torch.cat(list(loader)).cpu(), got)


def test_shuffle_follows_the_torch_seed(dev, img_dir):
    """shuffle=True draws its order, and rng=None its crops, in the consuming thread from the seeded
    global generators: the same seeds give the same epoch, and the order is a permutation."""
    from mx_det.restoration import DevicePatchLoader
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        random.seed(5)
        loader = DevicePatchLoader(img_dir, PATCH, 4, True, dev, shuffle=True, drop_last=True)
        runs.append(torch.cat(list(loader)).cpu())
        assert runs[-1].shape[0] == 8
    assert torch.equal(runs[0], runs[1])


def test_hand_off_with_a_late_loader_stream(dev, img_dir, monkeypatch):
    """Every image's device stage starts behind a spin on the loader stream: only the consumer's wait
    on the batch's event keeps it from reading the batch tensor before it is written."""
    from mx_det import restoration
    monkeypatch.delenv("MX_JPEG_DECODE", raising=False)
    ms = 5.0
    ls = delayed(monkeypatch, "loader", "side", ms, 0)  # only the stream beside the main one
    if ls.stream_name is None:
        pytest.skip("no stream runs beside the main stream")
    d = delayed_call(monkeypatch, restoration, "_stage_patch", ms)
    ref = _host_patches(img_dir, True, seed=11)
    loader = restoration.DevicePatchLoader(img_dir, PATCH, 4, True, dev, shuffle=False, drop_last=False,
                                           rng=random.Random(11))
    got = torch.cat([b.cpu() for b in loader])
    print(f"\nloader on {ls.stream_name}: {d.spins} spins of {ms:.1f} ms in {d.calls} device stages, "
          f"{d.waits_in_spin} waits in a spin")
    assert d.spins == d.calls == ON_DEVICE
    assert torch.equal(got, ref)
    torch.cuda.synchronize()


def test_unreadable_file_raises_in_the_consumer(dev, tmp_path):
    """A host-side error: PIL, the fallback of a file the parser refuses, cannot read it either. The
    exception reaches the consuming thread instead of leaving it blocked."""
    from PIL import UnidentifiedImageError
    from mx_det.restoration import DevicePatchLoader
    (tmp_path / "bad.jpg").write_bytes(b"this is no JPEG file" * 10)
    loader = DevicePatchLoader(tmp_path, PATCH, 4, True, dev, shuffle=False, drop_last=False)
    caught = []

    def consume():
        try:
            list(loader)
        except BaseException as e:
            caught.append(e)

    th = threading.Thread(target=consume, daemon=True)
    th.start()
    th.join(timeout=30.0)
    assert not th.is_alive(), "the consumer is still blocked"
    assert len(caught) == 1 and isinstance(caught[0], UnidentifiedImageError), caught


def test_train_restoration_script_device_loader(dev, tmp_path, monkeypatch):
    from mx_det.data import synth_image
    from mx_det.unet import RestorationUNet
    from scripts import train_restoration as tr
    for split, n in (("train", 16), ("val", 8)):
        d = tmp_path / split
        d.mkdir()
        for i in range(n):
            Image.fromarray(synth_image(i, 280, 300)).save(d / f"{i:04d}.jpg", quality=95)
    monkeypatch.setattr(tr, "PATCH_SIZE", PATCH)
    monkeypatch.setenv("MX_PATCH_LOADER", "bogus")
    with pytest.raises(ValueError):
        tr.main(tmp_path / "train", tmp_path / "val", tmp_path / "none", epochs=1)
    monkeypatch.setenv("MX_PATCH_LOADER", "device")
    best = tr.main(tmp_path / "train", tmp_path / "val", tmp_path / "out", epochs=2)
    hist = [json.loads(line) for line in open(tmp_path / "out/history.jsonl")]
    assert [h["epoch"] for h in hist] == [1, 2]
    assert set(hist[0]) == {"epoch", "train_loss", "lr", "val_psnr", "val_ssim", "elapsed_sec"}
    assert all(np.isfinite(h["train_loss"]) for h in hist)
    assert hist[0]["val_psnr"] is None and hist[1]["val_psnr"] is not None and np.isfinite(best)
    ck = torch.load(tmp_path / "out/best.pth", weights_only=True)
    assert set(ck) == {"model", "epoch", "psnr", "ssim"} and ck["epoch"] == 2
    RestorationUNet(channels=(32, 64, 128, 256)).load_state_dict(ck["model"])
    last = torch.load(tmp_path / "out/last.pth", weights_only=True)
    assert set(last) == {"model", "epoch"} and last["epoch"] == 2
    RestorationUNet(channels=(32, 64, 128, 256)).load_state_dict(last["model"])
