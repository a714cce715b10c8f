"""U-Net restoration training (reference scripts/train_restoration.py) on the HIP U-Net.

Drop-in pieces with the reference's names and semantics:
  ssim(pred, target, window_size=11)      train_restoration.py:142-164 (11x11 Gaussian sigma 1.5, C1/C2)
  CombinedLoss(ssim_weight=0.3)           :167-178  L1 + 0.3 * (1 - SSIM)
  compute_psnr(pred, target)              :185-190
  RestorationDataset(img_dir, patch, is_train)  :54-111 -- (corrupted, clean) f32 CHW patches; here the
      host only decodes, crops and flips (uint8) and the corruption of a whole batch runs on the device
      (ops.corrupt_u8: noise / motion blur / low-res, one random choice per patch) via RestorationBatcher
  train_epoch / validate                  :199-215 / :161-175
  DevicePatchLoader(img_dir, patch, batch, is_train, dev, ...)  the same patches produced on the device
      ahead of the step (MX_PATCH_LOADER=device in scripts/train_restoration.py): JPEG decode with only
      the crop reconstructed, in place of RestorationDataset + DataLoader
The loss runs as the fused HIP SSIM kernels (mx_ssim.hip: window sums, SSIM map, its derivative maps
and the L1 term in one forward launch + a finish block; one backward launch); the U-Net
forward/backward is the HIP path (mx_det.unet).
"""
import math
import random
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from . import augment, ops

NOISE, BLUR, LOWRES = ops.CORRUPT_NOISE, ops.CORRUPT_BLUR, ops.CORRUPT_LOWRES  # augmentations.py ops


def ssim(pred, target, window_size=11):
    """Mean SSIM of NCHW f32 images in [0, 1] (train_restoration.py:142-164 semantics: Gaussian window
    σ 1.5, zero-padded 'same' window sums, C1 = 0.01², C2 = 0.03², no clipping), computed by the fused
    device kernel mx_ssim_l1_fwd; differentiable in `pred`."""
    return ops.ssim(pred, target, window_size)


class CombinedLoss(nn.Module):
    """The reference's restoration loss, mean absolute error + ssim_weight · (1 − SSIM)
    (train_restoration.py:167-178), as one fused forward launch and one fused backward launch."""

    def __init__(self, ssim_weight=0.3):
        super().__init__()
        self.ssim_weight = ssim_weight

    def forward(self, pred, target):
        return ops.ssim_l1_loss(pred, target, self.ssim_weight)


@torch.no_grad()
def compute_psnr(pred, target):
    """Peak signal-to-noise ratio in dB for images in [0, 1] (train_restoration.py:185-190); identical
    images report 100 dB as the reference does."""
    err = float(torch.mean(torch.square(pred.float() - target.float())))
    return 100.0 if err == 0.0 else -10.0 * math.log10(err)


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def _resize_up(img, size):
    """cv2.resize(img, (max(w, size), max(h, size))) (bilinear) for images smaller than the patch."""
    h, w = img.shape[:2]
    if h >= size and w >= size:
        return img
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((max(w, size), max(h, size)), Image.BILINEAR))


class RestorationDataset(torch.utils.data.Dataset):
    """Clean uint8 RGB patches (H, W, 3) of the reference's crops; the corruption happens per batch on
    the device (RestorationBatcher). Train: random crop + 50 % horizontal flip; val: centre crop."""

    def __init__(self, img_dir, patch_size=256, is_train=True):
        self.img_paths = sorted(Path(img_dir).glob("*.jpg"))
        self.patch_size = patch_size
        self.is_train = is_train

    def __len__(self):
        return len(self.img_paths)

    def crop(self, img):
        img = _resize_up(img, self.patch_size)
        h, w = img.shape[:2]
        s = self.patch_size
        if self.is_train:
            y, x = random.randint(0, h - s), random.randint(0, w - s)
            p = img[y:y + s, x:x + s]
            if random.random() > 0.5:
                p = p[:, ::-1]
        else:
            y, x = (h - s) // 2, (w - s) // 2
            p = img[y:y + s, x:x + s]
        return np.ascontiguousarray(p)

    def __getitem__(self, idx):
        return torch.from_numpy(self.crop(_read_rgb(self.img_paths[idx])))


def collate_u8(batch):
    return torch.stack(batch)


# ---------------------------------------------------------------------------------- device patch loader
def draw_crop(rng, h, w, size, is_train):
    """(x0, y0, flip) of RestorationDataset.crop for an h x w frame (already resized up to the patch):
    the same three draws in the same order from `rng` (a random.Random, or the random module); the
    centre crop, and no draw, for validation."""
    if is_train:
        y, x = rng.randint(0, h - size), rng.randint(0, w - size)
        return x, y, rng.random() > 0.5
    return (w - size) // 2, (h - size) // 2, False


class PatchFileDataset(torch.utils.data.Dataset):
    """The files RestorationDataset lists, undecoded: item i is the bytes of the i-th sorted *.jpg as a
    uint8 CPU tensor."""

    def __init__(self, img_dir):
        self.img_paths = sorted(Path(img_dir).glob("*.jpg"))

    def __len__(self):
        return len(self.img_paths)

    def __getitem__(self, idx):
        return torch.from_numpy(np.fromfile(self.img_paths[idx], dtype=np.uint8))


def _collate_files(batch):
    return list(batch)


def _host_patch(data, size, x0, y0, flip):
    """The host path of one file with the crop already drawn: PIL decode, resize up, crop, flip ->
    uint8 [size, size, 3] (what RestorationDataset.crop returns for those draws)."""
    import io
    img = _resize_up(_read_rgb(io.BytesIO(data.tobytes())), size)
    p = img[y0:y0 + size, x0:x0 + size]
    return np.ascontiguousarray(p[:, ::-1] if flip else p)


def _patch_host_stage(data, info, entropy, size, crop):
    """Host half of one file the device path takes (a worker thread): the file's bytes pinned
    (entropy="device") or its coefficients decoded into pinned memory ("host") -> (info, pinned
    tensor); (None, patch) by the host path when the entropy decoder rejects the stream."""
    from . import jpeg
    if entropy == "device":
        return info, jpeg._pin_bytes(data)
    try:
        return jpeg.host_stage(data)
    except ValueError:  # a stream the strict decoder rejects but libjpeg decodes with a warning
        return None, _host_patch(data, size, *crop)


def _stage_patch(info, host, dev, entropy, box, flip, out, status):
    """Device half of one file, on the current (loader) stream: the pinned bytes or coefficients to HBM,
    the entropy decode where it runs on the device, and the window reconstruct into `out` (the
    file's slot of the batch). False when the device entropy decoder refuses the file."""
    from . import jpeg
    if entropy == "device":
        r = jpeg.entropy_stage(info, host, dev, status)
        if r is None:
            return False
        coefs = r[0]
    else:
        coefs = host.to(dev, non_blocking=True)
    jpeg.reconstruct_window(info, coefs, box, hflip=flip, out=out)
    return True


class DevicePatchLoader:
    """RestorationDataset + DataLoader on the device: yields the uint8 [B, S, S, 3] batches
    RestorationBatcher takes, already in HBM, decoded from the files by the hybrid or all-device JPEG
    decoder (MX_JPEG_DECODE) with only the crop reconstructed (mx_jpeg_reconstruct_window), bit-identical
    to what the host path crops for the same draws.

    A producer thread iterates a DataLoader of file bytes (the host loader's sampler semantics: shuffle,
    drop_last, len), parses each header, draws the crop (draw_crop: the draws stay in file order) and
    hands the rest of the file's host work -- pinning the bytes, or the host entropy decode into pinned
    memory -- to `workers` threads, up to `depth` batches ahead. A stager thread, one batch ahead, issues
    the copies, the device entropy decode and one window reconstruct per image into that image's slot
    of the batch tensor on the `loader` stream and records an event; the consumer waits on the event.
    With the entropy decode on the device the batch's status words are read once, after the event, and
    flagged files are redone through the host entropy decoder.

    Frames the parser refuses (progressive, CMYK, ...) and frames smaller than the patch on a side (the
    reference resizes those up) take the host path per file -- _read_rgb, _resize_up, the same drawn
    crop -- and are uploaded into their slot; host_fallbacks counts them. wait_s is the time the
    consumer waited for a staged batch.

    Crops: rng=None draws, at each __iter__ and in the consuming thread, a private
    random.Random(random.getrandbits(64)), and the shuffle order from a private generator seeded from
    torch's global one there, so set_seed still fixes the run and the module-level `random` stream is
    left to RestorationBatcher. For a given seed the patch sequence differs from the host loader's: that
    one interleaves its crop draws with the batcher's corruption draws, which cannot be kept once the
    loader runs ahead of the step."""

    def __init__(self, img_dir, patch_size, batch_size, is_train, dev, shuffle=False, drop_last=False, workers=4,
                 depth=2, rng=None):
        self.dataset = PatchFileDataset(img_dir)
        self.patch_size, self.is_train, self.dev = int(patch_size), bool(is_train), torch.device(dev)
        self.workers, self.depth, self.rng = int(workers), int(depth), rng
        self._gen = torch.Generator()
        self.loader = torch.utils.data.DataLoader(self.dataset, batch_size=batch_size, shuffle=shuffle, num_workers=0,
                                                  drop_last=drop_last, collate_fn=_collate_files, generator=self._gen)
        self.host_fallbacks = 0
        self.wait_s = 0.0

    def __len__(self):
        return len(self.loader)

    def _plan(self, data, rng, pool, entropy):
        """One file in the producer: header parse and crop draw here (the draws keep file order), the
        rest on the pool -> (future of (info, pinned tensor) or (None, patch), data, crop)."""
        from . import jpeg
        s = self.patch_size
        data = data.numpy()  # the decoders and PIL take the file as a byte buffer
        try:
            info = jpeg.parse(data)
        except (jpeg.JpegUnsupported, ValueError):
            info = None
        if info is None or info.height < s or info.width < s:
            import io
            from PIL import Image
            with Image.open(io.BytesIO(data.tobytes())) as im:  # raises for a file PIL cannot read either
                w, h = im.size
            crop = draw_crop(rng, max(h, s), max(w, s), s, self.is_train)
            return pool.submit(lambda: (None, _host_patch(data, s, *crop))), data, crop
        crop = draw_crop(rng, info.height, info.width, s, self.is_train)
        return pool.submit(_patch_host_stage, data, info, entropy, s, crop), data, crop

    def _stage(self, plans, ls, entropy):
        """One batch in the stager -> (uint8 [B, S, S, 3] device tensor, event on the loader stream)."""
        from . import jpeg
        from .conv import capture_lock
        s = self.patch_size
        done = [(f.result(), data, crop) for f, data, crop in plans]
        with capture_lock, torch.cuda.device(self.dev), torch.cuda.stream(ls):
            batch = torch.empty((len(done), s, s, 3), dtype=torch.uint8, device=self.dev)
            status = torch.zeros(len(done), dtype=torch.int32, device=self.dev)
            redo, on_device = [], []
            for k, ((info, host), data, (x0, y0, flip)) in enumerate(done):
                if info is None:
                    self.host_fallbacks += 1
                    batch[k].copy_(torch.from_numpy(host))
                elif _stage_patch(info, host, self.dev, entropy, (x0, y0, s, s), flip, batch[k], status[k:k + 1]):
                    on_device.append(k)
                else:
                    redo.append(k)
            ev = torch.cuda.Event()
            ev.record(ls)
            if entropy == "device" and (on_device or redo):
                ev.synchronize()
                flagged = status.cpu()
                redo += [k for k in on_device if int(flagged[k]) != 0]
                for k in redo:
                    (info, _), data, (x0, y0, flip) = done[k]
                    info, host = _patch_host_stage(data, info, "host", s, (x0, y0, flip))
                    if info is None:
                        self.host_fallbacks += 1
                        batch[k].copy_(torch.from_numpy(host))
                    else:
                        _stage_patch(info, host, self.dev, "host", (x0, y0, s, s), flip, batch[k], None)
                if redo:
                    ev = torch.cuda.Event()
                    ev.record(ls)
        return batch, ev

    def __iter__(self):
        import queue
        import sys
        import threading
        import time
        from concurrent.futures import ThreadPoolExecutor
        from . import jpeg
        from .conv import dedicated_stream
        entropy = jpeg.env_entropy()
        rng = self.rng if self.rng is not None else random.Random(random.getrandbits(64))
        self._gen.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        ls = dedicated_stream(self.dev, "loader")
        q, staged = queue.Queue(maxsize=max(1, self.depth)), queue.Queue(maxsize=1)
        stop = threading.Event()
        old_switch = sys.getswitchinterval()  # see engine.PrefetchJpegLoader
        sys.setswitchinterval(min(old_switch, 0.0005))

        def put(qu, item):
            while not stop.is_set():
                try:
                    qu.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def produce():
            try:
                with ThreadPoolExecutor(max(1, self.workers)) as pool:
                    for files in self.loader:
                        if not put(q, [self._plan(data, rng, pool, entropy) for data in files]):
                            return
            except BaseException as e:  # surfaced in the consuming thread
                put(q, e)
                return
            put(q, None)

        def stager():
            try:
                while not stop.is_set():
                    try:
                        item = q.get(timeout=0.1)
                    except queue.Empty:
                        if not threads[0].is_alive() and q.empty():
                            raise RuntimeError("DevicePatchLoader: the producer thread ended without a result")
                        continue
                    if isinstance(item, list):
                        item = self._stage(item, ls, entropy)
                    if not put(staged, item) or item is None or isinstance(item, BaseException):
                        return
            except BaseException as e:  # surfaced in the consuming thread
                put(staged, e)

        threads = [threading.Thread(target=produce, name="mx-patch-produce", daemon=True),
                   threading.Thread(target=stager, name="mx-patch-stage", daemon=True)]
        for th in threads:
            th.start()
        try:
            while True:
                t0 = time.perf_counter()
                while True:
                    try:
                        item = staged.get(timeout=0.1)
                        break
                    except queue.Empty:
                        if not threads[1].is_alive() and staged.empty():
                            raise RuntimeError("DevicePatchLoader: the stager thread ended without a result")
                self.wait_s += time.perf_counter() - t0
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                batch, ev = item
                main = torch.cuda.current_stream(self.dev)
                main.wait_event(ev)
                batch.record_stream(main)
                yield batch
        finally:
            stop.set()
            sys.setswitchinterval(old_switch)
            for th in threads:
                th.join(timeout=5.0)


class RestorationBatcher:
    """uint8 clean patches [B,S,S,3] (host) -> (corrupted, clean) f32 NCHW in [0, 1] on the device;
    each patch gets random.choice(noise, blur, lowres) as in _apply_random_corruption (:92-100), or a
    uniform choice of `kinds` when those are given ("jpeg": compression at augment.JPEG_QUALITY; "night",
    "haze", "rain": level 3 of their augment.SEVERITY rows, the batch then one ops.corrupt_batch_u8 call).
    severities other than the default (3,): each patch also draws random.choice(severities) after its
    kind, and the batch is one ops.corrupt_batch_u8 call (augment.SEVERITY: blind-severity training)."""

    def __init__(self, dev, kinds=augment.DEFAULT_KINDS, severities=augment.DEFAULT_SEVERITIES):
        self.dev = dev
        self.kinds = augment.check_kinds(kinds)
        self.severities = augment.check_severities(severities)

    def __call__(self, clean_u8):
        x = clean_u8.to(self.dev, non_blocking=True)
        if self.severities != augment.DEFAULT_SEVERITIES:
            specs = []
            for _ in range(x.shape[0]):
                kind = augment._choice(self.kinds)
                specs.append(augment.severity_spec(kind, random.choice(self.severities)))
            cor = ops.corrupt_batch_u8(x, specs, seed=random.getrandbits(62), subsampling=augment.JPEG_SUBSAMPLING)
        else:
            if self.kinds == augment.DEFAULT_KINDS:
                codes = [random.choice((NOISE, BLUR, LOWRES)) for _ in range(x.shape[0])]
            else:
                codes = [augment.RandomCorruptionGPU.CODES[random.choice(list(self.kinds))] for _ in range(x.shape[0])]
            if set(self.kinds) & set(augment.WEATHER_KINDS):  # not mx_corrupt_u8 ops: the batched entry, at level 3
                names = {c: k for k, c in augment.RandomCorruptionGPU.CODES.items()}
                cor = ops.corrupt_batch_u8(x, [augment.severity_spec(names[c], 3) for c in codes],
                                           seed=random.getrandbits(62), subsampling=augment.JPEG_SUBSAMPLING)
            else:
                cor = ops.corrupt_u8(x, codes, seed=random.getrandbits(62), quality=augment.JPEG_QUALITY,
                                     subsampling=augment.JPEG_SUBSAMPLING)
        to = lambda t: t.permute(0, 3, 1, 2).float().div_(255.0)  # noqa: E731
        return to(cor), to(x)


def train_epoch(model, loader, batcher, optimizer, criterion, log_every=200, epoch=0):
    model.train()
    total, n = 0.0, len(loader)
    for i, clean in enumerate(loader):
        corrupted, target = batcher(clean)
        restored = model(corrupted)
        loss = criterion(restored, target)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        v = float(loss.item())
        total += v
        if (i + 1) % log_every == 0 or (i + 1) == n:
            print(f"  [Epoch {epoch:03d}] batch {i + 1}/{n}  loss={v:.4f}", flush=True)
    return total / max(n, 1)


@torch.no_grad()
def validate(model, loader, batcher):
    model.eval()
    tp, ts, n = 0.0, 0.0, 0
    for clean in loader:
        corrupted, target = batcher(clean)
        restored = model(corrupted)
        b = corrupted.size(0)
        tp += compute_psnr(restored, target) * b
        ts += float(ssim(restored, target)) * b
        n += b
    return tp / max(n, 1), ts / max(n, 1)
