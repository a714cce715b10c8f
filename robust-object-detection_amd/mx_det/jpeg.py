"""Baseline-JPEG decode onto the device. Two ways to the quantised coefficients:

entropy="host" (the default): the Huffman-coded bitstream is decoded on the host (libmx_det
mx_jpeg_decode_coefs, a sequential bit-at-a-time loop) and the coefficients (int16, ~1.5 B per pixel
at 4:2:0, about four times the file's size) are copied to HBM.

entropy="device" (MX_JPEG_DECODE=device for read_file and the loaders): only the file's bytes are
copied and mx_jpeg_entropy_decode decodes the scan on the device. The scan does have parallel
structure, restart markers or not: a Huffman stream re-synchronises, so lanes decode fixed-size
subsequences speculatively and a fix-up iteration makes the result the sequential decoder's, bit for
bit. A stream the device decoder flags (truncated, corrupt: a non-zero status word) is decoded by the
host path, so results and exceptions are those of entropy="host" for every input.

Either way the device then dequantises, runs the libjpeg islow IDCT, upsamples the chroma and converts
YCbCr -> RGB (mx_jpeg_reconstruct). Output: uint8 [H, W, 3] on the device, bit-identical to
libjpeg-turbo's default decode -- PIL Image.open(p).convert("RGB") (coco_detection_dataset.py:23), or
with bgr=True cv2.imread (restore_testsets.py:99). Progressive / arithmetic / CMYK / 4:4:0 files raise
NotImplementedError (MX_EUNSUPPORTED); callers that must accept them decode those on the host.

A window of the frame (reconstruct_window / decode_window, mx_jpeg_reconstruct_window) is reconstructed
from the same coefficients without the rest: the U-Net patch loader (mx_det.restoration) keeps one crop
per frame.

Encode (encode / write_file / encode_coefs, below) runs wholly on the device -- pixel stage and
entropy coder -- and is byte-identical to PIL's Image.save(format="JPEG", quality, subsampling).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import JpegInfo


class JpegUnsupported(NotImplementedError):
    pass


def parse(data):
    """Marker parse of the bytes `data` -> JpegInfo (host)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    info = JpegInfo()
    rc = _lib.load().mx_jpeg_parse(buf.ctypes.data, buf.size, ctypes.byref(info))
    if rc == -2:
        raise JpegUnsupported(_lib.load().mx_last_error().decode())
    if rc != 0:
        raise ValueError(_lib.load().mx_last_error().decode())
    return info


def decode_coefs(data, info=None, out=None):
    """Host entropy decode -> (info, int16 [coef_total]) of quantised natural-order coefficients: a numpy
    array, or `out` (an int16 CPU tensor of >= coef_total elements, e.g. pinned) filled in place. The
    decoder is a ctypes call into libmx_det, which releases the GIL: threads decode in parallel."""
    info = parse(data) if info is None else info
    buf = np.frombuffer(data, dtype=np.uint8)
    if out is None:
        coefs = np.empty(info.coef_total, dtype=np.int16)
        ptr = coefs.ctypes.data
    else:
        if not (out.dtype == torch.int16 and out.device.type == "cpu" and out.is_contiguous()
                and out.numel() >= info.coef_total):
            raise ValueError("decode_coefs: out must be a contiguous int16 CPU tensor of coef_total elements")
        coefs, ptr = out, out.data_ptr()
    rc = _lib.load().mx_jpeg_decode_coefs(buf.ctypes.data, buf.size, ctypes.byref(info), ptr)
    if rc != 0:
        raise ValueError(_lib.load().mx_last_error().decode())
    return info, coefs


def host_stage(data):
    """The host half of decode(): marker parse + entropy decode straight into pinned memory ->
    (info, pinned int16 tensor), ready for an asynchronous copy (device_stage). Thread-safe."""
    from .conv import capture_lock
    info = parse(data)
    # pinned allocations (cudaHostAlloc on a cache miss) are prohibited while another thread has a graph
    # capture open in global mode: the training thread's captures (frcnn._Graphs) hold capture_lock
    with capture_lock:
        host = torch.empty(info.coef_total, dtype=torch.int16, pin_memory=True)
    return decode_coefs(data, info, out=host)


def _reconstruct(info, dev, device, bgr):
    ws = torch.empty(_lib.load().mx_jpeg_workspace(ctypes.byref(info)), dtype=torch.uint8, device=device)
    out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=device)
    _lib.call("mx_jpeg_reconstruct", dev.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), out.data_ptr(),
              int(bool(bgr)), _lib.stream())
    return out


def device_stage(info, host, device, bgr=False):
    """The device half: coefficients to HBM (non-blocking from pinned memory), then dequantise + islow
    IDCT + chroma upsampling + YCbCr -> RGB in mx_jpeg_reconstruct on the current stream."""
    return _reconstruct(info, host.to(device, non_blocking=True), device, bgr)


def env_entropy():
    """Where read_file, the loaders (mx_det.engine) and the offline scripts decode the scan:
    MX_JPEG_DECODE = host (the default) or device."""
    mode = os.environ.get("MX_JPEG_DECODE", "host")
    if mode not in ("host", "device"):
        raise ValueError("MX_JPEG_DECODE is 'host' or 'device'")
    return mode


def set_subseq(bits):
    """Bits one lane of the device entropy decoder walks (64 .. 65536, default 512): a process setting,
    results identical."""
    if _lib.load().mx_jpeg_entropy_decode_set_subseq(int(bits)) != 0:
        raise ValueError(_lib.load().mx_last_error().decode())


def decode_coefs_chunked(data, subseq_bits=0, info=None):
    """The device entropy decoder's passes run serially on the host (mx_jpeg_decode_coefs_chunked, the
    CPU reference of the kernels) -> (info, int16 [coef_total], status)."""
    info = parse(data) if info is None else info
    buf = np.frombuffer(data, dtype=np.uint8)
    coefs = np.empty(info.coef_total, dtype=np.int16)
    status = ctypes.c_int32(0)
    rc = _lib.load().mx_jpeg_decode_coefs_chunked(buf.ctypes.data, buf.size, ctypes.byref(info), int(subseq_bits),
                                                  coefs.ctypes.data, ctypes.byref(status))
    if rc != 0:
        raise ValueError(_lib.load().mx_last_error().decode())
    return info, coefs, status.value


def _pin_bytes(data):
    from .conv import capture_lock
    buf = np.frombuffer(data, dtype=np.uint8)
    with capture_lock:  # see host_stage
        host = torch.empty(buf.size, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = buf
    return host


def host_stage_bytes(data):
    """The host half with the entropy decode on the device: marker parse + the file's bytes in pinned
    memory -> (info, pinned uint8 tensor). Thread-safe."""
    return parse(data), _pin_bytes(data)


def entropy_stage(info, host, device, status=None, offset=0):
    """File bytes (a CPU uint8 tensor, pinned for a non-blocking copy) to HBM -- the file's size, not
    coef_total * 2 bytes -- and mx_jpeg_entropy_decode on the current stream -> (int16 [coef_total]
    device tensor, status), or None when the entry point refuses the file (a Huffman table the host
    decoder rejects too). status: a one-element int32 device tensor to fill (a slot of a batch's status
    words), allocated when None; 0 means the coefficients are mx_jpeg_decode_coefs', anything else that
    the host must decode the file. No host synchronisation. offset: extra bytes in front of the device
    copy (tests: the scan at another alignment)."""
    lib = _lib.load()
    n = host.numel()
    dev = torch.empty(offset + n, dtype=torch.uint8, device=device)
    dev[offset:].copy_(host, non_blocking=True)
    nscan = n - info.scan_off
    ws = torch.empty(max(int(lib.mx_jpeg_entropy_decode_workspace(ctypes.byref(info), nscan)), 1), dtype=torch.uint8,
                     device=device)
    coefs = torch.empty(info.coef_total, dtype=torch.int16, device=device)
    if status is None:
        status = torch.empty(1, dtype=torch.int32, device=device)
    rc = lib.mx_jpeg_entropy_decode(dev.data_ptr() + offset + info.scan_off, nscan, ctypes.byref(info), ws.data_ptr(),
                                    ws.numel(), coefs.data_ptr(), status.data_ptr(), _lib.stream())
    if rc == -1:
        return None
    if rc != 0:
        raise _lib.MxError(f"mx_jpeg_entropy_decode failed ({rc}): {lib.mx_last_error().decode()}")
    return coefs, status


def device_stage_bytes(info, host, device, bgr=False, status=None):
    """The device half with the entropy decode on the device: entropy_stage + mx_jpeg_reconstruct ->
    (uint8 [H, W, 3], status), or None (see entropy_stage). The image is valid where the status reads 0."""
    r = entropy_stage(info, host, device, status)
    if r is None:
        return None
    return _reconstruct(info, r[0], device, bgr), r[1]


def decode_coefs_device(data, device, info=None):
    """Device entropy decode -> (info, int16 [coef_total] device tensor, int32 [1] device status tensor;
    0: the coefficients equal decode_coefs'). The file's bytes go up as one pinned, non-blocking copy."""
    info = parse(data) if info is None else info
    r = entropy_stage(info, _pin_bytes(data), device)
    if r is None:
        raise ValueError(_lib.load().mx_last_error().decode())
    return info, r[0], r[1]


def decode(data, device, bgr=False, pin=True, entropy="host"):
    """JPEG bytes -> uint8 [H, W, 3] tensor on `device` (RGB, or BGR with bgr=True). entropy="device":
    the parse on the host, the entropy decode and the reconstruction on the device, then one read of
    the status word; a flagged file goes through the host path, so results and exceptions are those of
    entropy="host" for every input."""
    if entropy not in ("host", "device"):
        raise ValueError("decode: entropy is 'host' or 'device'")
    if entropy == "device":
        r = device_stage_bytes(*host_stage_bytes(data), device, bgr)
        if r is not None and int(r[1].item()) == 0:
            return r[0]
    if pin:
        return device_stage(*host_stage(data), device, bgr)
    info, coefs = decode_coefs(data)
    return _reconstruct(info, torch.from_numpy(coefs).to(device), device, bgr)


# ------------------------------------------------------------------------------------------ window
def window_cover(info, box):
    """Blocks each component of `info` needs for the window box = (x0, y0, w, h), the fancy
    upsampling's one-sample halo included: an int32 [3, 4] array of (bx0, by0, bx1, by1), high end
    exclusive (zeros for the absent components of a grey frame). Host only (mx_jpeg_window_cover: the
    function the kernel calls per tile)."""
    x0, y0, w, h = (int(v) for v in box)
    cover = np.zeros((3, 4), dtype=np.int32)
    rc = _lib.load().mx_jpeg_window_cover(ctypes.byref(info), x0, y0, w, h, cover.ctypes.data)
    if rc != 0:
        raise ValueError(_lib.load().mx_last_error().decode())
    return cover


def reconstruct_window(info, coefs_dev, box, hflip=False, bgr=False, out=None):
    """The window box = (x0, y0, w, h) of the frame from its device coefficients (decode_coefs' layout)
    -> uint8 [h, w, 3] on the device: decode(...)[y0:y0 + h, x0:x0 + w], flipped left-right with
    hflip, bit for bit, with work proportional to the window (mx_jpeg_reconstruct_window, on the
    current stream). out: a uint8 [h, w, 3] device tensor to fill instead, dense inside a row but with
    any row stride (batch[b], or a column range of it)."""
    x0, y0, w, h = (int(v) for v in box)
    if out is None:
        out = torch.empty((max(h, 0), max(w, 0), 3), dtype=torch.uint8, device=coefs_dev.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == coefs_dev.device
              and tuple(out.shape) == (h, w, 3) and out.stride(2) == 1 and out.stride(1) == 3
              and (h <= 1 or out.stride(0) >= 3 * w)):
        raise ValueError("reconstruct_window: out must be a uint8 [h, w, 3] tensor on the coefficients' device with "
                         "dense rows")
    if coefs_dev.dtype != torch.int16 or coefs_dev.numel() < info.coef_total or not coefs_dev.is_contiguous():
        raise ValueError("reconstruct_window: coefs_dev must be a contiguous int16 tensor of coef_total elements")
    row_bytes = out.stride(0) if h > 1 else max(out.stride(0), 3 * w)
    _lib.call("mx_jpeg_reconstruct_window", coefs_dev.data_ptr(), ctypes.byref(info), x0, y0, w, h, int(bool(hflip)),
              int(bool(bgr)), out.data_ptr(), row_bytes, _lib.stream())
    return out


def decode_window(data, device, box, hflip=False, bgr=False, entropy="host"):
    """JPEG bytes -> the window box = (x0, y0, w, h) of the decoded frame, uint8 [h, w, 3] on `device`:
    decode(data, device, bgr)[y0:y0 + h, x0:x0 + w] (flipped left-right with hflip) without
    reconstructing the rest of the frame. The entropy decode covers the whole scan, on the host or the
    device as in decode(); a file the device decoder flags goes through the host entropy path."""
    if entropy not in ("host", "device"):
        raise ValueError("decode_window: entropy is 'host' or 'device'")
    if entropy == "device":
        info, host = host_stage_bytes(data)
        r = entropy_stage(info, host, device)
        if r is not None:
            out = reconstruct_window(info, r[0], box, hflip, bgr)
            if int(r[1].item()) == 0:
                return out
    info, host = host_stage(data)
    return reconstruct_window(info, host.to(device, non_blocking=True), box, hflip, bgr)


def read_file(path, device, bgr=False):
    with open(path, "rb") as f:
        return decode(f.read(), device, bgr=bgr, entropy=env_entropy())


# ------------------------------------------------------------------------------------------ encode
# Byte-identical to PIL's Image.save(format="JPEG", quality=q, subsampling=s) (libjpeg-turbo, the
# encoder behind cv2.imwrite too): the pixel stage (colour, chroma downsampling, islow forward DCT,
# quantisation: mx_jpeg_forward) and the entropy coder (mx_jpeg_entropy) both run on the device; only
# the finished scan bytes come back.
_EOI = b"\xff\xd9"


def _rc(rc):
    if rc == -2:
        raise JpegUnsupported(_lib.load().mx_last_error().decode())
    if rc != 0:
        raise ValueError(_lib.load().mx_last_error().decode())


def encode_info(width, height, quality=95, subsampling=2):
    """JpegInfo of an encode: geometry, scaled Annex K quantisation tables, standard Huffman tables.
    subsampling in PIL's numbering: 0 = 4:4:4, 2 = 4:2:0."""
    info = JpegInfo()
    _rc(_lib.load().mx_jpeg_encode_info(int(width), int(height), int(quality), int(subsampling), ctypes.byref(info)))
    return info


def header(info):
    """The marker segments from SOI up to and including SOS (host)."""
    buf = np.empty(2048, dtype=np.uint8)
    n = ctypes.c_int64(0)
    _rc(_lib.load().mx_jpeg_write_header(ctypes.byref(info), buf.ctypes.data, buf.size, ctypes.byref(n)))
    return buf[:n.value].tobytes()


def encode_coefs(info, coefs):
    """Host Huffman coder: quantised natural-order int16 coefficients (decode_coefs' layout; a numpy
    array or a CPU tensor) with the tables of `info` -> the complete JPEG file as bytes."""
    if torch.is_tensor(coefs):
        coefs = coefs.numpy()
    coefs = np.ascontiguousarray(coefs, dtype=np.int16).reshape(-1)
    if coefs.size < info.coef_total:
        raise ValueError("encode_coefs: fewer than coef_total coefficients")
    lib = _lib.load()
    head = header(info)
    buf = np.empty(max(int(lib.mx_jpeg_scan_bound(ctypes.byref(info))), 1), dtype=np.uint8)
    n = ctypes.c_int64(0)
    _rc(lib.mx_jpeg_encode_coefs(ctypes.byref(info), coefs.ctypes.data, buf.ctypes.data, buf.size, ctypes.byref(n)))
    return head + buf[:n.value].tobytes() + _EOI


def forward(img, info, bgr=False):
    """Device pixel stage: uint8 [H, W, 3] device tensor -> int16 [coef_total] device tensor of the
    quantised coefficients libjpeg-turbo would code (dummy blocks included)."""
    coefs = torch.empty(info.coef_total, dtype=torch.int16, device=img.device)
    _lib.call("mx_jpeg_forward", img.data_ptr(), int(bool(bgr)), ctypes.byref(info), coefs.data_ptr(), _lib.stream())
    return coefs


def encode(img, quality=95, subsampling=2, bgr=False, entropy="device"):
    """uint8 [H, W, 3] device tensor (RGB, or BGR with bgr=True) -> the bytes of the JPEG file PIL's
    Image.save(format="JPEG", quality=quality, subsampling=subsampling) writes for those pixels.
    entropy="device": the Huffman coder runs on the device too (mx_jpeg_entropy) and two host
    synchronisations happen per image: reading the length of the scan (one int64), then copying that
    many bytes back. entropy="host": the coefficients are copied back (one synchronisation) and coded
    by mx_jpeg_encode_coefs. Grey, 4:2:2 and non-uint8 input raise ValueError."""
    if not (torch.is_tensor(img) and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3):
        raise ValueError("encode: a uint8 [H, W, 3] tensor is required")
    if img.device.type != "cuda":
        raise ValueError("encode: a device tensor is required")
    if subsampling not in (0, 2):
        raise ValueError("encode: subsampling 0 (4:4:4) or 2 (4:2:0) only")
    if entropy not in ("device", "host"):
        raise ValueError("encode: entropy is 'device' or 'host'")
    img = img.contiguous()
    info = encode_info(img.shape[1], img.shape[0], quality, subsampling)
    with torch.cuda.device(img.device):
        coefs = forward(img, info, bgr)
        if entropy == "host":
            return encode_coefs(info, coefs.cpu())
        lib = _lib.load()
        ws = torch.empty(lib.mx_jpeg_entropy_workspace(ctypes.byref(info)), dtype=torch.uint8, device=img.device)
        cap = int(lib.mx_jpeg_scan_bound(ctypes.byref(info)))
        out = torch.empty(cap, dtype=torch.uint8, device=img.device)
        nbytes = torch.empty(1, dtype=torch.int64, device=img.device)
        _lib.call("mx_jpeg_entropy", coefs.data_ptr(), ctypes.byref(info), ws.data_ptr(), ws.numel(), out.data_ptr(),
                  cap, nbytes.data_ptr(), _lib.stream())
        n = int(nbytes.item())  # synchronisation 1
        if n < 0 or n > cap:
            raise _lib.MxError(f"mx_jpeg_entropy: scan of {n} bytes (capacity {cap})")
        scan = out[:n].cpu().numpy().tobytes()  # synchronisation 2
    return header(info) + scan + _EOI


def write_file(path, img, **kw):
    """encode(img, **kw) written to `path`."""
    data = encode(img, **kw)
    with open(path, "wb") as f:
        f.write(data)
