"""Detection overlays and side-by-side panels on the device (csrc/mx_draw.hip; contracts in
include/mx_det.h): the drawing half of the reference's scripts/demo_inference.py, which is all cv2 there.

  Overlay(...).batch(...)   frames, label plates and text for a batch of images of any sizes in one launch,
                            reading boxes / labels / scores / counts where the fused detection tail left
                            them (FasterRCNN.detect_padded); only `drawn`, the number of rows drawn per
                            image, is worth reading back
  compose(panels, 480)      the panels resized to one height (cv2.resize's INTER_LINEAR taps) and laid side
                            by side with 3-column separators, one launch
  draw_boxes / add_title    numpy-in / numpy-out drop-ins with the reference's names and signatures
  select_images             the reference's pick of the demo images

The text is the project's own 5x7 bitmap font, not cv2's Hershey strokes, and frames are not anti-aliased:
the pixels are defined by mx_draw_batch_u8's contract (tests/draw_ref.py restates it in numpy), not by
OpenCV. Colours are applied positionally to the image's channels, as the reference hands its RGB-looking
triples to cv2 on BGR images."""
import ctypes
import json
import random

import numpy as np
import torch

from . import _lib

# scripts/demo_inference.py:35-43
CLASS_NAMES = {1: "pedestrian", 2: "car", 3: "van", 4: "truck", 5: "bus", 6: "motor"}
CLASS_COLORS = {1: (30, 144, 255), 2: (0, 200, 0), 3: (255, 165, 0), 4: (148, 103, 189), 5: (220, 20, 60),
                6: (255, 215, 0)}
DEFAULT_COLOR = (200, 200, 200)
SEPARATOR = 3
MAX_CLASSES, MAX_NAME, MAX_TITLE, MAX_PANELS = 32, 15, 64, 8


def tile():
    """(rows, columns) of the output tile one workgroup of mx_draw_batch_u8 owns, and the capacity of its
    row list."""
    out = (ctypes.c_int32 * 3)()
    _lib.call("mx_draw_batch_tile", out)
    return int(out[0]), int(out[1]), int(out[2])


def font():
    """The glyph table: uint8 [95, 7], ASCII 32..126, bit 4 of a row byte = the leftmost column."""
    out = np.zeros((95, 7), np.uint8)
    _lib.call("mx_draw_font", out.ctypes.data)
    return out


def format_score(s):
    """The overlay's score text for the f32 value s (mx_draw_format_score)."""
    out = ctypes.create_string_buffer(5)
    _lib.call("mx_draw_format_score", float(np.float32(s)), out)
    return out.value.decode()


def _table(entries, what):
    """{label: value} or a sequence for labels 1.. -> a list indexed by label - 1 (None: no entry)."""
    if isinstance(entries, dict):
        for k in entries:
            if not (isinstance(k, (int, np.integer)) and 1 <= int(k) <= MAX_CLASSES):
                raise ValueError(f"{what}: labels must be integers in 1..{MAX_CLASSES}, got {k!r}")
        n = max([int(k) for k in entries], default=0)
        return [entries.get(k) for k in range(1, n + 1)]
    entries = list(entries)
    if len(entries) > MAX_CLASSES:
        raise ValueError(f"{what}: at most {MAX_CLASSES} entries, got {len(entries)}")
    return entries


class Overlay:
    """The per-launch settings of mx_draw_batch_u8. class_names / colors: {label: value} as the reference's
    CLASS_NAMES / CLASS_COLORS, or sequences for labels 1, 2, ... (at most 32; names of at most 15 bytes).
    A label without a name renders as cls<label>, one without a colour in (200, 200, 200). conf_thr: a
    scored row is drawn when score >= conf_thr. bar: the title-bar height batch() uses when titles are
    given."""

    def __init__(self, class_names=CLASS_NAMES, colors=CLASS_COLORS, conf_thr=0.35, label_scale=2, title_scale=3,
                 bar=40):
        names = [("" if v is None else str(v)).encode("utf-8") for v in _table(class_names, "class_names")]
        for v in names:
            if len(v) > MAX_NAME:
                raise ValueError(f"class_names: {v!r} is longer than {MAX_NAME} bytes")
        cols = [DEFAULT_COLOR if v is None else tuple(int(c) for c in v) for v in _table(colors, "colors")]
        for v in cols:
            if len(v) != 3 or not all(0 <= c <= 255 for c in v):
                raise ValueError(f"colors: {v!r} is not three bytes")
        for nm, sc in (("label_scale", label_scale), ("title_scale", title_scale)):
            if not 1 <= int(sc) <= 8:
                raise ValueError(f"{nm} must be in 1..8, got {sc!r}")
        if not 0 <= int(bar) <= 1024:
            raise ValueError(f"bar must be in 0..1024, got {bar!r}")
        self.names, self.colors = names, cols
        self.conf_thr, self.label_scale, self.title_scale, self.bar = float(conf_thr), int(label_scale), int(title_scale), int(bar)
        self._names_c = (ctypes.c_char_p * max(len(names), 1))(*names)
        self._colors_c = (ctypes.c_uint8 * max(3 * len(cols), 1))(*[c for v in cols for c in v])

    def batch(self, images, boxes, labels, scores=None, counts=None, titles=None):
        """images: uint8 [N, H, W, 3] or a list of uint8 [H, W, 3] device tensors. boxes [N, D, 4] f32 xyxy,
        labels [N, D] int64, scores [N, D] f32 or None (ground-truth mode: every row, the name alone) --
        tensors, or lists of per-image [D_i, ...] tensors (a scores list may hold None for single images:
        ground truth and detections in one launch); counts: int32 [N] on the device (rows past an
        image's count are ignored), None = every row. titles: one string per image (<= 64 bytes) above the
        image on a bar of self.bar rows, or None: no bar. -> (list of uint8 [bar + H, W, 3] tensors, drawn
        int32 [N] on the device: rows drawn per image, -1 where the count was -1). Stream-ordered; nothing is
        read back."""
        imgs = [im for im in images]
        n = len(imgs)
        if not (len(boxes) == n and len(labels) == n and (scores is None or len(scores) == n)):
            raise ValueError("Overlay.batch: one boxes / labels / scores entry per image")
        if titles is not None and len(titles) != n:
            raise ValueError("Overlay.batch: one title per image")
        if n == 0:
            return [], torch.zeros(0, dtype=torch.int32)
        dev = imgs[0].device
        if dev.type != "cuda":
            raise ValueError("Overlay.batch: device tensors are required (the overlay is a HIP kernel)")
        bar = self.bar if titles is not None else 0
        keep = []  # contiguous copies stay alive until the launch is enqueued
        descs = (_lib.DrawDesc * n)()
        if counts is None:
            counts = torch.tensor([int(b.shape[0]) for b in boxes], dtype=torch.int32).to(dev)
        if not (counts.dtype == torch.int32 and counts.shape == (n,) and counts.device == dev):
            raise ValueError("Overlay.batch: counts is an int32 [N] tensor on the images' device")
        counts = counts.contiguous()
        outs = []
        for i, im in enumerate(imgs):
            if not (im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.device == dev):
                raise ValueError("Overlay.batch: images are uint8 [H, W, 3] tensors on one device")
            im = im.contiguous()
            b = boxes[i].to(torch.float32).contiguous()
            lab = labels[i].to(torch.int64).contiguous()
            sc = None if scores is None or scores[i] is None else scores[i].to(torch.float32).contiguous()
            D = int(b.shape[0])
            if not (b.shape == (D, 4) and lab.shape == (D,) and (sc is None or sc.shape == (D,))
                    and b.device == dev and lab.device == dev and (sc is None or sc.device == dev)):
                raise ValueError(f"Overlay.batch: image {i}: boxes [D, 4], labels [D], scores [D] on the images' device")
            H, W = int(im.shape[0]), int(im.shape[1])
            out = torch.empty((bar + H, W, 3), dtype=torch.uint8, device=dev)
            title = b"" if titles is None else str(titles[i]).encode("utf-8")
            if len(title) > MAX_TITLE:
                raise ValueError(f"Overlay.batch: title of {len(title)} bytes (at most {MAX_TITLE})")
            d = descs[i]
            d.src, d.dst = im.data_ptr(), out.data_ptr()
            d.boxes, d.labels = (b.data_ptr(), lab.data_ptr()) if D else (None, None)
            d.scores = sc.data_ptr() if sc is not None and D else None
            d.count = counts.data_ptr() + 4 * i
            d.H, d.W, d.D, d.bar, d.title_len = H, W, D, bar, len(title)
            d.title = title
            keep += [im, b, lab, sc]
            outs.append(out)
        drawn = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("mx_draw_batch_u8", descs, n, self._names_c, len(self.names), self._colors_c, len(self.colors),
                      self.conf_thr, self.label_scale, self.title_scale, drawn.data_ptr(), _lib.stream())
        return outs, drawn


def panel_widths(shapes, target_h=480):
    """The width of each (h, w) panel at height target_h, as the reference computes it in Python floats."""
    return [int(w * (target_h / h)) for h, w in shapes]


def compose(panels, target_h=480):
    """uint8 [h_p, w_p, 3] device tensors (1..8) -> the uint8 [target_h, sum(dw_p) + 3 * (P - 1), 3] canvas of
    mx_panels_compose_u8: every panel resized to (dw_p, target_h) with cv2.resize's INTER_LINEAR u8 taps,
    dw_p = panel_widths, separated by 3 columns of (200, 200, 200). One launch, stream-ordered."""
    panels = [p.contiguous() for p in panels]
    P = len(panels)
    if not 1 <= P <= MAX_PANELS:
        raise ValueError(f"compose: 1..{MAX_PANELS} panels, got {P}")
    dev = panels[0].device
    for p in panels:
        if not (p.dtype == torch.uint8 and p.dim() == 3 and p.shape[2] == 3 and p.device == dev and dev.type == "cuda"):
            raise ValueError("compose: panels are uint8 [h, w, 3] tensors on one device")
    dws = panel_widths([(int(p.shape[0]), int(p.shape[1])) for p in panels], target_h)
    if min(dws) < 1:
        raise ValueError(f"compose: a panel's width at height {target_h} is below one pixel")
    descs = (_lib.PanelDesc * P)()
    for d, p, dw in zip(descs, panels, dws):
        d.src, d.h, d.w, d.dw = p.data_ptr(), int(p.shape[0]), int(p.shape[1]), dw
    canvas = torch.empty((int(target_h), sum(dws) + SEPARATOR * (P - 1), 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("mx_panels_compose_u8", descs, P, int(target_h), canvas.data_ptr(), _lib.stream())
    return canvas


# ---------------------------------------------------------------------------------- reference drop-ins
_default = None


def _default_overlay():
    global _default
    if _default is None:
        _default = Overlay(conf_thr=float("-inf"))  # the reference's draw_boxes draws every row it is given
    return _default


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("mx_det.draw: the overlay is a HIP kernel and needs a GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _rows(boxes, labels, scores, dev):
    b = torch.as_tensor(np.asarray(boxes, dtype=np.float32).reshape(-1, 4)).to(dev)
    lab = torch.as_tensor(np.asarray(labels).astype(np.int64).reshape(-1)).to(dev)
    sc = None if scores is None else torch.as_tensor(np.asarray(scores, dtype=np.float32).reshape(-1)).to(dev)
    return b, lab, sc


def draw_boxes(img, boxes, labels, scores=None, is_gt=False):
    """scripts/demo_inference.py:90-123 on the device: numpy uint8 [H, W, 3] in, a drawn copy out. Every row is
    drawn (the reference filters by confidence before it calls this); is_gt changes nothing, as there."""
    dev = _device()
    b, lab, sc = _rows(boxes, labels, scores, dev)
    outs, _ = _default_overlay().batch([torch.as_tensor(np.ascontiguousarray(img)).to(dev)], [b], [lab],
                                       None if sc is None else [sc])
    return outs[0].cpu().numpy()


def add_title(img, title, height=40):
    """scripts/demo_inference.py:126-136: a (40, 40, 40) bar of `height` rows with the centred title above img."""
    dev = _device()
    ov = Overlay(bar=height)
    z = torch.zeros((0, 4), device=dev)
    outs, _ = ov.batch([torch.as_tensor(np.ascontiguousarray(img)).to(dev)], [z], [z[:, 0].to(torch.int64)], None,
                       titles=[title])
    return outs[0].cpu().numpy()


def select_images(ann_file, n=5, seed=42):
    """scripts/demo_inference.py:69-84: the images with the most annotations -- a stable sort by count
    descending over the images in file order, the top 50, then random.seed(seed) and random.sample of n."""
    with open(ann_file, encoding="utf-8") as f:
        ds = json.load(f)
    per = {}
    for a in ds.get("annotations", []):
        per[a["image_id"]] = per.get(a["image_id"], 0) + 1
    counts = [(i, per.get(i, 0)) for i in dict.fromkeys(im["id"] for im in ds["images"])]
    counts.sort(key=lambda x: -x[1])
    top = counts[:50]
    random.seed(seed)
    return [s[0] for s in random.sample(top, min(n, len(top)))]
