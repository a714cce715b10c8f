"""numpy restatement of mx_draw_batch_u8 and mx_panels_compose_u8 (include/mx_det.h), written the slow,
literal way: the painter loops over the rows in order and paints frame, plate, text; the composer resizes
each panel with OpenCV's INTER_LINEAR u8 fixed-point taps and stacks. The glyph table comes from the library
(mx_draw_font); the score text is Python's own "%.2f" with the contract's clamp."""
import math

import numpy as np

LIM = float(1 << 20)
WHITE = (255, 255, 255)
DEFAULT = (200, 200, 200)


def font():
    from mx_det import draw
    return draw.font()


def score_text(s):
    """mx_draw_format_score's contract from Python's formatting of the exact f32 value."""
    s = float(np.float32(s))
    if not s > 0.0:
        return "0.00"
    if s >= 9.995:
        return "9.99"
    return f"{s:.2f}"


def _fill(img, xa, ya, xb, yb, col):
    """Inclusive ranges clipped to the image."""
    H, W = img.shape[:2]
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)
    if xa <= xb and ya <= yb:
        img[ya:yb + 1, xa:xb + 1] = col
    return img


def put_text(img, text, x, y, s, glyphs, col=WHITE, ylo=0, yhi=None):
    """Glyph block of `text` (bytes) with its top-left at (x, y), scale s; clipped to rows ylo..yhi."""
    H, W = img.shape[:2]
    yhi = H - 1 if yhi is None else yhi
    for k, ch in enumerate(text):
        g = glyphs[ch - 32] if 32 <= ch <= 126 else glyphs[ord("?") - 32]
        for row in range(7):
            for c in range(5):
                if (int(g[row]) >> (4 - c)) & 1:
                    xa, ya = x + 6 * s * k + s * c, y + s * row
                    for yy in range(max(ya, ylo, 0), min(ya + s - 1, yhi, H - 1) + 1):
                        for xx in range(max(xa, 0), min(xa + s - 1, W - 1) + 1):
                            img[yy, xx] = col
    return img


def label_text(label, names, score):
    label = int(label)
    name = names[label - 1] if 1 <= label <= len(names) and names[label - 1] else f"cls{label}"
    return (name if score is None else f"{name} {score_text(score)}").encode("utf-8")


def paint(src, boxes, labels, scores, count, names, colors, conf_thr=0.35, label_scale=2, title=None, bar=0,
          title_scale=3, glyphs=None):
    """-> (uint8 [bar + H, W, 3], drawn). names / colors: lists for labels 1, 2, ...; scores None: ground truth."""
    glyphs = font() if glyphs is None else glyphs
    H, W = src.shape[:2]
    out = np.empty((bar + H, W, 3), np.uint8)
    out[:bar] = 40
    if bar and title:
        t = title.encode("utf-8") if isinstance(title, str) else title
        tw, th = 6 * title_scale * len(t), 7 * title_scale
        put_text(out, t, (W - tw) // 2, (bar + th) // 2 - th, title_scale, glyphs, ylo=0, yhi=bar - 1)
    img = out[bar:]
    img[:] = src
    count = int(count)
    if count < 0:
        return out, -1
    drawn = 0
    thr = np.float32(conf_thr)
    s, th = label_scale, 7 * label_scale
    ys, xs = np.ogrid[:H, :W]
    for i in range(min(count, len(boxes))):
        if scores is not None and not (np.float32(scores[i]) >= thr):
            continue
        c = [float(v) for v in boxes[i]]
        if not all(math.isfinite(v) and abs(v) < LIM for v in c):
            continue
        x1, y1, x2, y2 = [int(v) for v in c]
        lab = int(labels[i])
        col = tuple(colors[lab - 1]) if 1 <= lab <= len(colors) else DEFAULT
        text = label_text(lab, names, None if scores is None else scores[i])
        tw = 6 * s * len(text)
        # frame: the outer rectangle less the inner one
        outer = (xs >= x1 - 1) & (xs <= x2 + 1) & (ys >= y1 - 1) & (ys <= y2 + 1)
        inner = (xs >= x1 + 1) & (xs <= x2 - 1) & (ys >= y1 + 1) & (ys <= y2 - 1)
        img[outer & ~inner] = col
        _fill(img, x1, y1 - th - 6, x1 + tw + 4, y1, col)
        put_text(img, text, x1 + 2, y1 - 3 - th, s, glyphs)
        drawn += 1
    return out, drawn


# ------------------------------------------------------------------------------------------- compose
def _lin_coef(ssize, dsize, d):
    """OpenCV's INTER_LINEAR source index and 11-bit taps for destination index d (resize.cpp)."""
    scale = 1.0 / (float(dsize) / ssize)
    f = np.float32((d + 0.5) * scale - 0.5)
    s = int(np.floor(f))
    f = np.float32(f - np.float32(s))
    if s < 0:
        f, s = np.float32(0), 0
    if s >= ssize - 1:
        f, s = np.float32(0), ssize - 1
    a0 = int(np.rint(np.float32((np.float32(1) - f) * np.float32(2048))))
    a1 = int(np.rint(np.float32(f * np.float32(2048))))
    return s, a0, a1


def resize_linear(src, dw, dh):
    h, w = src.shape[:2]
    cx = [_lin_coef(w, dw, x) for x in range(dw)]
    cy = [_lin_coef(h, dh, y) for y in range(dh)]
    c0 = np.array([c[0] for c in cx])
    c1 = np.minimum(c0 + 1, w - 1)
    a0 = np.array([c[1] for c in cx], np.int64)[None, :, None]
    a1 = np.array([c[2] for c in cx], np.int64)[None, :, None]
    s64 = src.astype(np.int64)
    hor = s64[:, c0] * a0 + s64[:, c1] * a1  # [h, dw, 3]
    r0 = np.array([c[0] for c in cy])
    r1 = np.minimum(r0 + 1, h - 1)
    b0 = np.array([c[1] for c in cy], np.int64)[:, None, None]
    b1 = np.array([c[2] for c in cy], np.int64)[:, None, None]
    v = ((((hor[r0] >> 4) * b0) >> 16) + (((hor[r1] >> 4) * b1) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def widths(shapes, target_h):
    """The reference's expression (demo_inference.py:243-244)."""
    out = []
    for h, w in shapes:
        scale = target_h / h
        out.append(int(w * scale))
    return out


def compose(panels, target_h=480):
    dws = widths([p.shape[:2] for p in panels], target_h)
    parts = []
    for i, (p, dw) in enumerate(zip(panels, dws)):
        if i:
            parts.append(np.full((target_h, 3, 3), 200, np.uint8))
        parts.append(resize_linear(p, dw, target_h))
    return np.concatenate(parts, 1)
