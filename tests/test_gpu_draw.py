"""mx_draw_batch_u8 and mx_panels_compose_u8 on the GPU, every output bit for bit against the numpy painter and
composer of tests/draw_ref.py: tile and image borders, degenerate and out-of-range rows, painter's order,
counts and thresholds, list chunking, mixed batches, ground-truth mode, titles, scales."""
import numpy as np
import pytest
import torch

import draw_ref as R

pytestmark = pytest.mark.gpu

NAMES = ["pedestrian", "car", "van", "truck", "bus", "motor"]
COLORS = [(30, 144, 255), (0, 200, 0), (255, 165, 0), (148, 103, 189), (220, 20, 60), (255, 215, 0)]
THR = 0.35


@pytest.fixture(scope="module")
def geo(dev):
    from mx_det import draw
    return draw.tile()  # (TR, TC, capacity)


@pytest.fixture(scope="module")
def glyphs(dev):
    return R.font()


def _img(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _case(src, boxes=(), labels=None, scores=None, count=None, title=None):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    D = len(boxes)
    labels = np.asarray(labels if labels is not None else [1 + k % 6 for k in range(D)], np.int64).reshape(-1)
    return dict(src=src, boxes=boxes, labels=labels,
                scores=None if scores is None else np.asarray(scores, np.float32).reshape(-1),
                count=D if count is None else count, title=title)


def run(dev, cases, gt=False, conf_thr=THR, label_scale=2, title_scale=3, bar=40):
    """One launch for `cases`; -> (outputs, drawn) as numpy."""
    from mx_det import draw
    ov = draw.Overlay(NAMES, COLORS, conf_thr=conf_thr, label_scale=label_scale, title_scale=title_scale, bar=bar)
    t = lambda a: torch.from_numpy(a).to(dev)
    titled = any(c["title"] is not None for c in cases)
    scores = None if gt else [t(c["scores"] if c["scores"] is not None else np.ones(len(c["boxes"]), np.float32))
                              for c in cases]
    outs, drawn = ov.batch([t(c["src"]) for c in cases], [t(c["boxes"]) for c in cases], [t(c["labels"]) for c in cases],
                           scores, torch.tensor([c["count"] for c in cases], dtype=torch.int32).to(dev),
                           [c["title"] or "" for c in cases] if titled else None)
    return [o.cpu().numpy() for o in outs], drawn.cpu().numpy()


def check(dev, glyphs, cases, gt=False, conf_thr=THR, label_scale=2, title_scale=3, bar=40):
    outs, drawn = run(dev, cases, gt, conf_thr, label_scale, title_scale, bar)
    titled = any(c["title"] is not None for c in cases)
    for k, c in enumerate(cases):
        sc = None if gt else (c["scores"] if c["scores"] is not None else np.ones(len(c["boxes"]), np.float32))
        want, n = R.paint(c["src"], c["boxes"], c["labels"], sc, c["count"], NAMES, COLORS, conf_thr, label_scale,
                          title=(c["title"] or "") if titled else None, bar=bar if titled else 0,
                          title_scale=title_scale, glyphs=glyphs)
        assert outs[k].shape == want.shape, k
        bad = np.argwhere((outs[k] != want).any(2))
        assert bad.size == 0, (k, len(bad), bad[:5].tolist())
        assert drawn[k] == n, (k, drawn[k], n)
    return outs, drawn


# ------------------------------------------------------------------------------------------- overlay
def test_no_rows_is_a_copy(dev, geo, glyphs):
    TR, TC, _ = geo
    src = _img(0, TR + 3, TC + 9)
    outs, drawn = check(dev, glyphs, [_case(src)])
    assert np.array_equal(outs[0], src) and drawn[0] == 0


def test_one_box_across_tiles_and_an_image_below_one_tile(dev, geo, glyphs):
    TR, TC, _ = geo
    a = _case(_img(1, TR + 5, 2 * TC + 3), [[TC - 20.7, TR - 3.2, TC + 30.9, TR + 3.5]], [2], [0.87])
    b = _case(_img(2, 5, 7), [[1.5, 2.5, 4.2, 3.9]], [1], [0.5])
    outs, drawn = check(dev, glyphs, [a, b])
    assert list(drawn) == [1, 1] and not np.array_equal(outs[0], a["src"]) and not np.array_equal(outs[1], b["src"])


def test_image_borders_and_degenerate_rows(dev, geo, glyphs):
    H, W = 45, 110
    inf, nan, big = float("inf"), float("nan"), float(1 << 20)
    rows = {
        "left": [-6, 30, 20, 40], "right": [90, 28, 130, 41], "top": [30, -9, 60, 12], "bottom": [30, 30, 60, 70],
        "touch_left": [1, 30, 20, 40], "touch_right": [80, 30, W - 2, 40], "touch_top": [40, 1, 60, 10],
        "touch_bottom": [40, 30, 60, H - 2], "plate_crosses_top": [10, 12, 30, 30], "plate_crosses_right": [70, 30, 100, 40],
        "all_over": [-5, -5, W + 5, H + 5], "outside": [200, 200, 240, 240], "outside_negative": [-300, -300, -200, -200],
        "plate_above_row_0": [20, -40, 60, -25], "only_frame_bottom_visible": [20, -40, 60, 0],
        "x2_below_x1": [60, 30, 40, 40], "x2_two_below_x1": [60, 30, 58, 40], "x2_one_below_x1": [60, 30, 59, 40],
        "y2_below_y1": [30, 40, 60, 25], "zero_area": [50, 35, 50, 35], "thin": [50, 30, 51, 31],
        "fractions_truncate": [-0.9, 30.99, 20.99, -0.5 + 41],
    }
    cases = [_case(_img(10 + k, H, W), [r], [1 + k % 6], [0.4 + 0.01 * k]) for k, r in enumerate(rows.values())]
    _, drawn = check(dev, glyphs, cases)
    assert list(drawn) == [1] * len(rows)
    dead = [[nan, 5, 20, 20], [5, nan, 20, 20], [5, 5, inf, 20], [5, 5, 20, -inf], [big, 5, 20, 20], [5, -big, 20, 20],
            [5, 5, 20, np.nextafter(np.float32(big), np.float32(inf))]]
    cases = [_case(_img(40 + k, H, W), [r, [8, 25, 30, 40]], [1, 2], [0.9, 0.9]) for k, r in enumerate(dead)]
    cases.append(_case(_img(60, H, W), [[5, 5, np.nextafter(np.float32(big), np.float32(0)), 20]], [3], [0.9]))
    _, drawn = check(dev, glyphs, cases)
    assert list(drawn) == [1] * len(cases)  # the dead row is not counted; the row just inside the bound is


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_edges_on_and_beside_a_tile_boundary(dev, geo, glyphs, d):
    TR, TC, _ = geo
    H, W = 3 * TR + 4, 2 * TC + 6
    tw, th = 6 * 2 * len("car 0.50"), 14
    X, Y = TC + d, 2 * TR + d  # the column / row the edge lands on
    rows = [[X + 1, Y + 1, X + 30, Y + 9],          # outer left / top edge at X, Y
            [X - 30, Y - 9, X - 1, Y - 1],          # outer right / bottom edge at X, Y
            [X - 1, Y - 1, X + 30, Y + 9],          # inner edge (x1 + 1, y1 + 1) at X, Y
            [X - 30, Y - 9, X + 1, Y + 1],          # inner edge (x2 - 1, y2 - 1) at X, Y
            [X - tw - 4, Y, X - tw + 8, Y + 5],     # plate's right and bottom edge at X, Y
            [X, Y + th + 6, X + 9, Y + th + 11],    # plate's left and top edge at X, Y
            [X - 2, Y + th + 3, X + 9, Y + th + 8]]  # text block's top-left at X, Y
    cases = [_case(_img(70 + k, H, W), [r], [2], [0.5]) for k, r in enumerate(rows)]
    check(dev, glyphs, cases)


def test_painters_order_follows_the_row_order(dev, glyphs):
    src = _img(3, 70, 150)
    boxes = np.array([[20, 30, 90, 60], [40, 22, 110, 50], [30, 40, 120, 66]], np.float32)
    labels, scores = np.array([1, 2, 3]), np.array([0.9, 0.8, 0.7], np.float32)
    outs = []
    for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        o, drawn = check(dev, glyphs, [_case(src, boxes[perm], labels[perm], scores[perm])])
        assert drawn[0] == 3
        outs.append(o[0])
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
    assert not np.array_equal(outs[1], outs[2])


def test_count_threshold_and_failed_count(dev, glyphs):
    H, W = 40, 90
    full = [-10, -10, W + 10, H + 10]
    lo = np.nextafter(np.float32(THR), np.float32(0))
    boxes = [[5, 22, 30, 35], [40, 24, 60, 36], [62, 25, 80, 30], full, full]
    scores = [THR, lo, float("nan"), 0.9, 0.9]
    a = _case(_img(4, H, W), boxes, [1, 2, 3, 4, 5], scores, count=3)       # rows 3, 4 lie beyond the count
    b = _case(_img(5, H, W), boxes, [1, 2, 3, 4, 5], scores, count=-1)      # a failed NMS
    c = _case(_img(6, H, W), boxes[:3], [1, 2, 3], [0.9, 0.9, 0.9], count=9)  # a count over D counts as D
    e = _case(_img(7, H, W), boxes, [1, 2, 3, 4, 5], scores, count=0)
    outs, drawn = check(dev, glyphs, [a, b, c, e])
    assert list(drawn) == [1, -1, 3, 0]
    assert np.array_equal(outs[1], b["src"]) and np.array_equal(outs[3], e["src"])
    # NaN as the threshold draws nothing; -inf draws every finite-scored row
    _, drawn = check(dev, glyphs, [a], conf_thr=float("nan"))
    assert drawn[0] == 0
    _, drawn = check(dev, glyphs, [a], conf_thr=float("-inf"))
    assert drawn[0] == 2


def test_list_chunking_at_and_over_the_capacity(dev, geo, glyphs):
    TR, TC, cap = geo
    H, W = 3 * TR, 2 * TC
    rng = np.random.default_rng(8)
    cases = []
    for k, D in enumerate((cap, cap + 1, 2 * cap + 3)):
        x1 = rng.integers(2, TC - 12, D)
        y1 = rng.integers(TR + 2, 2 * TR - 4, D)
        boxes = np.stack([x1, y1, x1 + rng.integers(0, 9, D), y1 + rng.integers(0, 3, D)], 1).astype(np.float32)
        scores = rng.uniform(0.3, 1.0, D).astype(np.float32)  # some below the threshold
        cases.append(_case(_img(80 + k, H, W), boxes, rng.integers(0, 9, D), scores))
    _, drawn = check(dev, glyphs, cases, label_scale=1)
    assert all(0 < n < len(c["boxes"]) for n, c in zip(drawn, cases))
    # a hit in the first chunk only, under misses in the later ones: the walk crosses empty chunks
    D = 2 * cap + 3
    boxes = np.tile(np.array([[W + 50, H + 50, W + 60, H + 60]], np.float32), (D, 1))
    boxes[3] = [10, TR + 4, 40, TR + 12]
    outs, drawn = check(dev, glyphs, [_case(_img(90, H, W), boxes)], label_scale=1)
    assert drawn[0] == D and not np.array_equal(outs[0], _img(90, H, W))


def test_mixed_batch_equals_each_image_alone(dev, geo, glyphs):
    TR, TC, _ = geo
    rng = np.random.default_rng(9)

    def rows(H, W, D):
        x1, y1 = rng.uniform(-10, W, D), rng.uniform(-10, H, D)
        return np.stack([x1, y1, x1 + rng.uniform(0, 60, D), y1 + rng.uniform(0, 40, D)], 1), rng.integers(1, 8, D), \
            rng.uniform(0.2, 1.0, D)

    a = _case(_img(20, 2 * TR + 1, TC + 17), *rows(2 * TR + 1, TC + 17, 12), count=9, title="Blur + FRCNN (Baseline)")
    b = _case(_img(21, 9, 33), title="empty")
    c = _case(_img(22, TR - 1, 3 * TC), *rows(TR - 1, 3 * TC, 30), title="Clean (Ground Truth)")
    outs, drawn = check(dev, glyphs, [a, b, c], title_scale=1, bar=12)
    assert drawn[1] == 0 and drawn[0] > 0 and drawn[2] > 0
    for k, one in enumerate((a, b, c)):
        o, n = run(dev, [one], title_scale=1, bar=12)
        assert np.array_equal(o[0], outs[k]) and n[0] == drawn[k]
    # 17 images: the second launch of the call
    many = [_case(_img(100 + k, 20 + k, 40 + 3 * k), [[5, 12, 20 + k, 18]], [1 + k % 7], [0.5 + 0.02 * k]) for k in range(17)]
    _, drawn = check(dev, glyphs, many, label_scale=1)
    assert list(drawn) == [1] * 17


def test_ground_truth_mode_and_labels_outside_the_table(dev, glyphs):
    H, W = 60, 330
    boxes = [[5, 25, 40, 50], [60, 25, 100, 50], [150, 25, 200, 50], [5, 52, 30, 58], [120, 52, 140, 58]]
    labels = [0, 7, 123, -5, 3]
    a = _case(_img(30, H, W), boxes, labels)
    outs, drawn = check(dev, glyphs, [a], gt=True)
    assert drawn[0] == 5
    assert R.label_text(0, NAMES, None) == b"cls0" and R.label_text(123, NAMES, None) == b"cls123"
    assert R.label_text(-5, NAMES, None) == b"cls-5" and R.label_text(3, NAMES, None) == b"van"
    # the unnamed labels take the default colour, label 3 its own
    assert tuple(outs[0][24, 4]) == (200, 200, 200) and tuple(outs[0][51, 119]) == COLORS[2]
    far = _case(_img(31, 40, 600), [[4, 20, 30, 30], [4, 38, 30, 39]], [np.iinfo(np.int64).min, np.iinfo(np.int64).max],
                [0.5, 0.25])
    check(dev, glyphs, [far], label_scale=1, conf_thr=0.0)  # the longest text: cls-9223372036854775808 0.50


def test_titles_clip_to_the_bar_and_the_image(dev, glyphs):
    src = _img(32, 12, 50)
    wide = "Blur + FRCNN (Augmented, BNAdapt)"  # 33 * 18 pixels wide: clipped on both sides of a 50-pixel image
    cases = [_case(src, [[10, 8, 30, 11]], [1], [0.5], title=wide), _case(_img(33, 12, 401), title="Clean (Ground Truth)"),
             _case(_img(34, 6, 90), title="café \x01~"), _case(_img(35, 6, 90), title="x" * 64)]
    outs, _ = check(dev, glyphs, cases, bar=40)
    assert outs[0].shape == (52, 50, 3) and (outs[1][:40] == 255).any() and (outs[1][:40] == 40).any()
    check(dev, glyphs, cases, bar=10)  # a bar lower than the title: clipped above and below
    check(dev, glyphs, cases, bar=1, title_scale=2)
    check(dev, glyphs, cases, bar=41, title_scale=1)  # odd bar + th


@pytest.mark.parametrize("scale", [1, 3])
def test_label_scales(dev, glyphs, scale):
    a = _case(_img(36, 80, 260), [[10, 40, 120, 70], [100, 30, 250, 60]], [5, 6], [0.995, 0.005])
    _, drawn = check(dev, glyphs, [a], label_scale=scale, conf_thr=0.0)
    assert drawn[0] == 2


def test_numpy_drop_ins(dev, glyphs):
    from mx_det import draw
    src = _img(37, 50, 120)
    boxes, labels, scores = [[10.6, 25.2, 60.9, 44.1]], [2], [0.349]  # below 0.35: draw_boxes draws what it is given
    got = draw.draw_boxes(src, boxes, labels, scores)
    want, _ = R.paint(src, np.float32(boxes), labels, np.float32(scores), 1, NAMES, COLORS, float("-inf"), glyphs=glyphs)
    assert np.array_equal(got, want)
    got = draw.draw_boxes(src, boxes, labels, is_gt=True)
    want, _ = R.paint(src, np.float32(boxes), labels, None, 1, NAMES, COLORS, glyphs=glyphs)
    assert np.array_equal(got, want)
    got = draw.add_title(src, "Clean (Ground Truth)")
    want, _ = R.paint(src, np.zeros((0, 4)), [], None, 0, NAMES, COLORS, title="Clean (Ground Truth)", bar=40, glyphs=glyphs)
    assert got.shape == (90, 120, 3) and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- compose
def _compose(dev, panels, target_h):
    from mx_det import draw
    got = draw.compose([torch.from_numpy(p).to(dev) for p in panels], target_h).cpu().numpy()
    want = R.compose(panels, target_h)
    assert got.shape == want.shape
    bad = np.argwhere((got != want).any(2))
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    return got


def test_compose_one_panel(dev):
    p = _img(50, 37, 91)
    got = _compose(dev, [p], 24)
    assert got.shape == (24, int(91 * (24 / 37)), 3)
    assert np.array_equal(_compose(dev, [p], 37), p)  # the same size: a copy


def test_compose_three_panels_up_down_and_half(dev):
    from mx_det import draw
    shapes = [(11, 17), (23, 5), (48, 64)]  # at 24: an up-scale, a down-scale, exactly one half
    panels = [_img(51 + k, h, w) for k, (h, w) in enumerate(shapes)]
    dws = draw.panel_widths(shapes, 24)
    assert dws == R.widths(shapes, 24) == [int(17 * (24 / 11)), int(5 * (24 / 23)), 32]
    got = _compose(dev, panels, 24)
    assert got.shape == (24, sum(dws) + 6, 3)
    x = dws[0]
    assert (got[:, x:x + 3] == 200).all() and (got[:, x + 3 + dws[1]:x + 6 + dws[1]] == 200).all()


def test_compose_width_one_panel_and_many_tiles(dev, geo):
    TR, TC, _ = geo
    panels = [_img(54, 30, 1), _img(55, 2 * TR + 3, 3 * TC + 7), _img(56, 1, 9)]
    assert R.widths([p.shape[:2] for p in panels], 30)[0] == 1
    _compose(dev, panels, 30)
    _compose(dev, [_img(57 + k, 7 + k, 9 + 2 * k) for k in range(8)], 2 * TR + 1)  # eight panels
