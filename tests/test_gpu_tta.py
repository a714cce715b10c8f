"""Flip test-time augmentation on the device (mx_det_views_fold, mx_det_select_vote,
ops.detections_postprocess_views) and the eval forward that uses it (FasterRCNN.tta): each kernel bit for
bit against the numpy restatement of tests/tta_ref.py on hand-built candidates, the composed path against
detection_candidates + the numpy fold + the CPU oracle's batched_nms + the numpy vote, under graph capture,
and at model level."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

THR, NMS_THR = 0.05, 0.5
F32 = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """Bitwise equality of two arrays / tensors (NaNs and signed zeros included)."""
    a = _np(a) if torch.is_tensor(a) else np.asarray(a)
    b = _np(b) if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_outputs(got, ref):
    ob, osc, ol, counts = got
    rb, rs, rl, rc = ref[:4]
    assert ob.dtype == torch.float32 and osc.dtype == torch.float32 and ol.dtype == torch.int64
    assert counts.dtype == torch.int32 and counts.tolist() == rc.tolist()
    assert _same(ol, rl) and _same(osc, rs)
    assert _same(ob, rb), np.argwhere(_np(ob) != rb)[:8]


# ------------------------------------------------------------------------------------------ 1. fold
def _fold_inputs(C, V=2, N=2, P=5, seed=0):
    rng = np.random.default_rng(seed)
    n = V * N * P * (C - 1)
    hw = np.array([[41., 37.], [29., 53.]], F32)
    block = np.repeat(np.arange(V * N, dtype=np.int32), P * (C - 1))
    w = hw[block % N, 1]
    x = np.sort(rng.uniform(0, 1, (n, 2)).astype(F32) * w[:, None], 1)
    x[::7, 1] = w[::7]  # x2 on the right edge: mirrors to exactly 0
    x[3::7, 0] = 0
    y = np.sort(rng.uniform(0, 29, (n, 2)).astype(F32), 1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)
    grp = block.copy()
    dead = rng.random(n) < 0.3
    dead[[0, n - 1]] = True
    grp[dead] = V * N
    assert all((grp[block == b] == V * N).any() and (grp[block == b] == b).any() for b in range(V * N))
    wrong = np.flatnonzero(~dead)[[1, -2]]  # a live value that names another block: dead here
    grp[wrong] = (block[wrong] + 1) % (V * N)
    d = np.flatnonzero(dead)
    boxes[d[0]] = np.nan
    boxes[d[1]] = [np.inf, -np.inf, np.inf, 3.0]
    boxes[d[-1]] = [-np.inf, 1.0, np.nan, np.inf]
    return boxes, grp, hw, (V, N, P, C)


@pytest.mark.parametrize("C", [2, 7])
def test_fold(dev, C):
    from mx_det import _lib, ops
    boxes, grp, hw, (V, N, P, C) = _fold_inputs(C)
    flips = (False, True)
    rb, rg = T.fold(boxes, grp, hw, V, N, P, C, flips)
    live = rg < N
    assert live.any() and (~live).any() and not np.array_equal(rb[live], boxes[live])
    assert (rb[live, 0] >= 0).all() and (rb[live, 0] <= rb[live, 2]).all() and (rb[live, 0] == 0).any()
    d_boxes, d_grp, d_hw = (torch.from_numpy(a).to(dev) for a in (boxes, grp, hw))
    # canary prefill: every element of both outputs is written
    ob = torch.full_like(d_boxes, -12345.0)
    og = torch.full_like(d_grp, -77)
    n = boxes.shape[0]
    import ctypes
    _lib.call("mx_det_views_fold", d_boxes.data_ptr(), d_grp.data_ptr(), d_hw.data_ptr(), n, V, N, P, C,
              (ctypes.c_int32 * V)(*map(int, flips)), ob.data_ptr(), og.data_ptr(), _lib.stream())
    assert not (_np(ob) == -12345.0).any() and not (_np(og) == -77).any()
    assert _same(ob, rb) and _same(og, rg)
    assert _same(d_boxes, boxes) and _same(d_grp, grp)  # the inputs are only read
    gb, gg = ops.detection_views_fold(d_boxes, d_grp, d_hw, V, N, P, C, flips)
    assert _same(gb, rb) and _same(gg, rg) and gb.data_ptr() != d_boxes.data_ptr()
    # in place
    ib, ig = ops.detection_views_fold(d_boxes, d_grp, d_hw, V, N, P, C, flips, inplace=True)
    assert ib.data_ptr() == d_boxes.data_ptr() and ig.data_ptr() == d_grp.data_ptr()
    assert _same(d_boxes, rb) and _same(d_grp, rg)
    # no view flipped: only the groups change
    kb, kg = ops.detection_views_fold(torch.from_numpy(boxes).to(dev), torch.from_numpy(grp).to(dev), d_hw, V, N, P, C,
                                      (False, False))
    assert _same(kb, boxes) and _same(kg, rg)


# ------------------------------------------------------------------------------------------ 2. select-vote
VOTE = dict(V=2, N=3, P=150)
BIG = np.array([10., 10., 50., 60.], F32)      # the survivor with voters in several ballot rounds
LONE0 = np.array([200., 100., 215., 130.], F32)
PAIR8 = (np.array([300., 0., 304., 5.], F32), np.array([300., 0., 304., 4.], F32))    # IoU = float32(0.8)
PAIR5 = (np.array([320., 0., 322., 2.], F32), np.array([320., 0., 322., 1.], F32))    # IoU = 0.5


def _vote_inputs(C, seed=0):
    """Hand-built folded candidates. Image 0: BIG (class 1) with 180 jittered copies over both views plus
    a few that overlap it too little; five lone survivors of the last class, the first with perfect copies
    in another class, another image and a dead slot; the two exact-threshold pairs. Image 1: a lone
    survivor first, then 130 survivors of which every third has two or three voters. Image 2: live
    candidates, no survivor. -> (boxes, scores, labels, grp, keep, nk, marks)."""
    V, N, P = VOTE["V"], VOTE["N"], VOTE["P"]
    rng = np.random.default_rng(seed)
    n = V * N * P * (C - 1)
    cl = C - 1  # the last class (1 when C == 2)

    def slot(v, i, r, c):
        return ((v * N + i) * P + r) * (C - 1) + (c - 1)

    boxes = np.tile(np.array([600., 600., 640., 640.], F32), (n, 1)) + rng.uniform(0, 5, (n, 4)).astype(F32)
    scores = rng.uniform(0.06, 1.0, n).astype(F32)
    labels = np.tile(np.arange(1, C, dtype=np.int64), V * N * P)
    grp = np.full(n, N, np.int32)
    surv = [[], [], []]

    def put(v, i, r, c, box, live=True, score=None):
        t = slot(v, i, r, c)
        boxes[t] = box
        grp[t] = i if live else N
        if score is not None:
            scores[t] = score
        return t

    # image 0, class 1: BIG + 180 voters (rows 1..90 of view 0, 0..89 of view 1: candidates 0..90 and
    # 150..239 of its walk, four ballot rounds) + 8 near misses
    k_big = put(0, 0, 0, 1, BIG, score=0.99)
    surv[0].append(k_big)
    for v, rows in ((0, range(1, 91)), (1, range(0, 90))):
        for r in rows:
            put(v, 0, r, 1, BIG + rng.uniform(-0.4, 0.4, 4).astype(F32))
    for j, r in enumerate(range(91, 95)):
        put(0, 0, r, 1, BIG + np.array([8. + j, 0, 8. + j, 0], F32))  # IoU about 0.6: below 0.8
        put(1, 0, r, 1, BIG + np.array([0, 9. + j, 0, 9. + j], F32))
    # image 0, last class: lone survivors; LONE0 has perfect copies that must not vote
    lone = []
    for j in range(5):
        lone.append(put(0 if j % 2 == 0 else 1, 0, 100 + j, cl, LONE0 + F32(20 * j) * np.array([1, 0, 1, 0], F32),
                        score=0.9 - 0.01 * j))
    surv[0] += lone
    if C > 2:
        put(0, 0, 100, 1 if cl != 1 else 2, LONE0)      # another class, same row
        put(1, 0, 120, cl - 1, LONE0)
    put(0, 1, 140, cl, LONE0)                            # another image (live there)
    put(1, 2, 100, cl, LONE0)
    put(1, 0, 130, cl, LONE0, live=False)                # dead
    put(0, 0, 131, cl, LONE0, live=False)
    # the exact-threshold pairs, survivor in view 0 and the candidate in view 1
    k8 = put(0, 0, 110, cl, PAIR8[0], score=0.5)
    put(1, 0, 111, cl, PAIR8[1], score=0.25)
    k5 = put(0, 0, 112, cl, PAIR5[0], score=0.4)
    put(1, 0, 113, cl, PAIR5[1], score=0.125)
    surv[0] += [k8, k5]
    # image 1: a lone survivor first, then a grid of 130 survivors, every third with mates in the other view
    for j in range(131):
        c = 1 + j % (C - 1)
        base = np.array([10. + 30 * (j % 12), 10. + 30 * (j // 12), 32. + 30 * (j % 12), 33. + 30 * (j // 12)], F32)
        k = put(j % 2, 1, j, c, base, score=0.95 - 0.005 * j)
        surv[1].append(k)
        if j % 3 == 1:
            put(1 - j % 2, 1, j, c, base + rng.uniform(-0.5, 0.5, 4).astype(F32))
            if j % 2:
                put(1 - j % 2, 1, (j + 140) % P, c, base + rng.uniform(-0.5, 0.5, 4).astype(F32))
    # image 2: live, none kept
    for r in range(0, P, 3):
        put(r % 2, 2, r, 1, BIG + rng.uniform(-2, 2, 4).astype(F32))
    keep = np.zeros(n, np.int64)
    order = surv[0] + surv[1]
    keep[:len(order)] = order
    assert len(set(order)) == len(order) and all(grp[k] == (0 if k in surv[0] else 1) for k in order)
    return boxes, scores, labels, grp, keep, len(order), dict(big=k_big, lone=lone, k8=k8, k5=k5)


def _run_vote(dev, inp, C, D, vote_iou, ratios=None, nk=None):
    from mx_det import ops
    boxes, scores, labels, grp, keep, nk0, _ = inp
    d = [torch.from_numpy(a).to(dev) for a in (keep, boxes, scores, labels, grp)]
    num_keep = torch.tensor([nk0 if nk is None else nk], dtype=torch.int64, device=dev)
    return ops.detection_select_vote(d[0], num_keep, d[1], d[2], d[3], d[4], VOTE["V"], VOTE["N"], VOTE["P"], C, D,
                                     vote_iou, None if ratios is None else torch.from_numpy(ratios).to(dev))


RATIOS = np.array([[1.5, 0.75], [0.3333333, 2.25], [1.2345, 0.987]], F32)


@pytest.mark.parametrize("with_ratios", [True, False])
@pytest.mark.parametrize("D", [1, 100])
@pytest.mark.parametrize("C", [2, 7, 91])
def test_select_vote(dev, C, D, with_ratios):
    inp = _vote_inputs(C)
    boxes, scores, labels, grp, keep, nk, marks = inp
    V, N, P = VOTE["V"], VOTE["N"], VOTE["P"]
    ratios = RATIOS if with_ratios else None
    ref = T.select_vote(keep, nk, boxes, scores, labels, grp, V, N, P, C, D, 0.8, ratios)
    plain = T.select_vote(keep, nk, boxes, scores, labels, grp, V, N, P, C, D, 2.0, ratios)
    voters = ref[4]
    # the reference sees what the input was built for
    assert ref[3].tolist() == [min(len(marks["lone"]) + 3, D), min(131, D), 0]
    assert voters[0][0] > 128 and voters[1][0] == 1  # several ballot rounds; a lone voter
    assert not _same(ref[0][0, 0], plain[0][0, 0]) and _same(ref[0][1, 0], plain[0][1, 0])
    if D == 100:
        assert voters[0][1:6] == [1] * 5  # LONE0's perfect copies (other class / image / dead) do not vote
        assert voters[0][6:8] == [2, 1]   # IoU float32(0.8) votes at 0.8, IoU 0.5 does not
        assert _same(ref[0][0, 1:6], plain[0][0, 1:6]) and not _same(ref[0][0, 6], plain[0][0, 6])
        assert sorted(set(voters[1])) == [1, 2, 3]
        assert (ref[0][1] != plain[0][1]).any()
    got = _run_vote(dev, inp, C, D, 0.8, ratios)
    _assert_outputs(got, ref)
    ob = _np(got[0])
    assert not ob[2].any() and not _np(got[1])[2].any() and not _np(got[2])[2].any()  # the image with no survivor


@pytest.mark.parametrize("vote_iou,want", [(0.8, [2, 1]), (float(np.nextafter(F32(0.8), F32(1))), [1, 1]),
                                           (0.5, [2, 2]), (float(np.nextafter(F32(0.5), F32(1))), [2, 1])])
def test_select_vote_thresholds(dev, vote_iou, want):
    """Both exact pairs on both sides of the threshold: the voter changes the box exactly when its f32
    IoU is >= the f32 threshold."""
    C, D = 7, 100
    inp = _vote_inputs(C)
    boxes, scores, labels, grp, keep, nk, marks = inp
    ref = T.select_vote(keep, nk, boxes, scores, labels, grp, VOTE["V"], VOTE["N"], VOTE["P"], C, D, vote_iou)
    assert ref[4][0][6:8] == want
    got = _run_vote(dev, inp, C, D, vote_iou)
    _assert_outputs(got, ref)
    ob = _np(got[0])[0]
    assert _same(ob[6], boxes[marks["k8"]]) == (want[0] == 1) and _same(ob[7], boxes[marks["k5"]]) == (want[1] == 1)


@pytest.mark.parametrize("vote_iou", [2.0, float("nan")])
@pytest.mark.parametrize("with_ratios", [True, False])
def test_voting_off_is_detection_select(dev, vote_iou, with_ratios):
    from mx_det import ops
    C, D = 7, 100
    inp = _vote_inputs(C)
    boxes, scores, labels, grp, keep, nk, _ = inp
    ratios = RATIOS if with_ratios else None
    got = _run_vote(dev, inp, C, D, vote_iou, ratios)
    d = [torch.from_numpy(a).to(dev) for a in (keep, boxes, scores, labels, grp)]
    want = ops.detection_select(d[0], torch.tensor([nk], dtype=torch.int64, device=dev), d[1], d[2], d[3], d[4],
                                VOTE["N"], D, None if ratios is None else torch.from_numpy(ratios).to(dev))
    assert int(want[3].sum()) > D
    for a, b in zip(got, want):
        assert _same(a, b)


def test_failed_nms_and_empty_input(dev):
    from mx_det import ops
    C, D = 7, 100
    inp = _vote_inputs(C)
    ob, osc, ol, counts = _run_vote(dev, inp, C, D, 0.8, RATIOS, nk=-1)  # a failed NMS: never an empty result
    assert counts.tolist() == [-1] * VOTE["N"]
    assert not _np(ob).any() and not _np(osc).any() and not _np(ol).any()
    ob, osc, ol, counts = _run_vote(dev, inp, C, D, 0.8, nk=0)
    assert counts.tolist() == [0] * VOTE["N"] and not _np(ob).any()
    # n == 0: no rows at all
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    N, V = 2, 2
    hw = torch.ones(N, 2, device=dev)
    b, g = ops.detection_views_fold(z(0, 4), z(0, dt=torch.int32), hw, V, N, 0, C, (False, True))
    assert b.shape == (0, 4) and g.shape == (0,)
    ob, osc, ol, counts = ops.detection_select_vote(z(0, dt=torch.int64), z(1, dt=torch.int64), z(0, 4), z(0),
                                                    z(0, dt=torch.int64), z(0, dt=torch.int32), V, N, 0, C, 5, 0.8)
    assert counts.tolist() == [0, 0] and ob.shape == (N, 5, 4) and not _np(ob).any() and not _np(ol).any()
    ob, osc, ol, counts = ops.detections_postprocess_views(z(0, C), z(0, 4 * C), z(0, 4), z(0, dt=torch.int32), hw, N, V,
                                                           (False, True), THR, NMS_THR, 5, 0.8)
    assert counts.tolist() == [0, 0] and not _np(ob).any() and not _np(osc).any()


# ------------------------------------------------------------------------------------------ 3. composed
COMPOSED = dict(N=3, V=2, per=300, C=7, D=100, boosted=60)
HW = torch.tensor([[320., 400.], [300., 380.], [320., 400.]])
RATIOS3 = torch.tensor([[1.5, 0.75], [1.0, 1.0], [2.0, 1.25]])
FLIPS = (False, True)


def _views_inputs(seed):
    """The clustered rows of test_gpu_detections' composed inputs in two views: view 1's RoIs sit at the
    mirrored cluster centres with their own jitter, logits and regression, so after the fold both views
    crowd the same 40 clusters. Image 0: most candidates live in both views (per-class NMS); image 1:
    background wins except in 60 rows per view (coordinate trick); image 2: nothing over the score
    threshold. Some rows are exact copies of another (tied scores)."""
    N, V, per, C = COMPOSED["N"], COMPOSED["V"], COMPOSED["per"], COMPOSED["C"]
    g = torch.Generator().manual_seed(seed)
    R = V * N * per
    cell = torch.arange(40)
    cx, cy = (cell % 8) * 45.0 + 30, (cell // 8) * 56.0 + 34
    which = torch.randint(0, 40, (R,), generator=g)
    block = torch.arange(V * N).repeat_interleave(per)
    view, image = block // N, block % N
    x = torch.where(view == 1, HW[image, 1] - cx[which], cx[which])
    ctr = torch.stack([x, cy[which]], 1) + torch.randn(R, 2, generator=g) * 1.5
    wh = torch.tensor([36., 44.]) + torch.randn(R, 2, generator=g) * 2
    rois = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    reg = torch.randn(R, 4 * C, generator=g) * 0.15
    logits = torch.randn(R, C, generator=g) * 0.5
    for v in range(V):
        b1, b2 = (v * N + 1) * per, (v * N + 2) * per
        logits[b1:b1 + per, 0] += 4.0
        rows = b1 + torch.arange(COMPOSED["boosted"])
        logits[rows, torch.randint(1, C, (COMPOSED["boosted"],), generator=g)] += 3.5
        logits[b2:b2 + per, 0] += 12.0
    for base in (4, per + 7, N * per + 30):  # exact duplicates
        logits[base + 1:base + 6], reg[base + 1:base + 6], rois[base + 1:base + 6] = logits[base], reg[base], rois[base]
    for base in (40, per + 40):  # the same logits on other boxes: tied scores that both survive, near the top
        logits[base, 2] += 3.0
        logits[base + 1:base + 12] = logits[base]
    img = block.to(torch.int32)
    for b in range(V * N):  # padded rows, dead
        img[(b + 1) * per - 7:(b + 1) * per] = V * N
    return logits, reg, rois, img, HW.clone(), RATIOS3.clone()


def _reference_chain(logits, reg, rois, img, hw, ratios, vote_iou=0.8):
    """ops.detection_candidates -> numpy fold -> the CPU oracle's batched_nms per image -> numpy vote and
    select. -> (select_vote's tuple, live per image after the fold, survivors per image)."""
    from mx_det import ops
    from oracle.cpu_backend import CpuBackend
    be = CpuBackend()
    N, V, C, D = COMPOSED["N"], COMPOSED["V"], COMPOSED["C"], COMPOSED["D"]
    P = logits.shape[0] // (V * N)
    scores, boxes, labels, grp = ops.detection_candidates(logits, reg, rois, img, hw.repeat(V, 1), V * N, THR)
    scores, labels = _np(scores), _np(labels)
    fb, fg = T.fold(_np(boxes), _np(grp), _np(hw), V, N, P, C, FLIPS)
    keep, live, surv = [], [], []
    for i in range(N):
        idx = np.flatnonzero(fg == i)
        live.append(int(idx.size))
        k = _np(be.batched_nms(torch.from_numpy(fb[idx]), torch.from_numpy(scores[idx]), torch.from_numpy(labels[idx]),
                               NMS_THR)) if idx.size else np.zeros(0, np.int64)
        surv.append(int(k.size))
        keep.append(idx[k])
    keep = np.concatenate(keep).astype(np.int64)
    ref = T.select_vote(keep, keep.size, fb, scores, labels, fg, V, N, P, C, D, vote_iou, _np(ratios))
    plain = T.select_vote(keep, keep.size, fb, scores, labels, fg, V, N, P, C, D, 2.0, _np(ratios))
    return ref, plain, live, surv


def _chain(t):
    from mx_det import ops
    logits, reg, rois, img, hw, ratios = t
    return ops.detections_postprocess_views(logits, reg, rois, img, hw, COMPOSED["N"], COMPOSED["V"], FLIPS, THR, NMS_THR,
                                            COMPOSED["D"], 0.8, ratios=ratios, max_seg=COMPOSED["per"])


def test_composed_path_bitwise(dev):
    from mx_det import ops
    D = COMPOSED["D"]
    t = [x.to(dev) for x in _views_inputs(1)]
    ref, plain, live, surv = _reference_chain(*t)
    print("live per image after the fold", live, "survivors", surv, "max voters", max(ref[4][0]))
    assert live[0] > 1000 and 1 <= live[1] <= 1000 and live[2] == 0  # both dispatch regimes and an empty image
    assert surv[0] > D and 0 < surv[1] < live[1]
    assert max(ref[4][0]) >= 2 and max(ref[4][1]) >= 2
    assert (ref[0][0] != plain[0][0]).any() and (ref[0][1] != plain[0][1]).any()  # voting moved boxes
    s = ref[1][0]
    assert (s[1:] == s[:-1]).any()  # tied scores among the returned detections: the order by index is on trial
    got = _chain(t)
    _assert_outputs(got, ref)
    # the default segment bound gives the same result
    logits, reg, rois, img, hw, ratios = t
    got2 = ops.detections_postprocess_views(logits, reg, rois, img, hw, COMPOSED["N"], COMPOSED["V"], FLIPS, THR, NMS_THR,
                                            D, 0.8, ratios=ratios)
    assert all(_same(a, b) for a, b in zip(got, got2))


def test_graph_replay_matches_eager_and_reference(dev):
    """The composed path holds no host synchronisation and no per-call state: captured once, replayed on
    new contents of its static inputs, it gives the eager result and the reference bit for bit. The loop
    is the one of test_gpu_detections' graph test (replay, the eager chain behind it on the same stream,
    one synchronise); the reference, whose CPU work waits for the device, comes after the last replay."""
    static = [t.to(dev) for t in _views_inputs(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream
        _chain(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _chain(static)
    for seed in (3, 4):
        fresh = [t.to(dev) for t in _views_inputs(seed)]
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        eager = _chain(fresh)
        torch.cuda.synchronize()
        assert int(eager[3].sum()) > 0
        for a, b in zip(out, eager):
            assert _same(a, b), (seed, out[3].tolist(), eager[3].tolist())
    _assert_outputs(out, _reference_chain(*fresh)[0])


# ------------------------------------------------------------------------------------------ 4. model
ORIGINAL = ((180, 240), (200, 210))


class _Recorder:
    """The HIP backend with the two fused tails recorded."""

    def __init__(self, be):
        self._be, self.views, self.plain = be, [], []

    def __getattr__(self, k):
        return getattr(self._be, k)

    def detections_postprocess_views(self, *a, **kw):
        self.views.append((a, kw))
        return self._be.detections_postprocess_views(*a, **kw)

    def detections_postprocess(self, *a, **kw):
        self.plain.append((a, kw))
        return self._be.detections_postprocess(*a, **kw)


@pytest.fixture(scope="module")
def model(dev):
    from mx_det import frcnn
    from mx_det.backend import HipBackend
    torch.manual_seed(0)
    m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    m.roi_heads.box_predictor = frcnn.FastRCNNPredictor(m.roi_heads.box_predictor.cls_score.in_features, 7)
    m.transform.min_size, m.transform.max_size = 256, 512  # a small canvas: the tail is what is tested
    m.rpn._pre = dict(training=2000, testing=200)  # under 1000 candidates per image: padded proposal rows
    m = m.to(dev).eval()
    rec = _Recorder(HipBackend("f32"))
    m.set_backend(rec)
    g = torch.Generator().manual_seed(5)
    images = [torch.randint(0, 256, s + (3,), dtype=torch.uint8, generator=g).to(dev) for s in ORIGINAL]
    return m, rec, images


@pytest.fixture
def fresh(model):
    """The module's model with tta off and an empty record, before and after the test."""
    m, rec, images = model
    m.tta = None
    rec.views.clear()
    rec.plain.clear()
    yield m, rec, images
    m.tta = None
    m.set_backend(rec).eval()


def _dicts_equal(a, b):
    return len(a) == len(b) and all(list(x) == list(y) and all(_same(x[k], y[k]) for k in x) for x, y in zip(a, b))


def test_model_tta(fresh, monkeypatch):
    from mx_det import ops
    from mx_det.tta import TTA
    from oracle.cpu_backend import CpuBackend
    m, rec, images = fresh
    monkeypatch.delenv("MX_FUSED_DETECTIONS", raising=False)
    assert m.tta is None and m.roi_heads.fused_detections is False  # the fused tail is used whatever this says
    m.tta = TTA()
    seen = {}
    inner_fp, inner_tf = m.rpn.filter_proposals_padded, m.transform.forward

    def padded(*a, **kw):
        seen["proposals"] = inner_fp(*a, **kw)
        return seen["proposals"]

    def transform(imgs, targets, be):
        seen["images"] = imgs
        out = inner_tf(imgs, targets, be)
        seen["sizes"] = list(out[0].image_sizes)
        return out

    monkeypatch.setattr(m.rpn, "filter_proposals_padded", padded)
    monkeypatch.setattr(m.transform, "forward", transform)
    with torch.no_grad():
        out = m(images)
    assert len(rec.views) == 1 and not rec.plain
    (logits, reg, rois, img, hw, N, V, flips, thr, nms_thr, D, vote_iou), kw = rec.views[0]
    C = logits.shape[1]
    assert (N, V, tuple(flips), C, D, thr, nms_thr, vote_iou) == (2, 2, (False, True), 7,
                                                                  m.roi_heads.detections_per_img, 0.05, 0.5, 0.8)
    # the image list: the originals, then their mirrors along W
    assert len(seen["images"]) == V * N
    for i in range(N):
        assert torch.equal(seen["images"][i], images[i]) and torch.equal(seen["images"][N + i], images[i].flip(1))
    assert seen["sizes"][:N] == seen["sizes"][N:]
    # V * N blocks of post padded rows, view-major, dead exactly where the RPN's validity mask is False
    pb, _, valid = seen["proposals"]
    post = valid.shape[1]
    assert pb.shape == (V * N, post, 4) and logits.shape[0] == V * N * post and torch.equal(rois, pb.reshape(-1, 4))
    bi = torch.arange(V * N, dtype=torch.int32, device=img.device).repeat_interleave(post)
    assert torch.equal(img, torch.where(valid.reshape(-1), bi, V * N))
    assert valid.any(1).all() and kw["max_seg"] == post
    # hw and ratios belong to the N originals
    import math
    sizes = []
    for h, w in ORIGINAL:  # F.interpolate(recompute_scale_factor=True): floor(in * scale) in double
        sc = min(256 / min(h, w), 512 / max(h, w))
        sizes.append((math.floor(h * sc), math.floor(w * sc)))
    assert hw.cpu().tolist() == [[float(h), float(w)] for h, w in sizes]
    want = torch.tensor([[torch.tensor(o, dtype=torch.float32) / torch.tensor(s, dtype=torch.float32)
                          for o, s in zip(os_, ss)] for os_, ss in zip(ORIGINAL, sizes)])
    assert _same(kw["ratios"], want)

    # the restated chain on the recorded inputs
    scores, boxes, labels, grp = ops.detection_candidates(logits, reg, rois, img, hw.repeat(V, 1), V * N, thr)
    scores, labels = _np(scores), _np(labels)
    fb, fg = T.fold(_np(boxes), _np(grp), _np(hw), V, N, post, C, flips)
    be = CpuBackend()
    keep = []
    for i in range(N):
        idx = np.flatnonzero(fg == i)
        k = _np(be.batched_nms(torch.from_numpy(fb[idx]), torch.from_numpy(scores[idx]), torch.from_numpy(labels[idx]),
                               nms_thr))
        keep.append(idx[k])
    keep = np.concatenate(keep).astype(np.int64)
    rb, rs, rl, rc, voters = T.select_vote(keep, keep.size, fb, scores, labels, fg, V, N, post, C, D, vote_iou,
                                           _np(kw["ratios"]))
    print("model: survivors", rc.tolist(), "max voters", [max(v) for v in voters])
    assert min(rc) > 0 and max(max(v) for v in voters) >= 2
    assert isinstance(out, list) and len(out) == N
    for i, o in enumerate(out):
        assert list(o) == ["boxes", "labels", "scores"]
        c = int(rc[i])
        assert o["boxes"].shape == (c, 4) and o["labels"].shape == (c,) and o["scores"].shape == (c,) and c <= D
        assert _same(o["boxes"], rb[i, :c]) and _same(o["scores"], rs[i, :c]) and _same(o["labels"], rl[i, :c])
        s, b = _np(o["scores"]), _np(o["boxes"]).astype(np.float64)
        assert (s[1:] <= s[:-1]).all()
        # inside the original image: a resized coordinate <= w times f32(W / w) is at most W (1 + 2^-24)^2
        H, W = ORIGINAL[i]
        slack = 1 + 2.0 ** -23
        assert (b >= 0).all() and (b[:, [0, 2]] <= W * slack).all() and (b[:, [1, 3]] <= H * slack).all()
        assert (b[:, 2] >= b[:, 0]).all() and (b[:, 3] >= b[:, 1]).all()


def test_model_input_forms(fresh):
    """Batched uint8 [B, H, W, 3], uint8 HWC lists and float CHW lists are all mirrored along W."""
    from mx_det.tta import TTA
    m, rec, _ = fresh
    g = torch.Generator().manual_seed(9)
    dev = next(m.parameters()).device
    batch = torch.randint(0, 256, (2, 160, 224, 3), dtype=torch.uint8, generator=g).to(dev)
    m.tta = TTA()
    seen = []
    inner = m.transform.forward
    m.transform.forward = lambda imgs, t, be: (seen.append(imgs), inner(imgs, t, be))[1]
    try:
        with torch.no_grad():
            a = m(batch)
            b = m(list(batch))
            c = m([im.permute(2, 0, 1).float() / 255 for im in batch])
    finally:
        del m.transform.forward
    assert torch.is_tensor(seen[0]) and torch.equal(seen[0], torch.cat([batch, batch.flip(2)]))
    assert all(torch.equal(seen[1][2 + i], batch[i].flip(1)) for i in range(2))
    assert all(seen[2][2 + i].shape == (3, 160, 224) and torch.equal(seen[2][2 + i], seen[2][i].flip(2)) for i in range(2))
    assert len(rec.views) == 3 and len(a) == len(b) == len(c) == 2
    assert _dicts_equal(a, b)
    assert all(list(o) == ["boxes", "labels", "scores"] and o["boxes"].shape[0] == o["scores"].shape[0] for o in c)


def test_model_tta_off_and_guards(fresh, monkeypatch):
    from mx_det.adapt import BNAdapter
    from mx_det.tta import TTA
    m, rec, images = fresh
    monkeypatch.delenv("MX_FUSED_DETECTIONS", raising=False)
    with torch.no_grad():
        monkeypatch.setattr(m.roi_heads, "fused_detections", True)
        fused = m(images)
        assert len(rec.plain) == 1 and not rec.views
        m.tta = TTA()
        voted = m(images)
        assert len(rec.views) == 1 and len(rec.plain) == 1
        m.tta = None  # off again: the fused path's output, bit for bit
        again = m(images)
        assert len(rec.plain) == 2 and len(rec.views) == 1 and _dicts_equal(fused, again)
        assert not _dicts_equal(fused, voted)
        monkeypatch.setattr(m.roi_heads, "fused_detections", False)
        torch_tail = m(images)  # the torch tail: neither fused entry is called
        assert len(rec.plain) == 2 and len(rec.views) == 1
        assert len(torch_tail) == 2 and all(list(o) == ["boxes", "labels", "scores"] for o in torch_tail)
        # training mode ignores tta
        m.tta = TTA()
        assert m.train()._tta_views(rec) is None
        m.eval()
        # an enabled BNAdapter beside tta is refused; disabled again, tta runs
        with BNAdapter(m, mode="batch", prior=16):
            with pytest.raises(ValueError, match="BNAdapter"):
                m(images)
        assert len(rec.views) == 1
        m(images)
        assert len(rec.views) == 2

    class _NoViews:
        name = "hip"

        def __getattr__(self, k):
            if k == "detections_postprocess_views":
                raise AttributeError(k)
            return getattr(rec, k)

    with pytest.raises(NotImplementedError, match="test-time augmentation"):
        m.set_backend(_NoViews())(images)
    m.set_backend(rec)
