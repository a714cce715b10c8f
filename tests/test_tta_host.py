"""Everything about flip test-time augmentation that needs no GPU: the MX_TTA parser and the TTA record,
the invariants of the numpy restatement the GPU tests compare against (tests/tta_ref.py), the argument
rejections of the two entries (they return before any HIP call) and the model's guards that fire before
any kernel."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as T  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------ parser
def test_parse_env_good_values():
    from mx_det import tta
    assert tta.parse_env("") is None and tta.parse_env(None) is None
    t = tta.parse_env("flip")
    assert t.views == ("identity", "hflip") and t.vote_iou == 0.8 and t.flips == (False, True)
    assert tta.parse_env("flip:0.65").vote_iou == 0.65
    assert tta.parse_env(" FLIP : 1 ").vote_iou == 1.0
    assert tta.parse_env("flip:").vote_iou == 0.8


@pytest.mark.parametrize("value,match", [("mirror", "only augmentation"), ("scale:0.5", "only augmentation"),
                                         ("flip:abc", "must be a number"), ("flip:0", r"\(0, 1\]"),
                                         ("flip:1.5", r"\(0, 1\]"), ("flip:nan", r"\(0, 1\]"),
                                         ("flip:-0.2", r"\(0, 1\]")])
def test_parse_env_bad_values(value, match):
    from mx_det import tta
    with pytest.raises(ValueError, match=match) as e:
        tta.parse_env(value)
    assert "MX_TTA" in str(e.value) and repr(value) in str(e.value)


def test_tta_record():
    from mx_det.tta import TTA
    t = TTA()
    assert t.views == ("identity", "hflip") and t.vote_iou == 0.8 and t.flips == (False, True)
    assert TTA(views=("identity",)).flips == (False,) and TTA(views="identity").views == ("identity",)
    for bad in (("hflip",), ("identity", "vflip"), (), ("identity", "identity"), ("hflip", "identity")):
        with pytest.raises(ValueError, match="views"):
            TTA(views=bad)
    for bad in (0.0, 1.01, float("nan"), -1):
        with pytest.raises(ValueError, match="vote_iou"):
            TTA(vote_iou=bad)


# ------------------------------------------------------------------------------------------ restatement
def _rand_boxes(rng, m, w=64.0, h=48.0):
    x = np.sort(rng.uniform(0, w, (m, 2)).astype(F32), 1)
    y = np.sort(rng.uniform(0, h, (m, 2)).astype(F32), 1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)


def test_a_lone_voter_returns_its_box_bitwise():
    rng = np.random.default_rng(0)
    boxes = _rand_boxes(rng, 500)
    scores = rng.uniform(1e-3, 1, 500).astype(F32)
    for k in range(500):
        hit = np.zeros(500, bool)
        hit[k] = True
        got = T.vote(boxes[k], boxes, scores, hit)
        assert got.dtype == F32 and got.tobytes() == boxes[k].tobytes()
    # no voter at all: the box itself
    assert T.vote(boxes[3], boxes, scores, np.zeros(500, bool)).tobytes() == boxes[3].tobytes()


def test_a_voted_coordinate_lies_within_the_voters_range():
    rng = np.random.default_rng(1)
    moved = 0
    for trial in range(200):
        m = int(rng.integers(2, 40))
        base = _rand_boxes(rng, 1)[0]
        boxes = (base + rng.normal(0, 0.7, (m, 4))).astype(F32)
        scores = rng.uniform(0.05, 1, m).astype(F32)
        hit = rng.random(m) < 0.7
        if not hit.any():
            continue
        got = T.vote(boxes[0], boxes, scores, hit)
        assert (got >= boxes[hit].min(0)).all() and (got <= boxes[hit].max(0)).all()
        moved += got.tobytes() != boxes[0].tobytes()
    assert moved > 100


def test_mirroring_twice_restores_integer_boxes():
    rng = np.random.default_rng(2)
    V, N, P, C = 2, 2, 6, 3
    n = V * N * P * (C - 1)
    hw = np.array([[30., 37.], [40., 53.]], F32)
    grp = np.repeat(np.arange(V * N, dtype=np.int32), P * (C - 1))
    img = grp % N
    wi = hw[img, 1].astype(np.int64)
    x = np.sort(np.stack([rng.integers(0, wi + 1), rng.integers(0, wi + 1)], 1), 1)
    boxes = np.stack([x[:, 0], rng.integers(0, 20, n), x[:, 1], rng.integers(20, 30, n)], 1).astype(F32)
    once, g1 = T.fold(boxes, grp, hw, V, N, P, C, (True, True))
    assert (g1 == img).all() and (once[:, 0] <= once[:, 2]).all() and (once[:, 0] >= 0).all()
    assert (once[:, 2] <= hw[img, 1]).all() and not np.array_equal(once, boxes)
    assert np.array_equal(once[:, [1, 3]], boxes[:, [1, 3]])
    # the folded groups are image indices: as blocks of a V = 1 fold they are live where image == block
    twice = once.copy()
    for b in range(V * N):
        sl = slice(b * P * (C - 1), (b + 1) * P * (C - 1))
        i = b % N
        back, _ = T.fold(once[sl], np.zeros(P * (C - 1), np.int32), hw[i:i + 1], 1, 1, P, C, (True,))
        twice[sl] = back
    assert twice.tobytes() == boxes.tobytes()
    # an unflipped view keeps its boxes; a dead slot keeps its box and gets group N
    grp2 = grp.copy()
    grp2[::5] = V * N
    grp2[1] = 3  # a live value of another block
    keep, g2 = T.fold(boxes, grp2, hw, V, N, P, C, (False, True))
    half = n // 2
    assert keep[:half].tobytes() == boxes[:half].tobytes()
    dead = grp2 != grp
    assert (g2[dead] == N).all() and keep[dead].tobytes() == boxes[dead].tobytes() and (g2[~dead] == img[~dead]).all()


def test_hand_computed_dyadic_vote():
    boxes = np.array([[0, 0, 8, 8], [4, 0, 8, 8]], F32)
    scores = np.array([0.75, 0.25], F32)
    got = T.vote(boxes[0], boxes, scores, np.array([True, True]))
    assert got.tolist() == [1.0, 0.0, 8.0, 8.0]  # x1 = (0.75 * 0 + 0.25 * 4) / 1


def test_iou_is_exact_at_the_thresholds():
    a = np.array([0, 0, 4, 5], F32)
    b = np.array([[0, 0, 4, 4]], F32)
    v = T.iou(a, b)[0]
    assert v.dtype == F32 and v == F32(0.8)  # 16 / 20 rounds to float32(0.8)
    assert v >= F32(0.8) and not v >= np.nextafter(F32(0.8), F32(1))
    c = np.array([0, 0, 2, 2], F32)
    d = np.array([[0, 0, 2, 1]], F32)
    h = T.iou(c, d)[0]
    assert h == F32(0.5) and h >= F32(0.5) and not h >= np.nextafter(F32(0.5), F32(1))
    assert T.iou(a, a[None])[0] == F32(1.0)
    with np.errstate(all="ignore"):
        assert np.isnan(T.iou(a, np.array([[np.nan, 0, 4, 4]], F32))[0])
        assert not T.iou(a, np.array([[np.nan, 0, 4, 4]], F32))[0] >= F32(0.1)


def test_select_vote_restated_at_the_thresholds():
    """One image, one class, the two exact pairs in one view each: the voter set changes exactly at
    float32(0.8) / float32(0.5)."""
    V, N, P, C, D = 2, 1, 2, 2, 4
    boxes = np.array([[0, 0, 4, 5], [10, 10, 12, 12], [0, 0, 4, 4], [10, 10, 12, 11]], F32)
    scores = np.array([0.9, 0.8, 0.3, 0.2], F32)
    labels = np.ones(4, np.int64)
    grp = np.zeros(4, np.int32)
    keep = np.array([0, 1, 0, 0], np.int64)
    for thr, want in ((0.8, [2, 1]), (np.nextafter(F32(0.8), F32(1)), [1, 1]), (0.5, [2, 2]),
                      (np.nextafter(F32(0.5), F32(1)), [2, 1])):
        ob, osc, ol, counts, voters = T.select_vote(keep, 2, boxes, scores, labels, grp, V, N, P, C, D, thr)
        assert counts.tolist() == [2] and voters == [want], thr
        assert osc[0].tolist() == [F32(0.9), F32(0.8), 0, 0] and ol[0].tolist() == [1, 1, 0, 0]
    off = T.select_vote(keep, 2, boxes, scores, labels, grp, V, N, P, C, D, 2.0)
    nan = T.select_vote(keep, 2, boxes, scores, labels, grp, V, N, P, C, D, float("nan"))
    assert off[4] == [[None, None]] and off[0].tobytes() == nan[0].tobytes()
    assert off[0][0, :2].tobytes() == boxes[:2].tobytes()
    assert T.select_vote(keep, -1, boxes, scores, labels, grp, V, N, P, C, D, 0.8)[3].tolist() == [-1]


# ------------------------------------------------------------------------------------------ ABI
def _lib():
    from mx_det import _lib
    lib = _lib.load()
    lib.mx_last_error.restype = ctypes.c_char_p
    return lib


def test_entries_reject_bad_sizes_before_any_launch():
    lib = _lib()
    P = ctypes.c_void_p(64)  # never dereferenced: the checks return first
    flips = (ctypes.c_int32 * 2)(0, 1)
    V, N, Pr, C = 2, 2, 5, 7
    n = V * N * Pr * (C - 1)
    for bad in (dict(n=n + 1), dict(V=0), dict(V=65, n=65 * N * Pr * (C - 1)), dict(C=1, n=0), dict(N=0, n=0),
                dict(Pr=1 << 28, n=1 << 30)):
        a = dict(n=n, V=V, N=N, Pr=Pr, C=C)
        a.update(bad)
        rc = lib.mx_det_views_fold(P, P, P, a["n"], a["V"], a["N"], a["Pr"], a["C"], flips, P, P, None)
        assert rc == -1 and b"mx_det_views_fold: bad sizes" in lib.mx_last_error(), bad
        rc = lib.mx_det_select_vote(P, P, P, P, P, P, a["n"], a["V"], a["N"], a["Pr"], a["C"], 100, 0.8, None, P, P, P,
                                    P, None)
        assert rc == -1 and b"mx_det_select_vote: bad sizes" in lib.mx_last_error(), bad
    assert lib.mx_det_views_fold(P, P, P, n, V, N, Pr, C, None, P, P, None) == -1
    assert b"null flip flags" in lib.mx_last_error()
    assert lib.mx_det_views_fold(P, P, None, n, V, N, Pr, C, flips, P, P, None) == -1
    assert b"mx_det_views_fold: null pointer" in lib.mx_last_error()
    assert lib.mx_det_select_vote(P, P, P, P, P, P, n, V, N, Pr, C, 0, 0.8, None, P, P, P, P, None) == -1
    assert b"mx_det_select_vote: bad sizes" in lib.mx_last_error()
    assert lib.mx_det_select_vote(P, P, P, P, P, P, n, V, N, Pr, C, 100, 0.8, None, P, P, P, None, None) == -1
    assert b"mx_det_select_vote: null pointer" in lib.mx_last_error()
    # an empty fold launches nothing
    assert lib.mx_det_views_fold(None, None, None, 0, V, N, 0, C, flips, None, None, None) == 0


# ------------------------------------------------------------------------------------------ model guards
def test_model_guards_without_a_gpu():
    """tta is None by default; on a backend without the views tail an eval forward raises before any
    work, and a training forward ignores it."""
    import torch
    from mx_det import frcnn
    from mx_det.tta import TTA
    from oracle.cpu_backend import CpuBackend
    m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    assert m.tta is None
    be = CpuBackend()
    m.set_backend(be)
    m.eval()
    assert m._tta_views(be) is None
    m.tta = TTA()
    with pytest.raises(NotImplementedError, match="test-time augmentation"):
        m([torch.zeros(3, 64, 64)])
    m.train()
    assert m._tta_views(be) is None
