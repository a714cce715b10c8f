"""Device COCOeval (mx_coco_match / mx_coco_accumulate behind mx_det.coco_device.DeviceCOCOeval)
against the host evaluator mx_det.coco.COCOeval. Every operation of the kernels is one IEEE f64
operation in the host code's order, so the bar is np.array_equal: bitwise, no tolerance."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from mx_det.coco import COCO, COCOeval

pytestmark = pytest.mark.gpu


def _coco(anns, img_ids, cat_ids):
    return COCO({"images": [{"id": i} for i in img_ids], "annotations": anns,
                 "categories": [{"id": c, "name": f"c{c}"} for c in cat_ids]})


def _ann(aid, img, cat, xywh, crowd=0):
    return {"id": aid, "image_id": img, "category_id": cat, "bbox": [float(v) for v in xywh],
            "area": float(xywh[2]) * float(xywh[3]), "iscrowd": crowd}


def _host_results(dets):
    """Result dicts as engine.evaluate builds them from the model's f32 outputs."""
    res = []
    for img, boxes, scores, labels in dets:
        for (x1, y1, x2, y2), sc, lb in zip(boxes.tolist(), scores.tolist(), labels.tolist()):
            res.append({"image_id": img, "category_id": int(lb), "bbox": [x1, y1, x2 - x1, y2 - y1],
                        "score": float(sc)})
    return res


def _host_eval(gt, dets):
    ev = COCOeval(gt, gt.loadRes(_host_results(dets)), "bbox")
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


def _device_eval(gt, dets, dev):
    import torch
    from mx_det.coco_device import DeviceCOCOeval
    ev = DeviceCOCOeval(gt, dev)
    for img, boxes, scores, labels in dets:
        ev.add(img, torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev))
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


def _det(img, boxes_xyxy, scores, labels):
    return (img, np.asarray(boxes_xyxy, np.float32).reshape(-1, 4), np.asarray(scores, np.float32).reshape(-1),
            np.asarray(labels, np.int64).reshape(-1))


def _assert_same_eval(hev, dev_ev):
    assert dev_ev.eval["counts"] == hev.eval["counts"]
    for name in ("precision", "recall", "scores"):
        h, d = hev.eval[name], dev_ev.eval[name]
        assert d.dtype == h.dtype and d.shape == h.shape, name
        assert np.array_equal(h, d), (name, int(np.sum(h != d)))
    assert np.asarray(dev_ev.stats).dtype == np.asarray(hev.stats).dtype
    assert np.array_equal(np.asarray(hev.stats), np.asarray(dev_ev.stats))


def _assert_same_matches(hev, dev_ev):
    """dtMatches, dtIgnore, gtIgnore (and the detection order) of every non-None evalImgs entry."""
    p = hev.params
    m = dev_ev.matches()
    seg = {(int(k), int(i)): s for s, (k, i) in enumerate(zip(m["seg_cat"], m["seg_img"]))}
    n_entries, I = 0, len(p.imgIds)
    for k in range(len(p.catIds)):
        for a in range(len(p.areaRng)):
            for i in range(I):
                e = hev.evalImgs[(k * len(p.areaRng) + a) * I + i]
                if e is None:
                    assert (k, i) not in seg
                    continue
                n_entries += 1
                s = seg[k, i]
                d0, d1 = m["dt_off"][s], m["dt_off"][s + 1]
                g0, g1 = m["gt_off"][s], m["gt_off"][s + 1]
                assert np.array_equal(np.asarray(e["dtScores"], np.float64), m["dt_score"][d0:d1]), (k, a, i)
                assert np.array_equal(e["dtMatches"], m["dtm"][a, :, d0:d1].astype(np.float64)), (k, a, i)
                assert np.array_equal(e["dtIgnore"].astype(np.uint8), m["dt_ig"][a, :, d0:d1]), (k, a, i)
                # host GTs are in visiting order (non-ignored first); the device keeps annotation order
                host_ig = dict(zip(e["gtIds"], np.asarray(e["gtIgnore"]).tolist()))
                dev_ig = dict(zip(m["gt_id"][g0:g1].tolist(), m["gt_ig"][a, g0:g1].tolist()))
                assert len(e["gtIds"]) == g1 - g0 and host_ig == dev_ig, (k, a, i)
    assert n_entries == len(seg) * len(p.areaRng)
    return n_entries


# ---- 1. the hand-computable cases of tests/test_coco_eval.py ------------------------------------
def _gt_simple(boxes, cats=None, crowd=None):
    anns = [_ann(i + 1, 1, (cats or [1] * len(boxes))[i], b, (crowd or [0] * len(boxes))[i])
            for i, b in enumerate(boxes)]
    return _coco(anns, [1], (1, 2))


def _both(gt, dets, dev):
    hev, dev_ev = _host_eval(gt, dets), _device_eval(gt, dets, dev)
    _assert_same_eval(hev, dev_ev)
    _assert_same_matches(hev, dev_ev)
    return dev_ev


def test_perfect_detections(dev):
    gt = _gt_simple([[10, 10, 50, 40], [100, 80, 30, 30]], cats=[1, 2])
    ev = _both(gt, [_det(1, [[10, 10, 60, 50], [100, 80, 130, 110]], [0.9, 0.8], [1, 2])], dev)
    assert abs(ev.stats[0] - 1.0) < 1e-12 and abs(ev.stats[1] - 1.0) < 1e-12


def test_false_positive_ranked_first_halves_ap(dev):
    gt = _gt_simple([[10, 10, 50, 40]])
    ev = _both(gt, [_det(1, [[300, 300, 320, 320], [10, 10, 60, 50]], [0.95, 0.5], [1, 1])], dev)
    assert abs(ev.stats[1] - 0.5) < 1e-12


def test_partial_iou_thresholds(dev):
    gt = _gt_simple([[0, 0, 10, 10]])
    ev = _both(gt, [_det(1, [[0, 0, 10, 6.2]], [0.9], [1])], dev)  # IoU 0.62 (f32 6.2: 0.6199999...)
    assert abs(ev.stats[0] - 0.3) < 1e-12 and abs(ev.stats[1] - 1.0) < 1e-12
    ap50 = ev.eval["precision"][0, :, 0, 0, 2]
    assert abs(np.mean(ap50[ap50 > -1]) - 1.0) < 1e-12


def test_crowd_gt_is_ignored(dev):
    gt = _gt_simple([[0, 0, 100, 100], [200, 200, 20, 20]], crowd=[1, 0])
    ev = _both(gt, [_det(1, [[10, 10, 30, 30], [200, 200, 220, 220]], [0.9, 0.5], [1, 1])], dev)
    assert abs(ev.stats[1] - 1.0) < 1e-12


# ---- 2. one seeded adversarial set: 7 images, 3 categories, one call ----------------------------
def _adversarial():
    """Category 1 carries the matching cases; category 2 has detections but no GT anywhere (-1);
    category 3 has GT but no detections (precision 0). Image 5 has neither GT nor detections."""
    rng = np.random.default_rng(20240607)
    anns, dets, next_id = [], [], [1]

    def add_gt(img, cat, xywh, crowd=0, aid=None):
        if aid is None:
            aid = next_id[0]
            next_id[0] += 1
        anns.append(_ann(aid, img, cat, xywh, crowd))

    def random_image(img, n_gt, n_dt):
        # half-pixel grid: equal boxes and exact IoU ties occur; two-decimal scores: tied scores
        xy = np.round(rng.uniform(0, 900, (n_gt, 2)) * 2) / 2
        wh = np.round(rng.uniform(8, 140, (n_gt, 2)) * 2) / 2
        gtb = np.concatenate([xy, wh], 1)
        for j, b in enumerate(gtb):
            add_gt(img, 1, b, crowd=int(n_gt >= 5 and j % 11 == 3))
        boxes = []
        for j in range(n_dt):
            if n_gt and j % 4 != 3:  # near a GT (several detections per GT), else anywhere
                b = gtb[rng.integers(n_gt)].copy()
                b += np.round(rng.normal(0, [3, 3, 4, 4]) * 2) / 2 * (rng.random() < 0.8)
                b[2:] = np.maximum(b[2:], 2)
            else:
                b = np.concatenate([np.round(rng.uniform(0, 900, 2)), np.round(rng.uniform(8, 140, 2))])
            boxes.append([b[0], b[1], b[0] + b[2], b[1] + b[3]])
        if n_dt:
            dets.append(_det(img, boxes, np.round(rng.random(n_dt), 2), np.ones(n_dt)))

    random_image(1, 5, 100)
    random_image(2, 70, 137)   # 137 > maxDets[-1]: truncated to the 100 best
    random_image(3, 130, 100)  # 70 and 130 GTs cross a 64-lane wave
    random_image(4, 1, 1)
    # image 5: nothing. image 6: category-1 detections without GT, category-2 detections (no GT anywhere)
    dets.append(_det(6, [[10, 10, 50, 50], [20, 20, 80, 90], [300, 300, 332, 332]], [0.5, 0.5, 0.9], [1, 1, 1]))
    dets.append(_det(6, [[10, 10, 50, 50], [100, 100, 150, 150]], [0.7, 0.5], [2, 2]))
    dets.append(_det(1, [[0, 0, 40, 40]], [0.5], [2]))
    # image 7: hand-built cases, far apart from each other
    add_gt(7, 1, [0, 0, 200, 200], crowd=1)            # crowd with several detections inside it
    add_gt(7, 1, [20, 20, 40, 40])                     # and a plain GT inside the crowd region
    add_gt(7, 1, [1000, 0, 50, 50])                    # duplicated GT boxes: exact IoU ties
    add_gt(7, 1, [1000, 0, 50, 50])
    add_gt(7, 1, [1000, 0, 50, 50])
    add_gt(7, 1, [1500, 0, 32, 32])                    # areas exactly 32^2 and 96^2: range boundaries
    add_gt(7, 1, [1700, 0, 96, 96])
    add_gt(7, 1, [2000, 0, 10, 5])                     # IoU exactly 0.5 with [2000, 0, 10, 10]
    add_gt(7, 1, [2200, 0, 10, 5.4999])                # IoU just under 0.55 with [2200, 0, 10, 10]
    add_gt(7, 1, [2400, 0, 30, 30], aid=0)             # a GT whose id is 0: matched, read as unmatched
    add_gt(7, 1, [3000, 0, 40, 39])                    # stop rule: in "small" this one is ignored (IoU .975)
    add_gt(7, 1, [3000, 0, 40, 24])                    # ... and this one is not (IoU .6): it takes the match
    add_gt(7, 3, [100, 100, 60, 60])                   # category 3: GT, never a detection
    add_gt(2, 3, [100, 100, 20, 20])
    dets.append(_det(7, [[10, 10, 50, 50], [100, 100, 150, 150], [60, 120, 100, 190], [20, 20, 60, 60],
                         [1000, 0, 1050, 50], [1000, 0, 1050, 50], [1000, 0, 1050, 50], [1000, 0, 1050, 50],
                         [1500, 0, 1532, 32], [1700, 0, 1796, 96], [1900, 0, 1932, 32], [1900, 100, 1996, 196],
                         [2000, 0, 2010, 10], [2200, 0, 2210, 10], [2400, 0, 2430, 30], [3000, 0, 3040, 40]],
                     [0.9, 0.9, 0.8, 0.7, 0.6, 0.6, 0.6, 0.6, 0.5, 0.5, 0.5, 0.5, 0.45, 0.45, 0.4, 0.3],
                     np.ones(16)))
    return _coco(anns, [1, 2, 3, 4, 5, 6, 7], (1, 2, 3)), dets


@pytest.fixture(scope="module")
def adversarial():
    gt, dets = _adversarial()
    return gt, dets, _host_eval(gt, dets)


def test_adversarial_set_is_what_it_claims(adversarial):
    """The set holds the cases it is there for (checked on the host evaluator's own records)."""
    gt, dets, hev = adversarial
    n_gt = {(i, c): 0 for i in range(1, 8) for c in (1, 2, 3)}
    for a in gt.dataset["annotations"]:
        n_gt[a["image_id"], a["category_id"]] += 1
    n_dt = {k: 0 for k in n_gt}
    for img, _, _, labels in dets:
        for lb in labels.tolist():
            n_dt[img, lb] += 1
    assert {0, 1, 5, 70, 130} <= set(n_gt.values()) and {0, 1, 100, 137} <= set(n_dt.values())
    assert all(n_gt[5, c] == 0 and n_dt[5, c] == 0 for c in (1, 2, 3))
    assert sum(n_gt[i, 2] for i in range(1, 8)) == 0 and sum(n_dt[i, 2] for i in range(1, 8)) > 0
    assert sum(n_dt[i, 3] for i in range(1, 8)) == 0 and sum(n_gt[i, 3] for i in range(1, 8)) > 0
    prec = hev.eval["precision"]
    assert np.all(prec[:, :, 1] == -1) and np.all(prec[:, :, 2, 0, 2] == 0)
    e = hev.evalImgs[(0 * 4 + 0) * 7 + 6]  # category 1, all areas, image 7
    dtm = {tuple(d): e["dtMatches"][:, j] for j, d in enumerate(
        [tuple(x["bbox"]) for x in hev.cocoDt.loadAnns(e["dtIds"])])}
    assert dtm[2000.0, 0.0, 10.0, 10.0][0] != 0          # IoU exactly 0.5 matches at t = 0.5
    assert np.all(dtm[2200.0, 0.0, 10.0, 10.0][1:] == 0)  # just under 0.55
    ig = {tuple(d): e["dtIgnore"][:, j] for j, d in enumerate(
        [tuple(x["bbox"]) for x in hev.cocoDt.loadAnns(e["dtIds"])])}
    assert np.all(ig[100.0, 100.0, 50.0, 50.0]) and np.all(ig[60.0, 120.0, 40.0, 70.0])  # inside the crowd
    ids = {a["id"]: a for a in gt.dataset["annotations"]}
    small = hev.evalImgs[(0 * 4 + 1) * 7 + 6]  # the stop rule, area range "small"
    j = [tuple(x["bbox"]) for x in hev.cocoDt.loadAnns(small["dtIds"])].index((3000.0, 0.0, 40.0, 40.0))
    assert ids[int(small["dtMatches"][0, j])]["bbox"] == [3000.0, 0.0, 40.0, 24.0] and not small["dtIgnore"][0, j]
    assert ids[int(small["dtMatches"][9, j])]["bbox"] == [3000.0, 0.0, 40.0, 39.0] and small["dtIgnore"][9, j]
    assert ids[int(e["dtMatches"][0, j])]["bbox"] == [3000.0, 0.0, 40.0, 39.0]


def test_adversarial_matches(adversarial, dev):
    gt, dets, hev = adversarial
    dev_ev = _device_eval(gt, dets, dev)
    # segments: category 1 on images 1-4, 6, 7; category 2 on images 1, 6; category 3 on images 2, 7
    assert _assert_same_matches(hev, dev_ev) == 4 * (6 + 2 + 2)
    _assert_same_eval(hev, dev_ev)


def test_adversarial_params_and_shapes(adversarial, dev):
    gt, dets, hev = adversarial
    dev_ev = _device_eval(gt, dets, dev)
    assert dev_ev.params.imgIds == hev.params.imgIds and dev_ev.params.catIds == hev.params.catIds
    assert dev_ev.eval["precision"].shape == (10, 101, 3, 4, 3) and dev_ev.eval["recall"].shape == (10, 3, 4, 3)
    assert dev_ev.eval["params"] is dev_ev.params and len(dev_ev.stats) == 12


def test_no_detections_at_all(dev):
    """GT only: every segment has an empty detection range (recall 0, precision 0)."""
    gt = _gt_simple([[10, 10, 50, 40], [100, 80, 30, 30]], cats=[1, 2])
    ev = _both(gt, [], dev)
    assert np.all(ev.eval["recall"][:, :, 0, :] == 0) and ev.stats[0] == 0


def test_no_ground_truth_at_all(dev):
    """Detections only: segments without GT, every output -1."""
    gt = _coco([], [1, 2], (1, 2))
    ev = _both(gt, [_det(2, [[0, 0, 10, 10], [5, 5, 40, 40]], [0.5, 0.25], [1, 2])], dev)
    assert np.all(ev.eval["precision"] == -1) and np.all(ev.eval["recall"] == -1) and ev.stats[0] == -1


def test_detections_outside_the_image_set_are_refused(dev):
    gt = _gt_simple([[0, 0, 10, 10]])
    with pytest.raises(AssertionError, match="Results do not correspond"):
        _device_eval(gt, [_det(99, [[0, 0, 10, 10]], [0.5], [1])], dev)


# ---- 3. engine.evaluate: device_eval on and off return the same dict ------------------------------
from _coco_eval_worker import stub_setup  # noqa: E402

def test_engine_evaluate_device_equals_host(tmp_path, dev, monkeypatch):
    from mx_det import coco, engine
    monkeypatch.delenv("MX_DEVICE_COCOEVAL", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    model, loader, ann_file = stub_setup(tmp_path, dev)
    host = engine.evaluate(model, loader, ann_file, dev, per_class=True, device_eval=False)
    assert set(host) == {"mAP50_95", "mAP50", "per_class_ap50"} and 0 < host["mAP50"] < 1

    def no_host_eval(self):
        raise AssertionError("the host evaluator ran")

    monkeypatch.setattr(coco.COCOeval, "evaluate", no_host_eval)
    assert engine.evaluate(model, loader, ann_file, dev, per_class=True, device_eval=True) == host
    monkeypatch.setenv("MX_DEVICE_COCOEVAL", "1")  # the switch the scripts reach it through
    assert engine.evaluate(model, loader, ann_file, dev, per_class=True) == host
    plain = engine.evaluate(model, loader, ann_file, dev)
    assert plain == {k: host[k] for k in ("mAP50_95", "mAP50")}
    monkeypatch.setenv("MX_DEVICE_COCOEVAL", "0")
    with pytest.raises(AssertionError, match="the host evaluator ran"):
        engine.evaluate(model, loader, ann_file, dev)


@pytest.mark.timeout(170)
def test_engine_evaluate_two_ranks(tmp_path, dev):
    """World 2 (tests/_coco_eval_worker.py): each rank evaluates its shard, the packed detections are
    combined across the ranks, rank 0 returns the one-process result and rank 1 None."""
    from mx_det import engine
    model, loader, ann_file = stub_setup(tmp_path, dev)
    single = engine.evaluate(model, loader, ann_file, dev, per_class=True, device_eval=False)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    env.pop("MX_DEVICE_COCOEVAL", None)
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(here, "_coco_eval_worker.py"),
           str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=160)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    assert [d["n_images"] for d in res] == [2, 1]
    assert res[0]["host"] == single and res[0]["device"] == single
    assert res[1]["host"] is None and res[1]["device"] is None
