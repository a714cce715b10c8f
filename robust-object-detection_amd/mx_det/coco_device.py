"""COCOeval (bbox) on the device: mx_coco_match + mx_coco_accumulate (csrc/mx_coco.hip) behind the
interface of mx_det.coco.COCOeval.

DeviceCOCOeval takes detections as device tensors (add), sorts and segments them with torch's device
sorts, and runs pycocotools' evaluate / accumulate as two HIP entry points; `.params`, `.eval`
(precision, recall, scores, counts) and `.stats` have the shapes, dtypes and bit-identical values of
the host evaluator (tests/test_gpu_coco_device.py). The conversion of a detection follows the host
path of engine.evaluate + COCO.loadRes: f32 box and score -> f64, w = x2 - x1 and h = y2 - y1 in f64,
area = w * h. There is no host fallback: without the library the calls raise.
"""
import numpy as np
import torch

from . import _lib
from .coco import COCOeval, Params


class DeviceCOCOeval:
    """COCOeval(cocoGt, cocoDt, "bbox") with the detections given by add() instead of a result COCO.

    params.imgIds / catIds are fixed at construction (the GT arrays are built once, from every image
    and category of cocoGt); iouThrs, recThrs, maxDets and areaRng are read by evaluate / accumulate."""

    def __init__(self, cocoGt, device):
        self.cocoGt, self.device = cocoGt, torch.device(device)
        self.params = Params()
        self.params.imgIds = sorted(cocoGt.getImgIds())
        self.params.catIds = sorted(cocoGt.getCatIds())
        self.eval, self.stats = {}, []
        self._dets = []
        self._m = None  # evaluate()'s device arrays
        self._build_gt()

    # -- inputs ------------------------------------------------------------------------------------
    def _build_gt(self):
        p, dev = self.params, self.device
        img_ids = [int(i) for i in np.unique(p.imgIds)]
        cat_ids = [int(c) for c in np.unique(p.catIds)]
        self._I, self._K = len(img_ids), len(cat_ids)
        img_index = {v: i for i, v in enumerate(img_ids)}
        cat_index = {v: k for k, v in enumerate(cat_ids)}
        # the host evaluator's GT order: images ascending, each image's annotations in dataset order
        anns = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=img_ids, catIds=cat_ids))
        n = len(anns)
        key = np.array([cat_index[a["category_id"]] * self._I + img_index[a["image_id"]] for a in anns], np.int64)
        order = np.argsort(key, kind="stable")
        xywh = np.array([anns[i]["bbox"] for i in order], np.float64).reshape(n, 4)
        area = np.array([anns[i]["area"] for i in order], np.float64)
        crowd = np.array([1 if anns[i]["iscrowd"] else 0 for i in order], np.uint8)
        gid = np.array([anns[i]["id"] for i in order], np.int64)
        self._img_ids = torch.tensor(img_ids, dtype=torch.int64, device=dev)
        self._cat_ids = torch.tensor(cat_ids, dtype=torch.int64, device=dev)
        self._gt_key = torch.from_numpy(key[order]).to(dev)
        self._gt_xywh = torch.from_numpy(xywh).to(dev)
        self._gt_area = torch.from_numpy(area).to(dev)
        self._gt_crowd = torch.from_numpy(crowd).to(dev)
        self._gt_id = torch.from_numpy(gid).to(dev)

    def add(self, image_id, boxes_xyxy, scores, labels):
        """One image's detections (or several images': image_id a tensor with one id per detection),
        device tensors, in result order. Nothing is copied to the host."""
        dev = self.device
        n = int(boxes_xyxy.shape[0])
        if n == 0:
            return
        if torch.is_tensor(image_id):
            ids = image_id.to(dev, torch.int64, non_blocking=True).reshape(-1)
            ids = ids.expand(n) if ids.numel() == 1 else ids
        else:
            ids = torch.full((n,), int(image_id), dtype=torch.int64, device=dev)
        if ids.numel() != n or scores.numel() != n or labels.numel() != n:
            raise ValueError("add: image ids, boxes, scores and labels differ in length")
        self._dets.append((ids, boxes_xyxy.to(dev).float().reshape(n, 4), scores.to(dev).float().reshape(n),
                           labels.to(dev, torch.int64).reshape(n)))

    @staticmethod
    def _lookup(table, values):
        """Index of each value in the sorted table, and whether it is there."""
        if table.numel() == 0:
            return torch.zeros_like(values), torch.zeros_like(values, dtype=torch.bool)
        idx = torch.searchsorted(table, values).clamp_(max=table.numel() - 1)
        return idx, table[idx] == values

    # -- evaluate ----------------------------------------------------------------------------------
    def evaluate(self):
        p, dev = self.params, self.device
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        if len(p.imgIds) != self._I or len(p.catIds) != self._K:
            raise ValueError("DeviceCOCOeval: params.imgIds / catIds are fixed at construction")
        I, K = self._I, self._K
        f64, i64 = torch.float64, torch.int64
        if self._dets:
            ids = torch.cat([d[0] for d in self._dets])
            box = torch.cat([d[1] for d in self._dets]).to(f64)
            score = torch.cat([d[2] for d in self._dets]).to(f64)
            lab = torch.cat([d[3] for d in self._dets])
            ii, ok_img = self._lookup(self._img_ids, ids)
            if not bool(ok_img.all()):
                raise AssertionError("Results do not correspond to current coco set")
            ci, ok_cat = self._lookup(self._cat_ids, lab)  # other categories are not evaluated
            key = (ci * I + ii)[ok_cat]
            box, score = box[ok_cat], score[ok_cat]
            # (category, image, score descending), ties in result order: two stable sorts
            o1 = torch.sort(score, descending=True, stable=True).indices
            o2 = torch.sort(key[o1], stable=True).indices
            order = o1[o2]
            key, box, score = key[order], box[order], score[order]
            # at most maxDets[-1] per segment
            _, counts = torch.unique_consecutive(key, return_counts=True)
            starts = torch.cumsum(counts, 0) - counts
            rank = torch.arange(key.numel(), device=dev) - torch.repeat_interleave(starts, counts)
            keep = rank < int(p.maxDets[-1])
            key, box, score = key[keep], box[keep], score[keep]
        else:
            key = torch.empty(0, dtype=i64, device=dev)
            box = torch.empty((0, 4), dtype=f64, device=dev)
            score = torch.empty(0, dtype=f64, device=dev)
        w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        dt_xywh = torch.stack([box[:, 0], box[:, 1], w, h], 1).contiguous()
        dt_area = w * h
        ND, NG = int(key.numel()), int(self._gt_key.numel())
        seg = torch.unique(torch.cat([self._gt_key, key]))  # sorted: (category, image)
        S = int(seg.numel())
        end = torch.full((1,), K * I, dtype=i64, device=dev)
        bounds = torch.cat([seg, end])
        dt_off = torch.searchsorted(key, bounds).to(torch.int32)
        gt_off = torch.searchsorted(self._gt_key, bounds).to(torch.int32)
        cats = torch.arange(K + 1, dtype=i64, device=dev) * I
        cat_dt_off = torch.searchsorted(key, cats).to(torch.int32)
        cat_gt_off = torch.searchsorted(self._gt_key, cats).to(torch.int32)
        if S:
            mx = torch.stack([(gt_off[1:] - gt_off[:-1]).max(), (dt_off[1:] - dt_off[:-1]).max()]).tolist()
            max_g, max_d = int(mx[0]), int(mx[1])
        else:
            max_g = max_d = 0
        area_rng = torch.tensor(np.asarray(p.areaRng, np.float64).reshape(-1, 2), dtype=f64, device=dev)
        iou_thr = torch.tensor(np.asarray(p.iouThrs, np.float64), dtype=f64, device=dev)
        A, T = int(area_rng.shape[0]), int(iou_thr.numel())
        dtm = torch.empty((A, T, ND), dtype=i64, device=dev)
        dt_ig = torch.empty((A, T, ND), dtype=torch.uint8, device=dev)
        gt_ig = torch.empty((A, NG), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("mx_coco_match", _lib.ptr(dt_xywh), _lib.ptr(dt_area), _lib.ptr(dt_off), ND,
                      _lib.ptr(self._gt_xywh), _lib.ptr(self._gt_area), _lib.ptr(self._gt_crowd), _lib.ptr(self._gt_id),
                      _lib.ptr(gt_off), NG, S, _lib.ptr(area_rng), A, _lib.ptr(iou_thr), T, max_g, max_d,
                      _lib.ptr(dtm), _lib.ptr(dt_ig), _lib.ptr(gt_ig), _lib.stream())
        self._m = dict(key=key, score=score, dt_off=dt_off, gt_off=gt_off, cat_dt_off=cat_dt_off,
                       cat_gt_off=cat_gt_off, seg=seg, dtm=dtm, dt_ig=dt_ig, gt_ig=gt_ig, S=S, ND=ND, NG=NG, A=A, T=T,
                       area_rng=area_rng, iou_thr=iou_thr, dt_xywh=dt_xywh, dt_area=dt_area)

    def matches(self):
        """evaluate()'s result on the host: per segment s = (category index seg_cat[s], image index
        seg_img[s]) the detections dt_off[s]:dt_off[s+1] (score order) of dtm / dt_ig [A][T][ND] and
        the GTs gt_off[s]:gt_off[s+1] (annotation order) of gt_ig [A][NG] / gt_id [NG]."""
        m = self._m
        if m is None:
            raise RuntimeError("Please run evaluate() first")
        seg = m["seg"].cpu().numpy()
        return {"seg_cat": seg // max(self._I, 1), "seg_img": seg % max(self._I, 1),
                "dt_off": m["dt_off"].cpu().numpy(), "gt_off": m["gt_off"].cpu().numpy(),
                "dtm": m["dtm"].cpu().numpy(), "dt_ig": m["dt_ig"].cpu().numpy(), "gt_ig": m["gt_ig"].cpu().numpy(),
                "gt_id": self._gt_id.cpu().numpy(), "dt_score": m["score"].cpu().numpy()}

    # -- accumulate --------------------------------------------------------------------------------
    def accumulate(self):
        m, p, dev = self._m, self.params, self.device
        if m is None:
            raise RuntimeError("Please run evaluate() first")
        f64 = torch.float64
        K, A, T, ND, NG = self._K, m["A"], m["T"], m["ND"], m["NG"]
        rec_thr = torch.tensor(np.asarray(p.recThrs, np.float64), dtype=f64, device=dev)
        max_dets = torch.tensor([int(v) for v in p.maxDets], dtype=torch.int32, device=dev)
        R, M = int(rec_thr.numel()), int(max_dets.numel())
        # each category's detections by score descending, ties in (image, rank) order
        o1 = torch.sort(m["score"], descending=True, stable=True).indices
        o2 = torch.sort((m["key"] // max(self._I, 1))[o1], stable=True).indices
        perm = o1[o2].contiguous()
        precision = torch.empty((T, R, K, A, M), dtype=f64, device=dev)
        scores = torch.empty((T, R, K, A, M), dtype=f64, device=dev)
        recall = torch.empty((T, K, A, M), dtype=f64, device=dev)
        with torch.cuda.device(dev):
            nws = _lib.load().mx_coco_accumulate_workspace(ND)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            _lib.call("mx_coco_accumulate", _lib.ptr(m["dtm"]), _lib.ptr(m["dt_ig"]), _lib.ptr(m["gt_ig"]),
                      _lib.ptr(m["score"]), _lib.ptr(perm), _lib.ptr(m["dt_off"]), m["S"], ND, NG,
                      _lib.ptr(m["cat_dt_off"]), _lib.ptr(m["cat_gt_off"]), K, A, T, _lib.ptr(max_dets), M,
                      _lib.ptr(rec_thr), R, _lib.ptr(precision), _lib.ptr(scores), _lib.ptr(recall), _lib.ptr(ws), nws,
                      _lib.stream())
        self.eval = {"params": p, "counts": [T, R, K, A, M], "precision": precision.cpu().numpy(),
                     "recall": recall.cpu().numpy(), "scores": scores.cpu().numpy()}

    # a few numpy means over self.eval: the host code as is
    _summarize = COCOeval._summarize
    summarize = COCOeval.summarize
