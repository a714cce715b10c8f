"""numpy restatement of the test-time-augmentation tail (include/mx_det.h: mx_det_views_fold,
mx_det_select_vote): the fold as elementwise f32, the IoU with every operation in np.float32 (one
rounding each, torchvision's box_iou order), the voting sums as a plain ascending f64 loop."""
import numpy as np

F32 = np.float32


def fold(boxes, grp, hw, V, N, P, C, flips):
    """boxes [n, 4] f32, grp [n] int32, hw [N, 2] f32 (h, w), flips [V] -> (boxes_out, grp_out)."""
    boxes = np.asarray(boxes, F32)
    grp = np.asarray(grp, np.int32)
    n = V * N * P * (C - 1)
    assert boxes.shape == (n, 4) and grp.shape == (n,)
    ob, og = boxes.copy(), np.full(n, N, np.int32)
    per = P * (C - 1)
    for b in range(V * N):
        v, i = divmod(b, N)
        sl = slice(b * per, (b + 1) * per)
        live = grp[sl] == b
        og[sl][live] = i
        if flips[v]:
            w = F32(hw[i][1])
            x1, x2 = boxes[sl, 0], boxes[sl, 2]
            ob[sl, 0] = np.where(live, w - x2, x1)  # f32 - f32 array ops: one rounding each
            ob[sl, 2] = np.where(live, w - x1, x2)
    return ob, og


def iou(box, others):
    """f32 IoU of box [4] against others [m, 4]: inter / ((area1 + area2) - inter), NaN where undefined."""
    a = np.asarray(box, F32)
    o = np.asarray(others, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        area_a = F32(F32(a[2] - a[0]) * F32(a[3] - a[1]))
        area_o = (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1])
        ltx, lty = np.maximum(a[0], o[:, 0]), np.maximum(a[1], o[:, 1])
        rbx, rby = np.minimum(a[2], o[:, 2]), np.minimum(a[3], o[:, 3])
        w, h = rbx - ltx, rby - lty
        w = np.where(w < 0, F32(0), w)  # NaN stays NaN, as torch.clamp(min=0)
        h = np.where(h < 0, F32(0), h)
        inter = w * h
        out = inter / ((area_a + area_o) - inter)
    assert out.dtype == F32
    return out


def vote(box, cand_boxes, cand_scores, hit):
    """The score-weighted mean of the voters (hit mask over the candidates, in ascending order): f64 sums
    added one by one, one f64 division per coordinate, one rounding to f32. No voter: the box itself."""
    idx = np.flatnonzero(hit)
    if idx.size == 0:
        return np.asarray(box, F32).copy()
    ss = np.float64(0.0)
    sb = np.zeros(4, np.float64)
    for t in idx:
        w = np.float64(cand_scores[t])
        ss = ss + w
        for q in range(4):
            sb[q] = sb[q] + w * np.float64(cand_boxes[t, q])
    with np.errstate(all="ignore"):
        return (sb / ss).astype(F32)


def select_vote(keep, num_keep, boxes, scores, labels, grp, V, N, P, C, D, vote_iou, ratios=None):
    """-> (out_boxes [N, D, 4], out_scores [N, D], out_labels [N, D], counts [N], voters): voters[g] lists
    the number of voters of each selected survivor of image g (None where voting is off)."""
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    labels = np.asarray(labels, np.int64)
    grp = np.asarray(grp, np.int32)
    keep = np.asarray(keep, np.int64)
    n = V * N * P * (C - 1)
    assert boxes.shape == (n, 4)
    thr = F32(vote_iou)
    on = bool(thr <= F32(1.0))  # False for NaN
    ob = np.zeros((N, D, 4), F32)
    osc = np.zeros((N, D), F32)
    ol = np.zeros((N, D), np.int64)
    counts = np.zeros(N, np.int32)
    voters = [[] for _ in range(N)]
    if num_keep < 0:
        counts[:] = -1
        return ob, osc, ol, counts, voters
    kept = keep[:min(num_keep, n)]
    kg = grp[kept] if kept.size else np.zeros(0, np.int32)
    r = np.arange(P)
    for g in range(N):
        mine = kept[kg == g][:D]
        counts[g] = mine.size
        for d, k in enumerate(mine):
            b, c = boxes[k].copy(), int(labels[k])
            if on and 1 <= c < C:
                t = np.concatenate([((v * N + g) * P + r) * (C - 1) + (c - 1) for v in range(V)])  # ascending
                with np.errstate(invalid="ignore"):
                    hit = (grp[t] == g) & (iou(b, boxes[t]) >= thr)
                voters[g].append(int(hit.sum()))
                b = vote(b, boxes[t], scores[t], hit)
            else:
                voters[g].append(None)
            if ratios is not None:
                rh, rw = F32(ratios[g][0]), F32(ratios[g][1])
                b = np.array([b[0] * rw, b[1] * rh, b[2] * rw, b[3] * rh], F32)
            ob[g, d], osc[g, d], ol[g, d] = b, scores[k], labels[k]
    return ob, osc, ol, counts, voters
