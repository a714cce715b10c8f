"""Detection postprocessing on the device (mx_det_candidates -> mx_batched_nms_grouped -> mx_det_select,
ops.detections_postprocess) and the eval forward that uses it (RoIHeads.fused_detections /
MX_FUSED_DETECTIONS=1): each kernel against torch on the same numbers, the composed path bit for bit
against the torch filter chain of RoIHeads.postprocess_detections + the CPU oracle's batched_nms, under
graph capture, and at model level."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROI_W = (10.0, 10.0, 5.0, 5.0)
THR, NMS_THR = 0.05, 0.5
F32 = torch.float32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


# ------------------------------------------------------------------------------------------ reference
def _reference(scores, boxes, img, N, C, D, ratios=None, thr=THR, nms_thr=NMS_THR):
    """RoIHeads.postprocess_detections' torch filter chain on the CPU, per image, from the dense
    (row, class) scores [R*(C-1)] / boxes [R*(C-1), 4] and the image of each row; batched_nms by label from
    the CPU oracle; [:D]; GeneralizedRCNNTransform.postprocess' multiply. -> (list of dicts, live counts
    before NMS, survivors after NMS)."""
    from oracle.cpu_backend import CpuBackend
    be = CpuBackend()
    scores, boxes, img = scores.cpu(), boxes.cpu(), img.cpu()
    R = img.shape[0]
    sc_all = scores.view(R, C - 1)
    bx_all = boxes.view(R, C - 1, 4)
    out, live, surv = [], [], []
    for i in range(N):
        rows = torch.where(img == i)[0]
        sc = sc_all[rows].reshape(-1)
        bx = bx_all[rows].reshape(-1, 4)
        labels = torch.arange(1, C).view(1, -1).expand(rows.shape[0], C - 1).reshape(-1)
        k = torch.where(sc > thr)[0]
        bx, sc, labels = bx[k], sc[k], labels[k]
        ws, hs = bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]
        k = torch.where((ws >= 1e-2) & (hs >= 1e-2))[0]
        bx, sc, labels = bx[k], sc[k], labels[k]
        live.append(int(sc.shape[0]))
        k = be.batched_nms(bx, sc, labels, nms_thr) if sc.shape[0] else torch.zeros(0, dtype=torch.int64)
        surv.append(int(k.shape[0]))
        k = k[:D]
        b = bx[k]
        if ratios is not None:
            rh, rw = ratios[i, 0].cpu(), ratios[i, 1].cpu()
            b = torch.stack((b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh), 1)
        out.append({"boxes": b, "labels": labels[k], "scores": sc[k]})
    return out, live, surv


def _assert_padded_equals(got, ref, D):
    ob, osc, ol, counts = (t.cpu() for t in got)
    N = len(ref)
    assert ob.shape == (N, D, 4) and osc.shape == (N, D) and ol.shape == (N, D) and counts.shape == (N,)
    assert ob.dtype == F32 and osc.dtype == F32 and ol.dtype == torch.int64 and counts.dtype == torch.int32
    assert counts.tolist() == [r["scores"].shape[0] for r in ref]
    for i, r in enumerate(ref):
        c = int(counts[i])
        assert torch.equal(ol[i, :c], r["labels"])
        assert _same_bits(osc[i, :c], r["scores"])
        assert _same_bits(ob[i, :c], r["boxes"])
        assert not _bits(ob[i, c:]).any() and not _bits(osc[i, c:]).any() and not ol[i, c:].any()


# ------------------------------------------------------------------------------------------ 1. candidates
NAN_LOGIT, NAN_REG, INF_DW, INF_DX, ZERO_ROI, FLIP_ROI, FAR_ROI = 20, 21, 22, 26, 23, 24, 25


def _candidate_inputs(C, R=257, N=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    # rows of images 0 and 2 and dead rows (N) interleaved; image 1 owns no row
    img = torch.tensor([0, 2, N], dtype=torch.int32)[torch.randint(0, 3, (R,), generator=g)]
    img[NAN_LOGIT:INF_DX + 1] = torch.tensor([0, 2, 0, 2, 0, 2, 0], dtype=torch.int32)
    hw = torch.tensor([[200., 300.], [100., 100.], [250., 180.]])
    ctr = torch.rand(R, 2, generator=g) * torch.tensor([340., 280.]) - 20
    wh = torch.rand(R, 2, generator=g) * 116 + 4
    rois = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    logits = torch.randn(R, C, generator=g) * 2
    logits[:10] = torch.where(torch.rand(10, C, generator=g) < 0.5, -80.0, 80.0)  # needs the max subtraction
    logits[10:14] = logits[10:14] * 0.1 - 80.0
    reg = torch.randn(R, 4 * C, generator=g) * 0.5
    logits[NAN_LOGIT, 3 % C] = float("nan")
    reg[NAN_REG] = float("nan")
    reg[INF_DW, 2::4] = float("inf")   # dw: clamped by clip
    reg[INF_DX, 0::8] = float("inf")   # dx of classes 0, 2, ..: an infinite box, clamped to the image bound
    reg[INF_DX, 4::8] = float("-inf")  # dx of classes 1, 3, ..
    rois[ZERO_ROI] = torch.tensor([50., 60., 50., 90.])
    rois[FLIP_ROI] = torch.tensor([120., 40., 80., 90.])
    rois[FAR_ROI] = torch.tensor([900., 700., 950., 760.])
    reg[FAR_ROI] = 0.0
    logits[ZERO_ROI:FAR_ROI + 1] = 0.0
    logits[ZERO_ROI:FAR_ROI + 1, 1] = 5.0  # class 1 passes the score filter: these rows die by size
    return logits, reg, rois, img, hw


@pytest.mark.parametrize("C,strided", [(2, False), (7, False), (7, True), (91, False)])
def test_candidates(dev, C, strided):
    from mx_det import ops
    N = 3
    logits, reg, rois, img, hw = _candidate_inputs(C)
    R = logits.shape[0]
    if strided:  # the predictor's layout: logits and regression are column slices of one [R, 5C + 5] matrix
        o = torch.full((R, 5 * C + 5), 7.0)
        o[:, :C], o[:, C:5 * C] = logits, reg
        o = o.to(dev)
        d_logits, d_reg = o[:, :C], o[:, C:5 * C]
        assert d_logits.stride(0) > C and d_reg.stride(0) > 4 * C and not d_reg.is_contiguous()
    else:
        d_logits, d_reg = logits.to(dev), reg.to(dev)
    scores, boxes, labels, grp = ops.detection_candidates(d_logits, d_reg, rois.to(dev), img.to(dev), hw.to(dev), N,
                                                          THR)
    n = R * (C - 1)
    assert scores.shape == (n,) and boxes.shape == (n, 4) and labels.shape == (n,) and grp.shape == (n,)
    assert labels.dtype == torch.int64 and grp.dtype == torch.int32

    # scores: f64 softmax rounded to f32, 1e-6 absolute
    ref = torch.softmax(logits.double(), -1)[:, 1:].to(F32).reshape(-1)
    got = scores.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert nan.view(R, C - 1)[NAN_LOGIT].all() and int(nan.sum()) == C - 1
    err = (got[~nan].double() - ref[~nan].double()).abs().max().item()
    print(f"C={C} softmax max abs err {err:.3e}")
    assert err <= 1e-6

    # boxes: ops.box_decode + torch's scalar clamp on the device, bitwise (dead rows: not clamped)
    dec = ops.box_decode(reg.to(dev), rois.to(dev), ROI_W).reshape(R, C, 4)[:, 1:].clone()
    for i in range(N):
        rows = torch.where(img.to(dev) == i)[0]
        h, w = float(hw[i, 0]), float(hw[i, 1])
        b = dec[rows]
        dec[rows] = torch.stack((b[..., 0].clamp(0, w), b[..., 1].clamp(0, h), b[..., 2].clamp(0, w),
                                 b[..., 3].clamp(0, h)), -1)
    assert _same_bits(boxes, dec.reshape(-1, 4))
    bx = boxes.cpu().view(R, C - 1, 4)
    assert torch.isnan(bx[NAN_REG]).all()
    assert torch.isfinite(bx[INF_DW]).all()
    assert torch.equal(bx[INF_DX, 0, 0::2], torch.zeros(2))  # class 1: -inf -> 0
    if C > 2:
        assert torch.equal(bx[INF_DX, 1, 0::2], torch.full((2,), float(hw[int(img[INF_DX]), 1])))  # class 2: +inf -> w

    assert torch.equal(labels.cpu(), torch.arange(1, C).repeat(R))

    # grp: the rule re-evaluated on the CPU from the kernel's own numbers
    s, b = scores.cpu(), boxes.cpu()
    row_img = img.repeat_interleave(C - 1)
    live = ((row_img < N) & (s > torch.tensor(THR, dtype=F32)) & (b[:, 2] - b[:, 0] >= torch.tensor(1e-2, dtype=F32))
            & (b[:, 3] - b[:, 1] >= torch.tensor(1e-2, dtype=F32)))
    want = torch.where(live, row_img, torch.tensor(N, dtype=torch.int32))
    assert torch.equal(grp.cpu(), want)
    gr = grp.cpu().view(R, C - 1)
    for r in (NAN_LOGIT, NAN_REG, ZERO_ROI, FLIP_ROI, FAR_ROI):
        assert (gr[r] == N).all(), r
    assert (gr[img == N] == N).all() and not (gr == 1).any()
    assert (gr == 0).any() and (gr == 2).any()
    # every kind of filter is exercised: dead by score alone and by size alone
    by_score = (row_img < N) & ~(s > torch.tensor(THR, dtype=F32))
    assert by_score.any() and ((row_img < N) & (s > torch.tensor(THR, dtype=F32)) & ~live).any()


# ------------------------------------------------------------------------------------------ 2. select
@pytest.mark.parametrize("D", [1, 100])
@pytest.mark.parametrize("with_ratios", [True, False])
def test_select(dev, D, with_ratios):
    from mx_det import ops
    N = 4
    want = [0, D - 1, D, D + 37]  # survivors per image
    g = torch.Generator().manual_seed(10 + D)
    n = sum(want) + 150
    boxes = torch.rand(n, 4, generator=g) * 300
    scores = torch.rand(n, generator=g)
    labels = torch.randint(1, 7, (n,), generator=g)
    perm = torch.randperm(n, generator=g)
    perm = perm[perm != 0]
    perm = torch.cat([perm[:want[0] + want[1]], torch.zeros(1, dtype=torch.int64), perm[want[0] + want[1]:]])
    # suppressed entries keep an image, some are dead; entry 0 belongs to image 2, so a reader that ran
    # into keep's tail (zeros) would count it
    grp = torch.randint(0, N + 1, (n,), generator=g).to(torch.int32)
    surv, off = [], 0
    for i, c in enumerate(want):
        idx = perm[off:off + c]
        off += c
        grp[idx] = i
        surv.append(idx)
    keep = torch.zeros(n, dtype=torch.int64)
    nk = sum(want)
    keep[:nk] = torch.cat(surv)
    ratios = torch.tensor([[1.5, 0.75], [1.0, 1.0], [0.3333333, 2.25], [1.2345, 0.987]]) if with_ratios else None

    def run(num_keep):
        return ops.detection_select(keep.to(dev), torch.tensor([num_keep], dtype=torch.int64, device=dev),
                                    boxes.to(dev), scores.to(dev), labels.to(dev), grp.to(dev), N, D,
                                    ratios.to(dev) if with_ratios else None)

    ref = []
    for i, idx in enumerate(surv):
        k = idx[:D]
        b = boxes[k]
        if with_ratios:
            rh, rw = ratios[i, 0], ratios[i, 1]
            b = torch.stack((b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh), 1)
        ref.append({"boxes": b, "labels": labels[k], "scores": scores[k]})
    got = run(nk)
    _assert_padded_equals(got, ref, D)
    assert got[3].tolist() == [0, min(D - 1, D), D, D]

    empty = [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64), "scores": torch.zeros(0)}] * N
    _assert_padded_equals(run(0), empty, D)
    ob, osc, ol, counts = run(-1)  # a failed NMS: never an empty result
    assert counts.tolist() == [-1] * N
    assert not _bits(ob).any() and not _bits(osc).any() and not ol.any()


# ------------------------------------------------------------------------------------------ 3. composed
COMPOSED = dict(N=3, per=400, C=7, D=100)


def _composed_inputs(seed):
    """Image 0: most of its 2400 candidates are live (per-class NMS); image 1: background wins except in
    150 rows (coordinate trick); image 2: nothing over the score threshold. Boxes sit in 40 clusters
    per image; some rows are exact copies of another (tied scores)."""
    N, per, C = COMPOSED["N"], COMPOSED["per"], COMPOSED["C"]
    g = torch.Generator().manual_seed(seed)
    R = N * per
    cell = torch.arange(40)
    cx, cy = (cell % 8) * 50.0 + 25, (cell // 8) * 64.0 + 32   # 8 x 5 grid on a 320 x 400 image
    which = torch.randint(0, 40, (R,), generator=g)
    ctr = torch.stack([cx[which], cy[which]], 1) + torch.randn(R, 2, generator=g) * 1.5
    wh = torch.tensor([36., 44.]) + torch.randn(R, 2, generator=g) * 2
    rois = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    reg = torch.randn(R, 4 * C, generator=g) * 0.15
    logits = torch.randn(R, C, generator=g) * 0.5
    logits[per:2 * per, 0] += 4.0
    rows = per + torch.arange(150)
    logits[rows, torch.randint(1, C, (150,), generator=g)] += 3.5
    logits[2 * per:, 0] += 12.0
    for base in (4, per + 7, per + 90):  # exact duplicates
        logits[base + 1:base + 6], reg[base + 1:base + 6], rois[base + 1:base + 6] = logits[base], reg[base], rois[base]
    for base in (40, per + 40):  # the same logits on other boxes: tied scores that both survive, near the top
        logits[base, 2] += 3.0
        logits[base + 1:base + 12] = logits[base]
    img = torch.arange(N, dtype=torch.int32).repeat_interleave(per)
    img[per - 10:per] = N  # padded rows, dead
    img[2 * per - 10:2 * per] = N
    hw = torch.tensor([[320., 400.], [300., 380.], [320., 400.]])
    ratios = torch.tensor([[1.5, 0.75], [1.0, 1.0], [2.0, 1.25]])
    return logits, reg, rois, img, hw, ratios


def test_composed_path_bitwise(dev):
    from mx_det import ops
    N, C, D = COMPOSED["N"], COMPOSED["C"], COMPOSED["D"]
    logits, reg, rois, img, hw, ratios = (t.to(dev) for t in _composed_inputs(1))
    scores, boxes, _, _ = ops.detection_candidates(logits, reg, rois, img, hw, N, THR)
    ref, live, surv = _reference(scores, boxes, img, N, C, D, ratios)
    print("live per image", live, "survivors", surv)
    assert live[0] > 1000 and 1 <= live[1] <= 1000 and live[2] == 0  # both dispatch regimes and an empty image
    assert surv[0] > D and 0 < surv[1] < live[1]
    for r in ref[:2]:  # tied scores among the returned detections: the order by index is on trial
        assert (r["scores"][1:] == r["scores"][:-1]).any()
    got = ops.detections_postprocess(logits, reg, rois, img, hw, N, THR, NMS_THR, D, ratios=ratios,
                                     max_seg=COMPOSED["per"])
    _assert_padded_equals(got, ref, D)
    # the default segment bound (no knowledge of the rows per image) gives the same result
    got2 = ops.detections_postprocess(logits, reg, rois, img, hw, N, THR, NMS_THR, D, ratios=ratios)
    assert all(_same_bits(a, b) for a, b in zip(got, got2))


def test_no_rows(dev):
    from mx_det import ops
    N, C, D = 2, 7, 5
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    ob, osc, ol, counts = ops.detections_postprocess(z(0, C), z(0, 4 * C), z(0, 4), z(0, dt=torch.int32),
                                                     torch.ones(N, 2, device=dev), N, THR, NMS_THR, D)
    assert counts.tolist() == [0, 0] and ob.shape == (N, D, 4)
    assert not _bits(ob).any() and not _bits(osc).any() and not ol.any()


# ------------------------------------------------------------------------------------------ 4. graph capture
def test_graph_replay_matches_eager(dev):
    """The composed path holds no host synchronisation and no per-call state: captured once, replayed
    on new contents of its static inputs, it gives the eager result bit for bit."""
    from mx_det import ops
    N, D = COMPOSED["N"], COMPOSED["D"]

    def chain(t):
        logits, reg, rois, img, hw, ratios = t
        return ops.detections_postprocess(logits, reg, rois, img, hw, N, THR, NMS_THR, D, ratios=ratios,
                                          max_seg=COMPOSED["per"])

    static = [t.to(dev) for t in _composed_inputs(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream
        chain(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain(static)
    for seed in (3, 4):
        fresh = [t.to(dev) for t in _composed_inputs(seed)]
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        ref = chain(fresh)
        torch.cuda.synchronize()
        assert int(ref[3].sum()) > 0
        for a, b in zip(out, ref):
            assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------ 5 / 6. model
ORIGINAL = ((180, 240), (200, 210))


class _Recorder:
    """The HIP backend with detections_postprocess recorded."""

    def __init__(self, be):
        self._be, self.calls = be, []

    def __getattr__(self, k):
        return getattr(self._be, k)

    def detections_postprocess(self, *a, **kw):
        self.calls.append((a, kw))
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


@pytest.mark.parametrize("switch", ["attribute", "env"])
def test_model_fused_detections(model, switch, monkeypatch):
    from mx_det import ops
    m, rec, images = model
    rec.calls.clear()
    if switch == "env":
        monkeypatch.setenv("MX_FUSED_DETECTIONS", "1")
    else:
        monkeypatch.setattr(m.roi_heads, "fused_detections", True)
    seen = {}
    inner = m.rpn.filter_proposals_padded

    def padded(*a, **kw):
        seen["proposals"] = inner(*a, **kw)
        return seen["proposals"]

    monkeypatch.setattr(m.rpn, "filter_proposals_padded", padded)
    with torch.no_grad():
        out = m(images)
    assert len(rec.calls) == 1
    (logits, reg, rois, img, hw, N, thr, nms_thr, D), kw = rec.calls[0]
    C = logits.shape[1]
    assert (N, C, D, thr, nms_thr) == (2, 7, m.roi_heads.detections_per_img, 0.05, 0.5)

    # the padded rows of the RPN, dead exactly where its validity mask is False
    pb, _, valid = seen["proposals"]
    post = valid.shape[1]
    assert logits.shape[0] == N * post and torch.equal(rois, pb.reshape(-1, 4))
    bi = torch.arange(N, dtype=torch.int32, device=img.device).repeat_interleave(post)
    assert torch.equal(img, torch.where(valid.reshape(-1), bi, N))
    assert not valid.all() and valid.any(1).all()  # some padded rows, no empty image

    # the ratios transform.postprocess computes, and the resized sizes
    import math
    sizes = []
    for h, w in ORIGINAL:  # F.interpolate(recompute_scale_factor=True): floor(in * scale) in double
        sc = min(256 / min(h, w), 512 / max(h, w))
        sizes.append((math.floor(h * sc), math.floor(w * sc)))
    assert hw.cpu().tolist() == [[float(h), float(w)] for h, w in sizes]
    want = torch.tensor([[torch.tensor(o, dtype=F32) / torch.tensor(s, dtype=F32) for o, s in zip(os_, ss)]
                         for os_, ss in zip(ORIGINAL, sizes)])
    assert _same_bits(kw["ratios"], want)
    assert len(set(want.reshape(-1).tolist())) == 4 and 1.0 not in want.reshape(-1).tolist()

    scores, boxes, _, _ = ops.detection_candidates(logits, reg, rois, img, hw, N, thr)
    ref, live, surv = _reference(scores, boxes, img, N, C, D, kw["ratios"])
    print("model: live", live, "survivors", surv)
    assert len(out) == N and min(surv) > 0
    for o, r in zip(out, ref):
        assert list(o) == ["boxes", "labels", "scores"]
        assert o["boxes"].dtype == F32 and o["scores"].dtype == F32 and o["labels"].dtype == torch.int64
        k = o["scores"].shape[0]
        assert k <= D and o["boxes"].shape == (k, 4) and o["labels"].shape == (k,)
        assert torch.equal(o["labels"].cpu(), r["labels"])
        assert _same_bits(o["scores"], r["scores"]) and _same_bits(o["boxes"], r["boxes"])
        s = o["scores"].cpu()
        assert (s[1:] <= s[:-1]).all()
        assert ((o["labels"] >= 1) & (o["labels"] <= C - 1)).all()


def test_model_switch_off_keeps_the_torch_tail(model, monkeypatch):
    m, rec, images = model
    rec.calls.clear()
    monkeypatch.delenv("MX_FUSED_DETECTIONS", raising=False)
    assert m.roi_heads.fused_detections is False
    with torch.no_grad():
        out = m(images)
    assert len(rec.calls) == 0
    assert len(out) == 2 and all(list(o) == ["boxes", "labels", "scores"] for o in out)
    assert all(0 < o["scores"].shape[0] <= m.roi_heads.detections_per_img for o in out)
