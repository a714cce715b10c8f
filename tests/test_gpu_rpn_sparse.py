"""Row-sparse backward of the RPN head (csrc/mx_rpn_sparse.hip, mx_conv2d_wgrad_x3_rows, conv.RowLists).

The RPN loss gives a gradient to at most batch_size_per_image sampled anchors per image, so the raw
head maps' gradient is exactly zero on all but a few hundred pixels. The lists of those pixels (S0) and
of their 3x3 dilations (S1, S2), and the lists of the 32-pixel K-steps that hold them, are checked
against a numpy dilation, overflow and guard words included; the head convs' weight gradients, which
run only the listed K-steps, against float64 torch with test_gpu_x3.py's bound (relative L2 < 1e-4 and
10x below the same gradient from TF32-rounded operands) and bit for bit against the dense path,
across graph replays and in a whole train step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------ lists
def _dilate(m):
    """3x3 dilation of a bool [N, H, W] mask inside each image."""
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(m)
    H, W = m.shape[1:]
    for dh in range(3):
        for dw in range(3):
            out |= p[:, dh:dh + H, dw:dw + W]
    return out


def _build(dev, g, caps, entry="mx_rpn_rows_build"):
    """mx_rpn_rows_build / mx_rpn_tiles_build on g [N, H, W, C] with guard words behind every list, the
    counts and the scratch: (lists, counts, flag, guards intact)."""
    from mx_det import _lib
    from mx_det._lib import call
    N, H, W, C = g.shape
    P = N * H * W
    lib = _lib.load()
    wsb = lib.mx_rpn_rows_workspace(P)
    offs, o = [], 0
    for c in caps:
        offs.append(o)
        o += c + 4
    cnt_off = o
    buf = torch.full((o + 3 + 4,), GUARD, dtype=torch.int32, device=dev)
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ptr = [buf[a:].data_ptr() for a in offs]
    call(entry, g.data_ptr(), N, H, W, C, 3, ptr[0], caps[0], ptr[1], caps[1], ptr[2], caps[2],
         buf[cnt_off:].data_ptr(), flag.data_ptr(), ws.data_ptr(), wsb, _lib.stream())
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    lists = [b[a:a + c] for a, c in zip(offs, caps)]
    guards = all((b[a + c:a + c + 4] == GUARD).all() for a, c in zip(offs, caps))
    guards = guards and (b[cnt_off + 3:] == GUARD).all() and bool((ws[wsb:] == 0x5A).all())
    return lists, b[cnt_off:cnt_off + 3], int(flag), guards


def _canvas_hw():
    from mx_det import frcnn
    _, Hc, Wc = frcnn.RPNHead.canvas_layout([(7, 11), (4, 6), (2, 3), (1, 2)])
    return Hc, Wc


def _patterns(N, H, W, cap0):
    P = N * H * W
    flat = lambda idx: np.isin(np.arange(P), idx).reshape(N, H, W)
    rng = np.random.default_rng(H * 131 + W)
    pats = {
        "corners": flat([0, W - 1, (H - 1) * W, H * W - 1, P - H * W, P - 1]),
        "image_seam": flat([H * W - 1, H * W]),
        "border_row": flat(np.arange((H - 1) * W, H * W)),
        "none": flat([]),
        "capacity": flat(rng.choice(P, cap0, replace=False)),
        "capacity_plus_1": flat(rng.choice(P, cap0 + 1, replace=False)),
        "all": flat(np.arange(P)),
    }
    return pats


@pytest.mark.parametrize("hw", [(5, 7), (13, 21), "canvas"])
def test_row_lists_match_numpy_dilation(dev, hw):
    from mx_det import _lib
    lib = _lib.load()
    N, A5 = 2, 15
    H, W = _canvas_hw() if hw == "canvas" else hw
    P = N * H * W
    NB = max(W, 6)  # S0 holds a full border row; small enough for S1 / S2 to overflow on "all"
    caps = [lib.mx_rpn_rows_capacity(P, NB, l) for l in range(3)]
    assert caps == [min(P, NB), min(P, 9 * NB), min(P, 25 * NB)]
    T = (P + 31) // 32
    NBT = 2  # K-step lists: a capacity that the larger patterns overflow
    tcaps = [lib.mx_rpn_tiles_capacity(P, NBT, l) for l in range(3)]
    assert tcaps == [min(T, NBT), min(T, 6 * NBT), min(T, 10 * NBT)]
    rng = np.random.default_rng(3)
    for name, m0 in _patterns(N, H, W, caps[0]).items():
        g = np.zeros((N, H, W, A5), np.float32)
        g[..., 0] = -0.0                                    # a negative zero does not mark a pixel
        ch = rng.integers(0, A5, size=(N, H, W))
        val = rng.choice(np.array([1.0, -2.5, 1e-42, -1e-45], np.float32), size=(N, H, W))  # denormals mark
        np.put_along_axis(g, ch[..., None], np.where(m0, val, g[..., 0])[..., None].astype(np.float32), 3)
        if name == "all":
            g[:] = 1.0
        gd = torch.from_numpy(g).to(dev)
        for entry, cps, per in (("mx_rpn_rows_build", caps, 1), ("mx_rpn_tiles_build", tcaps, 32)):
            lists, counts, flag, guards = _build(dev, gd, cps, entry)
            assert guards, (name, entry)
            m, over = m0, False
            for l in range(3):
                if l:
                    m = _dilate(m)
                ref = np.unique(np.flatnonzero(m.reshape(-1)) // per)  # pixels, or their 32-pixel K-steps
                assert counts[l] == ref.size, (name, entry, l, counts, ref.size)
                n = min(ref.size, cps[l])
                assert np.array_equal(lists[l][:n], ref[:n]), (name, entry, l)
                assert (lists[l][n:] == GUARD).all(), (name, entry, l)  # nothing written past the count
                over |= ref.size > cps[l]
            assert flag == int(over), (name, entry, flag, over)


# ------------------------------------------------------------------------------- tower backward
def tf32(t):
    i = t.float().contiguous().view(torch.int32).to(torch.int64)
    r = ((i + 0xFFF + ((i >> 13) & 1)) >> 13) << 13
    return (((r + 2 ** 31) % 2 ** 32) - 2 ** 31).to(torch.int32).view(torch.float32)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _check(got, ref64, tf32_ref):
    """tests/test_gpu_x3.py's bound of the dense x3 dgrad / wgrad."""
    e = rel(got, ref64)
    et = rel(tf32_ref, ref64)
    print(f"rel err {e:.3e} (tf32 operands {et:.3e})")
    assert e < 1e-4, e
    assert e * 10 < et or e < 1e-6, (e, et)


B = 20  # batch_size_per_image of the tests: S0 capacity 2 * 20 = 40 pixels


def _head(dev, C, seed=0):
    from mx_det import frcnn
    torch.manual_seed(seed)
    h = frcnn.RPNHead(C, 3)
    with torch.no_grad():
        for p in h.parameters():  # the 0.01-std init gives ReLU towers of ~1e-3: use O(1) activations
            p.copy_(torch.randn(p.shape) * (0.5 if p.dim() == 1 else (2.0 / (p[0].numel())) ** 0.5))
    return h.to(dev)


def _grad_map(N, H, W, k, seed):
    """A raw-map gradient [N, H, W, 15] with k nonzero pixels, the four corners first."""
    g = torch.Generator().manual_seed(seed)
    P = N * H * W
    corners = [0, W - 1, (H - 1) * W, H * W - 1, P - H * W, P - 1]
    rest = [i for i in torch.randperm(P, generator=g).tolist() if i not in corners]
    idx = torch.tensor((corners + rest)[:k], dtype=torch.int64)
    gm = torch.zeros(P, 15)
    gm[idx] = torch.randn(idx.numel(), 15, generator=g)
    return gm.view(N, H, W, 15)


def _run_head(h, x, gout, sparse, monkeypatch):
    from mx_det.backend import HipBackend
    monkeypatch.setenv("MX_RPN_SPARSE_BWD", "1" if sparse else "0")
    monkeypatch.setenv("MX_CONV_TUNE", "0")  # the library's default 128 x 128 wgrad: the kernel with a tile-list form
    h.__dict__["sparse_rows_per_image"] = B
    be = HipBackend("f32")
    for p in h.parameters():
        p.grad = None
    xd = x.detach().clone().requires_grad_(True)
    w = torch.cat([h.cls_logits.weight, h.bbox_pred.weight])
    b = torch.cat([h.cls_logits.bias, h.bbox_pred.bias])
    y = h._run(xd, be, w, b)
    y.backward(gout)
    torch.cuda.synchronize()
    out = {n: p.grad.detach().clone() for n, p in h.named_parameters()}
    out["dx"] = xd.grad.detach().clone()
    return out


def _reference(h, x, gout):
    """float64 torch.nn.functional tower on the CPU: every gradient, and each tower conv's weight
    gradient from TF32-rounded operands (the bound's yardstick)."""
    hp = {n: p.detach().double().cpu() for n, p in h.named_parameters()}
    xs = [x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)]
    ps = {n: v.clone().requires_grad_(True) for n, v in hp.items()}
    t = xs[0]
    acts = []
    for i in range(2):
        z = F.conv2d(t, ps[f"conv.{i}.0.weight"], ps[f"conv.{i}.0.bias"], 1, 1)
        z.retain_grad()
        t = F.relu(z)
        acts.append((xs[-1] if i == 0 else acts[-1][2], z, t))
    w = torch.cat([ps["cls_logits.weight"], ps["bbox_pred.weight"]])
    b = torch.cat([ps["cls_logits.bias"], ps["bbox_pred.bias"]])
    y = F.conv2d(t, w, b)
    y.backward(gout.double().cpu().permute(0, 3, 1, 2))
    ref = {n: v.grad for n, v in ps.items()}
    ref["dx"] = xs[0].grad.permute(0, 2, 3, 1)
    tf = {}
    for i, (xin, z, _) in enumerate(acts):
        wshape = ps[f"conv.{i}.0.weight"].shape
        tf[f"conv.{i}.0.weight"] = torch.nn.grad.conv2d_weight(tf32(xin.detach()).double(), wshape,
                                                              tf32(z.grad).double(), 1, 1)
    # the 1x1 head: cls_logits (A rows) and bbox_pred (4A rows) are one conv
    dwh = torch.nn.grad.conv2d_weight(tf32(acts[-1][2].detach()).double(), w.shape,
                                      tf32(gout.cpu().permute(0, 3, 1, 2)).double())
    A = ps["cls_logits.weight"].shape[0]
    tf["cls_logits.weight"], tf["bbox_pred.weight"] = dwh[:A], dwh[A:]
    return ref, tf


@pytest.mark.parametrize("C,H,W", [(32, 13, 21), (32, 40, 56), (256, 13, 21)])
def test_tower_backward_sparse_vs_f64_and_dense(dev, monkeypatch, C, H, W):
    """The weight gradients of both tower convs and of the 1x1 head run only the K-steps of S0 / S1:
    against f64 with the dense x3 bound, two sparse runs bitwise identical, and every gradient -- those
    three and everything the sparse path does not touch -- bitwise equal to the dense path."""
    N = 2
    h = _head(dev, C)
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(1)).to(dev)
    for k in (0, 1, 37, N * B):
        gout = _grad_map(N, H, W, k, 10 + k).to(dev)
        sp = _run_head(h, x, gout, True, monkeypatch)
        sp2 = _run_head(h, x, gout, True, monkeypatch)
        de = _run_head(h, x, gout, False, monkeypatch)
        from mx_det import conv as mc
        mc.rows_check()  # no overflow up to the capacity
        ref, tf = _reference(h, x, gout)
        for n in sp:
            assert torch.equal(sp[n], sp2[n]), (k, n)
            assert torch.equal(sp[n], de[n]), (k, n)
            if n in tf:
                print(k, n, end=" ")
                _check(sp[n], ref[n], tf[n])
            else:
                assert rel(sp[n], ref[n]) < 1e-4, (k, n, rel(sp[n], ref[n]))


def test_dense_gradient_sets_the_flag_and_raises(dev, monkeypatch):
    """A gradient with more nonzero pixels than N * B (ones_like: the graph warm-ups') overflows: the
    run completes, the flag is set, rows_check raises once and clears it; rows_reset forgets it."""
    from mx_det import conv as mc
    h = _head(dev, 32)
    # 2 x 40 x 56 = 140 K-steps against a capacity of N * B = 40 (a map of fewer K-steps than N * B
    # cannot overflow: its list holds them all)
    x = torch.randn(2, 40, 56, 32, generator=torch.Generator().manual_seed(1)).to(dev)
    ones = torch.ones(2, 40, 56, 15, device=dev)
    mc.rows_reset(dev)
    _run_head(h, x, ones, True, monkeypatch)
    assert int(mc._rows_flags[dev.index][0]) == 1
    with pytest.raises(RuntimeError, match="row-sparse"):
        mc.rows_check()
    assert int(mc._rows_flags[dev.index][0]) == 0
    mc.rows_check()
    _run_head(h, x, ones, True, monkeypatch)
    mc.rows_reset(dev)
    assert int(mc._rows_flags[dev.index][0]) == 0
    mc.rows_check()


# ------------------------------------------------------------------------------------ graph replay
def test_graph_replay_matches_eager_sparse(dev, monkeypatch):
    """Captured as frcnn._Graphs captures the trunk (ones_like warm-ups, zero gradients at capture),
    then replayed with k = 5, 0 and capacity nonzero pixels in that order: every replay's gradients
    are bitwise the eager sparse ones, and the warm-ups' overflow flag is cleared after the capture."""
    from mx_det import conv as mc, frcnn
    from mx_det.backend import HipBackend
    monkeypatch.setenv("MX_RPN_SPARSE_BWD", "1")
    monkeypatch.setenv("MX_CONV_TUNE", "0")  # capture and eager runs launch the same default kernels
    N, H, W, C = 2, 40, 56, 32  # 140 K-steps: the ones_like warm-ups overflow the capacity of 40
    h = _head(dev, C)
    h.__dict__["sparse_rows_per_image"] = B
    be = HipBackend("f32")
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(1)).to(dev)

    def fn(t):
        w = torch.cat([h.cls_logits.weight, h.bbox_pred.weight])
        b = torch.cat([h.cls_logits.bias, h.bbox_pred.bias])
        return (h._run(t, be, w, b),)
    g = frcnn._Graphs(fn, list(h.parameters()), h, x, input_grad=True)
    torch.cuda.synchronize()
    assert int(mc._rows_flags[dev.index][0]) == 0  # set by the ones_like warm-ups, cleared after the capture
    mc.rows_check()
    for k in (5, 0, N * B):
        gout = _grad_map(N, H, W, k, 20 + k).to(dev)
        eager = _run_head(h, x, gout, True, monkeypatch)
        for p in h.parameters():
            p.grad = None
        xd = x.detach().clone().requires_grad_(True)
        (y,) = g(xd)
        y.backward(gout)
        torch.cuda.synchronize()
        for n, p in h.named_parameters():
            assert torch.equal(p.grad, eager[n]), (k, n)
        assert torch.equal(xd.grad, eager["dx"]), k
        mc.rows_check()


# ------------------------------------------------------------------------------------- model level
def _step(dev, base, imgs, tg, monkeypatch, sparse, graphs):
    import copy
    monkeypatch.setenv("MX_RPN_SPARSE_BWD", sparse)
    monkeypatch.setenv("MX_GRAPHS", graphs)
    monkeypatch.setenv("MX_GRAD_CHAIN", "0")  # the graphs then sum in the eager order (test_gpu_model.py)
    monkeypatch.setenv("MX_CONV_TUNE", "0")   # every wgrad the default 128 x 128 kernel: the one with a tile-list form
    m = copy.deepcopy(base)
    torch.manual_seed(5)
    ld = m(imgs, tg)
    sum(ld.values()).backward()
    torch.cuda.synchronize()
    return ({k: float(v.detach()) for k, v in ld.items()},
            {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})


def test_model_step_sparse_vs_dense_and_graphed(dev, monkeypatch):
    """One train step at 2 x 256 x 320: the losses and every parameter gradient are bitwise the dense
    backward's (the skipped K-steps only ever added exact zeros), the RPN head's weight gradients are
    not all zero, and the graphed step is bitwise equal to the eager sparse one."""
    from mx_det import conv as mc, frcnn
    from mx_det.data import synth_batch
    torch.manual_seed(0)
    base = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    base.roi_heads.box_predictor = frcnn.FastRCNNPredictor(1024, 7)
    frcnn.set_trainable_layers(base.backbone.body, 3)
    base = base.to(dev).train()
    imgs, tg = synth_batch(0, 2, H=256, W=320, device=dev)
    ls, gs = _step(dev, base, imgs, tg, monkeypatch, "1", "0")
    ld, gd = _step(dev, base, imgs, tg, monkeypatch, "0", "0")
    lg, gg = _step(dev, base, imgs, tg, monkeypatch, "1", "1")
    mc.rows_check()
    assert ls == ld == lg, (ls, ld, lg)
    assert set(gs) == set(gd) == set(gg)
    tower = {"rpn.head.conv.0.0.weight", "rpn.head.conv.1.0.weight", "rpn.head.cls_logits.weight",
             "rpn.head.bbox_pred.weight"}
    for n in gs:
        if n in tower:
            assert gd[n].abs().max() > 0, n
        assert torch.equal(gs[n], gd[n]), n
        assert torch.equal(gs[n], gg[n]), n
