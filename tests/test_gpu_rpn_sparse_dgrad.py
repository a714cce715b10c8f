"""Listed-rows backward of the RPN head: mx_conv2d_dgrad_x3_rows, mx_act_bias_bwd_rows, mx_rpn_lists_build
and their wiring (conv.RowLists sparse=True, conv.MaskMul, MX_RPN_SPARSE_BWD = 1 / wgrad / 0).

Everything here is an equality: a rows form computes, for each listed pixel, the sum the dense launch of
the same shape and cfg computes, in its order, and leaves every other row alone; the listed-rows
activation pass keeps the dense launch's grid, lanes and partials. So the checks are torch.equal
against the dense entry on a gradient that is zero off the list -- no tolerance -- plus NaN canaries
for what must stay untouched or unread."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_rpn_sparse import B, GUARD, _build, _canvas_hw, _grad_map, _head, _patterns, _step

pytestmark = pytest.mark.gpu

N = 2
CAP = 160     # static capacity of the kernel-level lists (>= 129 entries, < the 308 canvas pixels)
PADROWS = 8   # NaN canary rows in front of and behind every output buffer


def _maps():
    return [(13, 21), _canvas_hw()]


def _lists(H, W):
    """name -> (entries written to the device list, the count the device reports)."""
    P = N * H * W
    rng = np.random.default_rng(H * 977 + W)
    pick = lambda n: np.sort(rng.choice(P, n, replace=False)).astype(np.int64)
    over = pick(CAP + 1)
    return {
        "empty": (np.zeros(0, np.int64), 0),
        "corners": (np.array(sorted({0, W - 1, (H - 1) * W, H * W - 1, P - H * W, P - 1}), np.int64), None),
        "image_seam": (np.array([H * W - 1, H * W], np.int64), None),
        "border_row": (np.arange((H - 1) * W, H * W, dtype=np.int64), None),
        "n127": (pick(127), None), "n128": (pick(128), None), "n129": (pick(129), None),
        "capacity": (pick(CAP), None),
        "capacity_plus_1": (over[:CAP], CAP + 1),   # a cut list: the count says one more than was written
    }


def _dev_list(dev, entries, count=None):
    """(list tensor with guard words behind CAP entries, count tensor, CAP); unwritten entries hold the
    guard pattern, an index far outside any test map."""
    buf = torch.full((CAP + 4,), GUARD, dtype=torch.int32)
    buf[:len(entries)] = torch.from_numpy(np.asarray(entries, np.int64)).to(torch.int32)
    cnt = torch.tensor([len(entries) if count is None else count], dtype=torch.int32)
    return buf.to(dev), cnt.to(dev), CAP


def _cfgs():
    from mx_det import _lib
    # 128 x 128 unsplit (the headline tower dgrads' instance), the library default of the shape, and the
    # 64 x 128 unsplit instance (what the default picks for maps between 320 and 512 row tiles)
    return {"t128": _lib.ConvCfg(128, 128, 1, 0, 3, 0, 0), "default": None, "t64": _lib.ConvCfg(64, 128, 1, 0, 3, 0, 0)}


class _Dgrad:
    """The 3x3 stride-1 f32 dgrad of one shape through the C entries, dense and rows form."""

    def __init__(self, dev, H, W, C, seed):
        from mx_det import _lib, conv as mc
        self.lib, self.call, self.st = _lib.load(), _lib.call, _lib.stream
        self.dev, self.H, self.W, self.C, self.P = dev, H, W, C, N * H * W
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)
        _, self.wt = mc.pack_weight(w, C, (1, 1), (1, 1), kpad=C, krsc=False, dgrad=True, split=True)
        self.sh = _lib.ConvShape(N, H, W, C, C, 3, 3, H, W, 1, 1, 1, 1)
        self.gen = g

    def supported(self, cfg):
        return bool(self.lib.mx_conv2d_dgrad_x3_rows_supported(ctypes.byref(self.sh), cfg))

    def dense(self, dy, res, cfg):
        dx = torch.empty(N, self.H, self.W, self.C, device=self.dev)
        wsb = self.lib.mx_conv_workspace_x3(ctypes.byref(self.sh), 1, cfg)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=self.dev)
        self.call("mx_conv2d_dgrad_x3", ctypes.byref(self.sh), dy.data_ptr(), self.wt.data_ptr(),
                  res.data_ptr() if res is not None else None, dx.data_ptr(), None, None, None, None, 0, None, 0,
                  ws.data_ptr() if wsb else None, wsb, self.st(), cfg)
        return dx

    def rows(self, dy, res_ptr, out, lst, cfg):
        self.call("mx_conv2d_dgrad_x3_rows", ctypes.byref(self.sh), dy.data_ptr(), self.wt.data_ptr(), res_ptr,
                  out.data_ptr(), lst[0].data_ptr(), lst[1].data_ptr(), lst[2], self.st(), cfg)

    def canary(self):
        """A NaN-filled buffer of PADROWS + P + PADROWS rows and the view of its P map rows."""
        buf = torch.full((self.P + 2 * PADROWS, self.C), float("nan"), device=self.dev)
        return buf, buf[PADROWS:PADROWS + self.P]


@pytest.mark.parametrize("C", [32, 64, 256])
@pytest.mark.parametrize("mi", [0, 1])
def test_rows_dgrad_equals_dense_on_listed_rows(dev, C, mi):
    """For every list and cfg with a rows form: listed rows == the dense dgrad of the zero-off-list
    gradient (with and without a residual, out of place and in place); every other row, the canary rows
    around the buffer included, is untouched; rows past a cut list's capacity are not computed."""
    H, W = _maps()[mi]
    d = _Dgrad(dev, H, W, C, 100 + C + mi)
    P = d.P
    ran = 0
    for cname, cfg in _cfgs().items():
        if not d.supported(cfg):
            assert cname == "default", (cname, C, H, W)  # split K on these small maps: the caller runs densely
            continue
        for name, (ent, count) in _lists(H, W).items():
            lst = _dev_list(dev, ent, count)
            idx = torch.from_numpy(ent).to(dev)
            dy = torch.zeros(P, C)
            dy[ent] = torch.randn(len(ent), C, generator=d.gen)
            dy = dy.to(dev).view(N, H, W, C)
            rvals = torch.randn(len(ent), C, generator=d.gen).to(dev)
            res = torch.zeros(P, C, device=dev)
            res[idx] = rvals
            ref = d.dense(dy, None, cfg).view(P, C)
            ref_res = d.dense(dy, res.view(N, H, W, C), cfg).view(P, C)
            unlisted = torch.ones(P, dtype=torch.bool, device=dev)
            unlisted[idx] = False
            # no residual, into a NaN buffer
            buf, out = d.canary()
            d.rows(dy, None, out, lst, cfg)
            assert torch.equal(out[idx], ref[idx]), (cname, name)
            assert bool(torch.isnan(out[unlisted]).all()) and bool(torch.isnan(buf[:PADROWS]).all()) and \
                bool(torch.isnan(buf[PADROWS + P:]).all()), (cname, name)
            # residual read from another buffer
            buf, out = d.canary()
            d.rows(dy, res.data_ptr(), out, lst, cfg)
            assert torch.equal(out[idx], ref_res[idx]), (cname, name)
            assert bool(torch.isnan(out[unlisted]).all()), (cname, name)
            # in place: the residual buffer takes the rows; NaN canaries on every unlisted row
            buf, out = d.canary()
            out[idx] = rvals
            d.rows(dy, out.data_ptr(), out, lst, cfg)
            assert torch.equal(out[idx], ref_res[idx]), (cname, name)
            assert bool(torch.isnan(out[unlisted]).all()) and bool(torch.isnan(buf[:PADROWS]).all()) and \
                bool(torch.isnan(buf[PADROWS + P:]).all()), (cname, name)
            assert bool((lst[0][CAP:] == GUARD).all())
            ran += 1
    assert ran == 2 * len(_lists(H, W))  # both unsplit tiles ran every list


def test_rows_dgrad_out_of_range_entries_store_nothing(dev):
    """An entry outside [0, P) is a masked row: nothing is read or stored for it, its neighbours in the
    list are computed as usual."""
    H, W = 13, 21
    d = _Dgrad(dev, H, W, 64, 7)
    P = d.P
    cfg = _cfgs()["t128"]
    ent = np.array([-1, 3, 7, P, P + 5, 0x7FFFFFFF], np.int64)
    good = torch.tensor([3, 7], device=dev)
    lst = _dev_list(dev, ent)
    dy = torch.randn(N, H, W, 64, generator=d.gen).to(dev)
    ref = d.dense(dy, None, cfg).view(P, 64)
    buf, out = d.canary()
    d.rows(dy, None, out, lst, cfg)
    assert torch.equal(out[good], ref[good])
    keep = torch.ones(P + 2 * PADROWS, dtype=torch.bool, device=dev)
    keep[good + PADROWS] = False
    assert bool(torch.isnan(buf[keep]).all())


def test_conv_dgrad_rows_wrapper_default_cfg(dev, monkeypatch):
    """conv.conv_dgrad(rows=...) under the library default of a small map (split K: no rows form) runs the
    dense launch; under a map whose default is an unsplit 64 x 128 tile, the rows form -- both equal the
    dense result on the listed rows, zero-filled elsewhere."""
    from mx_det import conv as mc
    monkeypatch.setenv("MX_CONV_TUNE", "0")
    for (H, W, C, sup) in ((13, 21, 256, False), (104, 100, 128, True)):
        d = _Dgrad(dev, H, W, C, 11)
        assert d.supported(None) == sup, (H, W, C)
        P = d.P
        ent = np.sort(np.random.default_rng(5).choice(P, 129, replace=False)).astype(np.int64)
        lst = _dev_list(dev, ent)
        dy = torch.zeros(P, C)
        dy[ent] = torch.randn(len(ent), C, generator=d.gen)
        dy = dy.to(dev).view(N, H, W, C)
        ref = mc.conv_dgrad(dy, d.wt, (N, H, W, C), 3, 3, (1, 1), (1, 1)).view(P, C)
        got = mc.conv_dgrad(dy, d.wt, (N, H, W, C), 3, 3, (1, 1), (1, 1), rows=lst).view(P, C)
        idx = torch.from_numpy(ent).to(dev)
        assert torch.equal(got[idx], ref[idx])
        if sup:
            rest = torch.ones(P, dtype=torch.bool, device=dev)
            rest[idx] = False
            assert bool((got[rest] == 0).all())


# ------------------------------------------------------------------------------------- act pass
@pytest.mark.parametrize("K", [32, 64, 256])
@pytest.mark.parametrize("mi", [0, 1])
def test_act_rows_equals_dense(dev, K, mi):
    """Written rows and db equal mx_act_bias_bwd on the zero-off-list gradient, with and without the frame
    mask; unlisted rows of gy are never read (NaN there) and of g never written (NaN canaries); two
    runs on one workspace agree."""
    from mx_det import conv as mc
    H, W = _maps()[mi]
    P = N * H * W
    g = torch.Generator().manual_seed(300 + K + mi)
    y = torch.randn(N, H, W, K, generator=g).to(dev)
    mask = (torch.rand(1, H, W, 1, generator=g) < 0.7).float().to(dev)
    for name, (ent, count) in _lists(H, W).items():
        lst = _dev_list(dev, ent, count)
        idx = torch.from_numpy(ent).to(dev)
        gy = torch.zeros(P, K)
        gy[ent] = torch.randn(len(ent), K, generator=g)
        gy = gy.to(dev)
        unlisted = torch.ones(P, dtype=torch.bool, device=dev)
        unlisted[idx] = False
        gy_nan = gy.clone()
        gy_nan[unlisted] = float("nan")
        for m in (None, mask):
            gyd = gy.view(N, H, W, K) if m is None else gy.view(N, H, W, K) * m
            ref_g, ref_db = mc.act_bias_bwd(gyd, y, mc.ACT_RELU, K, True, g_dtype=torch.float32)
            outs = []
            for _ in range(2):
                buf = torch.full((P + 2 * PADROWS, K), float("nan"), device=dev)
                out = buf[PADROWS:PADROWS + P]
                db = torch.full((K,), float("nan"), device=dev)
                ws = mc.bn_scratch(mc._lib.load().mx_act_bias_bwd_workspace(P, K), dev)
                mc.call("mx_act_bias_bwd_rows", gy_nan.data_ptr(), y.data_ptr(), m.data_ptr() if m is not None else None,
                        H * W if m is not None else 0, P, K, lst[0].data_ptr(), lst[1].data_ptr(), lst[2],
                        out.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), mc._s())
                assert torch.equal(out[idx], ref_g.view(P, K)[idx]), (name, m is not None)
                assert torch.equal(db, ref_db), (name, m is not None)
                assert bool(torch.isnan(out[unlisted]).all()) and bool(torch.isnan(buf[:PADROWS]).all()) and \
                    bool(torch.isnan(buf[PADROWS + P:]).all()), (name, m is not None)
                outs.append((out[idx].clone(), db.clone()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        # the Python wrapper: one fill, then the rows
        got_g, got_db = mc.act_bias_bwd_rows(gy_nan.view(N, H, W, K), y, True, lst, mask)
        ref_g, ref_db = mc.act_bias_bwd(gy.view(N, H, W, K) * mask, y, mc.ACT_RELU, K, True, g_dtype=torch.float32)
        assert torch.equal(got_g, ref_g) and torch.equal(got_db, ref_db), name


# ------------------------------------------------------------------------------------ list build
@pytest.mark.parametrize("hw", [(5, 7), (13, 21), "canvas"])
def test_lists_build_equals_the_two_entries(dev, hw):
    """mx_rpn_lists_build's pixel lists and K-step lists are mx_rpn_rows_build's and mx_rpn_tiles_build's:
    entries, counts, cut at the capacity with guard words intact, and the flag."""
    from mx_det import _lib
    lib = _lib.load()
    A5 = 15
    H, W = _canvas_hw() if hw == "canvas" else hw
    P = N * H * W
    NB, NBT = max(W, 6), 2
    caps = [lib.mx_rpn_rows_capacity(P, NB, l) for l in range(3)]
    tcaps = [lib.mx_rpn_tiles_capacity(P, NBT, l) for l in range(3)]
    rng = np.random.default_rng(3)
    for name, m0 in _patterns(N, H, W, caps[0]).items():
        g = np.zeros((N, H, W, A5), np.float32)
        ch = rng.integers(0, A5, size=(N, H, W))
        np.put_along_axis(g, ch[..., None], np.where(m0, 1.5, 0.0)[..., None].astype(np.float32), 3)
        if name == "all":
            g[:] = 1.0
        gd = torch.from_numpy(g).to(dev)
        rl, rc, rf, ok1 = _build(dev, gd, caps, "mx_rpn_rows_build")
        tl, tc, tf, ok2 = _build(dev, gd, tcaps, "mx_rpn_tiles_build")
        assert ok1 and ok2
        sizes = caps + tcaps[:2]
        offs, o = [], 0
        for c in sizes:
            offs.append(o)
            o += c + 4
        buf = torch.full((o + 3 + 4 + 2 + 4,), GUARD, dtype=torch.int32, device=dev)
        wsb = lib.mx_rpn_rows_workspace(P)
        ws = torch.full((wsb + 64,), 0x5A, dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr = [buf[a:].data_ptr() for a in offs]
        cnt, tcnt = o, o + 3 + 4
        _lib.call("mx_rpn_lists_build", gd.data_ptr(), N, H, W, A5, ptr[0], caps[0], ptr[1], caps[1], ptr[2], caps[2],
                  buf[cnt:].data_ptr(), ptr[3], tcaps[0], ptr[4], tcaps[1], buf[tcnt:].data_ptr(), flag.data_ptr(),
                  ws.data_ptr(), wsb, _lib.stream())
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        for l in range(3):
            assert np.array_equal(b[offs[l]:offs[l] + caps[l]], rl[l]), (name, l)
            assert (b[offs[l] + caps[l]:offs[l] + caps[l] + 4] == GUARD).all(), (name, l)
        for l in range(2):
            assert np.array_equal(b[offs[3 + l]:offs[3 + l] + tcaps[l]], tl[l]), (name, l)
            assert (b[offs[3 + l] + tcaps[l]:offs[3 + l] + tcaps[l] + 4] == GUARD).all(), (name, l)
        assert np.array_equal(b[cnt:cnt + 3], rc) and np.array_equal(b[tcnt:tcnt + 2], tc[:2]), name
        assert (b[cnt + 3:tcnt] == GUARD).all() and (b[tcnt + 2:] == GUARD).all() and bool((ws[wsb:] == 0x5A).all())
        # the flag: any of the five lists it builds overflowed (S2's K-steps are not among them)
        over = any(rc[l] > caps[l] for l in range(3)) or any(tc[l] > tcaps[l] for l in range(2))
        assert int(flag) == int(over), (name, int(flag), rc, tc)


# --------------------------------------------------------------------------------- head level
MODES = ("1", "wgrad", "0")


def _run_head_mode(h, x, gout, mode, monkeypatch, poison=False):
    """test_gpu_rpn_sparse._run_head with the switch's three values; poison: freshly freed NaN blocks of
    every intermediate's size sit in the allocator when the backward starts."""
    from mx_det.backend import HipBackend
    monkeypatch.setenv("MX_RPN_SPARSE_BWD", mode)
    monkeypatch.setenv("MX_CONV_TUNE", "0")
    h.__dict__["sparse_rows_per_image"] = B
    be = HipBackend("f32")
    for p in h.parameters():
        p.grad = None
    xd = x.detach().clone().requires_grad_(True)
    w = torch.cat([h.cls_logits.weight, h.bbox_pred.weight])
    b = torch.cat([h.cls_logits.bias, h.bbox_pred.bias])
    y = h._run(xd, be, w, b)
    if poison:
        torch.cuda.synchronize()
        px = x.numel() // x.shape[3]
        blocks = [torch.full((px * c,), float("nan"), device=x.device) for c in (x.shape[3], 16) for _ in range(4)]
        torch.cuda.synchronize()
        del blocks
    y.backward(gout)
    torch.cuda.synchronize()
    out = {n: p.grad.detach().clone() for n, p in h.named_parameters()}
    out["dx"] = xd.grad.detach().clone()
    return out


# (32, 13, 21): the default dgrad splits K, so the dgrads run densely behind the listed-rows passes;
# (128, 104, 100): 325 row tiles of 64 x 128, unsplit -- the rows-form dgrads run
@pytest.mark.parametrize("C,H,W", [(32, 13, 21), (128, 104, 100)])
def test_head_backward_three_modes_equal(dev, monkeypatch, C, H, W):
    from mx_det import conv as mc
    h = _head(dev, C)
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(1)).to(dev)
    for k in (0, 1, 37, N * B):
        gout = _grad_map(N, H, W, k, 10 + k).to(dev)
        runs = {m: _run_head_mode(h, x, gout, m, monkeypatch) for m in MODES}
        again = _run_head_mode(h, x, gout, "1", monkeypatch)
        poisoned = _run_head_mode(h, x, gout, "1", monkeypatch, poison=True)
        mc.rows_check()
        for n in runs["0"]:
            for m in ("1", "wgrad"):
                assert torch.equal(runs[m][n], runs["0"][n]), (k, m, n)
            assert torch.equal(again[n], runs["0"][n]), (k, n)
            assert torch.equal(poisoned[n], runs["0"][n]), (k, n)  # nothing depends on what the allocator held
        if k:
            assert runs["0"]["dx"].abs().max() > 0 and runs["0"]["conv.0.0.bias"].abs().max() > 0


def test_head_backward_128_row_tile(dev, monkeypatch):
    """A map of 518 row tiles of 128 x 128: the default pick is the headline instance."""
    C, H, W = 128, 184, 180
    assert _Dgrad(dev, H, W, C, 1).supported(None)
    h = _head(dev, C)
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(1)).to(dev)
    gout = _grad_map(N, H, W, 37, 47).to(dev)
    sp = _run_head_mode(h, x, gout, "1", monkeypatch)
    de = _run_head_mode(h, x, gout, "0", monkeypatch)
    for n in de:
        assert torch.equal(sp[n], de[n]), n


def test_graph_replay_matches_eager(dev, monkeypatch):
    """One capture (ones_like warm-ups overflow the lists by design), replayed for k = 5, 0 and the
    capacity in that order: each replay's gradients are the eager dense ones."""
    from mx_det import conv as mc, frcnn
    from mx_det.backend import HipBackend
    monkeypatch.setenv("MX_RPN_SPARSE_BWD", "1")
    monkeypatch.setenv("MX_CONV_TUNE", "0")
    C, H, W = 128, 104, 100
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
    assert int(mc._rows_flags[dev.index][0]) == 0
    mc.rows_check()
    for k in (5, 0, N * B):
        gout = _grad_map(N, H, W, k, 20 + k).to(dev)
        eager = _run_head_mode(h, x, gout, "0", monkeypatch)
        monkeypatch.setenv("MX_RPN_SPARSE_BWD", "1")
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


def test_canvas_path_with_mask_three_modes_equal(dev, monkeypatch):
    """RPNHead.raw on five levels: level 0 alone and the canvas of the small levels with its frame mask
    (conv.MaskMul hands it to the listed-rows pass); every parameter and feature gradient equal under
    1, wgrad and 0."""
    from mx_det import conv as mc
    from mx_det.backend import HipBackend
    C = 32
    hws = [(26, 42), (13, 21), (7, 11), (4, 6), (2, 3)]
    h = _head(dev, C)
    h.__dict__["sparse_rows_per_image"] = B
    gen = torch.Generator().manual_seed(9)
    feats0 = [torch.randn(N, a, b, C, generator=gen).to(dev) for a, b in hws]
    monkeypatch.setenv("MX_CONV_TUNE", "0")
    res = {}
    gouts = None
    for m in MODES:
        monkeypatch.setenv("MX_RPN_SPARSE_BWD", m)
        for p in h.parameters():
            p.grad = None
        feats = [f.detach().clone().requires_grad_(True) for f in feats0]
        r0, r1 = h.raw(feats, HipBackend("f32"))
        if gouts is None:
            gouts = [_grad_map(N, r.shape[1], r.shape[2], 31, 60 + i).to(dev) for i, r in enumerate((r0, r1))]
        torch.autograd.backward([r0, r1], gouts)
        torch.cuda.synchronize()
        out = {n: p.grad.detach().clone() for n, p in h.named_parameters()}
        out.update({f"feat{i}": f.grad.detach().clone() for i, f in enumerate(feats)})
        res[m] = out
    mc.rows_check()
    for n in res["0"]:
        assert res["0"][n].abs().max() > 0, n
        for m in ("1", "wgrad"):
            assert torch.equal(res[m][n], res["0"][n]), (m, n)


def test_model_step_three_modes_eager_and_graphed(dev, monkeypatch):
    """One 2 x 256 x 320 train step: losses and every parameter gradient equal under 1, wgrad and 0, eager
    and graphed."""
    from mx_det import conv as mc, frcnn
    from mx_det.data import synth_batch
    torch.manual_seed(0)
    base = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    base.roi_heads.box_predictor = frcnn.FastRCNNPredictor(1024, 7)
    frcnn.set_trainable_layers(base.backbone.body, 3)
    base = base.to(dev).train()
    imgs, tg = synth_batch(0, 2, H=256, W=320, device=dev)
    ref_l, ref_g = _step(dev, base, imgs, tg, monkeypatch, "0", "0")
    for mode in MODES:
        for graphs in ("0", "1"):
            if (mode, graphs) == ("0", "0"):
                continue
            l, g = _step(dev, base, imgs, tg, monkeypatch, mode, graphs)
            assert l == ref_l, (mode, graphs, l, ref_l)
            assert set(g) == set(ref_g)
            for n in g:
                assert torch.equal(g[n], ref_g[n]), (mode, graphs, n)
    mc.rows_check()
    assert ref_g["rpn.head.conv.0.0.weight"].abs().max() > 0
