"""Edge cases of the small kernels against torch / numpy on the CPU: mx_pool.hip (max-pool, nearest
upsample + add), mx_unet.hip (up-concat, reflect pad, restore finish) and the fused RPN / RoI losses.

References are computed on the CPU from the same values (bf16 inputs as their exact f32 values). Every
backward case uses integer-valued gradients in [-2, 2]: their sums are exact in f32 and round once to
bf16, so every pool / upsample / copy comparison is bit-exact.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
NINF = float("-inf")


def _same(a, b):
    """Element-wise equal, NaN == NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _int_grad(shape, g):
    return torch.randint(-2, 3, shape, generator=g).float()


# ---------------------------------------------------------------------------------------- max-pool
POOL_CFGS = [(3, 2, 1), (2, 2, 0), (1, 2, 0)]  # ResNet stem, U-Net, P6 (LastLevelMaxPool)
POOL_HW = [(7, 9), (8, 8), (5, 6), (1, 1)]


def _pool_out(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def pool_input(kind, N, H, W, C, k, g):
    """NHWC f32 input of one max-pool case (every value exact in bf16)."""
    if kind == "ties":
        # {0, 1, 2}, mostly zeros, laid out in 2x2 blocks of one value with a quarter of the entries
        # redrawn: most windows hold their maximum more than once
        pr = torch.tensor([0.6, 0.2, 0.2])
        hb, wb = (H + 1) // 2, (W + 1) // 2
        blk = torch.multinomial(pr, N * hb * wb * C, True, generator=g).view(N, hb, wb, C)
        x = blk.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W].clone()
        iid = torch.multinomial(pr, N * H * W * C, True, generator=g).view(N, H, W, C)
        x = torch.where(torch.rand(N, H, W, C, generator=g) < 0.25, iid, x)
        return x.float()
    x = torch.randint(-3, 4, (N, H, W, C), generator=g).float()
    r = torch.rand(N, H, W, C, generator=g)
    if kind == "ninf":
        x[r < 0.3] = NINF
        x[:, :3, :3] = NINF  # the first window of every configuration is entirely -inf
        return x
    assert kind == "nan"
    x[r < 0.12] = NAN
    if k > 1 and H >= 4 and W >= 4:
        # the window of output (1, 1) is rows / columns 1..3 (k3 s2 p1) or 2..3 (k2 s2): NaN at its
        # first, a middle and its last position, and two NaNs in one window (channels 0..3)
        lo = 1 if k == 3 else 2
        x[0, lo:4, lo:4, :4] = 1.0
        x[0, lo, lo, 0] = NAN
        x[0, lo + (k == 3), 3, 1] = NAN
        x[0, 3, 3, 2] = NAN
        x[0, lo, lo, 3] = NAN
        x[0, 3, 3, 3] = NAN
    return x


def tie_fraction(x, k, s, p):
    """Fraction of the pooling windows (per channel) that hold their maximum at least twice."""
    xc = F.pad(x.permute(0, 3, 1, 2), (p, p, p, p), value=NINF)
    win = xc.unfold(2, k, s).unfold(3, k, s).reshape(*xc.shape[:2], -1, k * k)
    mx = win.max(-1, keepdim=True).values
    return ((win == mx).sum(-1) >= 2).float().mean().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["ties", "ninf", "nan"])
@pytest.mark.parametrize("k,s,p", POOL_CFGS)
def test_maxpool_edges(dev, k, s, p, kind, dtype):
    """mx_maxpool_fwd / _bwd == F.max_pool2d(return_indices=True) and its autograd: values (NaN-aware),
    the int32 argmax (torch's flat h*W + w: the first maximum on ties, the first valid position of an
    all -inf window, the last NaN), and the gradient, bit-exact."""
    from mx_det.backend import _MaxPool
    g = torch.Generator().manual_seed(100 * k + 10 * len(kind) + (dtype == torch.bfloat16))
    N = 2
    ran = 0
    for H, W in POOL_HW:
        Ho, Wo = _pool_out(H, W, k, s, p)
        if Ho < 1 or Wo < 1:
            continue  # (1, 1) under k2: no output
        for C in (8, 24):
            x = pool_input(kind, N, H, W, C, k, g)
            assert torch.equal(x.to(dtype).float().nan_to_num(7.0), x.nan_to_num(7.0))
            if kind == "ties" and k > 1 and H * W > 1:  # a one-element window cannot hold a tie
                assert tie_fraction(x, k, s, p) >= 0.5, (H, W, C, tie_fraction(x, k, s, p))
            xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
            yr, ir = F.max_pool2d(xr, k, s, p, return_indices=True)
            if kind == "ninf":
                assert bool((yr == NINF).any()), "no window entirely -inf"
            if kind == "nan" and k > 1 and H >= 4:
                assert bool(yr[0, :4, 1, 1].isnan().all())
            gy = _int_grad(yr.shape, g)
            yr.backward(gy)
            xd = x.to(dev, dtype).requires_grad_(True)
            y = _MaxPool.apply(xd, k, s, p)
            (arg,) = y.grad_fn.saved_tensors
            y.backward(gy.permute(0, 2, 3, 1).contiguous().to(dev, dtype))
            tag = (H, W, C)
            assert y.dtype == dtype and _same(y.float().cpu(), yr.detach().permute(0, 2, 3, 1)), tag
            assert arg.dtype == torch.int32 and torch.equal(arg.cpu().long(), ir.permute(0, 2, 3, 1)), tag
            gx = xd.grad
            ref = xr.grad.permute(0, 2, 3, 1).to(dtype)  # exact f32 sums, rounded once
            assert gx.dtype == dtype and torch.equal(gx.cpu(), ref), tag
            if k == 2 and H % 2:  # the last row is in no window
                assert bool((gx[:, H - 1] == 0).all()), tag
            if k == 2 and W % 2:
                assert bool((gx[:, :, W - 1] == 0).all()), tag
            ran += 1
    assert ran == (6 if k == 2 else 8)


# --------------------------------------------------------------------------------- nearest upsample
UP_SIZES = [((13, 21), (25, 42)), ((6, 2), (74, 82)), ((3, 4), (123, 94)), ((5, 5), (5, 5)), ((1, 1), (7, 3)),
            ((9, 10), (4, 3))]


def near_src_f32(d, n_in, n_out):
    """min(floor(d * f32(in / out)), in - 1) with the product in f32: F.interpolate(mode="nearest")."""
    sc = np.float32(n_in) / np.float32(n_out)
    return min(int(np.floor(np.float32(d) * sc)), n_in - 1)


def f32_index_differs(n_in, n_out):
    """Destinations whose f32 source index differs from the integer form d * in // out."""
    return [d for d in range(n_out) if near_src_f32(d, n_in, n_out) != min(d * n_in // n_out, n_in - 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("src,dst", UP_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_upsample_add_edges(dev, src, dst, with_add, dtype):
    """mx_upsample_nearest_fwd / _bwd == F.interpolate(mode="nearest", size=...) (+ add) and its
    autograd, bit-exact: 2x-and-odd FPN sizes, sizes where the f32 scale of the source index differs
    from integer arithmetic (6 -> 74 at d = 37, 2 -> 82 at 41, 3 -> 123 at 41 and 82, 4 -> 94 at 47),
    the identity, a 1x1 source, and a downsample (never issued by the model, accepted by the entry)."""
    from mx_det.backend import _UpsampleAdd
    (H, W), (Ho, Wo) = src, dst
    if src == (6, 2):
        assert f32_index_differs(6, 74) == [37] and f32_index_differs(2, 82) == [41]
    if src == (3, 4):
        assert f32_index_differs(3, 123) == [41, 82] and f32_index_differs(4, 94) == [47]
    g = torch.Generator().manual_seed(H * 1000 + Wo + with_add)
    N = 2
    for C in (8, 16):
        x = torch.randint(-64, 65, (N, H, W, C), generator=g).float()
        a = torch.randint(-64, 65, (N, Ho, Wo, C), generator=g).float() if with_add else None
        gy = _int_grad((N, Ho, Wo, C), g)
        xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        ur = F.interpolate(xr, size=(Ho, Wo), mode="nearest")
        if (H, W) != (Ho, Wo):  # torch's own kernel follows the f32 index (checked where it matters)
            ih = [near_src_f32(d, H, Ho) for d in range(Ho)]
            iw = [near_src_f32(d, W, Wo) for d in range(Wo)]
            assert torch.equal(ur.detach(), xr.detach()[:, :, ih][:, :, :, iw])
        ur.backward(gy.permute(0, 3, 1, 2))
        yr = ur.detach().permute(0, 2, 3, 1) + (a if with_add else 0)
        xd = x.to(dev, dtype).requires_grad_(True)
        ad = a.to(dev, dtype).requires_grad_(True) if with_add else None
        y = _UpsampleAdd.apply(xd, ad, Ho, Wo)
        y.backward(gy.to(dev, dtype))
        assert y.dtype == dtype and torch.equal(y.detach().float().cpu(), yr), C  # |sums| <= 128: exact in bf16
        ref = xr.grad.permute(0, 2, 3, 1).to(dtype)  # exact f32 sums, rounded once
        assert xd.grad.dtype == dtype and torch.equal(xd.grad.cpu(), ref), C
        if with_add:
            assert torch.equal(ad.grad.float().cpu(), gy), C


# --------------------------------------------------------------------------------------- up-concat
GUARD = 64  # elements: 128 B (bf16) / 256 B (f32), keeps the kernels' 16-B vector alignment


def _carved(numel, dtype, dev):
    """(buffer, view): `numel` elements in the middle of a NaN-filled buffer."""
    buf = torch.full((numel + 2 * GUARD,), NAN, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf):
    return bool(buf[:GUARD].isnan().all()) and bool(buf[-GUARD:].isnan().all())


def up_concat_ref(up, skip):
    N, H, W, C4 = up.shape
    Cu = C4 // 4
    return torch.cat([up.view(N, H, W, 2, 2, Cu).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Cu), skip], 3)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cs", [8, 16])
@pytest.mark.parametrize("Cu", [8, 24])
def test_up_concat_edges(dev, Cu, Cs, dtype):
    """mx_up_concat / mx_up_concat_bwd == plain indexing (the (i, j, co) channel order of the
    transposed conv scattered to (2h+i, 2w+j), concatenated with the skip map) and its transpose,
    with and without gskip. Outputs lie in the middle of NaN-filled buffers: every output element is
    written (no NaN left) and nothing before or after them is."""
    from mx_det import _lib
    from mx_det import conv as mc
    g = torch.Generator().manual_seed(Cu * 100 + Cs)
    N, H, W = 2, 3, 5
    Co = Cu + Cs
    up = torch.randn(N, H, W, 4 * Cu, generator=g).to(dtype)
    skip = torch.randn(N, 2 * H, 2 * W, Cs, generator=g).to(dtype)
    upd, skd = up.to(dev), skip.to(dev)
    buf, out = _carved(N * 4 * H * W * Co, dtype, dev)
    _lib.call("mx_up_concat", upd.data_ptr(), skd.data_ptr(), mc.dcode(upd), N, H, W, Cu, Cs, out.data_ptr(),
              _lib.stream())
    ref = up_concat_ref(up, skip)
    assert torch.equal(out.view(N, 2 * H, 2 * W, Co).cpu(), ref)
    assert _guards_intact(buf)
    gc = _int_grad((N, 2 * H, 2 * W, Co), g).to(dtype)
    gcd = gc.to(dev)
    gup_ref = gc[..., :Cu].reshape(N, H, 2, W, 2, Cu).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, 4 * Cu)
    # the transpose of the forward: <up_concat(u, s), g> == <u, gup> + <s, gskip>
    assert float((ref.double() * gc.double()).sum()) == pytest.approx(
        float((up.double() * gup_ref.double()).sum() + (skip.double() * gc[..., Cu:].double()).sum()), abs=1e-6)
    for with_gskip in (True, False):
        bu, gup = _carved(N * H * W * 4 * Cu, dtype, dev)
        bs, gsk = _carved(N * 4 * H * W * Cs, dtype, dev)
        _lib.call("mx_up_concat_bwd", gcd.data_ptr(), mc.dcode(gcd), N, H, W, Cu, Cs, gup.data_ptr(),
                  gsk.data_ptr() if with_gskip else None, _lib.stream())
        assert torch.equal(gup.view(N, H, W, 4 * Cu).cpu(), gup_ref), with_gskip
        assert _guards_intact(bu) and _guards_intact(bs)
        if with_gskip:
            assert torch.equal(gsk.view(N, 2 * H, 2 * W, Cs).cpu(), gc[..., Cu:])
        else:
            assert bool(gsk.isnan().all())  # not passed, not written


# ------------------------------------------------------------------------------------- reflect pad
PAD_SIZES = [((45, 70), (48, 80)), ((1, 1), (16, 16)), ((3, 2), (16, 16)), ((2, 5), (16, 16)), ((16, 16), (16, 16))]


def reflect_pad_ref(img, Hp, Wp):
    B, H, W, _ = img.shape
    return np.pad(img, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0)), mode="symmetric")


@pytest.mark.parametrize("src,dst", PAD_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_reflect_pad_edges(dev, src, dst):
    """mx_reflect_pad_u8 == np.pad(mode="symmetric") at the bottom / right (cv2 BORDER_REFLECT): a
    size of 1, a pad several times the size (the reflection folds back and forth), and no pad."""
    from mx_det import _lib
    (H, W), (Hp, Wp) = src, dst
    rng = np.random.default_rng(H * 100 + W)
    img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    n = 2 * Hp * Wp * 3
    buf = torch.full((n + 2 * GUARD,), 171, dtype=torch.uint8, device=dev)
    out = buf[GUARD:GUARD + n]
    s = torch.from_numpy(img).to(dev)
    _lib.call("mx_reflect_pad_u8", s.data_ptr(), 2, H, W, 3, Hp, Wp, out.data_ptr(), _lib.stream())
    assert np.array_equal(out.view(2, Hp, Wp, 3).cpu().numpy(), reflect_pad_ref(img, Hp, Wp))
    assert bool((buf[:GUARD] == 171).all()) and bool((buf[-GUARD:] == 171).all())


# ---------------------------------------------------------------------------------- restore finish
def restore_finish_ref(img, res, H, W):
    v = img.astype(np.float32) / np.float32(255.0) + res
    v = (v.clip(np.float32(0), np.float32(1)) * np.float32(255.0)).clip(np.float32(0), np.float32(255))
    assert v.dtype == np.float32
    return v.astype(np.uint8)[:, :H, :W]


def restore_finish_case():
    """(padded image, residual): sums exactly on, just below and just above k/255, below 0, above 1
    and ordinary ones; the padded rows / columns hold 255 + 1.0 (255 wherever the crop indexed them)."""
    rng = np.random.default_rng(7)
    B, Hp, Wp, H, W = 2, 48, 80, 45, 70
    img = rng.integers(0, 256, (B, Hp, Wp, 3), dtype=np.uint8)
    x = img.astype(np.float32) / np.float32(255.0)
    k = rng.integers(0, 256, img.shape).astype(np.float32) / np.float32(255.0)
    on = (k - x).astype(np.float32)
    mode = rng.integers(0, 6, img.shape)
    res = np.select([mode == 0, mode == 1, mode == 2, mode == 3, mode == 4],
                    [on, np.nextafter(on, np.float32(-9)), np.nextafter(on, np.float32(9)),
                     -x - np.float32(0.25), np.float32(1.5) - x],
                    (rng.standard_normal(img.shape) * 0.05).astype(np.float32)).astype(np.float32)
    img[:, H:], img[:, :, W:] = 255, 255
    res[:, H:], res[:, :, W:] = 1.0, 1.0
    return img, res, H, W


def test_restore_finish_edges(dev):
    """mx_restore_finish == the same f32 formula in numpy, bit-exact: u8 / 255f + residual, clamp to
    [0, 1], * 255f, clamp, truncation to uint8, cropped from the padded 48 x 80 to 45 x 70."""
    from mx_det import _lib
    img, res, H, W = restore_finish_case()
    B, Hp, Wp, _ = img.shape
    ref = restore_finish_ref(img, res, H, W)
    # the case holds what it claims: both clamps, exact k/255 sums, and crop-visible padding
    s = img.astype(np.float32) / np.float32(255.0) + res
    assert (s[:, :H, :W] < 0).any() and (s[:, :H, :W] > 1).any()
    assert (ref == 0).any() and (ref == 255).any() and 0.02 < (ref == 255).mean() < 0.5
    n = B * H * W * 3
    buf = torch.full((n + 2 * GUARD,), 171, dtype=torch.uint8, device=dev)
    out = buf[GUARD:GUARD + n]
    si, sr = torch.from_numpy(img).to(dev), torch.from_numpy(res).to(dev)
    _lib.call("mx_restore_finish", si.data_ptr(), B, Hp, Wp, sr.data_ptr(), H, W, out.data_ptr(), _lib.stream())
    got = out.view(B, H, W, 3).cpu().numpy()
    assert np.array_equal(got, ref), (int((got != ref).sum()), "of", ref.size)
    assert bool((buf[:GUARD] == 171).all()) and bool((buf[-GUARD:] == 171).all())


# ------------------------------------------------------------------------------------ fused losses
LOGITS = torch.tensor([-100.0, -30.0, -1e-3, 0.0, 1e-3, 30.0, 100.0])


def _draw_logits(shape, g):
    return LOGITS[torch.randint(0, len(LOGITS), shape, generator=g)]


@pytest.mark.parametrize("positives", [True, False], ids=["pos", "nopos"])
def test_rpn_loss_extreme_logits(dev, positives):
    """ops.rpn_loss at saturating and near-zero logits == torchvision's compute_loss formulation in
    f64 on the CPU (test_rpn_loss_fused_matches_torch's tolerances); with no positive sampled the box
    loss is exactly 0 and grad_deltas all zero. Everything finite."""
    from mx_det import ops
    g = torch.Generator().manual_seed(11)
    N, A = 1, 300
    x = _draw_logits((N, A), g)
    d = torch.randn(N, A, 4, generator=g)
    t = torch.randn(N, A, 4, generator=g)
    lab = torch.randint(-1, 2, (N, A), generator=g).float()
    r = torch.rand(N, A, generator=g)
    pm = (lab == 1) & (r < 0.5) & positives
    nm = (lab == 0) & (r < 0.5)
    assert bool(nm.any()) and bool(pm.any()) == positives
    for v in LOGITS:  # every logit value is sampled
        assert bool(((x == v) & (pm | nm)).any()), float(v)
    xd, dd = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    lo, lb = ops.rpn_loss(xd, dd, lab.to(dev), t.to(dev), pm.to(dev), nm.to(dev), 1.0 / 9)
    (lo * 1.5 + lb * 0.5).backward()
    xr, dr = x.double().requires_grad_(True), d.double().requires_grad_(True)
    sm = pm | nm
    cnt = sm.sum()
    ro = torch.where(sm, F.binary_cross_entropy_with_logits(xr, lab.double().clamp(min=0), reduction="none"),
                     0.0).sum() / cnt
    rb = torch.where(pm, F.smooth_l1_loss(dr, t.double(), beta=1.0 / 9, reduction="none").sum(-1), 0.0).sum() / cnt
    (ro * 1.5 + rb * 0.5).backward()
    got = [lo.detach(), lb.detach(), xd.grad, dd.grad]
    assert all(bool(torch.isfinite(v).all()) for v in got)
    torch.testing.assert_close(lo.detach().cpu().double(), ro.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lb.detach().cpu().double(), rb.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(xd.grad.cpu().double(), xr.grad, rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(dd.grad.cpu().double(), dr.grad, rtol=1e-4, atol=1e-8)
    if not positives:
        assert float(lb.detach()) == 0.0 and bool((dd.grad == 0).all())


@pytest.mark.parametrize("positives", [True, False], ids=["pos", "allbg"])
def test_roi_loss_extreme_logits(dev, positives):
    """ops.roi_loss at saturating and near-zero logits, R = 257 (one RoI past a 256-thread block) ==
    fastrcnn_loss in f64 on the CPU (test_roi_loss_fused_matches_torch's tolerances), on strided views
    of one predictor output; with every label 0 the box loss is exactly 0 and grad_reg all zero."""
    from mx_det import ops
    g = torch.Generator().manual_seed(12)
    R, C = 257, 7
    o = torch.cat([_draw_logits((R, C), g), torch.randn(R, 4 * C, generator=g)], 1)
    lab = torch.randint(0, C, (R,), generator=g)
    lab[torch.rand(R, generator=g) < 0.6] = 0
    lab[R - 1] = 3  # the RoI of the second block is a positive
    if not positives:
        lab.zero_()
    t = torch.randn(R, 4, generator=g)
    od = o.to(dev).requires_grad_(True)
    lc, lb = ops.roi_loss(od[:, :C], od[:, C:], lab.to(dev), t.to(dev), 1.0 / 9)
    (lc * 0.7 + lb * 1.3).backward()
    orf = o.double().requires_grad_(True)
    rc = F.cross_entropy(orf[:, :C], lab)
    reg = orf[:, C:].reshape(R, -1, 4)[torch.arange(R), lab]
    rb = torch.where(lab > 0, F.smooth_l1_loss(reg, t.double(), beta=1.0 / 9, reduction="none").sum(-1), 0.0).sum() / R
    (rc * 0.7 + rb * 1.3).backward()
    assert all(bool(torch.isfinite(v).all()) for v in (lc.detach(), lb.detach(), od.grad))
    torch.testing.assert_close(lc.detach().cpu().double(), rc.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lb.detach().cpu().double(), rb.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(od.grad.cpu().double(), orf.grad, rtol=1e-4, atol=1e-7)
    if not positives:
        assert float(lb.detach()) == 0.0 and bool((od.grad[:, C:] == 0).all())
