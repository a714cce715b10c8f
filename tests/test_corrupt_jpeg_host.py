"""JPEG compression as a corruption, host side (no GPU): the two entry points are declared and bound,
every argument check of mx_corrupt_jpeg_u8 returns before a launch, the workspace is B x the component
planes of mx_jpeg_encode_info, MX_CORRUPTIONS / MX_EXTRA_VARIANTS parse and refuse unknown names, and
the default corruption kinds draw from `random` exactly as before."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mx_corrupt_jpeg_workspace", "mx_corrupt_jpeg_u8")


def test_symbols_declared_exported_and_bound():
    from mx_det import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mx_det.h")).read(), flags=re.S)
    lib = _lib.load()
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, src), s
        assert s in _lib.declared_symbols() and hasattr(lib, s), s


def _call(img=0x10000, B=2, H=40, W=72, q=(15, 90), sub=2, bgr=0, ws=0x40000, ws_bytes=1 << 30, out=0x80000):
    """mx_corrupt_jpeg_u8 with made-up device addresses: a call that is refused never touches them."""
    from mx_det import _lib
    lib = _lib.load()
    arr = (ctypes.c_int32 * max(len(q), 1))(*q) if q is not None else None
    if ws_bytes < 0:
        ws_bytes += lib.mx_corrupt_jpeg_workspace(B, H, W, sub)
        assert ws_bytes > 0
    rc = lib.mx_corrupt_jpeg_u8(img, B, H, W, arr, sub, bgr, ws, ws_bytes, out, None)
    return rc, lib.mx_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(img=None), "null"),
    (dict(out=None), "null"),
    (dict(q=None), "null"),
    (dict(ws=None), "workspace"),
    (dict(q=(15, -1)), "quality"),
    (dict(q=(101, 15)), "quality"),
    (dict(sub=1), "subsampling"),
    (dict(sub=3), "subsampling"),
    (dict(out=0x10000), "out must not be img"),
    (dict(out=0x10000 + 40 * 72 * 3), "overlap"),
    (dict(ws_bytes=-1), "workspace"),  # one byte short of mx_corrupt_jpeg_workspace()
    (dict(H=0), "shape"),
    (dict(W=70000), "65535"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_argument_errors_come_before_any_launch(kw, word):
    rc, msg = _call(**kw)
    assert rc == -1 and word in msg, (rc, msg)


def test_all_quality_zero_is_a_no_op_without_a_workspace():
    assert _call(q=(0, 0), ws=None, ws_bytes=0)[0] == 0
    assert _call(B=0, q=(), ws=None, ws_bytes=0)[0] == 0


@pytest.mark.parametrize("sub", [2, 0])
@pytest.mark.parametrize("hw", [(1, 1), (9, 5), (17, 130), (121, 163), (800, 1333)])
def test_workspace_is_the_planes_of_encode_info(hw, sub):
    from mx_det import _lib, jpeg
    H, W = hw
    lib = _lib.load()
    for q in (15, 95):  # the geometry does not depend on the quality
        info = jpeg.encode_info(W, H, q, sub)
        planes = sum(info.bw[c] * info.bh[c] * 64 for c in range(3))
        for B in (1, 5):
            assert lib.mx_corrupt_jpeg_workspace(B, H, W, sub) == B * planes
        assert planes == lib.mx_jpeg_workspace(ctypes.byref(info))
    assert lib.mx_corrupt_jpeg_workspace(1, H, W, 1) == 0
    assert lib.mx_corrupt_jpeg_workspace(-1, H, W, sub) == 0


def test_mx_corruptions_parses_and_refuses(monkeypatch):
    from mx_det import augment
    monkeypatch.delenv("MX_CORRUPTIONS", raising=False)
    assert augment.env_kinds() == ("noise", "blur", "lowres") == augment.DEFAULT_KINDS
    monkeypatch.setenv("MX_CORRUPTIONS", "noise, jpeg")
    assert augment.env_kinds() == ("noise", "jpeg")
    assert augment.env_kinds("jpeg") == ("jpeg",)
    assert augment.env_kinds(["blur", "jpeg"]) == ("blur", "jpeg")
    monkeypatch.setenv("MX_CORRUPTIONS", "noise,fog")
    with pytest.raises(ValueError):
        augment.env_kinds()
    for bad in (("fog",), ()):
        with pytest.raises(ValueError):
            augment.RandomCorruption(kinds=bad)
        with pytest.raises(ValueError):
            augment.RandomCorruptionGPU(kinds=bad)


def test_mx_extra_variants_parses_and_refuses(monkeypatch):
    from mx_det import augment
    from scripts import build_corrupted_testsets as b
    from scripts import eval_all, eval_restored, restore_testsets
    four = ["Test_Clean", "Test_Noise", "Test_Blur", "Test_LowRes"]
    monkeypatch.delenv("MX_EXTRA_VARIANTS", raising=False)
    assert augment.env_extra_variants() == []
    assert b.variants() == four == eval_all.all_variants() and eval_restored.VARIANTS == four
    assert restore_testsets.variants_to_restore() == four[1:]
    monkeypatch.setenv("MX_EXTRA_VARIANTS", "jpeg")
    assert augment.env_extra_variants() == [("Test_JPEG", "JPEG")]
    assert b.variants() == four + ["Test_JPEG"] == eval_all.all_variants()
    assert restore_testsets.variants_to_restore() == four[1:] + ["Test_JPEG"]
    assert eval_all.short("Test_JPEG") == "JPEG" and eval_all.short("Test_Blur") == "Blur"
    for bad in ("jpeg,fog", "noise", "JPEG"):
        monkeypatch.setenv("MX_EXTRA_VARIANTS", bad)
        with pytest.raises(ValueError):
            b.variants()
        with pytest.raises(ValueError):
            eval_all.all_variants()


def test_default_kinds_consume_the_same_draws(monkeypatch):
    """The decision rule of RandomCorruptionGPU / _apply_random_corruption before `kinds`, restated, with
    the device call replaced by a recorder: same codes, same seeds, same state of `random`."""
    import torch
    from mx_det import augment, ops
    x = torch.zeros((2, 2, 3), dtype=torch.uint8)
    calls = []
    monkeypatch.setattr(ops, "corrupt_u8", lambda img, codes, **kw: calls.append((list(codes), kw.get("seed"))) or img)

    def before(p=0.5):
        if random.random() > p:
            return None
        code = {"noise": 1, "blur": 2, "lowres": 3}[random.choice(["noise", "blur", "lowres"])]
        return [code], random.getrandbits(63)

    random.seed(4)
    want = [c for c in (before() for _ in range(40)) if c is not None]
    want_state = random.getstate()
    aug = augment.RandomCorruptionGPU(p=0.5)
    random.seed(4)
    for _ in range(40):
        aug(x)
    assert random.getstate() == want_state
    assert calls == want and len({c[0][0] for c in calls}) == 3
    # other kinds: the keep draw, a uniform choice of the given kinds, the seed
    del calls[:]
    aug = augment.RandomCorruptionGPU(p=1.0, kinds=("jpeg", "blur"))
    random.seed(6)
    for _ in range(10):
        aug(x)
    random.seed(6)
    want = []
    for _ in range(10):
        random.random()
        want.append(([{"jpeg": ops.CORRUPT_JPEG, "blur": ops.CORRUPT_BLUR}[random.choice(["jpeg", "blur"])]],
                     random.getrandbits(63)))
    assert calls == want and ops.CORRUPT_JPEG == 4
    # the host chooser: the reference's call for the default kinds
    seen = []
    monkeypatch.setattr(augment, "apply_noise", lambda img, s: seen.append("noise"))
    monkeypatch.setattr(augment, "apply_motion_blur", lambda img, k, a: seen.append("blur"))
    monkeypatch.setattr(augment, "apply_lowres", lambda img, f: seen.append("lowres"))
    monkeypatch.setattr(augment, "apply_jpeg", lambda img, q: seen.append(("jpeg", q)))
    random.seed(8)
    want = [random.choice(["noise", "blur", "lowres"]) for _ in range(12)]
    want_state = random.getstate()
    random.seed(8)
    for _ in range(12):
        augment._apply_random_corruption(None)
    assert seen == want and random.getstate() == want_state
    del seen[:]
    augment._apply_random_corruption(None, kinds=("jpeg",))
    assert seen == [("jpeg", 15)]
