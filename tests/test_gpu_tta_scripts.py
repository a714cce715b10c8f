"""scripts.eval_all under MX_TTA on a tiny synthetic test set: the <name>_TTA entries beside the unchanged
single-view ones, in the reference schema, and a bad value refused before any checkpoint is read."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = {"Test_Clean": (96, 128), "Test_Noise": (80, 144)}


@pytest.fixture(scope="module")
def files(dev, tmp_path_factory):
    """The synthetic test sets and one checkpoint with seeded random weights."""
    from mx_det import frcnn
    from mx_det.data import write_coco_split
    root = tmp_path_factory.mktemp("tta_scripts")
    for i, (v, (h, w)) in enumerate(SIZES.items()):
        write_coco_split(root / "testsets" / v, "val", 300 + 10 * i, 3, h, w, mean_boxes=4)
    torch.manual_seed(11)
    m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    m.roi_heads.box_predictor = frcnn.FastRCNNPredictor(m.roi_heads.box_predictor.cls_score.in_features, 7)
    with torch.no_grad():  # a detection tail that keeps some boxes on random weights
        m.roi_heads.box_predictor.cls_score.weight.mul_(20.0)
    torch.save({"model": m.state_dict()}, root / "best.pth")
    return root / "testsets", root / "best.pth"


@pytest.fixture
def script(files, tmp_path, monkeypatch):
    from mx_det import engine
    from scripts import eval_all
    for k in ("MX_TTA", "MX_BN_ADAPT", "MX_BN_ADAPT_FREEZE_AFTER", "MX_EXTRA_VARIANTS", "MX_SEVERITIES"):
        monkeypatch.delenv(k, raising=False)
    ts, ck = files
    load = engine.load_frcnn_checkpoint
    loaded = []

    def load_small(path, d):
        mm = load(path, d)
        mm.transform.min_size, mm.transform.max_size = 128, 192
        loaded.append(mm)
        return mm

    monkeypatch.setattr(eval_all, "load_frcnn_checkpoint", load_small)
    monkeypatch.setattr(eval_all, "VARIANTS", list(SIZES))
    monkeypatch.setattr(eval_all, "COCO_TESTSET_ROOT", ts)
    monkeypatch.setattr(eval_all, "CKPTS", {"FasterRCNN": ck})
    monkeypatch.setattr(eval_all, "OUT_DIR", tmp_path / "out")
    return eval_all, loaded, tmp_path / "out"


def test_eval_all_adds_the_tta_entries(script, monkeypatch):
    eval_all, loaded, out = script
    monkeypatch.setenv("MX_TTA", "flip:0.8")
    res = eval_all.main()
    assert list(res) == ["FasterRCNN", "FasterRCNN_TTA"]
    # only the script reads the environment: the plain pass ran one view, the second pass two
    assert len(loaded) == 2 and loaded[0].tta is None
    assert loaded[1].tta.views == ("identity", "hflip") and loaded[1].tta.vote_iou == 0.8
    on = json.load(open(out / "eval_results.json"))
    assert list(on) == ["FasterRCNN", "FasterRCNN_TTA"]
    for name in on:
        assert list(on[name]) == list(SIZES)
        for r in on[name].values():
            assert set(r) == {"mAP50_95", "mAP50", "per_class_ap50"}
            assert 0.0 <= r["mAP50_95"] <= r["mAP50"] <= 1.0
    rows = (out / "eval_results.csv").read_text().splitlines()
    assert [r.split(",")[0] for r in rows[1:5]] == ["FasterRCNN", "FasterRCNN", "FasterRCNN_TTA", "FasterRCNN_TTA"]
    # the single-view entry is what a run without MX_TTA writes
    monkeypatch.delenv("MX_TTA")
    monkeypatch.setattr(eval_all, "OUT_DIR", out.parent / "off")
    off = eval_all.main()
    assert list(off) == ["FasterRCNN"] and off["FasterRCNN"] == res["FasterRCNN"] and loaded[2].tta is None


@pytest.mark.parametrize("value", ["mirror", "flip:2", "flip:x"])
def test_eval_all_refuses_a_bad_value_before_any_checkpoint(script, monkeypatch, tmp_path, value):
    eval_all, loaded, out = script
    monkeypatch.setattr(eval_all, "CKPTS", {"FasterRCNN": tmp_path / "missing.pth"})
    monkeypatch.setenv("MX_TTA", value)
    with pytest.raises(ValueError, match="MX_TTA"):
        eval_all.main()
    assert not loaded and not out.exists()
