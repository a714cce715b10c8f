"""scripts.demo_inference on a tiny synthetic Clean / Blur test-set pair and two random-weight checkpoints: one
JPEG per selected image, named after the ground-truth and drawn counts, its bytes those of the device
encoder on the canvas tests/draw_ref.py builds from the same detections; MX_DEMO_EXTRA adds panels, and a bad
value is refused before a checkpoint is opened."""
import json
import re

import numpy as np
import pytest
import torch

import draw_ref as R

pytestmark = pytest.mark.gpu

H, W, IDS = 96, 128, (700, 701, 702)


@pytest.fixture(scope="module")
def files(dev, tmp_path_factory):
    """Test_Clean / Test_Blur written with the device JPEG encoder, and two checkpoints with seeded weights."""
    from mx_det import frcnn, jpeg
    from mx_det.data import synth_image, synth_target
    root = tmp_path_factory.mktemp("demo_scripts")
    images, anns = [], []
    for i in IDS:
        img = torch.from_numpy(synth_image(i, H, W)).to(dev)
        blur = torch.nn.functional.avg_pool2d(img.permute(2, 0, 1)[None].float(), (1, 9), 1, (0, 4)).round()
        for v, x in (("Test_Clean", img), ("Test_Blur", blur[0].permute(1, 2, 0).to(torch.uint8).contiguous())):
            d = root / "testsets" / v / "images" / "val"
            d.mkdir(parents=True, exist_ok=True)
            jpeg.write_file(d / f"{i}.jpg", x, quality=95)
        images.append({"id": i, "file_name": f"{i}.jpg", "width": W, "height": H})
        t = synth_target(i, H, W, mean_boxes=3 + (i - IDS[0]))
        for b, lab in zip(t["boxes"].tolist(), t["labels"].tolist()):
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": lab, "iscrowd": 0,
                         "bbox": [b[0], b[1], b[2] - b[0], b[3] - b[1]], "area": (b[2] - b[0]) * (b[3] - b[1])})
    # an empty annotation: counted by the selection, not drawn
    anns.append({"id": len(anns) + 1, "image_id": IDS[0], "category_id": 2, "iscrowd": 0, "bbox": [5, 5, 0, 7], "area": 0})
    for v in ("Test_Clean", "Test_Blur"):
        a = root / "testsets" / v / "annotations"
        a.mkdir(parents=True, exist_ok=True)
        (a / "instances_val.json").write_text(json.dumps({"images": images, "annotations": anns, "categories": []}))
    cks = {}
    for name, seed in (("FasterRCNN", 11), ("FasterRCNN_aug", 12)):
        torch.manual_seed(seed)
        m = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
        m.roi_heads.box_predictor = frcnn.FastRCNNPredictor(m.roi_heads.box_predictor.cls_score.in_features, 7)
        with torch.no_grad():  # a detection tail that keeps some boxes on random weights
            m.roi_heads.box_predictor.cls_score.weight.mul_(20.0)
        torch.save({"model": m.state_dict()}, root / f"{name}.pth")
        cks[name] = root / f"{name}.pth"
    return root / "testsets", cks, anns


@pytest.fixture
def script(files, tmp_path, monkeypatch):
    from mx_det import engine
    from scripts import demo_inference as demo
    for k in ("MX_DEMO_EXTRA", "MX_TTA", "MX_BN_ADAPT"):
        monkeypatch.delenv(k, raising=False)
    ts, cks, _ = files
    load = engine.load_frcnn_checkpoint
    loaded, calls = [], []

    def load_small(path, d):
        mm = load(path, d)
        mm.transform.min_size, mm.transform.max_size = 128, 192
        padded = mm.detect_padded

        def recording(images):
            out = padded(images)
            calls.append(tuple(t.cpu().numpy() for t in out))
            return out

        mm.detect_padded = recording
        loaded.append(mm)
        return mm

    monkeypatch.setattr(demo, "load_frcnn_checkpoint", load_small)
    monkeypatch.setattr(demo, "COCO_TESTSET_ROOT", ts)
    monkeypatch.setattr(demo, "CKPTS", cks)
    monkeypatch.setattr(demo, "OUT_DIR", tmp_path / "demo")
    return demo, loaded, calls, tmp_path / "demo"


def _expected(demo, files, dev, img_id, dets, titles):
    """The canvas the painter and the composer of draw_ref build from the recorded detections."""
    from mx_det import jpeg
    ts, _, anns = files
    names = [demo.CLASS_NAMES[k] for k in range(1, 7)]
    colors = [demo.CLASS_COLORS[k] for k in range(1, 7)]
    bgr = lambda v: jpeg.read_file(ts / v / "images" / "val" / f"{img_id}.jpg", dev).cpu().numpy()[..., ::-1]
    clean, blur = bgr("Test_Clean"), bgr("Test_Blur")
    gt = [a for a in anns if a["image_id"] == img_id and a["bbox"][2] > 0 and a["bbox"][3] > 0]
    gtb = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in gt],
                   np.float32).reshape(-1, 4)
    glyphs = R.font()
    panels = [R.paint(clean, gtb, [a["category_id"] for a in gt], None, len(gt), names, colors, title=titles[0], bar=40,
                      glyphs=glyphs)[0]]
    drawn = []
    for (ob, osc, ol, cnt), title in zip(dets, titles[1:]):
        p, n = R.paint(blur, ob[0], ol[0], osc[0], cnt[0], names, colors, demo.CONF_THRESHOLD, title=title, bar=40,
                       glyphs=glyphs)
        panels.append(p)
        drawn.append(n)
    return R.compose(panels, 480), len(gt), drawn


def _check_files(demo, files, dev, calls, written, titles):
    from mx_det import jpeg
    ids = demo.select_images(str(files[0] / "Test_Clean" / "annotations" / "instances_val.json"), demo.N_SAMPLES)
    assert sorted(ids) == sorted(IDS) and len(written) == len(ids)
    per = len(titles) - 1
    assert len(calls) == per * len(ids)
    dw = int(W * (480 / (40 + H)))
    for k, (img_id, path) in enumerate(zip(ids, written)):
        m = re.fullmatch(rf"FRCNN_img{img_id:04d}_gt(\d+)_base(\d+)_aug(\d+)\.jpg", path.name)
        assert m, path.name
        canvas, n_gt, drawn = _expected(demo, files, dev, img_id, calls[per * k:per * (k + 1)], titles)
        assert [int(g) for g in m.groups()] == [n_gt, drawn[0], drawn[1]]
        got = jpeg.read_file(path, dev, bgr=True)
        assert tuple(got.shape) == (480, len(titles) * dw + 3 * (len(titles) - 1), 3) == canvas.shape
        want = jpeg.encode(torch.from_numpy(canvas).to(dev), quality=92, bgr=True)
        assert path.read_bytes() == want
    return ids


def test_demo_writes_one_comparison_per_image(script, files, dev, capsys):
    demo, loaded, calls, out = script
    written = demo.main()
    assert len(loaded) == 2 and sorted(p.name for p in out.iterdir()) == sorted(p.name for p in written)
    titles = ["Clean (Ground Truth)", "Blur + FRCNN (Baseline)", "Blur + FRCNN (Augmented)"]
    _check_files(demo, files, dev, calls, written, titles)
    assert any(c[3][0] > 0 for c in calls)  # the random heads keep some detections
    assert "skipped" in capsys.readouterr().out


def test_demo_extra_tta_adds_a_panel(script, files, dev, monkeypatch):
    demo, loaded, calls, out = script
    monkeypatch.setenv("MX_DEMO_EXTRA", "tta")
    written = demo.main()
    titles = ["Clean (Ground Truth)", "Blur + FRCNN (Baseline)", "Blur + FRCNN (Augmented)",
              "Blur + FRCNN (Augmented, TTA)"]
    _check_files(demo, files, dev, calls, written, titles)
    assert loaded[1].tta is None  # put back after each augmented forward


def test_detect_padded_hands_out_the_fused_tail_as_it_is(files, dev):
    from mx_det import engine, jpeg
    ts, cks, _ = files
    m = engine.load_frcnn_checkpoint(cks["FasterRCNN_aug"], dev)
    m.transform.min_size, m.transform.max_size = 128, 192
    img = jpeg.read_file(ts / "Test_Blur" / "images" / "val" / f"{IDS[1]}.jpg", dev)
    with torch.no_grad():
        ob, osc, ol, counts = m.detect_padded([img])
        m.check_padded()  # no count of -1: passes, and waits for nothing twice
        m.check_padded()
        plain = m([img])
    D = m.roi_heads.detections_per_img
    assert ob.shape == (1, D, 4) and osc.shape == (1, D) and ol.shape == (1, D) and counts.shape == (1,)
    assert ob.dtype == torch.float32 and ol.dtype == torch.int64 and counts.dtype == torch.int32
    c = int(counts[0])
    assert 0 < c <= D and not ob[0, c:].any() and not osc[0, c:].any() and not ol[0, c:].any()
    assert (osc[0, :c - 1] >= osc[0, 1:c]).all() and (ol[0, :c] >= 1).all()
    # the switch is taken back: the plain forward answers with its list of dicts
    assert isinstance(plain, list) and set(plain[0]) == {"boxes", "labels", "scores"}
    m.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.detect_padded([img])


def test_demo_extra_titles_and_order():
    from scripts import demo_inference as demo
    assert demo.parse_extra("") == [] and demo.parse_extra(" BNAdapt , tta") == ["bnadapt", "tta"]
    assert demo.EXTRAS == {"tta": "TTA", "bnadapt": "BNAdapt"}


@pytest.mark.parametrize("value", ["bogus", "tta,tta", "tta;bnadapt"])
def test_demo_refuses_a_bad_extra_before_any_checkpoint(script, monkeypatch, tmp_path, value):
    demo, loaded, calls, out = script
    monkeypatch.setattr(demo, "CKPTS", {"FasterRCNN": tmp_path / "missing.pth", "FasterRCNN_aug": tmp_path / "missing.pth"})
    monkeypatch.setenv("MX_DEMO_EXTRA", value)
    with pytest.raises(ValueError, match="MX_DEMO_EXTRA"):
        demo.main()
    assert not loaded and not out.exists()
