"""engine.evaluate on a stub detector: the fixture of tests/test_gpu_coco_device.py's engine tests, and
the rank body of its two-rank case (torch.distributed.run, gloo, both ranks on cuda:0): each rank
evaluates its shard of the loader with the host evaluator and with the device evaluator and writes
what evaluate() returned to argv[1]/rank{k}.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "robust-object-detection_amd")]

import torch  # noqa: E402


class Stub(torch.nn.Module):
    """Fixed detections per image; the image's first pixel says which."""

    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, imgs):
        return [self.table[int(im[0, 0, 0])] for im in imgs]


def stub_setup(out_dir, dev):
    """(model, loader of three bs=1 batches, annotation file): two classes, a crowd GT, tied scores, an
    image without detections."""
    def ann(aid, img, cat, xywh, crowd=0):
        return {"id": aid, "image_id": img, "category_id": cat, "bbox": [float(v) for v in xywh],
                "area": float(xywh[2] * xywh[3]), "iscrowd": crowd}

    anns = [ann(1, 11, 1, [10, 10, 50, 40]), ann(2, 11, 2, [100, 80, 30, 30]), ann(3, 12, 1, [0, 0, 20, 20]),
            ann(4, 12, 1, [40, 40, 33, 31], crowd=1), ann(5, 13, 2, [5, 5, 100, 100])]
    ann_file = os.path.join(str(out_dir), "ann.json")
    with open(ann_file, "w") as f:
        json.dump({"images": [{"id": i} for i in (11, 12, 13)], "annotations": anns,
                   "categories": [{"id": 1, "name": "car"}, {"id": 2, "name": "bus"}]}, f)

    def out(boxes, scores, labels):
        return {"boxes": torch.tensor(boxes, dtype=torch.float32, device=dev).reshape(-1, 4),
                "scores": torch.tensor(scores, dtype=torch.float32, device=dev),
                "labels": torch.tensor(labels, dtype=torch.int64, device=dev)}

    table = {0: out([[10, 10, 60, 50], [12, 9, 58, 52], [100, 80, 130, 111]], [0.9, 0.9, 0.3], [1, 1, 2]),
             1: out([[1, 0, 20, 21], [45, 45, 60, 60], [200, 200, 230, 260]], [0.8, 0.7, 0.95], [1, 1, 2]),
             2: out([], [], [])}
    loader = []
    for j, img_id in enumerate((11, 12, 13)):
        img = torch.zeros((8, 8, 3), dtype=torch.uint8)
        img[0, 0, 0] = j
        loader.append(([img], [{"image_id": torch.tensor(img_id)}]))
    return Stub(table).to(dev), loader, ann_file


def main():
    import torch.distributed as dist
    from mx_det import engine
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    own = os.path.join(out_dir, f"r{rank}")  # each rank writes its own copy of the annotation file
    os.makedirs(own, exist_ok=True)
    model, loader, ann_file = stub_setup(own, dev)
    shard = loader[rank::world]  # engine.ShardSampler's split
    res = {"rank": rank, "n_images": len(shard),
           "host": engine.evaluate(model, shard, ann_file, dev, per_class=True, device_eval=False),
           "device": engine.evaluate(model, shard, ann_file, dev, per_class=True, device_eval=True)}
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
