"""Flip test-time augmentation of the detector's eval forward (opt-in; the reference evaluates one view).

The image and its horizontal mirror both go through the model; the two detection sets are fused on the
device (mx_det.ops.detections_postprocess_views, csrc/mx_detect.hip):

  fold    the mirrored view's candidates come back into the image's frame, x1' = w - x2, x2' = w - x1
          in continuous coordinates (w = the resized width), and both views share the image's group
  NMS     one class-wise NMS per image over the candidates of both views (torchvision's dispatch rule)
  vote    each of the first detections_per_img survivors takes the score-weighted mean of the
          candidates of its image and class whose IoU with it is >= vote_iou (box voting, Gidaris &
          Komodakis 2015; Detectron's bbox_vote); its score and label stay its own

Set `model.tta = TTA()` (FasterRCNN.tta, None by default). Training mode ignores it; it cannot be
combined with an enabled mx_det.adapt.BNAdapter. The fused detection tail is used whatever
RoIHeads.fused_detections says. Scores are not rescaled by view consensus."""
import math

VIEWS = ("identity", "hflip")


def parse_env(value):
    """MX_TTA=flip[:<vote_iou>] -> TTA, or None when unset / empty. `flip` without a threshold takes 0.8."""
    if not value:
        return None
    kind, _, iou = value.partition(":")
    if kind.strip().lower() != "flip":
        raise ValueError(f"MX_TTA: the only augmentation is 'flip', got {value!r}")
    try:
        v = float(iou) if iou.strip() else 0.8
    except ValueError:
        raise ValueError(f"MX_TTA: vote_iou must be a number, got {value!r}") from None
    try:
        return TTA(vote_iou=v)
    except ValueError:
        raise ValueError(f"MX_TTA: vote_iou must be in (0, 1], got {value!r}") from None


class TTA:
    """The views of a test-time-augmented eval forward and the voting threshold.

    views: "identity" and / or "hflip", each at most once, "identity" first (the kernels take any
    number of views with a flip flag each; these two are the ones the model builds). vote_iou in (0, 1]:
    a candidate votes for a survivor when their IoU is at least this."""

    def __init__(self, views=VIEWS, vote_iou=0.8):
        views = (views,) if isinstance(views, str) else tuple(views)
        bad = [v for v in views if v not in VIEWS]
        if bad or not views or len(set(views)) != len(views) or views[0] != "identity":
            raise ValueError(f"views must be 'identity' alone or {VIEWS}, got {views!r}")
        vote_iou = float(vote_iou)
        if not (0.0 < vote_iou <= 1.0) or math.isnan(vote_iou):
            raise ValueError(f"vote_iou must be in (0, 1], got {vote_iou!r}")
        self.views, self.vote_iou = views, vote_iou

    @property
    def flips(self):
        """One flag per view: the view is mirrored horizontally."""
        return tuple(v == "hflip" for v in self.views)

    def __repr__(self):
        return f"TTA(views={self.views!r}, vote_iou={self.vote_iou!r})"
