"""Test-time BatchNorm adaptation of the detector's eval forward (opt-in; the reference evaluates with
the training statistics only).

Prediction-time BN (Nado et al. 2020) re-estimates every BatchNorm layer's statistics on the test data;
Schneider et al. 2020 (eq. 1) blend them with the training ("source") statistics under a prior of P
images. Per layer and channel, in f64 on the device (mx_bn_finalize_adapt, csrc/mx_bn.hip):

  batch     m_b = sum z / count,  v_b = max(sum z^2 / count - m_b^2, 0)   (biased, as train-mode BN)
  target    mode "batch":  (m_t, v_t) = (m_b, v_b), n = images of this forward; nothing persists
            mode "stream": a state (rows, mean, M2) per layer, zero after reset(), merged with every
            forward by Chan's formula; (m_t, v_t) = (mean', M2'/rows'), n = images since the reset,
            this forward included (a host integer: nothing is read back)
  blend     a = P/(P+n),  mu = a*running_mean + (1-a)*m_t,  var = a*running_var + (1-a)*v_t
  apply     invstd = 1/sqrt(var + eps), scale = gamma*invstd, shift = beta - mu*scale

The adapted layers run conv (with statistics partials) -> finalize -> apply instead of the folded eval
conv. freeze() (stream mode) stops the merging and keeps (mu, var): from then on the layers run the
folded conv with them, at the cost of plain eval. The module's registered buffers and its `training`
flag are never touched (model.state_dict() is the same bytes before and after); the modules in scope
carry a mark in their __dict__, as conv.count_batches marks them.

Scope: the backbone and the FPN. The box head's four BatchNorms keep their source statistics: in the
fused eval tail the head runs on N x post padded RoI rows, so a batch statistic would count dead rows,
and its row population depends on the proposals.

With world > 1 every rank adapts on its own shard of the test set, with no collective: stream-mode
results then depend on the sharding."""
import torch

from . import conv as mc

MODES = ("batch", "stream")
_SCOPES = {"backbone": "backbone.body", "fpn": "backbone.fpn"}


class _Layer:
    """One BatchNorm2d's adaptation record (the module's __dict__["_mx_adapt"])."""

    def __init__(self, owner):
        self.owner = owner
        self.state = None  # stream mode: [3][K] f64 rows, mean, M2
        self.mean = self.var = None  # the blended statistics of the latest forward ([K] f32)
        self.images = 0
        self.frozen = False

    def __deepcopy__(self, memo):
        return None  # a copy of an adapted model starts without adaptation (conv.bn_adapting reads None as off)

    def prepare(self, K, device):
        if self.mean is None:
            self.mean = torch.zeros(K, dtype=torch.float32, device=device)
            self.var = torch.ones(K, dtype=torch.float32, device=device)
            if self.owner.mode == "stream":
                self.state = torch.zeros((3, K), dtype=torch.float64, device=device)

    def count(self, images):
        """n of the blend for a forward of `images` images."""
        if self.owner.mode == "batch":
            self.images = images
        else:
            self.images += images
        return self.images

    def reset(self):
        self.images, self.frozen = 0, False
        if self.state is not None:
            self.state.zero_()


def parse_env(value):
    """MX_BN_ADAPT=<mode>[:<prior>] -> (mode, prior), or None when unset / empty. A mode without a prior
    takes 16."""
    if not value:
        return None
    mode, _, prior = value.partition(":")
    mode = mode.strip().lower()
    if mode not in MODES:
        raise ValueError(f"MX_BN_ADAPT: mode must be one of {MODES}, got {value!r}")
    try:
        p = float(prior) if prior.strip() else 16.0
    except ValueError:
        raise ValueError(f"MX_BN_ADAPT: prior must be a number, got {value!r}") from None
    return mode, p


class BNAdapter:
    """Test-time BatchNorm adaptation of `model`'s eval forward (see the module docstring).

    mode "stream" (default) accumulates the statistics over the forwards since reset() -- for callers who
    stream a test set at batch size 1; "batch" uses each forward's own statistics. prior: P >= 0, in
    images (P = 0 with mode "batch" normalises as train-mode BN does). scope: "backbone" and / or "fpn";
    None adapts every mx_det BatchNorm2d under `model` (a bare block). "box_head" is refused.

    enable() / disable() switch the adaptive branch of conv.conv_bn (also `with adapter:`); reset()
    clears the statistics and the image count and unfreezes; freeze() (stream mode) keeps the current
    blended statistics and runs the folded eval conv with them. Each rank of a multi-GPU evaluation
    adapts on its own shard with no collective, so stream-mode results depend on the sharding."""

    def __init__(self, model, mode="stream", prior=16, scope=("backbone", "fpn")):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        prior = float(prior)
        if not 0.0 <= prior < float("inf"):
            raise ValueError(f"prior must be a finite number >= 0, got {prior!r}")
        self.model, self.mode, self.prior, self.enabled = model, mode, prior, False
        roots = [model]
        if scope is not None:
            scope = (scope,) if isinstance(scope, str) else tuple(scope)
            if "box_head" in scope:
                raise ValueError("scope 'box_head': the box head's BatchNorms keep their source statistics -- in the "
                                 "fused eval tail the head runs on N x post padded RoI rows, so a batch statistic "
                                 "would count dead rows, and its row population depends on the proposals")
            bad = [s for s in scope if s not in _SCOPES]
            if bad:
                raise ValueError(f"scope entries must be among {tuple(_SCOPES)}, got {bad}")
            roots = [model.get_submodule(_SCOPES[s]) for s in scope]
        self.layers = []  # (module, record), in module order
        for r in roots:
            for m in r.modules():
                if isinstance(m, mc.BatchNorm2d) and all(m is not q for q, _ in self.layers):
                    self.layers.append((m, _Layer(self)))
        if not self.layers:
            raise ValueError("no BatchNorm2d in scope")

    # ---- switches ----------------------------------------------------------------------------
    def enable(self):
        from .frcnn import _be
        be = _be(self.model)
        if not getattr(be, "bn_adapt", False):
            raise NotImplementedError(f"backend {getattr(be, 'name', type(be).__name__)!r} has no test-time BatchNorm "
                                      "adaptation (mx_bn_finalize_adapt is a HIP kernel)")
        for m, rec in self.layers:
            other = m.__dict__.get("_mx_adapt")
            if other is not None and other.owner is not self and other.owner.enabled:
                raise RuntimeError("another enabled BNAdapter already adapts this model")
            m.__dict__["_mx_adapt"] = rec
        self.enabled = True
        return self

    def disable(self):
        self.enabled = False
        for m, rec in self.layers:
            if m.__dict__.get("_mx_adapt") is rec:
                del m.__dict__["_mx_adapt"]
        return self

    def __enter__(self):
        return self.enable()

    def __exit__(self, *exc):
        self.disable()

    def reset(self):
        for _, rec in self.layers:
            rec.reset()
        return self

    def freeze(self):
        if self.mode != "stream":
            raise RuntimeError("freeze() needs mode 'stream' (batch mode keeps no statistics)")
        if self.images_seen == 0:
            raise RuntimeError("freeze() before any adapted forward: there are no statistics to keep")
        for _, rec in self.layers:
            rec.frozen = rec.mean is not None  # a layer no forward reached keeps adapting
        return self

    @property
    def frozen(self):
        return any(rec.frozen for _, rec in self.layers)

    @property
    def images_seen(self):
        """Images merged since the last reset (stream mode), or of the latest forward (batch mode)."""
        return max(rec.images for _, rec in self.layers)

    def states(self):
        """The layers' state tensors [3][K] f64 (rows, mean, M2), None where no forward has run."""
        return [rec.state for _, rec in self.layers]
