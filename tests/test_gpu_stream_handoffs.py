"""The training step's cross-stream hand-offs under a delayed stream (tests/_stream_delay.py).

The step hands data between HIP streams at the FPN output blocks (`fpn`), the RPN head's canvas chain
(`rpn_head`), the RPN target / sampler chain (`rpn_targets`, which also builds the padded GT batch the
RoI sampler reads on the main stream), the side-stream weight gradients (`wgrad`, forked early or
late), the JPEG prefetch loader (`loader`), and when the next step reuses blocks a side stream
allocated. With the machine's own timing a missing wait at any of them almost always loses its race
harmlessly. Here one side of each hand-off is made late by twice the wall time of a whole serial
train step, so a consumer that does not wait runs before its producer, and the step's losses and
gradients -- which the project states are bit-identical with and without the side streams -- change.

No product wait is ever removed to show that the tests bite: test_harness_sees_a_missing_wait (pure
torch ops on a preallocated buffer), the delay size and the asserted spin counts are that evidence.
"""
import copy
import time

import pytest
import torch

from _stream_delay import cycles_per_ms, delayed, delayed_call, spin, stream_beside

pytestmark = pytest.mark.gpu

STREAM_KNOBS = ("MX_FPN_STREAMS", "MX_RPN_STREAMS", "MX_RPN_LOSS_STREAM", "MX_SIDE_WGRAD")
# knobs a run sets explicitly or leaves at the default; none is inherited from the environment
OTHER_KNOBS = ("MX_WGRAD_FORK", "MX_GRAD_CHAIN", "MX_STAGE_GRAPH", "MX_SEG_GRAPHS", "MX_RPN_DEFER_LOSSES")
LOSSES = ["loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"]
# wgrad is requested once per conv (some 70 per backward of this model): every 13th request is
# delayed, so the spins fall across the whole backward of both steps
WGRAD_EVERY, WGRAD_MAX_SPINS = 13, 12


def _run(base, batches, env, delay=None, timed=None, gt_pending=None):
    """Two train steps (forward + backward, no optimizer step, grads cleared between them) of a copy
    of `base` on the two batches: [(losses, grads)] per step. `delay` = (name, where, ms, max_spins,
    every) applies one delayed(); the Delay counter is returned with the steps. `gt_pending` collects,
    per step, whether the GT batch's event was still pending when the host issued the RoI heads.

    After each step the cached padded GT batch is zeroed in place and dropped, so every step builds
    its own. Otherwise the cache keeps the previous batch alive while the next is built, and over
    alternating batches the allocator hands the builder the block that held the same batch two steps
    earlier: a consumer that read it too early would find the right boxes. Zeroed, a recycled block
    holds no boxes at all (count 0), which is well defined and changes every loss."""
    from mx_det import frcnn
    with pytest.MonkeyPatch.context() as mp:
        for k in STREAM_KNOBS + OTHER_KNOBS:
            mp.delenv(k, raising=False)
        mp.setenv("MX_GRAPHS", "0")
        mp.setenv("MX_CONV_TUNE", "0")
        for k, v in env.items():
            mp.setenv(k, v)
        d = delayed(mp, *delay) if delay is not None else None
        m = copy.deepcopy(base)
        if gt_pending is not None:
            events, real_event = [], frcnn._gt_event

            def gt_event(stream):
                events.append(real_event(stream))
                return events[-1]

            mp.setattr(frcnn, "_gt_event", gt_event)
            m.roi_heads.register_forward_pre_hook(lambda *_: gt_pending.append(not events[-1].query()))
        torch.manual_seed(5)
        steps = []
        for imgs, tg in batches:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ld = m(imgs, tg)
            assert list(ld) == LOSSES
            sum(ld.values()).backward()
            torch.cuda.synchronize()
            if timed is not None:
                timed.append((time.perf_counter() - t0) * 1e3)
            steps.append(({k: float(v.detach()) for k, v in ld.items()},
                          {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}))
            for p in m.parameters():
                p.grad = None
            for t in frcnn._gt_batch.cache[2]:
                t.zero_()
            frcnn._gt_batch.cache = None
        torch.cuda.synchronize()
        return steps, d


@pytest.fixture(scope="module")
def setup(dev):
    """The model (built as tests/test_gpu_model.py::_model, the transform shrunk so that the 320x480
    batches are not resized to 800 pixels), two different batches, the serial reference run (every
    stream knob off) and the delay: twice the wall time T of one serial step."""
    from mx_det import frcnn
    from mx_det.data import synth_batch
    torch.manual_seed(0)
    base = frcnn.fasterrcnn_resnet50_fpn_v2(weights=None)
    base.roi_heads.box_predictor = frcnn.FastRCNNPredictor(base.roi_heads.box_predictor.cls_score.in_features, 7)
    frcnn.set_trainable_layers(base.backbone.body, 3)
    base = base.to(dev).train()
    base.transform.min_size, base.transform.max_size = 320, 480
    batches = [synth_batch(0, 2, H=320, W=480, device=dev), synth_batch(2, 2, H=320, W=480, device=dev)]
    serial = {k: "0" for k in STREAM_KNOBS}
    _run(base, batches[:1], serial)  # warm-up: library load, allocator, per-shape constants
    times = []
    ref, _ = _run(base, batches, serial, timed=times)
    T = max(times)
    cycles_per_ms()
    print(f"\nstream hand-offs: serial step T = {times[0]:.1f} / {times[1]:.1f} ms, delay per spin = {2 * T:.1f} ms, "
          f"{cycles_per_ms():.0f} sleep cycles/ms")
    assert set(ref[0][1]) == set(ref[1][1]) and len(ref[0][1]) > 50
    assert ref[0][0] != ref[1][0], "the two steps must differ (a stale read of step 1 would otherwise pass)"
    return {"base": base, "batches": batches, "ref": ref, "ms": 2 * T}


def _assert_same(steps, ref, what):
    for i, ((l, g), (rl, rg)) in enumerate(zip(steps, ref)):
        assert l == rl, (what, "step", i + 1, l, rl)
        assert set(g) == set(rg), (what, "step", i + 1)
        bad = [k for k in rg if not torch.equal(g[k], rg[k])]
        assert not bad, (what, "step", i + 1, len(bad), "of", len(rg), "gradients differ", bad[:8])


def _check_delay(label, d, ms, extra=""):
    """Print what the delay did and assert that it could bite: a stream beside the main one, >= 1 spin
    (a renamed stream or a changed default must not turn the test into a no-op)."""
    print(f"\n{label} on {d.stream_name}: {d.spins} spins of {ms:.1f} ms in {d.calls} requests, "
          f"{d.waits_in_spin} waits in a spin{extra}")
    assert d.stream_name is not None, "no stream beside the main stream"
    assert d.spins >= 1, (label, d.calls)


def test_harness_sees_a_missing_wait(dev):
    """The only intentionally unsynchronised code of the suite, on a preallocated buffer with pure
    torch ops: a dedicated stream spins, then fills the buffer with 1. A clone on the main stream after
    main.wait_stream(side) is all ones; without the wait it is all zeros -- the spin makes a missing
    wait visible instead of letting it lose the race. (The stream is the first of `selfcheck`,
    `selfcheck+1`, ... that does not share the main stream's hardware queue: two streams on one queue
    run in submission order, which no delay can undo.)"""
    ms = 50.0
    main = torch.cuda.current_stream()
    side, name = stream_beside(dev, "selfcheck")
    assert side is not None, "no dedicated stream runs beside the main stream"
    print(f"\nself-check on stream {name}")
    for wait in (True, False):
        buf = torch.zeros(1 << 16, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert spin(ms)
            buf.fill_(1)
        if wait:
            main.wait_stream(side)
        got = buf.clone()
        torch.cuda.synchronize()
        assert bool((got == (1 if wait else 0)).all()), (wait, float(got.sum()))
        assert bool((buf == 1).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("where", ["side", "main"])
@pytest.mark.parametrize("name", ["fpn", "rpn_head", "rpn_targets"])
def test_train_step_bitwise_under_delay(setup, name, where):
    """Default stream knobs, one stream (or the main stream where it requests that stream) late by 2T
    per request: both steps' losses == and every gradient torch.equal to the serial reference. The
    second step runs on another batch -- the GT batch is rebuilt (a stale read would give step 1's
    boxes) and the side streams' blocks of step 1 are reused."""
    pending = [] if name == "rpn_targets" else None
    steps, d = _run(setup["base"], setup["batches"], {}, (name, where, setup["ms"], 8, 1), gt_pending=pending)
    _check_delay(f"{name}/{where}", d, setup["ms"],
                 f"; GT event pending at the RoI heads: {pending}" if pending else "")
    _assert_same(steps, setup["ref"], (name, where))


@pytest.mark.parametrize("where", ["side", "main"])
@pytest.mark.parametrize("fork", ["early", "late"])
def test_side_wgrad_bitwise_under_delay(setup, fork, where):
    """The side-stream weight gradients, forked before (early) or after (late) their dgrad, with the
    wgrad stream or the stream issuing the backward late at requests spread over both backwards."""
    steps, d = _run(setup["base"], setup["batches"], {"MX_WGRAD_FORK": fork},
                    ("wgrad", where, setup["ms"], WGRAD_MAX_SPINS, WGRAD_EVERY))
    _check_delay(f"wgrad/{fork}/{where}", d, setup["ms"])
    assert d.calls > WGRAD_EVERY, ("the spins must reach beyond the first convs of the backward", d.calls)
    _assert_same(steps, setup["ref"], ("wgrad", fork, where))


def test_gt_batch_race_with_graphed_trunk(setup):
    """The historical race in its configuration: the trunk a HIP-graph replay (MX_GRAPHS=1; with
    MX_GRAD_CHAIN=0 bit-identical to eager), the RPN target chain eager beside it on `rpn_targets`,
    which builds the padded GT batch the RoI sampler reads on the main stream. With that stream late the
    sampler must still wait for the batch (the event recorded after it, waited for right before the
    RoI heads). spin() skips itself during the capture."""
    pending = []
    steps, d = _run(setup["base"], setup["batches"], {"MX_GRAPHS": "1", "MX_GRAD_CHAIN": "0"},
                    ("rpn_targets", "side", setup["ms"], 8, 1), gt_pending=pending)
    _check_delay("graphed trunk, rpn_targets/side", d, setup["ms"], f"; GT event pending at the RoI heads: {pending}")
    _assert_same(steps, setup["ref"], "graphed trunk, rpn_targets/side")


def test_prefetch_loader_under_delay(dev, setup, tmp_path, monkeypatch):
    """engine.PrefetchJpegLoader with the loader stream late by 2T in front of every image's device
    stage (tests/test_jpeg.py::test_prefetch_loader_matches_pil's body): the training stream waits for
    the batch's event, so every image still equals PIL's decode and the targets the reference
    dataset's, staged on the consumer running dry and on the training loop's kick."""
    from torch.utils.data import DataLoader
    from mx_det import jpeg
    from mx_det.data import write_coco_split
    from mx_det.dataset import COCODetectionDataset, collate_fn, uint8_transform
    from mx_det.engine import PrefetchJpegLoader
    ann = write_coco_split(tmp_path, "train", 0, 5, H=120, W=176, mean_boxes=6)
    raw = COCODetectionDataset(str(tmp_path / "images/train"), str(ann), transforms=uint8_transform, raw=True)
    ref = COCODetectionDataset(str(tmp_path / "images/train"), str(ann), transforms=uint8_transform)
    ls = delayed(monkeypatch, "loader", "side", setup["ms"], 0)  # only the stream beside the main one
    assert ls.stream_name is not None, "no stream beside the main stream"
    d = delayed_call(monkeypatch, jpeg, "device_stage", setup["ms"])
    for kicked in (False, True):
        loader = PrefetchJpegLoader(DataLoader(raw, batch_size=2, shuffle=False, collate_fn=collate_fn), dev,
                                    workers=3)
        seen = 0
        for images, targets in loader:
            for im, t in zip(images, targets):
                r_img, r_t = ref[seen]
                assert im.device.type == "cuda" and torch.equal(im.cpu(), r_img)
                assert sorted(t) == sorted(r_t)
                for k in r_t:
                    assert t[k].dtype == r_t[k].dtype and torch.equal(t[k].cpu(), r_t[k]), k
                seen += 1
            if kicked:
                loader.kick()
        assert seen == 5
    print(f"\nloader on {ls.stream_name}: {d.spins} spins of {setup['ms']:.1f} ms in {d.calls} device stages, "
          f"{d.waits_in_spin} waits in a spin")
    assert d.spins == 10 and ls.calls == 2, (d.spins, d.calls, ls.calls)
    torch.cuda.synchronize()
