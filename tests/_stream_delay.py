"""Delayed-stream harness of tests/test_gpu_stream_handoffs.py.

A cross-stream hand-off with a missing wait almost always loses its race harmlessly: the side chains
are short. spin() makes one side of a hand-off late by a chosen time (a busy kernel on that stream),
so that a consumer which does not wait reads its input before the producer wrote it -- and the
result changes. delayed() puts such a spin at the single seam every framework side stream comes
from, mx_det.conv.dedicated_stream (frcnn, conv.wgrad_stream and engine resolve it through the conv
module at call time).
"""
import torch

_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond on the current device: one timed _sleep (after a short
    one that loads the kernel), measured once per process."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        n = 50_000_000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        _cycles_per_ms = n / max(e0.elapsed_time(e1), 1e-3)
    return _cycles_per_ms


def spin(ms):
    """Enqueue a busy kernel of about `ms` milliseconds on the current stream. A no-op (returns False)
    while the current stream is capturing: nothing new goes into a captured graph."""
    if torch.cuda.is_current_stream_capturing():
        return False
    torch.cuda._sleep(int(ms * cycles_per_ms()))
    return True


def runs_beside(stream, ms=5.0):
    """True when work on `stream` runs concurrently with the current stream. Streams are spread over a
    few hardware queues (GPU_MAX_HW_QUEUES), and two streams that share one run in submission order: a
    spin on the one then also holds the other back, and no missing wait between them can show. Timed
    with events only (a spin on `stream`, an event on the current stream behind it): no memory is
    shared, nothing races."""
    main = torch.cuda.current_stream()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(main)
    with torch.cuda.stream(stream):
        spin(ms)
    e1.record(main)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) < ms / 2


def stream_beside(device, name, tries=5):
    """(stream, its name): the framework's dedicated stream `name` when it runs beside the current
    stream, else the first of `name`+1, `name`+2, ... (further dedicated streams, created once) that
    does; consecutive new streams land on different hardware queues. (None, name) if none does."""
    from mx_det import conv as mc
    real = getattr(mc.dedicated_stream, "_real", mc.dedicated_stream)
    for k in range(tries):
        nm = name if k == 0 else f"{name}+{k}"
        s = real(device, nm)
        if runs_beside(s):
            return s, nm
    return None, name


class Delay:
    """What delayed() did: `calls` requests for the stream outside a capture, `spins` of them delayed,
    and `waits_in_spin`: how many times the other side of the hand-off issued a wait (wait_stream /
    wait_event) while the latest spin had not finished -- there the host was ahead of the late stream,
    so only that wait kept the consumer behind its producer. Reported, not asserted: it depends on the
    host never stalling for a whole spin."""

    def __init__(self):
        self.calls = 0
        self.spins = 0
        self.waits_in_spin = 0
        self.stream_name = None  # the stream that stood in for `name` (stream_beside)
        self._late = None   # raw handle of the stream that was made late
        self._event = None  # recorded right behind the latest spin

    def _spun(self):
        s = torch.cuda.current_stream()
        self._late = s.cuda_stream
        self._event = s.record_event()
        self.spins += 1

    def _watch(self, monkeypatch):
        real = torch.cuda.Stream.wait_event  # wait_stream(s) is wait_event(s.record_event())

        def wait_event(stream, event):
            if (self._event is not None and stream.cuda_stream != self._late
                    and not torch.cuda.is_current_stream_capturing() and not self._event.query()):
                self.waits_in_spin += 1
            return real(stream, event)

        monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)


def delayed(monkeypatch, name, where, ms, max_spins, every=1, device=None):
    """Wrap mx_det.conv.dedicated_stream: a request for stream `name` first enqueues spin(ms) on that
    stream (where="side") or on the caller's current stream (where="main"), then returns the stream.
    Every `every`-th request spins (a stream requested once per conv is delayed at calls spread over
    the whole backward, not only its first ones), `max_spins` in all; max_spins=0 only wraps.

    The stream returned for `name` is stream_beside(): the framework's own unless that shares a
    hardware queue with the current (main) stream, where the delay could not separate the two; then a
    further dedicated stream stands in for it for as long as the patch holds (every request for `name`
    gets the same one). Call it on the main stream. Returns the Delay counter; its stream_name is None
    when no stream beside the main one was found."""
    assert where in ("side", "main"), where
    from mx_det import conv as mc
    real = mc.dedicated_stream
    d = Delay()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    sub, chosen = stream_beside(device, name)
    d.stream_name = chosen if sub is not None else None
    key = device.index if device.index is not None else torch.cuda.current_device()

    def wrapped(device, nm):
        if nm != name:
            return real(device, nm)
        dv = torch.device(device)
        same = (dv.index if dv.index is not None else torch.cuda.current_device()) == key
        s = sub if (sub is not None and same) else real(device, nm)
        if torch.cuda.is_current_stream_capturing():
            return s
        d.calls += 1
        if d.spins < max_spins and (d.calls - 1) % every == 0:
            if where == "side":
                with torch.cuda.stream(s):
                    if spin(ms):
                        d._spun()
            elif spin(ms):
                d._spun()
        return s

    wrapped._real = getattr(real, "_real", real)
    monkeypatch.setattr(mc, "dedicated_stream", wrapped)
    d._watch(monkeypatch)
    return d


def delayed_call(monkeypatch, module, attr, ms):
    """Wrap module.attr (a function that enqueues device work on the current stream, such as
    mx_det.jpeg.device_stage inside the loader's stream context): spin(ms) first, then the real call.
    Returns the Delay counter."""
    real = getattr(module, attr)
    d = Delay()

    def wrapped(*a, **k):
        d.calls += 1
        if spin(ms):
            d._spun()
        return real(*a, **k)

    monkeypatch.setattr(module, attr, wrapped)
    d._watch(monkeypatch)
    return d
