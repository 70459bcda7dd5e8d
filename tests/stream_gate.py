"""Makes work on several HIP streams start at the same instant, and proves that it overlapped (helpers, no tests).

A *gate* is a spin kernel (``torch.cuda._sleep``) on a stream of its own followed by an event that every work stream waits on.  The
host enqueues all the work while the gate is shut, so nothing of it depends on how fast the host enqueues: when the spin ends,
every stream is runnable at once.  ``Gate.close_check()`` asserts that the gate was still shut after the last enqueue -- a gate
that opened earlier says nothing, and the run fails rather than pass quietly.

Each stream's work is bracketed by two timing events (``Gate.section``).  Two sections overlapped when each started before the
other ended (``overlapped``); ``require_overlap`` fails a test in which fewer than half of the repetitions did.
MEASURED on the MI355X with the default 4 hardware queues: 16 of 16 repetitions overlapped in every test of
tests/test_gpu_streams.py, alone and at the file's place in the whole suite."""
import contextlib
import functools

import torch

GATE_MS = 50.0
_GATE_STREAMS = {}


@functools.lru_cache(maxsize=None)
def calibrate(dev):
    """Cycle count that keeps ``torch.cuda._sleep`` busy for about GATE_MS milliseconds on ``dev`` (timed once, with events)."""
    probe = 20_000_000
    with torch.cuda.device(dev):
        torch.cuda._sleep(1000)                       # the kernel's first launch loads its code object
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.cuda._sleep(probe)
        t1.record()
        t1.synchronize()
    ms = t0.elapsed_time(t1)
    assert ms > 0.5, f"torch.cuda._sleep({probe}) took {ms} ms: too short to calibrate with"
    return int(probe * GATE_MS / ms)


def warm(streams):
    """One trivial launch and one timing event on each stream, waited for: a stream's first launch sets up its hardware queue,
    which can take longer than the gate stays shut.  Returns the streams."""
    for s in streams:
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
            torch.cuda.Event(enable_timing=True).record()
        s.synchronize()
    return streams


class Section:
    """The timing events around one stream's work; ``times()`` in milliseconds after the gate opened."""

    def __init__(self, gate, stream):
        self.gate, self.stream = gate, stream
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def times(self):
        return self.gate.opened.elapsed_time(self.t0), self.gate.opened.elapsed_time(self.t1)


class Gate:
    """Shuts ``streams`` (at most three) behind a spin of about GATE_MS on the gate stream.  Call after a device synchronise: the
    gate orders nothing against earlier work."""

    def __init__(self, streams, dev):
        assert 1 <= len(streams) <= 3
        self.dev = torch.device(dev)
        cycles = calibrate(self.dev)
        if self.dev not in _GATE_STREAMS:
            _GATE_STREAMS[self.dev] = warm([torch.cuda.Stream(self.dev)])[0]
        self.stream = _GATE_STREAMS[self.dev]
        self.opened = torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(cycles)
            self.opened.record()
        for s in streams:
            s.wait_event(self.opened)

    @contextlib.contextmanager
    def section(self, stream):
        """Brackets what the body enqueues on ``stream`` (through its pointer, ``stream.cuda_stream``) with timing events."""
        sec = Section(self, stream)
        sec.t0.record(stream)
        yield sec
        sec.t1.record(stream)

    def close_check(self):
        assert not self.opened.query(), "the gate opened before the host had enqueued everything: this run shows nothing"


def overlapped(a, b):
    """a, b: (start, end) of two sections on one clock."""
    return a[0] < b[1] and b[0] < a[1]


def all_overlapped(spans):
    return all(overlapped(spans[i], spans[j]) for i in range(len(spans)) for j in range(i + 1, len(spans)))


def require_overlap(flags, what):
    """flags: one bool per repetition.  Fails when fewer than half overlapped; returns the share."""
    share = sum(bool(f) for f in flags) / len(flags)
    assert share >= 0.5, f"{what}: only {sum(flags)} of {len(flags)} repetitions overlapped on the device: no evidence of concurrency"
    return share
