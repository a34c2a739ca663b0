"""A busy stream for the pairs tests (helper, no test in it): calls made on a context whose stream still holds work, with inputs that
arrive late, so that a launch on the wrong stream, a mirror refilled too early or a host argument read after the call's return
shows as a wrong answer (tests/test_gpu_pairs_stream_order.py).

`gate(S, ms)` queues a bounded delay on S, `late` a copy behind it, `held(S)` says whether the backlog is still there.  A `Run`
plays one call sequence in one of two modes: "idle" (the inputs in place, S synchronised before and after every call) or "gated"
(the OTHER valid input set in place, a gate, the real inputs queued behind it, the calls back to back, nothing waited for by the
test).  `run_case` runs a sequence idle on the real set, idle on the other set and gated on the real set, and asserts that the
gated results are the idle ones bit for bit, that the two idle results differ, that the backlog was still there after every call
that promises to wait for nothing, and that every call the case is about found the stream busy.  The gate is four times the host
time of the idle run's calls (each with the synchronisation behind it), at least 20 ms and at most 500 ms.

What lies in a buffer before its late copy, and what is written over a host argument once its call has returned, is always a second
valid input set of the same shape: a mis-ordered read gives a wrong answer, never a wild index or address."""
import ctypes as C
import time

import numpy as np

GATE_MIN_MS, GATE_MAX_MS, GATE_FACTOR = 20.0, 500.0, 4.0
_PROBE_CYCLES = 4000000
_CAL = {}


def own_stream_context(capi):
    """(S, ctx): a torch pool stream (non-blocking: the null stream orders nothing for it) and a context on it."""
    import torch
    S = torch.cuda.Stream()
    return S, capi.Context(0, stream=S.cuda_stream)


def _timed_ms(S, work):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(S):
        a.record(S)
        work()
        b.record(S)
    S.synchronize()
    return a.elapsed_time(b)


def calibrate(S):
    """Once per session: what one millisecond of delay on S costs -- cycles of torch.cuda._sleep, timed by two events around a
    short sleep; where the sleep does not delay the stream (under 0.2 ms for the probe), matmuls of a fixed size instead."""
    import torch
    if _CAL:
        return _CAL
    sleep = lambda: torch.cuda._sleep(_PROBE_CYCLES)
    _timed_ms(S, sleep)  # (the first launch loads the kernel)
    ms = min(_timed_ms(S, sleep) for _ in range(3))
    if ms >= 0.2:
        _CAL.update(kind="sleep", per_ms=_PROBE_CYCLES / ms)
    else:
        with torch.cuda.stream(S):
            m = torch.rand((1024, 1024), device="cuda:0")
        S.synchronize()

        def chain():
            for _ in range(16):
                torch.mm(m, m)
        _timed_ms(S, chain)
        ms = min(_timed_ms(S, chain) for _ in range(3))
        _CAL.update(kind="matmul", per_ms=16.0 / ms, m=m)
    print("stream_backlog: gate by %s, %.4g units per ms" % (_CAL["kind"], _CAL["per_ms"]))
    return _CAL


def gate(S, ms):
    """A delay of about `ms` milliseconds (at most GATE_MAX_MS) queued on S."""
    import torch
    cal = calibrate(S)
    ms = min(float(ms), GATE_MAX_MS)
    with torch.cuda.stream(S):
        if cal["kind"] == "sleep":
            torch.cuda._sleep(int(ms * cal["per_ms"]))
        else:
            for _ in range(max(1, int(ms * cal["per_ms"]))):
                torch.mm(cal["m"], cal["m"])


def late(S, dst, src_pinned):
    """The real content of `dst` (allocated, filled and synchronised before the gate) queued on S behind whatever S holds."""
    import torch
    assert src_pinned.is_pinned() and dst.is_cuda and dst.numel() == src_pinned.numel()
    with torch.cuda.stream(S):
        dst.copy_(src_pinned.view(dst.dtype).view(dst.shape), non_blocking=True)


def held(S):
    """The backlog is still there (to be taken the moment a call returns)."""
    return not S.query()


def gate_length_ms(idle_seconds):
    return min(max(GATE_FACTOR * idle_seconds * 1e3, GATE_MIN_MS), GATE_MAX_MS)


def pinned(a):
    """A pinned host tensor with the array's bytes (uint16 as int16)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).pin_memory()


def device_like(p):
    """A device tensor of a pinned tensor's shape and type, zero-filled and synchronised."""
    import torch
    t = torch.zeros(p.shape, dtype=p.dtype, device="cuda:0")
    torch.cuda.synchronize()
    return t


def overwrite(arg, other):
    """A host argument (numpy array or ctypes object) takes the bytes of the other valid set."""
    if isinstance(arg, np.ndarray):
        assert arg.shape == other.shape and arg.dtype == other.dtype
        np.copyto(arg, other)
    else:
        assert C.sizeof(arg) == C.sizeof(other)
        C.memmove(C.addressof(arg), C.addressof(other), C.sizeof(arg))


def clone(arg):
    if isinstance(arg, np.ndarray):
        return arg.copy()
    out = type(arg)()
    C.memmove(C.addressof(out), C.addressof(arg), C.sizeof(arg))
    return out


class Run:
    """One play of a call sequence.  mode "idle" | "gated"; which "real" | "stale": the input set the run is about (a gated run is
    always about the real set, with the stale one in place first)."""

    def __init__(self, S, mode, which, gate_ms=0.0):
        assert mode in ("idle", "gated") and which in ("real", "stale") and (mode == "idle" or which == "real")
        self.S, self.mode, self.which, self.gate_ms = S, mode, which, gate_ms
        self.log = []  # (label, held before the call, held after it, asserted, about)
        self.call_seconds = 0.0  # idle runs: the host time of the calls, each with the synchronisation behind it

    def place(self, buffers=(), outputs=()):
        """buffers: (device tensor, pinned real, pinned stale) triples; outputs: device tensors to reset.  Idle: the run's set goes
        in, synchronised.  Gated: the stale set goes in, synchronised; then a gate, and the real set queued behind it."""
        import torch
        S = self.S
        S.synchronize()
        first = "stale" if (self.mode == "gated" or self.which == "stale") else "real"
        with torch.cuda.stream(S):
            for o in outputs:
                o.zero_()
            for dst, real, stale in buffers:
                dst.copy_((stale if first == "stale" else real).view(dst.dtype).view(dst.shape), non_blocking=True)
        S.synchronize()
        if self.mode == "gated":
            gate(S, self.gate_ms)
            for dst, real, stale in buffers:
                late(S, dst, real)

    def regate(self, always=False):
        """A fresh gate where the last one has drained, or in any case with `always` (a stream that only holds the last calls' own
        kernels is busy too, for microseconds); gated runs only."""
        if self.mode == "gated" and (always or not held(self.S)):
            gate(self.S, self.gate_ms)

    def host(self, real, stale):
        """(the run's own copy of the host argument of its set, a function that overwrites it with the other set)."""
        mine, other = (real, stale) if self.which == "real" else (stale, real)
        arg = clone(mine)
        return arg, (lambda: overwrite(arg, other))

    def call(self, label, fn, after=None, asserted=False, about=True):
        """One library call; `after` overwrites its host arguments once it has returned.  asserted: the header says that the call
        waits for nothing, so the backlog must still be there when it returns; about: the case is about this call's ordering."""
        if self.mode == "idle":
            self.S.synchronize()
            t0 = time.perf_counter()
            out = fn()
            self.S.synchronize()
            self.call_seconds += time.perf_counter() - t0
        else:
            before = held(self.S)
            out = fn()
            self.log.append((label, before, held(self.S), asserted, about))
        if after is not None:
            after()
        return out

    def finish(self):
        self.S.synchronize()


def as_bytes(v):
    if isinstance(v, bytes):
        return v
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    if hasattr(v, "is_cuda"):
        return np.ascontiguousarray(v.cpu().numpy()).tobytes()
    return bytes(v)


def run_case(name, S, seq):
    """seq(run) plays the case's calls through run.place / run.call / run.finish and returns a dict of results.  Returns the idle
    results on the real set (as bytes) for further comparisons."""
    calibrate(S)
    S.synchronize()
    idle = Run(S, "idle", "real")
    real = {k: as_bytes(v) for k, v in seq(idle).items()}
    idle_s = idle.call_seconds  # (every call synchronised: an upper bound on what the gated run needs to enqueue them)
    stale = {k: as_bytes(v) for k, v in seq(Run(S, "idle", "stale")).items()}
    ms = gate_length_ms(idle_s)
    run = Run(S, "gated", "real", ms)
    t0 = time.perf_counter()
    got = {k: as_bytes(v) for k, v in seq(run).items()}
    gated_s = time.perf_counter() - t0
    same = sorted(k for k in real if real[k] == stale[k])
    wrong = sorted(k for k in real if got[k] != real[k])
    not_held = [l for (l, before, after, asserted, about) in run.log if asserted and not after]
    idle_start = [l for (l, before, after, asserted, about) in run.log if about and not before]
    print("%s: gate %.1f ms, idle host time %.2f ms, gated run %.1f ms; held after call: %s; real and stale idle results differ: %s; gated == idle: %s"
          % (name, ms, idle_s * 1e3, gated_s * 1e3, " ".join("%s=%d" % (l, after) for (l, before, after, asserted, about) in run.log),
             "yes" if not same else "NO (%s)" % ", ".join(same), "yes" if not wrong else "NO (%s)" % ", ".join(wrong)))
    assert not same, (name, "a stale read could not be seen in", same)
    assert not idle_start, (name, "calls the case is about found the stream idle: the gate is too short or an earlier call drained it", idle_start)
    assert not wrong, (name, "the gated run differs from the idle run in", wrong)
    assert not not_held, (name, "calls that wait for nothing drained the stream", not_held)
    return real
