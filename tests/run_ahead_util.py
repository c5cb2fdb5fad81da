"""Letting the host run ahead of the GPU (tests/test_gpu_run_ahead.py is the user).

Every other GPU test synchronises inside its loop, so by the time the host reuses a pinned slot, a ring buffer or a cached
recording the device has long finished with it.  Here a busy-wait kernel holds ONE non-default stream (``side``) while the host
enqueues a whole scenario behind it; the scenario's outputs are then compared, bit for bit, with those of the same scenario run
with a synchronisation after every step.

  * ``stalled(side[, milliseconds])``  the busy-wait as a context manager; ``pending()`` says whether it still holds the stream
  * ``stall_for(host_ms)``           how long to stall for a loop whose synchronous run took ``host_ms`` on the host
  * ``run_ahead(...)``               the method: synchronous run, stalled run, bitwise comparison, run-ahead depth

Stall sizing: ``STALL_FACTOR`` = 4 times the host wall time of the synchronous loop, at least ``STALL_FLOOR_MS`` = 300 ms, at
most ``STALL_CAP_MS`` = 2 s.  The synchronous loop's wall time is an upper bound of the host work of the same loop without its
waits; the stalled loop additionally instantiates recordings the synchronous one only noted, and it shares the host with other
processes, so four times that bound leaves the host room to get through the whole loop while the stall holds.  The floor
covers loops of a few milliseconds, where one scheduling hiccup would outlast any multiple.  The factor only trades spurious
failures against run time: every check reads ``pending()`` (an event query), never the clock.

No other stream tricks, no host callbacks, no environment variables.
"""
import contextlib
import time

import torch

STALL_FACTOR = 4.0
STALL_FLOOR_MS = 300.0
STALL_CAP_MS = 2000.0

_cycles_per_ms = None
_matmul_ms = None
_matmul_operand = None


def _elapsed_ms(enqueue) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    enqueue()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def _matmul_chain(count: int) -> None:
    a = _matmul_operand
    for _ in range(count):
        a = torch.mm(a, _matmul_operand) * (1.0 / 4096.0)


def calibrate() -> None:
    """Times the busy-wait once (after a warm-up) with events on the current stream; later calls are free."""
    global _cycles_per_ms, _matmul_ms, _matmul_operand
    if _cycles_per_ms is not None or _matmul_ms is not None:
        return
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        cycles = 10_000_000
        while True:
            ms = _elapsed_ms(lambda: torch.cuda._sleep(cycles))
            if ms >= 20.0 or cycles >= 10 ** 12:
                break
            cycles *= 10
        _cycles_per_ms = cycles / ms
    else:  # no sleep kernel in this torch build: a chain of large matrix products instead
        _matmul_operand = torch.ones(4096, 4096, device="cuda")
        _matmul_chain(2)
        torch.cuda.synchronize()
        _matmul_ms = _elapsed_ms(lambda: _matmul_chain(8)) / 8.0


def stall_for(host_ms: float) -> float:
    """Milliseconds to stall for a loop whose synchronous run took ``host_ms`` of host wall time (see the module docstring)."""
    return min(STALL_CAP_MS, max(STALL_FLOOR_MS, STALL_FACTOR * host_ms))


class Stall:
    def __init__(self, released):
        self._released = released

    def pending(self) -> bool:
        """The busy-wait has not finished: nothing enqueued on the stream behind it has run."""
        return not self._released.query()


@contextlib.contextmanager
def stalled(side, milliseconds: float = STALL_FLOOR_MS):
    """Enqueues a busy-wait of about ``milliseconds`` (default: the floor, for a single call) on ``side`` and an event behind
    it; yields a ``Stall``.  Leaving the context waits for the whole device, also when the body raised, so nothing stalled
    leaks into the next test.  Nothing in here waits for the stalled stream before that."""
    with torch.cuda.stream(side):
        calibrate()
    torch.cuda.synchronize()
    released = torch.cuda.Event()
    with torch.cuda.stream(side):
        if _cycles_per_ms is not None:
            torch.cuda._sleep(int(milliseconds * _cycles_per_ms))
        else:
            _matmul_chain(max(1, int(milliseconds / _matmul_ms)))
        released.record(side)
    try:
        yield Stall(released)
    finally:
        torch.cuda.synchronize()


def depth_of(pending) -> int:
    """The run-ahead depth: how many leading steps returned while the stall was still pending."""
    depth = 0
    for p in pending:
        if not p:
            break
        depth += 1
    return depth


class Outcome:
    """``expected`` / ``got``: per step the list of device outputs (clones) of the synchronous / the stalled run; ``host_expected``
    / ``host_got``: per step whatever else the step returned; ``pending``: per step whether the stall still held when the step
    had returned; ``stall_ms``."""

    def __init__(self, expected, got, host_expected, host_got, pending, stall_ms):
        self.expected, self.got, self.host_expected, self.host_got = expected, got, host_expected, host_got
        self.pending, self.stall_ms = pending, stall_ms
        self.depth = depth_of(pending)

    def mismatches(self):
        """Steps of which some output differs in a bit (NaN payloads included: the comparison is on the words)."""
        bad = []
        for k, (want, have) in enumerate(zip(self.expected, self.got)):
            if len(want) != len(have) or any(w.shape != h.shape or w.dtype != h.dtype or not torch.equal(_words(w), _words(h))
                                             for w, h in zip(want, have)):
                bad.append(k)
        return bad


def _words(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def run_ahead(side, label, steps, stalled_steps=None):
    """The method.  ``steps``: callables ``step() -> (device tensors, host value)`` that enqueue on the current stream and do
    not synchronise; the tensors need only be valid in stream order (they are copied behind the step, on the stream).

    1. every step with ``torch.cuda.synchronize()`` behind it: the expectation, and the host wall time of the loop;
    2. the steps of ``stalled_steps`` (default: the same ones, i.e. the same warmed-up handle) under
       ``stalled(side)`` with nothing that synchronises in the loop, ``pending()`` noted after each;
    3. the context is left (which synchronises).  Returns the ``Outcome``; prints one line with the depth."""
    with torch.cuda.stream(side):
        expected, host_expected = [], []
        started = time.perf_counter()
        for step in steps:
            tensors, host = step()
            torch.cuda.synchronize()
            expected.append([t.detach().clone() for t in tensors])
            host_expected.append(host)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - started) * 1e3
        store = [[torch.empty_like(t) for t in row] for row in expected]  # allocated before the stall, filled behind each step
        stall_ms = stall_for(host_ms)
        pending, host_got = [], []
        with stalled(side, stall_ms) as stall:
            for step, row in zip(stalled_steps if stalled_steps is not None else steps, store):
                tensors, host = step()
                assert len(tensors) == len(row)
                for dst, t in zip(row, tensors):
                    dst.copy_(t)
                host_got.append(host)
                pending.append(stall.pending())
    outcome = Outcome(expected, store, host_expected, host_got, pending, stall_ms)
    print(f"run-ahead {label}: depth {outcome.depth} of {len(pending)} steps (stall {stall_ms:.0f} ms, synchronous loop "
          f"{host_ms:.1f} ms)")
    return outcome
