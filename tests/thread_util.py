"""Host threads for the threading tests (tests/test_threads_cpu.py, tests/test_gpu_threads.py): every callable on a
``threading.Thread`` of its own, released together by a barrier, joined under a cap.

The cap is a guard against a silent hang, not a measurement.  A thread that is still alive at the cap cannot be stopped from
Python; it may sit inside the library with a device lock held.  So the first such thread sets ``STUCK``, and every GPU test of
the threading module looks at ``STUCK`` before it touches the card: after a hang nothing more is started there from this
process.
"""
from __future__ import annotations

import threading
import time

LIMIT_S = 120.0  # the join cap of every case
MAX_THREADS = 8
STUCK = None     # None, or the message of the first join that ran into the cap


class ThreadStuck(AssertionError):
    pass


def check_not_stuck():
    """First line of every GPU case: fail at once, without a GPU call, if an earlier case left a thread behind."""
    if STUCK is not None:
        raise ThreadStuck(f"not run: {STUCK}")


def run_threads(fns, limit_s=LIMIT_S, names=None):
    """``fns[i]()`` on thread i, all released together; returns ``([result of fns[i]], wall seconds)``.

    An exception in a thread is raised here again as an AssertionError that names the thread (the first one, in thread order).
    A thread still alive ``limit_s`` seconds after the start fails the caller with a message that names it and sets ``STUCK``."""
    global STUCK
    fns = list(fns)
    assert 1 <= len(fns) <= MAX_THREADS, f"{len(fns)} threads: a case has at most {MAX_THREADS}"
    names = list(names) if names is not None else [getattr(f, "__name__", "fn") for f in fns]
    names = [f"thread {i} ({n})" for i, n in enumerate(names)]
    barrier = threading.Barrier(len(fns) + 1)
    results, errors = [None] * len(fns), [None] * len(fns)
    began, ended = [None] * len(fns), [None] * len(fns)

    def body(i):
        try:
            barrier.wait(limit_s)
            began[i] = time.perf_counter()
            results[i] = fns[i]()
        except BaseException as e:  # noqa: BLE001  (handed to the caller below)
            errors[i] = e
        ended[i] = time.perf_counter()

    threads = [threading.Thread(target=body, args=(i,), name=names[i], daemon=True) for i in range(len(fns))]
    for t in threads:
        t.start()
    barrier.wait(limit_s)
    t0 = time.perf_counter()
    for t in threads:
        t.join(max(0.0, limit_s - (time.perf_counter() - t0)))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        msg = f"{', '.join(alive)} still running after {limit_s:.0f} s"
        if STUCK is None:
            STUCK = msg
        raise ThreadStuck(msg)
    for i, e in enumerate(errors):
        if e is not None:
            raise AssertionError(f"{names[i]}: {type(e).__name__}: {e}") from e
    # from the first thread's start to the last one's end (this thread may wake from the barrier well behind them)
    wall = max(ended) - min(t for t in began if t is not None) if any(t is not None for t in began) else 0.0
    return results, wall


def report(case, n_threads, rounds, wall_s, verdict="identical"):
    """The one line a case prints: the margin to the cap is visible in it."""
    print(f"{case}: {n_threads} threads, {rounds} rounds, {wall_s:.3f} s (cap {LIMIT_S:.0f} s), {verdict}")
