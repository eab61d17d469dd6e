"""The host-only entry points of the library from eight threads at once (no GPU): vp_mseed_scan, vp_pick_host and the
thread-local text of vp_last_error.  ctypes releases the GIL around every call into the library, so the calls really overlap.
Every concurrent result is compared with the same call made alone on the main thread.

ORDER: test_scan_from_eight_threads comes first and makes no scan before its threads start.  The slicing-by-8 CRC-32C tables
of the miniSEED 3 scanner are a function-local static that the first scan of a process builds; run on its own, this module's
first concurrent scans are the ones that build it.
"""
import ctypes as C

import numpy as np

from tests import trigger_cases as TC
from tests.mseed_util import mixed_file_bytes
from tests.thread_util import report, run_threads
from volpick_amd import _lib

THREADS, ROUNDS = 8, 50
I64 = C.POINTER(C.c_int64)
REC_BYTES = C.sizeof(_lib.VpMseedRecord)
CAP = 1024


def _scan(lib, buf, nbytes=None, cap=CAP):
    """(rc, n_found, the table's bytes) of one vp_mseed_scan."""
    recs, n = (_lib.VpMseedRecord * cap)(), C.c_int64(-1)
    rc = lib.vp_mseed_scan(buf, len(buf) if nbytes is None else nbytes, recs, cap, C.byref(n))
    return rc, n.value, bytes(recs)[: max(0, min(n.value, cap)) * REC_BYTES]


def _pick_host(lib, x, thr_on, thr_off):
    cap = len(x) // 2 + 2
    on, off, pk = np.empty(cap, np.int64), np.empty(cap, np.int64), np.empty(cap, np.int64)
    val, n = np.empty(cap, np.float32), C.c_int()
    rc = lib.vp_pick_host(x.ctypes.data_as(C.c_void_p), len(x), thr_on, thr_off, on.ctypes.data_as(I64), off.ctypes.data_as(I64),
                          pk.ctypes.data_as(I64), val.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n))
    k = n.value
    return rc, k, on[:k].tobytes(), off[:k].tobytes(), pk[:k].tobytes(), val[:k].tobytes()


# ------------------------------------------------------------------------------------------------------------------
# refusals whose text names a byte offset of the caller's choosing: the scanner steps over 64 zero bytes at a time
def truncated_v3(offset):
    """(buffer, text): a miniSEED 3 header at `offset` whose payload length runs past the end of the buffer."""
    assert offset % 64 == 0
    head = bytearray(40)
    head[0:3] = b"MS\x03"
    head[36:40] = (100).to_bytes(4, "little")
    return bytes(offset) + bytes(head), f"miniSEED 3 record at byte {offset} runs past the end of the buffer".encode()


def no_blockette_1000(offset):
    """(buffer, text): a miniSEED 2 data header at `offset` with an empty blockette chain."""
    assert offset % 64 == 0
    head = bytearray(64)
    head[0:7] = b"000001D"
    return bytes(offset) + bytes(head), f"mseed record at byte {offset} has no (valid) blockette 1000".encode()


NULL_TEXT = b"vp_mseed_scan: null argument"


def test_scan_from_eight_threads(lib):
    # FIRST in the module, and no scan before the threads start (see the module's docstring)
    buf = mixed_file_bytes()

    def worker():
        return [_scan(lib, buf) for _ in range(ROUNDS)]

    got, wall = run_threads([worker] * THREADS)
    rc, n, table = _scan(lib, buf)  # the serial table, made after the threads
    assert rc == 0 and 0 < n <= CAP and len(table) == n * REC_BYTES
    recs = np.frombuffer(table, dtype=np.dtype(_lib.VpMseedRecord))
    assert (recs["quality"] < 256).any() and (recs["quality"] >= 0x300).any()  # both formats are in it
    for k, rounds in enumerate(got):
        for i, r in enumerate(rounds):
            assert r == (rc, n, table), f"thread {k} round {i}: record table differs from the serial one"
    report(f"vp_mseed_scan, {n} records (v2 + v3)", THREADS, ROUNDS, wall)


def test_pick_host_a_case_per_thread(lib):
    cases = TC.all_cases()
    mine = [cases[k * len(cases) // THREADS] for k in range(THREADS)]
    assert mine[0].name == "alt_even"  # the longest trigger list
    assert len({c.name for c in mine}) == THREADS
    serial = [[_pick_host(lib, c.x, *p) for p in c.pairs] for c in mine]
    assert all(r[0] == 0 for s in serial for r in s) and sum(r[1] for s in serial for r in s) > 1500

    def worker(c):
        return lambda: [[_pick_host(lib, c.x, *p) for p in c.pairs] for _ in range(ROUNDS)]

    got, wall = run_threads([worker(c) for c in mine], names=[c.name for c in mine])
    for k, rounds in enumerate(got):
        for i, r in enumerate(rounds):
            assert r == serial[k], f"thread {k} ({mine[k].name}) round {i}: triggers differ from the serial ones"
    report("vp_pick_host, a trigger case per thread", THREADS, ROUNDS, wall)


def test_error_text_stays_with_its_thread(lib):
    buf = mixed_file_bytes()
    rc0, n0, table0 = _scan(lib, buf)
    x = TC.case("alt_odd").x
    pick0 = _pick_host(lib, x, 0.5, 0.25)
    assert rc0 == 0 and pick0[0] == 0

    def refuser(k):
        # offsets no other thread uses: 64 (1 + k) and 64 (101 + k)
        b3, text3 = truncated_v3(64 * (1 + k))
        b2, text2 = no_blockette_1000(64 * (101 + k))

        def run():
            for i in range(ROUNDS):
                for b, text in ((b3, text3), (b2, text2), (None, NULL_TEXT)):
                    n = C.c_int64(-7)
                    recs = (_lib.VpMseedRecord * 4)()
                    rc = lib.vp_mseed_scan(b, len(b) if b is not None else 64, recs, 4, C.byref(n))
                    seen = lib.vp_last_error()
                    assert rc == -1 and seen == text, f"round {i}: rc {rc}, expected {text!r}, vp_last_error() says {seen!r}"
            return 3 * ROUNDS
        return run

    def valid(k):
        b3, text = truncated_v3(64 * (201 + k))

        def run():
            assert lib.vp_mseed_scan(b3, len(b3), None, 0, C.byref(C.c_int64())) == -1  # this thread's one refusal
            assert lib.vp_last_error() == text
            for i in range(ROUNDS):
                assert _scan(lib, buf) == (rc0, n0, table0), f"round {i}: scan differs from the serial one"
                seen = lib.vp_last_error()
                assert seen == text, f"round {i}, after a valid scan: expected {text!r}, vp_last_error() says {seen!r}"
                assert _pick_host(lib, x, 0.5, 0.25) == pick0, f"round {i}: triggers differ from the serial ones"
                seen = lib.vp_last_error()
                assert seen == text, f"round {i}, after a valid pick: expected {text!r}, vp_last_error() says {seen!r}"
            return 2 * ROUNDS
        return run

    fns = [refuser(k) if k % 2 == 0 else valid(k) for k in range(THREADS)]
    got, wall = run_threads(fns, names=["refuser" if k % 2 == 0 else "valid" for k in range(THREADS)])
    assert got == [3 * ROUNDS, 2 * ROUNDS] * (THREADS // 2)
    report("vp_last_error, 4 refusing and 4 valid threads", THREADS, ROUNDS, wall, "every thread read its own text")
