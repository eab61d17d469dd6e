"""The library from several host threads at once, on the GPU: the trace operations' per-device scratch and its lock, the
release calls against calls in flight, the thread-local error text, models and trainers on threads of their own, the
first-come-first-served gate of chip-filling PhaseNet launches under two submitters.

One rule for every case.  The calls are first made serially, one after another on the main thread, TWICE, and the two serial
results must be bit-identical (the kernels use no floating-point atomics; the integer trigger appends are sorted by the host).
Then the same calls are made from threads, released together, and every thread's every result must be bit-identical to the
serial one: dtype, shape and bytes, NaNs included.  There is no tolerance in this module.

The contract under test is "one handle, one thread at a time": no model, trainer or handle is shared between two running
threads (it may be created on one thread and used on another), and nothing here is built to make anything fault.  Every case
is a few seconds of work; tests/thread_util.py joins its threads under a cap of 120 s, and once a thread has run into the cap
no later case of this module touches the GPU.  Each case prints its thread count, rounds and wall time.
"""
import ctypes as C
import functools
import struct
import time

import numpy as np
import pytest

from tests import attributes_f64 as A
from tests import decimate_f64 as D
from tests import fourier_f64 as F
from tests import sosfilt_f64 as S
from tests import thread_util as TU
from tests.mseed_util import file_bytes, three_component
from volpick_amd import _lib

pytestmark = pytest.mark.gpu

ROUNDS = 8
VP_ERR_INVALID, VP_ERR_UNSUPPORTED = -1, -4
SENTINEL = -7.0


# ------------------------------------------------------------------------------------------------------------------
# bit-exact comparison
def bits(v):
    """`v` as something `==` compares bit for bit: arrays and tensors as (dtype, shape, bytes), floats as their eight bytes."""
    if hasattr(v, "data_ptr"):  # a torch tensor
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, (float, np.floating)):
        return ("f64", struct.pack("<d", float(v)))
    if isinstance(v, (tuple, list)):
        return tuple(bits(u) for u in v)
    if isinstance(v, dict):
        return tuple((k, bits(u)) for k, u in v.items())
    assert v is None or isinstance(v, (int, str, bytes, bool, np.integer)), type(v)
    return v


def where_differs(a, b):
    """A few words on the first difference of two `bits` values, for the assertion message."""
    if isinstance(a, tuple) and isinstance(b, tuple) and len(a) == 3 and isinstance(a[2], bytes) and isinstance(b[2], bytes):
        if a[:2] != b[:2]:
            return f"{a[:2]} against {b[:2]}"
        x, y = np.frombuffer(a[2], np.uint8), np.frombuffer(b[2], np.uint8)
        bad = np.flatnonzero(x != y)
        return f"{a[0]}{a[1]}: {len(bad)} bytes differ, the first at byte {int(bad[0])}"
    if isinstance(a, tuple) and isinstance(b, tuple):
        if len(a) != len(b):
            return f"{len(a)} items against {len(b)}"
        for i, (u, w) in enumerate(zip(a, b)):
            if u != w:
                return f"item {i}: {where_differs(u, w)}"
    return f"{a!r:.80} against {b!r:.80}"


class Job:
    """One thread's work: ``run(i)`` is its call of round i; rounds i and i + distinct make the same call.  ``rounds=None``
    takes the module's 8."""

    def __init__(self, label, run, distinct=1, rounds=None):
        self.label, self.run, self.distinct, self.rounds = label, run, distinct, ROUNDS if rounds is None else rounds


def serial_twice(jobs):
    """Every distinct call of every job, one after another on this thread, twice -> the results of the first pass."""
    passes = [[[bits(j.run(i)) for i in range(j.distinct)] for j in jobs] for _ in range(2)]
    for j, first, second in zip(jobs, *passes):
        for i, (u, w) in enumerate(zip(first, second)):
            assert u == w, f"SERIAL MISMATCH, {j.label}, call {i}: two serial runs differ: {where_differs(u, w)}"
    return passes[0]


def threaded(case, jobs, serial, extra=(), before_threads=None):
    """The jobs on a thread each (and `extra`: (label, callable) threads whose return value the caller checks); every result
    against `serial`.  Returns what the extra threads returned."""
    if before_threads is not None:
        before_threads()

    def worker(j):
        return lambda: [bits(j.run(i)) for i in range(j.rounds)]

    fns = [worker(j) for j in jobs] + [f for _, f in extra]
    got, wall = TU.run_threads(fns, names=[j.label for j in jobs] + [label for label, _ in extra])
    for k, j in enumerate(jobs):
        assert len(got[k]) == j.rounds
        for i, r in enumerate(got[k]):
            want = serial[k][i % j.distinct]
            assert r == want, f"{case}: thread {k} ({j.label}) round {i} differs from the serial result: {where_differs(r, want)}"
    TU.report(case, len(fns), max(j.rounds for j in jobs), wall)
    return got[len(jobs):]


def run_case(case, jobs, extra=(), before_threads=None):
    TU.check_not_stuck()
    return threaded(case, jobs, serial_twice(jobs), extra, before_threads)


# ------------------------------------------------------------------------------------------------------------------
# the trace operations through the Python surface
FILTER_LENGTHS = (8_193, 40_003, 100_001, 262_147)
DECIMATE_LENGTHS = (50, D.TILE + 1, 2 * D.TILE + 33, D.N_LONG)  # the seams of tests/test_gpu_decimate.py, ascending
# tests/test_gpu_fourier.py: either side of the one-pass / two-pass switch, the long trace, the first three-pass length
FOURIER_LENGTHS = ((F.length_for_passes(1, 0), 250), (F.length_for_passes(1, 1), 250), (F.N_LONG, 80), (F.length_for_passes(2, 1), 250))
KIND_OF_THREAD = ("int32", "float32", "float64", "int32")
FILTER_OF_THREAD = ("highpass 0.3 Hz", "bandpass 1-20 Hz", "highpass 1 Hz, 3 corners", "lowpass 20 Hz")
DETREND_OF_THREAD = ("simple", "linear", "demean", "linear")


def on_device(x, kind_name):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(D.KINDS[kind_name][1]))).cuda()


@functools.lru_cache(maxsize=None)
def mseed_buffer(n, k):
    """Three components of n samples: Steim-2 records for the short files, int32 records (miniSEED 3 for odd k) for the long."""
    from oracle import mseed as OM

    traces = three_component(n, np.random.default_rng(500 + n % 977), sta=f"T{k}")
    if n <= 50_000:
        return file_bytes(traces, reclen=512 if k % 2 == 0 else 4096)
    return OM.write_mseed3(traces, encoding=3, max_payload=4096) if k % 2 else file_bytes(traces, reclen=4096, encoding=3)


def read_job(n, k, device_resident):
    import volpick_amd as va

    buf = mseed_buffer(n, k)

    def run(i):
        st = va.read(buf, device_resident=device_resident)
        assert len(st) == 3 and all(tr.stats.npts == n for tr in st)
        return [(tr.id, tr._dev if device_resident else tr.data) for tr in st]

    return Job(f"read {n} samples" + (" (device)" if device_resident else ""), run)


def decimate_job(n, k):
    from volpick_amd.resample import decimate_device

    factor = D.FACTORS[k % len(D.FACTORS)]
    x = on_device(D.counts(n, 100 + k), KIND_OF_THREAD[k % 4])
    return Job(f"decimate {n} by {factor}", lambda i: decimate_device(x, D.RATE_OUT * factor, D.RATE_OUT))


def fourier_job(n, rate, k):
    from volpick_amd.resample import fourier_device

    x = on_device(D.counts(n, 3 * n + rate), KIND_OF_THREAD[k % 4])
    return Job(f"fourier {n} at {rate} Hz", lambda i: fourier_device(x, float(rate), F.RATE_OUT))


def sos_job(n, k, zerophase):
    from volpick_amd.signal import sos_filter_device

    name = FILTER_OF_THREAD[k % 4]
    x, sos = on_device(S.trace(n), KIND_OF_THREAD[k % 4]), S.sos_of(name)
    return Job(f"{name}, {n} samples" + (", zero-phase" if zerophase else ""), lambda i: sos_filter_device(x, sos, zerophase=zerophase))


def detrend_job(n, k):
    from volpick_amd.signal import detrend_device

    x, kind = on_device(S.trace(n), KIND_OF_THREAD[k % 4]), DETREND_OF_THREAD[k % 4]
    return Job(f"detrend {kind}, {n} samples", lambda i: detrend_device(x, kind))


# rows and frequency-index window per thread: the scratch holds the staged rows (and grows with them), the kernel's dynamic
# LDS follows the longest window of the call (the last one is at the cap of 2048 samples)
ATTR_OF_THREAD = ((4, (1.0, 6.0), 5.0), (60, (2.0, 8.0), 10.0), (600, (1.0, 3.0), 2.0), (2400, (10.24, 10.24), 20.48))


def attributes_job(n, k, shape=None):
    import torch

    from volpick_amd import attributes as VA

    n_rows, fi_window, snr_window = shape or ATTR_OF_THREAD[k % 4]
    x = torch.from_numpy(A.noise(n, 70 + k, 2.0, 1e4)).cuda()
    rng = np.random.default_rng(k)
    p = rng.integers(0, n, n_rows).astype(np.float64)
    s = p + rng.integers(100, 900, n_rows)
    s[::5] = np.nan
    p[3::7] = np.nan
    s = np.where(s < n, s, np.nan)
    rows = VA.plan_rows([n] * n_rows, p, s, 100, fi_window=fi_window, snr_window=snr_window, demean=bool(k % 2))
    rows["trace"] = 0
    return Job(f"attributes, {n_rows} rows of {n} samples", lambda i: VA.array_attributes(x, rows, raw=True))


def release_all():
    from volpick_amd.io import release_decode_scratch
    from volpick_amd.resample import release_decimate_scratch, release_fourier_scratch
    from volpick_amd.signal import release_filter_scratch

    return [f(0) for f in (release_decode_scratch, release_decimate_scratch, release_fourier_scratch, release_filter_scratch)]


OPERATIONS = {
    "read": lambda: [read_job(n, k, False) for k, n in enumerate(FILTER_LENGTHS)],
    "read, device resident": lambda: [read_job(n, k, True) for k, n in enumerate(FILTER_LENGTHS)],
    "decimate": lambda: [decimate_job(n, k) for k, n in enumerate(DECIMATE_LENGTHS)],
    "fourier": lambda: [fourier_job(n, rate, k) for k, (n, rate) in enumerate(FOURIER_LENGTHS)],
    "sos filter, one pass": lambda: [sos_job(n, k, False) for k, n in enumerate(FILTER_LENGTHS)],
    "sos filter, zero phase": lambda: [sos_job(n, k, True) for k, n in enumerate(FILTER_LENGTHS)],
    "detrend": lambda: [detrend_job(n, k) for k, n in enumerate(FILTER_LENGTHS)],
    "attributes": lambda: [attributes_job(n, k) for k, n in enumerate(FILTER_LENGTHS)],
}


@pytest.mark.parametrize("operation", list(OPERATIONS))
def test_a_one_operation_on_four_threads_with_growing_lengths(operation):
    """Thread k works on length n_k, ascending: the grow-only scratch is freed and enlarged while the others wait for its
    lock.  The scratch is released before the threads start, so the first concurrent call allocates."""
    TU.check_not_stuck()
    jobs = OPERATIONS[operation]()
    assert len(jobs) == 4
    run_case(f"a. {operation}", jobs, before_threads=release_all)


def test_b_five_operations_at_once():
    """A thread per operation, lengths cycling over three sizes: five pools, four of them on the null stream."""
    TU.check_not_stuck()
    sizes = FILTER_LENGTHS[:3]

    def cycle(label, make):
        made = [make(n, k) for k, n in enumerate(sizes)]
        return Job(label, lambda i: made[i % 3].run(i), distinct=3)

    def filter_then_detrend(n, k):
        from volpick_amd.signal import detrend_device

        f = sos_job(n, k, True)
        return Job(f.label + ", then detrend", lambda i: detrend_device(f.run(i), "linear"))

    jobs = [
        cycle("decode", lambda n, k: read_job(n, k, False)),
        cycle("decimate", lambda n, k: decimate_job(DECIMATE_LENGTHS[k + 1], k)),
        cycle("fourier", lambda n, k: fourier_job(*FOURIER_LENGTHS[k], k)),
        cycle("filter + detrend", filter_then_detrend),
        cycle("attributes", lambda n, k: attributes_job(n, k)),
    ]
    run_case("b. five operations at once", jobs, before_threads=release_all)


RELEASES = {
    "vp_mseed_release_scratch": lambda k, n: read_job(n, k, False),
    "vp_decimate_release_scratch": lambda k, n: decimate_job(n, k),
    "vp_resample_release_scratch": lambda k, n: fourier_job(n, 250, k),
    "vp_sos_filter_release_scratch": lambda k, n: sos_job(n, k, True),
}


@pytest.mark.parametrize("symbol", list(RELEASES))
def test_c_release_against_calls(symbol):
    """Two threads call the operation, a third frees its scratch between (and behind) their calls."""
    TU.check_not_stuck()
    lib = _lib.load()
    jobs = [RELEASES[symbol](k, n) for k, n in enumerate((40_003, 100_001))]

    def releaser():
        out = []
        for _ in range(ROUNDS):
            freed = C.c_size_t(0)
            out.append((getattr(lib, symbol)(0, C.byref(freed)), int(freed.value)))
            time.sleep(0.001)
        return out

    (freed,) = run_case(f"c. {symbol} against calls", jobs, extra=[("release", releaser)])
    assert len(freed) == ROUNDS and all(rc == 0 and n >= 0 for rc, n in freed), freed
    print(f"   bytes freed per release: {[n for _, n in freed]}")


def test_d_error_text_on_the_gpu_entry_points():
    """A is refused by vp_sos_filter (host validation, nothing launched), B filters, C is refused by vp_decimate_lowpass: each
    refused thread reads its own text after every call, B's results stay identical."""
    import torch

    from volpick_amd.resample import lowpass_sos

    TU.check_not_stuck()
    lib = _lib.load()
    n = 10_000
    d = on_device(S.trace(n), "int32")
    out_a = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    sos = np.ascontiguousarray(S.sos_of("highpass 0.3 Hz"), dtype=np.float64)
    five = np.ascontiguousarray(np.tile(sos, (3, 1))[:5])
    long_warmup = np.ascontiguousarray(lowpass_sos(50.0, 25000.0), dtype=np.float64)
    factor = 250
    out_c = torch.full(((n + factor - 1) // factor,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    DP = C.POINTER(C.c_double)
    kind = D.KINDS["int32"][0]

    def sos_call(in_kind, count, table):
        return lib.vp_sos_filter(0, C.c_void_p(d.data_ptr()), in_kind, count, table.ctypes.data_as(DP), len(table), 0,
                                 C.c_void_p(out_a.data_ptr()))

    refusals = (("vp_sos_filter: n_sections = 5", lambda: sos_call(kind, n, five)),
                ("vp_sos_filter: in_kind 3", lambda: sos_call(3, n, sos)),
                ("vp_sos_filter: n = -1 is negative", lambda: sos_call(kind, -1, sos)))

    def thread_a():
        for i in range(50):
            for text, call in refusals:
                rc = call()
                seen = _lib.last_error()
                assert rc == VP_ERR_INVALID and seen.startswith(text), f"round {i}: rc {rc}, expected '{text}...', read '{seen}'"
        return "a"

    def thread_c():
        for i in range(50):
            rc = lib.vp_decimate_lowpass(0, C.c_void_p(d.data_ptr()), kind, n, long_warmup.ctypes.data_as(DP), len(long_warmup),
                                         factor, C.c_void_p(out_c.data_ptr()), out_c.shape[0])
            seen = _lib.last_error()
            assert rc == VP_ERR_UNSUPPORTED and seen.startswith("vp_decimate_lowpass: largest pole radius"), \
                f"round {i}: rc {rc}, read '{seen}'"
        return "c"

    assert thread_a() == "a" and thread_c() == "c"  # alone first: these are the texts
    jobs = [sos_job(40_003, 1, True)]
    assert run_case("d. error text beside valid calls", jobs, extra=[("refused filter", thread_a), ("refused decimate", thread_c)]) == ["a", "c"]
    torch.cuda.synchronize()
    assert bool((out_a == SENTINEL).all()) and bool((out_c == SENTINEL).all())  # the refusals wrote nothing


# ------------------------------------------------------------------------------------------------------------------
# models
def make_stream(n, seed, station):
    import volpick_amd as va
    from volpick_amd.synthetic import synthetic_stream_array

    data, _, _ = synthetic_stream_array(n, seed=seed)
    t0 = va.UTCDateTime("2021-01-01T00:00:00")
    return va.Stream([va.Trace(data[i], dict(network="XX", station=station, location="", channel=f"HH{c}", starttime=t0,
                                             sampling_rate=100.0)) for i, c in enumerate("ZNE")])


def picks_and_rows(model, stream, **kw):
    """What classify() and annotate() give for `stream`, as plain values."""
    res = model.classify(stream, **kw)
    us = lambda t: None if t is None else int(t._us)
    picks = [(p.trace_id, p.phase, us(p.start_time), us(p.end_time), us(p.peak_time), float(p.peak_value)) for p in res.picks]
    dets = [(q.trace_id, us(q.start_time), us(q.end_time), float(q.peak_value)) for q in (getattr(res, "detections", None) or [])]
    rows = [(tr.id, int(tr.stats.starttime._us), np.asarray(tr.data)) for tr in model.annotate(stream, **kw)]
    return picks, dets, rows


class ModelSpec:
    """A model kind, the stream it classifies and the windows that stream gives."""

    def __init__(self, label, kind, n_windows, overlap, seed, flags=None):
        import volpick_amd as va

        self.label, self.cls, self.flags = label, getattr(va, kind), flags
        self.n_windows, self.overlap = n_windows, overlap
        T = 3001 if kind == "PhaseNet" else 6000
        self.n = T + (n_windows - 1) * (T - overlap)
        assert int(_lib.load().vp_window_starts(self.n, T, overlap, None, 0)) == n_windows
        self.stream = make_stream(self.n, seed, f"S{seed}")
        self.kw = dict(overlap=overlap, batch_size=256)

    def create(self):
        m = self.cls.from_pretrained("volpick")
        if self.flags is not None:
            m._plan_flags = self.flags
        return m.cuda()


def model_jobs(specs, rounds, in_thread):
    """-> (jobs for the serial passes, jobs for the threads, close()).  `in_thread`: each thread's model is created by the
    thread itself at its first call; otherwise on this thread, and handed over."""
    made = []

    def job(spec, lazy):
        box = {}

        def run(i):
            if "m" not in box:
                box["m"] = spec.create()
                made.append(box["m"])
            return picks_and_rows(box["m"], spec.stream, **spec.kw)

        if not lazy:
            box["m"] = spec.create()
            made.append(box["m"])
        return Job(spec.label, run, rounds=rounds)

    def close():
        for m in made:
            m._release()

    return [job(s, False) for s in specs], [job(s, in_thread) for s in specs], close


def check_models(case, specs, rounds, in_thread, extra=()):
    TU.check_not_stuck()
    serial_jobs, thread_jobs, close = model_jobs(specs, rounds, in_thread)
    try:
        serial = serial_twice(serial_jobs)
        for s, r in zip(specs, serial):
            assert len(r[0][0]) > 0 and len(r[0][2]) == 3, f"{s.label}: no picks or no annotated rows to compare"
        return threaded(case, thread_jobs, serial, extra)
    finally:
        if TU.STUCK is None:
            close()


@pytest.mark.parametrize("in_thread", (False, True), ids=("handed over", "created in the thread"))
def test_e_three_models_on_three_threads(in_thread):
    """A gated PhaseNet (200 windows in one forward batch), an ungated one (20 windows), an EQTransformer (8 windows), while
    a fourth thread creates and destroys a spare PhaseNet: vp_create / vp_destroy beside running forwards."""
    import volpick_amd as va

    specs = [ModelSpec("PhaseNet, 200 windows (gated)", "PhaseNet", 200, 1500, 31),
             ModelSpec("PhaseNet, 20 windows", "PhaseNet", 20, 1500, 32),
             ModelSpec("EQTransformer, 8 windows", "EQTransformer", 8, 3000, 33)]
    assert specs[0].n_windows >= 192 > specs[1].n_windows

    def spare():
        for _ in range(4):
            va.PhaseNet.from_pretrained("volpick").cuda()._release()
        return 4

    assert check_models(f"e. three models, {'created in their threads' if in_thread else 'handed over'}", specs, 6, in_thread,
                        extra=[("spare PhaseNet", spare)]) == [4]


@pytest.mark.parametrize("flags", (None, (0, 0, 0, 64)), ids=("gate on", "gate off"))
def test_f_two_gated_phasenets(flags):
    """Two submitters on the ForwardGate ring of the device (and the same with the gate switched off: same numbers)."""
    specs = [ModelSpec("PhaseNet, 200 windows", "PhaseNet", 200, 1500, 41, flags),
             ModelSpec("PhaseNet, 230 windows", "PhaseNet", 230, 1500, 42, flags)]
    assert all(s.n_windows >= 192 for s in specs)
    check_models(f"f. two chip-filling PhaseNets, {'gate off' if flags else 'gate on'}", specs, 10, False)


# ------------------------------------------------------------------------------------------------------------------
# trainers
def trainer_job(dtype, seed, lr=1e-3, steps=3, B=6):
    """-> (new(), Job factory): `new()` creates a trainer (on the calling thread), the job takes `steps` Adam steps with it and
    returns the losses, the launch count after each step, the weights and the Adam state."""
    from tests.test_gpu_train import make_batch
    from volpick_amd import PhaseNet
    from volpick_amd.train import PhaseNetTrainer

    x, y = make_batch(B, seed)

    def new():
        return PhaseNetTrainer(PhaseNet.from_pretrained("volpick"), max_batch=8, dtype=dtype)

    def job(tr):
        def run(i):
            losses, launches = [], []
            for _ in range(steps):
                losses.append(tr.step(x, y, lr))
                launches.append(int(tr._lib.vp_train_launch_count(tr._h)))
            assert all(np.isfinite(losses)) and all(c > 0 for c in launches)
            return losses, launches, tr._read(0), tr._read(2), tr._read(3)

        return Job(f"trainer {dtype}, B = {B}", run, rounds=1)

    return new, job


def check_trainers(case, makers, other_jobs=()):
    """`makers`: trainer_job(...) pairs.  Serial: twice, a fresh trainer each time.  Threads: the trainers are created here,
    before the barrier, and take their first step behind it."""
    TU.check_not_stuck()
    serial = []
    for _ in range(2):
        trainers = [new() for new, _ in makers]
        serial.append([[bits(job(tr).run(0))] for (_, job), tr in zip(makers, trainers)])
        for tr in trainers:
            tr.close()
    for k, (u, w) in enumerate(zip(*serial)):
        assert u == w, f"SERIAL MISMATCH, trainer {k}: two serial runs differ: {where_differs(u[0], w[0])}"
    others = list(other_jobs)
    serial_others = serial_twice(others)
    trainers = [new() for new, _ in makers]
    try:
        threaded(case, [job(tr) for (_, job), tr in zip(makers, trainers)] + others, serial[0] + serial_others)
    finally:
        if TU.STUCK is None:
            for tr in trainers:
                tr.close()
    return serial[0]


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_g_trainer_beside_inference_and_a_filter(dtype):
    """Three Adam steps while a PhaseNet runs forwards on a thread of its own and a third thread filters."""
    import torch

    from volpick_amd import PhaseNet
    from volpick_amd.synthetic import synthetic_windows

    TU.check_not_stuck()
    model = PhaseNet.from_pretrained("volpick").cuda()
    xw = torch.from_numpy(synthetic_windows(20, 3001, seed=5)).cuda()
    try:
        check_trainers(f"g. {dtype} trainer beside forwards and a filter", [trainer_job(dtype, 7)],
                       [Job("PhaseNet forward, 20 windows", lambda i: model(xw)), sos_job(100_001, 2, True)])
    finally:
        if TU.STUCK is None:
            model._release()


def test_h_two_trainers_on_two_threads():
    """fp32 and bf16, different batches, created before the barrier, first step behind it (the bf16 one then meets
    launch_wgrad_bf16's set-once flag); each trainer's launch counts are its serial ones (a thread-local counter)."""
    serial = check_trainers("h. an fp32 and a bf16 trainer", [trainer_job("fp32", 7), trainer_job("bf16", 8)])
    print(f"   launches per step: fp32 {list(serial[0][0][1])}, bf16 {list(serial[1][0][1])}")
