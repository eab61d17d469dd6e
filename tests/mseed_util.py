"""Synthetic miniSEED inputs shared by the CPU and GPU ingestion tests (made with the oracle's encoder)."""
import numpy as np

from oracle import mseed as OM

T0 = 1_600_000_000_123_400  # a BTIME-representable start (multiple of 100 us)


def seismogram(n, rng, scale=300, spikes=True):
    """Random-walk counts with occasional large steps so every Steim word kind occurs."""
    d = rng.integers(-scale, scale + 1, n)
    small = rng.random(n) < 0.5
    d = np.where(small, rng.integers(-7, 8, n), d)
    if spikes:
        big = rng.random(n) < 0.01
        d = np.where(big, rng.integers(-(1 << 27), 1 << 27, n), d)
    return np.clip(np.cumsum(d), -(1 << 30), (1 << 30) - 1).astype(np.int32)


def three_component(n, rng, start_us=T0, rate=100.0, net="XX", sta="VOLC", loc="", band="HH", **kw):
    return [dict(network=net, station=sta, location=loc, channel=band + c, start_us=start_us, rate=rate,
                 data=seismogram(n, rng, **kw)) for c in "ZNE"]


def file_bytes(traces, **kw):
    return OM.write_mseed(traces, **kw)


def mixed_file_bytes(seed=71, n=20000):
    """One buffer of miniSEED 2 records (512 bytes, Steim-2) followed by miniSEED 3 records (Steim-2, with extra headers): what
    the threading tests scan from several threads at once."""
    rng = np.random.default_rng(seed)
    v2 = file_bytes(three_component(n, rng), with_b1001=True)
    v3 = OM.write_mseed3(three_component(n, rng, sta="VOL3"), max_payload=640, extra_headers=b'{"a":1}')
    return v2 + v3
