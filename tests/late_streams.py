"""The seeded streams of the late-output tests (tests/test_late_output_abi.py pins the reference
mask to the oracle on them, on the CPU; tests/test_gpu_late_output.py feeds them to the engine).

Every stream is tests.streams.make_stream cut into batches, each followed by a bounded-
out-of-orderness watermark (max rowtime so far - delay - 1). One record per millisecond with a
jitter several windows wide makes every batch after the first a mix of elements ahead of and
behind the watermark: the reference's late share of each such batch lies between 5 % and 95 %
(asserted in test_late_output_abi.py), so both the kept and the dropped side are exercised, and a
batch (5,000 records) spans more than one chunk of the compaction pass."""
from __future__ import annotations

import numpy as np

from tests.streams import make_stream

N, BATCH, KEYS = 40_000, 5_000, 200

# name -> window, allowed lateness, purging trigger, value type, how the batches are handed in
CONFIGS = {
    "tumble1s_f64": dict(window=("tumble", 1000), lateness=0, purging=False, val_type="f64", feed="batch",
                         jitter=3000, delay=0),
    "hop3s1s_i64": dict(window=("hop", 3000, 1000), lateness=0, purging=False, val_type="i64", feed="batch",
                        jitter=6000, delay=0),
    "tumble1s_late500_i64": dict(window=("tumble", 1000), lateness=500, purging=False, val_type="i64", feed="batch",
                                 jitter=3000, delay=0),
    "tumble1s_late500_purging_f64": dict(window=("tumble", 1000), lateness=500, purging=True, val_type="f64",
                                         feed="batch", jitter=3000, delay=0),
    "hop3s1s_late500_f64": dict(window=("hop", 3000, 1000), lateness=500, purging=False, val_type="f64",
                                feed="batch", jitter=6000, delay=0),
    "tumble1s_rows_f64": dict(window=("tumble", 1000), lateness=0, purging=False, val_type="f64", feed="rows",
                              jitter=3000, delay=0),
    "tumble1s_narrow_i64": dict(window=("tumble", 1000), lateness=0, purging=False, val_type="i64", feed="narrow",
                                jitter=3000, delay=0),
    "hop3s1s_noval": dict(window=("hop", 3000, 1000), lateness=0, purging=False, val_type="none", feed="batch",
                          jitter=6000, delay=0),
}


def stream_of(name, n=N):
    """(key, ts, val, isnull) of a configuration: f64 values are multiples of 2^-10 (their sums
    are exact in any order), 10 % of the values NULL; val / isnull None without a value column."""
    c = CONFIGS[name]
    vt = c["val_type"]
    key, ts, val, isnull = make_stream(n, KEYS, "i64" if vt == "none" else vt, rate_per_ms=1, jitter_ms=c["jitter"],
                                       null_frac=0.1, seed=0x5EEDF11C + len(name))
    if vt == "f64":
        val = np.floor(val * 1024.0) / 1024.0
    if vt == "none":
        val, isnull = None, None
    return key, ts, val, isnull


def batches_of(name, ts, batch=BATCH):
    """(lo, hi, watermark after the batch)"""
    delay = CONFIGS[name]["delay"]
    mx = np.iinfo(np.int64).min
    for lo in range(0, len(ts), batch):
        hi = min(len(ts), lo + batch)
        mx = max(mx, int(ts[lo:hi].max()))
        yield lo, hi, mx - delay - 1
