#!/usr/bin/env python
"""Two CLASSIC handles on one seeded stream (200k records, 5k keys, DOUBLE values): how many DOUBLE
sums differ in their bits from one handle to the other, and by how many ulp. A DOUBLE SUM is
accumulated by LDS f64 atomics of several waves, so its summation order is the scheduler's; sums of
one or two values cannot differ. Why tests/test_gpu_fired_runs.py compares its twins on exactly
summable DOUBLE values.

    python scripts/double_sum_order_probe.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flink_amd as F   # noqa: E402
from tests.streams import make_stream   # noqa: E402

JMAX = (1 << 63) - 1
N, BATCH = 200_000, 25_000

for name, w in (("tumble", F.tumbling(1000)), ("hop", F.hopping(3000, 1000)), ("cumulate", F.cumulative(4000, 1000))):
    key, ts, val, _ = make_stream(N, 5_000, "f64", t0=1_600_000_000_000, rate_per_ms=25)
    out = []
    for rep in range(2):
        op = F.WindowAggOperator(w, expected_keys=5_000)
        rows = []
        for lo in range(0, N, BATCH):
            op.process_batch(key[lo:lo + BATCH], ts[lo:lo + BATCH], val[lo:lo + BATCH])
            rows.append(op.process_watermark(int(ts[lo:lo + BATCH].max()) - 1))
        rows.append(op.process_watermark(JMAX))
        r = np.concatenate(rows)
        out.append(r[np.lexsort((r["key"], r["window_end"]))])
        op.close()
    a, b = out
    d = np.abs(a["sum"].view(np.int64) - b["sum"].view(np.int64))
    same_other = all(np.array_equal(a[f], b[f]) for f in a.dtype.names if f not in ("sum", "avg"))
    print(f"probe {name}: rows {len(a)}, classic vs classic DOUBLE sums differing in bits {int((d > 0).sum())}, "
          f"max {int(d.max())} ulp, among rows with count <= 2: {int((d[a['count'] <= 2] > 0).sum())}; "
          f"other columns equal {same_other}", flush=True)
