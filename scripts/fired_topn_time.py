#!/usr/bin/env python
"""Times the Window Top-N selection (fg_set_fired_topn) at the headline's fire shape: one TUMBLE
window of `bench.py`'s stream (100M records of 10M uniform keys in one event-second, resident in
HBM) fired by one synchronous fg_advance_progress with FG_HOST output.

Per repetition (after a warm-up): reset, the batch, fg_synchronize, then the timed call. Printed:

  1. wall time of fg_advance_progress(FG_HOST) -- the fire, with --topn N > 0 the selection, and the
     copy of the returned rows to the host -- median, min and max of --reps repetitions
  2. with --topn N > 0, on a second handle with kernel timing on and the class mask on `topn` only:
     the class's time per fire, launches, rows in and out, and the bytes per fired row that time
     implies at 17 B read per row (order value, NULL byte, key)

--topn 0 leaves the selection off (every fired row is copied): the baseline form, which also runs
on a library built from a tree without the entry point (FLINKGPU_LIB=...).

    python scripts/fired_topn_time.py [--topn 100] [--agg count_star] [--records 100000000] [--reps 5]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

import bench   # noqa: E402
import flink_amd as F   # noqa: E402
from flink_amd import _lib as FL   # noqa: E402

JMAX = (1 << 63) - 1
AGGS = ("count_star", "sum", "avg")


def handle(keys, n, timing=False):
    return F.WindowAggOperator(F.tumbling(1000), aggs=AGGS, val_type="f64", expected_keys=int(keys * 1.05) + 1,
                               buffer_records=max(4 * n, 1 << 26), kernel_timing=timing)


def fire(op, cols):
    """one repetition: (seconds in fg_advance_progress(FG_HOST), rows returned, rows fired)"""
    op.reset()
    before = op.stats()["rows_fired"]
    op.process_batch(*cols)
    op.synchronize()
    r = FL.FgRows()
    t0 = time.perf_counter()
    FL.check(op._lib.fg_advance_progress(op._h, JMAX, FL.HOST, C.byref(r)), op._h)
    dt = time.perf_counter() - t0
    return dt, int(r.n), op.stats()["rows_fired"] - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topn", type=int, default=100)
    ap.add_argument("--agg", default="count_star")
    ap.add_argument("--ascending", action="store_true")
    ap.add_argument("--records", type=int, default=100_000_000, help="records of the one window")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    wl = bench.WORKLOADS["tumble"]
    dev = torch.device("cuda", 0)
    n = min(a.records, wl["rate"])   # (one event-second: one window)
    cols = bench.gen_columns(n, wl["keys"], wl["rate"], 0, dev)
    torch.cuda.synchronize()
    op = handle(wl["keys"], n)
    if a.topn > 0:
        op.set_fired_topn(a.topn, a.agg, not a.ascending)
    fire(op, cols)   # warm-up: allocations, region growth, the pinned host columns
    times = []
    for _ in range(a.reps):
        dt, returned, fired = fire(op, cols)
        times.append(dt)
    row_bytes = 8 * (3 + len(AGGS)) + 1
    print(f"== {n:,} records, {wl['keys']:,} keys, one window: {fired:,} rows fired, {returned:,} returned "
          f"(topn {a.topn}, order by {a.agg} {'asc' if a.ascending else 'desc'}); FG_HOST copy {returned * row_bytes:,} B")
    print(f"1. fg_advance_progress(FG_HOST): median {1e3 * statistics.median(times):.3f} ms  min {1e3 * min(times):.3f}  "
          f"max {1e3 * max(times):.3f}   reps (ms) {' '.join(f'{1e3 * t:.3f}' for t in times)}")
    op.close()
    if a.topn > 0:
        op = handle(wl["keys"], n, timing=True)
        op.set_fired_topn(a.topn, a.agg, not a.ascending)
        op.set_kernel_timing(["topn"])
        fire(op, cols)
        op.synchronize()
        ms = []
        for _ in range(a.reps):
            b = op.kernel_stats()["topn"]
            fire(op, cols)
            op.synchronize()
            k = op.kernel_stats()["topn"]
            ms.append(k["total_ms"] - b["total_ms"])
            rin, rout, ln = k["records"] - b["records"], k["rows"] - b["rows"], k["launches"] - b["launches"]
        med = statistics.median(ms)
        print(f"2. topn class per fire: median {med:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}  ({ln} bracket of 3 launches, "
              f"{rin:,} rows in, {rout:,} out); {1e6 * med / rin:.3f} ns per fired row, "
              f"{17 * rin / (med * 1e-3) / 1e12:.2f} TB/s at 17 B read per row")
        op.close()


if __name__ == "__main__":
    main()
