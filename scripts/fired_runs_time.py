#!/usr/bin/env python
"""Times run mode (fg_set_fired_runs: fired rows without their window_start / window_end / rowtime
columns, a run directory instead) against the classic output form, on the shapes of
`bench.py`, `bench.py --workload hop` and `bench.py --workload cumulate`.

One process keeps a classic and a run-mode handle on the same seeded stream (bench.py's generator,
resident in HBM) and alternates them, one bench step each (reset, the micro-batches with their
watermarks held and collected as bench.py does, the final Long.MAX_VALUE watermark):

  1. step time on a host clock that ends at the last collect, medians and spread of --reps
     repetitions after a warm-up step
  2. the fire classes' total_ms of kernel_stats for one step, on a second pair of handles with
     kernel timing on (timing brackets every launch, so it is kept out of 1.)
  3. bytes of the FG_HOST copy-out of one step's rows, from the shapes: (8 (1 + aggs) + 1) n
     against (8 (3 + aggs) + 1) n
  4. (cumulate, the workload with the most rows) the wall time one step spends in
     fg_collect_fired_to(FG_HOST), the call behind collect_fired(host=True)

    python scripts/fired_runs_time.py [--records 1000000000] [--reps 5] [--workloads tumble,hop,cumulate]
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
FIRE_CLASSES = ("merge_flush_fire", "merge_fire", "tile_fire", "tile_split_fire")


def handle(wl, keys, batch, runs, timing=False):
    wname, *wargs = wl["window"]
    return F.WindowAggOperator(getattr(F, wname)(*wargs), aggs=AGGS, val_type="f64", expected_keys=int(keys * 1.05) + 1,
                               buffer_records=max(4 * batch, 1 << 26), kernel_timing=timing, fired_runs=runs)


def step(op, cols, wl, batch, wm_every, host=False):
    """one bench step; returns (rows, seconds spent inside the collects)"""
    key, ts, val = cols
    n = key.numel()
    op.reset()
    rows, held, in_collect = 0, False, 0.0

    def collect():
        nonlocal rows, in_collect
        c0 = time.perf_counter()
        if host:   # the library call a JVM shim makes (no numpy copy of the columns on top)
            r = FL.FgRows()
            FL.check(op._lib.fg_collect_fired_to(op._h, FL.HOST, C.byref(r)), op._h)
        else:
            r = op.collect_fired()
        in_collect += time.perf_counter() - c0
        rows += r.n

    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        if held:
            collect()
            held = False
        wms = bench.watermarks_for(lo, hi, wl["rate"], wm_every, wl["delay"], wl["jitter"])
        if wms:
            op.process_watermarks(wms)
            held = True
    if held:
        collect()
    op.process_watermarks([JMAX])
    collect()
    return rows, in_collect


def timed(op, cols, wl, batch, wm_every, host=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows, in_collect = step(op, cols, wl, batch, wm_every, host)
    return time.perf_counter() - t0, rows, in_collect


def spread(xs):
    return f"median {1e3 * statistics.median(xs):9.3f} ms  min {1e3 * min(xs):9.3f}  max {1e3 * max(xs):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000_000, help="records per step (at least 100M)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="tumble,hop,cumulate")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.workloads.split(","):
        wl = bench.WORKLOADS[name]
        n, keys, batch, wm_every = a.records, wl["keys"], min(wl["batch"], a.records), wl.get("wm_every", 1_000_000)
        cols = bench.gen_columns(n, keys, wl["rate"], 0, dev, jitter=wl["jitter"], zipf=wl["zipf"])
        torch.cuda.synchronize()
        print(f"== {name}: {n:,} records per step, {keys:,} keys, micro-batches of {batch:,}, aggregates {','.join(AGGS)}")
        ops = {"classic": handle(wl, keys, batch, False), "runs": handle(wl, keys, batch, True)}
        times = {k: [] for k in ops}
        rows = {}
        for k, op in ops.items():   # warm-up: allocations, region growth
            timed(op, cols, wl, batch, wm_every)
        for _ in range(a.reps):
            for k, op in ops.items():
                t, rows[k], _ = timed(op, cols, wl, batch, wm_every)
                times[k].append(t)
        assert rows["classic"] == rows["runs"], rows
        nr = rows["runs"]
        for k in ops:
            print(f"1. step, {k:8s} {spread(times[k])}   reps (ms) {' '.join(f'{1e3 * t:.2f}' for t in times[k])}")
        mc, mr = statistics.median(times["classic"]), statistics.median(times["runs"])
        print(f"1. runs - classic: {1e3 * (mr - mc):+.3f} ms per step ({100 * (mr - mc) / mc:+.2f} %), "
              f"classic spread {1e3 * (max(times['classic']) - min(times['classic'])):.3f} ms; "
              f"per 1B records: classic {mc * 1e12 / n:.2f} ms, runs {mr * 1e12 / n:.2f} ms")
        b_classic, b_runs = (8 * (3 + len(AGGS)) + 1) * nr, (8 * (1 + len(AGGS)) + 1) * nr
        print(f"3. rows per step {nr:,}; FG_HOST copy-out bytes: classic {b_classic:,}  runs {b_runs:,}  "
              f"(x {b_runs / b_classic:.3f})")
        if name == "cumulate":
            hc = {k: [] for k in ops}
            for k, op in ops.items():   # warm-up: the pinned host columns
                timed(op, cols, wl, batch, wm_every, host=True)
            for _ in range(a.reps):
                for k, op in ops.items():
                    _, _, c = timed(op, cols, wl, batch, wm_every, host=True)
                    hc[k].append(c)
            for k in ops:
                print(f"4. collect_fired(host=True) per step, {k:8s} {spread(hc[k])}")
            print(f"4. runs / classic: x {statistics.median(hc['runs']) / statistics.median(hc['classic']):.3f}")
        for op in ops.values():
            op.close()
        # kernel timing on: the fire classes of one step
        for k, runs in (("classic", False), ("runs", True)):
            op = handle(wl, keys, batch, runs, timing=True)
            timed(op, cols, wl, batch, wm_every)
            op.synchronize()
            before = op.kernel_stats()
            timed(op, cols, wl, batch, wm_every)
            op.synchronize()
            after = op.kernel_stats()
            d = {c: after[c]["total_ms"] - before[c]["total_ms"] for c in FIRE_CLASSES}
            ln = {c: after[c]["launches"] - before[c]["launches"] for c in FIRE_CLASSES}
            print(f"2. fire classes, {k:8s} total {sum(d.values()):9.3f} ms  " +
                  "  ".join(f"{c} {d[c]:.3f} ms / {ln[c]}" for c in FIRE_CLASSES if ln[c]))
            op.close()
        del cols
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
