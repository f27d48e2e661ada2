#!/usr/bin/env python
"""Times the late-element side output (fg_set_late_output) against the same handle with the mode
off, on the stream of `bench.py --workload datastream` (TumblingEventTimeWindows 1 s, sum over
(long, long), 10k keys, 1M records per event-second, micro-batches of 1M, a watermark every 10k
records).

One process keeps a handle with the mode off and handles with it on, on the same seeded stream
(bench.py's generator, resident in HBM) and alternates them, one bench step each (reset, the
micro-batches with their watermarks held and collected as bench.py does, the final Long.MAX_VALUE
watermark). The stream as bench.py makes it is in order: nothing is late. For a late share, that
fraction of the elements (picked by a hash of the record index) arrives 2 s behind its place in the
stream -- a bounded-out-of-orderness delay 2 s too short for them -- so from the third micro-batch on
each of them meets a fired window.

  1. step time on a host clock that ends at the last collect, medians and spread of --reps
     repetitions after a warm-up step, for: mode off; mode on with fg_collect_late (device columns)
     after every micro-batch, as a shim does; mode on with one collect at the end of the step
  2. the late_out class of kernel_stats per micro-batch, on a handle with kernel timing on (timing
     brackets every launch, so it is kept out of 1.)

    python scripts/late_output_time.py [--records 10000000] [--reps 5] [--shares 0,0.01,0.1]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

import bench   # noqa: E402
import flink_amd as F   # noqa: E402

JMAX = (1 << 63) - 1


def handle(wl, keys, batch, late_output, timing=False):
    wname, *wargs = wl["window"]
    return F.WindowAggOperator(getattr(F, wname)(*wargs), aggs=("sum",), val_type="i64", mode="datastream",
                               expected_keys=int(keys * 1.05) + 1, buffer_records=max(4 * batch, 1 << 26),
                               kernel_timing=timing, late_output=late_output)


def step(op, cols, wl, batch, wm_every, collect_late):
    """one bench step; collect_late: None (mode off), "batch" or "step". Returns (rows, late records)."""
    key, ts, val = cols
    n = key.numel()
    op.reset()
    rows, late, held = 0, 0, False
    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        if collect_late == "batch":
            late += len(op.collect_late(host=False)["key"])
        if held:
            rows += op.collect_fired().n
            held = False
        wms = bench.watermarks_for(lo, hi, wl["rate"], wm_every, wl["delay"], wl["jitter"])
        if wms:
            op.process_watermarks(wms)
            held = True
    if held:
        rows += op.collect_fired().n
    op.process_watermarks([JMAX])
    rows += op.collect_fired().n
    if collect_late == "step":
        late += len(op.collect_late(host=False)["key"])
    return rows, late


def timed(op, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = step(op, *a)
    return time.perf_counter() - t0, r


def spread(xs):
    return f"median {1e3 * statistics.median(xs):8.3f} ms  min {1e3 * min(xs):8.3f}  max {1e3 * max(xs):8.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shares", default="0,0.01,0.1")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["datastream"]
    n, keys, batch, wm_every = a.records, wl["keys"], min(wl["batch"], a.records), wl["wm_every"]
    key, ts0, val = bench.gen_columns(n, keys, wl["rate"], 0, dev, jitter=wl["jitter"], zipf=wl["zipf"])
    val = val.to(torch.int64)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    pick = bench.lsr(bench.splitmix64(idx ^ 0x1A7E), 11).to(torch.float64) * (1.0 / float(1 << 53))
    del idx
    print(f"== datastream: {n:,} records per step, {keys:,} keys, micro-batches of {batch:,}, a watermark every {wm_every:,}")
    for share in (float(s) for s in a.shares.split(",")):
        ts = torch.where(pick < share, ts0 - 2000, ts0)
        cols = (key, ts, val)
        torch.cuda.synchronize()
        variants = {"off": (handle(wl, keys, batch, False), None),
                    "on/batch": (handle(wl, keys, batch, True), "batch"),
                    "on/step": (handle(wl, keys, batch, True), "step")}
        times = {k: [] for k in variants}
        res = {}
        for k, (op, how) in variants.items():   # warm-up: allocations, region growth, the late columns
            timed(op, cols, wl, batch, wm_every, how)
        for _ in range(a.reps):
            for k, (op, how) in variants.items():
                t, res[k] = timed(op, cols, wl, batch, wm_every, how)
                times[k].append(t)
        dropped = variants["off"][0].num_late_records_dropped
        assert res["off"][0] == res["on/batch"][0] == res["on/step"][0], res
        assert res["on/batch"][1] == res["on/step"][1] == dropped, (res, dropped)
        print(f"-- late share asked {share:.2%}: {dropped:,} of {n:,} elements late ({dropped / n:.3%}), "
              f"{res['off'][0]:,} rows fired")
        for k in variants:
            print(f"1. step, {k:9s} {spread(times[k])}   reps (ms) {' '.join(f'{1e3 * t:.2f}' for t in times[k])}")
        m = {k: statistics.median(v) for k, v in times.items()}
        for k in ("on/batch", "on/step"):
            print(f"1. {k} - off: {1e3 * (m[k] - m['off']):+.3f} ms per step ({100 * (m[k] - m['off']) / m['off']:+.2f} %), "
                  f"off spread {1e3 * (max(times['off']) - min(times['off'])):.3f} ms")
        for op, _ in variants.values():
            op.close()
        op = handle(wl, keys, batch, True, timing=True)
        timed(op, cols, wl, batch, wm_every, "batch")
        op.synchronize()
        before = op.kernel_stats()
        timed(op, cols, wl, batch, wm_every, "batch")
        op.synchronize()
        after = op.kernel_stats()
        d = {f: after["late_out"][f] - before["late_out"][f] for f in ("launches", "total_ms", "records", "rows")}
        print(f"2. late_out: {d['launches']} batches, {d['records']:,} elements, {d['rows']:,} late records, "
              f"{d['total_ms']:.3f} ms per step = {1e3 * d['total_ms'] / max(d['launches'], 1):.1f} us per micro-batch "
              f"(count + scan + scatter)")
        op.close()
        del ts, cols


if __name__ == "__main__":
    main()
