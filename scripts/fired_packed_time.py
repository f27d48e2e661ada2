#!/usr/bin/env python
"""Times fg_fired_packed at the headline's fire shape: one TUMBLE window of `bench.py`'s stream (100M
records of 10M uniform keys in one event-second, resident in HBM; 3 aggregates) fired by one
synchronous fg_advance_progress -- about 10M fired rows.

Per repetition (after a warm-up): reset, the batch, fg_synchronize, then the timed calls. Printed:

  (a) on a handle with kernel timing on and the class mask on `pack_rows` only: the class's time per
      call, launches and rows, the bytes the kernel moves (per row: 8 x arity + 1 read -- the key, the
      aggregates, the two window columns and the null_mask byte -- and 8 x (arity + 1) written) and
      the rate that implies, against the 6.29 TB/s a float4 copy streams on this GPU
  (b) wall time of fg_advance_progress(FG_DEVICE) + fg_fired_packed(FG_HOST, key field) against
      fg_advance_progress(FG_HOST) -- the columnar collect -- of the same fire, the two alternating
      in one loop; median, min and max of --reps repetitions each, and the bytes each copies out

--runs puts both handles in run mode (fg_set_fired_runs): the columnar copy then carries no window
columns, the packed rows still do.

    python scripts/fired_packed_time.py [--records 100000000] [--reps 7] [--runs]
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
STREAM_TBS = 6.29   # measured float4 copy rate of the GPU


def handle(keys, n, runs, timing=False):
    return F.WindowAggOperator(F.tumbling(1000), aggs=AGGS, val_type="f64", expected_keys=int(keys * 1.05) + 1,
                               buffer_records=max(4 * n, 1 << 26), kernel_timing=timing, fired_runs=runs)


def stage(op, cols):
    op.reset()
    op.process_batch(*cols)
    op.synchronize()


def fire_columnar(op, cols):
    """(seconds in fg_advance_progress(FG_HOST), rows)"""
    stage(op, cols)
    r = FL.FgRows()
    t0 = time.perf_counter()
    FL.check(op._lib.fg_advance_progress(op._h, JMAX, FL.HOST, C.byref(r)), op._h)
    return time.perf_counter() - t0, int(r.n)


def fire_packed(op, cols):
    """(seconds in fg_advance_progress(FG_DEVICE) + fg_fired_packed(FG_HOST), seconds of the pack alone, rows)"""
    stage(op, cols)
    r, p = FL.FgRows(), FL.FgPackedRows()
    t0 = time.perf_counter()
    FL.check(op._lib.fg_advance_progress(op._h, JMAX, FL.DEVICE, C.byref(r)), op._h)
    t1 = time.perf_counter()
    FL.check(op._lib.fg_fired_packed(op._h, 0, int(r.n), FL.PACK_KEY_FIELD, FL.HOST, C.byref(p)), op._h)
    t2 = time.perf_counter()
    assert p.n == r.n and p.stride == 8 * (len(AGGS) + 4)
    return t2 - t0, t2 - t1, int(p.n)


def spread(ts, unit=1e3):
    return (f"median {unit * statistics.median(ts):.3f}  min {unit * min(ts):.3f}  max {unit * max(ts):.3f}   "
            f"reps {' '.join(f'{unit * t:.3f}' for t in ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000, help="records of the one window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", action="store_true", help="run mode (fg_set_fired_runs)")
    a = ap.parse_args()
    wl = bench.WORKLOADS["tumble"]
    dev = torch.device("cuda", 0)
    n = min(a.records, wl["rate"])   # (one event-second: one window)
    cols = bench.gen_columns(n, wl["keys"], wl["rate"], 0, dev)
    torch.cuda.synchronize()
    arity = len(AGGS) + 3
    col_bytes = 8 * ((1 if a.runs else 3) + len(AGGS)) + 1
    row_bytes = 8 * (arity + 1)

    # (a) the kernel
    op = handle(wl["keys"], n, a.runs, timing=True)
    fire_packed(op, cols)   # warm-up: allocations, region growth, the pinned rows; lists the class
    op.set_kernel_timing(["pack_rows"])
    ms = []
    for _ in range(a.reps):
        b = op.kernel_stats()["pack_rows"]
        _, _, rows = fire_packed(op, cols)
        k = op.kernel_stats()["pack_rows"]
        ms.append(k["total_ms"] - b["total_ms"])
        assert k["launches"] - b["launches"] == 1 and k["rows"] - b["rows"] == rows == k["records"] - b["records"]
    op.close()
    read = 8 * (arity - (2 if a.runs else 0)) + 1
    moved = rows * (read + row_bytes)
    med = statistics.median(ms)
    print(f"== {n:,} records, {wl['keys']:,} keys, one window: {rows:,} rows packed, arity {arity}, stride {row_bytes} B"
          f"{' (run mode)' if a.runs else ''}")
    print(f"(a) pack_rows kernel per call, ms: {spread(ms, 1.0)}")
    print(f"    {moved:,} B moved ({read} B read + {row_bytes} B written per row): {moved / (med * 1e-3) / 1e12:.2f} TB/s, "
          f"{100 * moved / (med * 1e-3) / 1e12 / STREAM_TBS:.0f} % of the {STREAM_TBS} TB/s copy rate; "
          f"{1e6 * med / rows:.3f} ns per row")

    # (b) the two ways out, alternating
    pk, cl = handle(wl["keys"], n, a.runs), handle(wl["keys"], n, a.runs)
    fire_packed(pk, cols)
    fire_columnar(cl, cols)
    tp, tpack, tc = [], [], []
    for _ in range(a.reps):
        dt, dpack, rp = fire_packed(pk, cols)
        tp.append(dt)
        tpack.append(dpack)
        dt, rc = fire_columnar(cl, cols)
        tc.append(dt)
        assert rp == rc == rows
    pk.close()
    cl.close()
    print(f"(b) fg_advance_progress(FG_DEVICE) + fg_fired_packed(FG_HOST), ms: {spread(tp)}   ({rows * row_bytes:,} B copied)")
    print(f"      of which fg_fired_packed(FG_HOST), ms:                      {spread(tpack)}")
    print(f"    fg_advance_progress(FG_HOST) columns, ms:                      {spread(tc)}   ({rows * col_bytes:,} B copied)")
    print(f"    packed / columnar (medians): {statistics.median(tp) / statistics.median(tc):.3f}")


if __name__ == "__main__":
    main()
