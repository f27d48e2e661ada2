#!/usr/bin/env python
"""Times a checkpoint of a HOP 5 min / 1 min shaped state one micro-batch after the previous one:
the full image (snapshot_state: every resident slice exported and copied) against the selective one
(snapshot_plan -> keyed_state.wanted_slices -> snapshot_state_select: only the slices whose keyed
state the shim rewrites).

The state: --slices resident slices of --keys keys each (an image restored into a fresh handle, then
a first barrier that leaves every slice unchanged), then one micro-batch of --batch records into the
newest slice, then the timed barrier. Wall time from the call to the returned host image (copy=False),
medians of --reps repetitions, each on a fresh handle; the two paths alternate.

  1. rows and wall time of snapshot_state
  2. rows and wall time of snapshot_plan + wanted_slices + snapshot_state_select
  3. the export / export_select lines of kernel_stats for one barrier of each kind

    python scripts/snapshot_select_time.py [--keys 2000000] [--slices 5] [--batch 200000] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flink_amd as F   # noqa: E402
from flink_amd.keyed_state import HOP, SliceSpec, WindowAggsState   # noqa: E402

SIZE, SLIDE = 300_000, 60_000
T0 = 1_600_000_020_000   # a multiple of the slide


def image(keys, slices):
    """`slices` slices of `keys` keys each, ending T0 + SLIDE, T0 + 2 SLIDE, ..."""
    n = keys * slices
    i = np.arange(n, dtype=np.int64)
    return dict(key=i % keys, slice_end=T0 + SLIDE * (1 + i // keys), cnt_star=i % 5 + 1, cnt_val=i % 5 + 1, sum=i * 3 + 1)


def micro_batch(keys, slices, n, seed):
    rs = np.random.default_rng(seed)
    ts = T0 + SLIDE * (slices - 1) + np.sort(rs.integers(0, SLIDE, n))
    return rs.integers(0, keys, n).astype(np.int64), ts.astype(np.int64), rs.integers(0, 1000, n).astype(np.int64)


def handle(keys, timing=False):
    return F.WindowAggOperator(F.hopping(SIZE, SLIDE), val_type="i64", expected_keys=keys, kernel_timing=timing)


def full_barrier(op, backend):
    img, wm = op.snapshot_state(copy=False)
    return len(img["key"])


def select_barrier(op, backend):
    plan, wm = op.snapshot_plan()
    img, _ = op.snapshot_state_select(backend.wanted_slices(plan, wm), copy=False)
    return len(img["key"])


def prepared(img, a, barrier, timing=False):
    """a handle one micro-batch after its previous barrier (which allocated the image buffers)"""
    op = handle(a.keys, timing)
    op.restore_state(img, T0 - 1)
    backend = WindowAggsState(SliceSpec(HOP, SIZE, SLIDE), f64=False)
    op.snapshot_state(copy=False)   # sizes the image buffers for either path
    barrier(op, backend)            # the previous barrier
    op.process_batch(*micro_batch(a.keys, a.slices, a.batch, 7))
    op.prepare_snapshot_pre_barrier()
    op.synchronize()
    return op, backend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_000_000)
    ap.add_argument("--slices", type=int, default=5)
    ap.add_argument("--batch", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    img = image(a.keys, a.slices)
    times = {"full": [], "select": []}
    rows = {}
    for _ in range(a.reps):
        for name, barrier in (("full", full_barrier), ("select", select_barrier)):
            op, backend = prepared(img, a, barrier)
            t0 = time.perf_counter()
            rows[name] = barrier(op, backend)
            times[name].append(time.perf_counter() - t0)
            op.close()
    stats = {}
    for name, barrier in (("full", full_barrier), ("select", select_barrier)):
        op, backend = prepared(img, a, barrier, timing=True)
        op.synchronize()
        before = op.kernel_stats()
        barrier(op, backend)
        op.synchronize()
        after = op.kernel_stats()
        stats[name] = {k: {f: after[k][f] - before[k][f] for f in ("launches", "total_ms", "records")}
                       for k in ("export", "export_select")}
        op.close()
    print(f"state: {a.slices} slices x {a.keys} keys, micro-batch of {a.batch} records into the newest slice; "
          f"5 image columns (cnt_val aliases cnt_star: 4 copied), 32 B per row over PCIe")
    med = {}
    for name in ("full", "select"):
        med[name] = statistics.median(times[name])
        print(f"  {name}: repetitions (ms) {' '.join(f'{1e3 * t:.1f}' for t in times[name])}")
    print(f"1. snapshot_state                        rows {rows['full']:9d}  median {med['full'] * 1e3:8.1f} ms")
    print(f"2. snapshot_plan + snapshot_state_select rows {rows['select']:9d}  median {med['select'] * 1e3:8.1f} ms   "
          f"rows x {rows['select'] / rows['full']:.3f}  time x {med['select'] / med['full']:.3f}")
    for name in ("full", "select"):
        for k, s in stats[name].items():
            print(f"3. {name} barrier, kernel_stats {k}: launches {s['launches']} total_ms {s['total_ms']:.3f} "
                  f"records {s['records']}")


if __name__ == "__main__":
    main()
