#!/usr/bin/env python
"""Times the key-grouped snapshot of a 2-slice x 5M-key image (f64 TUMBLE state, the image of
restore_range_time.py) and the rescale restore that reads only its own key groups:

  1. snapshot_state plain vs grouped (set_snapshot_grouping) on the same handle state, and what a
     shim would pay for the same order on the host: np.argsort((slice, key group), stable) + a
     gather of the plain image's columns (the key groups given)
  2. restore to the range (0, 63): restore_state_range of the whole plain image against
     two_phase.restore_keyed of the grouped image, both host-resident
  3. the export / export_group lines of kernel_stats

Every repetition runs on a fresh handle (opened, restored and warmed by one untimed snapshot
outside the timed span); times are taken around synchronize; medians of --reps repetitions.

    python scripts/snapshot_grouped_time.py [--keys 5000000] [--slices 2] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flink_amd as F   # noqa: E402
from flink_amd import _lib as L, two_phase   # noqa: E402
from scripts.restore_range_time import MAXP, RANGE, TWM, image   # noqa: E402


def handle(keys, rng=(0, MAXP - 1), timing=False):
    return F.WindowAggOperator(F.tumbling(1000), val_type="f64", expected_keys=keys, max_parallelism=MAXP,
                               key_group_range=rng, kernel_timing=timing)


def med(ts, what):
    print(f"  {what}: repetitions (ms) {' '.join(f'{1e3 * t:.1f}' for t in ts)}")
    return statistics.median(ts)


def snapshot_times(img, keys, reps):
    plain, grouped = [], []
    for r in range(reps):
        for out, hash_ in ((plain, None), (grouped, L.KEYHASH_BINARYROW_BIGINT)):   # alternating
            op = handle(keys)
            op.restore_state(img, TWM)
            op.set_snapshot_grouping(hash_)
            op.snapshot_state(copy=False)   # warm-up: the image buffers are allocated here
            op.synchronize()
            t0 = time.perf_counter()
            op.snapshot_state(copy=False)
            op.synchronize()
            out.append(time.perf_counter() - t0)
            op.close()
    return med(plain, "plain"), med(grouped, "grouped")


def host_sort_time(plain, slices, kg, reps):
    ts = []
    sidx = np.repeat(np.arange(len(slices["rows"]), dtype=np.int64), slices["rows"])
    for _ in range(reps):
        t0 = time.perf_counter()
        order = np.argsort(sidx * MAXP + kg, kind="stable")
        cols = {c: v[order] for c, v in plain.items()}
        ts.append(time.perf_counter() - t0)
    del cols
    return med(ts, "host argsort + gather")


def restore_times(plain, grouped, index, keys, reps):
    whole, keyed, info_w, info_k = [], [], None, None
    for r in range(reps + 1):   # the first is the warm-up
        for out, fn in ((whole, lambda op: op.restore_state_range([(plain, TWM)])),
                        (keyed, lambda op: two_phase.restore_keyed(op, [(grouped, TWM, index)]))):
            op = handle(keys, RANGE)
            t0 = time.perf_counter()
            info = fn(op)
            op.synchronize()
            dt = time.perf_counter() - t0
            op.close()
            if r:
                out.append(dt)
            if out is whole:
                info_w = info
            else:
                info_k = info
    return med(whole, "restore_state_range, whole image"), med(keyed, "restore_keyed, grouped image"), info_w, info_k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=5_000_000)
    ap.add_argument("--slices", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    img = image(a.keys, a.slices)
    ncols = len(img)

    t_p, t_g = snapshot_times(img, a.keys, a.reps)
    op = handle(a.keys, timing=True)
    op.restore_state(img, TWM)
    plain, _ = op.snapshot_state()
    slices = op.snapshot_slices()
    op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
    op.snapshot_state(copy=False)
    grouped, _ = op.snapshot_state()
    index = op.snapshot_key_groups()
    stats = op.kernel_stats()
    op.close()
    t_s = host_sort_time(plain, slices, F.key_groups(plain["key"], MAXP).astype(np.int64), a.reps)
    n = len(plain["key"])
    print(f"image: {n} rows in {len(slices['rows'])} slices, {ncols} columns ({8 * ncols * n / 1e6:.0f} MB)")
    print(f"1. snapshot_state plain                    median {t_p * 1e3:9.1f} ms")
    print(f"   snapshot_state grouped                  median {t_g * 1e3:9.1f} ms   grouped/plain = {t_g / t_p:.2f}")
    print(f"   host argsort(stable) + gather           median {t_s * 1e3:9.1f} ms")
    for name in ("export", "export_group"):
        s = stats[name]
        print(f"   kernel_stats {name}: launches {s['launches']} total_ms {s['total_ms']:.3f} records {s['records']}")

    t_w, t_k, info_w, info_k = restore_times(plain, grouped, index, a.keys, a.reps)
    assert info_k["rows_in"] == info_k["rows_kept"] == info_w["rows_kept"], (info_w, info_k)
    for what, t, info in (("restore_state_range, whole plain image", t_w, info_w),
                          ("restore_keyed, grouped image          ", t_k, info_k)):
        print(f"2. {what}  median {t * 1e3:9.1f} ms   rows_in {info['rows_in']} rows_kept {info['rows_kept']} "
              f"uploaded {8 * ncols * info['rows_in'] / 1e6:.0f} MB")


if __name__ == "__main__":
    main()
