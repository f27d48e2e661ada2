#!/usr/bin/env python
"""Times a rescale restore of a 2-slice x 5M-key image (f64 TUMBLE state) for the range (0, 63):

  (a) the host path: union_image_for (key groups, numpy concatenate + mask) + restore_state
  (b) restore_state_range, the image in pageable host memory and then on the device

Three timed repetitions of each side after a warm-up, every one into a fresh handle (opened
outside the timed span). Prints the medians, the row counts and the kernel_stats lines of the
restore kernels.

    python scripts/restore_range_time.py [--keys 5000000] [--slices 2]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flink_amd as F   # noqa: E402
from flink_amd import two_phase   # noqa: E402

RANGE, MAXP, TWM = (0, 63), 128, 1_600_000_000_000


def image(keys, slices):
    k = np.tile(np.arange(keys, dtype=np.int64), slices)
    i = np.arange(len(k), dtype=np.int64)
    return dict(key=k, slice_end=np.repeat(TWM + 1000 * (1 + np.arange(slices, dtype=np.int64)), keys),
                cnt_star=i % 7 + 1, cnt_val=i % 7 + 1, sum=(i * 0.25).view(np.int64))


def handle(keys, timing=False):
    return F.WindowAggOperator(F.tumbling(1000), val_type="f64", expected_keys=keys, max_parallelism=MAXP,
                               key_group_range=RANGE, kernel_timing=timing)


def timed(keys, fn, reps=3):
    out, res = [], None
    for r in range(reps + 1):   # the first is the warm-up
        op = handle(keys)
        t0 = time.perf_counter()
        res = fn(op)
        op.synchronize()
        dt = time.perf_counter() - t0
        op.close()
        if r:
            out.append(dt)
    print(f"  repetitions (ms): {' '.join(f'{1e3 * t:.1f}' for t in out)}")
    return statistics.median(out), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=5_000_000)
    ap.add_argument("--slices", type=int, default=2)
    a = ap.parse_args()
    img = image(a.keys, a.slices)

    def host_path(op):
        filt, wm = two_phase.union_image_for([(img, TWM)], RANGE, MAXP)
        op.restore_state(filt, wm)
        return len(filt["key"])

    t_a, kept_a = timed(a.keys, host_path)
    t_h, info = timed(a.keys, lambda op: op.restore_state_range([(img, TWM)]))
    import torch
    dev = {c: torch.from_numpy(v).cuda() for c, v in img.items()}
    torch.cuda.synchronize()
    t_d, info_d = timed(a.keys, lambda op: op.restore_state_range([(dev, TWM)]))
    assert info["rows_kept"] == info_d["rows_kept"] == kept_a, (info, info_d, kept_a)
    print(f"rows_in {info['rows_in']} rows_kept {info['rows_kept']} slices {info['slices']} "
          f"state_regions {info['state_regions']}")
    print(f"(a) union_image_for + restore_state      median {t_a * 1e3:9.1f} ms")
    print(f"(b) restore_state_range, host image      median {t_h * 1e3:9.1f} ms   (a)/(b) = {t_a / t_h:.1f}")
    print(f"(b) restore_state_range, device image    median {t_d * 1e3:9.1f} ms   (a)/(b) = {t_a / t_d:.1f}")
    op = handle(a.keys, timing=True)
    op.restore_state_range([(dev, TWM)])
    for name, s in op.kernel_stats().items():
        if name.startswith("restore"):
            print(f"kernel_stats {name}: launches {s['launches']} total_ms {s['total_ms']:.3f} records {s['records']}")
    op.close()


if __name__ == "__main__":
    main()
