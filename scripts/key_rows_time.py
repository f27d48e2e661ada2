#!/usr/bin/env python
"""Times the way out of the key dictionary -- ids back to key rows on the host -- for a dictionary
of 4M distinct 32-B rows (bench.string_key_rows) and fired batches of 10k and 1M random ids:

  (old) fg_key_dict_lookup + fg_key_dict_copy_arena of the arena range the ids span
  (new) fg_key_dict_rows to the host (one call into a buffer of the exact size)

Both run in the same build, alternating, into pageable host arrays allocated once per batch size
(the warm-up of each path touches their pages); min / median / max of the repetitions and the
bytes each path copies device -> host. The new path's bytes must be
nbytes + 12 n + 8 (the packed rows, n + 1 offsets, n lengths) plus the 24 B of the call's one
counter read; that is asserted, and so is that both paths return the same rows.

    python scripts/key_rows_time.py [--keys 4000000] [--reps 7]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

import bench   # noqa: E402
import flink_amd as F   # noqa: E402
from flink_amd import _lib as L   # noqa: E402

COUNTER_READ = 24   # {total bytes, bad ids, lowest bad index}: the one host read of fg_key_dict_rows


def old_path(d, ids, arena, off, ln):
    """what KeyDictionary.lookup and GpuKeyRows.rows did: (arena range, its first byte, D2H bytes)"""
    n = len(ids)
    d._check(d._lib.fg_key_dict_lookup(d._h, L.HOST, n, ids.ctypes.data, off.ctypes.data, ln.ctypes.data))
    lo, hi = int(off.min()), int((off + ln).max())
    d._check(d._lib.fg_key_dict_copy_arena(d._h, lo, hi - lo, arena.ctypes.data))
    return arena[:hi - lo], lo, 12 * n + (hi - lo)


def new_path(d, ids, nbytes, buf, off, ln):
    n = len(ids)
    got = C.c_int64()
    d._check(d._lib.fg_key_dict_rows(d._h, L.HOST, n, ids.ctypes.data, buf.ctypes.data, nbytes, off.ctypes.data,
                                     ln.ctypes.data, C.byref(got)))
    return int(got.value) + 12 * n + 8 + COUNTER_READ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = bench.string_key_rows(torch.arange(a.keys, dtype=torch.int64, device=dev))
    packed = (rows.view(torch.uint8).reshape(-1), torch.arange(a.keys, dtype=torch.int64, device=dev) * 32,
              torch.full((a.keys,), 32, dtype=torch.int32, device=dev))
    d = F.KeyDictionary(max_parallelism=128, expected_keys=a.keys)
    all_ids, _ = d.intern(packed=packed, key_groups=False)
    all_ids = all_ids.cpu().numpy()
    assert len(d) == a.keys
    print(f"dictionary: {a.keys} rows of 32 B on {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(1)
    print("| ids | path | D2H bytes | min ms | median ms | max ms |")
    print("|---|---|---|---|---|---|")
    for n in (10_000, 1_000_000):
        ids = np.ascontiguousarray(all_ids[rng.integers(0, a.keys, n)])
        nbytes = 32 * n
        arena_buf = np.empty(40 * a.keys, dtype=np.uint8)   # (an arena entry: the id and the 32-B row)
        off_o, ln_o = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32)
        buf, off_n, ln_n = np.empty(nbytes, dtype=np.uint8), np.empty(n + 1, dtype=np.int64), np.empty(n, dtype=np.int32)
        t_old, t_new = [], []
        for r in range(a.reps + 1):   # the first of each is the warm-up; the paths alternate
            t0 = time.perf_counter()
            arena, lo, b_old = old_path(d, ids, arena_buf, off_o, ln_o)
            t1 = time.perf_counter()
            b_new = new_path(d, ids, nbytes, buf, off_n, ln_n)
            t2 = time.perf_counter()
            if r:
                t_old.append(t1 - t0)
                t_new.append(t2 - t1)
        # both paths return the same rows; the new path's bytes are the derived volume
        assert int(off_n[-1]) == nbytes and np.array_equal(ln_o, ln_n[:n])
        old_rows = arena[(off_o - lo)[:, None] + np.arange(32)]
        assert np.array_equal(old_rows.reshape(-1), buf)
        assert b_new == nbytes + 12 * n + 8 + COUNTER_READ
        for name, b, t in (("lookup + copy_arena", b_old, t_old), ("fg_key_dict_rows", b_new, t_new)):
            print(f"| {n} | {name} | {b} | {1e3 * min(t):.2f} | {1e3 * statistics.median(t):.2f} | {1e3 * max(t):.2f} |")
        print(f"  ({n} ids: bytes old / new = {b_old / b_new:.1f}, median old / new = "
              f"{statistics.median(t_old) / statistics.median(t_new):.1f})")
    d.set_timing(True)
    new_path(d, ids, nbytes, buf, off_n, ln_n)
    s = d.kernel_stats()["dict_rows"]
    print(f"kernel_stats dict_rows: launches {s['launches']} total_ms {s['total_ms']:.3f} records {s['records']}")
    d.close()


if __name__ == "__main__":
    main()
