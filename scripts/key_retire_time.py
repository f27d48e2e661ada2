#!/usr/bin/env python
"""Times fg_key_dict_retain on a dictionary of 4M distinct 32-B rows (bench.string_key_rows):

  retain a random 1M, 2M and all 4M of the ids; the retired rows are re-interned between the
  repetitions, so every repetition starts from 4M live keys. One warm-up, then --reps repetitions:
  min / median / max of the call's wall time, the "dict_retain" kernel class (all the call's
  kernels) and, beside it, the "dict_rebuild" class: the one table rebuild (clear + rehash) inside
  the call, at the same capacity. The multiple retain / rebuild is reported, not asserted.

  Then --rounds churn rounds of 1M carried + 1M fresh keys, each retaining exactly its own ids:
  the stats per round. Memory must be flat from round 2 on (asserted: arena_bytes and table_slots
  constant, issued not above 3M = the peak alive after an intern).

    python scripts/key_retire_time.py [--keys 4000000] [--reps 7] [--rounds 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

import bench   # noqa: E402
import flink_amd as F   # noqa: E402


def packed_rows(lo, hi, dev):
    """the device key rows of keys lo .. hi - 1, as intern takes them"""
    n = hi - lo
    rows = bench.string_key_rows(torch.arange(lo, hi, dtype=torch.int64, device=dev))
    return (rows.view(torch.uint8).reshape(-1), torch.arange(n, dtype=torch.int64, device=dev) * 32,
            torch.full((n,), 32, dtype=torch.int32, device=dev))


def delta(after, before, name):
    a, b = after[name], before.get(name, dict(launches=0, total_ms=0.0))
    return a["launches"] - b["launches"], a["total_ms"] - b["total_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    packed = packed_rows(0, a.keys, dev)
    d = F.KeyDictionary(max_parallelism=128, expected_keys=a.keys)
    d.set_timing(True)
    ids, _ = d.intern(packed=packed, key_groups=False)
    assert len(d) == a.keys
    print(f"dictionary: {a.keys} rows of 32 B on {torch.cuda.get_device_name(0)}; {d.stats()}")
    rng = np.random.default_rng(1)
    print("| kept | wall ms min / median / max | dict_retain kernels ms (median) | dict_rebuild ms (median) | retain / rebuild |")
    print("|---|---|---|---|---|")
    for kept in (a.keys // 4, a.keys // 2, a.keys):
        wall, kern, reb = [], [], []
        for r in range(a.reps + 1):   # the first is the warm-up
            keep = torch.from_numpy(rng.permutation(a.keys)[:kept]).to(dev)
            keep_ids = ids[keep]
            torch.cuda.synchronize()
            before = d.kernel_stats()
            t0 = time.perf_counter()
            st = d.retain(keep_ids)
            t1 = time.perf_counter()
            after = d.kernel_stats()
            assert st["live"] == kept and st["arena_bytes"] == 40 * kept and st["free_ordinals"] == a.keys - kept
            (ln, kms), (lb, rms) = delta(after, before, "dict_retain"), delta(after, before, "dict_rebuild")
            assert ln == 1 and lb == 1
            if r:
                wall.append(1e3 * (t1 - t0))
                kern.append(kms)
                reb.append(rms)
            ids, _ = d.intern(packed=packed, key_groups=False)   # the retired rows come back on the free ordinals
            st = d.stats()
            assert st["live"] == a.keys and st["issued"] == a.keys and st["free_ordinals"] == 0
        k, b = statistics.median(kern), statistics.median(reb)
        print(f"| {kept} | {min(wall):.2f} / {statistics.median(wall):.2f} / {max(wall):.2f} | {k:.3f} | {b:.3f} | {k / b:.1f} |")
    # churn: every round 1M carried + 1M fresh keys, then exactly those retained
    d.close()
    m = a.keys // 4
    d = F.KeyDictionary(max_parallelism=128, expected_keys=2 * m)   # (a fresh one: `issued` never shrinks)
    print(f"churn: {a.rounds} rounds of {m} carried + {m} fresh keys")
    print("| round | live | issued | free_ordinals | arena_bytes | table_slots | retired_total | retain wall ms |")
    print("|---|---|---|---|---|---|---|---|")
    flat = None
    for rnd in range(a.rounds):
        ids, _ = d.intern(packed=packed_rows(rnd * m, (rnd + 2) * m, dev), key_groups=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = d.retain(ids)
        t1 = time.perf_counter()
        print(f"| {rnd + 1} | {st['live']} | {st['issued']} | {st['free_ordinals']} | {st['arena_bytes']} | "
              f"{st['table_slots']} | {st['retired_total']} | {1e3 * (t1 - t0):.2f} |")
        assert st["live"] == 2 * m and st["arena_bytes"] == 40 * 2 * m
        if rnd >= 1:
            now = (st["arena_bytes"], st["table_slots"], st["issued"])
            assert flat is None or now == flat, (rnd, now, flat)
            flat = now
            assert st["issued"] <= 3 * m
    d.close()


if __name__ == "__main__":
    main()
