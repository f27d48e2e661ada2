#!/usr/bin/env python
"""Times one round of the two-phase edge through the C-ABI at world size 1 (fg_comm_round_begin +
_exchange + _end, host clock around a final device synchronise) for 1M partial rows, with

  (bigint) BIGINT keys: the ids move as they are (FG_KEYHASH_BINARYROW_BIGINT, no dictionaries)
  (keyed)  dictionary keys: every row ships its 32-B key row (bench.string_key_rows), the owner
           interns it (fg_comm_set_key_dicts, FG_KEYHASH_DICT_ID); both dictionaries already
           know every key, so the intern is lookups only -- the steady state of a job

Each round flushes the local operator's buffer of one slice (FG_ROUND_FLUSHED: 1M records of 1M
distinct keys, refilled outside the timed region) and merges it into the global operator, whose
state stays at 1M entries. The variants alternate in one process; the first rounds of each are
the warm-up. Then a few keyed rounds with the dictionaries' kernel timing on
(fg_key_dict_kernel_stats). The baseline a ship-once change would be judged against (DESIGN.md
section 7).

    python scripts/keyed_round_time.py [--rows 1000000] [--reps 9]
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
from flink_amd import _lib as L   # noqa: E402
from flink_amd.comm import Communicator, unique_id   # noqa: E402
from flink_amd.two_phase import FLUSHED, CapiRounds, GpuPair   # noqa: E402

MAXP = 128
T0 = 1_600_000_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    n = a.rows
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    comm = Communicator(0, 1, 0, unique_id())
    keys = torch.arange(n, dtype=torch.int64, device=dev)
    rows = bench.string_key_rows(keys)
    packed = (rows.view(torch.uint8).reshape(-1), torch.arange(n, dtype=torch.int64, device=dev) * 32,
              torch.full((n,), 32, dtype=torch.int32, device=dev))
    kd, ko = F.KeyDictionary(MAXP, n), F.KeyDictionary(MAXP, n)
    ids = kd.intern_rows(*packed)
    ko.intern_rows(rows.flip(0).contiguous().view(torch.uint8).reshape(-1), packed[1], packed[2])   # another order
    ts = torch.full((n,), T0, dtype=torch.int64, device=dev)
    val = torch.rand(n, dtype=torch.float64, device=dev)
    aggs = ("count_star", "count", "sum", "avg")

    def pair(dicts):
        local = F.WindowAggOperator(F.tumbling(1000), aggs=aggs, expected_keys=n, local_partials=True)
        glob = F.WindowAggOperator(F.tumbling(1000), aggs=aggs, expected_keys=n)
        return GpuPair(local, glob, dev, key_dicts=dicts)

    variants = {"bigint": (pair(None), CapiRounds(comm, MAXP, L.KEYHASH_BINARYROW_BIGINT), keys, None),
                "keyed": (pair((kd, ko)), CapiRounds(comm, MAXP, L.KEYHASH_DICT_ID), ids, (kd, ko))}

    def one_round(name):
        p, rounds, key, dicts = variants[name]
        comm.set_key_dicts(*(dicts or (None, None)))
        p.local.process_batch(key, ts, val)
        p.local.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rounds.begin(p, FLUSHED, T0, 0)
        r = rounds.exchange()
        rounds.end(p, dev)
        p.glob.synchronize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert r.rows_sent == r.rows_received == n, (r.rows_sent, r.rows_received)
        return dt

    times = {"bigint": [], "keyed": []}
    for rep in range(a.reps + 2):   # the first two of each are the warm-up; the variants alternate
        for name in ("bigint", "keyed"):
            dt = one_round(name)
            if rep >= 2:
                times[name].append(dt)
    print(f"{n} partial rows, 32-B key rows, world size 1 on {torch.cuda.get_device_name(0)}, {a.reps} rounds each")
    print("| keys | min ms | median ms | max ms |")
    print("|---|---|---|---|")
    for name, t in times.items():
        print(f"| {name} | {1e3 * min(t):.2f} | {1e3 * statistics.median(t):.2f} | {1e3 * max(t):.2f} |")
    print(f"median keyed / bigint = {statistics.median(times['keyed']) / statistics.median(times['bigint']):.2f}; "
          f"key bytes per round {32 * n}, lengths {4 * n}, columns {8 * 5 * n}")
    for d in (kd, ko):
        d.set_timing(True)
    for _ in range(3):
        one_round("keyed")
    for name, d in (("local", kd), ("owner", ko)):
        for k, s in d.kernel_stats().items():
            if s["launches"]:
                print(f"kernel_stats {name} {k}: launches {s['launches']} total_ms {s['total_ms']:.3f} "
                      f"records {s['records']}")
    assert len(kd) == len(ko) == n
    comm.set_key_dicts(None, None)
    for p, _, _, _ in variants.values():
        p.local.close()
        p.glob.close()
    kd.close()
    ko.close()
    comm.close()


if __name__ == "__main__":
    main()
