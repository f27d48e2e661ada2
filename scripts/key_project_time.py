"""The key selector on the GPU, timed: fg_key_dict_project of 10M records of one
STRING key of 9..16 bytes (32-byte key rows, the shape of bench.py --workload strings) beside its
yardstick, fg_key_dict_rows gathering the same 10M key rows (ids in intern order and shuffled). Kernel
time from fg_key_dict_set_timing (classes dict_project / dict_rows): 2 warm-up calls, then 9
repetitions; median, min and max, the bytes read and written by the call's contract, the TB/s of
those bytes and the nanoseconds per key byte. N=<records> overrides the size. Prints one JSON object.

    python scripts/key_project_time.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flink_amd as F   # noqa: E402
from flink_amd import keys as K   # noqa: E402

N = int(os.environ.get("N", 10_000_000))
WARM, REPS = 2, 9
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(1)


def records(arity):
    """n rows of [STRING key, (BIGINT rowtime, DOUBLE value)]: bit set, slots, 16 bytes of string"""
    ln = torch.randint(9, 17, (N,), device=dev, generator=g, dtype=torch.int64)
    words = 1 + arity + 2
    r = torch.zeros((N, words), dtype=torch.int64, device=dev)
    r[:, 1] = ((8 * (1 + arity)) << 32) | ln
    for f in range(1, arity):
        r[:, 1 + f] = torch.randint(0, 1 << 40, (N,), device=dev, generator=g, dtype=torch.int64)
    r[:, 1 + arity] = torch.randint(1, 1 << 62, (N,), device=dev, generator=g, dtype=torch.int64)
    tail = torch.randint(1, 1 << 62, (N,), device=dev, generator=g, dtype=torch.int64)
    keep = (ln - 8) * 8
    r[:, 2 + arity] = torch.where(keep >= 64, tail, tail & ((torch.ones_like(ln) << keep.clamp(max=62)) - 1))
    buf = r.view(torch.uint8).reshape(-1)
    off = torch.arange(N, device=dev, dtype=torch.int64) * (8 * words)
    lens = torch.full((N,), 8 * words, dtype=torch.int32, device=dev)
    return buf, off, lens


def stat(d, name):
    s = d.kernel_stats().get(name)
    return (s["total_ms"], s["launches"]) if s else (0.0, 0)


def timed(d, name, fn):
    out = []
    for i in range(WARM + REPS):
        t0, l0 = stat(d, name)
        fn()
        t1, l1 = stat(d, name)
        assert l1 == l0 + 1, (name, l0, l1)
        if i >= WARM:
            out.append(t1 - t0)
    a = np.array(out)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), reps=REPS)


res = {"n": N}
d = F.KeyDictionary(max_parallelism=128, expected_keys=N)
d.set_timing(True)
for arity, cols in ((1, ()), (3, (1, 2))):
    p = records(arity)
    proj = K.RowProjection(arity, [0], ["string"], col_fields=cols)
    kb, ko, kl, _, _ = d.project(p, proj)
    assert kb.numel() == 32 * N and int(ko[-1]) == 32 * N
    if arity == 1:   # the key rows of these records are the records themselves but for the pad bytes: spot check
        assert torch.equal(kb.view(torch.int64).reshape(N, 4)[:1000, :3], p[0].view(torch.int64).reshape(N, 4)[:1000, :3])
    r = timed(d, "dict_project", lambda: d.project(p, proj))
    in_bytes = p[0].numel() + 12 * N
    out_bytes = 32 * N + 12 * N + 8 + (8 + 1) * N * len(cols)
    r.update(bytes_read=in_bytes, bytes_written=out_bytes,
             TBps=(in_bytes + out_bytes) / r["median_ms"] / 1e9, ns_per_key_byte=r["median_ms"] * 1e6 / (32 * N))
    res[f"dict_project_arity{arity}_cols{len(cols)}"] = r
    if arity == 1:
        ids, _ = d.intern(packed=(kb, ko[:-1], kl), key_groups=False)
        r = timed(d, "dict_rows", lambda: d.rows(ids))
        in_bytes = (8 + 4 + 8 + 32) * N    # ids, an entry's length and offset, its arena bytes
        out_bytes = 32 * N + 12 * N + 8
        r.update(bytes_read=in_bytes, bytes_written=out_bytes, TBps=(in_bytes + out_bytes) / r["median_ms"] / 1e9,
                 ns_per_key_byte=r["median_ms"] * 1e6 / (32 * N), distinct_keys=len(d))
        res["dict_rows"] = r
        shuffled = ids[torch.randperm(N, device=dev, generator=g)]
        r = timed(d, "dict_rows", lambda: d.rows(shuffled))
        r.update(bytes_read=in_bytes, bytes_written=out_bytes, TBps=(in_bytes + out_bytes) / r["median_ms"] / 1e9,
                 ns_per_key_byte=r["median_ms"] * 1e6 / (32 * N))
        res["dict_rows_shuffled_ids"] = r
        del ids, shuffled
    del p, kb, ko, kl
d.close()
print(json.dumps(res, indent=1))
