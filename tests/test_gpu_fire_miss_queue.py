"""The plain tile fire's insert (k_tile_fire, insert_plain): a record whose key is in its home
bucket is settled in line, the others wait in a wave-private queue that is drained 64 at a time
and once more before the barrier that ends the item's inserts. Every case is TUMBLE, f64,
COUNT(*) / SUM / AVG, no lateness, 32-bit keys -- the tile path -- and compared row by row, late
drops included, with the oracle.

The keys are built from the two hashes the kernels use: a key's consumer bucket is
(fmix64(key) >> (64 - region_bits)) >> 2 -- one fire workgroup's LDS table -- and its home bucket
of four slots in that table umulhi(uint32(key) * 0x9E3779B1, 2048). A pass whose tile holds more
than 96 records of one consumer bucket takes the split fire instead (another insert), so the
streams that aim at one bucket are diluted by records of other buckets: fewer than 96 aimed
records in any 6,144 consecutive ones."""
import functools

import numpy as np
import pytest

from tests.test_gpu_parity import JMAX, assert_rows_equal, cfg_of, gpu_mk, oracle_mk

pytestmark = pytest.mark.gpu

AGGS = ("count_star", "sum", "avg")
CHK = dict(minmax=(), vmax=None, sums=True, sum0=False, aggs=AGGS)
BITS = 10            # TUMBLE operators from 4,096 expected keys: 2^10 regions, 256 consumer buckets
HOMES = 2048         # home buckets of the 8,192-slot table
TILE = 6144          # records of a pass-1 tile
SKEW = 96            # records of one bucket in a tile above which the pass counts as skewed
EMPTY32 = -(1 << 31)


def fmix64(k):
    h = np.asarray(k, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


def bucket_of(k, bits=BITS):
    return ((fmix64(k) >> np.uint64(64 - bits)) >> np.uint64(2)).astype(np.int64)


def home_of(k):
    h32 = (np.asarray(k, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)) * np.uint64(0x9E3779B1)
    h32 &= np.uint64(0xFFFFFFFF)
    return ((h32 * np.uint64(HOMES)) >> np.uint64(32)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def key_cells(span=1 << 22):
    """the keys of [0, span), their consumer and home buckets, and the keys per (consumer, home)"""
    k = np.arange(span, dtype=np.int64)
    b, h = bucket_of(k), home_of(k)
    return k, b, h, np.bincount(b * HOMES + h, minlength=(1 << (BITS - 2)) * HOMES).reshape(-1, HOMES)


def colliding_keys(n_first, n_next):
    """n_first keys of a small range with one consumer bucket and one home bucket, and n_next more
    of that consumer bucket whose home is the next home bucket."""
    k, b, h, cnt = key_cells()
    ok = (cnt[:, :-1] >= n_first) & (cnt[:, 1:] >= n_next)
    assert ok.any(), "no such cell in the key range"
    bb, hh = np.argwhere(ok)[0]
    first = k[(b == bb) & (h == hh)][:n_first]
    nxt = k[(b == bb) & (h == hh + 1)][:n_next]
    return first, nxt, int(bb), int(hh)


def diluted(aimed, bucket, every, rng, filler_keys=50_000):
    """`aimed` (keys of consumer bucket `bucket`) at every `every`-th position of a stream whose
    other records have keys of other buckets."""
    fill = np.arange(1 << 20, (1 << 20) + 2 * filler_keys, dtype=np.int64)
    fill = fill[bucket_of(fill) != bucket][:filler_keys]
    n = len(aimed) * every
    key = fill[rng.integers(0, len(fill), n)]
    key[::every] = aimed
    # the property the dilution is for: no tile-sized range holds a skewed bucket
    c = np.concatenate(([0], np.cumsum(bucket_of(key) == bucket)))
    assert (c[TILE:] - c[:-TILE]).max() < SKEW
    return key


def drive(O, batches, expected_keys=4096, size=1000, buffer_records=1 << 21):
    """batches: (key, ts, val, watermark or None). Rows and late drops compared after every
    watermark and at the end; returns the operator's kernel and state statistics."""
    cfg = dict(cfg_of("tumble", size), aggs=AGGS)
    g = gpu_mk(cfg, expected_keys=expected_keys, buffer_records=buffer_records, kernel_timing=True)
    o = oracle_mk(O, cfg)
    st0 = g.op.stats()
    for i, (key, ts, val, wm) in enumerate(batches):
        g.process_batch(key, ts, val)
        o.process_batch(key, ts, val)
        if wm is not None:
            g.process_watermark(wm)
            o.process_watermark(wm)
            assert_rows_equal(g.take_rows(), o.take_rows(), "f64", f"batch {i} wm {wm}", **CHK)
            assert g.late_dropped == o.late_dropped, f"late drops differ at batch {i}"
    g.process_watermark(JMAX)
    o.process_watermark(JMAX)
    assert_rows_equal(g.take_rows(), o.take_rows(), "f64", "final", **CHK)
    assert g.late_dropped == o.late_dropped
    ks, st = g.op.kernel_stats(), g.op.stats()
    g.close()
    o.close()
    assert ks["tile_fire"]["launches"] > 0, ks
    return ks, st0, st


def one_window(key, rng, parts=1, w0=0):
    """the stream as `parts` batches of one 1-s window (fired by the final watermark)"""
    n = len(key)
    ts = (w0 + rng.integers(0, 1000, n)).astype(np.int64)
    val = rng.random(n) * 1000.0
    cut = np.linspace(0, n, parts + 1).astype(int)
    return [(key[a:b], ts[a:b], val[a:b], None) for a, b in zip(cut[:-1], cut[1:])]


def test_home_bucket_overflow_chain(oracle_mod):
    """12 keys of one consumer bucket in one home bucket of four slots and 8 more in the next:
    the probes walk on over five buckets, and a queued record finds the key another lane
    inserted while it waited. ~20k records over the 20 keys in one window."""
    first, nxt, b, h = colliding_keys(12, 8)
    aimed = np.concatenate((first, nxt))
    assert len(first) == 12 and len(nxt) == 8 and len(np.unique(aimed)) == 20
    assert (bucket_of(aimed) == b).all() and (home_of(first) == h).all() and (home_of(nxt) == h + 1).all()
    rng = np.random.default_rng(11)
    key = diluted(aimed[rng.integers(0, 20, 20_000)], b, 72, rng)
    ks, st0, st = drive(oracle_mod, one_window(key, rng, parts=3))
    assert st0["state_regions"] == 1 << BITS and st["state_regions"] == 1 << BITS, (st0, st)


def test_all_first_occurrences(oracle_mod):
    """~60k distinct keys, each exactly once, in one window: every record misses its home bucket's
    copy and is queued, the queues drain continuously."""
    rng = np.random.default_rng(12)
    key = rng.permutation(np.arange(1000, 61_000, dtype=np.int64))
    assert len(np.unique(key)) == len(key) == 60_000
    assert np.bincount(bucket_of(key)).max() * TILE // len(key) < SKEW
    ks, st0, st = drive(oracle_mod, one_window(key, rng), expected_keys=60_000)
    assert st0["state_regions"] == 1 << BITS, st0


def test_one_key_everywhere(oracle_mod):
    """Every record of a consumer bucket carries one key -- whole 256-record windows of it, the
    same key queued by many lanes of one step -- then the bucket's records alternate between two
    keys of one home bucket: one row per key, no duplicate."""
    first, _, b, h = colliding_keys(2, 0)
    ka, kb = int(first[0]), int(first[1])
    assert ka != kb and bucket_of([ka, kb]).tolist() == [b, b] and home_of([ka, kb]).tolist() == [h, h]
    rng = np.random.default_rng(13)
    aimed = np.full(20_000, ka, dtype=np.int64)
    aimed[10_001::2] = kb   # 10,000 records (39 windows of 256) of ka, then ka / kb alternating
    key = diluted(aimed, b, 72, rng)
    ks, st0, st = drive(oracle_mod, one_window(key, rng, parts=2))
    assert st0["state_regions"] == 1 << BITS, st0


def test_sentinel_key(oracle_mod):
    """records of key -2^31 (the table's empty marker, kept in a slot of its own) among ordinary
    keys, negative ones included"""
    rng = np.random.default_rng(14)
    n = 300_000
    key = rng.integers(-2500, 2500, n).astype(np.int64)
    key[::150] = EMPTY32
    key[75::150] = EMPTY32 + 1
    assert (key == EMPTY32).sum() == 2000
    c = np.concatenate(([0], np.cumsum(bucket_of(key) == bucket_of([EMPTY32])[0])))
    assert (c[TILE:] - c[:-TILE]).max() < SKEW
    batches = one_window(key[:200_000], rng, parts=2)
    batches[-1] = batches[-1][:3] + (999,)
    batches += one_window(key[200_000:], rng, w0=1000)
    drive(oracle_mod, batches)


@pytest.mark.parametrize("sizes", [(1,), (63,), (65,), (6145,), (1, 63, 65, 6145)], ids=lambda s: "_".join(map(str, s)))
def test_tail_drain(oracle_mod, sizes):
    """Batches of 1, 63, 65 and 6,145 records of (nearly) distinct keys, each fired alone and all
    four as the passes of one window: the last window of a walk is short, the walk ends with
    records queued, and a bucket's whole tile range holds fewer than 64 misses."""
    rng = np.random.default_rng(15)
    batches = []
    for rep in range(2):   # the second window: the same operator again
        for n in sizes:
            key = rng.integers(0, 5000, n).astype(np.int64)
            ts = (1000 * rep + rng.integers(0, 1000, n)).astype(np.int64)
            batches.append((key, ts, rng.random(n) * 1000.0, None))
        batches[-1] = batches[-1][:3] + (1000 * rep + 999,)
    drive(oracle_mod, batches)


def test_full_table_through_the_queue(oracle_mod, monkeypatch):
    """The shape of test_tile_fire_bucket_overflow_splits at ~400k records: 2^6 regions, 16
    buckets of ~24k distinct keys against the 8,192-slot table, ten passes (more than a spread
    fire walks, so the plain fire takes them). A queued record that finds no slot fails the item;
    the regions split and are fired again from the same passes."""
    monkeypatch.setenv("FG_MIN_REGION_BITS", "6")
    rng = np.random.default_rng(16)
    n = 400_000
    key = rng.permutation(np.arange(n, dtype=np.int64))
    key[rng.integers(0, n, 20_000)] = key[rng.integers(0, n, 20_000)]   # some keys twice, some never
    per_bucket = np.bincount(bucket_of(np.unique(key), bits=6))
    assert len(per_bucket) == 16 and per_bucket.min() > 8192
    ks, st0, st = drive(oracle_mod, one_window(key, rng, parts=10))
    assert st0["state_regions"] == 64 and st["state_regions"] >= 128, (st0, st)
