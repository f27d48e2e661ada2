"""Top-N rows per fired window (fg_set_fired_topn) on the GPU.

The reference is never the selection under test: the same stream goes through the same calls to a
second operator with the selection off (the path the oracle parity tests check), and its rows are
reduced here with numpy: lexsort on (window_end, NULL side, +-order value, key), the first n of every
window. The order is restated below -- BIGINT columns as signed integers; DOUBLE columns in
Double.compare's order on doubleToLongBits (every NaN the canonical NaN, above +inf; -0.0 below
+0.0); a NULL aggregate the smallest value (last when descending, first when ascending); ties to the
smaller signed key. The comparison is exact: the rows, their order, every column, every bit.

DOUBLE streams hold multiples of 2^-10 (or single values per key), so that a sum has the same bits in
every summation order and two handles agree bit for bit (tests/test_gpu_fired_runs.py explains)."""
import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from tests.streams import keys_in_one_region, make_stream
from tests.test_gpu_fired_runs import check_directory

pytestmark = pytest.mark.gpu

JMAX = (1 << 63) - 1
T0 = 1_600_000_000_000
CHUNK = 16_384   # rows per workgroup of the candidate pass (fg_kernels.h kTopnChunk)


# ---- the reference ------------------------------------------------------------------------------------

def order_word(col):
    """int64 whose signed order is the column's SQL order"""
    if col.dtype == np.float64:
        b = col.view(np.int64).copy()
        nan = (b & np.int64(JMAX)) > np.int64(0x7FF0000000000000)
        b[nan] = np.int64(0x7FF8000000000000)                 # Double.doubleToLongBits
        return np.where(b >= 0, b, b ^ np.int64(JMAX))        # sign-magnitude -> two's complement order
    return col.astype(np.int64)


def select(rows, n, agg, desc):
    """ROW_NUMBER() OVER (PARTITION BY window_end ORDER BY agg [DESC]) <= n of the unselected rows"""
    null = rows[agg + "_null"]
    w = order_word(rows[agg])
    val = np.where(null, np.int64(0), ~w if desc else w)      # (~w = -w - 1: the reversed order, no overflow)
    side = null.astype(np.int8) if desc else (~null).astype(np.int8)
    r = rows[np.lexsort((rows["key"], val, side, rows["window_end"]))]
    we = r["window_end"]
    first = np.flatnonzero(np.r_[True, we[1:] != we[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(r)) - np.repeat(first, np.diff(np.r_[first, len(r)]))
    return r[rank < n]


def assert_rows_identical(exp, got, ctx=""):
    assert exp.dtype == got.dtype, ctx
    assert len(exp) == len(got), f"{ctx}: {len(exp)} expected rows, {len(got)} returned"
    for f in exp.dtype.names:
        x, y = exp[f], got[f]
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        bad = np.flatnonzero(x != y)
        assert len(bad) == 0, f"{ctx}: column {f} differs in {len(bad)} rows, first at {bad[:3]}: {exp[bad[:3]]} vs {got[bad[:3]]}"


class Pair:
    """an operator with the selection off and one with it on, driven through the same calls"""

    def __init__(self, window, topn, on_kw=None, **kw):
        self.topn = topn
        self.off = F.WindowAggOperator(window, **kw)
        self.on = F.WindowAggOperator(window, topn=topn, **dict(kw, **(on_kw or {})))
        self.rows_in = self.rows_out = 0

    def batch(self, key, ts, val=None, isnull=None):
        for op in (self.off, self.on):
            op.process_batch(key, ts, val, isnull)

    def check(self, full, got, ctx=""):
        exp = select(full, *self.topn)
        assert_rows_identical(exp, got, ctx)
        assert self.off.stats()["rows_fired"] == self.on.stats()["rows_fired"], ctx
        self.rows_in += len(full)
        self.rows_out += len(got)
        return full, got

    def watermark(self, wm, ctx=""):
        return self.check(self.off.process_watermark(wm), self.on.process_watermark(wm), f"{ctx} wm {wm}")

    def watermark_device(self, wm, ctx=""):
        a = self.off.rows_to_host(self.off.process_watermark(wm, device_output=True))
        d = self.on.process_watermark(wm, device_output=True)
        assert d.location == L.DEVICE
        return self.check(a, self.on.rows_to_host(d), f"{ctx} device wm {wm}")

    def close(self):
        self.off.close()
        self.on.close()


def windows_of(rows):
    we, cnt = np.unique(rows["window_end"], return_counts=True)
    return dict(zip(we.tolist(), cnt.tolist()))


# ---- 1. TUMBLE, BIGINT: COUNT(*) / SUM / AVG ---------------------------------------------------------

def bigint_stream():
    """150k records of ~40k keys in one second: one window of ~39k rows = two full chunks of the
    candidate pass and a ragged third; counts of 0 .. 12 (many ties), sums of both signs"""
    key, ts, _, _ = make_stream(150_000, 40_000, "i64", t0=T0, rate_per_ms=150)
    rng = np.random.default_rng(11)
    val = rng.integers(-1_000_000, 1_000_000, len(key)).astype(np.int64)
    return key, ts, val


@pytest.fixture(scope="module")
def bigint_full():
    key, ts, val = bigint_stream()
    op = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum", "avg"), val_type="i64", expected_keys=40_000)
    op.process_batch(key, ts, val)
    rows = op.process_watermark(JMAX)
    op.close()
    assert 2 * CHUNK < len(rows) < 3 * CHUNK and len(rows) % 1024 != 0
    assert len(np.unique(rows["window_end"])) == 1
    return rows


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("agg", ["count_star", "sum"])
@pytest.mark.parametrize("n", [1, 7, 1024])
def test_tumble_bigint(bigint_full, n, agg, desc):
    key, ts, val = bigint_stream()
    op = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum", "avg"), val_type="i64", expected_keys=40_000,
                             topn=(n, agg, desc))
    op.process_batch(key, ts, val)
    got = op.process_watermark(JMAX)
    assert op.stats()["rows_fired"] == len(bigint_full)
    op.close()
    assert len(got) == n
    assert_rows_identical(select(bigint_full, n, agg, desc), got, f"n={n} {agg} desc={desc}")


def test_tumble_bigint_device_rows_and_batches():
    """the same stream in batches with a watermark after each, device rows"""
    key, ts, val = bigint_stream()
    p = Pair(F.tumbling(250), (7, "avg", True), aggs=("count_star", "sum", "avg"), val_type="i64", expected_keys=40_000)
    for lo in range(0, len(key), 50_000):
        p.batch(key[lo:lo + 50_000], ts[lo:lo + 50_000], val[lo:lo + 50_000])
        p.watermark_device(int(ts[lo:lo + 50_000].max()) - 1)
    p.watermark_device(JMAX)
    assert p.rows_in > 60_000 and p.rows_out == 4 * 7
    p.close()


# ---- 2. n larger than a window's rows ------------------------------------------------------------------

def test_window_with_fewer_rows_than_n():
    p = Pair(F.tumbling(1000), (10, "sum", True), val_type="i64", expected_keys=100)
    key = np.array([5, -3, 9, 5, 9, 9], dtype=np.int64)
    p.batch(key, T0 + np.arange(6, dtype=np.int64), np.array([10, 20, 1, 10, 1, 1], dtype=np.int64))
    full, got = p.watermark(JMAX)
    assert len(full) == 3 and got["key"].tolist() == [-3, 5, 9] and got["sum"].tolist() == [20, 20, 3]   # (tie: key -3 first)
    empty = p.on.process_watermark(JMAX)    # nothing fires: no rows
    assert len(empty) == 0
    p.close()


# ---- 3. several windows of very unequal size in one call ---------------------------------------------

def hop_stream():
    """HOP 4 s / 1 s: 50k keys in second 0 (twice each for a fifth of them), 5 keys in second 7 --
    windows ending at +1 .. +4 s hold 50k rows (three full chunks and a tail), +8 .. +11 s five"""
    rng = np.random.default_rng(5)
    k0 = rng.permutation(50_000).astype(np.int64)
    k0 = np.concatenate([k0, k0[:10_000]])
    t0 = T0 + (np.arange(len(k0), dtype=np.int64) * 999) // len(k0)
    k1 = np.array([7, 3, 60_000, 11, 2], dtype=np.int64)
    t1 = T0 + 7_000 + np.arange(5, dtype=np.int64)
    key, ts = np.concatenate([k0, k1]), np.concatenate([t0, t1])
    val = (rng.integers(0, 4096, len(key)) / 1024.0).astype(np.float64)
    return key, ts, val


@pytest.mark.parametrize("topn", [(7, "sum", True), (100, "count_star", False)], ids=["7_sum_desc", "100_count_asc"])
def test_hop_one_watermark_fires_unequal_windows(topn):
    key, ts, val = hop_stream()
    p = Pair(F.hopping(4000, 1000), topn, expected_keys=50_000)
    p.batch(key, ts, val)
    full, got = p.watermark(JMAX)
    sizes = windows_of(full)
    assert len(sizes) == 8 and max(sizes.values()) == 50_000 and min(sizes.values()) == 5
    n = topn[0]
    assert windows_of(got) == {we: min(n, c) for we, c in sizes.items()}     # per-window counts and offsets
    assert (np.diff(got["window_end"]) >= 0).all()                          # windows by ascending window_end
    p.close()


# ---- 4. ties -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [True, False], ids=["wide_keys", "narrow_keys"])
def test_all_tied_gives_the_smallest_keys_in_key_order(wide):
    rng = np.random.default_rng(3)
    if wide:   # negative keys and keys beyond 2^32: the wide staging path
        key = np.concatenate([-(1 << 40) + np.arange(15_000), np.arange(-5_000, 5_000), (1 << 33) + np.arange(15_000)])
    else:
        key = np.arange(40_000)
    key = rng.permutation(key).astype(np.int64)
    ts = T0 + (np.arange(len(key), dtype=np.int64) % 1000)
    p = Pair(F.tumbling(1000), (100, "count_star", True), val_type="i64", expected_keys=40_000)
    p.batch(key, ts, np.ones(len(key), dtype=np.int64))
    full, got = p.watermark(JMAX)
    assert (full["count_star"] == 1).all() and len(full) == len(key)
    assert np.array_equal(got["key"], np.sort(key)[:100])
    p.close()


# ---- 5. a DOUBLE order column ---------------------------------------------------------------------------

def double_stream():
    """one value per special key (so SUM = MIN = MAX = the value where the engine keeps it), keys
    that hold only NULL values (NULL SUM / MIN / MAX), and 3,000 ordinary keys"""
    neg_nan = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
    pay_nan = np.array([0x7FF0000000000123], dtype=np.uint64).view(np.float64)[0]
    sp = np.array([-0.0, 0.0, -5.5, 3.25, np.inf, -np.inf, np.nan, neg_nan, pay_nan, -1e300, 1e-310], dtype=np.float64)
    ksp = 100_000 + np.arange(len(sp), dtype=np.int64)
    knull = 200_000 + np.arange(6, dtype=np.int64)
    rng = np.random.default_rng(9)
    kord = rng.integers(0, 3_000, 12_000).astype(np.int64)
    vord = (rng.integers(-4096, 4096, len(kord)) / 1024.0).astype(np.float64)
    key = np.concatenate([ksp, knull, knull, kord])
    val = np.concatenate([sp, np.zeros(12), vord])
    isnull = np.concatenate([np.zeros(len(sp)), np.ones(12), np.zeros(len(kord))]).astype(np.uint8)
    o = rng.permutation(len(key))
    key, val, isnull = key[o], val[o], isnull[o]
    ts = T0 + (np.arange(len(key), dtype=np.int64) % 2000)     # two windows
    return key, ts, val, isnull


@pytest.mark.parametrize("desc", [True, False], ids=["desc", "asc"])
@pytest.mark.parametrize("agg", ["sum", "min", "max"])
def test_double_order_column(agg, desc):
    key, ts, val, isnull = double_stream()
    p = Pair(F.tumbling(1000), (40, agg, desc), aggs=("count", "sum", "min", "max"), expected_keys=4_000)
    p.batch(key, ts, val, isnull)
    full, got = p.watermark(JMAX)
    # the reference rows hold what the order has to tell apart
    bits = full[agg].view(np.int64)[~full[agg + "_null"]]
    assert full[agg + "_null"].sum() >= 6                                        # the NULL aggregates
    assert np.isposinf(full[agg]).any() and np.isneginf(full[agg]).any()
    if agg == "sum":     # (SQL MIN / MAX compare with < and >: a NaN never replaces the accumulator)
        assert np.isnan(full[agg]).any()
    assert (bits == 0).any()                                                     # +0.0
    if agg != "sum":
        assert (bits == np.int64(-(1 << 63))).any()                              # -0.0 (a SUM starts from +0.0)
    # NULLs are the smallest: with n = 40 an ascending selection starts with them, a descending one has none
    if desc:
        assert not got[agg + "_null"].any()
    else:
        for we in np.unique(got["window_end"]):
            w = got[got["window_end"] == we]
            k = int(full[agg + "_null"][full["window_end"] == we].sum())
            assert w[agg + "_null"][:k].all() and not w[agg + "_null"][k:].any()
    p.close()


# ---- 6. run mode --------------------------------------------------------------------------------------

def test_run_mode_composes():
    key, ts, val = hop_stream()
    topn = (7, "sum", True)
    p = Pair(F.hopping(4000, 1000), topn, on_kw=dict(fired_runs=True), expected_keys=50_000)
    plain = F.WindowAggOperator(F.hopping(4000, 1000), topn=topn, expected_keys=50_000)
    for op in (p.off, p.on, plain):
        op.process_batch(key, ts, val)
    a = p.off.rows_to_host(p.off.process_watermark(T0 + 5_000, device_output=True))
    d = p.on.process_watermark(T0 + 5_000, device_output=True)
    assert d.window_start is None and d.window_end is None and d.rowtime is None    # run mode: NULL window columns
    assert d.n == 4 * 7 and d.key and d.null_mask and d.agg[0]
    runs = p.on.fired_runs()
    assert check_directory(runs, d.n) == 4                                          # exactly one run per window
    assert (np.diff(runs["window_end"]) > 0).all() and (runs["rows"] == 7).all()
    got = p.on.rows_to_host(d)
    p.check(a, got, "run mode, device")
    assert_rows_identical(plain.process_watermark(T0 + 5_000), got, "run mode vs window columns")
    full, got = p.watermark(JMAX, "run mode, host")
    runs = p.on.fired_runs()
    assert check_directory(runs, len(got)) == 4 and runs["rows"].tolist() == [5, 5, 5, 5]
    assert_rows_identical(plain.process_watermark(JMAX), got, "run mode vs window columns")
    plain.close()
    p.close()


# ---- 7. async ---------------------------------------------------------------------------------------------

def tumble_stream(n=120_000, keys=20_000, seconds=4, seed=21):
    key, ts, val, _ = make_stream(n, keys, "f64", t0=T0, rate_per_ms=n // (1000 * seconds), seed=seed)
    return key, ts, np.floor(val * 1024.0) / 1024.0


def test_two_async_advances_collected_to_host():
    key, ts, val = tumble_stream()
    p = Pair(F.tumbling(1000), (25, "sum", True), expected_keys=20_000)
    p.batch(key, ts, val)
    for op in (p.off, p.on):
        assert op.process_watermark(T0 + 1_999, device_output=True, wait=False) is None   # windows +1 s, +2 s
        assert op.process_watermark(T0 + 2_999, device_output=True, wait=False) is None   # window +3 s
    full, got = p.check(p.off.collect_fired(host=True), p.on.collect_fired(host=True), "collect")
    assert len(windows_of(full)) == 3 and len(got) == 75
    assert len(p.on.collect_fired(host=True)) == 0     # drained
    p.watermark(JMAX, "rest")
    p.close()


def test_uncollected_async_rows_lead_a_synchronous_advance():
    key, ts, val = tumble_stream()
    p = Pair(F.tumbling(1000), (25, "count_star", False), expected_keys=20_000)
    p.batch(key, ts, val)
    for op in (p.off, p.on):
        assert op.process_watermark(T0 + 1_999, device_output=True, wait=False) is None
    full, got = p.watermark(T0 + 3_500, "lead")     # its own windows (+3 s) after the async ones (+1 s, +2 s)
    assert len(windows_of(full)) == 3 and len(got) == 75
    p.watermark_device(JMAX, "rest")
    p.close()


# ---- 8. a window in more than one run --------------------------------------------------------------------

def test_window_split_over_several_runs_is_selected_once():
    """tests/test_gpu_fired_runs.py test_region_overflow_repeats_a_window's recipe: an operator sized for
    1,000 keys fires two windows of ~23k keys, one region keeps overflowing after its siblings passed, and
    its children's rows of both windows follow the siblings' rows -- each window sits in several runs"""
    key, ts, val, _ = make_stream(200_000, 20_000, "f64", t0=T0, rate_per_ms=100)
    val = np.floor(val * 1024.0) / 1024.0
    kc = keys_in_one_region(3_000)
    tc = T0 + np.arange(3_000, dtype=np.int64) % 1000
    vc = (np.arange(3_000) % 512) / 1024.0
    key, ts, val = np.concatenate([key, kc, kc]), np.concatenate([ts, tc, tc + 1000]), np.concatenate([val, vc, vc + 1.0])
    kw = dict(expected_keys=1_000, buffer_records=1 << 20)
    p = Pair(F.tumbling(1000), (50, "sum", False), **kw)
    runs_op = F.WindowAggOperator(F.tumbling(1000), fired_runs=True, **kw)     # shows the raw directory
    for op in (p.off, p.on, runs_op):
        op.process_batch(key, ts, val)
    raw = runs_op.process_watermark(T0 + 1_999)
    d = runs_op.fired_runs()
    assert len(np.unique(d["window_end"])) == 2 and len(d["rows"]) > 2, d         # a window in more than one run
    full, got = p.watermark(T0 + 1_999, "overflow")
    assert len(full) == len(raw) and len(got) == 100
    assert p.on.stats()["state_regions"] >= 16
    runs_op.close()
    p.close()


# ---- 9. accounting ----------------------------------------------------------------------------------------

def test_statistics_and_the_default_kernel_list():
    key, ts, val = tumble_stream()
    p = Pair(F.tumbling(1000), (10, "sum", True), expected_keys=20_000, kernel_timing=True)
    p.batch(key, ts, val)
    p.watermark(T0 + 2_500)
    p.watermark_device(JMAX)
    ks_on, ks_off = p.on.kernel_stats(), p.off.kernel_stats()
    # a handle that never had the selection on: its list is what it was, no launch of the pass
    assert "topn" not in ks_off and "late_out" not in ks_off
    assert list(ks_on)[:-1] == list(ks_off) and list(ks_on)[-1] == "topn"
    t = ks_on["topn"]
    assert t["records"] == p.rows_in == p.off.stats()["rows_fired"] and t["rows"] == p.rows_out == 40
    assert t["launches"] == 2 and t["total_ms"] > 0          # one bracket per returning call with rows
    assert p.on.stats() == p.off.stats()
    # late_out and topn both listed: topn last
    both = F.WindowAggOperator(F.tumbling(1000), mode="datastream", val_type="i64", aggs=("count_star", "sum"),
                               late_output=True, topn=(3, "sum", True), expected_keys=100, kernel_timing=True)
    assert list(both.kernel_stats())[-2:] == ["late_out", "topn"]
    both.close()
    p.close()


def test_snapshot_restore_and_refire():
    rng = np.random.default_rng(7)

    def recs(n, lo, hi):
        return (rng.integers(0, 300, n).astype(np.int64), rng.integers(lo, hi, n).astype(np.int64),
                rng.integers(-50, 50, n).astype(np.int64))
    kw = dict(val_type="i64", expected_keys=300, buffer_records=1 << 16)
    topn = (5, "sum", True)
    p = Pair(F.hopping(2000, 500), topn, **kw)
    p.batch(*recs(5000, 0, 5000))
    p.watermark(2999, "before the checkpoint")
    p2 = Pair(F.hopping(2000, 500), topn, **kw)
    images = []
    for old, new in ((p.off, p2.off), (p.on, p2.on)):
        old.prepare_snapshot_pre_barrier()
        img, wm = old.snapshot_state()
        images.append(img)
        new.restore_state(img, wm)
    for k in images[0]:     # the state is what it is with the selection off
        o0, o1 = (np.lexsort((im["key"], im["slice_end"])) for im in images)
        assert np.array_equal(images[0][k][o0], images[1][k][o1]), k
    p.close()
    p2.batch(*recs(4000, 0, 7000))
    p2.watermark(1999, "below the checkpoint's watermark")      # the re-fire of windows fired before it
    assert p2.rows_in > 0
    p2.batch(*recs(3000, 1000, 8000))
    p2.watermark(5999, "above it")
    p2.watermark(JMAX, "final")
    p2.close()


# ---- 10. switching ----------------------------------------------------------------------------------------

def test_switching_on_and_off():
    key, ts, val = tumble_stream()
    p = Pair(F.tumbling(1000), (10, "sum", True), expected_keys=20_000)
    p.batch(key, ts, val)
    for op in (p.off, p.on):
        assert op.process_watermark(T0 + 1_500, device_output=True, wait=False) is None
    for n in (0, 20):       # uncollected rows: neither off nor another n
        with pytest.raises(F.FlinkGpuError) as e:
            p.on.set_fired_topn(n, "sum")
        assert e.value.code == L.FG_ESTATE and "collect" in e.value.msg
    a, d = p.off.rows_to_host(p.off.collect_fired()), p.on.collect_fired()
    assert d.n == 10
    p.check(a, p.on.rows_to_host(d), "collect")
    p.on.set_fired_topn(0)                      # off: full rows again, in the fire's order
    full, got = p.off.process_watermark(T0 + 2_500), p.on.process_watermark(T0 + 2_500)
    assert len(got) == len(full) > 10
    o0, o1 = np.lexsort((full["key"], full["window_end"])), np.lexsort((got["key"], got["window_end"]))
    assert_rows_identical(full[o0], got[o1], "selection off")
    p.on.set_fired_topn(3, "count_star", False)     # on again, another order
    p.topn = (3, "count_star", False)
    p.watermark(JMAX, "on again")
    p.close()
