"""Fired rows as runs (fg_set_fired_runs / fg_fired_runs) on the GPU.

(a) Against the oracle: the golden operator cases through a run-mode operator (the structured rows
    it returns take their window columns from the run directory).
(b) Twins: a classic and a run-mode operator fed the same seeded stream through the same calls.
    After every call that returns rows the run directory must hold its invariants, the rows --
    sorted by (window_end, key) -- must be bit-equal (DOUBLE sums included: the arithmetic is the
    same code on the same input), the run-mode device FgRows must carry NULL window columns, and
    rows_fired must agree. A misplaced run boundary gives some row the wrong window, so the row
    comparison checks the boundaries too.

DOUBLE values of the twin streams are multiples of 2^-10 (tests/streams.py's values rounded down to
them): their sums are exact in every order, so the bits of a DOUBLE SUM / AVG do not depend on the
order in which the engine's LDS f64 atomics of several waves land -- which is scheduling order, not
fixed from one run to the next (DESIGN.md section 7b says the same of the restore). On the unrounded
stream two CLASSIC handles already differ from each other in the last bits of sums of three or more
values (DESIGN.md section 7f has the counts), so a bit-for-bit comparison there would measure the
scheduler, not run mode; test_unrounded_doubles checks on that stream everything that is defined
bit for bit."""
import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from flink_amd.window_agg import expand_runs
from tests.fixture_runner import load_operator_cases, run_case
from tests.gpu_adapter import GpuOperator, window_of
from tests.streams import make_stream

pytestmark = pytest.mark.gpu

JMAX = (1 << 63) - 1
T0 = 1_600_000_000_000


# ---- the directory -----------------------------------------------------------------------------------

def check_directory(runs, n):
    """the invariants include/flinkgpu.h states for fg_fired_runs; returns the number of runs"""
    ws, we, rt, first, rows = (runs[k] for k in ("window_start", "window_end", "rowtime", "first_row", "rows"))
    m = len(we)
    assert len(ws) == len(rt) == len(first) == len(rows) == m
    if n == 0:
        assert m == 0
        return 0
    assert m > 0 and first[0] == 0
    assert (rows > 0).all()
    assert np.array_equal(first[1:], (first + rows)[:-1])
    assert int(rows.sum()) == n
    assert np.array_equal(rt, we - 1)
    assert (we[1:] != we[:-1]).all()          # adjacent runs of one window are merged
    assert (ws < we).all()
    expand_runs(runs, n)                      # (the host expansion accepts it)
    return m


def assert_same_rows(classic, run, ctx=""):
    assert classic.dtype == run.dtype, ctx
    assert len(classic) == len(run), f"{ctx}: {len(classic)} classic rows, {len(run)} run-mode rows"
    a = classic[np.lexsort((classic["key"], classic["window_end"]))]
    b = run[np.lexsort((run["key"], run["window_end"]))]
    for f in a.dtype.names:   # bit-equal, column by column (a DOUBLE by its bits)
        x, y = a[f], b[f]
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        bad = np.flatnonzero(x != y)
        assert len(bad) == 0, f"{ctx}: column {f} differs in {len(bad)} rows, first {a[bad[:3]]} vs {b[bad[:3]]}"


def assert_null_window_columns(dev_rows):
    assert dev_rows.location == L.DEVICE
    assert dev_rows.window_start is None and dev_rows.window_end is None and dev_rows.rowtime is None
    if dev_rows.n > 0:
        assert dev_rows.key and dev_rows.null_mask and dev_rows.agg[0]


class Twins:
    """a classic and a run-mode operator of one configuration, driven through the same calls"""

    def __init__(self, window, **kw):
        self.c = F.WindowAggOperator(window, **kw)
        self.r = F.WindowAggOperator(window, fired_runs=True, **kw)
        self.n_runs = []      # runs of every checked call
        self.windows = []     # distinct windows of every checked call
        self.rows = 0

    def both(self):
        return (self.c, self.r)

    def batch(self, key, ts, val=None, isnull=None):
        for op in self.both():
            op.process_batch(key, ts, val, isnull)

    def check(self, classic_rows, run_rows, ctx):
        runs = self.r.fired_runs()
        self.n_runs.append(check_directory(runs, len(run_rows)))
        self.windows.append(len(np.unique(runs["window_end"])))
        assert_same_rows(classic_rows, run_rows, ctx)
        if "rowtime" in run_rows.dtype.names:   # DataStream: a run's rowtime is the classic column of its window
            for we, rt in zip(runs["window_end"], runs["rowtime"]):
                col = classic_rows["rowtime"][classic_rows["window_end"] == we]
                assert len(col) > 0 and (col == rt).all(), (ctx, we, rt)
        assert self.c.stats()["rows_fired"] == self.r.stats()["rows_fired"], ctx
        self.rows += len(run_rows)

    def watermark(self, wm, ctx=""):
        """a synchronous watermark, host rows"""
        a, b = self.c.process_watermark(wm), self.r.process_watermark(wm)
        self.check(a, b, f"{ctx} wm {wm}")

    def watermark_device(self, wm, ctx=""):
        a = self.c.rows_to_host(self.c.process_watermark(wm, device_output=True))
        d = self.r.process_watermark(wm, device_output=True)
        assert_null_window_columns(d)
        self.check(a, self.r.rows_to_host(d), f"{ctx} device wm {wm}")

    def collect(self, host, ctx=""):
        if host:
            a, b = self.c.collect_fired(host=True), self.r.collect_fired(host=True)
        else:
            a = self.c.rows_to_host(self.c.collect_fired())
            d = self.r.collect_fired()
            assert_null_window_columns(d)
            b = self.r.rows_to_host(d)
        self.check(a, b, f"{ctx} collect host={host}")

    def close(self):
        for op in self.both():
            op.close()


def stream(n=200_000, keys=5_000, vt="f64", rate=25, exact=True, **kw):
    """~200k records over 8 s (rate 25 / ms): 8 tumbling seconds, 10 hops, 8 cumulate steps.
    exact: DOUBLE values rounded down to multiples of 2^-10 (below 1000: 20 significant bits), so
    that a sum of up to 2^30 of them has the same bits in every summation order"""
    key, ts, val, isnull = make_stream(n, keys, vt, t0=T0, rate_per_ms=rate, **kw)
    if vt == "f64" and exact:
        val = np.floor(val * 1024.0) / 1024.0
    return key, ts, val, isnull


def drive(tw, cols, batch=25_000, delay=0, how="host"):
    key, ts, val, isnull = cols
    n = len(key)
    mx, nb = np.iinfo(np.int64).min, 0
    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        tw.batch(key[lo:hi], ts[lo:hi], val[lo:hi], None if isnull is None else isnull[lo:hi])
        mx = max(mx, int(ts[lo:hi].max()))
        wm = mx - delay - 1
        nb += 1
        if how == "host":
            tw.watermark(wm, f"batch {nb}")
        elif how == "device":
            tw.watermark_device(wm, f"batch {nb}")
        elif how in ("async_host", "async_device"):
            # several watermarks per batch (most of them quiet), collected once per two batches
            for op in tw.both():
                op.process_watermarks([wm - 700, wm - 300, wm])
            if nb % 2 == 0:
                tw.collect(how == "async_host", f"batch {nb}")
        elif how == "lead":
            # an async advance whose rows are not collected, then a synchronous one: its rows follow
            if nb % 2 == 1:
                for op in tw.both():
                    assert op.process_watermark(wm, device_output=True, wait=False) is None
            else:
                tw.watermark(wm, f"batch {nb}")
        else:
            assert how == "none"
    if how in ("async_host", "async_device"):
        for op in tw.both():
            op.process_watermarks([JMAX])
        tw.collect(how == "async_host", "final")
    elif how != "none":
        tw.watermark(JMAX, "final")


# ---- (a) the golden cases through a run-mode operator -------------------------------------------------

class RunModeOperator(GpuOperator):
    """GpuOperator over a run-mode WindowAggOperator; a restored copy keeps the mode"""

    def __init__(self, cfg):
        super().__init__(cfg, _op=F.WindowAggOperator(
            window_of(cfg), aggs=cfg.get("aggs", ("count_star", "count", "sum", "avg", "sum0")),
            val_type=cfg["val_type"], mode=cfg["mode"], shift_tz_offset_ms=cfg.get("tz_offset_ms", 0),
            expected_keys=1 << 12, buffer_records=1 << 20, proctime=cfg.get("proctime", False), zone=cfg.get("zone"),
            windowed=cfg.get("windowed", False), allowed_lateness=cfg.get("allowed_lateness", 0),
            purging_trigger=cfg.get("purging", False), fired_runs=True))

    def process_watermark(self, wm):
        super().process_watermark(wm)
        check_directory(self.op.fired_runs(), len(self._rows[-1]))

    def restore_copy(self):
        new = super().restore_copy()
        new.op.set_fired_runs(True)
        new.__class__ = RunModeOperator
        return new


GOLDEN = [c for c in load_operator_cases() if c["name"] in (
    "sql_tumble_3s_UTC", "sql_hop_3s_1s_UTC", "sql_cumulate_3s_1s_UTC", "sql_tumble_3s_Asia/Shanghai",
    "sql_hop_3s_1s_Asia/Shanghai", "sql_cumulate_3s_1s_Asia/Shanghai", "ds_tumble_3s_reduce", "ds_sliding_3s_1s_reduce")]


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_cases_in_run_mode(case):
    assert any(e[0] == "snapshot_restore" for e in case["events"])   # (their mid-stream restore)
    results, late = run_case(case, RunModeOperator)
    for step, got, exp in results:
        assert got == exp, f"{case['name']} step {step}: got {got} expected {exp}"
    if case["expected_late_dropped"] is not None:
        assert late == case["expected_late_dropped"]


def test_golden_selection_is_complete():
    assert len(GOLDEN) == 8


# ---- (b) twins ------------------------------------------------------------------------------------------

def test_tumble_tile_fire():
    tw = Twins(F.tumbling(1000), expected_keys=5_000, kernel_timing=True)
    drive(tw, stream())
    for op in tw.both():
        ks = op.kernel_stats()
        assert ks["tile_fire"]["launches"] > 0 and ks["tile_fire"]["rows"] > 0, ks   # (narrow keys: the tile path)
    assert tw.rows > 30_000
    tw.close()


def test_unrounded_doubles():
    """tests/streams.py's DOUBLE values as they are: the keys, windows, counts and NULL flags are
    bit-equal, and so are the DOUBLE SUM and AVG of every row summing at most two values (a + b has one
    value in either order); longer sums agree to the summation-order bound of n values below 1000,
    (n - 1) eps * 1000 n, as two classic handles do."""
    tw = Twins(F.tumbling(1000), expected_keys=5_000)
    key, ts, val, _ = stream(exact=False)
    tw.batch(key, ts, val)
    a, b = tw.c.process_watermark(JMAX), tw.r.process_watermark(JMAX)
    check_directory(tw.r.fired_runs(), len(b))
    a = a[np.lexsort((a["key"], a["window_end"]))]
    b = b[np.lexsort((b["key"], b["window_end"]))]
    for f in a.dtype.names:
        if f not in ("sum", "avg"):
            assert np.array_equal(a[f], b[f]), f
    short = a["count"] <= 2
    assert short.any() and (~short).any()
    for f in ("sum", "avg"):
        assert np.array_equal(a[f][short].view(np.int64), b[f][short].view(np.int64)), f
    n = a["count"].astype(np.float64)
    bound = (n - 1) * np.finfo(np.float64).eps * 1000.0 * n
    assert (np.abs(a["sum"] - b["sum"]) <= bound).all()
    assert (np.abs(a["avg"] - b["avg"]) <= bound / np.maximum(n, 1)).all()
    tw.close()


def test_one_watermark_over_three_windows():
    tw = Twins(F.tumbling(1000), expected_keys=5_000)
    cols = stream()
    drive(tw, cols, how="none")
    tw.watermark(T0 + 3_500, "jump")          # windows ending at +1 s, +2 s, +3 s in one advance
    assert tw.n_runs[-1] >= 3 and tw.windows[-1] == 3
    tw.watermark_device(T0 + 3_600, "quiet")  # nothing fires: no rows, no runs
    assert tw.n_runs[-1] == 0
    tw.watermark_device(JMAX, "rest")
    assert tw.n_runs[-1] >= 5
    tw.close()


@pytest.mark.parametrize("how", ["async_host", "async_device"])
@pytest.mark.parametrize("kind", ["tumble", "hop"])
def test_async_watermarks_collected_once(kind, how):
    tw = Twins(F.tumbling(1000) if kind == "tumble" else F.hopping(3000, 1000), expected_keys=5_000)
    drive(tw, stream(), how=how)
    assert max(tw.n_runs) >= 2    # a collect spans the windows of two batches
    tw.close()


@pytest.mark.parametrize("kind", ["tumble", "cumulate"])
def test_uncollected_async_rows_lead_a_synchronous_advance(kind):
    tw = Twins(F.tumbling(1000) if kind == "tumble" else F.cumulative(4000, 1000), expected_keys=5_000)
    drive(tw, stream(), how="lead")
    assert max(tw.n_runs) >= 2
    tw.close()


def test_hop_merge_fire_and_table_flush():
    tw = Twins(F.hopping(3000, 1000), expected_keys=5_000, kernel_timing=True)
    drive(tw, stream(jitter_ms=400), delay=200)
    for op in tw.both():
        ks = op.kernel_stats()
        assert ks["merge_fire"]["launches"] > 0 and ks["merge_fire"]["rows"] > 0, ks   # k_merge in fire mode
        assert ks["tile_flush"]["launches"] + ks["merge_flush"]["launches"] > 0, ks   # the slices' flushes
    tw.close()


def test_cumulate_fold_and_fire():
    tw = Twins(F.cumulative(4000, 1000), expected_keys=5_000, kernel_timing=True)
    drive(tw, stream())
    for op in tw.both():
        ks = op.kernel_stats()
        assert ks["tile_fire"]["rows"] + ks["merge_flush_fire"]["rows"] > 0, ks   # the fused fold + fire
    tw.close()


def test_wide_keys():
    cols = stream(key_spread=True)
    assert (np.abs(cols[0]) >= (1 << 32)).any()
    tw = Twins(F.tumbling(1000), expected_keys=5_000)
    drive(tw, cols)
    tw.close()


def test_null_values():
    tw = Twins(F.hopping(3000, 1000), expected_keys=5_000)
    drive(tw, stream(null_frac=0.2, jitter_ms=300), delay=100, how="device")
    tw.close()


@pytest.mark.parametrize("vt", ["f64", "i64"])
def test_five_aggregates_multi_value(vt):
    tw = Twins(F.cumulative(4000, 1000), aggs=("count_star", "count", "sum", "min", "max"), val_type=vt,
               expected_keys=5_000)
    drive(tw, stream(vt=vt, null_frac=0.1))
    tw.close()


def test_windowed_input():
    from tests.test_gpu_parity import windowed_rows
    key, ts, val, isnull = stream(n=100_000, keys=3_000, jitter_ms=500)
    r = windowed_rows("hop", 3000, 1000, key, ts, val, isnull)
    tw = Twins(F.hopping(3000, 1000), windowed=True, aggs=("count", "sum", "avg"), expected_keys=3_000)
    n, mx = len(r["key"]), np.iinfo(np.int64).min
    for lo in range(0, n, 40_000):
        hi = min(n, lo + 40_000)
        tw.batch(r["key"][lo:hi], r["wend"][lo:hi], r["val"][lo:hi])
        mx = max(mx, int(r["ts"][lo:hi].max()))
        tw.watermark(mx - 301, "windowed")
    tw.watermark(JMAX, "windowed final")
    assert tw.rows > 0
    tw.close()


@pytest.mark.parametrize("kind", ["tumble", "sliding"])
def test_datastream_rowtime_comes_from_the_run(kind):
    w = F.tumbling(1000) if kind == "tumble" else F.hopping(3000, 1000)
    tw = Twins(w, mode="datastream", val_type="i64", aggs=("count_star", "sum"), allowed_lateness=0,
               expected_keys=5_000)
    drive(tw, stream(vt="i64", jitter_ms=300), delay=100)
    rows = tw.r.process_watermark(JMAX)   # (nothing left)
    assert len(rows) == 0 and "rowtime" in rows.dtype.names
    tw.close()


def test_zipf_split_fire():
    """the smallest split-fire shape of tests/test_gpu_tile_split.py: 4M-record slices, Zipf 1.3"""
    cols = make_stream(6_000_000, 1_000_000, "i64", t0=T0, rate_per_ms=4_000, zipf=1.3)
    tw = Twins(F.tumbling(1000), val_type="i64", expected_keys=1_000_000, buffer_records=8_000_000,
               kernel_timing=True)
    drive(tw, cols, batch=2_000_000)
    for op in tw.both():
        ks = op.kernel_stats()
        assert ks["tile_split_fire"]["launches"] > 0, ks
    tw.close()


def test_region_overflow_repeats_a_window():
    """Two windows in one advance, each with ~20k keys in an operator sized for 1,000 (one region of
    3,584 entries): both fires overflow, the regions split and both are redone, as often as it takes.
    A region that overflows emits nothing, so with evenly spread keys every region would fail until all
    pass together and each window would still be one run. 3,000 more keys per window that share a region
    at every split (streams.keys_in_one_region) keep one region failing after its siblings passed: the
    siblings' rows of both windows are out, then that region's children are redone -- a window is in
    more than one run."""
    from tests.streams import keys_in_one_region
    key, ts, val, _ = stream(200_000, 20_000, rate=100)   # 2 s: two windows of 100k records
    kc = keys_in_one_region(3_000)
    tc = T0 + np.arange(3_000, dtype=np.int64) % 1000
    vc = (np.arange(3_000) % 512) / 1024.0
    key = np.concatenate([key, kc, kc])
    ts = np.concatenate([ts, tc, tc + 1000])
    val = np.concatenate([val, vc, vc + 1.0])
    tw = Twins(F.tumbling(1000), expected_keys=1_000, buffer_records=1 << 20)
    tw.batch(key, ts, val)
    tw.watermark(T0 + 1_999, "overflow")
    assert tw.rows > 2 * 3_584 * 4   # (far more keys per window than the one region held)
    assert tw.windows[-1] == 2
    assert tw.n_runs[-1] > tw.windows[-1], (tw.n_runs, tw.windows)
    for op in tw.both():
        assert op.stats()["state_regions"] >= 16
    tw.close()


def test_hop_restore_refires_below_and_above_the_checkpoint():
    rng = np.random.default_rng(7)

    def recs(n, lo, hi):
        return (rng.integers(0, 300, n).astype(np.int64), rng.integers(lo, hi, n).astype(np.int64),
                rng.integers(-50, 50, n).astype(np.int64))
    kw = dict(val_type="i64", expected_keys=300, buffer_records=1 << 16)
    tw = Twins(F.hopping(2000, 500), **kw)
    tw.batch(*recs(5000, 0, 5000))
    tw.watermark(2999, "before the checkpoint")
    tw2 = Twins(F.hopping(2000, 500), **kw)
    for old, new in zip(tw.both(), tw2.both()):
        old.prepare_snapshot_pre_barrier()
        new.restore_state(*old.snapshot_state())
    tw.close()
    assert tw2.r.fired_runs()["rows"].size == 0   # (a restore leaves no directory)
    tw2.batch(*recs(4000, 0, 7000))
    tw2.watermark(1999, "below the checkpoint's watermark")
    assert tw2.rows > 0
    tw2.batch(*recs(3000, 1000, 8000))
    tw2.watermark(5999, "above it")
    tw2.watermark(JMAX, "final")
    assert max(tw2.n_runs) >= 3
    tw2.close()


def test_reset_then_reuse():
    tw = Twins(F.hopping(3000, 1000), expected_keys=5_000)
    drive(tw, stream(n=100_000))
    for op in tw.both():
        op.reset()
    assert tw.r.fired_runs()["rows"].size == 0
    before = tw.rows
    drive(tw, stream(n=100_000, seed=1234), how="async_device")
    assert tw.rows > before
    tw.close()


def test_toggle_off_and_on_again():
    tw = Twins(F.tumbling(1000), expected_keys=5_000)
    cols = stream(n=100_000)
    drive(tw, cols)
    tw.r.set_fired_runs(True)      # idempotent
    tw.r.set_fired_runs(False)     # classic again: the window columns come back
    key, ts, val, _ = stream(n=50_000, seed=99)
    ts = ts + 10_000
    tw.batch(key, ts, val)
    a, b = tw.c.process_watermark(JMAX), tw.r.process_watermark(JMAX)
    assert_same_rows(a, b, "mode off")
    with pytest.raises(F.FlinkGpuError) as e:
        tw.r.fired_runs()
    assert e.value.code == L.FG_ESTATE
    tw.close()


# ---- refusals -----------------------------------------------------------------------------------------------

def test_local_partials_handle_is_refused():
    op = F.WindowAggOperator(F.tumbling(1000), local_partials=True, expected_keys=100)
    with pytest.raises(F.WindowSpecError, match="FG_FLAG_LOCAL_PARTIALS"):   # FG_EINVAL
        op.set_fired_runs(True)
    op.close()
    with pytest.raises(F.WindowSpecError, match="FG_FLAG_LOCAL_PARTIALS"):
        F.WindowAggOperator(F.tumbling(1000), local_partials=True, expected_keys=100, fired_runs=True)


def test_allowed_lateness_is_refused():
    op = F.WindowAggOperator(F.tumbling(1000), mode="datastream", val_type="i64", aggs=("count_star", "sum"),
                             allowed_lateness=500, expected_keys=100)
    with pytest.raises(F.WindowSpecError, match="allowed_lateness_ms"):       # FG_EINVAL
        op.set_fired_runs(True)
    op.set_fired_runs(False)   # (off is what it is)
    op.close()


def test_toggle_with_uncollected_rows_is_refused():
    key, ts, val, _ = stream(n=50_000)
    op = F.WindowAggOperator(F.tumbling(1000), expected_keys=5_000)
    op.process_batch(key, ts, val)
    assert op.process_watermark(T0 + 1_500, device_output=True, wait=False) is None
    with pytest.raises(F.FlinkGpuError) as e:
        op.set_fired_runs(True)
    assert e.value.code == L.FG_ESTATE and ("collect" in e.value.msg)
    n = op.collect_fired().n
    assert n > 0
    op.set_fired_runs(True)    # collected: allowed
    rows = op.process_watermark(JMAX)
    assert len(rows) > 0 and check_directory(op.fired_runs(), len(rows)) == 1
    op.close()


def test_fired_runs_on_a_classic_handle_is_refused():
    op = F.WindowAggOperator(F.tumbling(1000), expected_keys=100)
    with pytest.raises(F.FlinkGpuError) as e:
        op.fired_runs()
    assert e.value.code == L.FG_ESTATE and "run mode is off" in e.value.msg
    op.close()
