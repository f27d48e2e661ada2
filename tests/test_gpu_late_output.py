"""The late-element side output on the GPU (fg_set_late_output / fg_collect_late): with the mode on
the elements the ingest drops come back, in arrival order, and everything else the operator does is
what it does with the mode off. The expectation is tests/late_reference.dropped_mask (WindowOperator
restated, pinned to the oracle in tests/test_late_output_abi.py); every comparison is exact."""
import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from flink_amd.rows import fixed_part_size, pack_rows
from tests.fixture_runner import load_operator_cases, run_case
from tests.gpu_adapter import GpuOperator, window_of
from tests.late_reference import dropped_mask
from tests.late_streams import BATCH, CONFIGS, KEYS, batches_of, stream_of
from tests.test_late_output_abi import GOLDEN_LATE

pytestmark = pytest.mark.gpu
JMIN = -(1 << 63)


def window_obj(window):
    return F.tumbling(window[1]) if window[0] == "tumble" else F.hopping(window[1], window[2])


def make_op(window, val_type="i64", lateness=0, purging=False, late_output=False, **kw):
    aggs = ("count_star",) if val_type == "none" else ("count_star", "sum")
    return F.WindowAggOperator(window_obj(window), aggs=aggs, val_type=val_type, mode="datastream",
                               expected_keys=KEYS, buffer_records=1 << 16, allowed_lateness=lateness,
                               purging_trigger=purging, late_output=late_output, **kw)


def feed(op, how, key, ts, val, isnull):
    if how == "rows":
        rows = pack_rows([key, ts, val], nulls=[None, None, isnull.astype(bool)])
        op.process_rows(rows, stride=fixed_part_size(3), arity=3)
    elif how == "narrow":
        base = int(ts.min())
        op.process_batch(key.astype(np.int32), (ts - base).astype(np.uint32), val.astype(np.int32), isnull,
                         rowtime_base=base)
    else:
        op.process_batch(key, ts, val, isnull)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def assert_late(got, key, ts, val, isnull, mask, ctx, null_vals_zero=False):
    """the collected records are batch[mask], in order, over key, rowtime, value bits and NULL flag"""
    assert len(got["key"]) == int(mask.sum()), ctx
    assert np.array_equal(got["key"], key[mask]), ctx
    assert np.array_equal(got["rowtime"], ts[mask]), ctx
    nl = np.zeros(int(mask.sum()), dtype=np.uint8) if isnull is None else isnull[mask]
    assert got["val_null"].dtype == np.uint8 and np.array_equal(got["val_null"], nl), ctx
    if val is None:
        assert got["val"] is None, ctx
        return
    assert got["val"].dtype == val.dtype, ctx
    exp = bits(val[mask]).copy()
    if null_vals_zero:   # (a packed row's NULL field holds zero bytes: BinaryRowWriter.setNullAt)
        exp[nl != 0] = 0
    assert np.array_equal(bits(got["val"]), exp), ctx


def sorted_rows(r):
    return r[np.lexsort(tuple(bits(r[c]) if r[c].dtype.kind == "f" else r[c] for c in reversed(r.dtype.names)))]


def assert_same_rows(a, b, ctx):
    assert a.dtype == b.dtype and len(a) == len(b), ctx
    a, b = sorted_rows(a), sorted_rows(b)
    for c in a.dtype.names:
        assert np.array_equal(bits(a[c]) if a[c].dtype.kind == "f" else a[c],
                              bits(b[c]) if b[c].dtype.kind == "f" else b[c]), (ctx, c)


def assert_same_image(a, b, ctx):
    (ia, wa), (ib, wb) = a, b
    assert wa == wb and set(ia) == set(ib), ctx
    cols = [c for c in ("slice_end", "key", "cnt_star", "cnt_val", "sum") if c in ia]
    oa = np.lexsort(tuple(bits(ia[c]) for c in reversed(cols)))
    ob = np.lexsort(tuple(bits(ib[c]) for c in reversed(cols)))
    for c in cols:
        assert np.array_equal(bits(ia[c])[oa], bits(ib[c])[ob]), (ctx, c)


# ---- (a) golden ----------------------------------------------------------------------------------

class LateGpuOperator(GpuOperator):
    """the fixture runner's GPU operator with the late output on; collects after every batch"""

    def __init__(self, cfg):
        super().__init__(cfg, _op=F.WindowAggOperator(
            window_of(cfg), aggs=("count_star", "count", "sum", "avg", "sum0"), val_type=cfg["val_type"],
            mode=cfg["mode"], expected_keys=1 << 12, buffer_records=1 << 20,
            allowed_lateness=cfg.get("allowed_lateness", 0), purging_trigger=cfg.get("purging", False),
            late_output=True))
        self.late = []

    def process_batch(self, key, ts, val=None, isnull=None):
        super().process_batch(key, ts, val, isnull)
        r = self.op.collect_late()
        self.late += list(zip(r["key"].tolist(), r["val"].tolist(), r["rowtime"].tolist()))


@pytest.mark.parametrize("name", list(GOLDEN_LATE))
def test_golden_side_output(name):
    case = next(c for c in load_operator_cases() if c["name"] == name)
    made = []

    def mk(cfg):
        made.append(LateGpuOperator(cfg))
        return made[-1]
    results, late_dropped = run_case(case, mk)
    for step, got, exp in results:
        assert got == exp, f"{name} step {step}: got {got} expected {exp}"
    assert made[0].late == GOLDEN_LATE[name]
    assert late_dropped == 0


# ---- (b) twins -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONFIGS))
def test_twins(name):
    c = CONFIGS[name]
    key, ts, val, isnull = stream_of(name)
    kw = dict(val_type=c["val_type"], lateness=c["lateness"], purging=c["purging"])
    off, on = make_op(c["window"], **kw), make_op(c["window"], late_output=True, **kw)
    try:
        progress, collected = JMIN, 0
        for lo, hi, wm in batches_of(name, ts):
            b = (key[lo:hi], ts[lo:hi], None if val is None else val[lo:hi], None if isnull is None else isnull[lo:hi])
            for op in (off, on):
                feed(op, c["feed"], *b)
            mask = dropped_mask(b[1], progress, c["window"], c["lateness"], c["purging"])
            got = on.collect_late()
            assert_late(got, *b, mask, (name, lo), null_vals_zero=c["feed"] == "rows")
            collected += len(got["key"])
            assert_same_rows(on.process_watermark(wm), off.process_watermark(wm), (name, lo, wm))
            progress = max(progress, wm)
        assert collected == off.num_late_records_dropped > 0
        assert on.num_late_records_dropped == 0
        so, sn = off.stats(), on.stats()
        assert {k: v for k, v in sn.items() if k != "late_dropped"} == {k: v for k, v in so.items() if k != "late_dropped"}
        assert_same_image(on.snapshot_state(), off.snapshot_state(), name)
        assert_same_rows(on.process_watermark((1 << 63) - 1), off.process_watermark((1 << 63) - 1), (name, "end"))
        assert len(on.collect_late()["key"]) == 0
    finally:
        off.close()
        on.close()


# ---- (c) chunk edges -----------------------------------------------------------------------------

T0 = 1_700_000_000_000   # a window start of the 1 s tumbling window


def edge_patterns(n):
    i = np.arange(n)
    return {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool),
            "half": np.random.default_rng(n).random(n) < 0.5,
            "edges": (i % 256 == 255) | (i % 256 == 0)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3 * 16384 + 17])
def test_chunk_edges(n):
    window = ("tumble", 1000)
    op = make_op(window, val_type="i64", late_output=True)
    try:
        op.process_batch(np.array([1, 2], dtype=np.int64), np.array([T0 + 5, T0 + 900], dtype=np.int64),
                         np.array([1, 1], dtype=np.int64))
        assert len(op.collect_late()["key"]) == 0
        assert len(op.process_watermark(T0 + 999)) == 2   # the window [T0, T0 + 1000) fired
        i = np.arange(n, dtype=np.int64)
        key = (i * 7919) % KEYS
        val = i * 3 - 1000
        total = 0
        for pname, late in edge_patterns(n).items():
            # late elements fall into the fired window, the others into the two windows after it
            ts = np.where(late, T0 + (i * 37) % 1000, T0 + 1000 + (i * 41) % 2000).astype(np.int64)
            mask = dropped_mask(ts, T0 + 999, window)
            assert np.array_equal(mask, late), pname
            op.process_batch(key, ts, val)
            assert_late(op.collect_late(), key, ts, val, None, mask, (n, pname))
            total += int(late.sum())
        assert op.num_late_records_dropped == 0
        fired = op.process_watermark((1 << 63) - 1)
        assert int(fired["count_star"].sum()) == 4 * n - total   # the ingest went on discarding exactly them
    finally:
        op.close()


# ---- (d) accumulation ----------------------------------------------------------------------------

@pytest.mark.parametrize("host", [True, False], ids=["host", "device_output"])
def test_three_batches_one_collect(host):
    """the columns sized for the first, small batch grow under the third; their content survives"""
    window = ("tumble", 1000)
    op = make_op(window, val_type="f64", late_output=True)
    try:
        op.process_batch(np.array([1], dtype=np.int64), np.array([T0 + 5], dtype=np.int64), np.array([1.0]))
        op.process_watermark(T0 + 999)
        exp = {k: [] for k in ("key", "rowtime", "val", "val_null")}
        for b, n in enumerate((64, 700, 9000)):
            i = np.arange(n, dtype=np.int64)
            late = (i + b) % 3 != 0
            key = (i * 31 + b) % KEYS
            ts = np.where(late, T0 + (i * 37) % 1000, T0 + 1000 + (i * 41) % 2000).astype(np.int64)
            val = (i * 5 + b).astype(np.float64) / 1024.0
            isnull = ((i % 11) == 0).astype(np.uint8) if b == 1 else None   # (one batch with NULL flags)
            op.process_batch(key, ts, val, isnull)
            assert np.array_equal(dropped_mask(ts, T0 + 999, window), late)
            exp["key"].append(key[late])
            exp["rowtime"].append(ts[late])
            exp["val"].append(val[late])
            exp["val_null"].append(np.zeros(int(late.sum()), dtype=np.uint8) if isnull is None else isnull[late])
        got = op.collect_late(host=host)
        if not host:
            got = {k: v.cpu().numpy() for k, v in got.items()}
        for k, parts in exp.items():
            e = np.concatenate(parts)
            assert got[k].dtype == e.dtype and np.array_equal(bits(got[k]) if k == "val" else got[k],
                                                              bits(e) if k == "val" else e), k
        again = op.collect_late(host=host)
        assert len(again["key"]) == 0 and len(again["val"]) == 0
        assert op.num_late_records_dropped == 0
    finally:
        op.close()


# ---- (e) restore ---------------------------------------------------------------------------------

def test_restore_starts_without_late_elements():
    name = "hop3s1s_i64"
    c = CONFIGS[name]
    key, ts, val, isnull = stream_of(name)
    steps = list(batches_of(name, ts))
    src = make_op(c["window"], val_type="i64")
    off, on = make_op(c["window"], val_type="i64"), make_op(c["window"], val_type="i64", late_output=True)
    try:
        for lo, hi, wm in steps[:3]:
            src.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi], isnull[lo:hi])
            src.process_watermark(wm)
        src.prepare_snapshot_pre_barrier()
        img, timer_wm = src.snapshot_state()
        for op in (off, on):
            op.restore_state(img, timer_wm)
        # before any watermark the restored operator's progress is Long.MIN_VALUE: nothing is late,
        # although most of this batch lies behind the checkpoint's watermark
        lo, hi, wm = steps[3]
        b = (key[lo:hi], ts[lo:hi], val[lo:hi], isnull[lo:hi])
        assert dropped_mask(b[1], steps[2][2], c["window"]).mean() > 0.05
        for op in (off, on):
            op.process_batch(*b)
        assert len(on.collect_late()["key"]) == 0
        assert off.num_late_records_dropped == 0 and on.num_late_records_dropped == 0
        assert_same_rows(on.process_watermark(wm), off.process_watermark(wm), "first watermark")
        # ... and from the first watermark on the twins agree as they do without a restore
        lo, hi, wm2 = steps[4]
        b = (key[lo:hi], ts[lo:hi], val[lo:hi], isnull[lo:hi])
        for op in (off, on):
            op.process_batch(*b)
        mask = dropped_mask(b[1], wm, c["window"])
        assert 0 < mask.sum() < len(mask)
        assert_late(on.collect_late(), *b, mask, "after the restore")
        assert off.num_late_records_dropped == int(mask.sum()) and on.num_late_records_dropped == 0
        assert_same_rows(on.process_watermark(wm2), off.process_watermark(wm2), "second watermark")
        assert_same_image(on.snapshot_state(), off.snapshot_state(), "after the restore")
        # uncollected records are not state: a restore (and a reset) discards them
        lo, hi, _ = steps[5]
        on.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi], isnull[lo:hi])
        on.restore_state(img, timer_wm)
        assert len(on.collect_late()["key"]) == 0
        on.process_watermark(wm2)
        on.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi], isnull[lo:hi])
        on.reset()
        assert len(on.collect_late()["key"]) == 0
    finally:
        for op in (src, off, on):
            op.close()


# ---- (f) errors ----------------------------------------------------------------------------------

def works(op, t0=T0):
    """one window in and out"""
    op.process_batch(np.array([5, 5], dtype=np.int64), np.array([t0 + 1, t0 + 2], dtype=np.int64),
                     np.array([2, 3], dtype=np.int64))
    r = op.process_watermark(t0 + 999)
    r = r[r["key"] == 5]
    assert len(r) == 1 and int(r["count_star"][0]) == 2 and int(r["sum"][0]) == 5


def test_errors():
    sql = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum"), val_type="i64", expected_keys=KEYS)
    local = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum"), val_type="i64", expected_keys=KEYS,
                                local_partials=True)
    ds = make_op(("tumble", 1000))
    try:
        for op in (sql, local):
            with pytest.raises(L.WindowSpecError, match="sideOutputLateData"):   # FG_EINVAL
                op.set_late_output(True)
            op.set_late_output(False)   # (off is the default: idempotent)
        works(sql)
        with pytest.raises(L.WindowSpecError):
            F.WindowAggOperator(F.tumbling(1000), aggs=("count_star",), val_type="none", late_output=True)
        with pytest.raises(L.FlinkGpuError, match="late output is off") as ei:
            ds.collect_late()
        assert ei.value.code == L.FG_ESTATE
        works(ds)
        ds.set_late_output(True)
        ds.set_late_output(True)
        late = (np.array([7, 8, 9], dtype=np.int64), np.array([T0 + 3, T0 + 2000, T0 + 4], dtype=np.int64),
                np.array([1, 2, 3], dtype=np.int64))
        ds.process_batch(*late)
        with pytest.raises(L.FlinkGpuError, match="not collected") as ei:
            ds.set_late_output(False)
        assert ei.value.code == L.FG_ESTATE
        got = ds.collect_late()
        assert got["key"].tolist() == [7, 9] and got["rowtime"].tolist() == [T0 + 3, T0 + 4]
        assert got["val"].tolist() == [1, 3] and got["val_null"].tolist() == [0, 0]
        ds.set_late_output(False)
        ds.process_batch(*late)   # counted again, not kept
        assert ds.num_late_records_dropped == 2
        with pytest.raises(L.FlinkGpuError):
            ds.collect_late()
        works(ds, T0 + 5000)
    finally:
        for op in (sql, local, ds):
            op.close()


# ---- kernel timing, DataStream operator ----------------------------------------------------------

def test_kernel_stats_class():
    op = make_op(("tumble", 1000), kernel_timing=True)
    try:
        before = list(op.kernel_stats())
        assert "late_out" not in before
        op.set_late_output(True)
        assert list(op.kernel_stats()) == before + ["late_out"]   # (no existing class moves)
        works(op)
        n = 3 * 4096 + 5
        i = np.arange(n, dtype=np.int64)
        ts = np.where(i % 4 == 0, T0 + 7, T0 + 1500).astype(np.int64)
        op.process_batch(i % KEYS, ts, i)
        assert len(op.collect_late()["key"]) == (n + 3) // 4
        st = op.kernel_stats()["late_out"]
        assert st["launches"] == 2 and st["records"] == 2 + n and st["rows"] == (n + 3) // 4
    finally:
        op.close()


def test_datastream_operator_late_records():
    from flink_amd.datastream import DataStreamWindowOperator
    op = DataStreamWindowOperator("tumble", 1000, val_type="f64", agg="count", api="aggregate", late_output=True,
                                  expected_keys=KEYS)
    try:
        op.process_batch(np.array([1], dtype=np.int64), np.array([T0 + 1], dtype=np.int64), np.array([0.5]))
        assert len(op.late_records()) == 0
        assert op.process_watermark(T0 + 999)["value"].tolist() == [1]
        op.process_batch(np.array([3, 4, 3], dtype=np.int64), np.array([T0 + 9, T0 + 1009, T0 + 8], dtype=np.int64),
                         np.array([1.5, 2.5, -0.0]))
        r = op.late_records()
        assert r["key"].tolist() == [3, 3] and r["timestamp"].tolist() == [T0 + 9, T0 + 8]
        assert r["value"].tolist() == bits(np.array([1.5, -0.0])).tolist()   # (COUNT: f1 still leaves as it came)
        assert op.late_dropped == 0
    finally:
        op.close()
