"""fg_fired_packed on the GPU: the fired rows as packed BinaryRowData rows.

The reference is never the pack kernel: it is the columnar output of the same returning call (FG_HOST
columns, the path the oracle parity tests check), packed on the CPU by flink_amd.rows.pack_rows, whose
layout tests/test_abi.py::test_binary_row_layout pins. After that call fired_packed() on the same handle
must give the same bytes; every comparison is exact, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from flink_amd import rows as R
from flink_amd.keys import KeyDictionary, key_row
from flink_amd.window_agg import AGG_NAMES

pytestmark = pytest.mark.gpu

JMAX = (1 << 63) - 1
T0 = 1_600_000_000_000
SIX = ("count_star", "count", "sum", "avg", "min", "max")
# what fg_kernel_stats lists for a handle that never had the late output or the Top-N selection on
PARENT_CLASSES = ["ingest_count", "ingest_scan", "ingest_scatter", "ingest_part1", "ingest_part2", "merge_flush",
                  "merge_flush_fire", "merge_fire", "export", "restore", "merge_heavy", "tile_part1", "tile_fire",
                  "tile_materialize", "tile_flush", "tile_split_fire", "restore_filter", "restore_scatter",
                  "export_group", "export_select"]


# ---- the reference ------------------------------------------------------------------------------------

def packed_reference(op, rows, key_field):
    """pack_rows over the structured rows a returning call gave: [key,] aggregates, window_start, window_end"""
    fields, nulls = ([rows["key"]], [None]) if key_field else ([], [])
    for a in op.aggs:
        fields.append(rows[AGG_NAMES[a]])
        nulls.append(rows[AGG_NAMES[a] + "_null"])
    fields += [rows["window_start"], rows["window_end"]]
    nulls += [None, None]
    return R.pack_rows(fields, nulls)


def assert_packed(op, rows, p, key_field, lo=0, hi=None, ctx=""):
    hi = len(rows) if hi is None else hi
    arity = len(op.aggs) + 2 + (1 if key_field else 0)
    assert (p["n"], p["arity"], p["stride"]) == (hi - lo, arity, 8 * (arity + 1)), ctx
    exp = packed_reference(op, rows[lo:hi], key_field)
    assert p["rows"].dtype == np.uint8 and p["rows"].shape == exp.shape, ctx
    bad = np.flatnonzero(p["rows"] != exp)
    assert len(bad) == 0, f"{ctx}: {len(bad)} bytes differ, first in row {bad[0] // p['stride']} at byte {bad[0] % p['stride']}"
    if key_field:
        assert p["key"] is None, ctx
    else:
        assert p["key"].dtype == np.int64 and (p["key"] == rows["key"][lo:hi]).all(), ctx


def check_both_layouts(op, rows, ctx=""):
    for kf in (False, True):
        assert_packed(op, rows, op.fired_packed(key_field=kf), kf, ctx=f"{ctx} key_field={kf}")


def estate(fn):
    with pytest.raises(F.FlinkGpuError) as ei:
        fn()
    assert ei.value.code == L.FG_ESTATE
    return ei.value.msg


# ---- the streams --------------------------------------------------------------------------------------

def null_stream():
    """3,000 records of 700 keys over two 1-s windows; every record of 50 keys carries a NULL value"""
    rng = np.random.default_rng(0)
    n = 3000
    k = rng.integers(0, 700, n)
    key = k.astype(np.int64) * 7919 - 1000
    ts = T0 + np.arange(n, dtype=np.int64) * 2000 // n
    val = rng.integers(-1_000_000, 1_000_000, n).astype(np.int64)
    return key, ts, val, (k < 50).astype(np.uint8)


def hop_stream():
    """2,500 records of 300 keys over 3.5 s"""
    rng = np.random.default_rng(5)
    n = 2500
    key = rng.integers(-150, 150, n).astype(np.int64)
    ts = T0 + np.arange(n, dtype=np.int64) * 3500 // n
    val = rng.integers(-1000, 1000, n).astype(np.int64)
    return key, ts, val


def null_op(**kw):
    op = F.WindowAggOperator(F.tumbling(1000), aggs=SIX, val_type="i64", expected_keys=700, **kw)
    op.process_batch(*null_stream())
    return op


def hop_op(**kw):
    op = F.WindowAggOperator(F.hopping(4000, 1000), aggs=("count_star", "sum", "max"), val_type="i64", expected_keys=300, **kw)
    op.process_batch(*hop_stream())
    return op


@pytest.fixture(scope="module")
def fired_null():
    """(operator, the rows of its one returning call): shared by the tests that only pack"""
    op = null_op()
    rows = op.process_watermark(JMAX)
    yield op, rows
    op.close()


@pytest.fixture(scope="module")
def fired_hop_runs():
    op = hop_op(fired_runs=True)
    rows = op.process_watermark(JMAX)
    yield op, rows
    op.close()


# ---- 1. NULLs and both layouts -----------------------------------------------------------------------

def test_nulls_and_both_layouts(fired_null):
    op, rows = fired_null
    n = len(rows)
    assert len(np.unique(rows["window_end"])) == 2
    assert rows["sum_null"].any() and not rows["sum_null"].all()
    for a in ("sum", "avg", "min", "max"):
        assert (rows[a + "_null"] == rows["sum_null"]).all()
    assert not rows["count_star_null"].any() and not rows["count_null"].any()
    assert (rows["count"][rows["sum_null"]] == 0).all() and (rows["count_star"] > 0).all()
    assert n % 64 != 0 and n % 9 != 0 and n % 10 != 0 and n * 9 > 4 * 256   # (W = 9 and 10; several workgroups)
    check_both_layouts(op, rows, "tumble nulls")
    # what a reader gets back: NULL aggregates as zero bytes with their bit set, RowKind INSERT
    f, nl, kind = R.unpack_rows(op.fired_packed(key_field=True)["rows"], 9)
    assert (kind == 0).all() and (f[0] == rows["key"]).all() and not nl[0].any()
    assert (nl[3] == rows["sum_null"]).all() and (f[3][nl[3]] == 0).all() and (f[3][~nl[3]] == rows["sum"][~nl[3]]).all()
    assert (f[7] == rows["window_start"]).all() and (f[8] == rows["window_end"]).all()


# ---- 2. DOUBLE bits -----------------------------------------------------------------------------------

def test_double_bits_survive():
    specials = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1.5, -2.25e-300, 1.7976931348623157e308])
    nan_payload = np.array([0x7FF8000000000123, -0x0007FFFFFFFFFEDD], dtype=np.int64).view(np.float64)   # quiet NaNs
    vals = np.concatenate([specials, nan_payload])
    n = 203   # one value per key, one window
    key = np.arange(n, dtype=np.int64) - 100
    val = vals[np.arange(n) % len(vals)]
    ts = T0 + np.arange(n, dtype=np.int64)
    op = F.WindowAggOperator(F.tumbling(1000), aggs=("sum", "min", "max", "count"), val_type="f64", expected_keys=n)
    op.process_batch(key, ts, val)
    rows = op.process_watermark(JMAX)
    assert len(rows) == n
    # the reference holds the values whose bits matter: -0.0, both infinities, NaNs
    every = np.concatenate([rows["sum"], rows["min"], rows["max"]])
    bits = set(every.view(np.int64).tolist())
    assert {np.float64(-0.0).view(np.int64).item(), np.float64(np.inf).view(np.int64).item(),
            np.float64(-np.inf).view(np.int64).item()} <= bits and np.isnan(every).any()
    check_both_layouts(op, rows, "double bits")
    op.close()


# ---- 3. run mode --------------------------------------------------------------------------------------

def test_run_mode(fired_hop_runs):
    op, rows = fired_hop_runs
    runs = op.fired_runs()
    assert len(runs["rows"]) >= 4 and len(np.unique(rows["window_end"])) >= 4
    ws, we, _ = F.window_agg.expand_runs(runs, len(rows))
    assert (ws == rows["window_start"]).all() and (we == rows["window_end"]).all()
    check_both_layouts(op, rows, "hop runs")


def test_same_stream_with_run_mode_off(fired_hop_runs):
    op = hop_op()
    rows = op.process_watermark(JMAX)
    assert len(np.unique(rows["window_end"])) >= 4
    check_both_layouts(op, rows, "hop columns")
    # the two modes pack the same rows (as sets: the order of a fire's rows is the kernel's)
    a, b = op.fired_packed(key_field=True), fired_hop_runs[0].fired_packed(key_field=True)
    assert a["stride"] == b["stride"] == 56 and a["n"] == b["n"] == len(rows)
    assert sorted(map(bytes, a["rows"].reshape(-1, 56))) == sorted(map(bytes, b["rows"].reshape(-1, 56)))
    op.close()


# ---- 4. Top-N -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("runs", [False, True], ids=["columns", "runs"])
def test_topn_packs_the_selected_rows(fired_null, runs):
    op = null_op(topn=(3, "sum", True), fired_runs=runs)
    rows = op.process_watermark(JMAX)
    assert len(rows) == 6 and len(rows) < len(fired_null[1])
    assert (np.diff(rows["sum"][:3]) <= 0).all() and (np.diff(rows["sum"][3:]) <= 0).all()   # in rank order
    check_both_layouts(op, rows, "topn")
    op.close()


# ---- 5. ranges ----------------------------------------------------------------------------------------

def test_ranges(fired_null, fired_hop_runs):
    op, rows = fired_null
    n = len(rows)
    for kf in (False, True):
        full = op.fired_packed(key_field=kf)
        part = op.fired_packed(first_row=5, max_rows=77, key_field=kf)
        assert_packed(op, rows, part, kf, 5, 82, "rows 5..81")
        assert (part["rows"] == full["rows"][5 * full["stride"]:82 * full["stride"]]).all()
        assert_packed(op, rows, op.fired_packed(first_row=n - 3, max_rows=1000, key_field=kf), kf, n - 3, n, "clipped")
        for a in (dict(max_rows=0), dict(first_row=n), dict(first_row=n, max_rows=0), dict(first_row=17, max_rows=0)):
            e = op.fired_packed(key_field=kf, **a)
            assert e["n"] == 0 and e["rows"].size == 0 and e["stride"] == full["stride"], a
    # chunks, as a shim pulls them: each call on its own
    got = np.concatenate([op.fired_packed(first_row=f, max_rows=500)["rows"] for f in range(0, n, 500)])
    assert (got == op.fired_packed()["rows"]).all()
    # refused, and the handle stays usable
    for a in (dict(first_row=n + 1), dict(first_row=-1), dict(max_rows=-1), dict(first_row=-5, max_rows=-5)):
        with pytest.raises(F.WindowSpecError):
            op.fired_packed(**a)
    out = L.FgPackedRows()
    for flags in (2, 3, -1):
        assert L.load().fg_fired_packed(op._h, 0, 10, flags, L.HOST, C.byref(out)) == L.FG_EINVAL
        assert b"flag" in L.load().fg_last_error(op._h)
    assert L.load().fg_fired_packed(op._h, 0, 10, 0, 7, C.byref(out)) == L.FG_EINVAL
    assert L.load().fg_fired_packed(op._h, 0, 10, 0, L.HOST, None) == L.FG_EINVAL
    check_both_layouts(op, rows, "after the refusals")
    # run mode: a range across a run boundary
    rop, rrows = fired_hop_runs
    b = int(rop.fired_runs()["first_row"][2])
    assert rrows["window_end"][b - 1] != rrows["window_end"][b]
    for kf in (False, True):
        assert_packed(rop, rrows, rop.fired_packed(first_row=b - 3, max_rows=10, key_field=kf), kf, b - 3, b + 7, "across runs")
        assert_packed(rop, rrows, rop.fired_packed(first_row=b, max_rows=1, key_field=kf), kf, b, b + 1, "a run's first row")


# ---- 6. FG_DEVICE ---------------------------------------------------------------------------------------

def test_device_rows_equal_host_rows(fired_null, fired_hop_runs):
    for op, rows in (fired_null, fired_hop_runs):
        for kf in (False, True):
            d = op.fired_packed(first_row=3, max_rows=len(rows) - 10, key_field=kf, device=True)
            assert isinstance(d["rows"], int) and d["rows"] != 0 and (d["key"] is None) == kf
            h = op.packed_to_host(d)
            assert_packed(op, rows, h, kf, 3, len(rows) - 7, "device")
            assert (h["rows"] == op.fired_packed(first_row=3, max_rows=len(rows) - 10, key_field=kf)["rows"]).all()


# ---- 7. async -----------------------------------------------------------------------------------------

def test_async_advances_then_collect():
    op = null_op()
    assert op.process_watermark(T0 + 999, device_output=True, wait=False) is None
    assert op.process_watermark(T0 + 1999, device_output=True, wait=False) is None
    assert "fg_collect_fired" in estate(op.fired_packed)
    rows = op.collect_fired(host=True)
    assert len(np.unique(rows["window_end"])) == 2
    check_both_layouts(op, rows, "async")
    op.close()


# ---- 8. validity --------------------------------------------------------------------------------------

def test_validity_rule():
    op = hop_op(fired_runs=True)
    estate(op.fired_packed)                                    # no returning call yet
    assert len(op.process_watermark(T0 - 10_000)) == 0         # a returning call that fired nothing
    for kf in (False, True):
        e = op.fired_packed(key_field=kf)
        assert (e["n"], e["arity"], e["rows"].size) == (0, 5 + kf, 0)
    rows = op.process_watermark(T0 + 1999)
    assert len(rows) > 0
    op.fired_runs(), op.stats(), op.kernel_stats(), op.num_late_records_dropped, op.synchronize()
    check_both_layouts(op, rows, "after fired_runs and stats")   # (and a pack after a pack)
    key, ts, val = hop_stream()
    op.process_batch(key[-10:], ts[-10:], val[-10:])
    estate(op.fired_packed)                                    # the fired rows are no longer the call's
    rows = op.process_watermark(T0 + 2999)
    check_both_layouts(op, rows, "the next fire")
    op.set_fired_runs(False)
    estate(op.fired_packed)
    op.reset()
    estate(op.fired_packed)
    op.close()


# ---- 9. refusals --------------------------------------------------------------------------------------

def test_datastream_and_local_handles_are_refused():
    ds = F.WindowAggOperator(F.tumbling(1000), mode="datastream", aggs=("count_star", "sum"), val_type="i64")
    with pytest.raises(F.WindowSpecError, match="FG_MODE_DATASTREAM.*tuples"):
        ds.fired_packed()
    ds.process_batch(np.arange(5, dtype=np.int64), T0 + np.arange(5, dtype=np.int64), np.arange(5, dtype=np.int64))
    assert len(ds.process_watermark(T0 + 5000)) == 5
    with pytest.raises(F.WindowSpecError, match="FG_MODE_DATASTREAM"):
        ds.fired_packed(key_field=True)
    ds.close()
    lo = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum"), val_type="i64", local_partials=True)
    with pytest.raises(F.WindowSpecError, match="FG_FLAG_LOCAL_PARTIALS.*accumulator rows"):
        lo.fired_packed()
    lo.close()


# ---- 10. dictionary keys ------------------------------------------------------------------------------

def test_dictionary_ids():
    d = KeyDictionary(max_parallelism=128, expected_keys=64)
    names = [f"user-{i % 41:04d}-{'x' * (i % 3)}" for i in range(600)]
    ids, _ = d.intern(rows=[key_row([s], ["string"]) for s in names])
    ts = T0 + np.arange(600, dtype=np.int64) * 3
    val = np.arange(600, dtype=np.int64) - 300
    op = F.WindowAggOperator(F.tumbling(1000), aggs=("count_star", "sum"), val_type="i64", expected_keys=64)
    op.process_batch(ids, ts, val)
    rows = op.process_watermark(JMAX)
    pairs = {(int(i), int(t - T0) // 1000) for i, t in zip(ids, ts)}
    assert set(rows["key"].tolist()) == set(ids.tolist()) and len(rows) == len(pairs) == 2 * len(set(names))
    check_both_layouts(op, rows, "dictionary ids")
    assert (op.fired_packed()["key"] == rows["key"]).all()                      # the id column of the call
    f, nl, _ = R.unpack_rows(op.fired_packed(key_field=True)["rows"], 5)
    assert (f[0] == rows["key"]).all() and not nl[0].any()                      # field 0 is the id
    assert len(d.rows(op.fired_packed()["key"])[2]) == len(rows)                # (the key rows: fg_key_dict_rows)
    op.close()
    d.close()


# ---- 11. statistics -----------------------------------------------------------------------------------

def test_kernel_statistics():
    op, other = null_op(kernel_timing=True), null_op(kernel_timing=True)
    rows = op.process_watermark(JMAX)
    n = len(other.process_watermark(JMAX))
    assert n == len(rows)
    assert list(op.kernel_stats()) == PARENT_CLASSES                            # absent before the first pack
    assert op.fired_packed(max_rows=0)["n"] == 0 and op.fired_packed(first_row=n)["n"] == 0
    assert list(op.kernel_stats()) == PARENT_CLASSES                            # an n = 0 call packs nothing
    check_both_layouts(op, rows, "timed")                                       # two calls with rows
    assert op.fired_packed(first_row=5, max_rows=77)["n"] == 77                 # a third
    assert op.fired_packed(max_rows=0)["n"] == 0
    ks = op.kernel_stats()
    assert list(ks) == PARENT_CLASSES + ["pack_rows"]
    assert ks["pack_rows"]["launches"] == 3 and ks["pack_rows"]["records"] == ks["pack_rows"]["rows"] == 2 * n + 77
    assert ks["pack_rows"]["total_ms"] > 0
    assert list(other.kernel_stats()) == PARENT_CLASSES                         # a handle that never packs
    # after late_out and topn where those are listed; fg_set_kernel_timing's bit is the list's index
    tn = null_op(kernel_timing=True, topn=(3, "sum", True))
    trows = tn.process_watermark(JMAX)
    tn.set_kernel_timing(["topn"])
    assert tn.fired_packed()["n"] == len(trows)
    names = list(tn.kernel_stats())
    assert names == PARENT_CLASSES + ["topn", "pack_rows"]
    assert tn.kernel_stats()["pack_rows"]["launches"] == 0 and tn.kernel_stats()["pack_rows"]["rows"] == len(trows)
    tn.set_kernel_timing(["pack_rows"])
    tn.fired_packed()
    assert tn.kernel_stats()["pack_rows"]["launches"] == 1
    for o in (op, other, tn):
        o.close()
