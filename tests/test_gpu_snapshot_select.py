"""Selective snapshot images (fg_snapshot_plan -> mask -> fg_snapshot_state_select[_async]): the
engine exports and copies only the slices the caller asks for, in one k_export_sel launch.

The reference of most checks is the full image (snapshot_state) taken on the same handle right after
the select: the state is the same, only the `changed` flags differ. The full image is a select of
every slice through the same kernel, so these comparisons check the mask, the compaction and the
bookkeeping, not the kernel; the kernel's rows are pinned against images built in numpy alone
(test_narrow_and_wide_tables_against_numpy here, assert_state_is in test_gpu_restore_range). Values are
BIGINT wherever bits are compared (and every (key, slice) is one row of an image, so DOUBLE bits of
one handle's two images are equal too). The end-to-end cases drive the shim's policy
(keyed_state.wanted_slices / write_delta) against write_image and write_image_full."""
import numpy as np
import pytest

from tests.streams import batches_with_watermarks, keys_in_one_region, make_stream
from tests.test_gpu_incremental_state import KIND
from tests.test_gpu_parity import assert_rows_equal, cfg_of, gpu_mk, oracle_mk
from tests.test_gpu_restore_range import MAXP, OPS, mk, synth
from tests.test_gpu_snapshot_grouped import assert_same_rows, mid_stream

pytestmark = pytest.mark.gpu
TWM = 1_600_000_000_000


def restrict(img, slice_ends):
    keep = np.isin(img["slice_end"], slice_ends)
    return {c: np.asarray(v)[keep] for c, v in img.items()}


def select_and_full(op, want_of, copy=True):
    """plan, select with want_of(plan slices), then the full image of the same state"""
    plan, wm_plan = op.snapshot_plan()
    want = np.asarray(want_of(plan), dtype=np.uint8)
    img, wm = op.snapshot_state_select(want, copy=copy)
    if not copy:
        alias = img["cnt_val"].ctypes.data == img["cnt_star"].ctypes.data
        img = {c: v.copy() for c, v in img.items()}
        img["_alias"] = alias
    sl = op.snapshot_slices()
    full, wm_full = op.snapshot_state()
    sl_full = op.snapshot_slices()
    assert wm == wm_plan == wm_full
    return plan, want, img, sl, full, sl_full


def check_select(plan, want, img, sl, full, sl_full, ctx=""):
    sel = want != 0
    img = {c: v for c, v in img.items() if c != "_alias"}
    # the plan is the full image's slice list
    for c in ("slice_end", "first_row", "rows"):
        assert np.array_equal(plan[c], sl_full[c]), (ctx, c)
    assert np.array_equal(plan["first_row"], np.cumsum(plan["rows"]) - plan["rows"]), ctx
    assert (np.diff(plan["slice_end"]) > 0).all(), ctx
    # the selective image's slices: the selected ones, compact, changed as planned
    assert np.array_equal(sl["slice_end"], plan["slice_end"][sel]), ctx
    assert np.array_equal(sl["rows"], plan["rows"][sel]), ctx
    assert np.array_equal(sl["first_row"], np.cumsum(sl["rows"]) - sl["rows"]), ctx
    assert np.array_equal(sl["changed"], plan["changed"][sel]), ctx
    assert (np.diff(sl["slice_end"]) > 0).all(), ctx
    n = len(img["key"])
    assert n == int(plan["rows"][sel].sum()), (ctx, n)
    assert np.array_equal(img["slice_end"], np.repeat(sl["slice_end"], sl["rows"])), f"{ctx}: rows not grouped by slice"
    # per slice the same multiset of rows as the full image holds
    assert set(img) == set(full), ctx
    assert_same_rows(restrict(full, sl["slice_end"]), img, ctx)
    # the select cleared the flags of the selected slices only
    assert np.array_equal(sl_full["changed"], plan["changed"] & ~sel), f"{ctx}: changed flags after the select"


# ---- 1, 2: masks ----------------------------------------------------------------------------------

def test_all_ones_mask_is_the_full_image():
    op = mid_stream("hop_i64_big")
    try:
        r = select_and_full(op, lambda p: np.ones(len(p["slice_end"])))
    finally:
        op.close()
    plan, want, img, sl, full, sl_full = r
    assert len(plan["slice_end"]) >= 3 and len(full["key"]) > 3000 and plan["changed"].all()
    check_select(*r, ctx="all ones")
    for c in ("slice_end", "first_row", "rows", "changed"):
        assert np.array_equal(sl[c], plan[c]), c
    assert np.array_equal(sl["first_row"], sl_full["first_row"])
    assert len(img["key"]) == len(full["key"])


def test_subset_mask_first_last_and_a_middle_slice():
    op = mid_stream("hop_i64_big")
    try:
        def want_of(p):
            n = len(p["slice_end"])
            assert n >= 5, p["slice_end"]   # first, a gap, a middle one, a gap, last
            w = np.zeros(n, dtype=np.uint8)
            w[[0, 2, n - 1]] = 1
            return w
        r = select_and_full(op, want_of)
    finally:
        op.close()
    plan, want, img, sl, full, _ = r
    check_select(*r, ctx="subset")
    assert len(sl["slice_end"]) == 3 and 0 < len(img["key"]) < len(full["key"])
    assert len(img["key"]) == int(plan["rows"][want != 0].sum())


# ---- 3: table layouts in one launch ---------------------------------------------------------------

def narrow_and_wide_op():
    """in-order batches of 32-bit keys without NULLs flush from their tiles (tables with 16-B
    entries); then a batch with keys beyond 32 bits in later slices only (wide tables). Nothing fires
    (no watermark). Returns the open operator and the stream as it was fed."""
    import flink_amd as F
    n, keys = 120_000, 20_000
    key, ts, val, _ = make_stream(n, keys, "i64", rate_per_ms=30)   # in order, 4 s
    op = F.WindowAggOperator(F.hopping(3000, 1000), aggs=("count_star", "count", "sum", "avg", "sum0"), val_type="i64",
                             expected_keys=keys, kernel_timing=True)
    try:
        cut = int(np.searchsorted(ts, ts[0] - ts[0] % 1000 + 3000))   # (the stream starts on a slice boundary or after)
        assert 0 < cut < n
        for lo in range(0, cut, 30_000):
            hi = min(cut, lo + 30_000)
            op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        op.prepare_snapshot_pre_barrier()
        ks0 = op.kernel_stats()
        assert ks0["tile_flush"]["launches"] > 0, ks0   # the flush that leaves narrow tables
        k2 = key[cut:].copy()
        k2[::5] = k2[::5] * (1 << 33) + 7
        op.process_batch(k2, ts[cut:], val[cut:])
        op.prepare_snapshot_pre_barrier()
        ks1 = op.kernel_stats()
        assert ks1["tile_flush"]["launches"] == ks0["tile_flush"]["launches"], "the wide batch was tile-staged"
    except BaseException:
        op.close()
        raise
    return op, np.concatenate([key[:cut], k2]), ts, val


def test_narrow_tables_next_to_wide_ones():
    op, _, _, _ = narrow_and_wide_op()
    try:
        r = select_and_full(op, lambda p: np.ones(len(p["slice_end"])))
        check_select(*r, ctx="narrow + wide, all")
        assert len(r[0]["slice_end"]) >= 4 and (np.abs(r[2]["key"]) > (1 << 33)).any()
        r = select_and_full(op, lambda p: np.arange(len(p["slice_end"])) % 2 == 0)   # both layouts again
        check_select(*r, ctx="narrow + wide, every other")
    finally:
        op.close()


def test_narrow_and_wide_tables_against_numpy():
    """the images of narrow_and_wide_op's state against one built from its stream in numpy alone: a
    row per (key, slice), cnt_star = cnt_val = the records (no NULLs), sum their int64 sum. The full
    image, the all-ones select and the every-other-slice select."""
    op, key, ts, val = narrow_and_wide_op()
    try:
        full, _ = op.snapshot_state()
        plan, _ = op.snapshot_plan()
        assert len(plan["slice_end"]) == 4, plan["slice_end"]
        ones, _ = op.snapshot_state_select(np.ones(4, dtype=np.uint8))
        op.snapshot_plan()
        other, _ = op.snapshot_state_select(np.array([1, 0, 1, 0], dtype=np.uint8))
        other_sl = op.snapshot_slices()
    finally:
        op.close()
    assert (np.diff(ts) >= 0).all()   # in order: nothing is late
    se = (ts // 1000 + 1) * 1000
    order = np.lexsort((key, se))
    k, s, v = key[order], se[order], val[order]
    first = np.flatnonzero(np.r_[True, (k[1:] != k[:-1]) | (s[1:] != s[:-1])])
    cnt = np.diff(np.r_[first, len(k)]).astype(np.int64)
    want = {"key": k[first], "slice_end": s[first], "cnt_star": cnt, "cnt_val": cnt, "sum": np.add.reduceat(v, first)}
    ends = np.unique(se)
    assert len(ends) == 4 and len(first) == 65_893 and int((np.abs(want["key"]) > (1 << 33)).sum()) == 5_167
    assert_same_rows(want, full, "full image vs numpy")
    assert_same_rows(want, ones, "all-ones select vs numpy")
    assert np.array_equal(other_sl["slice_end"], ends[::2])
    assert_same_rows(restrict(want, ends[::2]), other, "every-other-slice select vs numpy")


def test_min_max_columns_and_null_counts():
    """("count_star", "sum", "min", "max") over a stream with NULL values: the v1 / v2 columns, and a
    cnt_val column of its own"""
    op = mid_stream("multi_value_i64")
    try:
        r = select_and_full(op, lambda p: np.arange(len(p["slice_end"])) != 1, copy=False)
    finally:
        op.close()
    plan, want, img, sl, full, _ = r
    check_select(*r, ctx="mv nulls")
    assert "min" in img and "max" in img and len(img["key"]) > 1000
    assert not img["_alias"] and (img["cnt_val"] < img["cnt_star"]).any()
    has = img["cnt_val"] > 0
    assert (img["min"][has] <= img["max"][has]).all()


def test_without_nulls_cnt_val_is_cnt_star():
    op = mid_stream("hop_i64_big")
    try:
        r = select_and_full(op, lambda p: np.arange(len(p["slice_end"])) >= 1, copy=False)
    finally:
        op.close()
    check_select(*r, ctx="no nulls")
    img = r[2]
    assert img["_alias"] and np.array_equal(img["cnt_val"], img["cnt_star"])


def test_regions_split_before_the_snapshot():
    """an operator opened for 8 keys (one region of 3,584 entries) takes 20,000: its regions split"""
    spec = OPS["hop_i64_big"]
    key, ts, val, _ = make_stream(120_000, 20_000, spec["vt"], jitter_ms=300, rate_per_ms=30, **spec["gen"])
    op = mk(spec, expected_keys=8)
    try:
        at_open = op.stats()["state_regions"]
        for lo, hi, wm in batches_with_watermarks(120_000, 30_000, ts, 1500):
            op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            op.process_watermark(wm)
        r = select_and_full(op, lambda p: np.arange(len(p["slice_end"])) % 2 == 1)
        assert op.stats()["state_regions"] > at_open
    finally:
        op.close()
    check_select(*r, ctx="split regions")
    assert len(r[0]["slice_end"]) >= 3 and len(r[2]["key"]) > 2 * 3584


def test_a_region_with_more_than_256_entries_and_empty_regions():
    """700 keys of one region (its workgroup strides 3 times over them), every other region empty;
    a second slice of ordinary keys"""
    s0 = TWM + 1000
    parts = [synth(keys_in_one_region(700), s0), synth(np.arange(300), s0 + 1000)]
    image = {c: np.concatenate([p[c] for p in parts]) for c in parts[0]}
    op = mk(OPS["tumble_f64"])
    try:
        op.restore_state(image, TWM)
        assert op.stats()["state_regions"] > 1
        r = select_and_full(op, lambda p: [1, 0])
        check_select(*r, ctx="one region")
        assert not r[0]["changed"].any()   # restored into an empty handle: the backend holds them
        assert_same_rows(restrict(image, [s0]), {c: v for c, v in r[2].items()}, "one region vs the restored image")
        r = select_and_full(op, lambda p: [1, 1])
        check_select(*r, ctx="one region + ordinary")
        assert_same_rows(image, r[2], "both slices vs the restored image")
    finally:
        op.close()


# ---- 4: changed bookkeeping -----------------------------------------------------------------------

def test_changed_flags_follow_the_mask():
    spec = OPS["hop_i64_big"]
    key, ts, val, _ = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])
    steps = list(batches_with_watermarks(60000, 10000, ts, 1500))
    op = mk(spec)
    try:
        for lo, hi, wm in steps[:4]:
            op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            op.process_watermark(wm)
        plan, _ = op.snapshot_plan()
        again, _ = op.snapshot_plan()
        for c in plan:   # a plan clears nothing
            assert np.array_equal(plan[c], again[c]), c
        n = len(plan["slice_end"])
        assert n >= 4 and plan["changed"].all()
        want = np.ones(n, dtype=np.uint8)
        want[1] = 0
        op.snapshot_state_select(want)
        plan2, _ = op.snapshot_plan()
        assert np.array_equal(plan2["slice_end"], plan["slice_end"])
        assert plan2["changed"].tolist() == [i == 1 for i in range(n)]   # left out: changed again
        # nothing selected: nothing cleared
        img0, _ = op.snapshot_state_select(np.zeros(n, dtype=np.uint8))
        assert len(img0["key"]) == 0
        assert op.snapshot_plan()[0]["changed"].tolist() == plan2["changed"].tolist()
        # written again: the slices the next batch touches are changed, the others stay unchanged
        lo, hi, wm = steps[4]
        op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        plan3, _ = op.snapshot_plan()
        touched = np.isin(plan3["slice_end"], np.unique((ts[lo:hi] // 1000 + 1) * 1000))
        old = np.isin(plan3["slice_end"], plan["slice_end"])
        assert touched.any() and (plan3["changed"][touched]).all()
        quiet = old & ~touched & (plan3["slice_end"] != plan["slice_end"][1])
        assert quiet.any() and not plan3["changed"][quiet].any()
        assert plan3["changed"][plan3["slice_end"] == plan["slice_end"][1]].all()
    finally:
        op.close()


# ---- 5: grouping ----------------------------------------------------------------------------------

def test_grouped_selective_image():
    from flink_amd import _lib as L, key_groups
    op = mid_stream("multi_value_i64")
    try:
        op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
        plan, _ = op.snapshot_plan()
        S = len(plan["slice_end"])
        assert S >= 3
        want = np.ones(S, dtype=np.uint8)
        want[1] = 0
        img, _ = op.snapshot_state_select(want)
        sl, idx = op.snapshot_slices(), op.snapshot_key_groups()
        full, _ = op.snapshot_state()
    finally:
        op.close()
    n = len(img["key"])
    first = idx["first_row"]
    assert idx["n_slices"] == S - 1 == len(sl["slice_end"]) and idx["max_parallelism"] == MAXP
    assert len(first) == (S - 1) * MAXP + 1 and first[-1] == n == int(plan["rows"][want != 0].sum())
    assert np.array_equal(first[:-1:MAXP], sl["first_row"])
    assert (np.diff(first) >= 0).all()
    kg = key_groups(img["key"], MAXP, L.KEYHASH_BINARYROW_BIGINT)
    expect = np.repeat(np.tile(np.arange(MAXP), S - 1), np.diff(first))
    assert np.array_equal(kg, expect), "a row lies outside its (slice, key group) run"
    assert np.array_equal(img["slice_end"], np.repeat(sl["slice_end"], sl["rows"]))
    assert_same_rows(restrict(full, sl["slice_end"]), img, "grouped")


# ---- 6: async -------------------------------------------------------------------------------------

def test_async_select_is_the_state_at_the_call():
    spec = OPS["hop_i64_big"]
    key, ts, val, _ = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])
    steps = list(batches_with_watermarks(60000, 10000, ts, 1500))
    a, b = mk(spec), mk(spec)
    try:
        for op in (a, b):
            for lo, hi, wm in steps[:4]:
                op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
                op.process_watermark(wm)
        plan_a, wm_a = a.snapshot_plan()
        want = (np.arange(len(plan_a["slice_end"])) % 2 == 0).astype(np.uint8)
        a.snapshot_state_select_async(want)
        fired = 0
        for lo, hi, wm in steps[4:6]:
            a.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            fired += len(a.process_watermark(wm))
        assert fired > 0
        img_a, wm_a2 = a.snapshot_state_wait()
        sl_a = a.snapshot_slices()
        plan_b, wm_b = b.snapshot_plan()
        img_b, wm_b2 = b.snapshot_state_select(want)
        sl_b = b.snapshot_slices()
        assert wm_a == wm_a2 == wm_b == wm_b2 and len(img_b["key"]) > 1000
        for c in plan_a:
            assert np.array_equal(plan_a[c], plan_b[c]) and np.array_equal(sl_a[c], sl_b[c]), c
        assert_same_rows(img_b, img_a, "async")
        # the operator went on: its next full image holds the later state
        later, _ = a.snapshot_state()
        assert later["slice_end"].max() > img_a["slice_end"].max()
    finally:
        a.close()
        b.close()


# ---- 7: order and arguments -----------------------------------------------------------------------

def test_order_and_arguments():
    from flink_amd import _lib as L
    spec = OPS["hop_i64_big"]
    key, ts, val, _ = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])
    steps = list(batches_with_watermarks(60000, 10000, ts, 1500))
    op = mk(spec)

    def estate(fn, *a):
        with pytest.raises(L.FlinkGpuError) as e:
            fn(*a)
        assert e.value.code == L.FG_ESTATE, e.value

    def still_fine(ctx):
        r = select_and_full(op, lambda p: np.arange(len(p["slice_end"])) % 2 == 0)
        check_select(*r, ctx=ctx)
        return r[0]

    try:
        # a fresh handle: nothing resident, an empty image
        plan, wm = op.snapshot_plan()
        assert len(plan["slice_end"]) == 0 and wm == -(1 << 63)
        img, _ = op.snapshot_state_select(None)
        assert len(img["key"]) == 0 and len(op.snapshot_slices()["slice_end"]) == 0
        estate(op.snapshot_state_select, None)          # the select consumed the plan
        for lo, hi, wm in steps[:3]:
            op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            op.process_watermark(wm)
        n = len(op.snapshot_plan()[0]["slice_end"])
        assert n >= 3
        ones = np.ones(n, dtype=np.uint8)
        # a batch, a watermark, a full snapshot between plan and select
        lo, hi, wm = steps[3]
        op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        estate(op.snapshot_state_select, ones)
        still_fine("after plan -> batch -> select")
        n = len(op.snapshot_plan()[0]["slice_end"])
        op.process_watermark(wm)
        estate(op.snapshot_state_select, np.ones(n, dtype=np.uint8))
        still_fine("after plan -> watermark -> select")
        op.snapshot_plan()
        op.snapshot_state()
        estate(op.snapshot_state_select, np.ones(n, dtype=np.uint8))
        # calls that keep the plan valid
        plan, _ = op.snapshot_plan()
        n = len(plan["slice_end"])
        op.stats(), op.num_late_records_dropped, op.kernel_stats(), op.synchronize(), op.stream
        # a wrong n: FG_EINVAL, and the plan is still there
        with pytest.raises(L.WindowSpecError):
            op.snapshot_state_select(np.ones(n + 1, dtype=np.uint8))
        with pytest.raises(L.WindowSpecError):
            op.snapshot_state_select(np.ones(n - 1, dtype=np.uint8))
        img, _ = op.snapshot_state_select(np.ones(n, dtype=np.uint8))
        assert len(img["key"]) == int(plan["rows"].sum())
        # while a snapshot is uncollected: no plan, no select, no second snapshot
        plan, _ = op.snapshot_plan()
        op.snapshot_state_select_async(np.ones(n, dtype=np.uint8))
        estate(op.snapshot_plan)
        estate(op.snapshot_state_select_async, np.ones(n, dtype=np.uint8))
        estate(op.snapshot_state_async)
        img, _ = op.snapshot_state_wait()
        assert len(img["key"]) == int(plan["rows"].sum())
        op.snapshot_state_async()
        estate(op.snapshot_plan)
        op.snapshot_state_wait()
        plan = still_fine("after the errors")
        # an all-zero mask
        op.snapshot_plan()
        img, _ = op.snapshot_state_select(np.zeros(len(plan["slice_end"]), dtype=np.uint8))
        assert len(img["key"]) == 0 and len(op.snapshot_slices()["slice_end"]) == 0
        still_fine("after the empty image")
    finally:
        op.close()


# ---- 8: one launch --------------------------------------------------------------------------------

def test_a_select_is_one_launch():
    op = mid_stream("hop_i64_big", kernel_timing=True)
    try:
        plan, _ = op.snapshot_plan()
        n = len(plan["slice_end"])
        assert n >= 4
        want = np.ones(n, dtype=np.uint8)
        want[1] = 0
        op.synchronize()
        before = op.kernel_stats()
        img, _ = op.snapshot_state_select(want)
        op.synchronize()
        after = op.kernel_stats()
        assert list(after)[-2:] == ["export_group", "export_select"]
        assert after["export_select"]["launches"] - before["export_select"]["launches"] == 1
        assert after["export"]["launches"] == before["export"]["launches"]
        assert after["export_select"]["records"] - before["export_select"]["records"] == len(img["key"]) > 0
        whole, _ = op.snapshot_state()
        op.synchronize()
        full = op.kernel_stats()
        assert full["export"]["launches"] - after["export"]["launches"] == 1   # the full image: one launch too
        assert full["export"]["records"] - after["export"]["records"] == len(whole["key"]) > len(img["key"])
        assert full["export_select"]["launches"] == after["export_select"]["launches"]
    finally:
        op.close()


def test_full_image_of_a_fresh_handle_and_of_changed_slices():
    """the full path's two ends: nothing resident (an empty image, no launch), and every slice changed
    (reported as the plan just before reports it, cleared by the image)"""
    op = mk(OPS["hop_i64_big"], kernel_timing=True)
    try:
        before = op.kernel_stats()
        img, _ = op.snapshot_state()
        op.synchronize()
        assert len(img["key"]) == 0 and len(op.snapshot_slices()["slice_end"]) == 0
        assert op.kernel_stats()["export"]["launches"] == before["export"]["launches"]
    finally:
        op.close()
    spec = OPS["hop_i64_big"]
    key, ts, val, _ = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])   # mid_stream's
    op = mk(spec)
    try:
        for lo, hi, wm in list(batches_with_watermarks(60000, 10000, ts, 1500))[:3]:
            op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            op.process_watermark(wm)
        plan, _ = op.snapshot_plan()
        first, _ = op.snapshot_state()
        sl = op.snapshot_slices()
        assert len(plan["slice_end"]) >= 3 and plan["changed"].all()
        for c in ("slice_end", "first_row", "rows", "changed"):
            assert np.array_equal(sl[c], plan[c]), c
        again, _ = op.snapshot_plan()
        assert np.array_equal(again["slice_end"], plan["slice_end"]) and not again["changed"].any()
        second, _ = op.snapshot_state()
        assert len(second["key"]) == int(plan["rows"].sum()) > 0
        assert_same_rows(first, second, "a second full image")
        assert not op.snapshot_slices()["changed"].any()
    finally:
        op.close()


# ---- 9: end to end with the shim's policy ---------------------------------------------------------

E2E = [
    # (name, cfg, stream, checkpoint steps, restore)
    ("tumble_zipf", cfg_of("tumble", 1000),
     dict(n=300_000, keys=20_000, batch=15_000, rate_per_ms=75, delay=400, jitter=600, zipf=1.1), (3, 4, 9, 14), True),
    ("hop", cfg_of("hop", 3000, 1000),
     dict(n=300_000, keys=20_000, batch=15_000, rate_per_ms=50, delay=300, jitter=500), (4, 5, 11), False),
    ("cumulate", cfg_of("cumulate", 4000, 1000),
     dict(n=300_000, keys=20_000, batch=15_000, rate_per_ms=50, delay=300, jitter=500), (4, 5, 11, 16), False),
]


@pytest.mark.parametrize("name,cfg,kw,ckpts,restore", E2E, ids=[c[0] for c in E2E])
def test_selective_checkpoints_equal_full_rewrite(oracle_mod, name, cfg, kw, ckpts, restore):
    from flink_amd.keyed_state import SliceSpec, WindowAggsState
    O = oracle_mod
    kw = dict(kw)
    n, keys, batch, delay, jitter = kw.pop("n"), kw.pop("keys"), kw.pop("batch"), kw.pop("delay"), kw.pop("jitter")
    key, ts, val, _ = make_stream(n, keys, cfg["val_type"], jitter_ms=jitter, **kw)
    spec = SliceSpec(KIND[cfg["kind"]], cfg["size"], cfg["slide"])
    delta, inc, full = WindowAggsState(spec), WindowAggsState(spec), WindowAggsState(spec)
    g = gpu_mk(cfg, expected_keys=keys, buffer_records=max(4 * batch, 1 << 16))
    o = oracle_mk(O, cfg)
    sizes = []
    for step, (lo, hi, wm) in enumerate(batches_with_watermarks(n, batch, ts, delay)):
        g.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        o.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        g.process_watermark(wm)
        o.process_watermark(wm)
        assert_rows_equal(g.take_rows(), o.take_rows(), cfg["val_type"], f"{name} step {step}", sums=True)
        if step not in ckpts:
            continue
        g.prepare_snapshot()
        o.prepare_snapshot()
        plan, twm = g.op.snapshot_plan()
        for b in (delta, inc, full):
            b.advance_watermark(twm)
        want = delta.wanted_slices(plan, twm)
        img, twm_s = g.op.snapshot_state_select(want)
        img_sl = g.op.snapshot_slices()
        assert twm_s == twm and len(img["key"]) == int(plan["rows"][want != 0].sum())
        delta.write_delta(img, img_sl, plan, twm)
        whole, twm_f = g.op.snapshot_state()
        sl = g.op.snapshot_slices()
        assert twm_f == twm
        for c in ("slice_end", "first_row", "rows"):
            assert np.array_equal(sl[c], plan[c]), (step, c)
        inc.write_image(whole, plan, twm)
        full.write_image_full(whole, sl, twm)
        sizes.append((len(img["key"]), len(whole["key"])))
        assert delta.entries == full.entries, f"{name} checkpoint at step {step}: entries differ"
        assert delta.timers == full.timers, f"{name} checkpoint at step {step}: timers differ"
        assert inc.entries == full.entries and inc.timers == full.timers, (name, step)
        if restore and step == max(ckpts):
            break   # (a failover right after the last checkpoint)
    assert sizes[0][0] == sizes[0][1] > 0   # a handle's first image: everything
    if cfg["kind"] == "hop":   # one micro-batch later: the older slices of the open windows stay on the GPU
        assert sizes[1][0] < sizes[1][1], sizes
    if not restore:
        g.close()
        o.close()
        return
    # failover after the last checkpoint: the new operator restores from the backend
    cols, twm = delta.image()
    cols = {k: v for k, v in cols.items() if k not in ("min", "max")}   # (one value accumulator)
    g2 = gpu_mk(cfg, expected_keys=keys, buffer_records=max(4 * batch, 1 << 16))
    g2.op.restore_state(cols, twm)
    o2 = o.restore_copy()
    g_base, o_base = g.late_dropped, o.late_dropped
    g.close()
    o.close()
    last = max(ckpts)
    for step, (lo, hi, wm) in enumerate(batches_with_watermarks(n, batch, ts, delay)):
        if step <= last:
            continue
        g2.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        o2.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        g2.process_watermark(wm)
        o2.process_watermark(wm)
        assert_rows_equal(g2.take_rows(), o2.take_rows(), cfg["val_type"], f"{name} restored step {step}", sums=True)
    g2.process_watermark((1 << 63) - 1)
    o2.process_watermark((1 << 63) - 1)
    assert_rows_equal(g2.take_rows(), o2.take_rows(), cfg["val_type"], f"{name} final", sums=True)
    assert g_base + g2.late_dropped == o_base + o2.late_dropped
    g2.close()
    o2.close()
