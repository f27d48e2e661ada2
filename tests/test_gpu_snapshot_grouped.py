"""Key-grouped snapshot images (fg_set_snapshot_grouping / fg_snapshot_key_groups) and the restore
that reads only its own key groups (two_phase.keyed_part / restore_keyed).

A grouped image must be the plain image in another order: the same rows, the same slices, every
slice's rows ascending by key group, and an index that is the cumulative (slice, key group)
histogram. Every expected key group comes from the ORACLE (key_groups_binaryrow, key_group), never
from the code under test; every column is compared bit for bit."""
import numpy as np
import pytest

from tests.streams import batches_with_watermarks, make_stream, splitmix64
from tests.test_gpu_restore_range import (JMAX, MAXP, OPS, assert_same_state, concat, host_filter, image_of, mk,
                                          subtasks, synth, take)

pytestmark = pytest.mark.gpu
TWM = 1_600_000_000_000          # timer watermark of the synth images (their slice ends 1 s later)
SEGMENT = 16384                  # rows per workgroup of the partition kernels (kRrSegment)


def sorted_rows(img):
    order = np.lexsort((img["key"], img["slice_end"]))
    return {c: np.asarray(v)[order] for c, v in img.items()}


def assert_same_rows(a, b, ctx=""):
    a, b = sorted_rows(a), sorted_rows(b)
    assert set(a) == set(b), ctx
    for c in a:
        assert len(a[c]) == len(b[c]), f"{ctx}: {len(b[c])} rows vs {len(a[c])} expected"
        assert np.array_equal(a[c].view(np.int64), b[c].view(np.int64)), f"{ctx}: column {c} differs"


def assert_grouped(img, slices, index, maxp, kg, ctx=""):
    """the image's rows lie slice by slice as `slices` says, ascending by the oracle's key group
    `kg` inside every slice, and `index` is the cumulative (slice, key group) histogram"""
    n, S = len(img["key"]), len(slices["slice_end"])
    first = index["first_row"]
    assert index["n_slices"] == S and index["max_parallelism"] == maxp, (ctx, index["n_slices"], S)
    assert first.dtype == np.int64 and len(first) == S * maxp + 1, ctx
    assert first[0] == 0 and first[-1] == n, (ctx, first[-1], n)
    assert int(slices["rows"].sum()) == n, ctx
    assert np.array_equal(first[:-1:maxp], slices["first_row"]), ctx
    sidx = np.repeat(np.arange(S, dtype=np.int64), slices["rows"])
    assert np.array_equal(img["slice_end"], slices["slice_end"][sidx]), ctx
    bins = sidx * maxp + np.asarray(kg, dtype=np.int64)
    assert (np.diff(bins) >= 0).all(), f"{ctx}: key groups descend inside a slice"
    hist = np.bincount(bins, minlength=S * maxp)
    assert np.array_equal(first, np.concatenate(([0], np.cumsum(hist)))), f"{ctx}: first_row is not the histogram's scan"


def grouped_snapshot(op):
    img, wm = op.snapshot_state()
    return img, wm, op.snapshot_slices(), op.snapshot_key_groups()


def mid_stream(name, **kw):
    """the operator of image_of(name) at its cut, still open"""
    spec = OPS[name]
    key, ts, val, isnull = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])
    op = mk(spec, **kw)
    for lo, hi, wm in batches_with_watermarks(40000, 10000, ts, 1500):
        op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi], None if isnull is None else isnull[lo:hi])
        op.process_watermark(wm)
    op.prepare_snapshot_pre_barrier()
    return op


# ---- same state, new order ----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(OPS))
def test_grouped_image_is_the_plain_image_reordered(oracle_mod, name):
    from flink_amd import _lib as L
    op = mid_stream(name)
    try:
        plain, wm_p = op.snapshot_state()
        sl_p = op.snapshot_slices()
        with pytest.raises(L.FlinkGpuError):   # FG_ESTATE: that image was taken with grouping off
            op.snapshot_key_groups()
        op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
        img, wm, sl, idx = grouped_snapshot(op)
    finally:
        op.close()
    assert wm == wm_p and len(sl["slice_end"]) >= 3 and len(img["key"]) > 3000
    assert ("min" in img) == ("aggs" in OPS[name])
    assert_same_rows(plain, img, name)
    for c in ("slice_end", "first_row", "rows"):
        assert np.array_equal(sl[c], sl_p[c]), (name, c)
    assert sl_p["changed"].all() and not sl["changed"].any()   # the first image cleared it
    assert_grouped(img, sl, idx, MAXP, oracle_mod.key_groups_binaryrow(img["key"], MAXP), name)


# ---- edges ----------------------------------------------------------------------------------------

def restore_and_group(op, image, twm, maxp, kg_of, key_hash=None, ctx=""):
    from flink_amd import _lib as L
    op.reset()
    op.restore_state(image, twm)
    op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT if key_hash is None else key_hash)
    img, _, sl, idx = grouped_snapshot(op)
    assert_same_rows(image, img, ctx)
    assert_grouped(img, sl, idx, maxp, kg_of(img["key"]), ctx)
    return img, sl, idx


@pytest.mark.parametrize("maxp", [128, 100, 1, 8193, 32768])
def test_row_counts_and_key_group_counts_at_the_edges(oracle_mod, maxp):
    """one-slice images around the wave, workgroup and segment sizes; max_parallelism a power of
    two, not one, a single bin, and beyond one LDS window of 8192 key groups (most bins empty)"""
    op = mk(OPS["tumble_f64"], (0, maxp - 1), maxp=maxp)
    try:
        for n in (0, 1, 63, 64, 65, 257, SEGMENT - 1, SEGMENT + 1):
            _, sl, idx = restore_and_group(op, synth(np.arange(n)), TWM, maxp,
                                           lambda k: oracle_mod.key_groups_binaryrow(k, maxp), ctx=f"maxp {maxp} n {n}")
            if n == 0:
                assert idx["n_slices"] == 0 and idx["first_row"].tolist() == [0]
            else:
                assert idx["n_slices"] == 1 and np.count_nonzero(np.diff(idx["first_row"])) <= min(n, maxp)
    finally:
        op.close()


def test_one_hot_key_group(oracle_mod):
    keys = np.arange(200_000)
    keys = keys[oracle_mod.key_groups_binaryrow(keys, MAXP) == 5]
    assert len(keys) > 1000
    op = mk(OPS["tumble_f64"])
    try:
        _, _, idx = restore_and_group(op, synth(keys), TWM, MAXP, lambda k: oracle_mod.key_groups_binaryrow(k, MAXP),
                                      ctx="hot bin")
        assert np.diff(idx["first_row"]).tolist() == [0] * 5 + [len(keys)] + [0] * 122
    finally:
        op.close()


def test_slice_ending_at_minus_one(oracle_mod):
    op = mk(dict(OPS["tumble_f64"], offset=999))
    try:
        image = concat([synth(np.arange(300), slice_end=-1), synth(np.arange(200, 500), slice_end=999)])
        _, sl, _ = restore_and_group(op, image, -5000, MAXP, lambda k: oracle_mod.key_groups_binaryrow(k, MAXP),
                                     ctx="slice end -1")
        assert sl["slice_end"].tolist() == [-1, 999] and sl["rows"].tolist() == [300, 300]
    finally:
        op.close()


def test_middle_slice_without_rows_for_the_handle(oracle_mod):
    """3 slices, the middle one holding only keys foreign to the handle's range (0, 63): the
    range restore keeps none of its rows, and the grouped image and its index agree with the
    oracle's filter"""
    O = oracle_mod
    keys = np.arange(2000)
    kg = O.key_groups_binaryrow(keys, MAXP)
    s0 = 1_600_000_001_000
    image = concat([synth(keys[:700], s0), synth(keys[kg >= 64], s0 + 1000), synth(keys[900:], s0 + 2000)])
    want, _ = host_filter(O, image, (0, 63))
    assert not (want["slice_end"] == s0 + 1000).any() and len(np.unique(want["slice_end"])) == 2
    from flink_amd import _lib as L
    op = mk(OPS["tumble_f64"], (0, 63))
    try:
        op.restore_state_range([image], TWM)
        op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
        img, _, sl, idx = grouped_snapshot(op)
        assert_same_rows(want, img, "middle slice")
        assert_grouped(img, sl, idx, MAXP, O.key_groups_binaryrow(img["key"], MAXP), "middle slice")
        assert (sl["rows"][sl["slice_end"] == s0 + 1000] == 0).all()
        assert (np.diff(idx["first_row"]).reshape(idx["n_slices"], MAXP)[:, 64:] == 0).all()
    finally:
        op.close()


# ---- hashes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("maxp", [128, 100])
def test_java_long_hash(oracle_mod, maxp):
    from flink_amd import _lib as L
    O = oracle_mod
    keys = np.unique(splitmix64(np.arange(600, dtype=np.uint64)).view(np.int64))

    def kg_of(k):
        u = np.asarray(k).view(np.uint64)
        h32 = ((u ^ (u >> np.uint64(32))) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        return np.array([O.key_group(int(h), maxp) for h in h32], dtype=np.int32)
    op = mk(OPS["tumble_f64"], (0, maxp - 1), maxp=maxp)
    try:
        _, _, idx = restore_and_group(op, synth(keys), TWM, maxp, kg_of, key_hash=L.KEYHASH_JAVA_LONG, ctx=f"java long {maxp}")
        assert np.count_nonzero(np.diff(idx["first_row"])) > maxp // 2
    finally:
        op.close()


@pytest.mark.parametrize("maxp", [128, 100])
def test_dict_id_hash(maxp):
    """an fg_key_dict id carries its key group in its low 7 bits at both max parallelisms"""
    from flink_amd import _lib as L
    rs = np.random.default_rng(3)
    ids = np.unique((rs.integers(0, 1 << 20, 800).astype(np.int64) << 7) | rs.integers(0, maxp, 800))
    op = mk(OPS["tumble_f64"], (0, maxp - 1), maxp=maxp)
    try:
        _, _, idx = restore_and_group(op, synth(ids), TWM, maxp, lambda k: (k & 127).astype(np.int32),
                                      key_hash=L.KEYHASH_DICT_ID, ctx=f"dict ids {maxp}")
        assert np.count_nonzero(np.diff(idx["first_row"])) > maxp // 2
    finally:
        op.close()


# ---- async ----------------------------------------------------------------------------------------

def test_async_grouped_image_is_the_state_at_the_async_call(oracle_mod):
    """_async, then two more batches and a firing watermark before _wait: image and index are those
    of a synchronous grouped snapshot of a twin stopped at the _async call"""
    from flink_amd import _lib as L
    spec = OPS["hop_i64_big"]
    key, ts, val, _ = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])
    a, b = mk(spec), mk(spec)
    try:
        steps = list(batches_with_watermarks(60000, 10000, ts, 1500))
        for op in (a, b):
            op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
            for lo, hi, wm in steps[:4]:
                op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
                op.process_watermark(wm)
        a.snapshot_state_async()
        fired = 0
        for lo, hi, wm in steps[4:6]:
            a.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            fired += len(a.process_watermark(wm))
        assert fired > 0
        img_a, wm_a = a.snapshot_state_wait()
        sl_a, idx_a = a.snapshot_slices(), a.snapshot_key_groups()
        img_b, wm_b, sl_b, idx_b = grouped_snapshot(b)
        assert wm_a == wm_b and len(img_b["key"]) > 3000 and len(sl_b["slice_end"]) >= 3
        assert_same_rows(img_b, img_a, "async")
        for c in sl_b:
            assert np.array_equal(sl_a[c], sl_b[c]), c
        assert idx_a["n_slices"] == idx_b["n_slices"] and np.array_equal(idx_a["first_row"], idx_b["first_row"])
        assert_grouped(img_a, sl_a, idx_a, MAXP, oracle_mod.key_groups_binaryrow(img_a["key"], MAXP), "async")
        # the operator went on: its next grouped image holds the later state
        img_2, _, sl_2, idx_2 = grouped_snapshot(a)
        assert sl_2["slice_end"].max() > sl_a["slice_end"].max()
        assert_grouped(img_2, sl_2, idx_2, MAXP, oracle_mod.key_groups_binaryrow(img_2["key"], MAXP), "after async")
    finally:
        a.close()
        b.close()


# ---- aliasing -------------------------------------------------------------------------------------

def test_cnt_val_aliases_cnt_star_only_without_nulls(oracle_mod):
    from flink_amd import _lib as L
    for name, alias in (("tumble_f64", True), ("cumulate_nulls", False)):
        op = mid_stream(name)
        try:
            plain, _ = op.snapshot_state()
            op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
            img, _ = op.snapshot_state(copy=False)
            same = img["cnt_val"].ctypes.data == img["cnt_star"].ctypes.data
            assert same == alias, name
            img = {c: v.copy() for c, v in img.items()}
            sl, idx = op.snapshot_slices(), op.snapshot_key_groups()
        finally:
            op.close()
        assert np.array_equal(img["cnt_val"], img["cnt_star"]) == alias, name
        assert_same_rows(plain, img, name)
        assert_grouped(img, sl, idx, MAXP, oracle_mod.key_groups_binaryrow(img["key"], MAXP), name)


# ---- off again, errors ----------------------------------------------------------------------------

def test_off_again_and_errors_leave_the_handle_usable(oracle_mod):
    from flink_amd import _lib as L
    O = oracle_mod
    image = synth(np.arange(5000))
    kg_of = lambda k: O.key_groups_binaryrow(k, MAXP)   # noqa: E731
    op, twin = mk(OPS["tumble_f64"]), mk(OPS["tumble_f64"])
    try:
        restore_and_group(op, image, TWM, MAXP, kg_of, ctx="on")
        # off: no index, and the image is a plain one again that restore_state accepts
        op.set_snapshot_grouping(None)
        plain, wm = op.snapshot_state()
        with pytest.raises(L.FlinkGpuError) as e:
            op.snapshot_key_groups()
        assert e.value.code == L.FG_ESTATE
        twin.restore_state(plain, wm)
        assert_same_state(op, twin, "off again")
        # an unknown hash
        with pytest.raises(L.WindowSpecError):
            op.set_snapshot_grouping(7)
        assert_same_rows(image, op.snapshot_state()[0], "after the unknown hash")
        with pytest.raises(L.FlinkGpuError):   # the refused call left the grouping off
            op.snapshot_key_groups()
        # an async snapshot pending
        op.snapshot_state_async()
        with pytest.raises(L.WindowSpecError):
            op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
        assert_same_rows(image, op.snapshot_state_wait()[0], "the pending image")
        restore_and_group(op, image, TWM, MAXP, kg_of, ctx="after the errors")
        # no image returned since the last snapshot call
        op.snapshot_state_async()
        with pytest.raises(L.FlinkGpuError) as e:
            op.snapshot_key_groups()
        assert e.value.code == L.FG_ESTATE
        img, _ = op.snapshot_state_wait()
        assert_grouped(img, op.snapshot_slices(), op.snapshot_key_groups(), MAXP, kg_of(img["key"]), "collected")
    finally:
        op.close()
        twin.close()


# ---- restore reads only its own -------------------------------------------------------------------

def test_keyed_part_takes_one_run_per_slice(oracle_mod):
    """(CPU arithmetic on a GPU image) keyed_part equals the oracle's filter of the grouped image"""
    from flink_amd import _lib as L, two_phase
    op = mid_stream("multi_value_i64")
    try:
        op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
        img, _, sl, idx = grouped_snapshot(op)
    finally:
        op.close()
    for rng in ((0, 127), (0, 63), (64, 127), (43, 85), (5, 5)):
        part = two_phase.keyed_part(img, idx, rng)
        want, keep = host_filter(oracle_mod, img, rng)
        assert keep.sum() > 0 and set(part) == set(img)
        for c in want:   # the same rows in the same order
            assert np.array_equal(part[c], want[c]), (rng, c)


@pytest.mark.parametrize("P,P2", [(1, 3), (3, 2)])
@pytest.mark.parametrize("kind,size,slide,vt", [("tumble", 1000, 0, "f64"), ("hop", 3000, 1000, "i64"),
                                                ("cumulate", 4000, 1000, "f64")])
def test_rescale_through_grouped_images_matches_oracle(oracle_mod, kind, size, slide, vt, P, P2):
    """test_rescale_matches_oracle with the old subtasks' images grouped and every new subtask
    restoring through restore_keyed: nothing foreign is handed in (rows_in == rows_kept)"""
    from flink_amd import _lib as L, two_phase
    from tests.test_gpu_parity import assert_rows_equal, cfg_of, oracle_mk
    O = oracle_mod
    cfg = cfg_of(kind, size, slide, vt)
    n, batch = 120_000, 10_000
    key, ts, val, _ = make_stream(n, 3000, vt, jitter_ms=1500)
    kg = O.key_groups_binaryrow(key, MAXP)
    subs = subtasks(cfg, P)
    o = oracle_mk(O, cfg)
    g_base = o_base = 0

    def rows_of():
        return np.concatenate([g.take_rows() for _, g in subs])

    try:
        step = 0
        for lo, hi, wm in batches_with_watermarks(n, batch, ts, 100):
            for (klo, khi), g in subs:
                m = (kg[lo:hi] >= klo) & (kg[lo:hi] <= khi)
                if m.any():
                    g.process_batch(key[lo:hi][m], ts[lo:hi][m], val[lo:hi][m])
                g.process_watermark(wm)
            o.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
            o.process_watermark(wm)
            assert_rows_equal(rows_of(), o.take_rows(), vt, f"step {step} wm {wm}")
            step += 1
            if step == 5:
                sources = []
                for _, g in subs:
                    g.prepare_snapshot()
                    g.op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
                    img, twm = g.op.snapshot_state()
                    sources.append((img, twm, g.op.snapshot_key_groups()))
                o.prepare_snapshot()
                o2 = o.restore_copy()
                g_base += sum(g.late_dropped for _, g in subs)
                o_base += o.late_dropped
                for _, g in subs:
                    g.close()
                o.close()
                o = o2
                subs = subtasks(cfg, P2)
                infos = [two_phase.restore_keyed(g.op, sources) for _, g in subs]
                for info in infos:
                    assert info["rows_in"] == info["rows_kept"] > 0, info   # nothing foreign was handed in
                assert sum(i["rows_kept"] for i in infos) == sum(len(im["key"]) for im, _, _ in sources)
        for _, g in subs:
            g.process_watermark(JMAX)
        o.process_watermark(JMAX)
        assert_rows_equal(rows_of(), o.take_rows(), vt, "final")
        late = g_base + sum(g.late_dropped for _, g in subs)
        assert late == o_base + o.late_dropped
    finally:
        for _, g in subs:
            g.close()
        o.close()


def test_restore_keyed_equals_restore_union():
    """the same grouped images through restore_keyed (its own runs only) and restore_union (every
    row, filtered on the GPU) leave the same state"""
    from flink_amd import _lib as L, two_phase
    spec = OPS["cumulate_nulls"]
    img, twm = image_of("cumulate_nulls")
    n = len(img["key"])
    grouped = []   # two old subtasks' images (the slices overlap), each grouped by a handle of its own
    for part, wm in ((take(img, slice(0, n // 3)), twm + 5), (take(img, slice(n // 3, n)), twm)):
        op = mk(spec)
        try:
            op.restore_state(part, wm)
            op.set_snapshot_grouping(L.KEYHASH_BINARYROW_BIGINT)
            g, w = op.snapshot_state()
            assert w == wm
            grouped.append((g, w, op.snapshot_key_groups()))
        finally:
            op.close()
    rng = (43, 85)
    a, b = mk(spec, rng), mk(spec, rng)
    try:
        ia = two_phase.restore_union(a, [(g, wm) for g, wm, _ in grouped])
        ib = two_phase.restore_keyed(b, grouped)
        assert ib["rows_in"] == ib["rows_kept"] == ia["rows_kept"] > 0 and ia["rows_in"] == n > 2 * ia["rows_kept"]
        assert_same_state(a, b, "restore_keyed")
    finally:
        a.close()
        b.close()
