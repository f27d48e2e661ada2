"""Restore on the GPU (fg_restore / restore_state and fg_restore_range / restore_state_range: one
pipeline behind two entry points).

A. For a key-group range R, restore_state_range(images) must leave bit for bit the state that
   restore_state(host_filter(concat(images), R)) leaves, the filter taken from the ORACLE's key
   groups (never from the code under test). Both entry points run the same kernels, so the state
   of either handle is also compared with the expected image built in numpy alone
   (assert_state_is). Images hold each (key, slice) once, so DOUBLE sums have no summation order
   to differ in: every column is compared bit-exactly.
A2. Plain restore_state, unfiltered, against the numpy image.
B. Rescale against the oracle: P subtasks snapshot mid-stream, P' new subtasks restore their
   key-group ranges out of all P images, and the fired rows keep matching the single oracle
   operator (DOUBLE sums within test_gpu_parity's 1e-9 relative bar, everything else exact)."""
import numpy as np
import pytest

from tests.streams import batches_with_watermarks, keys_in_one_region, make_stream, splitmix64

pytestmark = pytest.mark.gpu
MAXP = 128
JMAX = (1 << 63) - 1
RANGES = [(0, 127), (0, 63), (64, 127), (43, 85), (5, 5)]

OPS = {
    "tumble_f64": dict(kind="tumble", size=1000, slide=0, vt="f64", gen={}),
    "hop_i64_big": dict(kind="hop", size=3000, slide=1000, vt="i64", gen=dict(big_ints=True)),
    "cumulate_nulls": dict(kind="cumulate", size=4000, slide=1000, vt="f64", gen=dict(null_frac=0.2)),
    "multi_value_i64": dict(kind="tumble", size=1000, slide=0, vt="i64", gen=dict(null_frac=0.2),
                            aggs=("count_star", "sum", "min", "max")),
}


def mk(spec, rng=(0, MAXP - 1), expected_keys=1 << 12, maxp=MAXP, **kw):
    import flink_amd as F
    w = F.tumbling(spec["size"], spec.get("offset", 0)) if spec["kind"] == "tumble" else \
        {"hop": F.hopping, "cumulate": F.cumulative}[spec["kind"]](spec["size"], spec["slide"])
    aggs = spec.get("aggs", ("count_star", "count", "sum", "avg", "sum0"))
    return F.WindowAggOperator(w, aggs=aggs, val_type=spec["vt"], expected_keys=expected_keys, max_parallelism=maxp,
                               key_group_range=rng, **kw)


_IMAGES = {}


def image_of(name):
    """(image, timer watermark) of a real operator cut mid-stream with several slices resident;
    built once per operator kind and never modified. 10 records per ms (the keys do not depend on
    the rate): 40,000 records span 4.3 s, and the watermark trails by 1.5 s, so that the slices
    ending 3000, 4000 and 5000 (and a shared window's earlier ones) are resident at the cut."""
    if name not in _IMAGES:
        spec = OPS[name]
        key, ts, val, isnull = make_stream(60000, 3000, spec["vt"], jitter_ms=300, rate_per_ms=10, **spec["gen"])
        op = mk(spec)
        for lo, hi, wm in batches_with_watermarks(40000, 10000, ts, 1500):
            op.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi], None if isnull is None else isnull[lo:hi])
            op.process_watermark(wm)
        op.prepare_snapshot_pre_barrier()
        img, twm = op.snapshot_state()
        op.close()
        assert len(np.unique(img["slice_end"])) >= 3 and len(img["key"]) > 3000
        for v in img.values():
            v.setflags(write=False)
        _IMAGES[name] = (img, twm)
    return _IMAGES[name]


def host_filter(O, img, rng, kg=None):
    kg = O.key_groups_binaryrow(img["key"], MAXP) if kg is None else kg
    keep = (kg >= rng[0]) & (kg <= rng[1])
    return {c: np.asarray(v)[keep] for c, v in img.items()}, keep


def concat(imgs):
    return {c: np.concatenate([np.asarray(im[c]) for im in imgs]) for c in imgs[0]}


def take(img, sel):
    return {c: np.asarray(v)[sel] for c, v in img.items()}


def snap(op):
    img, wm = op.snapshot_state()
    order = np.lexsort((img["key"], img["slice_end"]))
    return {c: v[order] for c, v in img.items()}, wm


def assert_same_state(a, b, ctx=""):
    (ia, wa), (ib, wb) = snap(a), snap(b)
    assert wa == wb, f"{ctx}: timer watermark {wb} vs {wa}"
    assert set(ia) == set(ib), ctx
    for c in ia:
        assert len(ia[c]) == len(ib[c]), f"{ctx}: {len(ib[c])} rows vs {len(ia[c])} expected"
        assert np.array_equal(ia[c].view(np.int64), ib[c].view(np.int64)), f"{ctx}: column {c} differs"


def by_slice_and_key(img):
    order = np.lexsort((img["key"], img["slice_end"]))
    return {c: np.asarray(v)[order] for c, v in img.items()}


def assert_state_is(op, expected_image, ctx=""):
    """the operator's state against an image built in numpy alone (no engine code on this side):
    every column of the snapshot, sorted by (slice_end, key) and viewed as int64. DOUBLE sums are
    compared after x + 0.0, which maps -0.0 to +0.0 and changes nothing else."""
    from flink_amd import _lib as L
    got, exp = snap(op)[0], by_slice_and_key(expected_image)
    assert set(got) == set(exp), f"{ctx}: columns {sorted(got)} vs {sorted(exp)} expected"
    for c in got:
        g, e = got[c].view(np.int64), exp[c].view(np.int64)
        assert len(g) == len(e), f"{ctx}: {len(g)} rows vs {len(e)} expected"
        if c == "sum" and op.val_type == L.VAL_F64:
            g, e = ((x.view(np.float64) + 0.0).view(np.int64) for x in (g, e))
        assert np.array_equal(g, e), f"{ctx}: column {c} differs from the expected image"


def merged(img):
    """numpy merge of the rows of an i64 image that share (key, slice): counts and sums added,
    min of min, max of max"""
    s = by_slice_and_key(img)
    first = np.ones(len(s["key"]), dtype=bool)
    first[1:] = (s["key"][1:] != s["key"][:-1]) | (s["slice_end"][1:] != s["slice_end"][:-1])
    at = np.flatnonzero(first)
    out = dict(key=s["key"][at], slice_end=s["slice_end"][at])
    for c in ("cnt_star", "cnt_val", "sum"):
        out[c] = np.add.reduceat(s[c], at)
    if "min" in s:
        out["min"], out["max"] = np.minimum.reduceat(s["min"], at), np.maximum.reduceat(s["max"], at)
    return out


def check_range_restore(O, spec, images, rng, twm, to_device=False, kg_of=None, key_hash=None, expected_keys=1 << 12,
                        maxp=MAXP, ctx=""):
    """path A (host filter + restore_state) against path B (restore_state_range) on fresh handles"""
    cat = concat(images)
    kg = None if kg_of is None else kg_of(cat["key"])
    filt, keep = host_filter(O, cat, rng, kg)
    a = mk(spec, rng, expected_keys, maxp)
    b = mk(spec, rng, expected_keys, maxp)
    try:
        a.restore_state(filt, twm)
        if to_device:
            import torch
            images = [{c: torch.from_numpy(np.array(v)).cuda() for c, v in im.items()} for im in images]
        kw = {} if key_hash is None else dict(key_hash=key_hash)
        info = b.restore_state_range([(im, twm) for im in images], **kw)
        assert info["rows_in"] == len(cat["key"]), (ctx, info)
        assert info["rows_kept"] == int(keep.sum()), (ctx, info)
        assert info["slices"] == len(np.unique(cat["slice_end"][keep])), (ctx, info)
        assert info["state_regions"] == b.stats()["state_regions"] == a.stats()["state_regions"], (ctx, info)
        assert_same_state(a, b, ctx)
        assert_state_is(a, filt, ctx + " (restore_state)")
        assert_state_is(b, filt, ctx + " (restore_state_range)")
        return info, b.stats()
    finally:
        a.close()
        b.close()


def synth(keys, slice_end=1_600_000_001_000, mv=False):
    """one-slice image of the given keys, COUNT(v) below COUNT(*) on every third row"""
    n = len(keys)
    i = np.arange(n, dtype=np.int64)
    img = dict(key=np.asarray(keys, dtype=np.int64), slice_end=np.full(n, slice_end, dtype=np.int64), cnt_star=i % 5 + 1,
               cnt_val=i % 5 + 1 - (i % 3 == 0), sum=(i * 0.5 + 1.0).view(np.int64))
    if mv:   # (a row without a value holds the accumulators' identities, as a snapshot writes them)
        none = img["cnt_val"] == 0
        img["min"], img["max"] = np.where(none, JMAX, i - 7), np.where(none, -JMAX - 1, i + 7)
    return img


# ---- A. equivalence with restore_state ------------------------------------------------------------

def test_oracle_key_groups_of_the_stream(oracle_mod):
    """the ranges of the cases below are not vacuous (CPU side only)"""
    key = np.unique(make_stream(60000, 3000, "f64", jitter_ms=300)[0])
    kg = oracle_mod.key_groups_binaryrow(key, MAXP)
    assert len(key) == 3000 and len(np.unique(kg)) == 128
    assert [int(((kg >= lo) & (kg <= hi)).sum()) for lo, hi in ((0, 63), (64, 127))] == [1480, 1520]
    assert [int(((kg >= lo) & (kg <= hi)).sum()) for lo, hi in ((0, 42), (43, 85), (86, 127))] == [991, 1006, 1003]
    assert int((kg == 5).sum()) == 15


@pytest.mark.parametrize("rng", RANGES, ids=[f"{lo}-{hi}" for lo, hi in RANGES])
@pytest.mark.parametrize("name", list(OPS))
def test_range_restore_equals_host_filter(oracle_mod, name, rng):
    img, twm = image_of(name)
    info, _ = check_range_restore(oracle_mod, OPS[name], [img], rng, twm, ctx=f"{name} {rng}")
    assert info["rows_kept"] > 0
    if rng == (0, 127):
        assert info["rows_kept"] == info["rows_in"]


@pytest.mark.parametrize("n,kept", [(0, 0), (1, 0), (63, 33), (64, 33), (65, 34), (257, 121)])
def test_row_counts_at_wave_and_workgroup_edges(oracle_mod, n, kept):
    spec = OPS["tumble_f64"]
    img = synth(np.arange(n))
    info, _ = check_range_restore(oracle_mod, spec, [img], (0, 63), 1_600_000_000_000, ctx=f"n={n}")
    assert info["rows_kept"] == kept
    if n == 1:   # key 0 is foreign to (0, 63): the other half keeps it
        info, _ = check_range_restore(oracle_mod, spec, [img], (64, 127), 1_600_000_000_000, ctx="n=1 upper half")
        assert info["rows_kept"] == 1


def split_parts(img, seed=7):
    """3 parts of unequal size (cut inside slices, so a slice lies in two parts), an empty image in
    the middle, the second part's rows shuffled"""
    n = len(img["key"])
    a, b = n // 5, n // 5 + n // 2
    se = img["slice_end"]
    assert se[a - 1] == se[a] or se[b - 1] == se[b]
    perm = np.random.default_rng(seed).permutation(b - a) + a
    return [take(img, slice(0, a)), take(img, slice(0, 0)), take(img, perm), take(img, slice(b, n))]


@pytest.mark.parametrize("name", ["hop_i64_big", "multi_value_i64"])
def test_several_images(oracle_mod, name):
    img, twm = image_of(name)
    check_range_restore(oracle_mod, OPS[name], split_parts(img), (43, 85), twm, ctx=name)


@pytest.mark.parametrize("name", ["cumulate_nulls", "multi_value_i64"])
def test_device_images_equal_host_images(oracle_mod, name):
    img, twm = image_of(name)
    check_range_restore(oracle_mod, OPS[name], [img], (64, 127), twm, to_device=True, ctx=name + " one image")
    check_range_restore(oracle_mod, OPS[name], split_parts(img), (0, 63), twm, to_device=True, ctx=name + " parts")


# state_regions that the host implementation of restore_state left (the parent of the commit that
# made it the unfiltered case of the GPU pipeline), measured there on an MI355X
REGIONS_200K = {4096: 1024, 1000: 64}
REGIONS_ONE_REGION = 8192


@pytest.mark.parametrize("expected_keys", [4096, 1000])
def test_restore_grows_the_regions(oracle_mod, expected_keys):
    """A one-slice image of 200,000 keys into a handle sized for far fewer. A handle opened for
    4,096 keys or more starts at 2^10 regions (fg_open's floor for TUMBLE), which hold the ~100,000
    kept rows as they are -- neither restore path splits them; one opened for 1,000 keys starts with a
    single region and must split. Both must end with the regions and the state of path A."""
    spec = OPS["tumble_f64"]
    probe = mk(spec, expected_keys=expected_keys)
    before = probe.stats()["state_regions"]
    probe.close()
    info, stats = check_range_restore(oracle_mod, spec, [synth(np.arange(200_000))], (0, 63), 1_600_000_000_000,
                                      expected_keys=expected_keys, ctx="200k keys")
    assert info["rows_kept"] > 90_000
    assert stats["state_regions"] == REGIONS_200K[expected_keys], (info, before)
    if expected_keys < 4096:
        assert before == 1 and stats["state_regions"] > before, (info, before)


def test_restore_of_keys_in_one_region(oracle_mod):
    """3000 of a region's 3584 entries at every split: sizing stops at the finest split and succeeds"""
    _, stats = check_range_restore(oracle_mod, OPS["tumble_f64"], [synth(keys_in_one_region(3000))], (0, 127),
                                   1_600_000_000_000, ctx="one region")
    assert stats["state_regions"] == REGIONS_ONE_REGION


def test_slice_end_equal_to_the_dictionary_marker(oracle_mod):
    """the slice dictionary marks a free slot with all ones: a slice ending at -1 (TUMBLE 1 s with
    offset 999) is carried beside the table"""
    spec = dict(OPS["tumble_f64"], offset=999)
    parts = [synth(np.arange(300), slice_end=-1), synth(np.arange(200, 500), slice_end=999)]
    info, _ = check_range_restore(oracle_mod, spec, parts, (0, 63), -5000, ctx="slice end -1")
    assert info["slices"] == 2


def test_restore_into_a_live_handle(oracle_mod):
    """part 2 shares a slice with part 1 (disjoint keys) and adds new slices"""
    O, spec = oracle_mod, OPS["hop_i64_big"]
    img, twm = image_of("hop_i64_big")
    ends = np.unique(img["slice_end"])
    mid = ends[len(ends) // 2]
    first = (img["slice_end"] < mid) | ((img["slice_end"] == mid) & (img["key"] % 2 == 0))
    p1, p2 = take(img, first), take(img, ~first)
    assert (p1["slice_end"] == mid).any() and (p2["slice_end"] == mid).any() and (p2["slice_end"] > mid).any()
    rng = (43, 85)
    a, b = mk(spec, rng), mk(spec, rng)
    try:
        for part in (p1, p2):
            a.restore_state(host_filter(O, part, rng)[0], twm)
            b.restore_state_range([part], twm)
        assert_same_state(a, b, "live handle")
        union = host_filter(O, img, rng)[0]
        assert_state_is(a, union, "live handle (restore_state)")
        assert_state_is(b, union, "live handle (restore_state_range)")
    finally:
        a.close()
        b.close()


def test_java_long_hash(oracle_mod):
    from flink_amd import _lib as L
    O = oracle_mod
    keys = np.unique(splitmix64(np.arange(600, dtype=np.uint64)).view(np.int64))
    u = keys.view(np.uint64)
    h32 = ((u ^ (u >> np.uint64(32))) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    kg_of = lambda k: np.array([O.key_group(int(h), MAXP) for h in h32], dtype=np.int32)   # noqa: E731
    info, _ = check_range_restore(O, OPS["tumble_f64"], [synth(keys)], (43, 85), 1_600_000_000_000, kg_of=kg_of,
                                  key_hash=L.KEYHASH_JAVA_LONG, ctx="java long")
    assert 0 < info["rows_kept"] < len(keys)


@pytest.mark.parametrize("maxp", [128, 100])
def test_dict_id_hash(oracle_mod, maxp):
    """an fg_key_dict id carries its key group in its low 7 bits at both max parallelisms"""
    from flink_amd import _lib as L
    rs = np.random.default_rng(3)
    ids = np.unique((rs.integers(0, 1 << 20, 800).astype(np.int64) << 7) | rs.integers(0, maxp, 800))
    rng = (30, 70)
    info, _ = check_range_restore(oracle_mod, OPS["tumble_f64"], [synth(ids)], rng, 1_600_000_000_000,
                                  kg_of=lambda k: (k & 127).astype(np.int32), key_hash=L.KEYHASH_DICT_ID, maxp=maxp,
                                  ctx=f"dict ids maxp {maxp}")
    assert 0 < info["rows_kept"] < len(ids)


def test_errors_leave_the_handle_usable(oracle_mod):
    from flink_amd import _lib as L
    O = oracle_mod
    rng = (0, 63)
    twm = 1_600_000_000_000
    good = synth(np.arange(500))
    n_ends = 4097
    many = synth(np.arange(n_ends))
    many["slice_end"] = 1_600_000_001_000 + 1000 * np.arange(n_ends, dtype=np.int64)
    no_sum = dict(good, sum=None)
    for spec, bad, kw in ((OPS["multi_value_i64"], good, {}),                        # no min / max
                          (OPS["tumble_f64"], good, dict(key_hash=7)),               # unknown key hash
                          (OPS["tumble_f64"], no_sum, {}),                           # NULL sum column
                          (OPS["tumble_f64"], many, {})):                            # 4097 distinct slice ends
        mv = "aggs" in spec
        valid = synth(np.arange(500), mv=mv)
        a, b = mk(spec, rng), mk(spec, rng)
        try:
            with pytest.raises(L.WindowSpecError):
                b.restore_state_range([bad], twm, **kw)
            a.restore_state(host_filter(O, valid, rng)[0], twm)
            b.restore_state_range([valid], twm)
            assert_same_state(a, b, f"after error {sorted(kw)} {len(bad['key'])}")
            assert_state_is(a, host_filter(O, valid, rng)[0], "restore_state after an error")
            assert_state_is(b, host_filter(O, valid, rng)[0], "restore_state_range after an error")
        finally:
            a.close()
            b.close()
    # 4096 distinct slice ends are within the limit (few of the rows are kept)
    info, _ = check_range_restore(O, OPS["tumble_f64"], [take(many, slice(0, 4096))], (5, 5), twm, ctx="4096 slice ends")
    assert info["rows_in"] == 4096 and 0 < info["slices"] < 200
    # a range outside the key groups: fg_open takes it, the range restore refuses it
    a, b = mk(OPS["tumble_f64"]), mk(OPS["tumble_f64"], (5, 200))
    try:
        with pytest.raises(L.WindowSpecError):
            b.restore_state_range([good], twm)
        a.restore_state(good, twm)
        b.restore_state(good, twm)
        assert_same_state(a, b, "after the range error")
        assert_state_is(a, good, "restore_state beside the range error")
        assert_state_is(b, good, "restore_state after the range error")
    finally:
        a.close()
        b.close()


# ---- A2. plain restore_state against the numpy image -------------------------------------------------

TWM = 1_600_000_000_000


def check_plain_restore(spec, image, expected=None, twm=TWM, ctx="", **mk_kw):
    op = mk(spec, **mk_kw)
    try:
        op.restore_state(image, twm)
        assert_state_is(op, image if expected is None else expected, ctx)
        return op.stats()
    finally:
        op.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_plain_restore_at_wave_and_workgroup_edges(n):
    """every row is kept whatever the handle's key groups are: none configured, and one group"""
    check_plain_restore(OPS["tumble_f64"], synth(np.arange(n)), ctx=f"n={n}, no max parallelism", rng=(0, 0), maxp=0)
    check_plain_restore(OPS["tumble_f64"], synth(np.arange(n)), ctx=f"n={n}, range (5, 5)", rng=(5, 5))


def test_plain_restore_of_the_dictionary_marker_slice():
    spec = dict(OPS["tumble_f64"], offset=999)
    image = concat([synth(np.arange(300), slice_end=-1), synth(np.arange(300, 500), slice_end=999)])
    check_plain_restore(spec, image, twm=-5000, ctx="slice ends -1 and 999")


def test_plain_restore_of_keys_in_one_region():
    stats = check_plain_restore(OPS["tumble_f64"], synth(keys_in_one_region(3000)), ctx="one region")
    assert stats["state_regions"] == REGIONS_ONE_REGION


def test_plain_restore_multi_value():
    check_plain_restore(OPS["multi_value_i64"], synth(np.arange(500), mv=True), ctx="multi-value")


def test_plain_restore_merges_duplicate_rows():
    """100 (key, slice) pairs occur three times each, shuffled across the image: the state is their
    numpy merge (i64, so that the order of the additions cannot matter)"""
    base = synth(np.arange(400), mv=True)
    again = take(base, slice(150, 250))
    image = concat([base, again, again])
    image = take(image, np.random.default_rng(11).permutation(len(image["key"])))
    exp = merged(image)
    assert len(exp["key"]) == 400 and len(image["key"]) == 600
    assert np.array_equal(exp["cnt_star"][150:250], 3 * base["cnt_star"][150:250])
    check_plain_restore(OPS["multi_value_i64"], image, expected=exp, ctx="duplicates")


def many_slice_ends(n_ends):
    many = synth(np.arange(n_ends))
    many["slice_end"] = 1_600_000_001_000 + 1000 * np.arange(n_ends, dtype=np.int64)
    return many


def test_plain_restore_slice_end_limit():
    """every distinct slice end becomes a resident table: handles opened for 1,000 keys keep each at
    one region"""
    from flink_amd import _lib as L
    check_plain_restore(OPS["tumble_f64"], many_slice_ends(4096), ctx="4096 slice ends", expected_keys=1000)
    op = mk(OPS["tumble_f64"], expected_keys=1000)
    try:
        with pytest.raises(L.WindowSpecError, match="fg_restore:"):
            op.restore_state(many_slice_ends(4097), TWM)
        good = synth(np.arange(500))
        op.restore_state(good, TWM)
        assert_state_is(op, good, "after 4097 slice ends")
    finally:
        op.close()


@pytest.mark.parametrize("name,bad", [("tumble_f64", dict(synth(np.arange(500)), sum=None)),   # NULL sum column
                                      ("multi_value_i64", synth(np.arange(500)))],             # no min / max
                         ids=["null_sum", "no_min_max"])
def test_plain_restore_errors_leave_the_handle_usable(name, bad):
    from flink_amd import _lib as L
    op = mk(OPS[name])
    try:
        with pytest.raises(L.WindowSpecError):
            op.restore_state(bad, TWM)
        good = synth(np.arange(500), mv="aggs" in OPS[name])
        op.restore_state(good, TWM)
        assert_state_is(op, good, f"after {name} error")
    finally:
        op.close()


# ---- B. rescale against the oracle -----------------------------------------------------------------

def ranges_of(P):
    return [((r * MAXP + P - 1) // P, ((r + 1) * MAXP - 1) // P) for r in range(P)]


def subtasks(cfg, P):
    import flink_amd as F
    from tests.gpu_adapter import GpuOperator, window_of
    return [(rng, GpuOperator(cfg, _op=F.WindowAggOperator(window_of(cfg), aggs=("count_star", "count", "sum", "avg", "sum0"),
                                                           val_type=cfg["val_type"], expected_keys=3000,
                                                           buffer_records=1 << 16, max_parallelism=MAXP,
                                                           key_group_range=rng)))
            for rng in ranges_of(P)]


@pytest.mark.parametrize("P,P2", [(1, 3), (3, 2)])
@pytest.mark.parametrize("kind,size,slide,vt", [("tumble", 1000, 0, "f64"), ("hop", 3000, 1000, "i64"),
                                                ("cumulate", 4000, 1000, "f64")])
def test_rescale_matches_oracle(oracle_mod, kind, size, slide, vt, P, P2):
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
                images = []
                for _, g in subs:
                    g.prepare_snapshot()
                    images.append(g.op.snapshot_state())
                o.prepare_snapshot()
                o2 = o.restore_copy()
                g_base += sum(g.late_dropped for _, g in subs)
                o_base += o.late_dropped
                for _, g in subs:
                    g.close()
                o.close()
                o = o2
                subs = subtasks(cfg, P2)
                kept = sum(g.op.restore_state_range(images)["rows_kept"] for _, g in subs)
                assert kept == sum(len(im["key"]) for im, _ in images) > 0   # the new ranges partition the key groups
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


def test_restore_union_equals_union_image_for(oracle_mod):
    """the two-phase mirror: restore_union on a global operator's images against union_image_for +
    restore_state with the oracle's key groups"""
    from flink_amd import two_phase
    O, spec = oracle_mod, OPS["cumulate_nulls"]
    img, twm = image_of("cumulate_nulls")
    n = len(img["key"])
    images = [(take(img, slice(0, n // 3)), twm + 5), (take(img, slice(n // 3, n)), twm)]
    rng = (43, 85)
    a, b = mk(spec, rng), mk(spec, rng)
    try:
        filt, wm = two_phase.union_image_for(images, rng, MAXP, key_groups=lambda k: O.key_groups_binaryrow(k, MAXP))
        assert wm == twm
        a.restore_state(filt, wm)
        info = two_phase.restore_union(b, images)
        assert info["rows_kept"] == len(filt["key"])
        assert_same_state(a, b, "restore_union")
        assert_state_is(a, filt, "union_image_for + restore_state")
        assert_state_is(b, filt, "restore_union")
    finally:
        a.close()
        b.close()
