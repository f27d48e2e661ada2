"""Parity of the HIP engine with the oracle at the edges of time the other suites leave out:
nonzero window offsets of both signs, fixed zone offsets in the two-phase and windowed-input
paths, rowtimes below 0, the borders of the 32-bit rowtime fast path (a stream that enters it
mid-run, |t| >= 2^52, slices of 1 ms and of more than 2^32 ms).

Every step is compared, not only the final rows: with an offset, the step in which a row
appears is the thing under test. One small shape for every case (BASE); BIGINT values, so
everything is bit-exact; two cases repeat with DOUBLE under test_gpu_parity's REL_TOL.

Watermarks of the streams that cross epoch 0 are raised to max(wm, -slice): below -slice the
reference's getNextTriggerWatermark (truncated remainder of the watermark) flushes its buffer
one interval late and loses windows (divergences), which is not matched.

Each case asserts on the oracle's output that it is not vacuous: rows in at least 3 steps,
late drops wherever the jitter exceeds the delay, rows with negative window ends where the
case is about them."""
import numpy as np
import pytest

from tests.streams import batches_with_watermarks, make_stream
from tests.test_gpu_parity import JMAX, assert_rows_equal, cfg_of, drive_both, gpu_mk, oracle_mk

pytestmark = pytest.mark.gpu

H = 3600 * 1000
BASE = dict(n=24_000, keys=300, batch=2_000, rate_per_ms=4, jitter=1500, delay=100)
GEN_KEYS = ("t0", "rate_per_ms", "key_spread")


def kw_of(**over):
    return dict(BASE, **over)


def slice_of(cfg):
    return cfg["size"] if cfg["kind"] == "tumble" else int(np.gcd(cfg["size"], cfg["slide"])) if cfg["kind"] == "hop" \
        else cfg["slide"]


def stream_of(cfg, kw):
    return make_stream(kw["n"], kw["keys"], cfg["val_type"], jitter_ms=kw["jitter"],
                       **{k: kw[k] for k in GEN_KEYS if k in kw})


def steps_of(ts, kw, wm_floor):
    """(lo, hi, watermark) per batch; watermarks raised to wm_floor when given."""
    return [(lo, hi, wm if wm_floor is None else max(wm, wm_floor))
            for lo, hi, wm in batches_with_watermarks(kw["n"], kw["batch"], ts, kw["delay"])]


class Facts:
    """What the oracle alone makes of a case: the steps that gave rows, rows, rows with a
    negative window end, late drops."""

    def __init__(self):
        self.steps = self.rows = self.negative = self.late = 0

    def step(self, rows):
        self.steps += 1 if len(rows) else 0
        self.rows += len(rows)
        self.negative += int((rows["window_end"] < 0).sum())

    def check(self, kw, negative=False):
        assert self.steps >= 3, f"rows in {self.steps} steps only"
        if kw["jitter"] > kw["delay"]:
            assert self.late > 0, "a jitter beyond the delay and no late record"
        if negative:
            assert self.negative > 0, "no row with a negative window end"


def oracle_facts(O, cfg, kw, wm_floor=None):
    key, ts, val, _ = stream_of(cfg, kw)
    o, f = oracle_mk(O, cfg), Facts()
    for lo, hi, wm in steps_of(ts, kw, wm_floor):
        o.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        o.process_watermark(wm)
        f.step(o.take_rows())
    o.process_watermark(JMAX)
    f.step(o.take_rows())
    f.late = o.late_dropped
    o.close()
    return f


def drive_clamped(O, cfg, kw, wm_floor, expected_keys=None):
    """drive_both with every watermark raised to wm_floor; returns the oracle's Facts."""
    key, ts, val, _ = stream_of(cfg, kw)
    g = gpu_mk(cfg, expected_keys=expected_keys or kw["keys"], buffer_records=1 << 16)
    o, f = oracle_mk(O, cfg), Facts()
    for step, (lo, hi, wm) in enumerate(steps_of(ts, kw, wm_floor)):
        g.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        o.process_batch(key[lo:hi], ts[lo:hi], val[lo:hi])
        g.process_watermark(wm)
        o.process_watermark(wm)
        exp = o.take_rows()
        assert_rows_equal(g.take_rows(), exp, cfg["val_type"], f"step {step} wm {wm}")
        assert g.late_dropped == o.late_dropped, f"late drops differ at step {step}"
        f.step(exp)
    g.process_watermark(JMAX)
    o.process_watermark(JMAX)
    exp = o.take_rows()
    assert_rows_equal(g.take_rows(), exp, cfg["val_type"], "final")
    f.step(exp)
    f.late = o.late_dropped
    g.close()
    o.close()
    return f


def run_single(O, cfg, kw, wm_floor=None, expected_keys=None, negative=False):
    if wm_floor is None:
        oracle_facts(O, cfg, kw).check(kw, negative)
        late = drive_both(O, cfg, kw["n"], kw["keys"], kw["batch"], kw["delay"], kw["jitter"],
                          expected_keys=expected_keys, **{k: kw[k] for k in GEN_KEYS if k in kw})
        assert late > 0 or kw["jitter"] <= kw["delay"]
    else:
        drive_clamped(O, cfg, kw, wm_floor, expected_keys).check(kw, negative)


# ---- 1. offsets at positive times, single phase ------------------------------------------------
# (a hopping slice's record is dropped only once the slice's last window fired, 2 s behind the
# slice: those cases take a jitter of 4500 to hold late records)
SQL_OFFSET_CASES = [
    ("tumble_off-300", cfg_of("tumble", 1000, vt="i64", offset=-300), {}),
    ("tumble_off+700", cfg_of("tumble", 1000, vt="i64", offset=700), {}),
    ("hop_off+250_tz+8h", cfg_of("hop", 3000, 1000, vt="i64", offset=250, tz=8 * H), dict(jitter=4500)),
    ("cumulate_off-999_tz-5h", cfg_of("cumulate", 4000, 1000, vt="i64", offset=-999, tz=-5 * H), {}),
]
OFFSET_CASES = SQL_OFFSET_CASES + [
    ("ds_tumble", cfg_of("tumble", 1000, vt="i64", mode="datastream"), {}),
    ("ds_tumble_off-300", cfg_of("tumble", 1000, vt="i64", mode="datastream", offset=-300), {}),
    ("ds_sliding_off-400", cfg_of("hop", 3000, 1000, vt="i64", mode="datastream", offset=-400), dict(jitter=4500)),
    ("ds_lateness_tumble_off-300", dict(cfg_of("tumble", 1000, vt="i64", mode="datastream", offset=-300),
                                        allowed_lateness=800), {}),
]
# narrow keys on the tile path; keys over the whole BIGINT range (k_part1, not the tile path);
# 64 or more state regions
VARIANTS = [("plain", {}, None), ("spread", dict(key_spread=True), None), ("regions", {}, 200_000)]


@pytest.mark.parametrize("variant,gen,expected_keys", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("name,cfg,over", OFFSET_CASES, ids=[c[0] for c in OFFSET_CASES])
def test_offsets_single_phase(oracle_mod, name, cfg, over, variant, gen, expected_keys):
    run_single(oracle_mod, cfg, kw_of(**over, **gen), expected_keys=expected_keys)


@pytest.mark.parametrize("name,cfg,over", [c for c in SQL_OFFSET_CASES if c[0] in ("tumble_off-300", "hop_off+250_tz+8h")],
                         ids=["tumble_off-300", "hop_off+250_tz+8h"])
def test_offsets_single_phase_double(oracle_mod, name, cfg, over):
    run_single(oracle_mod, dict(cfg, val_type="f64"), kw_of(**over))


# ---- 2. two-phase: local -> route -> global against the oracle's local -> global pair ----------
def run_two_phase(O, cfg, kw, wm_floor=None, negative=False):
    """3 source partitions with a local operator each, partial rows routed to 2 owners by key
    group, as test_two_phase_parity does -- compared with the oracle's PHASE_LOCAL /
    PHASE_GLOBAL operators fed the same batches and watermarks, not with the single-phase
    oracle: with a window offset the local operators flush on the offset-0 trigger grid
    (getNextTriggerWatermark), so partials reach the global operators after their slice fired
    and are dropped there. The rows of every step and the global operators' late-drop counts
    must match."""
    import flink_amd as F
    from tests.fixture_runner import KIND, VT
    from tests.gpu_adapter import GpuOperator, window_of
    S, R, MAXP = 3, 2, 128
    key, ts, val, _ = stream_of(cfg, kw)
    aggs = ("count_star", "count", "sum", "avg", "sum0")
    mk = lambda local, keys: F.WindowAggOperator(window_of(cfg), aggs=aggs, val_type=cfg["val_type"], expected_keys=keys,
                                                 buffer_records=1 << 16, local_partials=local,
                                                 shift_tz_offset_ms=cfg["tz_offset_ms"])
    omk = lambda phase: O.OracleOperator(kind=KIND[cfg["kind"]], size=cfg["size"], slide=cfg["slide"],
                                         offset=cfg["offset"], tz_offset_ms=cfg["tz_offset_ms"],
                                         val_type=VT[cfg["val_type"]], phase=phase)
    gl, gg = [mk(True, kw["keys"]) for _ in range(S)], [mk(False, kw["keys"] // R + 1) for _ in range(R)]
    ol, og = [omk(O.PHASE_LOCAL) for _ in range(S)], [omk(O.PHASE_GLOBAL) for _ in range(R)]
    owner_of = lambda k: O.key_groups_binaryrow(k, MAXP).astype(np.int64) * R // MAXP
    src = np.arange(kw["n"]) % S
    adapter = GpuOperator.__new__(GpuOperator)
    adapter.cfg = cfg
    f = Facts()
    partial_rows = 0

    def advance(wm, ctx):
        nonlocal partial_rows
        for s in range(S):   # the local operators' partial rows cross the exchange
            rows = gl[s].process_watermark(wm)
            ol[s].process_watermark(wm)
            exp = ol[s].take_rows()
            partial_rows += len(exp)
            owner, eowner = owner_of(rows["key"]), owner_of(exp["key"])
            for r in range(R):
                m = owner == r
                if m.any():
                    gg[r].process_partials(rows["key"][m], rows["window_end"][m], rows["count_star"][m],
                                           rows["count"][m], rows["sum"][m])
                og[r].process_partials(exp[eowner == r])
        got = [g.process_watermark(wm) for g in gg]
        for o in og:
            o.process_watermark(wm)
        exp = np.concatenate([o.take_rows() for o in og])
        adapter._rows = [x for x in got if len(x)]
        assert_rows_equal(adapter.take_rows(), exp, cfg["val_type"], ctx)
        # (per partial row: equal only while the local operators flush when the reference's do)
        for r in range(R):
            assert gg[r].num_late_records_dropped == og[r].late_dropped, f"{ctx}: late drops of global operator {r}"
        f.step(exp)

    for step, (lo, hi, wm) in enumerate(steps_of(ts, kw, wm_floor)):
        for s in range(S):
            m = src[lo:hi] == s
            gl[s].process_batch(key[lo:hi][m], ts[lo:hi][m], val[lo:hi][m])
            ol[s].process_batch(key[lo:hi][m], ts[lo:hi][m], val[lo:hi][m])
        advance(wm, f"step {step} wm {wm}")
    advance(JMAX, "final")
    f.late = sum(o.late_dropped for o in og)
    for x in gl + gg + ol + og:
        x.close()
    assert partial_rows > 0
    f.check(kw, negative)   # late: partial rows dropped in the global phase


@pytest.mark.parametrize("name,cfg,over", SQL_OFFSET_CASES, ids=[c[0] for c in SQL_OFFSET_CASES])
def test_offsets_two_phase(oracle_mod, name, cfg, over):
    run_two_phase(oracle_mod, cfg, kw_of(**over))


# ---- 3. windowed input ---------------------------------------------------------------------------
def jrem(a, b):
    """Java's truncated remainder (the sign of the dividend)."""
    return np.fmod(a, b)


def windowed_rows(cfg, key, ts, val):
    """A window TVF's output: every record once per window that holds it (record-major), the
    window's end in local time (rowtime + tz) as its window_end column. Windows that do not
    hold the record are masked, so ends of either sign pass. Slice and window starts by
    TimeWindow.getWindowStartWithOffset, truncated remainder included."""
    kind, size, off = cfg["kind"], cfg["size"], cfg["offset"]
    S = slice_of(cfg)
    lt = ts + cfg["tz_offset_ms"]
    se = lt - jrem(lt - off + S, S) + S
    nw = size // S
    E = np.stack([se + j * S for j in range(nw)], axis=1)
    if kind != "cumulate":
        keep = np.ones_like(E, dtype=bool)
    else:
        ws = (se - 1) - jrem((se - 1) - off + size, size)
        keep = E <= (ws + size)[:, None]
    rep = keep.sum(axis=1)
    keep = keep.ravel()
    return dict(key=np.repeat(key, rep), wend=E.ravel()[keep], val=np.repeat(val, rep), ts=np.repeat(ts, rep))


def run_windowed(O, cfg, kw, wm_floor=None, negative=False):
    cfg = dict(cfg, windowed=True, count_star_index=-1 if cfg["kind"] == "hop" else 0)
    key, ts, val, _ = stream_of(cfg, kw)
    r = windowed_rows(cfg, key, ts, val)
    n = len(r["key"])
    per = n // kw["n"]   # rows per record: a batch holds the same records in every form
    g = gpu_mk(cfg, expected_keys=kw["keys"], buffer_records=1 << 16)
    o, f = oracle_mk(O, cfg), Facts()
    mx = np.iinfo(np.int64).min
    batch = kw["batch"] * max(per, 1)
    for step, lo in enumerate(range(0, n, batch)):
        hi = min(n, lo + batch)
        for op in (g, o):
            op.process_batch(r["key"][lo:hi], r["wend"][lo:hi], r["val"][lo:hi])
        mx = max(mx, int(r["ts"][lo:hi].max()))
        wm = mx - kw["delay"] - 1
        wm = wm if wm_floor is None else max(wm, wm_floor)
        g.process_watermark(wm)
        o.process_watermark(wm)
        exp = o.take_rows()
        assert_rows_equal(g.take_rows(), exp, cfg["val_type"], f"step {step} wm {wm}")
        assert g.late_dropped == o.late_dropped, f"late drops differ at step {step}"
        f.step(exp)
    g.process_watermark(JMAX)
    o.process_watermark(JMAX)
    exp = o.take_rows()
    assert_rows_equal(g.take_rows(), exp, cfg["val_type"], "final")
    f.step(exp)
    f.late = o.late_dropped
    g.close()
    o.close()
    f.check(kw, negative)


WINDOWED_CASES = [
    ("tumble_off-300_tz+8h", cfg_of("tumble", 1000, vt="i64", offset=-300, tz=8 * H)),
    ("hop_off+250_tz+8h", cfg_of("hop", 3000, 1000, vt="i64", offset=250, tz=8 * H)),
    ("cumulate_off-999_tz+8h", cfg_of("cumulate", 4000, 1000, vt="i64", offset=-999, tz=8 * H)),
    ("cumulate_tz+8h", cfg_of("cumulate", 4000, 1000, vt="i64", tz=8 * H)),
]


@pytest.mark.parametrize("name,cfg", WINDOWED_CASES, ids=[c[0] for c in WINDOWED_CASES])
def test_offsets_windowed_input(oracle_mod, name, cfg):
    run_windowed(oracle_mod, cfg, kw_of())


# ---- 4. across epoch 0 ---------------------------------------------------------------------------
# (cfg, stream overrides, clamp) -- clamp: watermarks raised to -slice. The tz=-8h case starts
# at a positive epoch (local ends negative), so it needs none.
EPOCH0_SQL = [
    ("tumble", cfg_of("tumble", 1000, vt="i64"), dict(t0=-6000), True),
    ("tumble_off-300", cfg_of("tumble", 1000, vt="i64", offset=-300), dict(t0=-6000), True),
    ("hop", cfg_of("hop", 3000, 1000, vt="i64"), dict(t0=-6000), True),
    # (cumulate: inside the first cumulative window below zero. From one window further down the
    # reference's getWindowStart, a truncated remainder, puts a window's start above its end;
    # that is not matched -- DESIGN.md, divergences)
    ("cumulate", cfg_of("cumulate", 4000, 1000, vt="i64"), dict(t0=-3500), True),
    ("cumulate_off-999", cfg_of("cumulate", 4000, 1000, vt="i64", offset=-999), dict(t0=-3500), True),
    ("tumble_tz-8h", cfg_of("tumble", 1000, vt="i64", tz=-8 * H), dict(t0=8 * H - 6000), False),
]
# (DataStream sliding windows are left out below zero: there the reference's assigner starts
# from a window that begins after the element and puts it into size / slide + 1 windows, which
# is not matched -- DESIGN.md, divergences)
EPOCH0_DS = [
    ("ds_tumble", cfg_of("tumble", 1000, vt="i64", mode="datastream"), dict(t0=-6000), True),
]


def floor_of(cfg, clamp):
    return -slice_of(cfg) if clamp else None


@pytest.mark.parametrize("name,cfg,over,clamp", EPOCH0_SQL + EPOCH0_DS, ids=[c[0] for c in EPOCH0_SQL + EPOCH0_DS])
def test_across_epoch_zero(oracle_mod, name, cfg, over, clamp):
    run_single(oracle_mod, cfg, kw_of(**over), wm_floor=floor_of(cfg, clamp), negative=True)


@pytest.mark.parametrize("name,cfg,over,clamp", EPOCH0_SQL, ids=[c[0] for c in EPOCH0_SQL])
def test_across_epoch_zero_two_phase(oracle_mod, name, cfg, over, clamp):
    """Partial rows of negative slice ends: classified under their slice's start
    (pseudo_rowtime, fg_window.h), they keep their slice."""
    if name == "tumble_off-300":
        # at t0 -6000 the global operators, which drop every partial row that arrives after its
        # slice fired, give rows in 2 steps only; 1 s later in 3
        over = dict(over, t0=-5000)
    run_two_phase(oracle_mod, cfg, kw_of(**over), wm_floor=floor_of(cfg, clamp), negative=True)


@pytest.mark.parametrize("name,cfg,over,clamp", EPOCH0_SQL, ids=[c[0] for c in EPOCH0_SQL])
def test_across_epoch_zero_windowed_input(oracle_mod, name, cfg, over, clamp):
    """Windowed rows of negative window ends keep their window."""
    run_windowed(oracle_mod, cfg, kw_of(**over), wm_floor=floor_of(cfg, clamp), negative=True)


# ---- 5. borders of the 32-bit rowtime fast path --------------------------------------------------
FAST_PATH_CASES = [
    # the anchor minus its 2^30 margin lies below the offset: the handle starts on the exact
    # path and enters the fast path after about 3 s of stream
    ("enter_fast_path", cfg_of("tumble", 1000, vt="i64"), dict(t0=(1 << 30) - 3000)),
    ("enter_fast_path_off+700", cfg_of("tumble", 1000, vt="i64", offset=700), dict(t0=(1 << 30) - 3000)),
    # |t| >= 2^52: floor_div_fast falls back to the integer division (late records, exact path)
    ("across_2^52", cfg_of("tumble", 1000, vt="i64"), dict(t0=(1 << 52) - 3000)),
    ("ds_across_2^52", cfg_of("tumble", 1000, vt="i64", mode="datastream"), dict(t0=(1 << 52) - 3000)),
    # (DataStream below zero: its operator has no trigger grid, so no watermark floor)
    # (below zero the truncated remainder puts a record into the window that starts at or after
    # it, one window later than above zero: the jitter grows by a window to hold late records)
    ("ds_across_-2^52", cfg_of("tumble", 1000, vt="i64", mode="datastream"), dict(t0=-(1 << 52) - 3000, jitter=2500)),
    # a slice of 1 ms: fast path off (S < 2)
    ("tumble_1ms", cfg_of("tumble", 1, vt="i64"), dict(n=4_000, batch=500, rate_per_ms=200, jitter=5, delay=2)),
    # a slice of 2^32 + 5 ms: fast path off (S >= 2^32); about three and a half windows
    ("tumble_2^32+5ms", cfg_of("tumble", (1 << 32) + 5, vt="i64"),
     dict(rate_per_ms=24_000 / (3.5 * ((1 << 32) + 5)), jitter=0, delay=0)),
]


@pytest.mark.parametrize("name,cfg,over", FAST_PATH_CASES, ids=[c[0] for c in FAST_PATH_CASES])
def test_fast_path_borders(oracle_mod, name, cfg, over):
    run_single(oracle_mod, cfg, kw_of(**over), negative=name.startswith("ds_") and over["t0"] < 0)
