"""GPU tests of fg_key_dict_retain / fg_key_dict_get_stats: keep the listed ids, retire every other
entry, compact the arena, rebuild the table, reuse the retired ordinals -- on dictionaries that each
hold one ~5,000-byte row among rows of 24-64 bytes, under forced tag collisions, after errors, under
the window engine against the oracle, and through the shim's checkpoint policy (keyed_state)."""
import struct

import numpy as np
import pytest

import flink_amd as F
from flink_amd import _lib as L
from flink_amd import keys as K
from tests.test_gpu_keys import MAXP, TYPES, check_interned, random_keys

pytestmark = pytest.mark.gpu

KG_BITS = K.dict_kg_bits(MAXP)
LONG_ROW = K.key_row(["x" * 4990, 7], TYPES)   # 24 + 4992 bytes: far larger than its neighbours
_ROWS = {}


def base_rows(n=40_000):
    """the key rows of random_keys(seed 3, 40,000), computed once for the module"""
    if "rows" not in _ROWS:
        _ROWS["rows"] = [K.key_row(list(k), TYPES) for k in random_keys(np.random.default_rng(3), 40_000)]
    return _ROWS["rows"][:n]


def entry_bytes(rows):
    return sum(8 + ((len(r) + 7) & ~7) for r in rows)


def ordinals(ids):
    return np.asarray(ids, dtype=np.int64) >> KG_BITS


@pytest.mark.parametrize("where", ["host", "device"])
def test_keep_half(where):
    rng = np.random.default_rng(21)
    rows = base_rows() + [LONG_ROW]
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=1000)   # the table has grown
    ids, _ = d.intern(rows)
    st0 = d.stats()
    assert st0["live"] == st0["issued"] == len(d) == 40_001 and st0["free_ordinals"] == st0["retired_total"] == 0
    assert st0["arena_bytes"] == entry_bytes(rows) and st0["table_slots"] > 2048
    keep = np.zeros(len(rows), dtype=bool)
    keep[rng.permutation(40_000)[:20_000]] = True
    keep[-1] = True   # the long row moves: entries before it die
    kept_ids, dead_ids = ids[keep], ids[~keep]
    kept_rows = [r for r, k in zip(rows, keep) if k]
    dead_rows = [r for r, k in zip(rows, keep) if not k]
    if where == "device":
        import torch
        st = d.retain(torch.from_numpy(kept_ids).to(torch.device("cuda", 0)))
    else:
        st = d.retain(kept_ids)
    assert st == d.stats()
    assert st["live"] == len(d) == 20_001 and st["retired_total"] == 20_000 and st["free_ordinals"] == 20_000
    assert st["issued"] == st0["issued"]
    assert st["arena_bytes"] == entry_bytes(kept_rows)
    assert st["table_slots"] <= st0["table_slots"]
    # kept ids keep their rows and their ids
    assert d.lookup(kept_ids) == kept_rows
    again, kgs = d.intern(kept_rows)
    assert np.array_equal(again, kept_ids)
    check_interned(d, kept_rows, again, kgs)
    assert d.stats() == st   # (nothing was new)
    # retired ids are unknown
    with pytest.raises(KeyError):
        d.rows(dead_ids[:100])
    with pytest.raises(KeyError):
        d.rows(np.concatenate([kept_ids[:50], dead_ids[-1:]]))
    # their rows are new keys, on reused ordinals
    new_ids, kgs = d.intern(dead_rows)
    assert len(set(new_ids.tolist())) == 20_000
    assert not set(new_ids.tolist()) & set(kept_ids.tolist())
    assert ordinals(new_ids).max() < st0["issued"]
    assert sorted(ordinals(new_ids).tolist()) == sorted(ordinals(dead_ids).tolist())   # the 20,000 free ones
    check_interned(d, dead_rows, new_ids, kgs)
    assert d.lookup(kept_ids) == kept_rows
    st2 = d.stats()
    assert st2["live"] == 40_001 and st2["issued"] == st0["issued"] and st2["free_ordinals"] == 0
    assert st2["arena_bytes"] == entry_bytes(rows) and st2["retired_total"] == 20_000
    d.close()


def test_churn_stays_bounded():
    base = base_rows()[:25_000]
    assert all(len(r) >= 24 for r in base)

    def fresh(rnd, count):   # rows never seen before: the BIGINT field (-5..4) of a base row moved by 100 per round
        return [r[:16] + struct.pack("<q", struct.unpack("<q", r[16:24])[0] + 100 * (rnd + 1)) + r[24:]
                for r in base[:count]]

    d = F.KeyDictionary(max_parallelism=MAXP)
    carried, slots1, seen, peak = [], None, set(), 0
    alive = set()
    for rnd in range(30):
        rows = carried + (fresh(rnd, 20_000) if rnd else [LONG_ROW] + fresh(rnd, 24_999))
        assert len(rows) == 25_000 and not set(rows[len(carried):]) & seen
        seen.update(rows)
        peak = max(peak, len(alive | set(rows)))   # alive after this intern, before the retain
        ids, _ = d.intern(rows)
        st = d.retain(ids)
        alive = set(rows)
        assert st["live"] == len(d) == 25_000, rnd
        assert st["arena_bytes"] == entry_bytes(rows), rnd
        slots1 = slots1 or st["table_slots"]
        assert st["table_slots"] <= slots1, rnd
        assert st["issued"] <= peak, (rnd, st)
        assert d.lookup(ids) == rows, rnd
        carried = [LONG_ROW] + rows[-4_999:]
    assert peak == 45_000 and len(seen) == 605_000
    st = d.stats()
    assert st["issued"] <= 45_000 and st["retired_total"] == 580_000
    d.close()


def test_forced_tag_collisions(monkeypatch):
    """6-bit tags: nearly every row is resolved on the host behind the row holding its tag; halving
    the dictionary kills holders whose side rows live, and side rows whose holders live"""
    monkeypatch.setenv("FG_DICT_TAG_BITS", "6")
    rng = np.random.default_rng(13)
    rows_all = base_rows(2_999) + [LONG_ROW]
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=16)
    ids, kgs = d.intern(rows_all)
    live = check_interned(d, rows_all, ids, kgs)
    assert d.stats()["side_rows"] > 2_000
    for rnd in range(3):
        rows = sorted(live)
        keep = rng.random(len(rows)) < 0.5
        kept = [r for r, k in zip(rows, keep) if k]
        gone = [r for r, k in zip(rows, keep) if not k]
        st = d.retain(np.array([live[r] for r in kept], dtype=np.int64))
        assert st["live"] == len(kept) and st["arena_bytes"] == entry_bytes(kept), rnd
        assert st["side_rows"] < len(kept), rnd   # (at least one row per tag is in the table)
        again, kgs = d.intern(kept)
        assert again.tolist() == [live[r] for r in kept], rnd   # every kept row keeps its id
        m = check_interned(d, kept, again, kgs)                  # ... and no two live rows share one
        assert d.stats()["live"] == len(kept), rnd               # (no row was interned a second time)
        new_ids, kgs2 = d.intern(gone)
        assert not set(new_ids.tolist()) & set(m.values()), rnd
        m2 = check_interned(d, gone, new_ids, kgs2)
        live = {**m, **m2}
        both, kgs3 = d.intern(rows)
        assert check_interned(d, rows, both, kgs3) == live, rnd
        assert len(d) == len(rows) == 3_000
    d.close()


def test_errors_leave_it_unchanged():
    import torch
    rows = base_rows(5_000) + [LONG_ROW]
    d = F.KeyDictionary(max_parallelism=MAXP)
    ids, _ = d.intern(rows)
    kept_ids, kept_rows = ids[1_000:], rows[1_000:]
    d.retain(kept_ids[:2_000], kept_ids[2_000:])   # two sets
    retired = ids[:1_000]
    st = d.stats()
    assert st["live"] == 4_001 and st["free_ordinals"] == 1_000

    def unchanged():
        assert d.stats() == st and len(d) == 4_001
        assert d.lookup(kept_ids) == kept_rows

    for bad in (-5, ((st["issued"] + 7) << KG_BITS) | 3, int(retired[17])):
        second = kept_ids[:500].copy()
        second[[17, 400]] = bad
        with pytest.raises(F.WindowSpecError, match=r"fg_key_dict_retain: 2 ids .* set 1 index 17\b"):
            d.retain(kept_ids, second)
        unchanged()
        with pytest.raises(F.WindowSpecError, match=r"fg_key_dict_retain: 1 ids .* set 0 index 4000\b"):
            d.retain(torch.from_numpy(np.append(kept_ids[:4_000], bad)).cuda())
        unchanged()
    # a stale id: the right ordinal under another key group
    stale = int(kept_ids[9]) ^ 1
    with pytest.raises(F.WindowSpecError, match=r"1 ids .* set 0 index 0\b"):
        d.retain(np.array([stale], dtype=np.int64))
    unchanged()
    # while an async intern is pending
    buf, off, ln = K.pack_key_rows(kept_rows[:100])
    dev = torch.device("cuda", 0)
    d.intern_async((torch.from_numpy(buf.copy()).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(ln).to(dev)))
    with pytest.raises(F.FlinkGpuError) as e:
        d.retain(kept_ids)
    assert e.value.code == L.FG_ESTATE
    d.intern_wait()
    unchanged()
    # no ids: the dictionary is emptied and interns again from ordinal 0
    st = d.retain()
    assert st["live"] == len(d) == 0 and st["arena_bytes"] == 0 and st["free_ordinals"] == st["issued"]
    assert st["retired_total"] == 5_001
    with pytest.raises(KeyError):
        d.rows(kept_ids[:10])
    ids2, kgs = d.intern(rows[:300])
    assert sorted(ordinals(ids2).tolist()) == list(range(300))
    check_interned(d, rows[:300], ids2, kgs)
    assert d.retain(np.empty(0, dtype=np.int64))["live"] == 0   # (all counts 0)
    d.close()


def churn_stream(rng, n, batch, rate, span, step):
    """batch b draws its keys from [step b, step b + span); event times as test_string_keys_stream_vs_oracle"""
    pick = np.concatenate([rng.integers(step * b, step * b + span, batch) for b in range(n // batch)])
    ts = (1_000_000 + np.arange(n) // rate + rng.integers(0, 300, n)).astype(np.int64)
    return pick, ts, rng.random(n) * 1000.0


@pytest.mark.parametrize("kind", ["tumble", "hop"])
def test_engine_parity_under_churn(oracle_mod, kind):
    """300,000 records in 50,000-record batches over 40,000 keys, batch b from keys [4000 b, 4000 b + 12,000);
    jitter (0..300 ms) and watermarks (400 ms behind) as test_string_keys_stream_vs_oracle, at 25 records
    per ms: a batch spans 2 s, so slices of the 3 s HOP expire between barriers and keys do retire (at
    that test's 100 per ms the whole stream is 3 s and no HOP slice expires before the last barrier)."""
    from tests.test_gpu_parity import assert_rows_equal, cfg_of, gpu_mk, oracle_mk
    rows_all = base_rows()
    index = {r: i for i, r in enumerate(rows_all)}
    n, batch = 300_000, 50_000
    pick, ts, val = churn_stream(np.random.default_rng(5), n, batch, 25, 12_000, 4_000)
    cfg = cfg_of(kind, 3000 if kind == "hop" else 1000, 1000 if kind == "hop" else 0)
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=12_000)
    g = gpu_mk(cfg, expected_keys=20_000)
    o = oracle_mk(oracle_mod, cfg)

    def check(ctx):
        r = g.take_rows()
        if len(r):
            r["key"] = [index[x] for x in d.lookup(r["key"])]
        assert_rows_equal(r, o.take_rows(), "f64", ctx)

    retired = 0
    for b, lo in enumerate(range(0, n, batch)):
        hi = lo + batch
        ids, _ = d.intern([rows_all[i] for i in pick[lo:hi]])
        g.process_batch(ids, ts[lo:hi], val[lo:hi])
        o.process_batch(pick[lo:hi].astype(np.int64), ts[lo:hi], val[lo:hi])
        wm = int(ts[hi - 1]) - 400
        g.process_watermark(wm)
        o.process_watermark(wm)
        check(f"wm {wm}")   # (fired ids are mapped back before the retain)
        assert g.late_dropped == o.late_dropped, b
        if b % 2 == 1:
            g.op.prepare_snapshot_pre_barrier()
            o.prepare_snapshot()
            img, _ = g.op.snapshot_state()
            st = d.retain(img["key"])
            assert st["live"] == len(np.unique(img["key"])), b
            retired = st["retired_total"]
    assert g.late_dropped == o.late_dropped
    g.process_watermark((1 << 63) - 1)
    o.process_watermark((1 << 63) - 1)
    check("final")
    assert retired > 0
    assert d.stats()["issued"] < len(np.unique(pick))
    g.close()
    o.close()
    d.close()


def test_shim_policy_mirror(oracle_mod):
    """writeKeyedState with flinkgpu.dictRetainFactor = 2 (the live floor lowered for the test): a due
    barrier selects every slice, leaves the backend as a full rewrite does, retains the image's keys;
    the stream goes on to the oracle's rows"""
    from flink_amd.keyed_state import HOP, SliceSpec, WindowAggsState, retain_due
    from tests.test_gpu_parity import assert_rows_equal, cfg_of, gpu_mk, oracle_mk
    rows_all = base_rows()
    index = {r: i for i, r in enumerate(rows_all)}
    n, batch = 160_000, 8_000
    pick, ts, val = churn_stream(np.random.default_rng(5), n, batch, 8, 1_500, 1_900)
    cfg = cfg_of("hop", 3000, 1000)
    spec = SliceSpec(HOP, 3000, 1000)
    shim, full = WindowAggsState(spec), WindowAggsState(spec)
    d = F.KeyDictionary(max_parallelism=MAXP, expected_keys=256)
    g = gpu_mk(cfg, expected_keys=8_000)
    o = oracle_mk(oracle_mod, cfg)
    due_at = []
    for b, lo in enumerate(range(0, n, batch)):
        hi = lo + batch
        ids, _ = d.intern([rows_all[i] for i in pick[lo:hi]])
        g.process_batch(ids, ts[lo:hi], val[lo:hi])
        o.process_batch(pick[lo:hi].astype(np.int64), ts[lo:hi], val[lo:hi])
        wm = int(ts[hi - 1]) - 400
        g.process_watermark(wm)
        o.process_watermark(wm)
        r = g.take_rows()
        if len(r):
            r["key"] = [index[x] for x in d.lookup(r["key"])]
        assert_rows_equal(r, o.take_rows(), "f64", f"step {b}")
        if b % 2 == 0:
            continue
        g.prepare_snapshot()
        o.prepare_snapshot()
        plan, twm = g.op.snapshot_plan()
        shim.advance_watermark(twm)
        full.advance_watermark(twm)
        due = retain_due(d.stats()["live"], int(plan["rows"].sum()), 2, min_live=1_000)
        want = shim.wanted_slices(plan, twm, force_all=due)
        if due:
            due_at.append(b)
            assert want.all() and len(want) == len(plan["slice_end"])
        img, _ = g.op.snapshot_state_select(want)
        img_sl = g.op.snapshot_slices()
        shim.write_delta(img, img_sl, plan, twm)
        if due:   # the image's key column is every id the operator holds
            assert len(img["key"]) == int(plan["rows"].sum())
            st = d.retain(img["key"])
            assert st["live"] == len(np.unique(img["key"])) < 2 * len(img["key"])
        whole, _ = g.op.snapshot_state()
        full.write_image_full(whole, g.op.snapshot_slices(), twm)
        assert shim.entries == full.entries and shim.timers == full.timers, b
    assert due_at and due_at[0] > 1, due_at   # the first barrier is not due; a later one is
    assert not retain_due(1 << 20, 1, 0) and not retain_due((1 << 16) - 1, 1, 2) and retain_due(1 << 16, 1, 2)
    g.process_watermark((1 << 63) - 1)
    o.process_watermark((1 << 63) - 1)
    r = g.take_rows()
    r["key"] = [index[x] for x in d.lookup(r["key"])]
    assert_rows_equal(r, o.take_rows(), "f64", "final")
    assert g.late_dropped == o.late_dropped
    assert d.stats()["issued"] < len(np.unique(pick))
    g.close()
    o.close()
    d.close()
