"""The launch plan of the flush and fire paths, pinned: for fixed inputs, which kernel class runs
how often, over how many records, and which class is credited with the fired rows
(fg_kernel_stats: launches, records, rows per class). These are host decisions of fg_engine.cpp's
merge-job machinery (flush_lanes, fire_one, the region retry), so they are exact: a change that
moves a lane to another path, launches once more or credits another class fails here even when
the rows still equal the oracle's (drive_both asserts those too)."""
import pytest

from tests.test_gpu_parity import LATENESS_CASES, cfg_of, drive_both

pytestmark = pytest.mark.gpu

INORDER = dict(n=300_000, keys=50_000, batch=100_000, rate_per_ms=100, delay=0, jitter=0)
ZIPF = dict(n=2_000_000, keys=200_000, batch=1_000_000, rate_per_ms=1_000, zipf=1.3, delay=0, jitter=0)

# name -> (config, stream, environment, classes that must have launched, classes that must not)
CASES = {
    "tumble_tile_fire": (cfg_of("tumble", 1000), INORDER, {}, ("tile_fire",), ()),
    # the same stream with tile staging off. (No FG_TILE knob is read any more, so the switch the
    # engine does have: keys spread over 64 bits -- the first pass 1 meets a wide key and tile
    # staging ends for good: wide staging, the two-pass partition, the merge that flushes and fires.)
    "tumble_merge_fire": (cfg_of("tumble", 1000), dict(INORDER, key_spread=True), {},
                          ("ingest_part2", "merge_flush_fire"), ("tile_fire",)),
    "tumble_ooo_flush": (cfg_of("tumble", 1000, vt="i64"), dict(n=200_000, keys=3000, batch=7_000, delay=300, jitter=900),
                         {}, ("merge_flush", "merge_flush_fire"), ()),
    "hop_tile_flush": (cfg_of("hop", 1000, 250), INORDER, {}, ("tile_flush", "merge_fire"), ()),
    "cumulate_fused": (cfg_of("cumulate", 1000, 250), INORDER, {}, ("tile_fire",), ()),
    # the smallest stream of test_datastream_allowed_lateness_parity: fired windows keep their state
    # (allowed lateness), which the compact merge does not write back -- the wide merge fires them
    "ds_lateness_retained": (LATENESS_CASES[0][1], LATENESS_CASES[0][2], {}, ("merge_flush_fire",), ()),
    "zipf_split": (cfg_of("tumble", 1000), ZIPF, {}, ("tile_split_fire",), ("merge_heavy",)),
    "zipf_heavy": (cfg_of("tumble", 1000), ZIPF, {"FG_TILE_SPLIT": "0"}, ("merge_heavy",), ("tile_split_fire",)),
    # 2^8 regions: 64 buckets per lane, fewer than the CUs, and slices of 500k records (> 2^18)
    "spread": (cfg_of("tumble", 1000), dict(n=1_000_000, keys=6_000, batch=500_000, rate_per_ms=500, delay=0, jitter=0),
               {"FG_MIN_REGION_BITS": "8"}, ("tile_split_fire",), ()),
    # test_regions_split_on_overflow[tumble]: an operator sized for 1,000 keys takes 400k
    "region_retry": (cfg_of("tumble", 1000), dict(n=800_000, keys=400_000, batch=100_000, delay=100, jitter=300,
                                                  expected_keys=1000), {}, ("merge_flush_fire",), ()),
}


def launch_plan(oracle_mod, name, setenv):
    """Drive case `name` (rows checked against the oracle) and return its launch plan:
    {class: (launches, records, rows)} of every class, and the handle's stats."""
    cfg, kw, env, _, _ = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    ks, st = {}, {}
    drive_both(oracle_mod, cfg, kstats=ks, stats=st, **kw)
    return {c: (v["launches"], v["records"], v["rows"]) for c, v in ks.items()}, st


# {class: (launches, records, rows)}; a class not listed is (0, 0, 0). Captured by running
# launch_plan on the parent of the commit that added this file (291d742, "Window Top-N on the GPU:
# fg_set_fired_topn returns n rows per window"), twice: both runs gave the same values for every
# class of every case, so every class is pinned. (The rows of a split fire are credited to
# tile_fire, the class of its job.)
PLANS = {
    "tumble_tile_fire": {"ingest_scan": (3, 0, 0), "tile_part1": (3, 300000, 0), "tile_fire": (3, 300000, 129593)},
    "tumble_merge_fire": {"ingest_scan": (4, 0, 0), "ingest_part1": (3, 300000, 0), "ingest_part2": (3, 300000, 0),
                          "merge_flush_fire": (3, 300000, 129593), "tile_part1": (1, 100000, 0)},
    "tumble_ooo_flush": {"ingest_count": (29, 200000, 0), "ingest_scan": (29, 0, 0), "ingest_scatter": (29, 200000, 0),
                         "merge_flush": (1, 63691, 0), "merge_flush_fire": (3, 101935, 9000)},
    "hop_tile_flush": {"ingest_scan": (3, 0, 0), "merge_fire": (15, 0, 569167), "tile_part1": (3, 300000, 0),
                       "tile_flush": (12, 300000, 0)},
    "cumulate_fused": {"ingest_scan": (3, 0, 0), "merge_fire": (8, 0, 297463), "tile_part1": (3, 300000, 0),
                       "tile_fire": (4, 100000, 102123), "tile_flush": (8, 200000, 0)},
    "ds_lateness_retained": {"ingest_count": (20, 142551, 0), "ingest_scan": (20, 0, 0),
                             "ingest_scatter": (20, 142551, 0), "merge_flush_fire": (4, 99561, 11458)},
    "zipf_split": {"ingest_scan": (2, 0, 0), "tile_part1": (2, 2000000, 0), "tile_fire": (0, 0, 70767),
                   "tile_split_fire": (2, 2000000, 0)},
    "zipf_heavy": {"ingest_scan": (3, 0, 0), "ingest_part1": (2, 2000000, 0), "ingest_part2": (2, 2000000, 0),
                   "merge_flush_fire": (2, 2000000, 70767), "merge_heavy": (4, 0, 0), "tile_part1": (1, 1000000, 0)},
    "spread": {"ingest_scan": (2, 0, 0), "tile_part1": (2, 1000000, 0), "tile_fire": (0, 0, 12000),
               "tile_split_fire": (2, 1000000, 0)},
    "region_retry": {"ingest_count": (8, 800000, 0), "ingest_scan": (8, 0, 0), "ingest_scatter": (8, 800000, 0),
                     "merge_flush_fire": (14, 800000, 711055), "merge_heavy": (2, 0, 0)},
}
# region_retry: the regions the retries grew the operator to, and its flushes (the parent's).
# fg_stats carries no count of the grows: the operator starts at one region (expected_keys=1000)
# and every grow doubles them, so state_regions is 2^grows.
RETRY_STATS = {"state_regions": 32, "flushes": 9}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_plan(oracle_mod, monkeypatch, name):
    plan, st = launch_plan(oracle_mod, name, monkeypatch.setenv)
    print(name, plan, st)
    for c in CASES[name][3]:
        assert plan[c][0] > 0, f"{name}: no {c} launch -- the shape left its path: {plan}"
    for c in CASES[name][4]:
        assert plan[c][0] == 0, f"{name}: {c} launched: {plan}"
    want = PLANS[name]
    assert {c: v for c, v in plan.items() if v != (0, 0, 0)} == want, \
        {c: (plan.get(c), want.get(c, (0, 0, 0))) for c in set(plan) | set(want) if plan.get(c) != want.get(c, (0, 0, 0))}
    if name == "region_retry":
        assert st["state_regions"] > 1, st
        assert {k: st[k] for k in RETRY_STATS} == RETRY_STATS, (st, RETRY_STATS)
