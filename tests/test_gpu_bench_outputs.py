"""bench.py --dump-outputs: the rows the last timed step fired, written as float64 columns.

A small configs[1]-shaped job (1M records, 20k keys, 4 windows of 1 s, 250k-record micro-batches,
asynchronous watermarks: the path the bench times; its row bound of 48 B x 1M records fits the
dump budget, so every row is written) run through bench.main() in this process. The
dumped rows are compared, every one, with the oracle over the same records; a second run with a
dump budget that does not hold a step's rows must write exactly the rows of the first whose key
the sample's hash keeps, in the same order.

Tolerance: keys, windows and COUNT(*) exact; DOUBLE SUM / AVG within 1e-9 relative (the GPU sums
a (key, window) in another order than the oracle's arrival order; north_star)."""
import contextlib
import io
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, KEYS, RATE, BATCH, WM_EVERY = 1_000_000, 20_000, 250_000, 250_000, 50_000
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--records", str(N), "--keys", str(KEYS), "--rate", str(RATE),
        "--batch", str(BATCH), "--wm-every", str(WM_EVERY)]
COLUMNS = ["key", "window_start", "window_end", "count_star", "sum", "avg"]


def run_bench(out_dir):
    """bench.main() with ARGS --dump-outputs out_dir; returns (result line, {column: array})"""
    import bench
    argv, buf = sys.argv, io.StringIO()
    sys.argv = ["bench.py"] + ARGS + ["--dump-outputs", str(out_dir)]
    try:
        with contextlib.redirect_stdout(buf):
            bench.main()
    finally:
        sys.argv = argv
    res = json.loads(buf.getvalue().strip().splitlines()[-1])
    return res, {c: np.load(out_dir / (c + ".npy")) for c in COLUMNS}


@pytest.fixture(scope="module")
def full_dump(tmp_path_factory):
    return run_bench(tmp_path_factory.mktemp("dump"))


def test_result_line_and_files(full_dump):
    res, cols = full_dump
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(N / (res["ms_per_step"] / 1e3), rel=1e-9)
    assert res["cpu_baseline"] is None and "h2d" not in res and res["roofline"]["copy_peak_gbs"] is None
    out = res["outputs"]
    assert out["columns"] == COLUMNS and out["key_fraction"] == 1.0
    assert out["rows"] > 0 and out["rows"] * res["steps"] == res["rows_fired"]
    for c in COLUMNS:
        assert cols[c].dtype == np.float64 and cols[c].shape == (out["rows"],)
    order = np.lexsort((cols["key"], cols["window_start"], cols["window_end"]))
    assert np.array_equal(order, np.arange(out["rows"])), "rows sorted by (window_end, window_start, key)"


def test_rows_match_the_oracle(full_dump, oracle_mod):
    import torch

    import bench
    O = oracle_mod
    _, cols = full_dump
    key, ts, val = (x.cpu().numpy() for x in bench.gen_columns(N, KEYS, RATE, 0, torch.device("cuda", 0)))
    wm_at, wm_val = [], []
    for lo in range(0, N, BATCH):   # the bench's schedule: a batch, then the watermarks that fall in it
        wms = bench.watermarks_for(lo, lo + BATCH, RATE, WM_EVERY)
        wm_at += [lo + BATCH] * len(wms)
        wm_val += wms
    wm_at.append(N)
    wm_val.append(bench.JMAX)
    cfg = O.Config(O.MODE_SQL, O.TUMBLE, 1000, 0, 0, 0, O.VAL_F64, 0)
    exp, late, _ = O.run_partitioned_rows(cfg, 4, 128, key, ts, val, np.array(wm_at, dtype=np.int64),
                                          np.array(wm_val, dtype=np.int64))
    assert late == 0 and len(exp) == len(cols["key"])
    e = exp[np.lexsort((exp["key"], exp["window_start"], exp["window_end"]))]
    for c, ec in (("key", "key"), ("window_start", "window_start"), ("window_end", "window_end"),
                  ("count_star", "cnt_star")):
        assert np.array_equal(cols[c], e[ec].astype(np.float64)), c
    for c, ec in (("sum", "sum_d"), ("avg", "avg_d")):
        assert not np.isnan(cols[c]).any() and not e[ec.replace("_d", "_null")].any()
        assert np.allclose(cols[c], e[ec], rtol=1e-9, atol=0), c


def test_sample_of_a_larger_output(full_dump, tmp_path, monkeypatch):
    """A budget that holds an eighth of a step's row bound (48 B x 1M records): the rows of the
    keys whose hash falls in the lowest eighth, as the full dump has them."""
    import bench
    _, full = full_dump
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 << 20)
    res, cols = run_bench(tmp_path)
    assert res["outputs"]["key_fraction"] == 1 / 8
    with np.errstate(over="ignore"):
        h = (full["key"].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(24)
    keep = h < np.uint64(1 << 37)
    assert 0 < keep.sum() < len(keep)
    for c in ("key", "window_start", "window_end", "count_star"):
        assert np.array_equal(cols[c], full[c][keep]), c
    for c in ("sum", "avg"):
        assert np.allclose(cols[c], full[c][keep], rtol=1e-9, atol=0), c
