"""CPU-side checks of the late-element side output (fg_set_late_output, fg_collect_late): the C-ABI
is exported, bound and documented with ABI 16 unchanged, the JNI glue compiles with the two new
natives, the Python operators carry the new surface -- and the numpy reference the GPU tests compare
with (tests/late_reference.dropped_mask, written from WindowOperator) is pinned to the oracle on every
stream those tests use."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from flink_amd import _lib as L
from flink_amd.datastream import DataStreamWindowOperator
from flink_amd.window_agg import WindowAggOperator
from tests.fixture_runner import KIND, load_operator_cases
from tests.late_reference import dropped_mask
from tests.late_streams import CONFIGS, batches_of, stream_of
from tests.streams import make_stream
from tests.test_abi import HEADER, ROOT, declared_symbols

NEW = ("fg_set_late_output", "fg_collect_late")
JMIN = -(1 << 63)


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for s in NEW:
        assert s in L.EXPORTS and s in declared_symbols(), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).restype is C.c_int, s
    assert list(lib.fg_set_late_output.argtypes) == [C.c_void_p, C.c_int32]
    assert list(lib.fg_collect_late.argtypes) == [C.c_void_p, C.c_int32, C.POINTER(L.FgLateRecords)]
    assert lib.fg_abi_version() == 16


def test_symbols_are_in_the_map_file():
    src = open(os.path.join(ROOT, "flink_amd", "csrc", "libflinkgpu.map")).read()
    glob = src[src.index("global:"):src.index("local:")]
    for s in NEW:
        assert re.search(r"\b%s;" % s, glob), s


def test_late_records_layout_matches_header(tmp_path):
    fields = [f for f, _ in L.FgLateRecords._fields_]
    assert fields == ["n", "location", "reserved0", "key", "rowtime", "val", "val_null"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flinkgpu.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(fg_late_records));']
    src += [f'printf("{f} %zu\\n", offsetof(fg_late_records, {f}));' for f in fields]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.FgLateRecords)
    for f in fields:
        assert int(got[f]) == getattr(L.FgLateRecords, f).offset, f


def test_header_documents_them():
    src = open(HEADER).read()
    doc = src[src.index("Late elements as a side output (ABI 16, added"):src.index("int  fg_set_late_output")]
    for word in NEW + ("FG_EINVAL", "FG_ESTATE", "FG_MODE_DATASTREAM", "FG_FLAG_LOCAL_PARTIALS", "FG_FLAG_PROCTIME",
                       "FG_FLAG_WINDOWED", "fg_late_dropped", "arrival order", "fg_add_rows", "fg_reset", "fg_restore",
                       "before it forwards a watermark", "late output and ingest disagree", "typedef struct fg_late_records"):
        assert word in doc, word
    assert "#define FG_ABI_VERSION 16" in src


def test_null_handles_are_refused():
    lib = L.load()
    assert lib.fg_set_late_output(None, 1) == L.FG_EINVAL
    assert lib.fg_set_late_output(None, 0) == L.FG_EINVAL
    assert lib.fg_collect_late(None, L.HOST, C.byref(L.FgLateRecords())) == L.FG_EINVAL


def test_operator_surface():
    for m in ("set_late_output", "collect_late"):
        assert callable(getattr(WindowAggOperator, m)), m
    assert inspect.signature(WindowAggOperator.__init__).parameters["late_output"].default is False
    assert inspect.signature(WindowAggOperator.collect_late).parameters["host"].default is True
    assert inspect.signature(DataStreamWindowOperator.__init__).parameters["late_output"].default is False
    assert callable(DataStreamWindowOperator.late_records)


def test_jni_glue_compiles_and_exports_the_natives(tmp_path):
    so = str(tmp_path / "libflinkgpujni.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "tests", "jni_stub"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "flink_gpu_jni.c"), "-o", so], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    pre = "Java_org_apache_flink_table_runtime_operators_window_gpu_FlinkGpu_"
    for nat in ("setLateOutput", "collectLate"):
        assert re.search(r"\bT %s%s\b" % (pre, nat), syms), nat
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    for s in NEW:
        assert re.search(r"\bU %s\b" % s, und), s
    jroot = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink")
    java = open(os.path.join(jroot, "table", "runtime", "operators", "window", "gpu", "FlinkGpu.java")).read()
    assert "public static native void setLateOutput(long h, boolean on);" in java
    assert "public static native long[] collectLate(long h);" in java
    op = open(os.path.join(jroot, "streaming", "runtime", "operators", "windowing", "gpu", "GpuWindowOperator.java")).read()
    for word in ("OutputTag<Tuple2<Long, V>> lateDataOutputTag", "FlinkGpu.setLateOutput(handle, true)",
                 "FlinkGpu.collectLate(handle)", "output.collect(lateDataOutputTag, new StreamRecord<>("):
        assert word in op, word


# ---- the reference mask against the oracle ------------------------------------------------------

def oracle_of(O, window, lateness, purging, val_type):
    return O.OracleOperator(mode=O.MODE_DATASTREAM, kind=KIND[window[0]], size=window[1],
                            slide=window[2] if window[0] == "hop" else 0,
                            val_type={"none": O.VAL_NONE, "i64": O.VAL_I64, "f64": O.VAL_F64}[val_type],
                            count_star_index=-1, allowed_lateness=lateness, purging=purging)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_mask_counts_what_the_oracle_drops(name):
    """per batch of every GPU-test stream: the mask's count is the increment of the oracle's
    numLateRecordsDropped; and the streams are mixed -- 5 % to 95 % of every batch that follows a
    watermark is late"""
    from oracle import oracle as O
    c = CONFIGS[name]
    key, ts, val, isnull = stream_of(name)
    o = oracle_of(O, c["window"], c["lateness"], c["purging"], c["val_type"])
    progress, seen, shares = JMIN, 0, []
    for lo, hi, wm in batches_of(name, ts):
        m = dropped_mask(ts[lo:hi], progress, c["window"], c["lateness"], c["purging"])
        o.process_batch(key[lo:hi], ts[lo:hi], None if val is None else val[lo:hi], None if isnull is None else isnull[lo:hi])
        assert o.late_dropped - seen == int(m.sum()), (name, lo)
        seen = o.late_dropped
        if progress != JMIN:
            shares.append(m.mean())
        o.process_watermark(wm)
        o.take_rows()
        progress = max(progress, wm)
    o.close()
    assert len(shares) >= 5
    assert 0.05 <= min(shares) and max(shares) <= 0.95, (name, shares)


@pytest.mark.parametrize("window", [("tumble", 2000), ("hop", 3000, 1000)], ids=["tumble2s", "hop3s1s"])
@pytest.mark.parametrize("lateness", [0, 500])
@pytest.mark.parametrize("purging", [False, True])
def test_mask_agrees_with_the_oracle_element_by_element(window, lateness, purging):
    """300 elements, one per batch, a watermark after every third"""
    from oracle import oracle as O
    key, tj, val, _ = make_stream(300, 5, "i64", t0=0, rate_per_ms=1, jitter_ms=9000, seed=77)
    step = np.arange(300, dtype=np.int64)
    ts = 1_000_000 + 20 * step + (tj - step)   # 6 s of stream time, each element up to 9 s ahead of it
    o = oracle_of(O, window, lateness, purging, "i64")
    progress, late = JMIN, 0
    for i in range(300):
        m = bool(dropped_mask(ts[i:i + 1], progress, window, lateness, purging)[0])
        o.process_batch(key[i:i + 1], ts[i:i + 1], val[i:i + 1], None)
        assert (o.late_dropped - late == 1) == m, (i, int(ts[i]), progress)
        late = o.late_dropped
        if i % 3 == 2:
            wm = int(ts[:i + 1].max()) - 2500
            o.process_watermark(wm)
            o.take_rows()
            progress = max(progress, wm)
    o.close()
    assert 30 <= late <= 270   # both answers occur


GOLDEN_LATE = {   # the elements WindowOperatorTest expects in the side output: (key, value, timestamp)
    "ds_tumble_2s_lateness0_side_output": [(2, 1, 1998)],
    "ds_sliding_3s_1s_lateness0_side_output": [(1, 1, 3001)],
    "ds_tumble_2s_lateness500_purging": [(2, 1, 1998)],
}


def window_of_case(cfg):
    return ("tumble", cfg["size"]) if cfg["kind"] == "tumble" else ("hop", cfg["size"], cfg["slide"])


def golden_late_elements(case):
    """the reference mask over the case's events, element by element"""
    cfg = case["config"]
    progress, out = JMIN, []
    for e in case["events"]:
        if e[0] == "wm":
            progress = max(progress, e[1])
        elif e[0] == "e":
            if dropped_mask(np.array([e[3]], dtype=np.int64), progress, window_of_case(cfg),
                            cfg.get("allowed_lateness", 0), cfg.get("purging", False))[0]:
                out.append((e[1], e[2], e[3]))
    return out


@pytest.mark.parametrize("name", list(GOLDEN_LATE))
def test_mask_gives_the_golden_side_output(name):
    case = next(c for c in load_operator_cases() if c["name"] == name)
    got = golden_late_elements(case)
    assert got == GOLDEN_LATE[name]
    assert len(got) == case["expected_late_dropped"]
    if name == "ds_sliding_3s_1s_lateness0_side_output":   # the final (1, 1, 3001), not the two before WM 6000
        last = max(i for i, e in enumerate(case["events"]) if e[0] == "e")
        assert tuple(case["events"][last][1:4]) == got[0]
