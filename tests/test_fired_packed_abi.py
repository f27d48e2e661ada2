"""fg_fired_packed (fired rows as packed BinaryRowData rows) at the drop-in boundary, without a
device: the symbol in the header, the map file and the binding, the struct's layout, the header's
contract, flink_amd.rows.unpack_rows as the inverse of pack_rows, and the JNI / Java side."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from flink_amd import _lib as L
from flink_amd import rows as R
from flink_amd.composite import CompositeWindowAggOperator
from flink_amd.window_agg import WindowAggOperator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "flinkgpu.h")).read()
JAVA = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink", "table", "runtime", "operators",
                    "window", "gpu")


def section():
    """the header comment of the new section, whitespace folded"""
    m = re.search(r"/\* Fired rows as packed BinaryRowData rows \(ABI 16, added\).*?\*/", HEADER, re.S)
    assert m, "the section is marked 'ABI 16, added'"
    return re.sub(r"\s*\n \*\s*", " ", m.group(0))


def test_symbol_declared_exported_and_bound():
    assert re.search(r"^int\s+fg_fired_packed\(fg_handle\* h, int64_t first_row, int64_t max_rows, int32_t flags,\s*"
                     r"int32_t out_location, fg_packed_rows\* out\);", HEADER, re.M)
    assert "enum fg_pack_flags { FG_PACK_KEY_FIELD = 1 };" in HEADER
    assert "#define FG_ABI_VERSION 16" in HEADER
    mapf = open(os.path.join(ROOT, "flink_amd", "csrc", "libflinkgpu.map")).read()
    assert re.search(r"^\s*fg_fired_packed;", mapf, re.M)
    assert "fg_fired_packed" in L.EXPORTS and L.PACK_KEY_FIELD == 1
    lib = L.load()
    assert lib.fg_abi_version() == 16
    assert lib.fg_fired_packed.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                            C.POINTER(L.FgPackedRows)]
    assert lib.fg_fired_packed.restype is C.c_int
    syms = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT fg_fired_packed\b", syms)


def test_struct_layout_matches_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flinkgpu.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(fg_packed_rows));']
    for f, _ in L.FgPackedRows._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(fg_packed_rows, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if ln)
    assert int(got["size"]) == C.sizeof(L.FgPackedRows) == 40
    for f, _ in L.FgPackedRows._fields_:
        assert int(got[f]) == getattr(L.FgPackedRows, f).offset, f


def test_null_arguments_are_einval():
    lib = L.load()
    out = L.FgPackedRows()
    assert lib.fg_fired_packed(None, 0, 1, 0, L.HOST, C.byref(out)) == L.FG_EINVAL
    assert lib.fg_fired_packed(None, 0, 1, 0, L.HOST, None) == L.FG_EINVAL


def test_header_section_states_the_contract():
    s = section()
    # the layout
    for phrase in ("little endian", "((arity + 71) / 64) * 8", "RowKind INSERT = 0", "bit 8 + f",
                   "agg[0] .. agg[num_aggs - 1], window_start, window_end", "arity = num_aggs + 2",
                   "calculateFixPartSizeInBytes(arity)", "eight zero bytes", "BinaryRowWriter.setNullAt",
                   "TIMESTAMP(3) compact epoch milliseconds"):
        assert phrase in s, phrase
    # the range, the locations, the errors
    for phrase in ("[first_row, min(first_row + max_rows, N))", "2 GiB", "pinned host memory", "fg_stream",
                   "FG_EINVAL, before any device work", "flag bits other than FG_PACK_KEY_FIELD", "first_row > N",
                   "max_rows < 0", "n * stride >= 2^31 with FG_HOST", "FG_MODE_DATASTREAM", "FG_FLAG_LOCAL_PARTIALS",
                   "FG_ESTATE unless the fired rows are still the ones the last returning call handed back",
                   "uncollected async rows", "fired nothing is valid and gives n = 0", "first_row == N", "max_rows == 0"):
        assert phrase in s, phrase
    # run mode, Top-N, the kernel class and its place
    for phrase in ("Run mode (fg_set_fired_runs)", "uploaded once per call", "one launch covers every run",
                   "Top-N (fg_set_fired_topn): the packed rows are the selected rows",
                   'class "pack_rows": records = rows = rows packed', 'after every other class, "late_out" and "topn" included'):
        assert phrase in s, phrase
    # the sentence an existing test pins stays
    assert 'class follows every other class but "topn" (fg_set_fired_topn)' in HEADER


@pytest.mark.parametrize("arity", [1, 3, 11, 57])
@pytest.mark.parametrize("extra", [0, 16], ids=["fixed", "wider"])
def test_unpack_rows_inverts_pack_rows(arity, extra):
    rng = np.random.default_rng(arity)
    n = 37
    fields = [rng.integers(-2 ** 62, 2 ** 62, n) for _ in range(arity)]
    fields[0] = rng.standard_normal(n)   # (a DOUBLE column: its bits)
    fields[0][:4] = [-0.0, np.nan, np.inf, -np.inf]
    nulls = [rng.random(n) < 0.3 if f % 2 == 0 else None for f in range(arity)]
    stride = R.fixed_part_size(arity) + extra
    buf = R.pack_rows(fields, nulls, stride=stride if extra else None)
    assert buf.size == n * stride and R.bit_set_width(arity) == (16 if arity == 57 else 8)
    got, gnull, kind = R.unpack_rows(buf, arity, stride if extra else None)
    assert len(got) == len(gnull) == arity and (kind == 0).all()
    for f in range(arity):
        nl = np.zeros(n, dtype=bool) if nulls[f] is None else nulls[f]
        assert got[f].dtype == np.int64 and (gnull[f] == nl).all(), f
        assert (got[f] == np.where(nl, 0, np.ascontiguousarray(fields[f]).view(np.int64))).all(), f
    assert (R.unpack_rows(buf.tobytes(), arity, stride)[0][arity - 1] == got[arity - 1]).all()
    assert (R.unpack_rows(R.pack_rows(fields, nulls, stride=stride, row_kind=3), arity, stride)[2] == 3).all()


def test_python_surface():
    p = inspect.signature(WindowAggOperator.fired_packed).parameters
    assert [(k, v.default) for k, v in p.items() if k != "self"] == \
        [("first_row", 0), ("max_rows", None), ("key_field", False), ("device", False)]
    assert not hasattr(CompositeWindowAggOperator, "fired_packed")   # (its rows are joined on the host)
    assert callable(R.unpack_rows)


def test_jni_glue_and_java_side(tmp_path):
    so = str(tmp_path / "libflinkgpujni.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "tests", "jni_stub"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "flink_gpu_jni.c"), "-o", so], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    pre = "Java_org_apache_flink_table_runtime_operators_window_gpu_FlinkGpu_"
    for nat in ("firedPacked", "advanceProgressDevice", "collectFiredDevice"):
        assert re.search(r"\bT %s%s\b" % (pre, nat), syms), nat
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bU fg_fired_packed\b", und)
    java = open(os.path.join(JAVA, "FlinkGpu.java")).read()
    assert re.search(r"public static native long firedPacked\(long h, long firstRow, long maxRows, int flags, "
                     r"ByteBuffer\[\] out, long\[\] shape\);", java)
    assert "public static final int PACK_KEY_FIELD = 1;" in java
    cfg = open(os.path.join(JAVA, "FgConfig.java")).read()
    assert '"table.exec.window-agg.gpu.fired-packed"' in cfg
    assert re.search(r"public static boolean firedPacked = Boolean\.parseBoolean\(System\.getProperty\(FIRED_PACKED_KEY, "
                     r'"false"\)\);', cfg)
    proc = open(os.path.join(JAVA, "GpuSlicingWindowProcessor.java")).read()
    for phrase in ("FlinkGpu.firedPacked(", "FlinkGpu.advanceProgressDevice(", "FlinkGpu.collectFiredDevice(",
                   "row.pointTo(seg, i * stride, stride)", "1L << 30", "FlinkGpu.PACK_KEY_FIELD"):
        assert phrase in proc, phrase
