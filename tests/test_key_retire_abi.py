"""CPU-side checks of retiring dictionary keys (fg_key_dict_retain, fg_key_dict_get_stats): the
C-ABI is exported, bound and documented with ABI 16 unchanged, the stats struct has the header's
layout, the JNI glue compiles with the two new natives, the Java shim carries the policy, and
keyed_state.retain_due decides as the shim does. No device is needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from flink_amd import _lib as L
from flink_amd import keys as K
from flink_amd.keyed_state import HOP, SliceSpec, WindowAggsState, retain_due
from tests.test_abi import HEADER, ROOT, declared_symbols

NEW = ("fg_key_dict_get_stats", "fg_key_dict_retain")
FIELDS = ["live", "issued", "free_ordinals", "arena_bytes", "table_slots", "side_rows", "retired_total", "reserved0"]
JAVA = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink", "table", "runtime", "operators",
                    "window", "gpu")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for s in NEW:
        assert s in L.EXPORTS and s in declared_symbols(), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).restype is C.c_int, s
    P = C.c_void_p
    assert list(lib.fg_key_dict_get_stats.argtypes) == [P, C.POINTER(L.FgKeyDictStats)]
    assert list(lib.fg_key_dict_retain.argtypes) == [P, C.c_int32, C.c_int32, C.POINTER(P), C.POINTER(C.c_int64),
                                                     C.POINTER(L.FgKeyDictStats)]
    assert lib.fg_abi_version() == 16


def test_symbols_are_in_the_map_file():
    src = open(os.path.join(ROOT, "flink_amd", "csrc", "libflinkgpu.map")).read()
    glob = src[src.index("global:"):src.index("local:")]
    for s in NEW:
        assert re.search(r"\b%s;" % s, glob), s


def test_header_declarations():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+fg_key_dict_retain\s*\(([^)]*)\)\s*;", src)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "fg_key_dict* d", "int32_t location", "int32_t n_sets", "const int64_t* const* ids", "const int64_t* counts",
        "fg_key_dict_stats* out"]
    m = re.search(r"int\s+fg_key_dict_get_stats\s*\(([^)]*)\)\s*;", src)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["fg_key_dict* d", "fg_key_dict_stats* out"]


def test_stats_layout_matches_header(tmp_path):
    assert [f for f, _ in L.FgKeyDictStats._fields_] == FIELDS
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flinkgpu.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(fg_key_dict_stats));']
    src += [f'printf("{f} %zu\\n", offsetof(fg_key_dict_stats, {f}));' for f in FIELDS]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.FgKeyDictStats) == 64
    for f in FIELDS:
        assert int(got[f]) == getattr(L.FgKeyDictStats, f).offset, f


def test_header_documents_the_contract():
    src = open(HEADER).read()
    doc = src[src.index("Retire keys without state and reuse their ids (ABI 16, added)"):src.index("int  fg_key_dict_retain(")]
    doc = " ".join(doc.replace("\n *", " ").split())   # (comment lines joined)
    for word in NEW + ("FG_EINVAL", "FG_ESTATE", "FG_EDEVICE", "unchanged", "reused", "fg_key_dict_rows",
                       "fg_key_dict_lookup", "fg_partition_keyed_by_owner", "no id outside", "lowest free ordinals",
                       "typedef struct fg_key_dict_stats", "empties the dictionary"):
        assert word in doc, word
    assert "#define FG_ABI_VERSION 16" in src
    assert "stable for the dictionary's life" not in src   # ids live until a retain retires them
    assert "fg_key_dict_retain retires it" in src
    assert re.search(r"valid until the next intern\s+\*?\s*or retain", src)


def test_null_dictionary_is_einval():
    lib = L.load()
    st = L.FgKeyDictStats()
    assert lib.fg_key_dict_get_stats(None, C.byref(st)) == L.FG_EINVAL
    ids = (C.c_int64 * 1)(0)
    sets = (C.c_void_p * 1)(C.addressof(ids))
    counts = (C.c_int64 * 1)(1)
    for loc in (L.HOST, L.DEVICE):
        assert lib.fg_key_dict_retain(None, loc, 1, sets, counts, C.byref(st)) == L.FG_EINVAL
        assert lib.fg_key_dict_retain(None, loc, 0, None, None, None) == L.FG_EINVAL


def test_python_surface():
    assert callable(K.KeyDictionary.retain) and callable(K.KeyDictionary.stats)
    assert inspect.signature(K.KeyDictionary.retain).parameters["id_arrays"].kind is inspect.Parameter.VAR_POSITIONAL
    assert "dict_retain" in K.KeyDictionary.kernel_stats.__doc__
    assert inspect.signature(WindowAggsState.wanted_slices).parameters["force_all"].default is False


def test_jni_glue_compiles_and_exports_the_natives(tmp_path):
    so = str(tmp_path / "libflinkgpujni.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "tests", "jni_stub"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "flink_gpu_jni.c"), "-o", so], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    pre = "Java_org_apache_flink_table_runtime_operators_window_gpu_FlinkGpu_"
    for nat in ("dictRetain", "dictStats"):
        assert re.search(r"\bT %s%s\b" % (pre, nat), syms), nat
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    for s in NEW:
        assert re.search(r"\bU %s\b" % s, und), s


def test_java_shim_carries_the_policy():
    gpu = open(os.path.join(JAVA, "FlinkGpu.java")).read()
    assert "public static native long[] dictRetain(long d, ByteBuffer ids, int n);" in gpu
    assert "public static native long[] dictStats(long d);" in gpu
    rows = open(os.path.join(JAVA, "GpuKeyRows.java")).read()
    m = re.search(r"void retain\(ByteBuffer keys, int count\) \{(.*?)\n    \}", rows, re.S)
    assert m, "GpuKeyRows declares no retain(ByteBuffer, int)"
    body = m.group(1)
    assert "FlinkGpu.dictRetain(dict, keys, count)" in body
    assert re.search(r"if \(bigint\) \{\s*return;", body)   # a no-op for a BIGINT key
    cfg = open(os.path.join(JAVA, "FgConfig.java")).read()
    assert 'dictRetainFactor = Long.getLong("flinkgpu.dictRetainFactor", 0)' in cfg
    proc = open(os.path.join(JAVA, "GpuSlicingWindowProcessor.java")).read()
    body = proc[proc.index("private void writeKeyedState()"):proc.index("private long namespaceOf(")]
    assert "FgConfig.dictRetainFactor" in body and "keys.retain(cols[0]," in body
    assert body.index("windowState.update(") < body.index("keys.retain(")   # after the image's rows are written


def test_retain_due_truth_table():
    lo = 1 << 16
    # factor: 0 (the default) never
    assert not retain_due(10 * lo, 1, 0) and not retain_due(10 * lo, 1, -1) and retain_due(10 * lo, 1, 1)
    # the live floor
    assert not retain_due(lo - 1, 0, 2) and retain_due(lo, 0, 2)
    # strictly more than factor x the state's rows
    assert not retain_due(2 * lo, lo, 2) and retain_due(2 * lo + 1, lo, 2) and not retain_due(2 * lo + 1, lo + 1, 2)
    # a lower floor, passed in
    assert retain_due(1001, 500, 2, min_live=1000) and not retain_due(999, 10, 2, min_live=1000)


def test_force_all_selects_every_slice():
    st = WindowAggsState(SliceSpec(HOP, 3000, 1000))
    plan = dict(slice_end=np.array([1000, 2000, 3000], dtype=np.int64), first_row=np.array([0, 2, 4], dtype=np.int64),
                rows=np.array([2, 2, 1], dtype=np.int64), changed=np.array([0, 1, 0], dtype=np.uint8))
    assert st.wanted_slices(plan, 500).tolist() == [0, 1, 0]
    assert st.wanted_slices(plan, 500, force_all=False).tolist() == [0, 1, 0]
    assert st.wanted_slices(plan, 500, force_all=True).tolist() == [1, 1, 1]
