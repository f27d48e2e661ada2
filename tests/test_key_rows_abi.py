"""fg_key_dict_rows (the packed key rows of ids, gathered on the GPU) as the C-ABI, the ctypes
binding, the Python interface and the Java shim declare it. No device is needed: the argument
checks run before any device call."""
import ctypes as C
import os
import re

from flink_amd import _lib as L
from flink_amd import keys as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flinkgpu.h")
JAVA = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink", "table", "runtime", "operators",
                    "window", "gpu")


def test_symbol_is_declared_exported_and_bound():
    src = open(HEADER).read()
    assert re.search(r"^int\s+fg_key_dict_rows\s*\(", src, re.M)
    assert "fg_key_dict_rows" in L.EXPORTS
    lib = L.load()
    P = C.c_void_p
    assert lib.fg_key_dict_rows.argtypes == [P, C.c_int32, C.c_int64, P, P, C.c_int64, P, P, C.POINTER(C.c_int64)]
    assert lib.fg_key_dict_rows.restype is C.c_int
    assert lib.fg_abi_version() == 16


def test_header_declaration_matches_the_issue():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+fg_key_dict_rows\s*\(([^)]*)\)\s*;", src)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["fg_key_dict* d", "int32_t location", "int64_t n", "const int64_t* ids", "uint8_t* out_bytes",
                    "int64_t cap_bytes", "int64_t* out_offsets", "int32_t* out_lengths", "int64_t* out_nbytes"]


def test_null_dictionary_is_einval():
    lib = L.load()
    nbytes = C.c_int64(-1)
    ids = (C.c_int64 * 1)(0)
    off = (C.c_int64 * 2)()
    ln = (C.c_int32 * 1)()
    for loc in (L.HOST, L.DEVICE):
        assert lib.fg_key_dict_rows(None, loc, 1, ids, None, 0, off, ln, C.byref(nbytes)) == L.FG_EINVAL
    assert lib.fg_key_dict_rows(None, L.HOST, 0, None, None, 0, None, None, None) == L.FG_EINVAL


def test_header_documents_the_contract():
    src = open(HEADER).read()
    end = src.index("int  fg_key_dict_rows(")
    start = src.rindex("fg_key_dict_lookup(", 0, end)
    doc = src[start:end]
    for word in ("FG_EFULL", "FG_ESTATE", "FG_EINVAL", "n + 1", "FG_HOST", "FG_DEVICE"):
        assert word in doc, word
    assert re.search(r"zero\s+padding|pad bytes are zero", doc)


def test_python_interface_exists():
    assert callable(K.KeyDictionary.rows)
    assert callable(K.reintern)
    assert "dict_rows" in K.KeyDictionary.kernel_stats.__doc__


def test_java_shim_uses_dict_rows():
    gpu = open(os.path.join(JAVA, "FlinkGpu.java")).read()
    m = re.search(r"public static native long dictRows\(([^)]*)\);", gpu, re.S)
    assert m, "FlinkGpu.java declares no dictRows"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 7
    assert "dictLookup(" in gpu and "dictCopyArena(" in gpu   # both stay declared
    rows = open(os.path.join(JAVA, "GpuKeyRows.java")).read()
    assert "FlinkGpu.dictRows(" in rows
    assert "dictCopyArena" not in rows
    jni = open(os.path.join(ROOT, "jni", "flink_gpu_jni.c")).read()
    assert re.search(r"FN\(dictRows\)", jni) and "fg_key_dict_rows(" in jni
