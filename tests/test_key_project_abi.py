"""fg_key_dict_project / fg_key_dict_intern_fields (the key selector on the GPU) as the C-ABI, the
ctypes binding, the Python reference and the Java shim declare them. No device is needed: the
argument checks run before any device call, and project_key_row is pure Python."""
import ctypes as C
import os
import re
import subprocess

import pytest

from flink_amd import _lib as L
from flink_amd import keys as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flinkgpu.h")
JAVA = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink", "table", "runtime", "operators",
                    "window", "gpu")
NEW = ("fg_key_dict_project", "fg_key_dict_intern_fields")
FIELDS = ["arity", "n_key_fields", "key_field", "key_kind", "n_cols", "col_field"]
KINDS = {"FG_FIELD_FIX1": 1, "FG_FIELD_FIX2": 2, "FG_FIELD_FIX4": 4, "FG_FIELD_FIX8": 8, "FG_FIELD_VAR": 16}


def test_symbols_are_declared_exported_and_bound():
    src = open(HEADER).read()
    lib = L.load()
    for s in NEW:
        assert re.search(r"^int\s+%s\s*\(" % s, src, re.M), s
        assert s in L.EXPORTS and hasattr(lib, s), s
        assert getattr(lib, s).restype is C.c_int, s
    P = C.c_void_p
    assert list(lib.fg_key_dict_project.argtypes) == [P, C.c_int32, C.c_int64, P, C.c_int64, P, P,
                                                      C.POINTER(L.FgRowProjection), P, C.c_int64, P, P, C.POINTER(P),
                                                      C.POINTER(P), C.POINTER(C.c_int64)]
    assert list(lib.fg_key_dict_intern_fields.argtypes) == [P, C.c_int32, C.c_int64, P, C.c_int64, P, P,
                                                            C.POINTER(L.FgRowProjection), P, P, C.POINTER(P), C.POINTER(P)]
    assert lib.fg_abi_version() == 16


def test_symbols_are_in_the_map_file():
    src = open(os.path.join(ROOT, "flink_amd", "csrc", "libflinkgpu.map")).read()
    glob = src[src.index("global:"):src.index("local:")]
    for s in NEW:
        assert re.search(r"\b%s;" % s, glob), s


def test_header_declarations():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+fg_key_dict_project\s*\(([^)]*)\)\s*;", src)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "fg_key_dict* d", "int32_t location", "int64_t n", "const uint8_t* bytes", "int64_t nbytes",
        "const int64_t* offsets", "const int32_t* lengths", "const fg_row_projection* proj", "uint8_t* out_key_bytes",
        "int64_t cap_bytes", "int64_t* out_key_offsets", "int32_t* out_key_lengths", "int64_t* const* out_cols",
        "uint8_t* const* out_col_null", "int64_t* out_nbytes"]
    m = re.search(r"int\s+fg_key_dict_intern_fields\s*\(([^)]*)\)\s*;", src)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "fg_key_dict* d", "int32_t location", "int64_t n", "const uint8_t* bytes", "int64_t nbytes",
        "const int64_t* offsets", "const int32_t* lengths", "const fg_row_projection* proj", "int64_t* out_id",
        "int32_t* out_kg", "int64_t* const* out_cols", "uint8_t* const* out_col_null"]


def test_header_documents_the_contract():
    src = open(HEADER).read()
    doc = src[src.index("The key selector on the GPU (ABI 16, added)"):src.index("int  fg_key_dict_project(")]
    for word in ("FG_EFULL", "FG_ESTATE", "FG_EINVAL", "FG_HOST", "FG_DEVICE", "n + 1", "RowKind", "setNullAt",
                 "0x80 | len", "2^24 - 4", "dict_project", "sizing call", "byte-exact"):
        assert word in doc, word


def test_projection_layout_and_kinds_match_header(tmp_path):
    """offsetof / sizeof of fg_row_projection and the fg_field_kind values from gcc on
    include/flinkgpu.h against the ctypes mirror"""
    assert [f for f, _ in L.FgRowProjection._fields_] == FIELDS
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flinkgpu.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(fg_row_projection));',
           'printf("max_key %d\\n", FG_PROJ_MAX_KEY_FIELDS);', 'printf("max_cols %d\\n", FG_PROJ_MAX_COLS);']
    src += [f'printf("{f} %zu\\n", offsetof(fg_row_projection, {f}));' for f in FIELDS]
    src += [f'printf("{k} %d\\n", (int){k});' for k in KINDS]
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.FgRowProjection) == 92
    assert (int(got["max_key"]), int(got["max_cols"])) == (L.PROJ_MAX_KEY_FIELDS, L.PROJ_MAX_COLS) == (8, 4)
    for f in FIELDS:
        assert int(got[f]) == getattr(L.FgRowProjection, f).offset, f
    for k, v in KINDS.items():
        assert int(got[k]) == v == getattr(L, k[3:]), k
    p = K.RowProjection(6, [4, 0], ["string", L.FIELD_FIX4], col_fields=(1, 3)).struct()
    assert (p.arity, p.n_key_fields, p.n_cols) == (6, 2, 2)
    assert list(p.key_field)[:2] == [4, 0] and list(p.key_kind)[:2] == [16, 4] and list(p.col_field)[:2] == [1, 3]


def test_null_dictionary_is_einval():
    lib = L.load()
    p = K.RowProjection(1, [0], ["bigint"]).struct()
    total = C.c_int64(-1)
    rows = (C.c_uint8 * 16)()
    off = (C.c_int64 * 2)()
    ln = (C.c_int32 * 1)(16)
    ids = (C.c_int64 * 1)()
    for loc in (L.HOST, L.DEVICE):
        assert lib.fg_key_dict_project(None, loc, 1, rows, 16, off, ln, C.byref(p), None, 0, off, ln, None, None,
                                       C.byref(total)) == L.FG_EINVAL
        assert lib.fg_key_dict_intern_fields(None, loc, 1, rows, 16, off, ln, C.byref(p), ids, None, None, None) == L.FG_EINVAL
    assert lib.fg_key_dict_project(None, L.HOST, 0, None, 0, None, None, None, None, 0, None, None, None, None,
                                   None) == L.FG_EINVAL


def w(x):
    return int(x).to_bytes(8, "little")


STRING_INT = 2   # input rows of [STRING s, INT i]: an 8-byte bit set and two slots, 24 bytes
VAR0 = K.RowProjection(STRING_INT, [0], [L.FIELD_VAR])
CASES = {
    # name: (input row, projection, key row), every byte written by hand
    "inline string": (w(0) + b"abc\0\0\0\0\x83" + w(7), VAR0, w(0) + b"abc\0\0\0\0\x83"),
    "7-byte string": (w(0) + b"abcdefg\x87" + w(7), VAR0, w(0) + b"abcdefg\x87"),
    "8-byte string": (w(0) + w(24 << 32 | 8) + w(7) + b"abcdefgh", VAR0, w(0) + w(16 << 32 | 8) + b"abcdefgh"),
    "short string in the variable part": (w(0) + w(24 << 32 | 5) + w(7) + b"abcde\xff\xff\xff", VAR0,
                                          w(0) + b"abcde\0\0\x85"),
    "NULL field": (w(1 << 8) + w(0x1234) + w(7), VAR0, w(1 << 8) + w(0)),
    "RowKind on input": (b"\x02" + b"\0" * 7 + b"abc\0\0\0\0\x83" + w(7), VAR0, w(0) + b"abc\0\0\0\0\x83"),
    "FIX4 with upper bytes": (w(0) + b"abc\0\0\0\0\x83" + w(0xDEADBEEF00000007),
                              K.RowProjection(STRING_INT, [1], [L.FIELD_FIX4]), w(0) + w(7)),
    "two VAR fields swapped": (w(0) + w(24 << 32 | 9) + w(40 << 32 | 17) + b"a" * 9 + b"\0" * 7 + b"b" * 17 + b"\0" * 7,
                               K.RowProjection(2, [1, 0], [L.FIELD_VAR, L.FIELD_VAR]),
                               w(0) + w(24 << 32 | 17) + w(48 << 32 | 9) + b"b" * 17 + b"\0" * 7 + b"a" * 9 + b"\0" * 7),
}


@pytest.mark.parametrize("name", list(CASES))
def test_project_key_row_against_hand_written_bytes(name):
    row, proj, want = CASES[name]
    assert K.project_key_row(row, proj) == want


def test_project_key_row_agrees_with_key_row_and_refuses_bad_rows():
    types = ["string", "bigint", "int", "double", "string", "boolean", "float", "smallint", "tinyint"]
    fields = ["grüße, welt", -5, 1 << 30, 2.5, None, True, 0.5, -300, -7]
    row = K.key_row(fields, types, row_kind=1)
    assert K.decode_key_row(row, types) == tuple(fields)
    for pick in ([0], [4, 0], [8, 7, 6, 5, 3, 2, 1], [0, 0]):
        proj = K.RowProjection(9, pick, [types[f] for f in pick])
        got = K.project_key_row(row, proj)
        assert got == K.key_row([fields[f] for f in pick], [types[f] for f in pick])
        assert K.decode_key_row(got, [types[f] for f in pick]) == tuple(fields[f] for f in pick)
    for bad in (w(0) + w(0x88 << 56) + w(0),                      # inline longer than 7
                w(0) + w(28 << 32 | 4) + w(0) + b"x" * 8,         # an offset that is no multiple of 8
                w(0) + w(16 << 32 | 8) + w(0) + b"x" * 8,         # ... below the fixed-length part
                w(0) + w(24 << 32 | 9) + w(0) + b"x" * 8,         # ... past the row
                w(0) + w(0)):                                     # shorter than the fixed-length part
        with pytest.raises(ValueError):
            K.project_key_row(bad, VAR0)


def test_python_interface_exists():
    assert callable(K.KeyDictionary.project) and callable(K.KeyDictionary.intern_fields)
    assert "dict_project" in K.KeyDictionary.kernel_stats.__doc__
    import flink_amd as F
    assert F.RowProjection is K.RowProjection and F.project_key_row is K.project_key_row


def test_java_shim_declares_the_natives():
    gpu = open(os.path.join(JAVA, "FlinkGpu.java")).read()
    jni = open(os.path.join(ROOT, "jni", "flink_gpu_jni.c")).read()
    for name, nargs, entry in (("dictProject", 13, "fg_key_dict_project("), ("dictInternFields", 11, "fg_key_dict_intern_fields(")):
        m = re.search(r"public static native \w+ %s\(([^)]*)\);" % name, gpu, re.S)
        assert m, f"FlinkGpu.java declares no {name}"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        m = re.search(r"JNIEXPORT \w+ JNICALL FN\(%s\)\(([^)]*)\)" % name, jni, re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == nargs + 2 and entry in jni
    for k, v in KINDS.items():
        assert re.search(r"\b%s = %d\b" % (k[3:], v), gpu), k
    rows = open(os.path.join(JAVA, "GpuKeyRows.java")).read()
    assert "void internFields(" in rows and "FlinkGpu.dictInternFields(" in rows
