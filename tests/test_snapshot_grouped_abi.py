"""CPU-side checks of the key-grouped snapshot's C-ABI (fg_set_snapshot_grouping,
fg_snapshot_key_groups): exported, bound with their argument types, documented in the header,
the ctypes mirror of fg_image_key_groups laid out as the C compiler lays it out, and the ABI
version unchanged (the entry points were added to ABI 16)."""
import ctypes as C
import os
import subprocess

from flink_amd import _lib as L
from tests.test_abi import HEADER, ROOT, declared_symbols

NEW = ("fg_set_snapshot_grouping", "fg_snapshot_key_groups")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for s in NEW:
        assert s in L.EXPORTS and s in declared_symbols(), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).restype is C.c_int, s
    assert list(lib.fg_set_snapshot_grouping.argtypes) == [C.c_void_p, C.c_int32]
    assert list(lib.fg_snapshot_key_groups.argtypes) == [C.c_void_p, C.POINTER(L.FgImageKeyGroups)]
    assert lib.fg_abi_version() == 16


def test_null_handles_are_refused():
    """both entry points check their arguments before anything else (no device is touched)"""
    lib = L.load()
    assert lib.fg_set_snapshot_grouping(None, 0) == L.FG_EINVAL
    assert lib.fg_snapshot_key_groups(None, C.byref(L.FgImageKeyGroups())) == L.FG_EINVAL


def test_header_documents_them():
    src = open(HEADER).read()
    for s in NEW + ("fg_image_key_groups", "KeyGroupRangeOffsets", "FG_ESTATE if no image was returned"):
        assert s in src, s
    doc = src[src.index("Key-grouped images"):src.index("int  fg_set_snapshot_grouping")]
    for word in ("key_hash < 0", "max_parallelism", "FG_EINVAL", "device memory", "cnt_val"):
        assert word in doc, word


def test_struct_layout_matches_the_header(tmp_path):
    py = L.FgImageKeyGroups
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flinkgpu.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(fg_image_key_groups));']
    for f, _ in py._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(fg_image_key_groups, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {a: int(v) for a, v in (ln.split() for ln in out if ln)}
    assert [f for f, _ in py._fields_] == ["n_slices", "max_parallelism", "first_row"]
    assert got["size"] == C.sizeof(py)
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset, f
