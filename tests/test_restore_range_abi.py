"""CPU-side checks of the rescale restore's boundary (fg_restore_range): the library exports it,
fg_restore_info has the header's layout in ctypes, the Python entry points exist, and the Java
native, its JNI export and the glue's call agree."""
import ctypes as C
import inspect
import os
import re
import subprocess

from flink_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JNI_C = os.path.join(ROOT, "jni", "flink_gpu_jni.c")
JAVA = os.path.join(ROOT, "java", "src", "main", "java", "org", "apache", "flink", "table", "runtime", "operators",
                    "window", "gpu")


def test_library_exports_fg_restore_range():
    lib = L.load()
    assert "fg_restore_range" in L.EXPORTS
    assert hasattr(lib, "fg_restore_range")
    assert lib.fg_restore_range.restype is C.c_int and len(lib.fg_restore_range.argtypes) == 7
    assert lib.fg_abi_version() == 16


def test_restore_info_layout_matches_header(tmp_path):
    """offsetof / sizeof of fg_restore_info from gcc on include/flinkgpu.h against the ctypes mirror"""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flinkgpu.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(fg_restore_info));']
    for f, _ in L.FgRestoreInfo._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(fg_restore_info, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {a: int(v) for a, v in (ln.split() for ln in out if ln)}
    assert [f for f, _ in L.FgRestoreInfo._fields_] == ["rows_in", "rows_kept", "slices", "state_regions"]
    assert got["size"] == C.sizeof(L.FgRestoreInfo)
    for f, _ in L.FgRestoreInfo._fields_:
        assert got[f] == getattr(L.FgRestoreInfo, f).offset, f


def test_python_entry_points_exist():
    from flink_amd import two_phase
    from flink_amd.window_agg import WindowAggOperator
    sig = inspect.signature(WindowAggOperator.restore_state_range)
    assert list(sig.parameters) == ["self", "images", "timer_watermark", "key_hash"]
    assert sig.parameters["timer_watermark"].default is None
    assert sig.parameters["key_hash"].default == L.KEYHASH_BINARYROW_BIGINT
    assert list(inspect.signature(two_phase.restore_union).parameters) == ["glob", "images", "key_hash"]


def test_java_native_jni_export_and_glue_agree():
    java = open(os.path.join(JAVA, "FlinkGpu.java")).read()
    m = re.search(r"public static native long restoreRange\(([^)]*)\)", java, re.S)
    assert m, "FlinkGpu.java declares no restoreRange"
    n_java = len([a for a in m.group(1).split(",") if a.strip()])
    src = open(JNI_C).read()
    m = re.search(r"JNIEXPORT jlong JNICALL FN\(restoreRange\)\(([^)]*)\)\s*\{(.*?)\n\}", src, re.S)
    assert m, "flink_gpu_jni.c exports no restoreRange"
    n_jni = len([a for a in m.group(1).split(",") if a.strip()]) - 2   # JNIEnv*, jclass
    assert n_java == n_jni == 11, (n_java, n_jni)
    assert "fg_restore_range(" in m.group(2)
    op = open(os.path.join(JAVA, "GpuTwoPhaseWindowAggOperator.java")).read()
    assert "FlinkGpu.restoreRange(" in op
    body = op[op.index("private void restoreGlobal("):]
    assert "RowData" not in body and "new long[" not in body   # no per-row objects on the restore path
