"""The pose-alignment entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_align_options / nvbx_align_sums / nvbx_align_result have the layout the header promises (compiled with gcc as C99) and the ctypes
structures mirror it field by field.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_default_align_options", "nvbx_align_points", "nvbx_align_depth", "nvbx_linearize_points")
STRUCTS = {
    "nvbx_align_options": ("AlignOptions", ("max_iterations", "subsampling", "min_weight", "huber_delta_m", "damping", "min_pivot_ratio",
                                            "stop_translation_m", "stop_rotation_rad", "min_valid", "max_depth_m")),
    "nvbx_align_sums": ("AlignSums", ("H", "b", "cost", "n_valid", "pad")),
    "nvbx_align_result": ("AlignResult", ("T_L_S", "T64", "step", "first", "last", "iterations", "status")),
}


def test_library_exports_the_alignment_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_alignment_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NAMES:
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert (res is C.c_int) == (decl.group(1) == "int") and (res is None) == (decl.group(1) == "void")
        assert len(args) == len(decl.group(2).split(",")), s
    ap = _lib.SIGNATURES["nvbx_align_points"][1]
    assert len(ap) == 6 and ap[2] is C.c_int64
    ad = _lib.SIGNATURES["nvbx_align_depth"][1]
    assert len(ad) == 8 and ad[2] is C.c_int32 and ad[3] is C.c_int32
    lp = _lib.SIGNATURES["nvbx_linearize_points"][1]
    assert len(lp) == 10 and lp[2] is C.c_int64


def test_struct_layouts_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib, mapper as M
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = ""
    for cname, (_, fields) in STRUCTS.items():
        body += '  printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (cname, cname)
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + '  printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [list(map(int, l.split())) for l in subprocess.check_output([str(exe)]).decode().splitlines()]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert rows[0] == [56, 8, 0, 4, 8, 12, 16, 24, 32, 40, 48, 52]
    assert rows[1] == [232, 8, 0, 168, 216, 224, 228]
    assert rows[2] == [712, 8, 0, 64, 192, 240, 472, 704, 708]
    for row, (cname, (pyname, fields)) in zip(rows, STRUCTS.items()):
        st = getattr(_lib, pyname)
        assert C.sizeof(st) == row[0] and C.alignment(st) == row[1], cname
        assert [f for f, _ in st._fields_] == list(fields), cname
        assert [getattr(st, f).offset for f in fields] == row[2:], cname
    assert M.ALIGN_RESULT_BYTES == 712


def test_default_options_and_status_codes(hip_lib):
    """nvbx_default_align_options is a pure host function; the status codes of the header, the mirror and the tests' model agree"""
    from isaac_ros_nvblox_amd import _lib, mapper as M
    import align_independent as A
    o = _lib.AlignOptions()
    hip_lib.nvbx_default_align_options(C.byref(o))
    for k, v in A.DEFAULTS.items():
        got = getattr(o, k)
        assert got == (C.c_float(v).value if isinstance(got, float) and k in ("min_weight", "huber_delta_m", "max_depth_m") else v), k
    txt = open(HEADER).read()
    for name in ("CONVERGED", "MAX_ITERATIONS", "TOO_FEW", "DEGENERATE", "LINEARIZED"):
        value = int(re.search(r"#define\s+NVBX_ALIGN_%s\s+(\d+)" % name, txt).group(1))
        assert value == getattr(M, "ALIGN_" + name) == getattr(A, name) and M.ALIGN_STATUS_NAMES[value] == name


def test_python_mapper_has_the_three_methods():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("align_points", "align_depth", "linearize_points"):
        assert callable(getattr(M.Mapper, name, None)), name
    assert hasattr(M.AlignResult, "T_L_S") and hasattr(M.AlignResult, "rmse_first") and hasattr(M.AlignResult, "rmse_last")
