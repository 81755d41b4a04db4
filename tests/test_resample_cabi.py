"""The resampling entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_resample_options has the layout the header promises (compiled with gcc as C99) and the ctypes structure mirrors it field by field; the
result record is nvbx_merge_result itself.  No compute calls here."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_default_resample_options", "nvbx_resample_map")
FIELDS = ("min_weight", "weight_scale", "merge_color", "taps")


def test_library_exports_the_resample_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_resample_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NAMES:
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert (res is C.c_int) == (decl.group(1) == "int") and (res is None) == (decl.group(1) == "void")
        assert len(args) == len(decl.group(2).split(",")), s
    rm = _lib.SIGNATURES["nvbx_resample_map"][1]
    assert len(rm) == 5 and rm[3] == C.POINTER(_lib.ResampleOptions)
    # the result record is the merge's: the declaration names nvbx_merge_result
    assert re.search(r"nvbx_resample_map\s*\([^;]*nvbx_merge_result\s*\*\s*result_dev\s*\)", txt)


def test_struct_layout_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = '  printf("%zu %zu", sizeof(nvbx_resample_options), _Alignof(nvbx_resample_options));\n'
    body += "".join('  printf(" %%zu", offsetof(nvbx_resample_options, %s));\n' % f for f in FIELDS) + '  printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    row = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert row == [16, 4, 0, 4, 8, 12]
    st = _lib.ResampleOptions
    assert C.sizeof(st) == 16 and C.alignment(st) == 4
    assert [f for f, _ in st._fields_] == list(FIELDS)
    assert [getattr(st, f).offset for f in FIELDS] == row[2:]
    assert [t for _, t in st._fields_] == [C.c_float, C.c_float, C.c_int32, C.c_int32]


def test_default_options_and_constants(hip_lib):
    """nvbx_default_resample_options is a pure host function; the constants of the header of the arithmetic and of the tests' model agree"""
    from isaac_ros_nvblox_amd import _lib
    import resample_independent as RI
    o = _lib.ResampleOptions()
    o.taps = 77
    hip_lib.nvbx_default_resample_options(C.byref(o))
    assert o.min_weight == C.c_float(RI.DEFAULTS["min_weight"]).value and o.weight_scale == RI.DEFAULTS["weight_scale"]
    assert o.merge_color == RI.DEFAULTS["merge_color"] and o.taps == RI.DEFAULTS["taps"] == 0
    hip_lib.nvbx_default_resample_options(None)                               # NULL: nothing happens
    math_h = open(os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc", "nvbx_resample_math.h")).read()
    assert float(re.search(r"#define\s+NVBX_RESAMPLE_MAX_RATIO\s+(\S+)", math_h).group(1)) == RI.MAX_RATIO
    assert int(re.search(r"#define\s+NVBX_RESAMPLE_MAX_TAPS\s+(\S+)", math_h).group(1)) == RI.MAX_TAPS


def test_python_mapper_has_the_methods():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("resample_from", "resample_options", "coarsened"):
        assert callable(getattr(M.Mapper, name, None)), name
    sig = inspect.signature(M.Mapper.resample_from)
    assert list(sig.parameters)[:4] == ["self", "other", "T_D_S", "out"] and sig.parameters["T_D_S"].default is None
    sig = inspect.signature(M.Mapper.coarsened)
    assert sig.parameters["factor"].default == 2.0 and sig.parameters["block_capacity"].default is None
