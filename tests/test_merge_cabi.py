"""The map-merging entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_merge_options / nvbx_merge_result have the layout the header promises (compiled with gcc as C99) and the ctypes structures mirror it
field by field.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_default_merge_options", "nvbx_merge_map")
STRUCTS = {
    "nvbx_merge_options": ("MergeOptions", ("min_weight", "weight_scale", "merge_color", "pad")),
    "nvbx_merge_result": ("MergeResult", ("source_blocks", "candidate_blocks", "blocks_allocated", "voxels_fused", "color_voxels_fused", "status", "pad")),
}


def test_library_exports_the_merge_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_merge_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NAMES:
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert (res is C.c_int) == (decl.group(1) == "int") and (res is None) == (decl.group(1) == "void")
        assert len(args) == len(decl.group(2).split(",")), s
    mm = _lib.SIGNATURES["nvbx_merge_map"][1]
    assert len(mm) == 5 and mm[3] == C.POINTER(_lib.MergeOptions)


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
    assert rows[0] == [16, 4, 0, 4, 8, 12]
    assert rows[1] == [64, 8, 0, 8, 16, 24, 32, 40, 44]
    for row, (cname, (pyname, fields)) in zip(rows, STRUCTS.items()):
        st = getattr(_lib, pyname)
        assert C.sizeof(st) == row[0] and C.alignment(st) == row[1], cname
        assert [f for f, _ in st._fields_] == list(fields), cname
        assert [getattr(st, f).offset for f in fields] == row[2:], cname
    assert M.MERGE_RESULT_BYTES == 64


def test_default_options_and_status_codes(hip_lib):
    """nvbx_default_merge_options is a pure host function; the status codes of the header, the mirror and the tests' model agree"""
    from isaac_ros_nvblox_amd import _lib, mapper as M
    import merge_independent as MI
    o = _lib.MergeOptions()
    hip_lib.nvbx_default_merge_options(C.byref(o))
    assert o.min_weight == C.c_float(MI.DEFAULTS["min_weight"]).value and o.weight_scale == MI.DEFAULTS["weight_scale"]
    assert o.merge_color == MI.DEFAULTS["merge_color"] and o.pad == 0
    txt = open(HEADER).read()
    for name in ("OK", "EMPTY_SOURCE", "NO_OVERLAP"):
        value = int(re.search(r"#define\s+NVBX_MERGE_%s\s+(\d+)" % name, txt).group(1))
        assert value == getattr(M, "MERGE_" + name) == getattr(MI, name) and M.MERGE_STATUS_NAMES[value] == name
    # the constants of the candidate rule: the header of the arithmetic and the model
    math_h = open(os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc", "nvbx_merge_math.h")).read()
    assert float(re.search(r"#define\s+NVBX_MERGE_MARGIN_VOX\s+(\S+)", math_h).group(1)) == MI.MARGIN_VOX
    assert float(re.search(r"#define\s+NVBX_MERGE_ROTATION_TOL\s+(\S+)", math_h).group(1)) == MI.ROTATION_TOL


def test_python_mapper_has_the_methods():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("merge_from", "merge_options"):
        assert callable(getattr(M.Mapper, name, None)), name
    for f in ("source_blocks", "candidate_blocks", "blocks_allocated", "voxels_fused", "color_voxels_fused", "status", "status_name"):
        assert hasattr(M.MergeResult, f), f
