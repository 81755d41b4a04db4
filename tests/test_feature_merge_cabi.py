"""The feature-merging entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_feature_merge_options / nvbx_feature_merge_result have the layout the header promises (compiled with gcc as C99) and the ctypes
structures mirror it field by field; the refusals that need no device.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_default_feature_merge_options", "nvbx_merge_features", "nvbx_set_feature_blocks")
STRUCTS = {
    "nvbx_feature_merge_options": ("FeatureMergeOptions", ("min_weight", "weight_scale", "reserved")),
    "nvbx_feature_merge_result": ("FeatureMergeResult", ("source_blocks", "candidate_blocks", "blocks_flagged", "voxels_fused", "status", "pad")),
}


def test_library_exports_the_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NAMES:
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert (res is C.c_int) == (decl.group(1) == "int") and (res is None) == (decl.group(1) == "void")
        assert len(args) == len(decl.group(2).split(",")), s
    mf = _lib.SIGNATURES["nvbx_merge_features"][1]
    assert len(mf) == 5 and mf[3] == C.POINTER(_lib.FeatureMergeOptions)
    assert _lib.SIGNATURES["nvbx_set_feature_blocks"] == _lib.SIGNATURES["nvbx_get_feature_blocks"]      # the mirror of the reader


def test_struct_layouts_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib, mapper as M
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = ""
    for cname, (_, fields) in STRUCTS.items():
        body += '  printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (cname, cname)
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + '  printf("\\n");\n'
    # the merge's own records do not change by a byte
    body += '  printf("%zu %zu\\n", sizeof(nvbx_merge_options), sizeof(nvbx_merge_result));\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [list(map(int, l.split())) for l in subprocess.check_output([str(exe)]).decode().splitlines()]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert rows[0] == [32, 4, 0, 4, 8]
    assert rows[1] == [64, 8, 0, 8, 16, 24, 32, 36]
    assert rows[2] == [16, 64]
    for row, (cname, (pyname, fields)) in zip(rows, STRUCTS.items()):
        st = getattr(_lib, pyname)
        assert C.sizeof(st) == row[0] and C.alignment(st) == row[1], cname
        assert [f for f, _ in st._fields_] == list(fields), cname
        assert [getattr(st, f).offset for f in fields] == row[2:], cname
    assert M.FEATURE_MERGE_RESULT_BYTES == 64


def test_default_options_and_status_codes(hip_lib):
    """nvbx_default_feature_merge_options is a pure host function; the status codes are the merge's, in the header, the mirror and the model"""
    from isaac_ros_nvblox_amd import _lib, mapper as M
    import feature_merge_independent as FM
    o = _lib.FeatureMergeOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    hip_lib.nvbx_default_feature_merge_options(C.byref(o))
    assert o.min_weight == FM.DEFAULTS["min_weight"] == 0.0 and o.weight_scale == FM.DEFAULTS["weight_scale"] == 1.0
    assert list(o.reserved) == [0] * 6
    hip_lib.nvbx_default_feature_merge_options(None)                 # a NULL is ignored
    assert (M.MERGE_OK, M.MERGE_EMPTY_SOURCE, M.MERGE_NO_OVERLAP) == (FM.OK, FM.EMPTY_SOURCE, FM.NO_OVERLAP)
    math_h = open(os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc", "nvbx_feature_merge_math.h")).read()
    assert '#include "nvbx_merge_math.h"' in math_h and "NVBX_MERGE_MARGIN_VOX" in math_h      # the margin is the merge's, not a second constant


def test_refusals_that_need_no_device(hip_lib):
    """NULL mappers: NVBX_E_INVALID, and the error names the call"""
    from isaac_ros_nvblox_amd import _lib
    T = (C.c_float * 16)(*[1.0 if i % 5 == 0 else 0.0 for i in range(16)])
    o = _lib.FeatureMergeOptions()
    hip_lib.nvbx_default_feature_merge_options(C.byref(o))
    buf = (C.c_int64 * 8)()
    assert hip_lib.nvbx_merge_features(None, None, T, C.byref(o), buf) == -1
    assert hip_lib.nvbx_last_error().decode().startswith("nvbx_merge_features: both mappers are required")
    assert hip_lib.nvbx_set_feature_blocks(None, None, 0, None, None, None) == -1
    assert hip_lib.nvbx_last_error().decode().startswith("nvbx_set_feature_blocks: invalid argument")


def test_python_mapper_has_the_methods():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("merge_features_from", "feature_merge_options", "set_feature_blocks"):
        assert callable(getattr(M.Mapper, name, None)), name
    for f in ("source_blocks", "candidate_blocks", "blocks_flagged", "voxels_fused", "status", "status_name"):
        assert hasattr(M.FeatureMergeResult, f), f
