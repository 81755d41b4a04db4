"""The feature-matching entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists, the
header defines the metric ids.  No compute calls here."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_match_features", "nvbx_match_points")


def test_library_exports_the_match_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_match_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NAMES:
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        assert res is C.c_int
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert len(args) == len(decl.group(1).split(",")), s
    assert re.search(r"#define\s+NVBX_MATCH_DOT\s+0\b", txt) and re.search(r"#define\s+NVBX_MATCH_COSINE\s+1\b", txt)
    f = _lib.SIGNATURES["nvbx_match_features"][1]
    assert f[2] is C.c_int32 and f[3] is C.c_int32 and f[4] is C.c_float and f[9] is C.c_int64       # n_queries, metric, min_weight, capacity_blocks
    p = _lib.SIGNATURES["nvbx_match_points"][1]
    assert p[2] is C.c_int64 and p[4] is C.c_int32 and p[5] is C.c_int32                              # n, n_queries, metric


def test_python_mapper_has_the_two_methods():
    from isaac_ros_nvblox_amd import mapper as M
    assert callable(getattr(M.Mapper, "match_features", None)) and callable(getattr(M.Mapper, "match_points", None))
