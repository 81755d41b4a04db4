"""The feature-segmentation entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_component has the layout the header promises (compiled with gcc as C99) and the ctypes structure and the numpy dtype of the tests'
model mirror it.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_label_components", "nvbx_segment_features")
FIELDS = ("label", "voxels", "min_xyz", "max_xyz", "sum_xyz", "peak_score", "peak_xyz")


def test_library_exports_the_segmentation_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_segmentation_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in NAMES:
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        assert res is C.c_int
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert len(args) == len(decl.group(1).split(",")), s
    lc = _lib.SIGNATURES["nvbx_label_components"][1]
    assert len(lc) == 12 and lc[4] is C.c_int64 and lc[6] is C.c_int32 and lc[7] is C.c_int32 and lc[10] is C.c_int64      # n_blocks, connectivity, min_voxels, capacity
    sf = _lib.SIGNATURES["nvbx_segment_features"][1]
    assert len(sf) == 17 and sf[2] is C.c_int32 and sf[3] is C.c_int32 and sf[4] is C.c_float and sf[6] is C.c_int32 and sf[7] is C.c_int32
    assert sf[12] is C.c_int64 and sf[15] is C.c_int64                                                                     # the two capacities


def test_component_layout_of_the_header_the_mirror_and_the_model(tmp_path):
    from isaac_ros_nvblox_amd import _lib, mapper as M
    import segment_independent as SI
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n  printf("%zu %zu", sizeof(nvbx_component), '
                   '_Alignof(nvbx_component));\n' + "".join('  printf(" %%zu", offsetof(nvbx_component, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    assert got == [72, 8, 0, 4, 8, 20, 32, 56, 60]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert C.sizeof(_lib.Component) == 72 and C.alignment(_lib.Component) == 8
    assert [f for f, _ in _lib.Component._fields_] == list(FIELDS)
    assert [getattr(_lib.Component, f).offset for f in FIELDS] == got[2:]
    assert SI.COMPONENT_DT.itemsize == 72 and [SI.COMPONENT_DT.fields[f][1] for f in FIELDS] == got[2:]
    assert M.COMPONENT_WORDS == 18 and M.Components._fields == FIELDS + ("centroid_m",)


def test_python_mapper_has_the_two_methods():
    from isaac_ros_nvblox_amd import mapper as M
    assert callable(getattr(M.Mapper, "label_components", None)) and callable(getattr(M.Mapper, "segment_features", None))
