"""The frontier and view-gain entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_gain has the layout the header promises (compiled with gcc as C) and the ctypes structure mirrors it field by field.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_find_frontiers": 10, "nvbx_frontier_clusters": 16, "nvbx_view_gain": 9}
GAIN_FIELDS = ("rays", "unknown_samples", "free_samples", "rays_hit")


def test_library_exports_the_frontier_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_frontier_calls_with_the_headers_argument_lists():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for s, n_args in NAMES.items():
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        params = [p.strip() for p in decl.group(1).split(",")]
        assert res is C.c_int and len(args) == len(params) == n_args, s
        for p, a in zip(params, args):
            if "*" in p or "[" in p:
                assert a in (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(_lib.Camera)), (s, p, a)       # a pointer
            else:
                assert a is kinds[p.split()[0]], (s, p, a)                                               # a scalar of the header's type
    assert _lib.SIGNATURES["nvbx_view_gain"][1][3] == C.POINTER(_lib.Camera)


def test_gain_record_layout_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = '  printf("%zu %zu", sizeof(nvbx_gain), _Alignof(nvbx_gain));\n'
    body += "".join('  printf(" %%zu", offsetof(nvbx_gain, %s));\n' % f for f in GAIN_FIELDS) + '  printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    row = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert row == [16, 4, 0, 4, 8, 12]
    assert C.sizeof(_lib.Gain) == 16 and C.alignment(_lib.Gain) == 4
    assert [f for f, _ in _lib.Gain._fields_] == list(GAIN_FIELDS)
    assert [getattr(_lib.Gain, f).offset for f in GAIN_FIELDS] == row[2:]


def test_python_mapper_has_the_methods_and_their_defaults():
    import inspect
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("find_frontiers", "frontier_clusters", "view_gain"):
        assert callable(getattr(M.Mapper, name, None)), name
    p = inspect.signature(M.Mapper.find_frontiers).parameters
    assert (p["min_weight"].default, p["free_distance_m"].default, p["min_unknown"].default, p["box_m"].default, p["out"].default) == (1e-4, None, 1, None, None)
    p = inspect.signature(M.Mapper.frontier_clusters).parameters
    assert (p["connectivity"].default, p["min_voxels"].default, p["out"].default) == (26, 1, None)
    p = inspect.signature(M.Mapper.view_gain).parameters
    assert list(p)[1:3] == ["poses", "cam"] and p["subsampling"].default is None and p["max_range_m"].default is None and p["out"].default is None
