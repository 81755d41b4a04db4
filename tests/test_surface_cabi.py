"""The surface-point and map-registration entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's
argument lists, nvbx_surface_options has the layout the header promises (compiled with gcc as C11, the header alone as C99) and the ctypes
structure mirrors it field by field; the library's defaults; the refusals that need no device.  No compute calls."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_surface_points": 7, "nvbx_align_map": 8, "nvbx_relocalize_map": 10}
OPTION_FIELDS = ("min_weight", "stride", "use_box", "require_color", "box_min_max_vox")
E_INVALID = -1


def test_library_exports_the_calls(hip_lib):
    for s in list(NAMES) + ["nvbx_default_surface_options"]:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_calls_with_the_headers_argument_lists():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    structs = {"nvbx_surface_options": _lib.SurfaceOptions, "nvbx_align_options": _lib.AlignOptions, "nvbx_align_color_options": _lib.AlignColorOptions,
               "nvbx_search_lattice": _lib.SearchLattice, "nvbx_score_options": _lib.ScoreOptions}
    for s, n_args in NAMES.items():
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        params = [p.strip() for p in decl.group(1).split(",")]
        assert res is C.c_int and len(args) == len(params) == n_args, s
        for p, a in zip(params, args):
            if "*" in p or "[" in p:
                named = [v for k, v in structs.items() if re.search(r"\b%s\b" % k, p)]
                assert a is C.c_void_p or (named and a == C.POINTER(named[0])), (s, p, a)
                if named:
                    assert a == C.POINTER(named[0]), (s, p, a)
            else:
                assert a is kinds[p.split()[0]], (s, p, a)
    assert _lib.SIGNATURES["nvbx_default_surface_options"] == (None, [C.POINTER(_lib.SurfaceOptions)])
    # nvbx_relocalize_map takes nvbx_relocalize_points' lattice, options and outputs, with the surface options in between
    tail = lambda name: [re.sub(r"\s+", " ", p.strip()) for p in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1).split(",")]      # noqa: E731
    a, b = tail("nvbx_relocalize_map"), tail("nvbx_relocalize_points")
    assert a[2:4] == b[3:5] and a[5:] == b[5:] and "nvbx_surface_options" in a[4]


def test_struct_layout_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    name = "nvbx_surface_options"
    body = '  printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (name, name)
    body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in OPTION_FIELDS) + '  printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    row = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])
    assert row == [40, 4, 0, 4, 8, 12, 16]
    s = _lib.SurfaceOptions
    assert C.sizeof(s) == row[0] and C.alignment(s) == row[1]
    assert [f for f, _ in s._fields_] == list(OPTION_FIELDS)
    assert [getattr(s, f).offset for f in OPTION_FIELDS] == row[2:]
    assert re.search(r"\}\s*nvbx_surface_options;\s*/\*\s*40 bytes; offsets 0 4 8 12 16\s*\*/", open(HEADER).read())


def test_library_defaults(hip_lib):
    from isaac_ros_nvblox_amd import _lib
    o = _lib.SurfaceOptions(9.0, 9, 9, 9, (C.c_int32 * 6)(*[9] * 6))
    hip_lib.nvbx_default_surface_options(C.byref(o))
    assert (o.min_weight, o.stride, o.use_box, o.require_color) == (C.c_float(1e-4).value, 1, 0, 0)
    assert list(o.box_min_max_vox) == [-(1 << 31)] * 3 + [(1 << 31) - 1] * 3
    hip_lib.nvbx_default_surface_options(None)      # tolerated


def test_refusals_that_need_no_device(hip_lib):
    count = C.c_int64(-7)
    assert hip_lib.nvbx_surface_points(None, None, None, None, None, 0, C.byref(count)) == E_INVALID
    assert b"nvbx_surface_points" in hip_lib.nvbx_last_error() and count.value == -7
    T = (C.c_float * 16)(*[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    res = C.create_string_buffer(1024)
    some = C.cast(C.create_string_buffer(64), C.c_void_p)      # an address that is no mapper: only ever compared
    for dst, src in ((None, None), (some, None), (None, some), (some, some)):
        assert hip_lib.nvbx_align_map(dst, src, T, None, None, None, res, None) == E_INVALID
        assert b"nvbx_align_map" in hip_lib.nvbx_last_error()
        assert hip_lib.nvbx_relocalize_map(dst, src, T, None, None, None, 0, None, None, res) == E_INVALID
        assert b"nvbx_relocalize_map" in hip_lib.nvbx_last_error()
    assert b"same mapper" in hip_lib.nvbx_last_error()


def test_python_mapper_has_the_methods_and_their_defaults():
    from isaac_ros_nvblox_amd import mapper as M
    p = inspect.signature(M.Mapper.surface_points).parameters
    assert (p["color"].default, p["normals"].default, p["capacity"].default, p["out"].default) == (False, False, None, None)
    p = inspect.signature(M.Mapper.align_map).parameters
    assert list(p)[1:3] == ["other", "T_D_S_guess"] and p["color_weight"].default is None and p["out"].default is None
    p = inspect.signature(M.Mapper.relocalize_map).parameters
    assert list(p)[1:6] == ["other", "T0", "half_extent_m", "half_yaw_rad", "steps"]
    assert callable(M.Mapper.surface_options)
