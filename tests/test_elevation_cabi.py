"""The elevation and traversability entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's
argument lists, nvbx_terrain_options has the layout the header promises (compiled with gcc as C) and the ctypes structure mirrors it field by
field, the constants and the Python methods are there with their defaults.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_default_terrain_options": 1, "nvbx_elevation_map": 11, "nvbx_traversability": 10}
OPTION_FIELDS = ("max_step_m", "max_slope_tan", "unknown_value", "min_known", "void_is_hazard", "distance_radius_px", "pad")
CONSTANTS = {"NVBX_ELEV_UNKNOWN": 0, "NVBX_ELEV_SURFACE": 1, "NVBX_ELEV_BLOCKED": 2, "NVBX_ELEV_VOID": 3,
             "NVBX_TERRAIN_UNKNOWN": 0, "NVBX_TERRAIN_OK": 1, "NVBX_TERRAIN_HAZARD": 2}


def test_library_exports_the_elevation_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_elevation_calls_with_the_headers_argument_lists():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for s, n_args in NAMES.items():
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        params = [p.strip() for p in decl.group(2).split(",")]
        assert res is (C.c_int if decl.group(1) == "int" else None) and len(args) == len(params) == n_args, s
        for p, a in zip(params, args):
            if "nvbx_terrain_options" in p:
                assert a == C.POINTER(_lib.TerrainOptions), (s, p, a)
            elif "*" in p:
                assert a is C.c_void_p, (s, p, a)                       # a pointer
            else:
                assert a is kinds[p.split()[0]], (s, p, a)               # a scalar of the header's type
    for name, value in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), txt), name


def test_option_record_layout_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib, mapper as M
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = '  printf("%zu %zu", sizeof(nvbx_terrain_options), _Alignof(nvbx_terrain_options));\n'
    body += "".join('  printf(" %%zu", offsetof(nvbx_terrain_options, %s));\n' % f for f in OPTION_FIELDS)
    body += "".join('  printf(" %%d", %s);\n' % name for name in CONSTANTS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + '  printf("\\n");\n  return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    row = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert row == [32, 4, 0, 4, 8, 12, 16, 20, 24] + list(CONSTANTS.values())
    assert C.sizeof(_lib.TerrainOptions) == 32 and C.alignment(_lib.TerrainOptions) == 4
    assert [f for f, _ in _lib.TerrainOptions._fields_] == list(OPTION_FIELDS)
    assert [getattr(_lib.TerrainOptions, f).offset for f in OPTION_FIELDS] == row[2:9]
    assert (M.ELEV_UNKNOWN, M.ELEV_SURFACE, M.ELEV_BLOCKED, M.ELEV_VOID, M.TERRAIN_UNKNOWN, M.TERRAIN_OK, M.TERRAIN_HAZARD) == tuple(CONSTANTS.values())


def test_defaults_of_the_options(hip_lib):
    from isaac_ros_nvblox_amd import _lib
    import numpy as np
    o = _lib.TerrainOptions()
    o.pad[0] = 7; o.pad[1] = 7
    hip_lib.nvbx_default_terrain_options(C.byref(o))      # host only: no device is touched
    f32 = lambda v: float(np.float32(v))                  # noqa: E731
    assert [getattr(o, f) for f in OPTION_FIELDS[:6]] == [f32(0.10), 0.5, 1000.0, 5, 0, 15] and list(o.pad) == [0, 0]


def test_python_mapper_has_the_methods_and_their_defaults():
    import inspect
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("terrain_options", "elevation_box", "elevation_map", "traversability"):
        assert callable(getattr(M.Mapper, name, None)), name
    p = inspect.signature(M.Mapper.elevation_box).parameters
    assert list(p)[1:] == ["aabb", "z_min_m", "z_max_m", "rows", "cols"] and p["rows"].default is None and p["cols"].default is None
    p = inspect.signature(M.Mapper.elevation_map).parameters
    assert list(p)[1:] == ["x0", "y0", "rows", "cols", "z_lo", "z_hi", "min_weight", "unknown_value", "out"]
    assert (p["min_weight"].default, p["unknown_value"].default, p["out"].default) == (1e-4, 1000.0, None)
    p = inspect.signature(M.Mapper.traversability).parameters
    assert list(p)[1:] == ["height", "status", "step", "slope", "distance", "out", "options"]
    assert (p["step"].default, p["slope"].default, p["distance"].default, p["out"].default) == (False, False, True, None)
    assert p["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(M.Mapper.terrain_options).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
