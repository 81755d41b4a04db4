"""The cost-field entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_cost_options has the layout the header promises (compiled with gcc as C) and the ctypes structure mirrors it field by field, the Python
methods are there with their defaults.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_default_cost_options": 1, "nvbx_cost_field": 9, "nvbx_trace_paths": 11}
OPTION_FIELDS = ("robot_radius_m", "inflation_radius_m", "penalty_per_m", "unknown_value", "max_penalty", "unknown_penalty", "allow_unknown", "pad")


def test_library_exports_the_plan_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_plan_calls_with_the_headers_argument_lists():
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
            if "nvbx_cost_options" in p:
                assert a == C.POINTER(_lib.CostOptions), (s, p, a)
            elif "*" in p:
                assert a is C.c_void_p, (s, p, a)                       # a pointer
            else:
                assert a is kinds[p.split()[0]], (s, p, a)               # a scalar of the header's type
    assert re.search(r"#define\s+NVBX_COST_UNREACHED\s+0x7fffffff\b", txt)


def test_option_record_layout_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib, mapper as M
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = '  printf("%zu %zu", sizeof(nvbx_cost_options), _Alignof(nvbx_cost_options));\n'
    body += "".join('  printf(" %%zu", offsetof(nvbx_cost_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %d\\n", NVBX_COST_UNREACHED == INT32_MAX);\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    row = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert row == [32, 4, 0, 4, 8, 12, 16, 20, 24, 28, 1]
    assert C.sizeof(_lib.CostOptions) == 32 and C.alignment(_lib.CostOptions) == 4
    assert [f for f, _ in _lib.CostOptions._fields_] == list(OPTION_FIELDS)
    assert [getattr(_lib.CostOptions, f).offset for f in OPTION_FIELDS] == row[2:10]
    assert M.COST_UNREACHED == 0x7fffffff


def test_defaults_of_the_options(hip_lib):
    from isaac_ros_nvblox_amd import _lib
    o = _lib.CostOptions()
    hip_lib.nvbx_default_cost_options(C.byref(o))      # host only: no device is touched
    assert [getattr(o, f) for f in OPTION_FIELDS] == [0.25, 0.75, 100.0, 1000.0, 200, 50, 0, 0]


def test_python_mapper_has_the_methods_and_their_defaults():
    import inspect
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("cost_options", "cost_field", "trace_paths", "slice_pixels"):
        assert callable(getattr(M.Mapper, name, None)), name
    p = inspect.signature(M.Mapper.cost_field).parameters
    assert list(p)[1:3] == ["image_dev", "sources_rc"] and p["out"].default is None and p["accepted"].default is None
    assert p["options"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(M.Mapper.trace_paths).parameters
    assert list(p)[1:5] == ["image_dev", "field", "starts_rc", "capacity"] and p["out"].default is None and p["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(M.Mapper.slice_pixels).parameters)[1:] == ["points_xy", "aabb"]
    assert inspect.signature(M.Mapper.cost_options).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
