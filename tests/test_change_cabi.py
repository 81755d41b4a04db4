"""The change-detection entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_change_options and nvbx_change_result have the layout the header promises (compiled with gcc as C11, the header alone as C99) and the
ctypes structures mirror them field by field; the defaults of the library and of the Python methods.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_find_changes": 11, "nvbx_change_clusters": 17}
OPTION_FIELDS = ("min_weight", "ref_min_weight", "free_distance_m", "occupied_distance_m", "sampling", "pad")
RESULT_FIELDS = ("blocks_scanned", "voxels_compared", "voxels_appeared", "voxels_removed", "blocks_changed", "status", "pad")


def test_library_exports_the_change_calls(hip_lib):
    for s in list(NAMES) + ["nvbx_default_change_options"]:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_change_calls_with_the_headers_argument_lists():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for s, n_args in NAMES.items():
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        params = [p.strip() for p in decl.group(1).split(",")]
        assert res is C.c_int and len(args) == len(params) == n_args, s
        for p, a in zip(params, args):
            if "*" in p or "[" in p:
                assert a in (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(_lib.ChangeOptions)), (s, p, a)      # a pointer
            else:
                assert a is kinds[p.split()[0]], (s, p, a)                                                     # a scalar of the header's type
        assert args[3] == C.POINTER(_lib.ChangeOptions) and "nvbx_change_options" in params[3]
        assert "nvbx_change_result" in params[-1] and "nvbx_mapper" in params[0] and "nvbx_mapper" in params[1]
    # the clusters call takes the argument tail of nvbx_frontier_clusters between the box and the result
    tail = lambda name, a, b: [p.strip() for p in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1).split(",")][a:b]      # noqa: E731
    assert tail("nvbx_change_clusters", 5, 16) == tail("nvbx_frontier_clusters", 5, 16)
    assert _lib.SIGNATURES["nvbx_default_change_options"] == (None, [C.POINTER(_lib.ChangeOptions)])
    assert re.search(r"\bvoid\s+nvbx_default_change_options\s*\(\s*nvbx_change_options\s*\*", txt)
    for k, v in (("OK", 0), ("EMPTY_MAP", 1), ("EMPTY_REFERENCE", 2), ("NO_OVERLAP", 3)):
        assert re.search(r"#define\s+NVBX_CHANGE_%s\s+%d\b" % (k, v), txt), k


def test_struct_layouts_of_the_header_and_the_mirror(tmp_path):
    from isaac_ros_nvblox_amd import _lib
    src = tmp_path / "t.c"; exe = tmp_path / "t"
    body = ""
    for name, fields in (("nvbx_change_options", OPTION_FIELDS), ("nvbx_change_result", RESULT_FIELDS)):
        body += '  printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (name, name)
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields) + '  printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nvblox_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [list(map(int, line.split())) for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", HEADER])      # plain C99
    assert rows[0] == [24, 4, 0, 4, 8, 12, 16, 20]
    assert rows[1] == [64, 8, 0, 8, 16, 24, 32, 40, 44]
    for struct, fields, row in ((_lib.ChangeOptions, OPTION_FIELDS, rows[0]), (_lib.ChangeResult, RESULT_FIELDS, rows[1])):
        assert C.sizeof(struct) == row[0] and C.alignment(struct) == row[1]
        assert [f for f, _ in struct._fields_] == list(fields)
        assert [getattr(struct, f).offset for f in fields] == row[2:]
    # the header states the sizes and offsets, as the other records do
    txt = open(HEADER).read()
    assert re.search(r"\}\s*nvbx_change_options;\s*/\*\s*24 bytes; offsets 0 4 8 12 16 20\s*\*/", txt)
    assert re.search(r"\}\s*nvbx_change_result;\s*/\*\s*64 bytes, 8-byte aligned DEVICE memory; offsets 0 8 16 24 32 40 44\s*\*/", txt)


def test_library_defaults(hip_lib):
    from isaac_ros_nvblox_amd import _lib
    o = _lib.ChangeOptions(9.0, 9.0, 9.0, 9.0, 9, 9)
    hip_lib.nvbx_default_change_options(C.byref(o))
    assert (o.min_weight, o.ref_min_weight) == (C.c_float(1e-4).value, C.c_float(1e-4).value)
    assert (o.free_distance_m, o.occupied_distance_m, o.sampling, o.pad) == (0.0, 0.0, 0, 0)
    hip_lib.nvbx_default_change_options(None)      # tolerated


def test_python_mapper_has_the_methods_and_their_defaults():
    import inspect
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("find_changes", "change_clusters"):
        assert callable(getattr(M.Mapper, name, None)), name
        p = inspect.signature(getattr(M.Mapper, name)).parameters
        assert list(p)[1:3] == ["ref", "T_M_R"]
        assert (p["min_weight"].default, p["ref_min_weight"].default, p["free_distance_m"].default, p["occupied_distance_m"].default,
                p["sampling"].default, p["box_m"].default, p["out"].default) == (1e-4, 1e-4, None, 0.0, "trilinear", None, None)
    p = inspect.signature(M.Mapper.change_clusters).parameters
    assert (p["connectivity"].default, p["min_voxels"].default) == (26, 8)
    assert M.CHANGE_STATUS_NAMES == {0: "OK", 1: "EMPTY_MAP", 2: "EMPTY_REFERENCE", 3: "NO_OVERLAP"}
    assert M.CHANGE_RESULT_BYTES == 64 and M.CHANGE_SAMPLING == {"trilinear": 0, "nearest": 1}
    assert isinstance(M.ChangeResult.status_name, property)
