"""The relocalisation entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists,
nvbx_pose_score / nvbx_score_options / nvbx_search_lattice / nvbx_relocalize_result have the layout the header promises (compiled with gcc as
C) and the ctypes structures mirror it field by field.  The calls that need no device -- the defaults, nvbx_search_lattice_poses and every
refusal that is decided before a mapper is looked at -- are made; no compute call is."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import relocalize_independent as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = ("nvbx_default_score_options", "nvbx_score_poses_points", "nvbx_score_poses_depth", "nvbx_search_lattice_poses", "nvbx_relocalize_points",
         "nvbx_relocalize_depth")
STRUCTS = {
    "nvbx_pose_score": ("PoseScore", ("points", "valid", "inliers", "conflicts", "abs_residual_q20")),
    "nvbx_score_options": ("ScoreOptions", ("min_weight", "inlier_distance_m", "conflict_distance_m", "max_depth_m", "subsampling")),
    "nvbx_search_lattice": ("SearchLattice", ("half_extent_m", "half_yaw_rad", "steps")),
    "nvbx_relocalize_result": ("RelocalizeResult", ("status", "best_index", "coarse", "T_coarse", "refined", "align")),
}


def test_library_exports_the_relocalisation_calls(hip_lib):
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
    sp = _lib.SIGNATURES["nvbx_score_poses_points"][1]
    assert len(sp) == 7 and sp[2] is C.c_int64 and sp[4] is C.c_int32
    sd = _lib.SIGNATURES["nvbx_score_poses_depth"][1]
    assert len(sd) == 9 and sd[2] is C.c_int32 and sd[3] is C.c_int32 and sd[6] is C.c_int32
    assert len(_lib.SIGNATURES["nvbx_relocalize_points"][1]) == 10 and len(_lib.SIGNATURES["nvbx_relocalize_depth"][1]) == 12


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
    assert rows[0] == [24, 8, 0, 4, 8, 12, 16]
    assert rows[1] == [20, 4, 0, 4, 8, 12, 16]
    assert rows[2] == [32, 4, 0, 12, 16]
    assert rows[3] == [832, 8, 0, 4, 8, 32, 96, 120]
    for row, (cname, (pyname, fields)) in zip(rows, STRUCTS.items()):
        st = getattr(_lib, pyname)
        assert C.sizeof(st) == row[0] and C.alignment(st) == row[1], cname
        assert [f for f, _ in st._fields_] == list(fields), cname
        assert [getattr(st, f).offset for f in fields] == row[2:], cname
    assert M.RELOC_RESULT_BYTES == 832
    assert _lib.RelocalizeResult.align.offset % 8 == 0 and C.sizeof(_lib.AlignResult) == 712


def test_default_options_and_status_codes(hip_lib):
    from isaac_ros_nvblox_amd import _lib, mapper as M
    o = _lib.ScoreOptions(1.0, 1.0, 1.0, 1.0, 0)
    hip_lib.nvbx_default_score_options(C.byref(o))
    for k, v in RI.SCORE_DEFAULTS.items():
        assert getattr(o, k) == v, k
    hip_lib.nvbx_default_score_options(None)                                       # ignored
    txt = open(HEADER).read()
    for name in ("OK", "NO_CANDIDATE"):
        value = int(re.search(r"#define\s+NVBX_RELOC_%s\s+(\d+)" % name, txt).group(1))
        assert value == getattr(M, "RELOC_" + name) == getattr(RI, name) and M.RELOC_STATUS_NAMES[value] == name


def _lattice(he, hy, steps):
    from isaac_ros_nvblox_amd import _lib
    return _lib.SearchLattice((C.c_float * 3)(*he), hy, (C.c_int32 * 4)(*steps))


def test_search_lattice_poses_are_the_models_and_bad_lattices_are_refused(hip_lib):
    """a host function: no device is touched"""
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, :3] = [[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]
    T0[:3, 3] = [1.5, -2.25, 0.75]
    p0 = T0.ctypes.data_as(C.c_void_p)
    for he, hy, steps in (((0.4, 0.4, 0.0), float(np.deg2rad(20.0)), (5, 5, 1, 9)), ((0.1, 0.2, 0.3), 0.7, (2, 3, 4, 5)), ((0.0, 0.0, 0.0), 0.0, (1, 1, 1, 1))):
        K = int(np.prod(steps))
        out = np.full((K + 1, 16), 7.0, np.float32)
        lat = _lattice(he, hy, steps)
        assert hip_lib.nvbx_search_lattice_poses(p0, C.byref(lat), out.ctypes.data_as(C.c_void_p)) == K
        assert np.array_equal(out[:K].reshape(K, 4, 4).view(np.uint32), RI.lattice_poses(T0, he, hy, steps).view(np.uint32))
        assert (out[K] == 7.0).all()                                                # nothing behind the K poses is written
    out = np.zeros((4, 16), np.float32); po = out.ctypes.data_as(C.c_void_p)
    ok = _lattice((0.1, 0.1, 0.1), 0.1, (1, 1, 1, 1))
    bad_T = T0.copy(); bad_T[1, 3] = np.inf
    refused = [hip_lib.nvbx_search_lattice_poses(None, C.byref(ok), po), hip_lib.nvbx_search_lattice_poses(p0, None, po),
               hip_lib.nvbx_search_lattice_poses(p0, C.byref(ok), None),
               hip_lib.nvbx_search_lattice_poses(bad_T.ctypes.data_as(C.c_void_p), C.byref(ok), po)]
    for he, hy, steps in (((0.1, 0.1, 0.1), 0.1, (0, 1, 1, 1)), ((0.1, 0.1, 0.1), 0.1, (1, 65, 1, 1)), ((0.1, 0.1, 0.1), 0.1, (64, 64, 64, 8)),
                          ((-0.1, 0.1, 0.1), 0.1, (1, 1, 1, 1)), ((0.1, float("nan"), 0.1), 0.1, (1, 1, 1, 1)), ((0.1, 0.1, 0.1), float("inf"), (1, 1, 1, 1)),
                          ((0.1, 0.1, 0.1), -1.0, (1, 1, 1, 1))):
        assert not RI.lattice_ok(he, hy, steps)
        refused.append(hip_lib.nvbx_search_lattice_poses(p0, C.byref(_lattice(he, hy, steps)), po))
    assert refused == [-1] * len(refused), refused
    assert b"nvbx_search_lattice_poses" in hip_lib.nvbx_last_error() and not out.any()


def test_a_null_mapper_is_refused_by_every_call(hip_lib):
    T0 = np.eye(4, dtype=np.float32); p0 = T0.ctypes.data_as(C.c_void_p)
    lat = _lattice((0.1, 0.1, 0.1), 0.1, (1, 1, 1, 1))
    buf = np.zeros(1024, np.uint8); pb = buf.ctypes.data_as(C.c_void_p)
    assert hip_lib.nvbx_score_poses_points(None, pb, 1, pb, 1, None, pb) == -1
    assert hip_lib.nvbx_score_poses_depth(None, pb, 1, 1, None, pb, 1, None, pb) == -1
    assert hip_lib.nvbx_relocalize_points(None, pb, 1, p0, C.byref(lat), None, 0, None, None, pb) == -1
    assert hip_lib.nvbx_relocalize_depth(None, pb, 1, 1, None, p0, C.byref(lat), None, 0, None, None, pb) == -1


def test_python_mapper_has_the_methods():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("score_options", "score_poses", "search_lattice", "relocalize_points", "relocalize_depth"):
        assert callable(getattr(M.Mapper, name, None)), name
    for name in ("status", "best_index", "coarse", "T_coarse", "refined", "T_L_S"):
        assert hasattr(M.RelocalizeResult, name), name
    assert M.PoseScore._fields == RI.Score._fields
