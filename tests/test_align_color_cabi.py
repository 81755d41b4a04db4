"""The colour point query and the alignment calls with a colour term exist: libnvblox_hip.so exports them, the ctypes mirror carries them with
the header's argument lists, nvbx_align_color_options / nvbx_align_color_result have the layout the header promises (compiled with gcc as C)
and the ctypes structures mirror it, the defaults are the documented ones.  The last test (gpu: a refusal needs a mapper) goes through every
refusal the calls add, with its text; nothing is launched by it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_query_colors": 8, "nvbx_default_align_color_options": 1, "nvbx_align_points_color": 9, "nvbx_align_depth_color": 11,
         "nvbx_linearize_points_color": 16}
STRUCTS = {
    "nvbx_align_color_options": ("AlignColorOptions", ("color_weight", "min_color_weight", "color_huber_levels", "pad")),
    "nvbx_align_color_result": ("AlignColorResult", ("color_cost_first", "color_cost_last", "n_color_first", "n_color_last")),
}


def test_library_exports_the_colour_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_colour_calls_with_the_headers_argument_counts():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s, count in NAMES.items():
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        assert (res is C.c_int) == (decl.group(1) == "int") and (res is None) == (decl.group(1) == "void")
        assert len(args) == len(decl.group(2).split(",")) == count, s
    assert _lib.SIGNATURES["nvbx_query_colors"][1][2] is C.c_int64 and _lib.SIGNATURES["nvbx_query_colors"][1][3] is C.c_float
    assert _lib.SIGNATURES["nvbx_align_points_color"][1][3] is C.c_int64
    assert _lib.SIGNATURES["nvbx_align_depth_color"][1][3] is C.c_int32 and _lib.SIGNATURES["nvbx_align_depth_color"][1][4] is C.c_int32
    assert _lib.SIGNATURES["nvbx_linearize_points_color"][1][3] is C.c_int64


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
    assert rows[0] == [16, 4, 0, 4, 8, 12]
    assert rows[1] == [24, 8, 0, 8, 16, 20]
    for row, (cname, (pyname, fields)) in zip(rows, STRUCTS.items()):
        st = getattr(_lib, pyname)
        assert C.sizeof(st) == row[0] and C.alignment(st) == row[1], cname
        assert [f for f, _ in st._fields_] == list(fields), cname
        assert [getattr(st, f).offset for f in fields] == row[2:], cname
    assert M.ALIGN_COLOR_RESULT_BYTES == 712 + 24 and M.ALIGN_RESULT_BYTES % 8 == 0


def test_default_colour_options(hip_lib):
    from isaac_ros_nvblox_amd import _lib
    import align_color_independent as AC
    o = _lib.AlignColorOptions(-1.0, -1.0, -1.0, 7)
    hip_lib.nvbx_default_align_color_options(C.byref(o))
    assert (o.color_weight, o.min_color_weight, o.color_huber_levels, o.pad) == (1.0, C.c_float(1e-4).value, 0.0, 0)
    assert AC.COLOR_DEFAULTS == dict(color_weight=1.0, min_color_weight=1e-4, color_huber_levels=0.0)
    hip_lib.nvbx_default_align_color_options(None)          # (NULL: nothing happens)


def test_python_mapper_has_the_colour_methods():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("query_color", "align_color_options", "align_points_color", "align_depth_color", "linearize_points_color"):
        assert callable(getattr(M.Mapper, name, None)), name
    for name in ("n_color", "color_rmse_first", "color_rmse_last", "T_L_S", "rmse_last"):
        assert hasattr(M.AlignColorResult, name), name
    assert issubclass(M.AlignColorResult, M.AlignResult)


@pytest.mark.gpu
def test_every_refusal_with_its_text(hip_lib):
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M
    lib = hip_lib
    m = M.Mapper(M.default_params(), device=0, block_capacity=1 << 10)
    occ = M.Mapper(M.default_params(projective_layer_type=1), device=0, block_capacity=1 << 10)
    h, ho = m._h, occ._h
    n = 8
    pts = torch.zeros((n, 3), dtype=torch.float32, device="cuda"); col = torch.zeros((n, 3), dtype=torch.uint8, device="cuda")
    depth = torch.ones((120, 160), dtype=torch.float32, device="cuda"); rgb = torch.zeros((120, 160, 3), dtype=torch.uint8, device="cuda")
    buf = torch.zeros(M.ALIGN_COLOR_RESULT_BYTES + 8, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n * 8, dtype=torch.float32, device="cuda")
    px, pc, pd, pi, po = (C.c_void_p(t.data_ptr()) for t in (pts, col, depth, rgb, out))
    pb = C.c_void_p(buf.data_ptr()); pcb = C.c_void_p(buf.data_ptr() + 712); odd = C.c_void_p(buf.data_ptr() + 716)
    T = np.eye(4, dtype=np.float32); pT = T.ctypes.data_as(C.c_void_p)
    Tbad = T.copy(); Tbad[0, 3] = np.nan; pTbad = Tbad.ctypes.data_as(C.c_void_p)
    cam = M.Camera(80.0, 80.0, 79.5, 59.5, 160, 120)
    nan = float("nan")

    def refused(rc, text):
        assert rc == -1, (rc, text)
        got = lib.nvbx_last_error().decode()
        assert got == text, (got, text)

    # nvbx_query_colors: nvbx_query_points' refusals, then the weight
    q = "nvbx_query_colors: invalid argument"
    refused(lib.nvbx_query_colors(None, px, n, 1e-4, None, po, None, po), q)
    refused(lib.nvbx_query_colors(h, px, -1, 1e-4, None, po, None, po), q)
    refused(lib.nvbx_query_colors(h, None, n, 1e-4, None, po, None, po), q)
    refused(lib.nvbx_query_colors(h, px, n, 1e-4, po, po, po, None), q)
    refused(lib.nvbx_query_colors(ho, px, n, 1e-4, None, None, None, po), "nvbx_query_colors: an occupancy mapper has no TSDF layer")
    refused(lib.nvbx_query_colors(h, px, n, nan, None, None, None, po), "nvbx_query_colors: min_color_weight is not a number")
    assert lib.nvbx_query_colors(h, None, 0, 1e-4, None, None, None, None) == 0          # n == 0 launches nothing

    def ap(who=None, mapper=h, points=px, colors=pc, count=n, pose=pT, opts=None, copts=None, res=pb, cres=pcb):
        o = None if opts is None else C.byref(opts); co = None if copts is None else C.byref(copts)
        if who == "depth":
            return lib.nvbx_align_depth_color(mapper, points, colors, 120, 160, pose, C.byref(cam), o, co, res, cres)
        if who == "lin":
            return lib.nvbx_linearize_points_color(mapper, points, colors, count, pose, o, co, res, cres, None, None, None, None, None, None, None)
        return lib.nvbx_align_points_color(mapper, points, colors, count, pose, o, co, res, cres)

    def opt(**kw):
        o = _lib.AlignOptions(); lib.nvbx_default_align_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def copt(**kw):
        o = _lib.AlignColorOptions(); lib.nvbx_default_align_color_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    for who, name, P, Cc in ((None, "nvbx_align_points_color", px, pc), ("lin", "nvbx_linearize_points_color", px, pc),
                             ("depth", "nvbx_align_depth_color", pd, pi)):
        kw = dict(who=who, points=P, colors=Cc)
        # what the plain calls refuse, in their order and words
        assert ap(**dict(kw, mapper=None)) == -1
        refused(ap(**dict(kw, pose=None)), name + ": the pose and result_dev are required")
        refused(ap(**dict(kw, res=None)), name + ": the pose and result_dev are required")
        refused(ap(**dict(kw, res=C.c_void_p(buf.data_ptr() + 4))), name + ": result_dev must be 8-byte aligned")
        refused(ap(**dict(kw, mapper=ho)), name + ": an occupancy mapper has no TSDF layer")
        refused(ap(**dict(kw, opts=opt(max_iterations=0))), name + ": max_iterations must be 1 .. 64")
        refused(ap(**dict(kw, opts=opt(min_valid=0))), name + ": min_valid must be >= 1")
        refused(ap(**dict(kw, opts=opt(damping=-1.0))), name + ": damping, min_pivot_ratio and the stop thresholds must be finite and >= 0")
        refused(ap(**dict(kw, opts=opt(min_weight=nan))), name + ": min_weight / huber_delta_m / max_depth_m is not a number")
        refused(ap(**dict(kw, pose=pTbad)), name + ": the pose is not finite or out of range")
        if who == "depth":
            refused(ap(**dict(kw, points=None)), name + ": the depth image and the camera are required")
            refused(ap(**dict(kw, opts=opt(subsampling=0))), name + ": subsampling must be >= 1")
        else:
            refused(ap(**dict(kw, count=-1)), name + ": n points need points_xyz_dev")
            refused(ap(**dict(kw, points=None)), name + ": n points need points_xyz_dev")
        # ... a plain refusal comes before a colour one
        refused(ap(**dict(kw, opts=opt(min_valid=0), colors=None, cres=None)), name + ": min_valid must be >= 1")
        # the colour refusals, in their order
        refused(ap(**dict(kw, colors=None, cres=None, copts=copt(color_weight=-1.0))), name + ": the points' colours are required")
        refused(ap(**dict(kw, cres=None, copts=copt(color_weight=-1.0))), name + ": color_result_dev is required")
        refused(ap(**dict(kw, cres=odd, copts=copt(color_weight=-1.0))), name + ": color_result_dev must be 8-byte aligned")
        for bad in (-1.0, nan, float("inf")):
            refused(ap(**dict(kw, copts=copt(color_weight=bad, min_color_weight=nan))), name + ": color_weight must be finite and >= 0")
        refused(ap(**dict(kw, copts=copt(min_color_weight=nan))), name + ": min_color_weight / color_huber_levels is not a number")
        refused(ap(**dict(kw, copts=copt(color_huber_levels=nan))), name + ": min_color_weight / color_huber_levels is not a number")
    # an empty cloud needs no colour pointer; NULL options are the defaults; the refused mappers stay usable
    assert ap(points=None, colors=None, count=0) == 0 and ap() == 0 and ap(who="lin") == 0 and ap(who="depth", points=pd, colors=pi) == 0
    m.synchronize()
    rec = _lib.AlignResult.from_buffer_copy(buf.cpu().numpy().tobytes()[:712])
    assert rec.status == M.ALIGN_TOO_FEW and rec.iterations == 1
