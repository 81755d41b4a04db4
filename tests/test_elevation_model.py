"""The model of tests/elevation_independent.py, checked without a GPU: its heights against an analytic tilted plane, its status, classes and
distances against a second, brute-force walk in pure Python, its distances against scipy's Euclidean distance transform, and
csrc/nvbx_terrain_math.h, compiled as C, against its classes and gradients on edge values."""
import ctypes
import math
import os
import subprocess

import numpy as np

import elevation_independent as EI

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")


# ---- heights
def test_heights_of_a_tilted_plane():
    """d = zc - (a x + b y + c) is linear in z, so the interpolated crossing of every column is the plane's height at the column's centre.
    Tolerance: the scene lies in |z| < 2 m, where a float32 ulp is 2^-22 m.  The voxel centre takes three roundings, the final sum one, each
    at most half an ulp of 2 m; the stored distances carry 2^-24 relative error on |d| < 0.1 m and the quotient a few ulp of 1, which the
    factor voxel_size = 0.05 brings below 1e-8 m.  Four ulp of 2 m, 4 x 2^-22 = 9.6e-7 m, bound the sum."""
    tol = 4.0 * 2.0 ** -22
    a, b, c = 0.21, -0.13, 1.1
    tsdf = EI.heightfield_blocks(lambda X, Y: a * X + b * Y + c, range(-2, 2), range(-1, 2), range(0, 5))
    box = (-16, -8, 24, 32, 0, 39)
    h, st = EI.elevation(tsdf, box)
    assert (st == EI.SURFACE).all()
    r, cc = np.mgrid[0:24, 0:32]
    want = a * ((box[0] + cc + 0.5) * EI.VS) + b * ((box[1] + r + 0.5) * EI.VS) + c
    assert want.min() > 0.5 and want.max() < 1.9
    err = np.abs(h.astype(np.float64) - want).max()
    assert err <= tol, err


# ---- a second walk, pure Python
def _walk_status(tsdf, box, mw):
    x0, y0, rows, cols, z_lo, z_hi = box
    st = np.zeros((rows, cols), np.uint8)

    def voxel(gx, gy, gz):
        blk = tsdf.get((gx >> 3, gy >> 3, gz >> 3))
        if blk is None:
            return None
        v = blk[((gx & 7) << 6) + ((gy & 7) << 3) + (gz & 7)]
        d, w = F32(v["distance"]), F32(v["weight"])
        return d if (w >= F32(mw) and not math.isnan(d)) else None
    for r in range(rows):
        for c in range(cols):
            col = [voxel(x0 + c, y0 + r, gz) for gz in range(z_lo, z_hi + 1)]
            if all(d is None for d in col):
                st[r, c] = EI.UNKNOWN
                continue
            tops = [i for i, d in enumerate(col) if d is not None and d <= 0]
            if not tops:
                st[r, c] = EI.VOID
            elif tops[-1] + 1 < len(col) and col[tops[-1] + 1] is not None:
                st[r, c] = EI.SURFACE
            else:
                st[r, c] = EI.BLOCKED
    return st


def test_status_against_a_column_walk():
    seen = set()
    for seed in (1, 2, 3):
        tsdf = EI.drawn_map(seed)
        h, st = EI.elevation(tsdf, EI.DRAWN_BOX)
        assert np.array_equal(st, _walk_status(tsdf, EI.DRAWN_BOX, EI.MIN_WEIGHT)), seed
        assert (h[st != EI.SURFACE] == F32(1000.0)).all() and (np.abs(h[st == EI.SURFACE]) < 2.0).all()
        seen |= set(np.unique(st).tolist())
    assert seen == {0, 1, 2, 3}


def _walk_classes_and_distance(h, st, o, vs):
    rows, cols = st.shape
    cls = np.zeros((rows, cols), np.uint8)
    for r in range(rows):
        for c in range(cols):
            s = int(st[r, c])
            if s == EI.BLOCKED or (s == EI.VOID and o["void_is_hazard"]):
                cls[r, c] = EI.T_HAZARD
            elif s == EI.SURFACE:
                nb = [(r + dr, c + dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if 0 <= r + dr < rows and 0 <= c + dc < cols and st[r + dr, c + dc] == EI.SURFACE]
                step = max([abs(F32(h[r, c] - h[q])) for q in nb if q != (r, c)] or [F32(0)])

                def grad(m, p):
                    km, kp = m in nb, p in nb
                    if km and kp:
                        return F32(F32(h[p] - h[m]) / F32(F32(2.0) * vs))
                    if kp:
                        return F32(F32(h[p] - h[r, c]) / vs)
                    if km:
                        return F32(F32(h[r, c] - h[m]) / vs)
                    return F32(0)
                gx, gy = grad((r, c - 1), (r, c + 1)), grad((r - 1, c), (r + 1, c))
                s2 = F32(F32(gx * gx) + F32(gy * gy))
                lim = F32(F32(o["max_slope_tan"]) * F32(o["max_slope_tan"]))
                ok = step <= F32(o["max_step_m"]) and s2 <= lim and len(nb) >= o["min_known"]
                cls[r, c] = EI.T_OK if ok else EI.T_HAZARD
    R = o["distance_radius_px"]
    haz = [tuple(p) for p in np.argwhere(cls == EI.T_HAZARD)]
    m = np.full((rows, cols), R * R + 1, np.int64)
    for r in range(rows):
        for c in range(cols):
            for (hr, hc) in haz:
                s = (hr - r) ** 2 + (hc - c) ** 2
                if s <= R * R and s < m[r, c]:
                    m[r, c] = s
    return cls, m


def test_classes_and_distances_against_a_brute_force_walk():
    vs = F32(EI.VS)
    for k, (shape, kw) in enumerate((((9, 11), {}), ((17, 13), dict(void_is_hazard=1, min_known=1, distance_radius_px=4)),
                                     ((12, 12), dict(max_step_m=0.03, max_slope_tan=0.3, min_known=9, distance_radius_px=32)))):
        h, st = EI.random_image(shape, 40 + k)
        got = EI.traversability(h, st, **kw)
        o = EI.options(**kw)
        cls, m = _walk_classes_and_distance(h, st, o, vs)
        assert np.array_equal(got["class"], cls), (shape, kw)
        assert set(np.unique(cls).tolist()) == {0, 1, 2}
        ok = cls == EI.T_OK
        assert np.array_equal(got["m"][ok], m[ok])
        R = o["distance_radius_px"]
        want = np.where(m <= R * R, vs * np.sqrt(m.astype(F32)), vs * F32(R + 1)).astype(F32)
        assert np.array_equal(got["distance"][ok], want[ok])
        assert (got["distance"][cls == EI.T_HAZARD] == 0).all() and (got["distance"][cls == EI.T_UNKNOWN] == F32(1000.0)).all()


def test_distances_against_scipys_distance_transform():
    from scipy import ndimage
    for k, shape in enumerate(((40, 50), (65, 65))):
        h, st = EI.random_image(shape, 60 + k)
        for R in (1, 15, 32):
            got = EI.traversability(h, st, distance_radius_px=R)
            edt = ndimage.distance_transform_edt(got["class"] != EI.T_HAZARD)          # pixels to the nearest hazard, float64
            m = np.rint(edt * edt).astype(np.int64)
            sel = (got["class"] == EI.T_OK) & (m <= R * R)
            assert sel.any() and np.array_equal(got["m"][sel], m[sel]), (shape, R)
            far = (got["class"] == EI.T_OK) & (m > R * R)
            assert (got["m"][far] == R * R + 1).all()
            assert np.array_equal(got["distance"][far], np.full(int(far.sum()), F32(EI.VS) * F32(R + 1), F32))


# ---- the header the kernels classify with, compiled as C
def test_the_shared_header_classifies_as_the_model(tmp_path):
    src = tmp_path / "terrain.c"; so = tmp_path / "terrain.so"
    src.write_text('#include "nvbx_terrain_math.h"\n'
                   "int cls(int status, float step, float slope2, int n_known, const nvbx_terrain_options* o) { return nvbx_terrain_class((uint8_t)status, step, slope2, n_known, o); }\n"
                   "float grad(int km, int kp, float hm, float h, float hp, float vs) { return nvbx_terrain_grad(km, kp, hm, h, hp, vs); }\n"
                   "int observed(float d, float w, float mw) { return nvbx_elev_observed(d, w, mw); }\n"
                   "int refused(const nvbx_terrain_options* o) { return nvbx_terrain_options_problem(o) != 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so), "-lm"])
    lib = ctypes.CDLL(str(so))
    from isaac_ros_nvblox_amd import _lib
    lib.cls.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    lib.grad.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 4; lib.grad.restype = ctypes.c_float
    lib.observed.argtypes = [ctypes.c_float] * 3
    nan, inf = float("nan"), float("inf")
    up = lambda v: float(np.nextafter(F32(v), F32(inf)))      # noqa: E731
    for kw in ({}, dict(void_is_hazard=1), dict(max_step_m=0.0, max_slope_tan=0.0, min_known=1), dict(min_known=9), dict(max_step_m=inf, max_slope_tan=inf)):
        o = EI.options(**kw)
        co = _lib.TerrainOptions(**o)
        assert lib.refused(ctypes.byref(co)) == 0, kw
        lim = float(F32(o["max_slope_tan"]) * F32(o["max_slope_tan"]))
        steps = [0.0, o["max_step_m"], up(o["max_step_m"]), nan, inf]
        slopes = [0.0, lim, up(lim), nan, inf]
        for status in (0, 1, 2, 3):
            for step in steps:
                for s2 in slopes:
                    for nk in (1, 4, 5, 8, 9):
                        want = EI.classes(np.array([[status]], np.uint8), np.array([[nk]]), np.array([[step]], F32), np.array([[s2]], F32), o)[0, 0]
                        assert lib.cls(status, step, s2, nk, ctypes.byref(co)) == int(want), (kw, status, step, s2, nk)
    vs = F32(EI.VS)
    for km in (0, 1):
        for kp in (0, 1):
            for hm, h, hp in ((1.0, 1.02, 1.07), (0.3, 0.3, 0.3), (-1.5, 0.25, 1.9)):
                want = EI._grad(km, kp, F32(hm), F32(h), F32(hp), vs)
                assert F32(lib.grad(km, kp, hm, h, hp, float(vs))) == F32(want), (km, kp, hm, h, hp)
    mw = float(F32(1e-4))
    below = float(np.nextafter(F32(1e-4), F32(0)))
    assert [lib.observed(0.1, mw, mw), lib.observed(0.1, below, mw), lib.observed(nan, 1.0, mw), lib.observed(0.1, nan, mw), lib.observed(-0.1, 0.0, 0.0)] == [1, 0, 0, 0, 1]
    for kw in (dict(max_step_m=nan), dict(max_step_m=-0.01), dict(max_slope_tan=nan), dict(max_slope_tan=-1.0), dict(unknown_value=nan),
               dict(min_known=0), dict(min_known=10), dict(distance_radius_px=-1), dict(distance_radius_px=33)):
        co = _lib.TerrainOptions(**EI.options(**kw))
        assert lib.refused(ctypes.byref(co)) == 1, kw


def test_the_kerb_scene_leaves_one_way_up():
    """the drawn scene of the end-to-end GPU test: the kerb is a hazard everywhere but on the ramp's middle row"""
    h, st = EI.elevation(EI.kerb_blocks(), EI.KERB_BOX)
    assert (st == EI.SURFACE).all()
    assert abs(float(h[20, 5]) - 0.30) < 1e-6 and abs(float(h[20, 40]) - 0.45) < 1e-6
    t = EI.traversability(h, st)
    kerb = t["class"][:, 31] == EI.T_HAZARD
    assert kerb[12:31].all() and kerb[1:7].all() and t["class"][9, 31] == EI.T_OK
    assert (t["class"][9, 1:47] == EI.T_OK).all()
