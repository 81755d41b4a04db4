"""The numpy model of nvbx_surface_points (tests/surface_independent.py) against geometry it cannot get right by accident: drawn planes and a
sphere, and each rule of SEMANTICS.md "Surface points" on the smallest field that shows it.  No GPU."""
import numpy as np
import pytest

import surface_independent as SI

F32 = np.float32
U = 2.0 ** -24      # half an ulp of 1 in float32: the relative error of one correctly rounded operation


def _flat(d=1.0, w=1.0):
    return {"d": np.full((8, 8, 8), d, F32), "w": np.full((8, 8, 8), w, F32)}


# ---- planes
@pytest.mark.parametrize("normal,offset", [((0, 0, 1), 0.31), ((1, 0, 0), -0.2), ((0.3, -0.5, 0.81), 0.17), ((-1, 2, 0.01), 0.05), ((1, 1, 1), 0.0)])
def test_every_crossing_of_a_plane_field_lies_on_the_plane(normal, offset):
    """d = n . x - c with |n| = 1 is linear, so the interpolated crossing is the edge's true intersection but for rounding.  With the stored
    distances d_i (1 + e_i), |e_i| <= u = 2^-24, and opposite signs, |d0| + |d1| = |d1 - d0|, so the difference's relative error is <= u + u,
    the quotient's <= 4 u to first order, and n . p - c = d0 - d0 (1 + <= 4.5 u): at most 4.5 u |d0| <= 4.5 u vs.  vs * t and the final sum
    add u vs and u |X|, the voxel centre three operations of at most u |X| each on each of the three axes, |X| the largest coordinate:
    |n . p - c| <= u (6 vs + 10 |X|) covers it."""
    vs = 0.05
    n = np.asarray(normal, np.float64); n /= np.linalg.norm(n)
    keys = [(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)]
    blocks = SI.blocks_from_function(keys, lambda x, y, z: n[0] * x + n[1] * y + n[2] * z - offset, vs)
    rows = SI.surface_rows(blocks, vs)
    assert len(rows["t"]) > 200
    p = rows["points"].astype(np.float64)
    bound = U * (6 * vs + 10 * np.abs(p).max())
    assert np.abs(p @ n - offset).max() <= bound
    # every edge of the lattice whose ends differ in sign is there exactly once (blocks at the border have no neighbour: those edges are open)
    assert len(SI.row_set(rows["points"])) == len(rows["t"])


def test_sphere_crossings_within_the_interpolation_bound():
    """d = |x - c| - R.  Along an edge of length vs the second derivative of d is at most 1 / rho, rho the distance from the centre, and an edge
    that crosses the surface stays at rho >= R - vs; linear interpolation over h = vs is off by at most max|d''| h^2 / 8.  Where the interpolant
    is zero the true d is therefore at most vs^2 / (8 (R - vs)) -- and d IS the distance from the sphere.  Rounding as in the plane test."""
    vs, R = 0.04, 0.5
    c = np.array([0.013, -0.021, 0.008])
    keys = [(x, y, z) for x in range(-3, 3) for y in range(-3, 3) for z in range(-3, 3)]
    blocks = SI.blocks_from_function(keys, lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - R, vs)
    rows = SI.surface_rows(blocks, vs)
    assert len(rows["t"]) > 1000
    p = rows["points"].astype(np.float64)
    bound = vs * vs / (8 * (R - vs)) + U * (6 * vs + 10 * np.abs(p).max())
    err = np.abs(np.linalg.norm(p - c, axis=1) - R)
    assert err.max() <= bound, (err.max(), bound)
    assert err.max() > 0.1 * bound      # (the bound is not slack by orders of magnitude: the field is curved)


# ---- the rules, one by one
def _rows_of(blk, **kw):
    return SI.surface_rows({(0, 0, 0): blk}, 0.1, **kw)


def test_zero_at_the_origin_voxel_crosses_towards_positive_only():
    b = _flat(1.0)
    b["d"][2, 3, 4] = 0.0                                  # (0 <= 0) != (1 <= 0): crossings on its three outgoing edges ...
    rows = _rows_of(b)
    out = [(t, a) for t, a in zip(rows["t"].tolist(), rows["axis"].tolist())]
    t0 = 2 * 64 + 3 * 8 + 4
    assert out == [(t0 - 64, 0), (t0 - 8, 1), (t0 - 1, 2), (t0, 0), (t0, 1), (t0, 2)]      # ... and on the three incoming ones (d1 == 0)
    centre = ((np.array([2, 3, 4], F32) * F32(0.1)) + F32(0.1) * F32(0.5)).astype(F32)
    assert all(np.array_equal(p, centre) for p in rows["points"][3:])                      # -0 / 1 = -0: the origin's own centre, bit for bit
    # -1 / (0 - 1) = 1: the lower voxel's centre + vs, the same point by another chain of three roundings: within two ulps of the coordinate
    assert all(np.abs(p - centre).max() <= 2 * np.spacing(centre.max()) for p in rows["points"][:3])
    b = _flat(-1.0); b["d"][2, 3, 4] = 0.0                 # zero among negatives: (0 <= 0) == (-1 <= 0) everywhere
    assert len(_rows_of(b)["t"]) == 0


def test_nan_and_weight_below_threshold_are_unobserved():
    b = _flat(1.0); b["d"][1, 1, 1] = -1.0
    assert len(_rows_of(b)["t"]) == 6
    for spoil in ("nan", "weight"):
        c = {"d": b["d"].copy(), "w": b["w"].copy()}
        if spoil == "nan":
            c["d"][1, 1, 2] = np.nan                       # the +z neighbour of the negative voxel
        else:
            c["w"][1, 1, 2] = 0.5e-4
        rows = _rows_of(c)
        assert len(rows["t"]) == 5 and (1 * 64 + 1 * 8 + 1, 2) not in set(zip(rows["t"].tolist(), rows["axis"].tolist()))
    c = {"d": b["d"].copy(), "w": b["w"].copy()}; c["w"][1, 1, 2] = 0.5e-4
    assert len(_rows_of(c, min_weight=0.5e-4)["t"]) == 6  # the threshold is inclusive


def test_box_is_inclusive_and_applies_to_the_origin_voxel():
    b = _flat(1.0); b["d"][3, 3, 3] = -1.0
    t0 = 3 * 64 + 3 * 8 + 3
    rows = _rows_of(b, box=(3, 3, 3, 3, 3, 3))             # the negative voxel alone: its three outgoing edges
    assert list(zip(rows["t"].tolist(), rows["axis"].tolist())) == [(t0, 0), (t0, 1), (t0, 2)]
    rows = _rows_of(b, box=(2, 3, 3, 2, 3, 3))             # its -x neighbour alone: the edge into it
    assert list(zip(rows["t"].tolist(), rows["axis"].tolist())) == [(t0 - 64, 0)]


def test_stride_uses_the_mathematical_modulo_on_negative_coordinates():
    assert SI.floor_mod(np.array([-7, -6, -3, -1, 0, 2, 3]), 3).tolist() == [2, 0, 0, 2, 0, 2, 0]
    blocks = {(-1, -1, -1): _flat(-1.0), (0, -1, -1): _flat(1.0)}      # a sign change across the x border of two blocks, at g_x = -1 -> 0
    rows = SI.surface_rows(blocks, 0.1, stride=1)
    assert len(rows["t"]) == 64
    assert len(SI.surface_rows(blocks, 0.1, stride=3)["t"]) == 0        # g_x = -1 is no multiple of 3
    blocks[(-1, -1, -1)]["d"][5:, :, :] = 1.0                            # now between g_x = -4 and -3
    rows = SI.surface_rows(blocks, 0.1, stride=2)
    g = 8 * rows["block"] + np.stack([rows["t"] >> 6, (rows["t"] >> 3) & 7, rows["t"] & 7], 1)
    assert len(rows["t"]) == 16 and set(g[:, 0].tolist()) == {-4} and set(g[:, 1].tolist()) == {-8, -6, -4, -2}
    assert len(SI.surface_rows(blocks, 0.1, stride=4)["t"]) == 4


def test_colour_comes_from_the_nearer_end_and_require_color_drops_the_rest():
    b = _flat(1.0); b["d"][1, 1, 1] = -0.25                # |d0| < |d1| going out, |d0| > |d1| coming in
    b["rgb"] = np.zeros((8, 8, 8, 3), np.uint8); b["cw"] = np.zeros((8, 8, 8), F32)
    b["rgb"][1, 1, 1] = (10, 20, 30); b["cw"][1, 1, 1] = 1.0
    b["rgb"][0, 1, 1] = (1, 2, 3); b["cw"][0, 1, 1] = 0.0  # a colour without weight is none
    rows = _rows_of(b)
    assert len(rows["t"]) == 6 and rows["colors"].tolist() == [[10, 20, 30]] * 6      # the negative voxel is the nearer end of all six edges
    b["d"][1, 1, 1] = -4.0                                 # now the far end of all six: the neighbours' colours, which have no weight
    assert _rows_of(b)["colors"].tolist() == [[0, 0, 0]] * 6
    assert len(_rows_of(b, require_color=True)["t"]) == 0
    b["cw"][1, 1, 2] = 2.0; b["rgb"][1, 1, 2] = (7, 8, 9)
    rows = _rows_of(b, require_color=True)
    assert list(zip(rows["t"].tolist(), rows["axis"].tolist())) == [(64 + 8 + 1, 2)] and rows["colors"].tolist() == [[7, 8, 9]]
    # |d0| == |d1|: the origin
    b = _flat(1.0); b["d"][1, 1, 1] = -1.0
    b["rgb"] = np.zeros((8, 8, 8, 3), np.uint8); b["cw"] = np.ones((8, 8, 8), F32)
    b["rgb"][1, 1, 1] = (5, 5, 5); b["rgb"][0, 1, 1] = (6, 6, 6); b["rgb"][2, 1, 1] = (7, 7, 7)
    rows = _rows_of(b)
    got = {(t, a): c for t, a, c in zip(rows["t"].tolist(), rows["axis"].tolist(), rows["colors"].tolist())}
    assert got[(0 * 64 + 8 + 1, 0)] == [6, 6, 6] and got[(64 + 8 + 1, 0)] == [5, 5, 5]


def test_missing_and_layerless_neighbour_blocks_give_no_crossing():
    neg, pos = _flat(-1.0), _flat(1.0)
    assert len(SI.surface_rows({(0, 0, 0): neg}, 0.1)["t"]) == 0
    assert len(SI.surface_rows({(0, 0, 0): neg, (1, 0, 0): pos, (0, 1, 0): {"rgb": np.zeros((8, 8, 8, 3), np.uint8), "cw": np.ones((8, 8, 8), F32)}}, 0.1)["t"]) == 64
    assert len(SI.surface_rows({(0, 0, 0): neg, (-1, 0, 0): pos}, 0.1)["t"]) == 64      # the origin is the lower block
    rows = SI.surface_rows({(0, 0, 0): neg, (-1, 0, 0): pos}, 0.1)
    assert set(map(tuple, rows["block"].tolist())) == {(-1, 0, 0)}


# ---- the room two mappers are registered in (tests/test_gpu_surface.py): the model alone recovers the pose to well below a voxel
def test_the_float64_model_recovers_the_rooms_pose_within_a_tenth_of_a_voxel():
    """Sub-voxel recovery is 0.1 voxel and the angle that is over the room's extent; the GPU test allows twice the distance measured here."""
    import surface_cases as SC
    first, second = SC.room_blocks(None), SC.room_blocks(SC.ROOM_T)
    rows = SI.surface_rows(second, SC.VS)
    planes = SC.room_planes()
    p_d = rows["points"].astype(np.float64) @ SC.ROOM_T[:3, :3].T + SC.ROOM_T[:3, 3]
    on = np.min(np.abs(np.stack([c - p_d @ n for n, c in planes], 1)), 1)
    assert on.max() <= U * (6 * SC.VS + 10 * np.abs(rows["points"]).max()) + 2e-9      # on a plane: the plane test's bound + the field's own f32 storage
    res, (dt, ang), n = SC.room_model_alignment()
    assert n == len(rows["t"]) > 1000 and res["n_valid"] > 800 and len(first) > 40
    assert dt <= 0.1 * SC.VS and ang <= 0.1 * SC.VS / (2 * SC.ROOM_HALF), (dt, ang)
    assert dt < 1e-6 and ang < 1e-6, (dt, ang)
