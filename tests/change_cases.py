"""Inputs of the change-detection tests (tests/test_change_model.py on the CPU, tests/test_gpu_change.py on the GPU): the analytic room before and
after its sphere was moved, seen in the same few 80 x 60 frames, the bound on where a labelled voxel may lie, and hand-made block sets drawn
with a fixed seed that reach every path of the sampling."""
import numpy as np

from isaac_ros_nvblox_amd import synthetic as S

import change_independent as CI
import merge_independent as MI

F32 = np.float32
CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
VS = 0.05
OLD_C, NEW_C, SPHERE_R = (1.5, 1.0, 0.6), (1.5, -1.0, 0.6), 0.5
# three eyes look at the old place; mirrored in y, at the new one.  They look down steeply (about 60 degrees): where a sphere hides the floor from
# some of them, the others must agree on it, and at a grazing angle one 80 x 60 pixel is a tenth of a metre of floor depth -- more than the gap
# between "free" and "occupied"
EYES = ((0.6, 0.2, 2.6), (1.0, 0.0, 2.8), (0.4, 0.8, 2.4))
# both room maps are fused with the nearest depth pixel: the default, bilinear interpolation of the depth image, blends the sphere's depth with the
# floor's along its silhouette and leaves wrong distances a metre behind it, on the floor -- changes of the fusion rule's making, not of the scene's
PARAMS = {"voxel_size": VS, "depth_interp_nearest": 1}
T_GENERAL =MI.pose([1.0, -2.0, 3.0], 11.0, [0.31, -0.17, 0.23])   # p_M = T p_R: the reference map lives in a frame of its own


def scenes():
    """(the reference scene, the scene now: the sphere moved from OLD_C to NEW_C)"""
    return S.Scene(), S.Scene(sphere_c=NEW_C)


def poses():
    out = []
    for c, sy in ((OLD_C, 1.0), (NEW_C, -1.0)):
        for e in EYES:
            eye = np.array([e[0], sy * e[1], e[2]])
            d = np.asarray(c) - eye
            out.append(S.look_pose(eye, np.arctan2(d[1], d[0]), np.arctan2(d[2], np.hypot(d[0], d[1]))))
    return out


def frames(scene):
    """[(depth, T_L_C)] of `scene` from poses()"""
    return [(S.render(scene, T, CAM, color=False)[0], T) for T in poses()]


def margin(truncation_m):
    """how far from the moved sphere's surface a labelled voxel may lie: the truncation distance (a voxel behind the surface is updated that
    far), sqrt(3) voxel sizes (a voxel centre against the point its ray hit) and one pixel footprint at the sphere's range (range / focal
    length: the silhouette is only that sharp), the range taken from the farthest eye"""
    rng = max(float(np.linalg.norm(np.asarray(OLD_C) - np.asarray(e))) for e in EYES)
    return float(truncation_m) + np.sqrt(3.0) * VS + rng / CAM[0]


def surface_distance(points, centre):
    """| |p - c| - r | of points [n, 3]"""
    return np.abs(np.linalg.norm(np.asarray(points, np.float64) - np.asarray(centre, np.float64), axis=1) - SPHERE_R)


def check_room(volume, truncation_m, what=""):
    """the analytic bound: every label-0 voxel lies within margin() of the new sphere's surface, every label-1 voxel of the old one's; both occur"""
    m = margin(truncation_m)
    for label, centre in ((CI.APPEARED, NEW_C), (CI.REMOVED, OLD_C)):
        p = CI.labelled_positions(volume, label, VS)
        assert len(p) > 0, (what, label)
        worst = float(surface_distance(p, centre).max())
        assert worst <= m, "%s: a voxel of label %d lies %.4f m from its sphere's surface, the margin is %.4f m" % (what, label, worst, m)


# ---------------------------------------------------------------------------------------------- hand-made blocks
def _draw(rng, n, dist=0.3):
    v = np.zeros((n, 512), CI.TSDF_DT)
    v["distance"] = rng.uniform(-dist, dist, (n, 512)).astype(F32)
    v["weight"] = rng.choice(np.array([0.5, 1.0, 3.0], F32), (n, 512))
    return v


def drawn_maps(seed, origin=(-1, -1, -1), free=VS, occupied=0.0, ref_min_weight=1e-4):
    """-> (m, ref): 2 x 2 x 2 blocks of m from `origin` (negative indices with the default) and a 4 x 4 x 4 cube of ref blocks around them with
    one block missing; distances drawn in +-0.3 m (an interpolant of eight of them still leaves both thresholds often), so both classes occur on both sides and samples cross block borders on every axis and on all
    three at once.  Planted: NaN distances on both sides, distances exactly equal to both thresholds on both sides, unobserved voxels in m,
    and one voxel of ref just below ref_min_weight."""
    rng = np.random.default_rng(seed)
    o = np.asarray(origin)
    mk = [tuple(int(q) for q in o + (x, y, z)) for x in range(2) for y in range(2) for z in range(2)]
    rk = [tuple(int(q) for q in o - 1 + (x, y, z)) for x in range(4) for y in range(4) for z in range(4)]
    rk.remove(tuple(int(q) for q in o + (1, 0, 1)))                          # one missing neighbour block inside the cube
    mv = _draw(rng, len(mk)); rv = _draw(rng, len(rk))
    for v in (mv, rv):
        v["distance"][:, 5::37] = F32(np.nan)
        v["distance"][:, 7::41] = F32(free)
        v["distance"][:, 11::43] = F32(occupied)
    mv["weight"][:, 3::29] = F32(0.0)
    below = np.nextafter(F32(ref_min_weight), F32(0.0))
    rv["weight"][:, 13::47] = below
    return dict(zip(mk, mv)), dict(zip(rk, rv))


def drawn_transforms():
    """the identity, a whole-block shift, a sub-voxel shift, a general rotation: (name, T_M_R)"""
    return (("identity", MI.pose([0, 0, 1], 0.0, [0, 0, 0])), ("block shift", MI.pose([0, 0, 1], 0.0, [8 * VS, -8 * VS, 0.0])),
            ("sub-voxel shift", MI.pose([0, 0, 1], 0.0, [0.017, -0.021, 0.009])), ("rotation", MI.pose([2.0, -1.0, 0.5], 23.0, [0.06, 0.11, -0.04])))
