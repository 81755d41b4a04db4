"""Independent numpy model of relocalisation (SEMANTICS.md "Relocalisation"; nvbx_score_poses_* / nvbx_search_lattice_poses /
nvbx_relocalize_*).  numpy only; shares no code with the library.  The pose application is restated in float32 (it decides which voxels
are corners), the classification compares float32 numbers, the sums are Python integers, the lattice tables are float64 rounded once.

As in align_independent the TSDF interpolant at the transformed points comes from one of two drivers:
  hybrid_query(mapper, ...)   Mapper.query_tsdf -- the library's own f32 interpolant: records must then agree with the GPU's bit for bit
  full_query(get_blocks, ...) query_independent.query over get_blocks, rounded to float32 -- nothing of the library's arithmetic is left
"""
import collections

import numpy as np

import query_independent as Q

OK, NO_CANDIDATE = 0, 1
SCORE_DEFAULTS = dict(min_weight=0.0, inlier_distance_m=0.0, conflict_distance_m=0.0, max_depth_m=0.0, subsampling=4)
MIN_INLIERS = 50
MAX_STEPS, MAX_POSES = 64, 1 << 20
Score = collections.namedtuple("Score", "points valid inliers conflicts abs_residual_q20")
INVALID = Score(-1, 0, 0, 0, 0)
F = np.float32


def thresholds(voxel_size, truncation_vox, **kw):
    """-> (min_weight, inlier_distance_m, conflict_distance_m) as float32: an option <= 0 selects one voxel size / half the truncation
    distance (f32 products) / 1e-4"""
    o = dict(SCORE_DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    vs = F(voxel_size)
    mw = F(o["min_weight"]) if F(o["min_weight"]) > 0 else F(1e-4)
    inl = F(o["inlier_distance_m"]) if F(o["inlier_distance_m"]) > 0 else vs
    con = F(o["conflict_distance_m"]) if F(o["conflict_distance_m"]) > 0 else F(0.5) * (F(truncation_vox) * vs)
    return mw, inl, con


def pose_in_range(T, voxel_size):
    """finite, and |t| below ((2^20 - 2) blocks) per axis, in float32"""
    T = np.asarray(T, F).reshape(4, 4)
    lim = (F(1 << 20) - F(2.0)) * (F(voxel_size) * F(8.0))
    return bool(np.isfinite(T).all() and (np.abs(T[:3, 3]) < lim).all())


def transform_f32(T, x):
    """p = ((R0 x + R1 y) + R2 z) + t per row, IEEE float32, products and sums rounded one by one"""
    T = np.asarray(T, F).reshape(4, 4); x = np.asarray(x, F).reshape(-1, 3)
    out = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            s = T[i, 0] * x[:, 0]
            s = s + T[i, 1] * x[:, 1]
            s = s + T[i, 2] * x[:, 2]
            out[:, i] = s + T[i, 3]
    return out


def taken_pixels(depth, cam, subsampling=1, max_depth_m=0.0):
    """the pixels (r s, c s) with 0 < depth <= max_depth_m as camera-frame points, row-major: ((c + 0.5) - cu) / fu * d in float32"""
    fu, fv, cu, cv = (F(v) for v in cam[:4])
    d = np.asarray(depth, F)[::subsampling, ::subsampling]
    rows = (np.arange(d.shape[0]) * subsampling).astype(F); cols = (np.arange(d.shape[1]) * subsampling).astype(F)
    rx = ((cols + F(0.5)) - cu) / fu; ry = ((rows + F(0.5)) - cv) / fv
    with np.errstate(invalid="ignore"):
        take = d > 0
        if max_depth_m > 0:
            take &= ~(d > F(max_depth_m))
    pts = np.stack([d * rx[None, :], d * ry[:, None], d], -1).astype(F)
    return pts[take]


def classify(d, valid, inlier, conflict):
    """one pose's record from the interpolant at its transformed points"""
    d = np.asarray(d, F); v = np.asarray(valid, bool)
    ad = np.abs(d[v])
    q = np.rint(ad * F(1048576.0))
    assert q.dtype == F
    return Score(len(d), int(v.sum()), int((ad <= F(inlier)).sum()), int((d[v] > F(conflict)).sum()), int(q.astype(np.int64).sum()))


def score_poses(query, x, poses, voxel_size, truncation_vox, **options):
    """-> one Score per pose.  query(p float32 [m, 3]) -> (d, g, valid); every pose's points go through ONE query call"""
    mw, inl, con = thresholds(voxel_size, truncation_vox, **options)
    x = np.asarray(x, F).reshape(-1, 3)
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    good = [k for k in range(len(poses)) if pose_in_range(poses[k], voxel_size)]
    out = [INVALID] * len(poses)
    if good and len(x):
        p = np.concatenate([transform_f32(poses[k], x) for k in good])
        d, _, valid = query(p)
        d = np.asarray(d).astype(F)
        for j, k in enumerate(good):
            out[k] = classify(d[j * len(x):(j + 1) * len(x)], valid[j * len(x):(j + 1) * len(x)], inl, con)
    else:
        for k in good:
            out[k] = Score(0, 0, 0, 0, 0)
    return out


def records(scores):
    """-> (counts int32 [K, 4], abs_residual_q20 int64 [K]): the layout Mapper.score_poses returns"""
    return (np.array([s[:4] for s in scores], np.int32).reshape(-1, 4), np.array([s[4] for s in scores], np.int64))


# ---- the lattice
def lattice_ok(half_extent_m, half_yaw_rad, steps):
    steps = [int(s) for s in steps]
    if len(steps) != 4 or any(s < 1 or s > MAX_STEPS for s in steps) or int(np.prod(steps)) > MAX_POSES:
        return False
    h = list(np.broadcast_to(np.asarray(half_extent_m, F), (3,))) + [F(half_yaw_rad)]
    return all(np.isfinite(v) and v >= 0 for v in h)


def offsets(half, s):
    """float64: 0 for one step, else -half + (2 half i) / (s - 1), half = the float32 the caller hands over"""
    h = float(F(half))
    if s == 1:
        return np.zeros(1)
    return np.array([-h + (2.0 * h * float(i)) / float(s - 1) for i in range(s)])


def lattice_tables(T0, half_extent_m, half_yaw_rad, steps):
    """-> (dx, dy, dz float32 offset tables, R float32 [nyaw, 3, 3] = Rz(yaw) R0: float64 products of R0's float32 entries, rounded once)"""
    T0 = np.asarray(T0, F).reshape(4, 4)
    he = np.broadcast_to(np.asarray(half_extent_m, F), (3,))
    off = [offsets(he[a], int(steps[a])).astype(F) for a in range(3)]
    R0 = T0[:3, :3].astype(np.float64)
    R = np.empty((int(steps[3]), 3, 3), F)
    for w, yaw in enumerate(offsets(half_yaw_rad, int(steps[3]))):
        c, s = np.cos(yaw), np.sin(yaw)
        R[w, 0] = (c * R0[0] - s * R0[1]).astype(F)
        R[w, 1] = (s * R0[0] + c * R0[1]).astype(F)
        R[w, 2] = R0[2].astype(F)
    return off[0], off[1], off[2], R


def lattice_index(steps, ix, iy, iz, iw):
    return ((ix * int(steps[1]) + iy) * int(steps[2]) + iz) * int(steps[3]) + iw


def lattice_unravel(steps, h):
    iw = h % int(steps[3]); h //= int(steps[3])
    iz = h % int(steps[2]); h //= int(steps[2])
    iy = h % int(steps[1]); h //= int(steps[1])
    return h, iy, iz, iw


def lattice_poses(T0, half_extent_m, half_yaw_rad, steps):
    """-> float32 [K, 4, 4], hypothesis h = ((ix ny + iy) nz + iz) nyaw + iw: t0 + (dx[ix], dy[iy], dz[iz]) in three float32 additions"""
    T0 = np.asarray(T0, F).reshape(4, 4)
    dx, dy, dz, R = lattice_tables(T0, half_extent_m, half_yaw_rad, steps)
    K = int(np.prod([int(s) for s in steps]))
    out = np.zeros((K, 4, 4), F)
    for h in range(K):
        ix, iy, iz, iw = lattice_unravel(steps, h)
        out[h, :3, :3] = R[iw]
        out[h, :3, 3] = T0[:3, 3] + np.array([dx[ix], dy[iy], dz[iz]], F)
        out[h, 3, 3] = 1.0
    return out


# ---- the selection
def select(scores, min_inliers=MIN_INLIERS):
    """-> (status, index): the record with the largest inliers - conflicts; ties: more inliers, then the lowest index"""
    best = None
    for h, s in enumerate(scores):
        cand = (s.inliers - s.conflicts, s.inliers, -h)
        if best is None or cand > best:
            best = cand
    h = -best[2]
    return (OK if scores[h].inliers >= min_inliers else NO_CANDIDATE), h


def winner_is_unique(scores):
    """no second record shares the winner's key and inlier count"""
    _, h = select(scores, 0)
    top = (scores[h].inliers - scores[h].conflicts, scores[h].inliers)
    return sum(1 for s in scores if (s.inliers - s.conflicts, s.inliers) == top) == 1


def hybrid_query(mapper, min_weight):
    import torch

    def q(p):
        d, g, v = mapper.query_tsdf(torch.from_numpy(np.ascontiguousarray(p)).cuda(), min_weight=float(min_weight), unknown_value=0.0)
        return d.cpu().numpy(), g.cpu().numpy(), v.cpu().numpy().astype(bool)
    return q


def full_query(get_blocks, voxel_size, min_weight):
    def q(p):
        return Q.query(get_blocks, Q.LAYER_TSDF, p, voxel_size, min_weight=float(min_weight), unknown_value=0.0)
    return q


# ---- the search the GPU tests and the model tests share: per alignment frame a lattice centred OFFSET_M / OFFSET_DEG off the truth
LATTICE = dict(half_extent_m=(0.4, 0.4, 0.0), half_yaw_rad=float(np.deg2rad(20.0)), steps=(5, 5, 1, 9))
OFFSET_M, OFFSET_DEG = 0.3, 15.0


def lattice_centre(T_true, frame):
    """T0: the truth moved OFFSET_M in the layer's x-y plane (a direction drawn per frame) and turned OFFSET_DEG about the layer's z through the
    sensor origin (sign drawn per frame), as float32"""
    rng = np.random.default_rng([7, frame])
    a = rng.uniform(0.0, 2.0 * np.pi); sign = rng.choice([-1.0, 1.0])
    yaw = sign * np.deg2rad(OFFSET_DEG)
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.asarray(T_true, np.float64).copy()
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ T[:3, :3]
    T[:3, 3] += OFFSET_M * np.array([np.cos(a), np.sin(a), 0.0])
    return T.astype(F)


def yaw_between(Ta, Tb):
    """the rotation about z that takes Tb's rotation to Ta's, radians (both differ by a rotation about z)"""
    dR = np.asarray(Ta, np.float64)[:3, :3] @ np.asarray(Tb, np.float64)[:3, :3].T
    return float(np.arctan2(dR[1, 0] - dR[0, 1], dR[0, 0] + dR[1, 1]))


def within_one_step(T_node, T_true, half_extent_m, half_yaw_rad, steps):
    """the node lies within one lattice step of the truth along every searched axis"""
    he = np.broadcast_to(np.asarray(half_extent_m, np.float64), (3,))
    dt = np.abs(np.asarray(T_node, np.float64)[:3, 3] - np.asarray(T_true, np.float64)[:3, 3])
    for a in range(3):
        step = 2.0 * he[a] / (int(steps[a]) - 1) if int(steps[a]) > 1 else None
        if step is not None and dt[a] > step + 1e-6:
            return False
    if int(steps[3]) > 1:
        return abs(yaw_between(T_node, T_true)) <= 2.0 * half_yaw_rad / (int(steps[3]) - 1) + 1e-6
    return True
