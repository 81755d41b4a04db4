"""Independent float64 model of the pose alignment (SEMANTICS.md "Pose alignment"; nvbx_align_points / nvbx_align_depth /
nvbx_linearize_points).  numpy only; shares no code with the library.  The point transform is restated in float32 (it decides which
voxels are corners), everything behind the TSDF interpolant is float64.

Two drivers over one Gauss-Newton loop (`run`), which differ in where (d, g, valid) at the transformed points come from:
  hybrid_query(mapper, ...)   Mapper.query_tsdf -- the library's own f32 interpolant: isolates the sums, the solve and the pose update
  full_query(get_blocks, ...) query_independent.query over get_blocks -- nothing of the library's arithmetic is left
"""
import numpy as np

import query_independent as Q

CONVERGED, MAX_ITERATIONS, TOO_FEW, DEGENERATE, LINEARIZED = 1, 2, 3, 4, 5
DEFAULTS = dict(max_iterations=10, subsampling=4, min_weight=1e-4, huber_delta_m=0.0, damping=0.0, min_pivot_ratio=1e-9,
                stop_translation_m=1e-5, stop_rotation_rad=1e-5, min_valid=50, max_depth_m=0.0)
SERIES_BELOW = 1e-8


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def apply_rt_f32(R, t, x):
    """p = ((R0 x + R1 y) + R2 z) + t per row in IEEE float32, no contraction: nvbx_transform_pointcloud's expression"""
    R = np.asarray(R, np.float32); t = np.asarray(t, np.float32); x = np.asarray(x, np.float32).reshape(-1, 3)
    out = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            s = R[i, 0] * x[:, 0]
            s = s + R[i, 1] * x[:, 1]
            s = s + R[i, 2] * x[:, 2]
            out[:, i] = s + t[i]
    return out


def backproject(depth, cam, subsampling=1, max_depth_m=0.0):
    """the pixels (r s, c s) with 0 < depth <= max_depth_m as camera-frame points, row-major pixel order, float32 arithmetic of
    nvbx_backproject_depth: ((c + 0.5) - cu) / fu * d"""
    fu, fv, cu, cv = (np.float32(v) for v in cam[:4])
    d = np.asarray(depth, np.float32)[::subsampling, ::subsampling]
    r = (np.arange(d.shape[0]) * subsampling).astype(np.float32); c = (np.arange(d.shape[1]) * subsampling).astype(np.float32)
    rx = ((c + np.float32(0.5)) - cu) / fu; ry = ((r + np.float32(0.5)) - cv) / fv
    with np.errstate(invalid="ignore"):
        take = (d > 0) & ~((max_depth_m > 0) & (d > np.float32(max_depth_m)))
    pts = np.stack([d * rx[None, :], d * ry[:, None], d], -1).astype(np.float32)
    return pts[take]


def terms(p, t_f32, d, g, valid, huber_delta_m=0.0):
    """the 29 per-point products of the valid points, float64: -> (hh [m, 6, 6] = (w J) J^T, bb [m, 6] = (w J) r, cc [m] = (w r) r)"""
    v = np.asarray(valid, bool)
    r = np.asarray(d, np.float64)[v]; gd = np.asarray(g, np.float64)[v]
    q = np.asarray(p, np.float32)[v].astype(np.float64) - np.asarray(t_f32, np.float32).astype(np.float64)
    J = np.concatenate([gd, np.stack([q[:, 1] * gd[:, 2] - q[:, 2] * gd[:, 1], q[:, 2] * gd[:, 0] - q[:, 0] * gd[:, 2],
                                      q[:, 0] * gd[:, 1] - q[:, 1] * gd[:, 0]], 1)], 1)
    ar = np.abs(r)
    delta = float(np.float32(huber_delta_m))
    w = np.ones_like(r)
    if delta > 0:
        far = ar > delta
        w[far] = delta / ar[far]
    wJ = w[:, None] * J
    return wJ[:, :, None] * J[:, None, :], wJ * r[:, None], (w * r) * r


def sums(p, t_f32, d, g, valid, huber_delta_m=0.0):
    """-> (H [6, 6], b [6], cost, n_valid) and the sums of the terms' magnitudes (for summation-order bounds)"""
    hh, bb, cc = terms(p, t_f32, d, g, valid, huber_delta_m)
    mag = (np.abs(hh).sum(0), np.abs(bb).sum(0), float(np.abs(cc).sum()))
    return hh.sum(0), bb.sum(0), float(cc.sum()), int(len(cc)), mag


def solve(H, b, damping=0.0, min_pivot_ratio=1e-9):
    """(H + damping diag(H)) xi = -b by Cholesky; -> (xi | None, smallest pivot met / max diag(H))"""
    H = np.asarray(H, np.float64); dmax = float(np.max(np.diag(H))) if H.size else 0.0
    A = H + damping * np.diag(np.diag(H))
    L = np.zeros((6, 6)); worst = np.inf
    for k in range(6):
        piv = A[k, k] - float(L[k, :k] @ L[k, :k])
        ratio = piv / dmax if dmax > 0 else 0.0
        if not (piv > min_pivot_ratio * dmax) or not (piv > 0):
            return None, ratio
        worst = min(worst, ratio)
        L[k, k] = np.sqrt(piv)
        for i in range(k + 1, 6):
            L[i, k] = (A[i, k] - float(L[i, :k] @ L[k, :k])) / L[k, k]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-b[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - float(L[i + 1:, i] @ x[i + 1:])) / L[i, i]
    return x, worst


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    """-> (R, V): R = I + A K + B K^2, V = I + B K + C K^2 (closed forms; the series below SERIES_BELOW)"""
    w = np.asarray(w, np.float64); t2 = float(w @ w); th = np.sqrt(t2)
    if th < SERIES_BELOW:
        A, B, Cc = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    else:
        A, B, Cc = np.sin(th) / th, 2.0 * np.sin(th / 2) ** 2 / t2, (th - np.sin(th)) / (t2 * th)
    K = hat(w); K2 = np.outer(w, w) - t2 * np.eye(3)
    return np.eye(3) + A * K + B * K2, np.eye(3) + B * K + Cc * K2


def exp_so3_series(w, n_terms=60):
    """R = sum K^n / n!, V = sum K^n / (n + 1)!: the definition, term by term"""
    K = hat(np.asarray(w, np.float64))
    R = np.zeros((3, 3)); V = np.zeros((3, 3)); P = np.eye(3); f = 1.0
    for n in range(n_terms):
        R = R + P / f
        f_next = f * (n + 1)
        V = V + P / f_next
        P = P @ K; f = f_next
    return R, V


def apply_step(T, xi):
    R, V = exp_so3(xi[3:])
    out = np.eye(4)
    out[:3, :3] = R @ T[:3, :3]; out[:3, 3] = T[:3, 3] + V @ xi[:3]
    return out


def perturb(T, rng, translation_m=0.03, rotation_deg=1.5):
    """a start `translation_m` and `rotation_deg` off T in drawn directions, as float32 (what a caller hands over)"""
    dt = rng.normal(size=3); dt *= translation_m / np.linalg.norm(dt)
    ax = rng.normal(size=3); ax *= np.deg2rad(rotation_deg) / np.linalg.norm(ax)
    out = np.asarray(T, np.float64).copy()
    out[:3, :3] = exp_so3(ax)[0] @ out[:3, :3]; out[:3, 3] += dt
    return out.astype(np.float32)


def pose_distance(Ta, Tb):
    """-> (translation difference in metres, rotation angle in radians, largest rotation-entry difference)"""
    Ta = np.asarray(Ta, np.float64); Tb = np.asarray(Tb, np.float64)
    dR = Ta[:3, :3] @ Tb[:3, :3].T
    # (from the antisymmetric part: a pose handed over in float32 is orthonormal to 1e-7 only, which the trace alone would read as 4e-4 rad)
    sk = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    ang = float(np.arctan2(np.linalg.norm(sk), (np.trace(dR) - 1.0) / 2.0))
    return float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])), ang, float(np.abs(Ta[:3, :3] - Tb[:3, :3]).max())


def hybrid_query(mapper, min_weight):
    import torch

    def q(p):
        d, g, v = mapper.query_tsdf(torch.from_numpy(np.ascontiguousarray(p)).cuda(), min_weight=min_weight, unknown_value=0.0)
        return d.cpu().numpy(), g.cpu().numpy(), v.cpu().numpy().astype(bool)
    return q


def full_query(get_blocks, voxel_size, min_weight):
    def q(p):
        return Q.query(get_blocks, Q.LAYER_TSDF, p, voxel_size, min_weight=min_weight, unknown_value=0.0)
    return q


def run(query, x, T_guess, opts=None, linearize_only=False):
    """The refinement loop.  query(p float32 [n, 3]) -> (d, g, valid).  -> dict(T [4, 4] f64, iterations, status, n_valid, first, last, step,
    poses: the pose after every iteration)."""
    o = options(**(opts or {}))
    T = np.asarray(T_guess, np.float32).astype(np.float64).reshape(4, 4).copy()
    T[3] = [0, 0, 0, 1]
    x = np.asarray(x, np.float32).reshape(-1, 3)
    res = dict(first=None, last=None, step=np.zeros(6), poses=[], status=0, iterations=0)
    for it in range(1 if linearize_only else o["max_iterations"]):
        Tf = T.astype(np.float32)
        p = apply_rt_f32(Tf[:3, :3], Tf[:3, 3], x)
        d, g, valid = query(p) if len(x) else (np.zeros(0), np.zeros((0, 3)), np.zeros(0, bool))
        H, b, cost, nv, _ = sums(p, Tf[:3, 3], d, g, valid, o["huber_delta_m"])
        cur = dict(H=H, b=b, cost=cost, n_valid=nv)
        res["last"] = cur
        if it == 0:
            res["first"] = cur
        res["iterations"] = it + 1
        res["step"] = np.zeros(6)
        if nv < o["min_valid"]:
            res["status"] = TOO_FEW
        else:
            xi, _ = solve(H, b, o["damping"], o["min_pivot_ratio"])
            if xi is None:
                res["status"] = DEGENERATE
            elif linearize_only:
                res["status"] = LINEARIZED; res["step"] = xi
            else:
                res["step"] = xi
                T = apply_step(T, xi)
                if np.linalg.norm(xi[:3]) <= o["stop_translation_m"] and np.linalg.norm(xi[3:]) <= o["stop_rotation_rad"]:
                    res["status"] = CONVERGED
                elif it + 1 >= o["max_iterations"]:
                    res["status"] = MAX_ITERATIONS
        res["poses"].append(T.copy())
        if res["status"]:
            break
    res["T"] = T; res["n_valid"] = res["last"]["n_valid"]
    return res


# ---- the room the tests align against: a 160 x 120 camera, ten frames of the circle trajectory
SMALL_CAM = (80.0, 80.0, 79.5, 59.5, 160, 120)
MAP_FRAMES = tuple(range(0, 40, 4))
ALIGN_FRAMES = (10, 22, 34)


def room_frame(i):
    """-> (depth, rgb, true pose) of trajectory frame i through SMALL_CAM"""
    from isaac_ros_nvblox_amd import synthetic as S
    T = S.trajectory_pose(i)
    d, rgb = S.render(S.Scene(), T, SMALL_CAM)
    return d, rgb, T


def starts(frame, T_true, n=3, seed=1):
    rng = np.random.default_rng([seed, frame])
    return [perturb(T_true, rng) for _ in range(n)]
