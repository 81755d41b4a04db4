"""A numpy float32 restatement of the feature layer's per-voxel rule (SEMANTICS.md "Feature layer"), written from the rule's text.

It shares no code with the library and does not import the oracle.  Every product, sum and quotient below is one float32 operation in the order
SEMANTICS.md fixes (no fused multiply-add: numpy has none); np.float16(x) of a float32 rounds to nearest even.

State of the layer: dict {(bx, by, bz): (values float16 [512, C], weights float32 [512])}, voxel t = vx * 64 + vy * 8 + vz.  A block is in the dict
once a feature frame has reached one of its voxels.
"""
import numpy as np

F = np.float32


class Rules:
    """The mapper parameters the rule reads."""

    def __init__(self, voxel_size=0.05, max_integration_distance_m=8.0, max_weight=5.0, truncation_distance_vox=4.0,
                 occlusion_threshold_m=None, subsampling=4):
        self.vs = F(voxel_size)
        self.bs = F(self.vs * F(8.0))
        self.max_dist = F(max_integration_distance_m)
        self.max_weight = F(max_weight)
        self.trunc = F(F(truncation_distance_vox) * self.vs)
        self.occ = self.trunc if occlusion_threshold_m is None else F(occlusion_threshold_m)
        self.sub = int(subsampling)


def in_band(distance, weight, trunc):
    """A TSDF voxel of the truncation band: observed and closer to the surface than the truncation distance."""
    return (weight > F(1e-4)) & (np.abs(distance) < trunc)


def pose_inverse(T_L_C):
    """p_C = R p_L + t from the row-major camera-to-layer transform: R = rotation transposed, t = -(R t_LC), summed left to right."""
    T = np.asarray(T_L_C, F).reshape(4, 4)
    R = T[:3, :3].T.copy()
    t = np.empty(3, F)
    for i in range(3):
        s = F(R[i, 0] * T[0, 3])
        s = F(s + F(R[i, 1] * T[1, 3]))
        s = F(s + F(R[i, 2] * T[2, 3]))
        t[i] = -s
    return R, t


def to_camera(R, t, x, y, z):
    out = []
    for i in range(3):
        s = R[i, 0] * x
        s = s + R[i, 1] * y
        s = s + R[i, 2] * z
        out.append((s + t[i]).astype(F))
    return out


def block_in_frustum(R, t, cam, rules, b):
    """Six planes; the block is outside when all eight corners are outside one of them."""
    fu, fv, cu, cv, w, h = F(cam[0]), F(cam[1]), F(cam[2]), F(cam[3]), F(int(cam[4])), F(int(cam[5]))
    q = np.arange(8)
    x = (F(1) * (b[0] + (q & 1))).astype(F) * rules.bs
    y = (F(1) * (b[1] + ((q >> 1) & 1))).astype(F) * rules.bs
    z = (F(1) * (b[2] + ((q >> 2) & 1))).astype(F) * rules.bs
    px, py, pz = to_camera(R, t, x.astype(F), y.astype(F), z.astype(F))
    outside = [fu * px + cu * pz < 0, fu * px + (cu - w) * pz > 0, fv * py + cv * pz < 0, fv * py + (cv - h) * pz > 0, pz < 0,
               (pz > rules.max_dist) if rules.max_dist > 0 else np.zeros(8, bool)]
    return not any(o.all() for o in outside)


def feature_taps(u, v, stride, rows_f, cols_f):
    """Bilinear taps of the feature grid at full-resolution pixel coordinate (u, v): (ok, x0, y0, ax, ay)."""
    u = np.asarray(u, F); v = np.asarray(v, F)
    uf = (u / F(stride)).astype(F) - F(0.5); vf = (v / F(stride)).astype(F) - F(0.5)
    fx = np.floor(uf); fy = np.floor(vf)
    with np.errstate(invalid="ignore"):
        x0 = np.where(np.isfinite(fx), fx, -1).astype(np.int64); y0 = np.where(np.isfinite(fy), fy, -1).astype(np.int64)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= cols_f - 1) & (y0 + 1 <= rows_f - 1)
    return ok, x0, y0, (uf - fx).astype(F), (vf - fy).astype(F)


def bilinear(ax, ay, t00, t10, t01, t11):
    one = F(1)
    top = (one - ax) * t00 + ax * t10
    bot = (one - ax) * t01 + ax * t11
    return ((one - ay) * top + ay * bot).astype(F)


def blend(old_f16, w0, f, max_weight):
    """One observation of weight 1 joins a voxel: -> (values float16, weight float32)."""
    w0 = np.asarray(w0, F)
    tw = (w0 + F(1)).astype(F)
    a = (w0 / tw).astype(F); b = (F(1) / tw).astype(F)
    v = (np.asarray(old_f16, np.float16).astype(F) * a + np.asarray(f, F) * b).astype(F)
    with np.errstate(over="ignore"):
        return v.astype(np.float16), np.minimum(tw, F(max_weight)).astype(F)


def voxel_update_mask(rules, b, synth, T_L_C, cam, stride, rows_f, cols_f):
    """Per voxel of block b: (reached, x0, y0, ax, ay)."""
    R, t = pose_inverse(T_L_C)
    fu, fv, cu, cv, w, h = F(cam[0]), F(cam[1]), F(cam[2]), F(cam[3]), F(int(cam[4])), F(int(cam[5]))
    tt = np.arange(512)
    vx, vy, vz = tt >> 6, (tt >> 3) & 7, tt & 7
    half = rules.vs * F(0.5)
    cx = ((F(b[0]) * rules.bs + vx.astype(F) * rules.vs).astype(F) + half).astype(F)
    cy = ((F(b[1]) * rules.bs + vy.astype(F) * rules.vs).astype(F) + half).astype(F)
    cz = ((F(b[2]) * rules.bs + vz.astype(F) * rules.vs).astype(F) + half).astype(F)
    px, py, pz = to_camera(R, t, cx, cy, cz)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (fu * (px / pz).astype(F) + cu).astype(F)
        v = (fv * (py / pz).astype(F) + cv).astype(F)
        ok = (pz > 0) & (u >= 0) & (v >= 0) & (u <= w) & (v <= h)
        if rules.max_dist > 0:
            ok &= ~(pz > rules.max_dist)
        f_ok, x0, y0, ax, ay = feature_taps(u, v, stride, rows_f, cols_f)
        srows, scols = synth.shape
        us = (u / F(rules.sub)).astype(F) - F(0.5); vs_ = (v / F(rules.sub)).astype(F) - F(0.5)
        sfx = np.floor(us); sfy = np.floor(vs_)
        sx0 = np.where(np.isfinite(sfx), sfx, -1).astype(np.int64); sy0 = np.where(np.isfinite(sfy), sfy, -1).astype(np.int64)
    s_ok = (sx0 >= 0) & (sy0 >= 0) & (sx0 + 1 <= scols - 1) & (sy0 + 1 <= srows - 1)
    ok = ok & f_ok & s_ok
    sx = np.where(ok, sx0, 0); sy = np.where(ok, sy0, 0)
    s00, s10, s01, s11 = synth[sy, sx], synth[sy, sx + 1], synth[sy + 1, sx], synth[sy + 1, sx + 1]
    ok &= (s00 > 0) & (s10 > 0) & (s01 > 0) & (s11 > 0)
    sd = bilinear((us - sfx).astype(F), (vs_ - sfy).astype(F), s00, s10, s01, s11)
    with np.errstate(invalid="ignore"):
        ok &= ~(np.abs(sd - pz) > rules.occ)
    return ok, x0, y0, ax, ay


def integrate(state, rules, blocks, band, synth, T_L_C, cam, stride, feat):
    """One feature frame.  blocks [n, 3]: the TSDF block set; band [n]: the block has a voxel in the truncation band; synth: the synthetic depth
    image of the pose at the colour path's subsampling; feat [rows_f, cols_f, C] float16.  Updates `state` in place and returns it."""
    feat = np.asarray(feat, np.float16)
    synth = np.asarray(synth, F)
    rows_f, cols_f, C = feat.shape
    ff = feat.astype(F)
    R, t = pose_inverse(T_L_C)
    for b, bd in zip(np.asarray(blocks).reshape(-1, 3), band):
        if not bd:
            continue
        b = tuple(int(q) for q in b)
        if not block_in_frustum(R, t, cam, rules, b):
            continue
        ok, x0, y0, ax, ay = voxel_update_mask(rules, b, synth, T_L_C, cam, stride, rows_f, cols_f)
        if not ok.any():
            continue
        if b not in state:      # the first frame that reaches the block finds it empty
            state[b] = (np.zeros((512, C), np.float16), np.zeros(512, F))
        vals, wts = state[b]
        i = np.nonzero(ok)[0]
        xx, yy = x0[i], y0[i]
        f = bilinear(ax[i, None], ay[i, None], ff[yy, xx], ff[yy, xx + 1], ff[yy + 1, xx], ff[yy + 1, xx + 1])
        nv, nw = blend(vals[i], wts[i, None], f, rules.max_weight)
        vals[i] = nv; wts[i] = nw[:, 0]
    return state


def voxel_of(points, voxel_size):
    """float64 floor(p / vs): (block index [n, 3], voxel t [n])."""
    g = np.floor(np.asarray(points, np.float64) / float(voxel_size)).astype(np.int64)
    b = g >> 3; v = g & 7
    return b, v[:, 0] * 64 + v[:, 1] * 8 + v[:, 2]
