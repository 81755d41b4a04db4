"""Independent float64 model of the colour point query and of the pose alignment with a colour term (SEMANTICS.md "Colour alignment and colour
queries"; nvbx_query_colors, nvbx_align_points_color / nvbx_align_depth_color / nvbx_linearize_points_color).  numpy only; shares no code with
the library.  The geometric half, the solve and the pose update are align_independent's; this file adds the colour interpolant over get_blocks,
the colour terms, the joint loop (`run`) in two drivers, and the drawn wall the tests align against.

  hybrid drivers   Mapper.query_tsdf + Mapper.query_color -- the library's own f32 interpolants: isolates the sums, the solve and the pose update
  full drivers     query_independent.query + color_query over get_blocks -- nothing of the library's arithmetic is left
"""
import numpy as np

import align_independent as A

LAYER_TSDF, LAYER_COLOR = 1, 2
VOX_LIMIT = 1 << 23
COLOR_DEFAULTS = dict(color_weight=1.0, min_color_weight=1e-4, color_huber_levels=0.0)
TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
COLOR_DT = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("pad", "u1"), ("weight", "<f4")])


def color_options(**kw):
    o = dict(COLOR_DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def luminance(rgb):
    """(77 r + 150 g + 29 b) / 256 of u8 triples [..., 3] -> float64 (exact)"""
    c = np.asarray(rgb).astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]).astype(np.float64) / 256.0


def _lattice(points, voxel_size):
    """the TSDF query's lattice per axis in IEEE f32: u = p / vs - 0.5, b = floor(u), t = u - b -> (b int64, t float64, ok)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        u = p / np.float32(voxel_size) - np.float32(0.5)
        f = np.floor(u)
        ok = (f >= -VOX_LIMIT) & (f <= VOX_LIMIT - 2)
        t = np.where(ok, u - f, 0.0).astype(np.float64)
    return np.where(ok, f, 0.0).astype(np.int64), t, ok


def _trilinear(c, t, vs):
    """c [n, 2, 2, 2] (i, j, k), t [n, 3] -> (value [n], gradient per metre [n, 3])"""
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    wx = np.stack([1 - tx, tx], 1); wy = np.stack([1 - ty, ty], 1); wz = np.stack([1 - tz, tz], 1)
    v = np.einsum("ni,nj,nk,nijk->n", wx, wy, wz, c)
    gx = np.einsum("nj,nk,njk->n", wy, wz, c[:, 1] - c[:, 0]) / vs
    gy = np.einsum("ni,nk,nik->n", wx, wz, c[:, :, 1] - c[:, :, 0]) / vs
    gz = np.einsum("ni,nj,nij->n", wx, wy, c[:, :, :, 1] - c[:, :, :, 0]) / vs
    return v, np.stack([gx, gy, gz], 1)


def color_query(get_blocks, points, voxel_size, min_color_weight=1e-4):
    """-> (rgb [n, 3], Y [n], gY [n, 3], valid [n]) in float64: the eight corners of the TSDF query's lattice must lie in blocks that carry the
    colour layer, with colour weight >= min_color_weight; zeros at an invalid point"""
    b, t, ok = _lattice(points, voxel_size)
    n = len(b)
    okp = ok.all(axis=1)
    idx = np.nonzero(okp)[0]
    ch = np.zeros((4, n, 2, 2, 2)); valid = okp.copy()
    corners = [(i, j, k) for k in (0, 1) for j in (0, 1) for i in (0, 1)]
    if len(idx):
        m = len(idx)
        vox = np.concatenate([b[idx] + np.array(o) for o in corners])
        keys, inv = np.unique(vox >> 3, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        blocks, found = get_blocks(LAYER_COLOR, keys.astype(np.int32))
        loc = vox & 7
        v = blocks[inv, loc[:, 2] + 8 * loc[:, 1] + 64 * loc[:, 0]]
        good = (np.asarray(found)[inv] != 0) & (v["weight"] >= np.float32(min_color_weight))
        rgb = np.stack([v["r"], v["g"], v["b"]], -1)
        vals = (luminance(rgb), rgb[:, 0].astype(np.float64), rgb[:, 1].astype(np.float64), rgb[:, 2].astype(np.float64))
        for q, (i, j, k) in enumerate(corners):
            for c in range(4):
                ch[c][idx, i, j, k] = vals[c][q * m:(q + 1) * m]
            valid[idx] &= good[q * m:(q + 1) * m]
    vs = float(np.float32(voxel_size))
    Y, gY = _trilinear(ch[0], t, vs)
    rgb = np.stack([_trilinear(ch[c], t, vs)[0] for c in (1, 2, 3)], 1)
    return np.where(valid[:, None], rgb, 0.0), np.where(valid, Y, 0.0), np.where(valid[:, None], gY, 0.0), valid


def color_terms(p, t_f32, Y, gY, Ys, both, voxel_size, color_weight=1.0, color_huber_levels=0.0):
    """the per-point colour products over the points `both` (geometric term valid and colour valid), float64, in the order the semantics state:
    -> (hh [m, 6, 6] = (lambda w_c J_c) J_c^T, bb [m, 6] = (lambda w_c J_c) r_c, cc [m] = (w_c e) e)"""
    v = np.asarray(both, bool)
    kappa = float(np.float32(voxel_size)) / 255.0
    e = np.asarray(Y, np.float64)[v] - np.asarray(Ys, np.float64)[v]
    gy = np.asarray(gY, np.float64)[v]
    q = np.asarray(p, np.float32)[v].astype(np.float64) - np.asarray(t_f32, np.float32).astype(np.float64)
    Jr = np.concatenate([gy, np.stack([q[:, 1] * gy[:, 2] - q[:, 2] * gy[:, 1], q[:, 2] * gy[:, 0] - q[:, 0] * gy[:, 2],
                                       q[:, 0] * gy[:, 1] - q[:, 1] * gy[:, 0]], 1)], 1)
    ae = np.abs(e)
    h = float(np.float32(color_huber_levels))
    wc = np.ones_like(e)
    if h > 0:
        far = ae > h
        wc[far] = h / ae[far]
    rc = kappa * e
    lw = float(np.float32(color_weight)) * wc
    Jc = kappa * Jr
    wJ = lw[:, None] * Jc
    return wJ[:, :, None] * Jc[:, None, :], wJ * rc[:, None], (wc * e) * e


def joint_sums(p, t_f32, d, g, valid, Y, gY, Ys, cvalid, voxel_size, huber_delta_m=0.0, color_weight=1.0, color_huber_levels=0.0):
    """-> dict(H, b, cost, n_valid, color_cost, n_color) of the joint system and mag = the sums of the terms' magnitudes (H, b, cost, color_cost)"""
    hh, bb, cc = A.terms(p, t_f32, d, g, valid, huber_delta_m)
    both = np.asarray(valid, bool) & np.asarray(cvalid, bool)
    ch, cb, ccc = color_terms(p, t_f32, Y, gY, Ys, both, voxel_size, color_weight, color_huber_levels)
    mag = (np.abs(hh).sum(0) + np.abs(ch).sum(0), np.abs(bb).sum(0) + np.abs(cb).sum(0), float(np.abs(cc).sum()), float(np.abs(ccc).sum()))
    return dict(H=hh.sum(0) + ch.sum(0), b=bb.sum(0) + cb.sum(0), cost=float(cc.sum()), n_valid=int(len(cc)), color_cost=float(ccc.sum()),
                n_color=int(len(ccc))), mag


def hybrid_color_query(mapper, min_color_weight):
    import torch

    def q(p):
        _, y, g, v = mapper.query_color(torch.from_numpy(np.ascontiguousarray(p)).cuda(), min_color_weight=min_color_weight, rgb=False)
        return y.cpu().numpy(), g.cpu().numpy(), v.cpu().numpy().astype(bool)
    return q


def full_color_query(get_blocks, voxel_size, min_color_weight):
    def q(p):
        return color_query(get_blocks, p, voxel_size, min_color_weight)[1:]
    return q


def run(query, cquery, x, rgb, T_guess, voxel_size, opts=None, copts=None, linearize_only=False):
    """The refinement loop over the joint system.  query(p) -> (d, g, valid); cquery(p) -> (Y, gY, valid); cquery None: the geometric term alone.
    x [n, 3] sensor-frame points, rgb [n, 3] u8 their colours.  -> align_independent.run's dict plus n_color and, in first / last, color_cost, n_color."""
    o = A.options(**(opts or {})); co = color_options(**(copts or {}))
    T = np.asarray(T_guess, np.float32).astype(np.float64).reshape(4, 4).copy()
    T[3] = [0, 0, 0, 1]
    x = np.asarray(x, np.float32).reshape(-1, 3)
    Ys = luminance(np.asarray(rgb, np.uint8).reshape(-1, 3))
    n = len(x)
    res = dict(first=None, last=None, step=np.zeros(6), poses=[], status=0, iterations=0)
    for it in range(1 if linearize_only else o["max_iterations"]):
        Tf = T.astype(np.float32)
        p = A.apply_rt_f32(Tf[:3, :3], Tf[:3, 3], x)
        d, g, valid = query(p) if n else (np.zeros(0), np.zeros((0, 3)), np.zeros(0, bool))
        Y, gY, cvalid = cquery(p) if (n and cquery is not None) else (np.zeros(n), np.zeros((n, 3)), np.zeros(n, bool))
        cur, _ = joint_sums(p, Tf[:3, 3], d, g, valid, Y, gY, Ys, cvalid, voxel_size, o["huber_delta_m"], co["color_weight"], co["color_huber_levels"])
        res["last"] = cur
        if it == 0:
            res["first"] = cur
        res["iterations"] = it + 1
        res["step"] = np.zeros(6)
        if cur["n_valid"] < o["min_valid"]:
            res["status"] = A.TOO_FEW
        else:
            xi, _ = A.solve(cur["H"], cur["b"], o["damping"], o["min_pivot_ratio"])
            if xi is None:
                res["status"] = A.DEGENERATE
            elif linearize_only:
                res["status"] = A.LINEARIZED; res["step"] = xi
            else:
                res["step"] = xi
                T = A.apply_step(T, xi)
                if np.linalg.norm(xi[:3]) <= o["stop_translation_m"] and np.linalg.norm(xi[3:]) <= o["stop_rotation_rad"]:
                    res["status"] = A.CONVERGED
                elif it + 1 >= o["max_iterations"]:
                    res["status"] = A.MAX_ITERATIONS
        res["poses"].append(T.copy())
        if res["status"]:
            break
    res["T"] = T; res["n_valid"] = res["last"]["n_valid"]; res["n_color"] = res["last"]["n_color"]
    return res


# ---- the drawn wall: a flat textured plane z = 0, on which the geometric system is exactly singular (three of its six directions slide)
WALL_VS = 0.05
WALL_TRUE_POSITION = (0.05, -0.03, 1.5)
WALL_DEPTH = 1.5
WALL_SUBSAMPLING = 4


def wall_pattern(x, y):
    """the wall's grey level at (x, y) metres"""
    return np.round(128.0 + 60.0 * np.sin(2.0 * np.pi * x / 0.8) + 40.0 * np.sin(2.0 * np.pi * y / 0.6 + 0.7))


def wall_blocks(grey=False):
    """-> (indices int32 [200, 3], tsdf [200, 512] TSDF_DT, color [200, 512] COLOR_DT): blocks over x, y in [-2, 2) m, z in [-0.4, 0.4) m at
    voxel size 0.05; TSDF clamp(z_centre, +-0.2) with weight 1; colour voxels of weight 1 with r = g = b = the pattern at the voxel centre
    (grey: 128 everywhere).  Voxel order z + 8 y + 64 x."""
    idx = np.array([(bx, by, bz) for bx in range(-5, 5) for by in range(-5, 5) for bz in (-1, 0)], np.int32)
    lx, ly, lz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")          # [x][y][z] -> linear z + 8 y + 64 x
    tsdf = np.zeros((len(idx), 512), TSDF_DT); color = np.zeros((len(idx), 512), COLOR_DT)
    for k, (bx, by, bz) in enumerate(idx):
        cx = ((8 * bx + lx) + 0.5) * WALL_VS; cy = ((8 * by + ly) + 0.5) * WALL_VS; cz = ((8 * bz + lz) + 0.5) * WALL_VS
        tsdf[k]["distance"] = np.clip(cz, -0.2, 0.2).astype(np.float32).reshape(-1)
        tsdf[k]["weight"] = 1.0
        level = (np.full(cx.shape, 128.0) if grey else wall_pattern(cx, cy)).astype(np.uint8).reshape(-1)
        for ch in ("r", "g", "b"):
            color[k][ch] = level
        color[k]["weight"] = 1.0
    return idx, tsdf, color


class DrawnMap:
    """get_blocks over drawn blocks held in numpy: what Mapper.get_blocks answers after set_blocks of the same data"""

    def __init__(self, indices, layers):
        self.at = {tuple(int(c) for c in i): k for k, i in enumerate(indices)}
        self.layers = layers          # {layer: [n, 512] records}

    def get_blocks(self, layer, indices):
        data = self.layers[layer]
        idx = np.asarray(indices, np.int32).reshape(-1, 3)
        out = np.zeros((len(idx), 512), data.dtype); found = np.zeros(len(idx), bool)
        for j, i in enumerate(idx):
            k = self.at.get(tuple(int(c) for c in i))
            if k is not None:
                out[j] = data[k]; found[j] = True
        return out, found


def wall_map(grey=False):
    idx, tsdf, color = wall_blocks(grey)
    return DrawnMap(idx, {LAYER_TSDF: tsdf, LAYER_COLOR: color})


def wall_pose():
    """the camera 1.5 m in front of the wall, looking straight at it: camera x = wall x, camera y = -wall y, camera z = -wall z"""
    T = np.eye(4)
    T[:3, :3] = np.diag([1.0, -1.0, -1.0]); T[:3, 3] = WALL_TRUE_POSITION
    return T


def wall_frame(grey=False):
    """-> (depth [120, 160] f32 = 1.5, rgb [120, 160, 3] u8: the pattern at each pixel's true wall point, true pose) through SMALL_CAM"""
    fu, fv, cu, cv, w, h = A.SMALL_CAM
    T = wall_pose()
    depth = np.full((h, w), WALL_DEPTH, np.float32)
    c = np.arange(w, dtype=np.float64)[None, :]; r = np.arange(h, dtype=np.float64)[:, None]
    xw = T[0, 3] + WALL_DEPTH * ((c + 0.5 - cu) / fu) + 0.0 * r
    yw = T[1, 3] - WALL_DEPTH * ((r + 0.5 - cv) / fv) + 0.0 * c
    level = (np.full(xw.shape, 128.0) if grey else wall_pattern(xw, yw)).astype(np.uint8)
    return depth, np.repeat(level[:, :, None], 3, axis=2), T


def wall_cloud(grey=False):
    """the frame's 1 200 points (pixels (4 r, 4 c)) with their colours and the true pose"""
    depth, rgb, T = wall_frame(grey)
    x = A.backproject(depth, A.SMALL_CAM, subsampling=WALL_SUBSAMPLING)
    return x, np.ascontiguousarray(rgb[::WALL_SUBSAMPLING, ::WALL_SUBSAMPLING].reshape(-1, 3)), T


def _start(T_true, dt, axis=None, deg=0.0):
    out = np.asarray(T_true, np.float64).copy()
    if axis is not None:
        ax = np.asarray(axis, np.float64); ax = ax * (np.deg2rad(deg) / np.linalg.norm(ax))
        out[:3, :3] = A.exp_so3(ax)[0] @ out[:3, :3]
    out[:3, 3] += np.asarray(dt, np.float64)
    return out.astype(np.float32)


def wall_starts(T_true=None):
    T = wall_pose() if T_true is None else T_true
    return [_start(T, (0.03, -0.02, 0.01), (0, 0, 1), 1.0), _start(T, (-0.04, 0.03, -0.02), (1, 1, 1), 1.5), _start(T, (0.05, 0.05, 0.0)),
            _start(T, (0.08, 0.0, 0.0)), _start(T, (0.12, 0.0, 0.0))]
