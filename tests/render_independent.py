"""Independent numpy float32 model of rendering and ray casts (SEMANTICS.md "Rendering and ray casts"; nvbx_render_view, nvbx_cast_rays).

The SERIAL march, one sample per step, restated from the semantics over a dict of blocks {(bx, by, bz): voxels[512]} as get_blocks hands them out
(host copies in the reference's voxel order z + 8y + 64x), plus the colour and normal look-ups at the hit point.  Every float operation is a numpy
float32 operation in the order the semantics state, so depth is expected to agree with an IEEE f32 implementation to the bit.  Imports neither the
product nor the oracle.
"""
import numpy as np

F = np.float32
OBSERVED_WEIGHT = F(1e-4)      # a TSDF voxel is observed when its weight is above this; the normal's corners need weight >= it
VOX_LIMIT = 1 << 23


def _keys(b):
    b = np.asarray(b, np.int64)
    return ((b[..., 0] + (1 << 20)) << 42) | ((b[..., 1] + (1 << 20)) << 21) | (b[..., 2] + (1 << 20))


class Volume:
    """blocks: dict {(bx, by, bz): structured array [512]} of one layer -> vectorised voxel look-up by global voxel index"""

    def __init__(self, blocks, fields):
        idx = np.array(sorted(blocks), np.int64).reshape(-1, 3)
        self.keys = _keys(idx) if len(idx) else np.zeros(0, np.int64)
        order = np.argsort(self.keys)
        self.keys = self.keys[order]
        self.data = {f: (np.stack([np.asarray(blocks[tuple(int(v) for v in idx[i])][f]) for i in order]) if len(idx)
                         else np.zeros((0, 512))) for f in fields}

    def lookup(self, vox):
        """vox int64 [n, 3] -> (found [n], {field: values [n]})"""
        vox = np.asarray(vox, np.int64)
        in_range = (np.abs(vox) < VOX_LIMIT).all(axis=-1)
        v = np.where(in_range[..., None], vox, 0)
        k = _keys(v >> 3)
        pos = np.searchsorted(self.keys, k)
        pos_c = np.minimum(pos, max(len(self.keys) - 1, 0))
        found = in_range & (len(self.keys) > 0) & (self.keys[pos_c] == k if len(self.keys) else False)
        loc = v & 7
        lin = loc[..., 2] + 8 * loc[..., 1] + 64 * loc[..., 0]
        out = {}
        for f, d in self.data.items():
            out[f] = np.where(found, d[pos_c, lin], 0) if len(self.keys) else np.zeros(vox.shape[:-1], d.dtype)
        return found, out


def _voxel_of(p, vs):
    """global voxel index floor(p / vs) per component in f32 (non-finite -> far out of range)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(p / F(vs))
    f = np.where(np.isfinite(f), f, F(3e9))
    return np.clip(f, -3e9, 3e9).astype(np.int64)


def cast(tsdf, origins, directions, voxel_size, trunc, eps_m, max_steps, max_len):
    """Serial sphere tracing of n rays: -> (t [n] f32, hit [n] bool).  Rules: sample the voxel that contains o + t d; unobserved (missing block or
    weight <= 1e-4): step `trunc` unless something positive has been seen, then give up; observed and distance < eps_m: a hit at t + distance if
    something positive has been seen, else give up; otherwise step by the distance.  At most max_steps samples, and only while t < max_len."""
    o = np.asarray(origins, F).reshape(-1, 3); d = np.asarray(directions, F).reshape(-1, 3)
    n = len(o)
    trunc, eps_m, max_len = F(trunc), F(eps_m), F(max_len)
    t = np.zeros(n, F); hit = np.zeros(n, bool); last_positive = np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        active = np.isfinite(d).all(axis=1) & np.isfinite(o).all(axis=1) & (d != 0).any(axis=1)
    for _ in range(int(max_steps)):
        active &= t < max_len
        a = np.nonzero(active)[0]
        if len(a) == 0:
            break
        ta = t[a]
        p = np.stack([o[a, k] + ta * d[a, k] for k in range(3)], axis=1)          # one multiply, one add per component, f32
        found, v = tsdf.lookup(_voxel_of(p, voxel_size))
        dist = v["distance"].astype(F); observed = found & (v["weight"].astype(F) > OBSERVED_WEIGHT)
        lp = last_positive[a]
        surface = observed & (dist < eps_m)
        stop = (~observed & lp) | surface
        is_hit = surface & lp
        step = np.where(observed, dist, trunc).astype(F)
        go = ~stop
        t[a[go]] = ta[go] + step[go]
        t[a[is_hit]] = ta[is_hit] + dist[is_hit]
        hit[a[is_hit]] = True
        last_positive[a] = lp | (observed & ~surface)
        active[a[stop]] = False
    return np.where(hit, t, F(0)).astype(F), hit


def view_rays(T_L_C, cam, subsampling):
    """rays of the rendered view: -> (origins [n, 3], directions [n, 3], dcz [n], (rows, cols)); ray (r, c) goes through the centre of
    full-resolution pixel (r s, c s)"""
    fu, fv, cu, cv, w, h = cam
    s = int(subsampling)
    rows, cols = int(h) // s, int(w) // s
    T = np.asarray(T_L_C, F).reshape(4, 4)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    rx = (((c * s).astype(F) + F(0.5)) - F(cu)) / F(fu)
    ry = (((r * s).astype(F) + F(0.5)) - F(cv)) / F(fv)
    nrm = np.sqrt((rx * rx + ry * ry) + F(1.0))
    dc = [rx / nrm, ry / nrm, F(1.0) / nrm]
    dl = []
    for i in range(3):
        a = T[i, 0] * dc[0]
        a = a + T[i, 1] * dc[1]
        a = a + T[i, 2] * dc[2]
        dl.append(a.astype(F))
    d = np.stack(dl, axis=-1).reshape(-1, 3)
    o = np.broadcast_to(T[:3, 3], d.shape).astype(F)
    return o, d, dc[2].reshape(-1).astype(F), (rows, cols)


def render_depth(tsdf, T_L_C, cam, subsampling, voxel_size, trunc, eps_m, max_steps, max_len):
    """-> (depth [rows, cols] f32, 0 = no surface; hit [rows, cols])"""
    o, d, dcz, shape = view_rays(T_L_C, cam, subsampling)
    t, hit = cast(tsdf, o, d, voxel_size, trunc, eps_m, max_steps, max_len)
    return np.where(hit, t * dcz, F(0)).astype(F).reshape(shape), hit.reshape(shape)


def hit_points(origins, directions, t):
    o = np.asarray(origins, F).reshape(-1, 3); d = np.asarray(directions, F).reshape(-1, 3); t = np.asarray(t, F)
    return np.stack([o[:, k] + t * d[:, k] for k in range(3)], axis=1)


def colors(color, origins, directions, t, hit, voxel_size):
    """colour [n, 3] u8 at the hit points: the colour voxel that contains P where its weight is > 0, grey 127 otherwise, 0 on a miss"""
    p = hit_points(origins, directions, t)
    found, v = color.lookup(_voxel_of(p, voxel_size))
    has = found & (v["weight"].astype(F) > 0)
    rgb = np.stack([np.where(has, v[ch], 127) for ch in ("r", "g", "b")], axis=1).astype(np.uint8)
    return np.where(np.asarray(hit, bool)[:, None], rgb, 0).astype(np.uint8)


def normals(tsdf, origins, directions, t, hit, voxel_size, min_weight=OBSERVED_WEIGHT):
    """unit gradient [n, 3] f32 of the trilinear TSDF interpolant at the hit points (corners b, b + 1 with u = p / vs - 0.5, b = floor(u), all of
    weight >= min_weight); 0 on a miss, where a corner is missing or where the gradient vanishes"""
    p = hit_points(origins, directions, t)
    hit = np.asarray(hit, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        u = p / F(voxel_size) - F(0.5)
        fl = np.floor(u)
    ok = hit & np.isfinite(fl).all(axis=1) & (np.abs(np.where(np.isfinite(fl), fl, 0)) < VOX_LIMIT - 2).all(axis=1)
    b = np.where(ok[:, None], fl, 0).astype(np.int64)
    w1 = np.where(ok[:, None], u - fl, 0).astype(np.float64); w0 = 1.0 - w1
    c = np.zeros((len(p), 2, 2, 2))
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                found, v = tsdf.lookup(b + np.array([i, j, k]))
                ok &= found & (v["weight"].astype(F) >= F(min_weight))
                c[:, i, j, k] = v["distance"]
    wx = np.stack([w0[:, 0], w1[:, 0]], 1); wy = np.stack([w0[:, 1], w1[:, 1]], 1); wz = np.stack([w0[:, 2], w1[:, 2]], 1)
    g = np.stack([np.einsum("nj,nk,njk->n", wy, wz, c[:, 1] - c[:, 0]),
                  np.einsum("ni,nk,nik->n", wx, wz, c[:, :, 1] - c[:, :, 0]),
                  np.einsum("ni,nj,nij->n", wx, wy, c[:, :, :, 1] - c[:, :, :, 0])], axis=1) / float(F(voxel_size))
    length = np.linalg.norm(g, axis=1)
    ok &= length > 0
    return np.where(ok[:, None], g / np.maximum(length, 1e-300)[:, None], 0.0).astype(F)
