"""A numpy model of nvbx_surface_points (SEMANTICS.md "Surface points") that shares no code with the product: float32 per operation, a dict of
blocks in, rows out.

A map is {(bx, by, bz): block}; a block is a dict with "d" and "w" (float32 [8, 8, 8], indexed [vx, vy, vz]) where it carries the TSDF layer and
"rgb" (uint8 [8, 8, 8, 3]) with "cw" (float32 [8, 8, 8], the colour weight) where it carries the colour layer.  Rows come out block by block in
the dict's order, inside a block by t = vx 64 + vy 8 + vz, then by axis."""
import numpy as np

F32 = np.float32
LIMIT = 1 << 20      # addressable block indices: -2^20 .. 2^20 - 1


def floor_mod(g, s):
    """g modulo s with the mathematical sign, on Python integers (numpy's % on negative int32 is the same; this one does not rely on it)"""
    g = np.asarray(g, np.int64)
    return g - (np.floor(g.astype(np.float64) / float(s)).astype(np.int64)) * s


def observed(d, w, min_weight):
    return (w >= F32(min_weight)) & (d == d)


def center(b, v, vs):
    vs = F32(vs)
    return (F32(b) * (F32(8.0) * vs) + np.asarray(v, F32) * vs) + vs * F32(0.5)


def crossing_offset(d0, d1, vs):
    with np.errstate(all="ignore"):
        return F32(vs) * ((-np.asarray(d0, F32)) / (np.asarray(d1, F32) - np.asarray(d0, F32)))


def _neighbour_field(blocks, key, axis, name, fill):
    """the field `name` of the voxels one step along `axis` from every voxel of block `key`; `fill` where the neighbour block gives nothing"""
    own = blocks[key][name]
    nk = tuple(key[i] + (1 if i == axis else 0) for i in range(3))
    nb = blocks.get(nk)
    ok = nb is not None and name in nb and all(-LIMIT <= c < LIMIT for c in nk)
    face_shape = list(own.shape); face_shape[axis] = 1
    if ok:
        face = np.take(nb[name], [0], axis=axis)
    else:
        face = np.full(face_shape, fill, own.dtype)
    rest = np.take(own, list(range(1, 8)), axis=axis)
    return np.concatenate([rest, face], axis=axis), ok


def surface_rows(blocks, vs, min_weight=1e-4, stride=1, box=None, require_color=False):
    """-> dict of arrays: block [n, 3] i32, t [n] i32, axis [n] i32, points [n, 3] f32, colors [n, 3] u8"""
    out = {"block": [], "t": [], "axis": [], "points": [], "colors": []}
    vx, vy, vz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    for key, blk in blocks.items():
        if "d" not in blk:
            continue
        d0 = np.asarray(blk["d"], F32); w0 = np.asarray(blk["w"], F32)
        g = [8 * key[0] + vx, 8 * key[1] + vy, 8 * key[2] + vz]
        keep = np.ones((8, 8, 8), bool)
        if box is not None:
            for i in range(3):
                keep &= (g[i] >= box[i]) & (g[i] <= box[3 + i])
        for i in range(3):
            keep &= floor_mod(g[i], stride) == 0
        o0 = observed(d0, w0, min_weight)
        has_rgb0 = "rgb" in blk
        rgb0 = np.asarray(blk["rgb"], np.uint8) if has_rgb0 else np.zeros((8, 8, 8, 3), np.uint8)
        cw0 = np.asarray(blk["cw"], F32) if has_rgb0 else np.zeros((8, 8, 8), F32)
        rows = []
        for axis in range(3):
            d1, ok = _neighbour_field(blocks, key, axis, "d", F32(np.nan))
            w1, _ = _neighbour_field(blocks, key, axis, "w", F32(0))
            inside = np.ones((8, 8, 8), bool)
            sl = [slice(None)] * 3; sl[axis] = 7
            inside[tuple(sl)] = ok                         # the last layer's neighbour lies in the next block
            o1 = observed(d1, w1, min_weight) & inside
            cross = keep & o0 & o1 & ((d0 <= 0) != (d1 <= 0))
            # colour: the endpoint nearer the surface
            nk = tuple(key[i] + (1 if i == axis else 0) for i in range(3))
            nb = blocks.get(nk, {})
            rgb1 = np.concatenate([np.take(rgb0, list(range(1, 8)), axis=axis),
                                   np.take(np.asarray(nb["rgb"], np.uint8) if "rgb" in nb else np.zeros((8, 8, 8, 3), np.uint8), [0], axis=axis)], axis=axis)
            cw1 = np.concatenate([np.take(cw0, list(range(1, 8)), axis=axis),
                                  np.take(np.asarray(nb["cw"], F32) if "rgb" in nb else np.zeros((8, 8, 8), F32), [0], axis=axis)], axis=axis)
            near0 = np.abs(d0) <= np.abs(d1)
            cw = np.where(near0, cw0, cw1)
            rgb = np.where(near0[..., None], rgb0, rgb1)
            has = cw > 0
            rgb = np.where(has[..., None], rgb, np.uint8(0))
            if require_color:
                cross &= has
            p = [center(key[0], vx, vs), center(key[1], vy, vs), center(key[2], vz, vs)]
            p[axis] = p[axis] + crossing_offset(d0, d1, vs)
            idx = np.nonzero(cross)
            t = (idx[0] * 64 + idx[1] * 8 + idx[2]).astype(np.int32)
            rows.append((t, np.full(len(t), axis, np.int32), np.stack([q[idx] for q in p], 1).astype(F32), rgb[idx]))
        t = np.concatenate([r[0] for r in rows]); ax = np.concatenate([r[1] for r in rows])
        order = np.lexsort((ax, t))
        out["block"].append(np.tile(np.asarray(key, np.int32), (len(t), 1)))
        out["t"].append(t[order]); out["axis"].append(ax[order])
        out["points"].append(np.concatenate([r[2] for r in rows])[order]); out["colors"].append(np.concatenate([r[3] for r in rows])[order])
    if not out["t"]:
        return {"block": np.zeros((0, 3), np.int32), "t": np.zeros(0, np.int32), "axis": np.zeros(0, np.int32),
                "points": np.zeros((0, 3), F32), "colors": np.zeros((0, 3), np.uint8)}
    return {k: np.concatenate(v) for k, v in out.items()}


def row_set(points, colors=None):
    """the rows as a set of byte strings: the points' bits, with the colours where given"""
    p = np.ascontiguousarray(points, F32).view(np.uint32).reshape(-1, 3)
    if colors is None:
        return set(map(bytes, p))
    c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    return set(bytes(a) + bytes(b) for a, b in zip(p, c))


def unit_normals(gradient, valid):
    """gradients [n, 3] f32 and their validity -> the normals: divided by sqrt((gx gx + gy gy) + gz gz) in float32, 0 where invalid or zero"""
    g = np.asarray(gradient, F32)
    ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F32)
    ok = np.asarray(valid, bool) & (ln > 0)
    with np.errstate(all="ignore"):
        n = (g / ln[:, None]).astype(F32)
    return np.where(ok[:, None], n, F32(0)).astype(F32)


# ---- drawn fields
def blocks_from_function(keys, fn, vs, weight=1.0):
    """blocks `keys` with d = fn(x, y, z) at the voxel centres (float64 in, float32 stored) and a constant weight"""
    vx, vy, vz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    out = {}
    for k in keys:
        x = (8 * k[0] + vx + 0.5) * float(vs); y = (8 * k[1] + vy + 0.5) * float(vs); z = (8 * k[2] + vz + 0.5) * float(vs)
        out[tuple(k)] = {"d": np.asarray(fn(x, y, z), np.float64).astype(F32), "w": np.full((8, 8, 8), weight, F32)}
    return out
