"""An independent model of frontiers and view gain (SEMANTICS.md "Frontiers and view gain") in numpy float32: the voxel classes, the frontier
rule over a sparse block set, clusters of frontier voxels, and the per-ray walk of view_gain.  It imports nothing from the product or the
oracle; the component records come from segment_independent's scipy-free union-find, another test-side model."""
import numpy as np

F32 = np.float32
TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
INDEX_LIMIT = 1 << 20                      # addressable block indices: [-2^20, 2^20) per axis
T512 = np.arange(512)
OFF = np.stack([T512 >> 6, (T512 >> 3) & 7, T512 & 7], 1)      # voxel t = vx 64 + vy 8 + vz
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def classify(distance, weight, min_weight, free_distance_m):
    """classes of stored voxels, float32 comparisons: observed iff w >= min_weight; free iff observed and d > free_distance_m (a NaN is not)"""
    d = np.asarray(distance, F32); w = np.asarray(weight, F32)
    with np.errstate(invalid="ignore"):
        obs = w >= F32(min_weight)
        free = obs & (d > F32(free_distance_m))
    return np.where(free, FREE, np.where(obs, OCCUPIED, UNKNOWN)).astype(np.uint8)


def block_classes(tsdf, min_weight, free_distance_m):
    """{block: TSDF_DT[512]} -> {block: classes [8, 8, 8] indexed [x, y, z]}"""
    return {k: classify(v["distance"], v["weight"], min_weight, free_distance_m).reshape(8, 8, 8) for k, v in tsdf.items()}


def in_range(b):
    return all(-INDEX_LIMIT <= int(q) < INDEX_LIMIT for q in b)


def frontiers(tsdf, min_weight, free_distance_m, min_unknown=1, box_vox=None):
    """tsdf: {block: TSDF_DT[512]} -> {block: (label int32[512], score float32[512])} for every block with a frontier voxel.
    box_vox: (min x, y, z, max x, y, z) inclusive in global voxel coordinates, or None"""
    cls = block_classes(tsdf, min_weight, free_distance_m)
    out = {}
    for b, c in cls.items():
        if not (c == FREE).any():
            continue
        unk = np.ones((10, 10, 10), bool)                      # the block and one voxel around it; what no block covers is unknown
        unk[1:9, 1:9, 1:9] = c == UNKNOWN
        for (dx, dy, dz) in FACES:
            nb = (b[0] + dx, b[1] + dy, b[2] + dz)
            if nb in cls and in_range(nb):
                n = cls[nb] == UNKNOWN
                if dx:
                    unk[0 if dx < 0 else 9, 1:9, 1:9] = n[7 if dx < 0 else 0, :, :]
                elif dy:
                    unk[1:9, 0 if dy < 0 else 9, 1:9] = n[:, 7 if dy < 0 else 0, :]
                else:
                    unk[1:9, 1:9, 0 if dz < 0 else 9] = n[:, :, 7 if dz < 0 else 0]
        u = unk.astype(np.int32)
        nu = (u[0:8, 1:9, 1:9] + u[2:10, 1:9, 1:9] + u[1:9, 0:8, 1:9] + u[1:9, 2:10, 1:9] + u[1:9, 1:9, 0:8] + u[1:9, 1:9, 2:10])
        fr = (c == FREE) & (nu >= int(min_unknown))
        if box_vox is not None:
            g = 8 * np.asarray(b, np.int64)[None] + OFF
            inside = np.all((g >= np.asarray(box_vox[:3])) & (g <= np.asarray(box_vox[3:])), axis=1).reshape(8, 8, 8)
            fr &= inside
        if fr.any():
            out[tuple(int(q) for q in b)] = (np.where(fr, 0, -1).astype(np.int32).reshape(512), np.where(fr, nu, 0).astype(F32).reshape(512))
    return out


def box_from_metres(box_m, voxel_size):
    """the wrapper's conversion: floor(p / voxel_size) in float32 of both corners"""
    b = np.asarray(box_m, F32).reshape(2, 3)
    return tuple(int(v) for v in np.floor(b / F32(voxel_size)).astype(np.int64).reshape(6))


def as_lists(fr):
    """{block: (label, score)} -> (block_idx [n, 3] int32, label [n, 512], score [n, 512]) in sorted block order"""
    ks = sorted(fr)
    if not ks:
        return np.zeros((0, 3), np.int32), np.zeros((0, 512), np.int32), np.zeros((0, 512), F32)
    return np.array(ks, np.int32), np.stack([fr[k][0] for k in ks]), np.stack([fr[k][1] for k in ks])


def clusters(fr, connectivity, min_voxels=1):
    """components of the frontier voxels in segment_independent's form: ({lowest voxel: record}, keys [n, 512]) over as_lists(fr)"""
    import segment_independent as SI
    idx, lab, sc = as_lists(fr)
    if not len(idx):
        return {}, np.zeros((0, 512), np.int64)
    return SI.model_union_find(idx, lab, sc, connectivity, min_voxels)


# ---------------------------------------------------------------------------------------------- view gain
def pose_ok(T, voxel_size, reach):
    """nvbx_render_view's pose rule in float32: finite, and everything within reach stays inside the addressable blocks"""
    T = np.asarray(T, F32).reshape(16)
    if not np.all(np.isfinite(T)):
        return False
    lim = (F32(INDEX_LIMIT) - F32(2.0)) * (F32(voxel_size) * F32(8.0)) - F32(reach)
    return bool(abs(T[3]) < lim and abs(T[7]) < lim and abs(T[11]) < lim)


def ray_directions(T, cam, s):
    """the rays of nvbx_render_view at subsampling s, float32, in its evaluation order: -> [rows / s, cols / s, 3] in the layer frame"""
    fu, fv, cu, cv, w, h = cam
    T = np.asarray(T, F32).reshape(4, 4)
    rows, cols = int(h) // s, int(w) // s
    c = (np.arange(cols, dtype=np.int64) * s).astype(F32); r = (np.arange(rows, dtype=np.int64) * s).astype(F32)
    rx = np.broadcast_to((((c + F32(0.5)) - F32(cu)) / F32(fu))[None, :], (rows, cols))
    ry = np.broadcast_to((((r + F32(0.5)) - F32(cv)) / F32(fv))[:, None], (rows, cols))
    n = np.sqrt((rx * rx + ry * ry) + F32(1.0))
    dc = [rx / n, ry / n, F32(1.0) / n]
    d = np.empty((rows, cols, 3), F32)
    for i in range(3):
        acc = T[i, 0] * dc[0]
        acc = acc + T[i, 1] * dc[1]
        acc = acc + T[i, 2] * dc[2]
        d[..., i] = acc
    return d


def sample_voxels(o, d, k, voxel_size):
    """global voxel of sample k of the rays (o, d[n, 3]): t = (k + 0.5) voxel_size, p = o + t d, floor(p / voxel_size), all float32"""
    vs = F32(voxel_size)
    t = (F32(k) + F32(0.5)) * vs
    p = np.asarray(o, F32)[None, :] + t * d
    return t, np.floor(p / vs).astype(np.int64)


def view_gain(tsdf, poses, cam, subsampling, max_range_m, voxel_size, min_weight, free_distance_m):
    """-> int32 [n, 4]: rays, unknown_samples, free_samples, rays_hit per pose; rays = -1 and zeros for a pose that fails pose_ok"""
    cls = {k: v.reshape(512) for k, v in block_classes(tsdf, min_weight, free_distance_m).items()}
    out = np.zeros((len(poses), 4), np.int32)
    for i, T in enumerate(poses):
        if not pose_ok(T, voxel_size, max_range_m):
            out[i, 0] = -1
            continue
        T = np.asarray(T, F32).reshape(4, 4)
        d = ray_directions(T, cam, subsampling).reshape(-1, 3)
        o = T[:3, 3]
        alive = np.ones(len(d), bool)
        unknown = free = hit = 0
        k = 0
        while alive.any():
            t, g = sample_voxels(o, d[alive], k, voxel_size)
            if not (t < F32(max_range_m)):
                break
            c = np.zeros(len(g), np.uint8)
            blocks = g >> 3
            lane = ((g[:, 0] & 7) << 6) + ((g[:, 1] & 7) << 3) + (g[:, 2] & 7)
            ub, inv = np.unique(blocks, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            for j, b in enumerate(ub):
                blk = cls.get(tuple(int(q) for q in b))
                if blk is not None and in_range(b):
                    sel = inv == j
                    c[sel] = blk[lane[sel]]
            unknown += int((c == UNKNOWN).sum()); free += int((c == FREE).sum()); hit += int((c == OCCUPIED).sum())
            ids = np.flatnonzero(alive)
            alive[ids[c == OCCUPIED]] = False
            k += 1
        out[i] = (len(d), unknown, free, hit)
    return out


def read_tsdf(mapper, M):
    """{block: TSDF_DT[512]} of a Mapper, through block_indices / get_blocks"""
    idx = mapper.block_indices(M.LAYER_TSDF)
    if not len(idx):
        return {}
    v, found = mapper.get_blocks(M.LAYER_TSDF, idx)
    assert found.all()
    return {tuple(int(q) for q in b): v[i].copy() for i, b in enumerate(idx)}
