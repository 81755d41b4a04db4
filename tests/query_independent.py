"""Independent float64 model of the interpolated point queries (SEMANTICS.md "Point queries"; nvbx_query_points).

Reads the corner voxels through a `get_blocks(layer, indices) -> (blocks, found)` callable (Mapper.get_blocks: host copies in the
reference's voxel order z + 8y + 64x) for the unique blocks the query points touch, and applies the semantics in numpy float64.
Only the corner coordinates follow the product's float32 rule (u = p / vs - 0.5, b = floor(u), t = u - b in IEEE f32): they decide
WHICH voxels are corners, and validity must agree exactly.  Shares no code with the library's kernels or the oracle.
"""
import numpy as np

LAYER_TSDF, LAYER_ESDF = 1, 4
VOX_LIMIT = 1 << 23          # addressable voxel indices: [-2^23, 2^23) (blocks [-2^20, 2^20))


def corner_coordinates(points, voxel_size):
    """-> (b int64 [n, 3], t float64 [n, 3], ok bool [n, 3]) with the f32 rule of the semantics."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        u = p / np.float32(voxel_size) - np.float32(0.5)
        f = np.floor(u)
        ok = (f >= -VOX_LIMIT) & (f <= VOX_LIMIT - 2)
        t = np.where(ok, u - f, 0.0).astype(np.float64)
    b = np.where(ok, f, 0.0).astype(np.int64)
    return b, t, ok


def plane_vz(slice_height, voxel_size):
    """global voxel z of a 2-D ESDF mapper's plane: floor(esdf_slice_height / voxel_size) in f32"""
    return int(np.floor(np.float32(slice_height) / np.float32(voxel_size)))


def _fetch(get_blocks, layer, vox, voxel_size, min_weight):
    """corner values (float64) and validity at global voxel indices vox [m, 3]"""
    blk = vox >> 3
    keys, inv = np.unique(blk, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    val = np.zeros(len(vox)); good = np.zeros(len(vox), bool)
    if len(keys) == 0:
        return val, good
    blocks, found = get_blocks(layer, keys.astype(np.int32))
    loc = vox & 7
    lin = loc[:, 2] + 8 * loc[:, 1] + 64 * loc[:, 0]          # the reference's order in host copies
    v = blocks[inv, lin]
    if layer == LAYER_TSDF:
        val = v["distance"].astype(np.float64)
        good = found[inv] & (v["weight"] >= np.float32(min_weight))
    else:
        val = np.sqrt(v["squared_distance_vox"].astype(np.float64)) * float(np.float32(voxel_size))
        val = np.where(v["is_inside"] != 0, -val, val)
        good = found[inv] & (v["observed"] != 0)
    return val, good


def query(get_blocks, layer, points, voxel_size, min_weight=0.0, unknown_value=1000.0, plane=None):
    """-> (distance [n], gradient [n, 3], valid [n]) in float64.  plane: ESDF of a 2-D mapper -- the global voxel z of its plane
    (bilinear in x, y; p.z ignored; gradient z = 0)."""
    b, t, ok = corner_coordinates(points, voxel_size)
    n = len(b)
    if plane is not None:
        b[:, 2] = plane; t[:, 2] = 0.0; ok[:, 2] = True
    okp = ok.all(axis=1)
    corners = [(i, j, k) for k in ((0,) if plane is not None else (0, 1)) for j in (0, 1) for i in (0, 1)]
    idx = np.nonzero(okp)[0]
    c = np.zeros((n, 2, 2, 2)); valid = okp.copy()
    if len(idx):
        allv = np.concatenate([b[idx] + np.array(o) for o in corners])
        val, good = _fetch(get_blocks, layer, allv, voxel_size, min_weight)
        m = len(idx)
        for q, (i, j, k) in enumerate(corners):
            c[idx, i, j, k] = val[q * m:(q + 1) * m]
            valid[idx] &= good[q * m:(q + 1) * m]
    vs = float(np.float32(voxel_size))
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    wx = np.stack([1 - tx, tx], 1); wy = np.stack([1 - ty, ty], 1); wz = np.stack([1 - tz, tz], 1)
    if plane is not None:
        c2 = c[:, :, :, 0]
        d = np.einsum("ni,nj,nij->n", wx, wy, c2)
        gx = np.einsum("nj,nj->n", wy, c2[:, 1, :] - c2[:, 0, :]) / vs
        gy = np.einsum("ni,ni->n", wx, c2[:, :, 1] - c2[:, :, 0]) / vs
        gz = np.zeros(n)
    else:
        d = np.einsum("ni,nj,nk,nijk->n", wx, wy, wz, c)
        gx = np.einsum("nj,nk,njk->n", wy, wz, c[:, 1] - c[:, 0]) / vs
        gy = np.einsum("ni,nk,nik->n", wx, wz, c[:, :, 1] - c[:, :, 0]) / vs
        gz = np.einsum("ni,nj,nij->n", wx, wy, c[:, :, :, 1] - c[:, :, :, 0]) / vs
    g = np.stack([gx, gy, gz], 1)
    d = np.where(valid, d, float(np.float32(unknown_value)))
    g = np.where(valid[:, None], g, 0.0)
    return d, g, valid


def corner_block_counts(points, voxel_size, plane=None):
    """number of distinct blocks (1, 2, 4, 8) the corners of each point lie in"""
    b, _, _ = corner_coordinates(points, voxel_size)
    cross = (b & 7) == 7
    if plane is not None:
        cross[:, 2] = False
    return 1 << cross.sum(axis=1)
