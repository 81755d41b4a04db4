"""Independent numpy model of map merging (SEMANTICS.md "Map merging"; nvbx_merge_map).

Works on dictionaries {(bx, by, bz): block[512]} of voxels in the reference's order z + 8y + 64x (what Mapper.get_blocks hands out): the
candidate rule in float64, positions, sampling, fusing and colour blending in float32 with the evaluation order the semantics pin, band
bits per x slab.  `dtype=np.float64` runs the interpolation and the fuse in float64 over the same corner voxels (the corner indices always
follow the f32 rule: they decide WHICH voxels are read).  Shares no code with the library; it may be used with tests/query_independent.py.
"""
import numpy as np

TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
COLOR_DT = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("pad", "u1"), ("weight", "<f4")])
OK, EMPTY_SOURCE, NO_OVERLAP = 0, 1, 2
DEFAULTS = {"min_weight": 1e-4, "weight_scale": 1.0, "merge_color": 1}
MARGIN_VOX = 0.01
ROTATION_TOL = 1e-5
VOX_LIMIT = 1 << 23
F32 = np.float32

_LANE = np.arange(512)
LANE_XYZ = np.stack([_LANE >> 6, (_LANE >> 3) & 7, _LANE & 7], 1)          # voxel (x, y, z) of lane z + 8y + 64x


# ---------------------------------------------------------------------------------------------- transforms and candidates (float64)
def rotation_error(T):
    """(largest |R^T R - I| entry, det R) of the f32 pose, in float64"""
    R = np.asarray(T, F32).reshape(4, 4)[:3, :3].astype(np.float64)
    return float(np.abs(R.T @ R - np.eye(3)).max()), float(np.linalg.det(R))


def rotation_ok(T):
    err, det = rotation_error(T)
    return bool(err <= ROTATION_TOL and det > 0.0)


def transforms(T):
    """-> (R_DS, t_DS, R_SD, t_SD) float32: the forward pair is T as it is, the inverse is summed in float64 and rounded once"""
    T = np.asarray(T, F32).reshape(4, 4)
    R_DS = T[:3, :3].copy(); t_DS = T[:3, 3].copy()
    R_SD = R_DS.T.copy()
    Rd = R_SD.astype(np.float64); td = t_DS.astype(np.float64)
    t_SD = np.empty(3, F32)
    for i in range(3):
        s = Rd[i, 0] * td[0]
        s = s + Rd[i, 1] * td[1]
        s = s + Rd[i, 2] * td[2]
        t_SD[i] = F32(-s)
    return R_DS, t_DS, R_SD, t_SD


def candidate_boxes(T, src_keys, voxel_size):
    """-> (lo [n, 3], hi [n, 3]) int64 block ranges of the destination per source block"""
    R_DS, t_DS, _, _ = transforms(T)
    R = R_DS.astype(np.float64); t = t_DS.astype(np.float64)
    vs = float(F32(voxel_size)); pad = MARGIN_VOX * vs
    s = np.asarray(src_keys, np.int64).reshape(-1, 3).astype(np.float64)
    c = np.stack([(8.0 * s + 0.5) * vs, (8.0 * s + 8.5) * vs], 0)          # [2, n, 3]
    mn = np.full(s.shape, np.inf); mx = np.full(s.shape, -np.inf)
    for q in range(8):
        x = c[q & 1, :, 0]; y = c[(q >> 1) & 1, :, 1]; z = c[(q >> 2) & 1, :, 2]
        for a in range(3):
            v = R[a, 0] * x
            v = v + R[a, 1] * y
            v = v + R[a, 2] * z
            v = v + t[a]
            mn[:, a] = np.minimum(mn[:, a], v); mx[:, a] = np.maximum(mx[:, a], v)
    kl = np.ceil((mn - pad) / vs - 0.5).astype(np.int64); kh = np.floor((mx + pad) / vs - 0.5).astype(np.int64)
    return kl >> 3, kh >> 3


def candidates(T, src_keys, voxel_size):
    """the set of destination blocks the merge goes over"""
    lo, hi = candidate_boxes(T, src_keys, voxel_size)
    out = set()
    for l, h in zip(lo, hi):
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    out.add((int(x), int(y), int(z)))
    return out


# ---------------------------------------------------------------------------------------------- positions and sampling
def sample_positions(T, blocks, voxel_size):
    """p_S float32 [n, 512, 3] of the voxel centres of destination blocks [n, 3]"""
    _, _, R, t = transforms(T)
    vs = F32(voxel_size)
    g = (8 * np.asarray(blocks, np.int64).reshape(-1, 1, 3) + LANE_XYZ[None]).astype(F32)
    pd = (g + F32(0.5)) * vs
    x, y, z = pd[..., 0], pd[..., 1], pd[..., 2]
    ps = np.empty_like(pd)
    for i in range(3):
        s = R[i, 0] * x
        s = s + R[i, 1] * y
        s = s + R[i, 2] * z
        ps[..., i] = s + t[i]
    return ps


def base_voxels(ps, voxel_size):
    """-> (b int64, t float32, ok) per axis: u = p / vs - 0.5, b = floor(u), t = u - b in float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = ps / F32(voxel_size) - F32(0.5)
        f = np.floor(u)
        ok = (f >= -VOX_LIMIT) & (f <= VOX_LIMIT - 2)
        t = np.where(ok, u - f, F32(0.0)).astype(F32)
    return np.where(ok, f, 0.0).astype(np.int64), t, ok.all(axis=-1)


def _key(b):
    b = np.asarray(b, np.int64) + (1 << 20)
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]


class _Table:
    """blocks of a dictionary stacked, found by sorted key"""

    def __init__(self, blocks, dt):
        ks = sorted(blocks)
        self.keys = _key(np.array(ks, np.int64).reshape(-1, 3)) if ks else np.zeros(0, np.int64)
        order = np.argsort(self.keys)
        self.keys = self.keys[order]
        self.data = np.stack([np.asarray(blocks[ks[i]], dt).reshape(512) for i in order]) if ks else np.zeros((0, 512), dt)

    def gather(self, vox):
        """voxels at global voxel indices vox [..., 3] -> (found, records)"""
        k = _key(vox >> 3)
        pos = np.searchsorted(self.keys, k)
        pos = np.minimum(pos, max(len(self.keys) - 1, 0))
        found = (self.keys[pos] == k) if len(self.keys) else np.zeros(k.shape, bool)
        l = vox & 7
        lin = l[..., 2] + 8 * l[..., 1] + 64 * l[..., 0]
        rec = self.data[np.where(found, pos, 0), lin] if len(self.keys) else np.zeros(k.shape, self.data.dtype)
        return found, rec


def _trilinear(c, tx, ty, tz):
    """c[..., i + 2j + 4k]: along x, then y, then z -- the order of the point query"""
    dx00 = c[..., 1] - c[..., 0]; dx10 = c[..., 3] - c[..., 2]; dx01 = c[..., 5] - c[..., 4]; dx11 = c[..., 7] - c[..., 6]
    a00 = c[..., 0] + tx * dx00; a10 = c[..., 2] + tx * dx10; a01 = c[..., 4] + tx * dx01; a11 = c[..., 6] + tx * dx11
    dy0 = a10 - a00; dy1 = a11 - a01
    b0 = a00 + ty * dy0; b1 = a01 + ty * dy1
    return b0 + tz * (b1 - b0)


def sample(src_table, ps, voxel_size, min_weight, dtype=F32):
    """-> (valid, d_s, w_s before weight_scale, b) at positions ps [..., 3]"""
    b, t, ok = base_voxels(ps, voxel_size)
    cd = np.zeros(ps.shape[:-1] + (8,), dtype); cw = np.zeros(ps.shape[:-1] + (8,), dtype)
    valid = ok.copy()
    for q in range(8):
        off = np.array([q & 1, (q >> 1) & 1, q >> 2], np.int64)
        found, rec = src_table.gather(b + off)
        valid &= found & (rec["weight"] >= F32(min_weight))
        cd[..., q] = rec["distance"]; cw[..., q] = rec["weight"]
    tt = t.astype(dtype)
    d = _trilinear(cd, tt[..., 0], tt[..., 1], tt[..., 2])
    w = _trilinear(cw, tt[..., 0], tt[..., 1], tt[..., 2])
    return valid, d, w, b


def blend_u8(c0, w0, c1, w1):
    with np.errstate(invalid="ignore", divide="ignore"):
        tw = w0 + w1
        a = w0 / tw; b = w1 / tw
        v = c0 * a + c1 * b
        v = np.floor(v + F32(0.5))
    return np.clip(np.nan_to_num(v), 0, 255).astype(np.uint8)          # (0 / 0 only where the result is not used)


def in_band(d, w, trunc):
    return (w > F32(1e-4)) & (np.abs(d) < F32(trunc))


def band_bits(block, trunc):
    """the eight per-slab band bits of a TSDF block (bit x = some voxel of slab x is in the band)"""
    m = in_band(block["distance"], block["weight"], trunc).reshape(8, 64).any(axis=1)
    return int(sum(1 << x for x in range(8) if m[x]))


# ---------------------------------------------------------------------------------------------- the merge
def merge(dst_tsdf, dst_color, src_tsdf, src_color, T, voxel_size, trunc, max_weight, min_weight=1e-4, weight_scale=1.0, merge_color=1,
          blocks=None, dtype=F32):
    """-> dict: tsdf / color (the destination's dictionaries afterwards; color holds the blocks that carry the colour layer), candidates (sorted
    list), fused / colored ({block: bool[512]}), band ({block: bits}) and the result record's fields.  The inputs are not modified.
    blocks: go over these destination blocks instead of the candidate set (the completeness check of the tests)."""
    out_t = {k: np.array(v, TSDF_DT).reshape(512) for k, v in dst_tsdf.items()}
    out_c = {k: np.array(v, COLOR_DT).reshape(512) for k, v in dst_color.items()}
    res = {"tsdf": out_t, "color": out_c, "fused": {}, "colored": {}, "band": {}, "source_blocks": len(src_tsdf), "candidates": [],
           "candidate_blocks": 0, "blocks_allocated": 0, "voxels_fused": 0, "color_voxels_fused": 0, "status": EMPTY_SOURCE}
    if not src_tsdf:
        return res
    cand = sorted(candidates(T, sorted(src_tsdf), voxel_size)) if blocks is None else sorted(tuple(int(q) for q in b) for b in blocks)
    res["candidates"] = cand; res["candidate_blocks"] = len(cand)
    res["blocks_allocated"] = sum(1 for k in cand if k not in dst_tsdf)
    st = _Table(src_tsdf, TSDF_DT); sc = _Table(src_color, COLOR_DT)
    trunc = F32(trunc); max_weight = F32(max_weight)
    carr = np.array(cand, np.int64).reshape(-1, 3)
    ps = sample_positions(T, carr, voxel_size)
    valid, ds, ws, _ = sample(st, ps, voxel_size, min_weight, dtype)
    ws = ws * dtype(F32(weight_scale))
    cur = np.stack([out_t[k] if k in out_t else np.zeros(512, TSDF_DT) for k in cand])
    dd = cur["distance"].astype(dtype); wd = cur["weight"].astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = wd + ws
        fuse = valid & (w > 0)
        d = (ds * ws + dd * wd) / w
        d = np.clip(d, -dtype(trunc), dtype(trunc))
        wn = np.minimum(w, dtype(max_weight))
    new = cur.copy()
    new["distance"] = np.where(fuse, d, dd).astype(F32); new["weight"] = np.where(fuse, wn, wd).astype(F32)
    new["distance"][~fuse] = cur["distance"][~fuse]; new["weight"][~fuse] = cur["weight"][~fuse]      # untouched, bit for bit
    colored = np.zeros(fuse.shape, bool)
    ccur = np.stack([out_c[k] if k in out_c else np.zeros(512, COLOR_DT) for k in cand])
    cnew = ccur.copy()
    if merge_color:
        with np.errstate(invalid="ignore", over="ignore"):
            n = np.floor(ps / F32(voxel_size))
        n = np.where(np.isfinite(n), n, 0.0).astype(np.int64)
        found, rec = sc.gather(n)
        colored = fuse & found & (rec["weight"] > 0)
        w0 = ccur["weight"]; w1 = rec["weight"]
        for ch in ("r", "g", "b"):
            cnew[ch] = np.where(colored, blend_u8(ccur[ch].astype(F32), w0, rec[ch].astype(F32), w1), ccur[ch])
        cnew["pad"] = np.where(colored, 0, ccur["pad"])
        cnew["weight"] = np.where(colored, np.minimum(w0 + w1, max_weight), w0)
    for i, k in enumerate(cand):
        out_t[k] = new[i]
        res["fused"][k] = fuse[i]; res["colored"][k] = colored[i]
        res["band"][k] = band_bits(new[i], trunc)
        if k in out_c or colored[i].any():
            out_c[k] = cnew[i]
    res["voxels_fused"] = int(fuse.sum()); res["color_voxels_fused"] = int(colored.sum())
    res["status"] = OK if res["voxels_fused"] else NO_OVERLAP
    return res


def read_layers(mapper, M):
    """({block: tsdf[512]}, {block: color[512]}) of a Mapper, through block_indices / get_blocks"""
    out = []
    for layer in (M.LAYER_TSDF, M.LAYER_COLOR):
        idx = mapper.block_indices(layer)
        d = {}
        if len(idx):
            v, found = mapper.get_blocks(layer, idx)
            assert found.all()
            d = {tuple(int(q) for q in b): v[i].copy() for i, b in enumerate(idx)}
        out.append(d)
    return out[0], out[1]


def reach(T, blocks, voxel_size):
    """per destination block: the number of distinct source blocks per axis its samples' corners reach (over lanes with an addressable position)"""
    ps = sample_positions(T, np.asarray(blocks, np.int64).reshape(-1, 3), voxel_size)
    b, _, ok = base_voxels(ps, voxel_size)
    lo = np.where(ok[..., None], b >> 3, np.iinfo(np.int64).max).min(axis=1)
    hi = np.where(ok[..., None], (b + 1) >> 3, np.iinfo(np.int64).min).max(axis=1)
    return hi - lo + 1


# ---------------------------------------------------------------------------------------------- transforms the tests draw
def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(axis, angle_deg, t):
    T = np.eye(4)
    T[:3, :3] = rodrigues(axis, np.deg2rad(angle_deg)); T[:3, 3] = t
    return T.astype(F32)


def drawn_transforms(n=12, seed=3):
    rng = np.random.default_rng(seed)
    out = [pose([0, 0, 1], 0.0, [0, 0, 0]), pose([0, 0, 1], 45.0, [-3.13, 0.77, -1.91]), pose([1, 1, 1], 180.0, [0.4 * 8 * 0.05, -2.5 * 8 * 0.05, 7.25 * 8 * 0.05])]
    for _ in range(n):
        axis = rng.normal(size=3)
        out.append(pose(axis, rng.uniform(0.0, 180.0), rng.uniform(-4.0, 4.0, 3)))
    return out
