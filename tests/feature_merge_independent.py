"""Independent numpy model of feature merging (SEMANTICS.md "Feature merging"; nvbx_merge_features).

Works on dictionaries {(bx, by, bz): (features [512, C] float16, weights [512] float32)} of feature blocks in the public layout (voxel
t = vx 64 + vy 8 + vz, what Mapper.feature_blocks hands out) and on the set of blocks the destination holds with its TSDF layer: the candidate
rule in float64, positions, the containing voxel and the blend in float32 with the evaluation order the semantics pin.  Shares no code with
the library; the transform and its float64 inverse are those of tests/merge_independent.py.
"""
import numpy as np

from merge_independent import transforms, pose, rodrigues, MARGIN_VOX, OK, EMPTY_SOURCE, NO_OVERLAP      # noqa: F401  (re-exported for the tests)

DEFAULTS = {"min_weight": 0.0, "weight_scale": 1.0}
VOX_LIMIT = 1 << 23
F32 = np.float32
F16 = np.float16

_LANE = np.arange(512)
LANE_XYZ = np.stack([_LANE >> 6, (_LANE >> 3) & 7, _LANE & 7], 1)          # voxel (x, y, z) of t = vx 64 + vy 8 + vz


# ---------------------------------------------------------------------------------------------- candidates (float64)
def candidate_boxes(T, src_keys, voxel_size):
    """-> (lo [n, 3], hi [n, 3]) int64 block ranges of the destination per source block: the cube [8 s vs, (8 s + 8) vs) of positions whose
    containing voxel lies in block s, transformed, padded, turned into the blocks with a voxel centre inside"""
    R_DS, t_DS, _, _ = transforms(T)
    R = R_DS.astype(np.float64); t = t_DS.astype(np.float64)
    vs = float(F32(voxel_size)); pad = MARGIN_VOX * vs
    s = np.asarray(src_keys, np.int64).reshape(-1, 3).astype(np.float64)
    c = np.stack([(8.0 * s) * vs, (8.0 * s + 8.0) * vs], 0)          # [2, n, 3]
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
    """the set of destination block indices the boxes name (before the destination's own blocks are looked at)"""
    lo, hi = candidate_boxes(T, src_keys, voxel_size)
    out = set()
    for l, h in zip(lo, hi):
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    out.add((int(x), int(y), int(z)))
    return out


# ---------------------------------------------------------------------------------------------- positions and the containing voxel (float32)
def source_positions(T, blocks, voxel_size):
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


def source_voxels(T, blocks, voxel_size):
    """-> (n int64 [k, 512, 3], addressable [k, 512]): n = floor(p_S / vs) per axis in float32"""
    ps = source_positions(T, blocks, voxel_size)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(ps / F32(voxel_size))
        ok = ((f >= -VOX_LIMIT) & (f < VOX_LIMIT)).all(axis=-1)
    return np.where(ok[..., None], f, 0.0).astype(np.int64), ok


def reach(T, blocks, voxel_size):
    """per destination block: the number of distinct source blocks per axis its voxels' n lie in (over the addressable ones)"""
    n, ok = source_voxels(T, np.asarray(blocks, np.int64).reshape(-1, 3), voxel_size)
    b = n >> 3
    lo = np.where(ok[..., None], b, np.iinfo(np.int64).max).min(axis=1)
    hi = np.where(ok[..., None], b, np.iinfo(np.int64).min).max(axis=1)
    return hi - lo + 1


def _key(b):
    b = np.asarray(b, np.int64) + (1 << 20)
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]


# ---------------------------------------------------------------------------------------------- the call
def merge_features(dst_tsdf_keys, dst_feat, src_feat, T, voxel_size, max_weight, min_weight=0.0, weight_scale=1.0):
    """-> dict: feat (the destination's feature dictionary afterwards), candidates (sorted list of the destination blocks visited), fused
    ({block: bool[512]}), flagged (sorted list) and the result record's fields.  The inputs are not modified.
    dst_tsdf_keys: the blocks the destination holds with its TSDF layer (dst_feat's keys are among them)."""
    out = {k: (np.array(f, F16), np.array(w, F32)) for k, (f, w) in dst_feat.items()}
    res = {"feat": out, "candidates": [], "fused": {}, "flagged": [], "source_blocks": len(src_feat), "candidate_blocks": 0, "blocks_flagged": 0,
           "voxels_fused": 0, "status": EMPTY_SOURCE}
    if not src_feat:
        return res
    have = set(tuple(int(q) for q in k) for k in dst_tsdf_keys)
    cand = sorted(candidates(T, sorted(src_feat), voxel_size) & have)
    res["candidates"] = cand; res["candidate_blocks"] = len(cand)
    res["status"] = NO_OVERLAP
    if not cand:
        return res
    ch = next(iter(src_feat.values()))[0].shape[1]
    sk = sorted(src_feat)
    skeys = _key(np.array(sk, np.int64)); order = np.argsort(skeys); skeys = skeys[order]
    sf = np.stack([np.asarray(src_feat[sk[i]][0], F16) for i in order]); sw = np.stack([np.asarray(src_feat[sk[i]][1], F32) for i in order])
    n, ok = source_voxels(T, np.array(cand, np.int64), voxel_size)
    k = _key(n >> 3)
    pos = np.minimum(np.searchsorted(skeys, k), len(skeys) - 1)
    found = ok & (skeys[pos] == k)
    l = n & 7
    lin = l[..., 2] + 8 * l[..., 1] + 64 * l[..., 0]
    pos = np.where(found, pos, 0)
    ws = np.where(found, sw[pos, lin], F32(0.0)).astype(F32)
    passed = found & (ws > 0) & (ws >= F32(min_weight))
    max_weight = F32(max_weight); scale = F32(weight_scale)
    for i, b in enumerate(cand):
        p = passed[i]
        if not p.any():
            continue                                              # not written, not flagged
        fresh = b not in out
        if fresh:
            old_f = np.zeros((512, ch), F16); old_w = np.zeros(512, F32)
            res["flagged"].append(b)
        else:
            old_f, old_w = out[b]
        f = sf[pos[i], lin[i]].astype(F32)                          # [512, C]
        with np.errstate(invalid="ignore", divide="ignore"):
            w0 = old_w.astype(F32); w1 = (ws[i] * scale).astype(F32)
            tw = (w0 + w1).astype(F32)
            ca = (w0 / tw).astype(F32); cb = (w1 / tw).astype(F32)
            v = ((old_f.astype(F32) * ca[:, None]).astype(F32) + (f * cb[:, None]).astype(F32)).astype(F32)
            nw = np.minimum(tw, max_weight)
        new_f = np.where(p[:, None], v.astype(F16), old_f); new_w = np.where(p, nw, old_w).astype(F32)
        out[b] = (new_f.astype(F16), new_w)
        res["fused"][b] = p
    res["blocks_flagged"] = len(res["flagged"])
    res["voxels_fused"] = int(sum(int(p.sum()) for p in res["fused"].values()))
    res["status"] = OK if res["voxels_fused"] else NO_OVERLAP
    return res


def read_features(mapper, M):
    """{block: (features [512, C], weights [512])} of a Mapper, through block_indices / feature_blocks"""
    idx = np.asarray(mapper.block_indices(M.LAYER_FEATURE), np.int32).reshape(-1, 3)
    if not len(idx):
        return {}
    f, w, found = mapper.feature_blocks(idx)
    assert found.all()
    return {tuple(int(q) for q in b): (f[i].copy(), w[i].copy()) for i, b in enumerate(idx)}
