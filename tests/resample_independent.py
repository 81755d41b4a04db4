"""Independent numpy model of map resampling (SEMANTICS.md "Resampling"; nvbx_resample_map).

Works on dictionaries {(bx, by, bz): block[512]} of voxels in the order z + 8y + 64x, as tests/merge_independent.py does, and takes that
model's building blocks (the f32 transform pair, the per-axis base voxel, the eight-corner sample, the colour blend, the band bits): the
candidate rule in float64 with two voxel sizes, the taps, their reduction, the fuse and the colour rule are written out here.  Float32 in
the evaluation order the semantics pin; `dtype=np.float64` evaluates the tap positions, the interpolation, the reduction and the fuse in
float64 over the same float32 inputs and the same corner voxels (the corner indices and the validity always follow the f32 rule: they
decide WHICH voxels are read).  Shares no code with the library."""
import math

import numpy as np

import merge_independent as MI

TSDF_DT, COLOR_DT = MI.TSDF_DT, MI.COLOR_DT
OK, EMPTY_SOURCE, NO_OVERLAP = MI.OK, MI.EMPTY_SOURCE, MI.NO_OVERLAP
DEFAULTS = {"min_weight": 1e-4, "weight_scale": 1.0, "merge_color": 1, "taps": 0}
MAX_RATIO, MAX_TAPS = 4.0, 4
F32 = np.float32
LANE_XYZ = MI.LANE_XYZ


# ---------------------------------------------------------------------------------------------- the host-side numbers
def ratio(vs_d, vs_s):
    """r = (double)vs_d / (double)vs_s of the two float32 voxel sizes"""
    return float(F32(vs_d)) / float(F32(vs_s))


def ratio_ok(vs_d, vs_s):
    if not (F32(vs_s) > 0 and F32(vs_d) > 0):
        return False
    return bool(1.0 <= ratio(vs_d, vs_s) <= MAX_RATIO)


def taps_for(r, taps=0):
    """n: `taps` in 1 .. 4 as it is, 0 = min(4, ceil(r)); None if refused"""
    if taps < 0 or taps > MAX_TAPS:
        return None
    return int(taps) if taps else int(min(MAX_TAPS, max(1, math.ceil(r))))


def tap_offsets(n):
    """o_i = ((float)i + 0.5f) / (float)n - 0.5f"""
    i = np.arange(n).astype(F32)
    return ((i + F32(0.5)) / F32(n) - F32(0.5)).astype(F32)


def reach_bound(r, n):
    """N = ceil((floor(sqrt(3) (8 - 1/n) r) + 2) / 8) + 1"""
    L = math.sqrt(3.0) * (8.0 - 1.0 / n) * r
    return int(math.ceil((math.floor(L) + 2.0) / 8.0)) + 1


# ---------------------------------------------------------------------------------------------- candidates (float64)
def candidate_boxes(T, src_keys, vs_s, vs_d, n):
    """-> (lo [m, 3], hi [m, 3]) int64 block ranges of the destination per source block"""
    R_DS, t_DS, _, _ = MI.transforms(T)
    R = R_DS.astype(np.float64); t = t_DS.astype(np.float64)
    vs = float(F32(vs_s)); vd = float(F32(vs_d))
    pad = MI.MARGIN_VOX * vs + 0.5 * vd * (1.0 - 1.0 / float(n))
    s = np.asarray(src_keys, np.int64).reshape(-1, 3).astype(np.float64)
    c = np.stack([(8.0 * s + 0.5) * vs, (8.0 * s + 8.5) * vs], 0)
    mn = np.full(s.shape, np.inf); mx = np.full(s.shape, -np.inf)
    for q in range(8):
        x = c[q & 1, :, 0]; y = c[(q >> 1) & 1, :, 1]; z = c[(q >> 2) & 1, :, 2]
        for a in range(3):
            v = R[a, 0] * x
            v = v + R[a, 1] * y
            v = v + R[a, 2] * z
            v = v + t[a]
            mn[:, a] = np.minimum(mn[:, a], v); mx[:, a] = np.maximum(mx[:, a], v)
    kl = np.ceil((mn - pad) / vd - 0.5).astype(np.int64); kh = np.floor((mx + pad) / vd - 0.5).astype(np.int64)
    return kl >> 3, kh >> 3


def candidates(T, src_keys, vs_s, vs_d, n):
    lo, hi = candidate_boxes(T, src_keys, vs_s, vs_d, n)
    out = set()
    for l, h in zip(lo, hi):
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    out.add((int(x), int(y), int(z)))
    return out


# ---------------------------------------------------------------------------------------------- taps
def tap_positions(T, blocks, vs_d, n, tap, dtype=F32):
    """p_S [m, 512, 3] of tap (ix, iy, iz) of every voxel of destination blocks [m, 3]: float32 as the semantics pin it, or the same
    expressions over the same float32 inputs evaluated in float64"""
    _, _, R, t = MI.transforms(T)
    R = R.astype(dtype); t = t.astype(dtype)
    off = tap_offsets(n).astype(dtype)
    g = (8 * np.asarray(blocks, np.int64).reshape(-1, 1, 3) + LANE_XYZ[None]).astype(dtype)
    o = np.array([off[tap[0]], off[tap[1]], off[tap[2]]], dtype)
    pd = ((g + dtype(0.5)) + o) * dtype(F32(vs_d))
    x, y, z = pd[..., 0], pd[..., 1], pd[..., 2]
    ps = np.empty_like(pd)
    for i in range(3):
        s = R[i, 0] * x
        s = s + R[i, 1] * y
        s = s + R[i, 2] * z
        ps[..., i] = s + t[i]
    return ps


def sample64(src_table, ps, ps64, vs_s, min_weight):
    """the float64 mode of one tap: the corners and the validity of the float32 rule, the interpolation parameter from the float64 position"""
    b, _, ok = MI.base_voxels(ps, vs_s)
    t = ps64 / float(F32(vs_s)) - 0.5 - b
    cd = np.zeros(ps.shape[:-1] + (8,), np.float64); cw = np.zeros(ps.shape[:-1] + (8,), np.float64)
    valid = ok.copy()
    for q in range(8):
        found, rec = src_table.gather(b + np.array([q & 1, (q >> 1) & 1, q >> 2], np.int64))
        valid &= found & (rec["weight"] >= F32(min_weight))
        cd[..., q] = rec["distance"]; cw[..., q] = rec["weight"]
    return valid, MI._trilinear(cd, t[..., 0], t[..., 1], t[..., 2]), MI._trilinear(cw, t[..., 0], t[..., 1], t[..., 2])


def tap_order(n):
    """x outer, y, z inner"""
    return [(ix, iy, iz) for ix in range(n) for iy in range(n) for iz in range(n)]


def reduce_taps(src_table, T, blocks, vs_s, vs_d, n, min_weight, dtype=F32):
    """-> (c int [m, 512], D, W): the number of valid taps and the sums of their distances and weights, in tap order from -0"""
    m = len(blocks)
    c = np.zeros((m, 512), np.int64)
    D = np.full((m, 512), -0.0, dtype); W = np.full((m, 512), -0.0, dtype)
    for tap in tap_order(n):
        ps = tap_positions(T, blocks, vs_d, n, tap)
        if dtype is F32:
            valid, d, w, _ = MI.sample(src_table, ps, vs_s, min_weight)
        else:
            valid, d, w = sample64(src_table, ps, tap_positions(T, blocks, vs_d, n, tap, np.float64), vs_s, min_weight)
        D = np.where(valid, D + d, D); W = np.where(valid, W + w, W)
        c += valid
    return c, D, W


def reach(T, blocks, vs_s, vs_d, n):
    """per destination block: the number of source blocks per axis from the lowest to the highest the corners of its taps lie in"""
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    lo = np.full((len(blocks), 3), np.iinfo(np.int64).max); hi = np.full((len(blocks), 3), np.iinfo(np.int64).min)
    for tap in tap_order(n):
        b, _, ok = MI.base_voxels(tap_positions(T, blocks, vs_d, n, tap), vs_s)
        lo = np.minimum(lo, np.where(ok[..., None], b >> 3, np.iinfo(np.int64).max).min(axis=1))
        hi = np.maximum(hi, np.where(ok[..., None], (b + 1) >> 3, np.iinfo(np.int64).min).max(axis=1))
    return hi - lo + 1


# ---------------------------------------------------------------------------------------------- the call
def resample(dst_tsdf, dst_color, src_tsdf, src_color, T, vs_s, vs_d, trunc, max_weight, min_weight=1e-4, weight_scale=1.0, merge_color=1, taps=0,
             blocks=None, dtype=F32):
    """-> dict as merge_independent.merge: tsdf / color (the destination afterwards), candidates, fused / colored / valid_taps per block, band
    and the result record's fields.  T None: the identity.  blocks: go over these destination blocks instead of the candidate set."""
    T = np.eye(4, dtype=F32) if T is None else np.asarray(T, F32).reshape(4, 4)
    r = ratio(vs_d, vs_s)
    n = taps_for(r, taps)
    assert ratio_ok(vs_d, vs_s) and n is not None, "refused by the library"
    out_t = {k: np.array(v, TSDF_DT).reshape(512) for k, v in dst_tsdf.items()}
    out_c = {k: np.array(v, COLOR_DT).reshape(512) for k, v in dst_color.items()}
    res = {"tsdf": out_t, "color": out_c, "fused": {}, "colored": {}, "valid_taps": {}, "band": {}, "source_blocks": len(src_tsdf), "candidates": [],
           "candidate_blocks": 0, "blocks_allocated": 0, "voxels_fused": 0, "color_voxels_fused": 0, "status": EMPTY_SOURCE, "taps": n}
    if not src_tsdf:
        return res
    cand = sorted(candidates(T, sorted(src_tsdf), vs_s, vs_d, n)) if blocks is None else sorted(tuple(int(q) for q in b) for b in blocks)
    res["candidates"] = cand; res["candidate_blocks"] = len(cand)
    res["blocks_allocated"] = sum(1 for k in cand if k not in dst_tsdf)
    st = MI._Table(src_tsdf, TSDF_DT); sc = MI._Table(src_color, COLOR_DT)
    trunc = F32(trunc); max_weight = F32(max_weight)
    carr = np.array(cand, np.int64).reshape(-1, 3)
    c, D, W = reduce_taps(st, T, carr, vs_s, vs_d, n, min_weight, dtype)
    n3 = n * n * n
    enough = 2 * c >= n3
    cur = np.stack([out_t[k] if k in out_t else np.zeros(512, TSDF_DT) for k in cand])
    dd = cur["distance"].astype(dtype); wd = cur["weight"].astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        ds = D / np.maximum(c, 1).astype(dtype)
        ws = W / dtype(n3) * dtype(F32(weight_scale))
        w = wd + ws
        fuse = enough & (w > 0)
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
        pc = MI.sample_positions(T, carr, vs_d)                            # the voxel's centre: the n = 1 tap
        with np.errstate(invalid="ignore", over="ignore"):
            nv = np.floor(pc / F32(vs_s))
        nv = np.where(np.isfinite(nv), nv, 0.0).astype(np.int64)
        found, rec = sc.gather(nv)
        has_tsdf, _ = st.gather(nv)                                        # the block carries both layers
        colored = fuse & found & has_tsdf & (rec["weight"] > 0)
        w0 = ccur["weight"]; w1 = rec["weight"]
        for ch in ("r", "g", "b"):
            cnew[ch] = np.where(colored, MI.blend_u8(ccur[ch].astype(F32), w0, rec[ch].astype(F32), w1), ccur[ch])
        cnew["pad"] = np.where(colored, 0, ccur["pad"])
        cnew["weight"] = np.where(colored, np.minimum(w0 + w1, max_weight), w0)
    for i, k in enumerate(cand):
        out_t[k] = new[i]
        res["fused"][k] = fuse[i]; res["colored"][k] = colored[i]; res["valid_taps"][k] = c[i]
        res["band"][k] = MI.band_bits(new[i], trunc)
        if k in out_c or colored[i].any():
            out_c[k] = cnew[i]
    res["voxels_fused"] = int(fuse.sum()); res["color_voxels_fused"] = int(colored.sum())
    res["status"] = OK if res["voxels_fused"] else NO_OVERLAP
    return res
