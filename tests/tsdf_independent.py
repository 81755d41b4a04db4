"""Independent float64 model of the projective TSDF update (UpdateTsdfVoxelFunctor as DESIGN.md 3 / SEMANTICS.md restate it): numpy only, whole arrays,
no code shared with the product or with oracle/nvblox_oracle.c.  Per voxel centre of a block: layer -> camera frame, pinhole projection, bilinear
depth with validity (all four taps in (0, +inf): NaN, <= 0 and both infinities are invalid), sdf = measured depth - voxel depth, the weighting
function (six modes, two formula sets), weighted blend, clamps.  Returns the expected {distance, weight} and a per-voxel "robust" mask: voxels whose
DECISIONS (in the image, taps valid, sdf >= -trunc, clamps) do not hang on the last bits of a float32 evaluation.

update_block_rules is the whole rule set in one place -- bilinear or nearest-pixel sampling, the two fuse switches, invalid-depth decay, the occupancy
update -- and reports per voxel which rule decided (RULES); voxels named `exact` are robust whatever the margins say (tests/depth_cases.py draws
frames on which a float32 evaluation of those voxels is exact)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
RULES = ("untouched-outside", "invalid-tap", "rejected-behind", "fused")
OUTSIDE, INVALID, REJECTED, FUSED = range(4)


def tap_valid(d):
    """a depth tap counts iff 0 < d < +inf"""
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.inf)


def weight_fn(mode, variant, ds, vd, trunc, vs, max_dist):
    w = np.ones_like(ds)
    if mode in (2, 3, 4):
        with np.errstate(over="ignore", divide="ignore"):
            w = 1.0 / (ds * ds)
            w = np.where(ds * ds > FLT_MAX, 0.0, np.where(w > FLT_MAX, np.inf, w))      # (float32's range: a square beyond it is +inf and its reciprocal 0; a reciprocal beyond it is +inf)
    elif mode == 5:
        w = np.minimum(1.0, 1.0 / ds) if variant == 0 else np.maximum(0.01, 1.0 - ds / max_dist)
    sdf = ds - vd
    if mode in (1, 3):
        if variant == 0:
            g = np.clip((trunc + sdf) / trunc, 0.0, None)
            w = np.where(sdf < 0.0, w * g, w)
        else:
            g = np.clip((trunc + sdf) / (trunc - vs), 0.0, None) if trunc > vs else np.zeros_like(sdf)
            w = np.where(sdf < -vs, w * g, w)
    elif mode == 4:
        if variant == 0:
            w = np.where(sdf > trunc, w * (trunc / np.where(sdf > trunc, sdf, 1.0)), w)
        else:
            g = np.clip((trunc + sdf) / trunc, 0.0, None)
            w = np.where(sdf < 0.0, w * g * g, w)
    return w


def update_block(prev_d, prev_w, block_index, depth, T_L_C, cam, p, margin=2e-4):
    """prev_d / prev_w: [512] float64 in voxel order z + 8 y + 64 x; depth [rows, cols]; T_L_C 4x4; cam (fu, fv, cu, cv, w, h); p: the parameter struct."""
    fu, fv, cu, cv, w, h = cam
    vs = float(p.voxel_size); bs = 8.0 * vs; trunc = float(p.truncation_distance_vox) * vs
    max_dist = float(p.max_integration_distance_m); max_w = float(p.max_weight)
    rows, cols = depth.shape
    lin = np.arange(512); vx, vy, vz = lin // 64, (lin // 8) % 8, lin % 8
    pl = np.stack([block_index[0] * bs + vx * vs + vs / 2, block_index[1] * bs + vy * vs + vs / 2, block_index[2] * bs + vz * vs + vs / 2], 1)
    T = np.asarray(T_L_C, np.float64); R = T[:3, :3]; t = T[:3, 3]
    pc = (pl - t) @ R                                   # R^T (p - t)
    z = pc[:, 2]
    zs = np.where(z > 0, z, 1.0)
    u = fu * pc[:, 0] / zs + cu; v = fv * pc[:, 1] / zs + cv
    in_img = (z > 0) & (u >= 0) & (v >= 0) & (u <= w) & (v <= h)
    in_rng = ~(max_dist > 0) | (z <= max_dist)
    uc, vc = u - 0.5, v - 0.5
    x0 = np.floor(uc).astype(np.int64); y0 = np.floor(vc).astype(np.int64)
    in_taps = (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= cols - 1) & (y0 + 1 <= rows - 1)
    xs = np.clip(x0, 0, cols - 2); ys = np.clip(y0, 0, rows - 2)
    d = depth.astype(np.float64)
    f00, f10, f01, f11 = d[ys, xs], d[ys, xs + 1], d[ys + 1, xs], d[ys + 1, xs + 1]
    taps_ok = tap_valid(f00) & tap_valid(f10) & tap_valid(f01) & tap_valid(f11)
    ax, ay = uc - np.floor(uc), vc - np.floor(vc)
    ds = (1 - ay) * ((1 - ax) * f00 + ax * f10) + ay * ((1 - ax) * f01 + ax * f11)
    sdf = ds - z
    upd = in_img & in_rng & in_taps & taps_ok & (sdf >= -trunc)
    ds_s = np.where(upd, ds, 1.0)
    wm = weight_fn(int(p.weighting_mode), int(p.tsdf_weighting_variant), ds_s, np.where(upd, z, 0.0), trunc, vs, max_dist)
    wsum = wm + prev_w
    upd = upd & (wsum > 0)
    fused = np.clip((np.where(upd, sdf, 0.0) * wm + prev_d * prev_w) / np.where(wsum > 0, wsum, 1.0), -trunc, trunc)
    out_d = np.where(upd, fused, prev_d); out_w = np.where(upd, np.minimum(wsum, max_w), prev_w)
    # decisions that hang on the last bits: close to the image border / a tap boundary / the range limit / sdf == -trunc / depth edges (taps that differ much make ds sensitive)
    spread = np.maximum.reduce([f00, f10, f01, f11]) - np.minimum.reduce([f00, f10, f01, f11])
    robust = ((np.abs(z) > 1e-3) & (np.minimum.reduce([np.abs(u), np.abs(v), np.abs(u - w), np.abs(v - h)]) > margin * 50) &
              (np.minimum(np.abs(uc - np.round(uc)), np.abs(vc - np.round(vc))) > margin * 50) & (np.abs(z - max_dist) > margin) &
              (np.abs(sdf + trunc) > margin) & (spread < 0.5))
    return out_d, out_w, upd, robust


def project_and_sample(block_index, depth, T_L_C, cam, vs, max_dist):
    """shared geometry of the update rules below: voxel depth z, measured depth ds, masks (in view & range, four valid taps, some tap invalid), robustness inputs"""
    fu, fv, cu, cv, w, h = cam
    bs = 8.0 * vs
    rows, cols = depth.shape
    lin = np.arange(512); vx, vy, vz = lin // 64, (lin // 8) % 8, lin % 8
    pl = np.stack([block_index[0] * bs + vx * vs + vs / 2, block_index[1] * bs + vy * vs + vs / 2, block_index[2] * bs + vz * vs + vs / 2], 1)
    T = np.asarray(T_L_C, np.float64); pc = (pl - T[:3, 3]) @ T[:3, :3]
    z = pc[:, 2]; zs = np.where(z > 0, z, 1.0)
    u = fu * pc[:, 0] / zs + cu; v = fv * pc[:, 1] / zs + cv
    seen = (z > 0) & (u >= 0) & (v >= 0) & (u <= w) & (v <= h) & (~(max_dist > 0) | (z <= max_dist))
    uc, vc = u - 0.5, v - 0.5
    x0 = np.floor(uc).astype(np.int64); y0 = np.floor(vc).astype(np.int64)
    in_taps = (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= cols - 1) & (y0 + 1 <= rows - 1)
    xs = np.clip(x0, 0, cols - 2); ys = np.clip(y0, 0, rows - 2)
    d = depth.astype(np.float64)
    f00, f10, f01, f11 = d[ys, xs], d[ys, xs + 1], d[ys + 1, xs], d[ys + 1, xs + 1]
    valid = tap_valid(f00) & tap_valid(f10) & tap_valid(f01) & tap_valid(f11)
    ax, ay = uc - np.floor(uc), vc - np.floor(vc)
    ds = (1 - ay) * ((1 - ax) * f00 + ax * f10) + ay * ((1 - ax) * f01 + ax * f11)
    spread = np.maximum.reduce([f00, f10, f01, f11]) - np.minimum.reduce([f00, f10, f01, f11])
    near_edge = ((np.abs(z) < 1e-3) | (np.minimum.reduce([np.abs(u), np.abs(v), np.abs(u - w), np.abs(v - h)]) < 0.01) |
                 (np.minimum(np.abs(uc - np.round(uc)), np.abs(vc - np.round(vc))) < 0.01) | (np.abs(z - max_dist) < 2e-4))
    return z, ds, seen & in_taps & valid, seen & in_taps & ~valid, spread, near_edge


def update_block_occupancy(prev_lo, block_index, depth, T_L_C, cam, p):
    """ProjectiveOccupancyIntegrator as restated: a voxel in front of the measured surface by more than the half width adds logit(free), within +- the half
    width logit(occupied), behind it logit(unobserved); clamp +-10.  -> (log-odds [512], robust mask)"""
    lo = lambda q: np.log(np.float32(q) / (np.float32(1.0) - np.float32(q)))
    hw = float(p.occupied_region_half_width_m)
    z, ds, got, _, spread, near_edge = project_and_sample(block_index, depth, T_L_C, cam, float(p.voxel_size), float(p.max_integration_distance_m))
    upd = np.where(z < ds - hw, lo(p.free_region_occupancy_probability), np.where(z <= ds + hw, lo(p.occupied_region_occupancy_probability), lo(p.unobserved_region_occupancy_probability)))
    out = np.where(got, np.clip(prev_lo + upd, -10.0, 10.0), prev_lo)
    robust = ~near_edge & (np.abs(z - (ds - hw)) > 2e-4) & (np.abs(z - (ds + hw)) > 2e-4) & (spread < 0.5)
    return out, robust


def update_block_invalid_decay(prev_d, prev_w, block_index, depth, T_L_C, cam, p):
    """[U] invalid-depth decay: a voxel that projects into the image onto an invalid (<= 0) depth tap has its weight multiplied by the factor (and is not
    integrated); everything else as update_block"""
    nd, nw, upd, rob = update_block(prev_d, prev_w, block_index, depth, T_L_C, cam, p)
    z, ds, got, bad, spread, near_edge = project_and_sample(block_index, depth, T_L_C, cam, float(p.voxel_size), float(p.max_integration_distance_m))
    nw = np.where(bad, prev_w * float(p.invalid_depth_decay_factor), nw); nd = np.where(bad, prev_d, nd)
    return nd, nw, rob & ~near_edge


def voxel_geometry(block_index, T_L_C, cam, vs):
    """camera-frame centres [512, 3] of a block's voxels (order z + 8 y + 64 x) and their pixel coordinates (u, v); (u, v) of a voxel at depth <= 0 are those of depth 1"""
    fu, fv, cu, cv = cam[:4]
    bs = 8.0 * vs
    lin = np.arange(512); vx, vy, vz = lin // 64, (lin // 8) % 8, lin % 8
    pl = np.stack([block_index[0] * bs + vx * vs + vs / 2, block_index[1] * bs + vy * vs + vs / 2, block_index[2] * bs + vz * vs + vs / 2], 1)
    T = np.asarray(T_L_C, np.float64); pc = (pl - T[:3, 3]) @ T[:3, :3]
    zs = np.where(pc[:, 2] > 0, pc[:, 2], 1.0)
    return pc, fu * pc[:, 0] / zs + cu, fv * pc[:, 1] / zs + cv


def sample_depth(depth, u, v, nearest):
    """-> (inside the tap range, the taps read [4, n] (nearest: the pixel four times), the measured depth where every tap is finite, distance in pixels to the next change of taps)"""
    rows, cols = depth.shape
    d = depth.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if nearest:
            c = np.floor(u).astype(np.int64); r = np.floor(v).astype(np.int64)
            inside = (c >= 0) & (r >= 0) & (c < cols) & (r < rows)
            f = d[np.clip(r, 0, rows - 1), np.clip(c, 0, cols - 1)]
            return inside, np.stack([f, f, f, f]), f, np.minimum(np.abs(u - np.round(u)), np.abs(v - np.round(v)))
        uc, vc = u - 0.5, v - 0.5
        x0 = np.floor(uc).astype(np.int64); y0 = np.floor(vc).astype(np.int64)
        inside = (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= cols - 1) & (y0 + 1 <= rows - 1)
        xs = np.clip(x0, 0, max(cols - 2, 0)); ys = np.clip(y0, 0, max(rows - 2, 0))
        x1 = np.minimum(xs + 1, cols - 1); y1 = np.minimum(ys + 1, rows - 1)
        taps = np.stack([d[ys, xs], d[ys, x1], d[y1, xs], d[y1, x1]])
        ax, ay = uc - np.floor(uc), vc - np.floor(vc)
        ds = (1 - ay) * ((1 - ax) * taps[0] + ax * taps[1]) + ay * ((1 - ax) * taps[2] + ax * taps[3])
        return inside, taps, ds, np.minimum(np.abs(uc - np.round(uc)), np.abs(vc - np.round(vc)))


def update_block_rules(prev_d, prev_w, block_index, depth, T_L_C, cam, p, exact=None, margin=2e-4):
    """One camera frame onto one block, every rule of the projective update: -> (distance [512], weight [512], rule [512] (RULES), robust [512]).
    An occupancy mapper (projective_layer_type 1) holds its log-odds in `distance`, weight stays as it is.  exact: bool [512], voxels that count as
    robust without margins."""
    w, h = cam[4], cam[5]
    vs = float(p.voxel_size); trunc = float(p.truncation_distance_vox) * vs
    max_dist = float(p.max_integration_distance_m); max_w = float(p.max_weight)
    pc, u, v = voxel_geometry(block_index, T_L_C, cam, vs)
    z = pc[:, 2]
    seen = (z > 0) & (u >= 0) & (v >= 0) & (u <= w) & (v <= h) & ((z <= max_dist) if max_dist > 0 else True)
    inside, taps, ds, tap_edge = sample_depth(np.asarray(depth), u, v, int(p.depth_interp_nearest))
    valid = tap_valid(taps).all(0)
    got = seen & inside & valid; bad = seen & inside & ~valid
    ds = np.where(got, ds, 1.0); zz = np.where(got, z, 0.0)
    sdf = ds - zz
    rule = np.where(got, FUSED, np.where(bad, INVALID, OUTSIDE))
    prev_d = np.asarray(prev_d, np.float64); prev_w = np.asarray(prev_w, np.float64)
    with np.errstate(all="ignore"):
        spread = np.where(valid, taps.max(0) - taps.min(0), 0.0)       # (an invalid tap decides whatever its weight: only a change of taps matters there)
    robust = ((np.abs(z) > 1e-3) & (np.minimum.reduce([np.abs(u), np.abs(v), np.abs(u - w), np.abs(v - h)]) > margin * 50) & (tap_edge > margin * 50) &
              (np.abs(z - max_dist) > margin) & (spread < 0.5))
    if int(p.projective_layer_type) == 1:
        lo = lambda q: float(np.log(np.float32(q) / (np.float32(1.0) - np.float32(q))))
        hw = float(p.occupied_region_half_width_m)
        step = np.where(zz < ds - hw, lo(p.free_region_occupancy_probability),
                        np.where(zz <= ds + hw, lo(p.occupied_region_occupancy_probability), lo(p.unobserved_region_occupancy_probability)))
        out_d = np.where(got, np.clip(prev_d + step, -10.0, 10.0), prev_d); out_w = prev_w.copy()
        robust &= ~got | ((np.abs(zz - (ds - hw)) > margin) & (np.abs(zz - (ds + hw)) > margin))
    else:
        rejected = (sdf <= -trunc) if int(p.tsdf_skip_at_negative_truncation) else (sdf < -trunc)
        wm = weight_fn(int(p.weighting_mode), int(p.tsdf_weighting_variant), ds, zz, trunc, vs, max_dist)
        wsum = wm + prev_w
        with np.errstate(invalid="ignore"):
            fuse = got & ~rejected & (wsum > 0) & (wsum < np.inf)          # (a measurement of infinite weight is none)
        wnew = np.minimum(wsum, max_w)
        with np.errstate(all="ignore"):
            if not int(p.tsdf_weight_clamp_before_blend):
                blend = (sdf * wm + prev_d * prev_w) / np.where(fuse, wsum, 1.0)
            else:
                wp = np.maximum(wnew - wm, 0.0)
                blend = (sdf * wm + prev_d * wp) / np.where(fuse, wm + wp, 1.0)
        out_d = np.where(fuse, np.clip(np.where(fuse, blend, 0.0), -trunc, trunc), prev_d); out_w = np.where(fuse, wnew, prev_w)
        rule = np.where(got & ~fuse, REJECTED, rule)
        decay = float(p.invalid_depth_decay_factor)
        if decay >= 0.0:
            out_w = np.where(bad, prev_w * decay, out_w)
        robust &= ~got | (np.abs(sdf + trunc) > margin)
    if exact is not None:
        robust = robust | np.asarray(exact, bool)
    if int(p.projective_layer_type) != 1:
        # a depth below 1e-15 m under inverse-square weighting: the weight 1 / d^2 leaves float32's range (d^2 underflows), nothing to compare
        robust = robust & ~(got & (wm > 1e30) & (wm < np.inf))
    return out_d, out_w, rule, robust
