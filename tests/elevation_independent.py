"""An independent model of the elevation map and of traversability (SEMANTICS.md "Elevation and traversability") in numpy float32, in the
evaluation order the rules are written in: the voxel classes, the column rule and the interpolated height over a sparse block set; n_known,
step, the one- or two-sided gradients, the classes and the integer nearest-hazard search over a height / status image pair.  It imports
nothing from the product or the oracle.  Besides the model: the drawn maps and images the tests of both sides share."""
import numpy as np

F32 = np.float32
TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
UNKNOWN, SURFACE, BLOCKED, VOID = 0, 1, 2, 3                   # status
T_UNKNOWN, T_OK, T_HAZARD = 0, 1, 2                            # class
DEFAULTS = dict(max_step_m=0.10, max_slope_tan=0.5, unknown_value=1000.0, min_known=5, void_is_hazard=0, distance_radius_px=15)
VS = 0.05
MIN_WEIGHT = 1e-4


def options(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def read_tsdf(mapper, M):
    """{block: TSDF_DT[512]} of a Mapper, through block_indices / get_blocks: the blocks that carry the TSDF layer"""
    idx = mapper.block_indices(M.LAYER_TSDF)
    if not len(idx):
        return {}
    v, found = mapper.get_blocks(M.LAYER_TSDF, idx)
    assert found.all()
    return {tuple(int(q) for q in b): v[i].copy() for i, b in enumerate(idx)}


def elevation_box(aabb, z_min_m, z_max_m, voxel_size):
    vs = F32(voxel_size); a = np.asarray(aabb, F32)
    x0, y0 = int(np.rint(a[0] / vs)), int(np.rint(a[1] / vs))
    return (x0, y0, int(np.rint(a[4] / vs)) - y0, int(np.rint(a[3] / vs)) - x0, int(np.floor(F32(z_min_m) / vs)), int(np.floor(F32(z_max_m) / vs)))


def elevation(tsdf, box, min_weight=MIN_WEIGHT, unknown_value=1000.0, voxel_size=VS):
    """tsdf {block: TSDF_DT[512]}, voxel t = vx 64 + vy 8 + vz; box = (x0, y0, rows, cols, z_lo, z_hi) -> (height f32, status u8) [rows, cols].
    One block column at a time: the band's voxels of its 64 columns as [z, x, y] stacks, then the column rule on all 64."""
    x0, y0, rows, cols, z_lo, z_hi = (int(v) for v in box)
    vs = F32(voxel_size); bs = vs * F32(8.0); mw = F32(min_weight)
    height = np.full((rows, cols), F32(unknown_value), F32)
    status = np.zeros((rows, cols), np.uint8)
    n = z_hi - z_lo + 1
    for by in range(y0 >> 3, ((y0 + rows - 1) >> 3) + 1):
        for bx in range(x0 >> 3, ((x0 + cols - 1) >> 3) + 1):
            D = np.zeros((n, 8, 8), F32); O = np.zeros((n, 8, 8), bool)
            for bz in range(z_lo >> 3, (z_hi >> 3) + 1):
                blk = tsdf.get((bx, by, bz))
                if blk is None:
                    continue                                                       # not allocated, or without the TSDF layer: unobserved
                d = blk["distance"].reshape(8, 8, 8); w = blk["weight"].reshape(8, 8, 8)
                for vz in range(8):
                    gz = 8 * bz + vz
                    if z_lo <= gz <= z_hi:
                        D[gz - z_lo] = d[:, :, vz]
                        with np.errstate(invalid="ignore"):
                            O[gz - z_lo] = (w[:, :, vz] >= mw) & (d[:, :, vz] == d[:, :, vz])
            with np.errstate(invalid="ignore"):
                solid = O & (D <= F32(0.0))
            for vx in range(8):
                for vy in range(8):
                    r, c = 8 * by + vy - y0, 8 * bx + vx - x0
                    if not (0 <= r < rows and 0 <= c < cols):
                        continue
                    if not O[:, vx, vy].any():
                        status[r, c] = UNKNOWN
                    elif not solid[:, vx, vy].any():
                        status[r, c] = VOID
                    else:
                        k = int(np.flatnonzero(solid[:, vx, vy])[-1])              # zt = z_lo + k
                        if k + 1 < n and O[k + 1, vx, vy]:
                            zt = z_lo + k
                            d0, d1 = D[k, vx, vy], D[k + 1, vx, vy]
                            centre = (F32(zt >> 3) * bs + F32(zt & 7) * vs) + vs * F32(0.5)
                            with np.errstate(all="ignore"):
                                height[r, c] = centre + vs * ((-d0) / (d1 - d0))
                            status[r, c] = SURFACE
                        else:
                            status[r, c] = BLOCKED
    return height, status


def _grad(km, kp, hm, h, hp, vs):
    with np.errstate(all="ignore"):
        if km and kp:
            return (hp - hm) / (F32(2.0) * vs)
        if kp:
            return (hp - h) / vs
        if km:
            return (h - hm) / vs
    return F32(0.0)


def stencil(height, status, voxel_size=VS):
    """-> (n_known int [rows, cols], step f32, slope2 f32): plain loops over the pixels"""
    h = np.asarray(height, F32); known = np.asarray(status) == SURFACE
    rows, cols = h.shape
    vs = F32(voxel_size)
    nk = np.zeros((rows, cols), np.int32); step = np.zeros((rows, cols), F32); slope2 = np.zeros((rows, cols), F32)

    def kn(r, c):
        return 0 <= r < rows and 0 <= c < cols and bool(known[r, c])
    for r in range(rows):
        for c in range(cols):
            if not known[r, c]:
                continue
            n = 0; s = F32(0.0)
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    if kn(r + dr, c + dc):
                        n += 1
                        if dr or dc:
                            with np.errstate(all="ignore"):
                                v = np.abs(h[r, c] - h[r + dr, c + dc])
                            if v > s:
                                s = v
            nk[r, c] = n; step[r, c] = s
            gx = _grad(kn(r, c - 1), kn(r, c + 1), h[r, c - 1] if c > 0 else F32(0), h[r, c], h[r, c + 1] if c + 1 < cols else F32(0), vs)
            gy = _grad(kn(r - 1, c), kn(r + 1, c), h[r - 1, c] if r > 0 else F32(0), h[r, c], h[r + 1, c] if r + 1 < rows else F32(0), vs)
            with np.errstate(all="ignore"):
                slope2[r, c] = F32(gx * gx) + F32(gy * gy)
    return nk, step, slope2


def classes(status, nk, step, slope2, o):
    status = np.asarray(status)
    known = status == SURFACE
    with np.errstate(invalid="ignore"):
        lim = F32(o["max_slope_tan"]) * F32(o["max_slope_tan"])
        bad = ~(step <= F32(o["max_step_m"])) | ~(slope2 <= lim) | (nk < int(o["min_known"]))
    cls = np.full(status.shape, T_UNKNOWN, np.uint8)
    cls[known] = T_OK
    cls[known & bad] = T_HAZARD
    cls[status == BLOCKED] = T_HAZARD
    if o["void_is_hazard"]:
        cls[status == VOID] = T_HAZARD
    return cls


def distance(cls, o, voxel_size=VS):
    """the integer minimum over every offset of the disc, then one correctly rounded float32 square root"""
    R = int(o["distance_radius_px"]); vs = F32(voxel_size)
    rows, cols = cls.shape
    haz = np.zeros((rows + 2 * R, cols + 2 * R), bool)
    haz[R:R + rows, R:R + cols] = cls == T_HAZARD
    none = R * R + 1
    m = np.full((rows, cols), none, np.int64)
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            s = dr * dr + dc * dc
            if s <= R * R:
                m = np.where(haz[R + dr:R + dr + rows, R + dc:R + dc + cols], np.minimum(m, s), m)
    out = np.where(m < none, vs * np.sqrt(m.astype(F32)), vs * F32(R + 1)).astype(F32)
    out[cls == T_HAZARD] = F32(0.0)
    out[cls == T_UNKNOWN] = F32(o["unknown_value"])
    return out, m


def traversability(height, status, voxel_size=VS, **kw):
    o = options(**kw)
    nk, step, slope2 = stencil(height, status, voxel_size)
    cls = classes(status, nk, step, slope2, o)
    dist, m = distance(cls, o, voxel_size)
    return {"class": cls, "step": step, "slope2": slope2, "distance": dist, "n_known": nk, "m": m}


# ---------------------------------------------------------------------------------------------- drawn maps
def block(distance, weight=1.0):
    """one block from [x, y, z] arrays (or scalars) of distance and weight"""
    b = np.zeros(512, TSDF_DT)
    b["distance"] = np.broadcast_to(np.asarray(distance, F32), (8, 8, 8)).reshape(512)
    b["weight"] = np.broadcast_to(np.asarray(weight, F32), (8, 8, 8)).reshape(512)
    return b


def heightfield_blocks(hfun, bx_range, by_range, bz_range, voxel_size=VS, weight=1.0):
    """{block: voxels} with d = voxel centre z - hfun(x, y) of the column's centre (float64, rounded once to float32)"""
    out = {}
    v = (np.arange(8) + 0.5) * voxel_size
    for bx in bx_range:
        for by in by_range:
            X, Y = np.meshgrid(bx * 8 * voxel_size + v, by * 8 * voxel_size + v, indexing="ij")
            H = hfun(X, Y)
            for bz in bz_range:
                zc = bz * 8 * voxel_size + v
                out[(bx, by, bz)] = block((zc[None, None, :] - H[:, :, None]).astype(F32), weight)
    return out


def upload(mapper, M, tsdf):
    ks = sorted(tsdf)
    if ks:
        mapper.set_blocks(M.LAYER_TSDF, np.array(ks, np.int32), np.stack([tsdf[k] for k in ks]))


def drawn_map(seed, min_weight=MIN_WEIGHT):
    """a 6 x 6 x 4 block box, blocks present with p = 0.6, d uniform in +- 0.2, weights drawn from {0, min_weight, 1}"""
    rng = np.random.default_rng(seed)
    out = {}
    for bx in range(-3, 3):
        for by in range(-2, 4):
            for bz in range(-1, 3):
                if rng.random() < 0.6:
                    d = rng.uniform(-0.2, 0.2, (8, 8, 8)).astype(F32)
                    w = rng.choice(np.array([0.0, min_weight, 1.0], F32), (8, 8, 8))
                    out[(bx, by, bz)] = block(d, w)
    return out
DRAWN_BOX = (-24 - 3, -16 - 2, 48 + 5, 48 + 6, -6, 21)      # the drawn box and a rim of unallocated columns around it; the band cuts blocks at both ends


# the kerb scene: floor at 0.30 m for x < 1.6 m, a platform 0.15 m higher beyond, joined by a ramp three pixels wide (rows 8 .. 10) that climbs
# over the ten columns 22 .. 31; everywhere else the kerb is a step of 0.15 m between columns 31 and 32
KERB_ROWS, KERB_COLS, KERB_RAMP_ROWS, KERB_RAMP_COLS = 32, 48, (8, 9, 10), tuple(range(22, 32))
KERB_BOX = (0, 0, KERB_ROWS, KERB_COLS, 0, 15)
KERB_FIELD = dict(robot_radius_m=0.05, inflation_radius_m=0.3)


def kerb_height(X, Y, voxel_size=VS):
    c = np.floor(X / voxel_size + 1e-9).astype(int); r = np.floor(Y / voxel_size + 1e-9).astype(int)
    h = np.where(c >= 32, 0.45, 0.30)
    on_ramp = (r >= 8) & (r <= 10) & (c >= 22) & (c < 32)
    return np.where(on_ramp, 0.30 + 0.15 * (c - 21) / 11.0, h)


def kerb_blocks():
    return heightfield_blocks(kerb_height, range(0, 6), range(0, 4), range(0, 2))


# ---------------------------------------------------------------------------------------------- drawn images
def random_image(shape, seed):
    """a height / status pair with every status, heights near 1 m with steps and slopes around the default limits"""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    r, c = np.mgrid[0:rows, 0:cols]
    h = (1.0 + 0.02 * c * (rng.random() < 0.5) + 0.012 * r + 0.03 * rng.standard_normal(shape) * (rng.random(shape) < 0.3)).astype(F32)
    st = rng.choice(np.array([UNKNOWN, SURFACE, BLOCKED, VOID], np.uint8), shape, p=[0.06, 0.86, 0.04, 0.04])
    h[st != SURFACE] = F32(1000.0)
    return h, st


def flat_image(shape, h=1.0):
    return np.full(shape, F32(h), F32), np.full(shape, SURFACE, np.uint8)


IMAGE_SHAPES = ((1, 1), (3, 3), (63, 65), (64, 64), (65, 130))      # the word edges of a 64-bit row mask
