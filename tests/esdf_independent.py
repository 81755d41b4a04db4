"""The ESDF on DRAWN site sets: the truth it is judged by, the block writer that puts exactly a drawn site set into a map, and the catalogue
of patterns drawn to break the distance transforms (csrc/nvbx_esdf_edt.h, csrc/esdf.hip, csrc/esdf3d.hip).  Plain numpy, integer arithmetic;
nothing here imports the project or its checker (tests/test_esdf_model.py validates it on the CPU against scipy and the checker).

THE DEFINITION (SEMANTICS.md "ESDF 2-D", "Limits of the cut-off radius").  r = float32(esdf_max_distance_m) / float32(voxel_size),
max_sq = float32(r * r), ri = max(1, floor(r)).  A site at integer offset d from a voxel counts iff float32(|d|^2) <= max_sq and every
|d_axis| <= ri; the voxel's value is the minimum |d|^2 over the sites that count, as float32, or max_sq if none does.  For r < 1 only the
sites themselves have a distance (0): ri is 1 but max_sq is below 1.

THE MARKING RULE (SEMANTICS.md "ESDF 2-D", "Ground-plane-relative slice"), by which a TSDF or occupancy read-back says what the site set is:
voxel_marks (each voxel by itself), column_bands / column_marks_2d (the column rule over the z band, fixed or per column over a ground plane),
volume_marks_3d, block_band / esdf_blocks_expected (which ESDF blocks an update creates); tests/test_esdf_mark_model.py validates these against
the checker on the drawn cases of tests/esdf_mark_cases.py.

ARRAYS.  2-D fields are [y, x] (row = y, like the slice image), 3-D fields [x, y, z] (like a block's voxels); parents are stored in the
ARRAY's axis order ((dy, dx) resp. (dx, dy, dz)), so that position + parent indexes the same array.
"""
import collections

import numpy as np

TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
_BIG = np.int32(1 << 30)

# ------------------------------------------------------------------------------------------------ the radius


def radius_of(esdf_max_distance_m, voxel_size):
    """(r, max_sq, ri) as the product derives them from its two float32 parameters."""
    r = np.float32(esdf_max_distance_m) / np.float32(voxel_size)
    return r, np.float32(r * r), max(1, int(np.floor(r)))


def cutoff(r):
    """(max_sq, ri) of a radius in voxels that is already the float32 quotient."""
    r = np.float32(r)
    return np.float32(r * r), max(1, int(np.floor(r)))


def radius_blocks(r):
    """rb: blocks a site can reach across (ceil(ri / 8))."""
    return (min(cutoff(r)[1], 63) + 7) // 8


def distance_for_radius(r_nominal, voxel_size):
    """The float32 esdf_max_distance_m a caller would write for `r_nominal` voxels: float32(r * voxel_size).  Its quotient by the voxel size
    need not be r_nominal again (0.35 / 0.05 is below 7 in float32): the tests take whatever comes out, through radius_of."""
    return float(np.float32(float(r_nominal) * float(voxel_size)))


def distance_below_radius(limit, voxel_size):
    """The largest float32 distance whose quotient by the voxel size is below `limit` voxels."""
    vs = np.float32(voxel_size)
    d = np.float32(float(limit) * float(voxel_size))
    while d / vs < np.float32(limit):
        d = np.nextafter(d, np.float32(np.inf))
    while not d / vs < np.float32(limit):
        d = np.nextafter(d, np.float32(-np.inf))
    return float(d)


def distance_at_least_radius(limit, voxel_size):
    """The smallest float32 distance whose quotient by the voxel size is >= `limit` voxels."""
    return float(np.nextafter(np.float32(distance_below_radius(limit, voxel_size)), np.float32(np.inf)))

# ------------------------------------------------------------------------------------------------ the truth


def edt_bruteforce(sites, where, r, budget=4_000_000):
    """(sq float32, count int32), shaped like `sites` (2-D or 3-D boolean): for every voxel of `where` the minimum squared integer distance
    to a site that counts (see THE DEFINITION) and how many sites attain it; max_sq and 0 where none counts (and outside `where`).
    Chunked over the sites: no temporary holds more than `budget` elements."""
    sites = np.asarray(sites, bool); where = np.asarray(where, bool)
    assert sites.shape == where.shape and sites.ndim in (2, 3)
    max_sq, ri = cutoff(r)
    sq = np.full(sites.shape, max_sq, np.float32); cnt = np.zeros(sites.shape, np.int32)
    q = np.argwhere(where).astype(np.int32); p = np.argwhere(sites).astype(np.int32)
    if len(q) == 0 or len(p) == 0:
        return sq, cnt
    best = np.full(len(q), _BIG, np.int32); n = np.zeros(len(q), np.int32)
    step = max(1, budget // len(q))
    for s0 in range(0, len(p), step):
        pc = p[s0:s0 + step]
        d2 = np.zeros((len(q), len(pc)), np.int32); ok = np.ones((len(q), len(pc)), bool)
        for a in range(sites.ndim):
            d = pc[None, :, a] - q[:, None, a]
            ok &= np.abs(d) <= ri
            d2 += d * d
        ok &= d2.astype(np.float32) <= max_sq
        d2[~ok] = _BIG
        m = d2.min(1)
        c = (d2 == m[:, None]).sum(1).astype(np.int32)
        n = np.where(m < best, c, np.where((m == best) & (m < _BIG), n + c, n))
        best = np.minimum(best, m)
    hit = best < _BIG
    sq[tuple(q.T)] = np.where(hit, best.astype(np.float32), max_sq)
    cnt[tuple(q.T)] = np.where(hit, n, 0)
    return sq, cnt


def check_parents(sites, sq, parent, where, r):
    """Independent of any tie rule.  For every voxel of `where`: if sq < max_sq, position + parent is a site, |parent|^2 == sq and every
    |component| <= ri.  If sq == max_sq the parent is zero -- or, where a site lies at EXACTLY the cut-off (max_sq is an integer: r = 40, a
    site 40 voxels away), such a parent of squared length max_sq.  (edt_bruteforce's count tells the two apart: the tests assert
    parent != 0 exactly where count > 0.)  Raises AssertionError naming the first offenders."""
    sites = np.asarray(sites, bool); where = np.asarray(where, bool)
    max_sq, ri = cutoff(r)
    q = np.argwhere(where)
    s = np.asarray(sq)[tuple(q.T)]; p = np.asarray(parent)[tuple(q.T)].astype(np.int64)
    assert p.shape == (len(q), sites.ndim)
    assert not (s > max_sq).any() and not (s < 0).any(), "squared distance outside [0, max_sq]"
    nonzero = (p != 0).any(1)
    must = (s < max_sq) | nonzero                      # these carry a parent that has to be a valid one
    bad_zero = (s < max_sq) & ~nonzero & (s != 0)
    assert not bad_zero.any(), ("distance below the cut-off without a parent", q[bad_zero][:5].tolist())
    t = q + p
    inside = ((t >= 0) & (t < np.array(sites.shape))).all(1)
    assert inside[must].all(), ("parent points outside the field", q[must & ~inside][:5].tolist())
    tc = np.where(inside[:, None], t, 0)
    is_site = sites[tuple(tc.T)] & inside
    len2 = (p * p).sum(1)
    bad = must & (~is_site | (len2.astype(np.float32) != s) | (np.abs(p) > ri).any(1))
    assert not bad.any(), ("parent is not a site at the stored distance within ri", q[bad][:5].tolist(), p[bad][:5].tolist(), s[bad][:5].tolist())
    own = sites[tuple(q.T)]
    assert ((s == 0) == own).all(), "distance 0 exactly on the sites"
    return int(must.sum())


def numpy_propagation(sites, dom, max_sq):
    """Independent restatement (numpy, whole-array) of esdf_propagation = 1: synchronous 4-neighbour parent propagation, key
    (sq, dy, dx), cut-off max_sq, restricted to `dom`.  Returns sq (float, max_sq where no site is known)."""
    H_, W_ = sites.shape
    NONE = np.int64(2 ** 31 - 1)
    cur = np.where(sites, np.int64((64 << 7) | 64), NONE)
    for _ in range(4096):
        best = cur.copy()
        for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            nb = np.full_like(cur, NONE)
            # neighbour at (x + ox, y + oy)
            ys = slice(max(0, -oy), H_ - max(0, oy)); xs = slice(max(0, -ox), W_ - max(0, ox))
            ysn = slice(max(0, oy), H_ - max(0, -oy)); xsn = slice(max(0, ox), W_ - max(0, -ox))
            nb[ys, xs] = np.where(dom[ysn, xsn], cur[ysn, xsn], NONE)
            dx = (nb & 127) - 64 + ox; dy = ((nb >> 7) & 127) - 64 + oy
            sq = dx * dx + dy * dy
            ok = (nb != NONE) & (sq.astype(np.float32) <= np.float32(max_sq)) & (np.abs(dx) <= 63) & (np.abs(dy) <= 63)
            cand = np.where(ok, (sq << 14) | ((dy + 64) << 7) | (dx + 64), NONE)
            best = np.minimum(best, cand)
        best = np.where(dom, best, NONE)
        if np.array_equal(best, cur):
            break
        cur = best
    return np.where(cur == NONE, np.float32(max_sq), (cur >> 14).astype(np.float32))

# ------------------------------------------------------------------------------------------------ the block writer and reader


def slice_geometry(params):
    """(bz_lo, bz_hi, bz_out, vz_out): the TSDF block rows of the slice's z band and the block row / voxel row the slice is written to."""
    vs = np.float32(params.voxel_size)
    kz = [int(np.floor(np.float32(h) / vs)) for h in (params.esdf_slice_min_height, params.esdf_slice_max_height, params.esdf_slice_height)]
    return kz[0] >> 3, kz[1] >> 3, kz[2] >> 3, kz[2] & 7


def _voxel_values(params):
    """(site distance, free distance, weight): a site is inside (d <= 0) within esdf_max_site_distance_vox, free space is observed at +truncation."""
    vs = np.float32(params.voxel_size)
    site_d = -np.float32(0.5) * vs
    assert abs(site_d) <= np.float32(params.esdf_max_site_distance_vox) * vs
    free_d = np.float32(params.truncation_distance_vox) * vs
    assert free_d > np.float32(params.esdf_max_site_distance_vox) * vs
    return site_d, free_d, np.float32(max(1.0, 2.0 * float(params.esdf_min_weight)))


def alloc_voxels(alloc):
    """block mask -> voxel mask (8 voxels per block and axis)."""
    v = np.asarray(alloc, bool)
    for a in range(v.ndim):
        v = np.repeat(v, 8, axis=a)
    return v


def tsdf_blocks_2d(pattern, alloc, params, origin=(0, 0)):
    """(indices [n, 3] int32, blocks [n, 512] TSDF_DT) for set_blocks: the columns drawn in `pattern` [y, x] become sites, every other column of
    the blocks allocated in `alloc` [by, bx] observed free space; every block row of the z band, and every z of it, alike.  origin = (bx, by)
    of alloc[0, 0].  Block voxel order z + 8 y + 64 x."""
    pattern = np.asarray(pattern, bool); alloc = np.asarray(alloc, bool)
    assert pattern.shape == (alloc.shape[0] * 8, alloc.shape[1] * 8) and not (pattern & ~alloc_voxels(alloc)).any()
    site_d, free_d, w = _voxel_values(params)
    bz_lo, bz_hi, _, _ = slice_geometry(params)
    idx = []; data = []
    for by, bx in np.argwhere(alloc):
        col = pattern[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].T                     # [x, y]
        b = np.zeros((8, 8, 8), TSDF_DT)
        b["distance"] = np.where(col[:, :, None], site_d, free_d); b["weight"] = w
        for bz in range(bz_lo, bz_hi + 1):
            idx.append((origin[0] + int(bx), origin[1] + int(by), bz)); data.append(b.reshape(512))
    return np.asarray(idx, np.int32).reshape(-1, 3), np.asarray(data, TSDF_DT).reshape(-1, 512)


def tsdf_blocks_3d(sites, alloc, params, origin=(0, 0, 0)):
    """The same for a 3-D site set: sites [x, y, z], alloc [bx, by, bz]; each voxel by itself."""
    sites = np.asarray(sites, bool); alloc = np.asarray(alloc, bool)
    assert sites.shape == tuple(8 * s for s in alloc.shape) and not (sites & ~alloc_voxels(alloc)).any()
    site_d, free_d, w = _voxel_values(params)
    idx = []; data = []
    for bx, by, bz in np.argwhere(alloc):
        b = np.zeros((8, 8, 8), TSDF_DT)
        b["distance"] = np.where(sites[bx * 8:bx * 8 + 8, by * 8:by * 8 + 8, bz * 8:bz * 8 + 8], site_d, free_d); b["weight"] = w
        idx.append((origin[0] + int(bx), origin[1] + int(by), origin[2] + int(bz))); data.append(b.reshape(512))
    return np.asarray(idx, np.int32).reshape(-1, 3), np.asarray(data, TSDF_DT).reshape(-1, 512)


def voxel_marks(blocks, params):
    """(site, observed, inside) of TSDF voxels, each by itself (SEMANTICS.md "ESDF 2-D"): observed = weight >= esdf_min_weight; inside = observed
    and distance <= 0; site = observed and |distance| <= esdf_max_site_distance_vox voxels (and, site rule 0, distance <= 0).  The site limit is
    the float32 product of the two parameters.  An occupancy mapper (projective_layer_type 1) holds log-odds -- a plain float array, or voxels with
    a field log_odds: observed = v != 0, inside = site = v > 0 (a -0.0 is unknown like 0.0)."""
    if int(params.projective_layer_type) == 1:
        blocks = np.asarray(blocks)
        v = np.asarray(blocks["log_odds"] if blocks.dtype.names else blocks, np.float32)
        return v > 0, v != 0, v > 0
    d = np.asarray(blocks["distance"], np.float32); w = np.asarray(blocks["weight"], np.float32)
    obs = w >= np.float32(params.esdf_min_weight)
    ins = obs & (d <= 0)
    site = obs & (np.abs(d) <= np.float32(params.esdf_max_site_distance_vox) * np.float32(params.voxel_size))
    if int(params.esdf_site_rule) == 0:
        site &= d <= 0
    return site, obs, ins


def column_marks_2d(tsdf_idx, tsdf_blocks, params, origin, shape_blocks):
    """Dense [y, x] (site, observed, inside) over the box origin (bx, by) + shape_blocks (nby, nbx): the column rule applied to a TSDF read-back --
    a column is marked by ANY voxel of it within the z band (voxel rows, not block rows; each voxel judged by itself, so two voxels that each
    meet half of a rule do not add up).  The band is [esdf_slice_min_height, esdf_slice_max_height], or, over a ground plane, the column's own
    (column_bands)."""
    kz_lo, kz_hi = column_bands(params, origin, shape_blocks)
    Hh, W = shape_blocks[0] * 8, shape_blocks[1] * 8
    out = [np.zeros((Hh, W), bool) for _ in range(3)]
    for i, b in zip(np.asarray(tsdf_idx, np.int64).reshape(-1, 3).tolist(), tsdf_blocks):
        x0, y0 = (i[0] - origin[0]) * 8, (i[1] - origin[1]) * 8
        if not (0 <= x0 < W and 0 <= y0 < Hh):
            continue
        kz = i[2] * 8 + np.arange(8)
        lo = kz_lo[y0:y0 + 8, x0:x0 + 8].T[:, :, None]; hi = kz_hi[y0:y0 + 8, x0:x0 + 8].T[:, :, None]       # [x, y, 1]
        zsel = (kz >= lo) & (kz <= hi)                                                                       # [x, y, z]
        if not zsel.any():
            continue
        for o, m in zip(out, voxel_marks(np.asarray(b).reshape(8, 8, 8), params)):
            o[y0:y0 + 8, x0:x0 + 8] |= (m & zsel).any(2).T
    return tuple(out)


def plane_on(params):
    """The z band follows the ground plane (SEMANTICS.md "Ground-plane-relative slice"): the switch, a plane that points up (n_z > 1e-3) and a
    positive thickness; otherwise the fixed heights apply."""
    return bool(int(params.esdf_use_ground_plane)) and bool(np.float32(params.esdf_ground_plane[2]) > np.float32(1e-3)) \
        and bool(np.float32(params.slice_height_thickness_m) > 0)


def plane_quotients(params, x, y):
    """(lower, upper) edge of the plane-relative band at (x, y) metres, in voxels: (h + above) / vs and (h + above + thickness) / vs with
    h = -(n_x x + n_y y + d) / n_z -- in float64, from the plane coefficients, heights and voxel size as float32 holds them."""
    n = [float(np.float32(v)) for v in params.esdf_ground_plane]
    vs = float(np.float32(params.voxel_size))
    above = float(np.float32(params.slice_height_above_plane_m)); thick = float(np.float32(params.slice_height_thickness_m))
    h = -(n[0] * np.asarray(x, np.float64) + n[1] * np.asarray(y, np.float64) + n[3]) / n[2]
    return (h + above) / vs, (h + above + thick) / vs


def _column_centres(params, origin, shape_blocks):
    vs = float(np.float32(params.voxel_size))
    x = (origin[0] * 8 + np.arange(shape_blocks[1] * 8) + 0.5) * vs
    y = (origin[1] * 8 + np.arange(shape_blocks[0] * 8) + 0.5) * vs
    return np.meshgrid(x, y)                                                                               # [y, x] each


def column_bands(params, origin, shape_blocks):
    """(kz_lo, kz_hi) [y, x] int64: the voxel rows of every column's z band over the box origin (bx, by) + shape_blocks (nby, nbx).  Fixed
    heights: floor(height / voxel_size) of the float32 quotient, the same for all columns.  Over a ground plane: floor of plane_quotients at the
    column's centre ((b * 8 + v + 0.5) * voxel_size)."""
    shape = (shape_blocks[0] * 8, shape_blocks[1] * 8)
    if not plane_on(params):
        vs = np.float32(params.voxel_size)
        lo, hi = (int(np.floor(np.float32(h) / vs)) for h in (params.esdf_slice_min_height, params.esdf_slice_max_height))
        return np.full(shape, lo, np.int64), np.full(shape, hi, np.int64)
    qlo, qhi = plane_quotients(params, *_column_centres(params, origin, shape_blocks))
    return np.floor(qlo).astype(np.int64), np.floor(qhi).astype(np.int64)


def block_band(params, bx, by):
    """(bz_lo, bz_hi): the TSDF block rows the band of block column (bx, by) can touch.  Fixed heights: those of slice_geometry.  Over a ground
    plane: from the lowest and the highest of the plane's heights at the block's four corners (a plane is extremal there)."""
    if not plane_on(params):
        return slice_geometry(params)[:2]
    bs = 8 * float(np.float32(params.voxel_size))
    xs, ys = np.meshgrid([bx * bs, (bx + 1) * bs], [by * bs, (by + 1) * bs])
    qlo, qhi = plane_quotients(params, xs, ys)
    lo, hi = int(np.floor(qlo.min())) >> 3, int(np.floor(qhi.max())) >> 3
    assert hi - lo <= 61, "a plane-relative band of more than 62 blocks (the product cuts it off there) is not modelled"
    return lo, hi


def band_margin(params, origin, shape_blocks):
    """How far (in voxels) the nearest band quotient of the box lies from an integer, over every column centre and every block corner: drawn
    planes keep this at 1e-3 or more, so that floor() is the same in float32 as in exact arithmetic.  inf without a plane."""
    if not plane_on(params):
        return np.inf
    bs = 8 * float(np.float32(params.voxel_size))
    cx, cy = np.meshgrid((origin[0] + np.arange(shape_blocks[1] + 1)) * bs, (origin[1] + np.arange(shape_blocks[0] + 1)) * bs)
    q = np.concatenate([np.ravel(v) for v in plane_quotients(params, *_column_centres(params, origin, shape_blocks)) + plane_quotients(params, cx, cy)])
    return float(np.abs(q - np.rint(q)).min())


def esdf_blocks_expected(dirty_idx, params):
    """The ESDF blocks that an update creates (or keeps) for the dirty TSDF (or occupancy) blocks `dirty_idx`, as a set of (bx, by, bz).  2-D: a
    dirty block (bx, by, bz) within the band's block rows of its column (block_band) stands for ESDF block (bx, by, bz_out); one outside the band
    for nothing.  3-D: every dirty block for the ESDF block of its own index."""
    idx = [tuple(int(v) for v in i) for i in np.asarray(dirty_idx, np.int64).reshape(-1, 3)]
    if int(params.esdf_mode) == 1:
        return set(idx)
    bz_out = slice_geometry(params)[2]
    out = set()
    for bx, by, bz in idx:
        lo, hi = block_band(params, bx, by)
        if lo <= bz <= hi:
            out.add((bx, by, bz_out))
    return out


def volume_marks_3d(tsdf_idx, tsdf_blocks, params, origin, shape_blocks):
    """Dense [x, y, z] (site, observed, inside) over the box: 3-D ESDF, every voxel marked by its own TSDF voxel."""
    dims = tuple(8 * s for s in shape_blocks)
    out = [np.zeros(dims, bool) for _ in range(3)]
    for i, b in zip(np.asarray(tsdf_idx, np.int64).reshape(-1, 3).tolist(), tsdf_blocks):
        s = [(i[a] - origin[a]) * 8 for a in range(3)]
        if not all(0 <= s[a] < dims[a] for a in range(3)):
            continue
        sl = tuple(slice(s[a], s[a] + 8) for a in range(3))
        for o, m in zip(out, voxel_marks(np.asarray(b).reshape(8, 8, 8), params)):
            o[sl] = m
    return tuple(out)


Fields = collections.namedtuple("Fields", "dom sq parent site observed inside")


def slice_fields(idx, blocks, params, origin=None, shape_blocks=None):
    """ESDF blocks (reference voxel layout, [x][y][z]) -> dense [y, x] fields of the slice plane over the box origin (bx, by) + shape_blocks
    (nby, nbx) (default: the blocks' own bounding box).  parent = (dy, dx); every block must lie in the slice's block row and in the box, and
    no parent may leave the plane."""
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    _, _, bz_out, vz_out = slice_geometry(params)
    assert (idx[:, 2] == bz_out).all(), "an ESDF block outside the slice's block row"
    if origin is None:
        origin = (int(idx[:, 0].min()), int(idx[:, 1].min()))
        shape_blocks = (int(idx[:, 1].max()) - origin[1] + 1, int(idx[:, 0].max()) - origin[0] + 1)
    Hh, W = shape_blocks[0] * 8, shape_blocks[1] * 8
    f = Fields(np.zeros((Hh, W), bool), np.zeros((Hh, W), np.float32), np.zeros((Hh, W, 2), np.int32), np.zeros((Hh, W), bool),
               np.zeros((Hh, W), bool), np.zeros((Hh, W), bool))
    for k, (bx, by, _) in enumerate(idx.tolist()):
        pl = np.asarray(blocks[k]).reshape(8, 8, 8)[:, :, vz_out].T                  # [y, x]
        x0, y0 = (bx - origin[0]) * 8, (by - origin[1]) * 8
        assert 0 <= x0 < W and 0 <= y0 < Hh, ("ESDF block outside the box", (bx, by))
        ys, xs = slice(y0, y0 + 8), slice(x0, x0 + 8)
        assert not f.dom[ys, xs].any()
        f.dom[ys, xs] = True; f.sq[ys, xs] = pl["squared_distance_vox"]
        f.parent[ys, xs, 0] = pl["parent_direction"][:, :, 1]; f.parent[ys, xs, 1] = pl["parent_direction"][:, :, 0]
        assert not pl["parent_direction"][:, :, 2].any(), "a 2-D parent with a z component"
        f.site[ys, xs] = pl["is_site"] != 0; f.observed[ys, xs] = pl["observed"] != 0; f.inside[ys, xs] = pl["is_inside"] != 0
    return f, origin


def volume_fields(idx, blocks, origin=None, shape_blocks=None):
    """ESDF blocks -> dense [x, y, z] fields over the box origin (bx, by, bz) + shape_blocks; parent = (dx, dy, dz)."""
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    if origin is None:
        origin = tuple(int(v) for v in idx.min(0)); shape_blocks = tuple(int(v) for v in (idx.max(0) - idx.min(0) + 1))
    dims = tuple(8 * s for s in shape_blocks)
    f = Fields(np.zeros(dims, bool), np.zeros(dims, np.float32), np.zeros(dims + (3,), np.int32), np.zeros(dims, bool), np.zeros(dims, bool),
               np.zeros(dims, bool))
    for k, i in enumerate(idx.tolist()):
        b = np.asarray(blocks[k]).reshape(8, 8, 8)
        s = [(i[a] - origin[a]) * 8 for a in range(3)]
        assert all(0 <= s[a] < dims[a] for a in range(3)), ("ESDF block outside the box", i)
        sl = tuple(slice(s[a], s[a] + 8) for a in range(3))
        assert not f.dom[sl].any()
        f.dom[sl] = True; f.sq[sl] = b["squared_distance_vox"]; f.parent[sl] = b["parent_direction"]
        f.site[sl] = b["is_site"] != 0; f.observed[sl] = b["observed"] != 0; f.inside[sl] = b["is_inside"] != 0
    return f, origin

# ------------------------------------------------------------------------------------------------ the patterns

# name, sites (2-D [y, x] / 3-D [x, y, z]), alloc (block mask), probes = ((position, expected squared distance or None = max_sq), ...):
# what the pattern was drawn to produce at that voxel, asserted against the brute force by tests/test_esdf_model.py
Case = collections.namedtuple("Case", "name sites alloc probes")


def _case(name, shape, pts, alloc, probes=()):
    s = np.zeros(shape, bool)
    for p in pts:
        assert all(0 <= int(v) < n for v, n in zip(p, shape)), (name, p, shape)
        s[tuple(int(v) for v in p)] = True
    s &= alloc_voxels(alloc)
    s.setflags(write=False)
    a = np.array(alloc, bool); a.setflags(write=False)
    return Case(name, s, a, tuple(probes))


def random_sites(shape, density, seed):
    """floor(density * voxels) distinct random positions (at least 3): the density is met exactly, not on average."""
    n = int(np.prod(shape))
    k = max(3, int(density * n))
    flat = np.random.default_rng(seed).choice(n, k, replace=False)
    return [tuple(int(v) for v in p) for p in np.stack(np.unravel_index(flat, shape), -1)]


def cutoff_offsets(r):
    """((a, b), sq) of the lattice offsets just inside and just outside the cut-off, found from max_sq: the largest a^2 + b^2 that still counts and
    the smallest that does not (0 <= a, b <= ri + 1; among equals the most diagonal one)."""
    max_sq, ri = cutoff(r)
    a, b = np.meshgrid(np.arange(ri + 2), np.arange(ri + 2), indexing="ij")
    s = a * a + b * b
    counts = (s.astype(np.float32) <= max_sq) & (a <= ri) & (b <= ri)
    out = []
    for sel, pick in ((counts, s[counts].max()), (~counts, s[~counts].min())):
        k = np.argwhere(sel & (s == pick))
        k = k[np.argmax(k.min(1))]
        out.append(((int(k[0]), int(k[1])), int(pick)))
    return out[0], out[1]


def field_blocks_2d(r):
    return 2 * radius_blocks(r) + 3


def patterns_2d(r, seed=0):
    """The 2-D catalogue for radius r (the float32 quotient) on a field of (2 rb + 3)^2 blocks; every case says in a word why it exists."""
    max_sq, ri = cutoff(r)
    nb = field_blocks_2d(r); N = 8 * nb; cb = nb // 2; c = 8 * cb + 4
    full = np.ones((nb, nb), bool)
    in_range = lambda s: np.float32(s) <= max_sq                                       # noqa: E731
    out = []
    # one site alone, on each corner voxel of a block and in the middle of the field: every voxel within r is a probe at its own offset
    for vy, vx in ((0, 0), (0, 7), (7, 0), (7, 7)):
        out.append(_case("single_y%dx%d" % (vy, vx), (N, N), [(8 * cb + vy, 8 * cb + vx)], full, [((8 * cb + vy, 8 * cb + vx), 0)]))
    out.append(_case("single_centre", (N, N), [(c, c)], full, [((c, c), 0), ((c, c + 1), 1 if in_range(1) else None)]))
    # ties: two and four sites equidistant from a whole row / column / diagonal of voxels
    k = min(ri, 5)
    tie = k * k if in_range(k * k) else None
    out.append(_case("tie_along_y", (N, N), [(c - k, c), (c + k, c)], full, [((c, c), tie)]))
    out.append(_case("tie_along_x", (N, N), [(c, c - k), (c, c + k)], full, [((c, c), tie)]))
    out.append(_case("tie_diagonal", (N, N), [(c - k, c + k), (c + k, c - k)], full, [((c, c), 2 * k * k if in_range(2 * k * k) else None)]))
    out.append(_case("tie_four", (N, N), [(c - k, c - k), (c - k, c + k), (c + k, c - k), (c + k, c + k)], full, [((c, c), 2 * k * k if in_range(2 * k * k) else None)]))
    # reach: one site exactly ri from probe A along a direction, another exactly ri + 1 from probe B (B is ri + 5 to the side: neither probe sees
    # the other's site)
    for name, (ey, ex) in (("+x", (0, 1)), ("-x", (0, -1)), ("+y", (1, 0)), ("-y", (-1, 0))):
        oy, ox = ex, ey
        pb = (c + oy * (ri + 5), c + ox * (ri + 5))
        out.append(_case("reach" + name, (N, N), [(c + ey * ri, c + ex * ri), (pb[0] + ey * (ri + 1), pb[1] + ex * (ri + 1))], full,
                         [((c, c), ri * ri if in_range(ri * ri) else None), (pb, None)]))
    # the cut-off itself: four sites at the lattice offset whose squared length is the last that counts / the first that does not
    (ins, s_in), (outs, s_out) = cutoff_offsets(r)
    for name, (a, b), want in (("cutoff_inside", ins, s_in), ("cutoff_outside", outs, None)):
        pts = {(c + sy * a, c + sx * b) for sy in (-1, 1) for sx in (-1, 1)}
        out.append(_case(name, (N, N), sorted(pts), full, [((c, c), want)]))
    # dense words for the row pass
    out.append(_case("full_row", (N, N), [(c - 3, x) for x in range(N)], full, [((c, c), 9 if in_range(9) else None)]))
    out.append(_case("full_column", (N, N), [(y, c + 2) for y in range(N)], full, [((c, c), 4 if in_range(4) else None)]))
    # sparse random sites
    out.append(_case("random_sparse", (N, N), random_sites((N, N), 0.01, 200 + seed + ri), full))
    # every site in one block, the rest of the field free: the window of an update is one block + R
    rng = np.random.default_rng(100 + seed + ri)
    one = [(8 * cb + int(v[0]), 8 * cb + int(v[1])) for v in rng.integers(0, 8, (6, 2))]
    out.append(_case("one_block", (N, N), one, full))
    # an allocation with holes: the exact transform sees through them, the iterative one does not
    out.append(holes_2d(r, seed))
    return out


def holes_2d(r, seed=0):
    _, ri = cutoff(r)
    nb = field_blocks_2d(r); N = 8 * nb; cb = nb // 2; c = 8 * cb + 4
    alloc = np.ones((nb, nb), bool)
    alloc[cb, cb + 1] = False; alloc[cb - 1, cb - 1] = False; alloc[cb + 1, cb] = False
    if nb >= 7:
        alloc[0:nb - 2, 1] = False                   # a wall of missing blocks with a gap at its end
    return _case("holes", (N, N), [(c, c)] + random_sites((N, N), 0.009, 250 + seed + ri), alloc)


def field_blocks_3d(r):
    return 2 * radius_blocks(r) + 3


def strips_3d(nb):
    """Three axis-aligned strips and one diagonal strip of blocks through the centre block of an nb^3 box."""
    cb = nb // 2
    a = np.zeros((nb, nb, nb), bool)
    a[:, cb, cb] = True; a[cb, :, cb] = True; a[cb, cb, :] = True
    a[np.arange(nb), np.arange(nb), np.arange(nb)] = True
    return a


def alloc_3d(r, cap=7):
    nb = field_blocks_3d(r)
    return np.ones((nb, nb, nb), bool) if nb <= cap else strips_3d(nb)


def patterns_3d(r, seed=0):
    """The 3-D catalogue on a box of (2 rb + 3)^3 blocks: all of them allocated up to 7^3, beyond that only three axis-aligned strips and one
    diagonal strip through the centre block (sites outside the allocation are dropped)."""
    max_sq, ri = cutoff(r)
    nb = field_blocks_3d(r); N = 8 * nb; cb = nb // 2; c = 8 * cb + 4
    alloc = alloc_3d(r)
    shape = (N, N, N)
    in_range = lambda s: np.float32(s) <= max_sq                                       # noqa: E731
    ctr = np.array([c, c, c])
    out = []
    corners = [(8 * cb + 7 * i, 8 * cb + 7 * j, 8 * cb + 7 * k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    for p in (corners[0], corners[7], corners[3]):
        out.append(_case("single_%d%d%d" % tuple(v & 7 for v in p), shape, [p], alloc, [(p, 0)]))
    k = min(ri, 3)
    E = np.eye(3, dtype=int)
    out.append(_case("ties_three_axes", shape, [tuple(ctr + s * k * E[a]) for a in range(3) for s in (-1, 1)], alloc, [((c, c, c), k * k if in_range(k * k) else None)]))
    # reach along an axis: a site exactly ri from the centre on one side, exactly ri + 1 on the other (the voxel next to the centre sees them the other way round)
    for a, name in enumerate("xyz"):
        out.append(_case("reach_" + name, shape, [tuple(ctr + ri * E[a]), tuple(ctr - (ri + 1) * E[a])], alloc,
                         [((c, c, c), ri * ri if in_range(ri * ri) else None), (tuple(ctr - E[a]), ri * ri if in_range(ri * ri) else None)]))
    # ... and along the space diagonal: the last diagonal offset that counts on one side, the first that does not on the other
    d = max(v for v in range(ri + 1) if in_range(3 * v * v) or v == 0)
    out.append(_case("reach_diagonal", shape, [tuple(ctr + d), tuple(ctr - (d + 1))], alloc, [((c, c, c), 3 * d * d if in_range(3 * d * d) else None)]))
    rng = np.random.default_rng(300 + seed + ri)
    vox = np.argwhere(alloc_voxels(alloc))
    out.append(_case("random_sparse", shape, vox[rng.choice(len(vox), max(4, len(vox) // 2000), replace=False)], alloc))
    return out


def one_block_3d(r, seed=0):
    """Sites in the centre block only (two opposite corners + a few random voxels), strips allocated: the widest key fields of the y and z passes."""
    nb = field_blocks_3d(r); N = 8 * nb; cb = nb // 2
    rng = np.random.default_rng(400 + seed)
    pts = [(8 * cb, 8 * cb, 8 * cb), (8 * cb + 7, 8 * cb + 7, 8 * cb + 7)] + [tuple(8 * cb + int(v) for v in q) for q in rng.integers(0, 8, (4, 3))]
    return _case("one_block", (N, N, N), pts, strips_3d(nb))
