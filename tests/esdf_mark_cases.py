"""The ESDF site-marking pass on DRAWN TSDF columns, bands and ground planes: what tests/test_esdf_mark_model.py (CPU, the model against the checker)
and tests/test_gpu_esdf_marking.py (GPU, the product against the model and the checker) share.

The drawn ESDF tests (tests/esdf_independent.py tsdf_blocks_2d) write every z of every band block alike, with values far from every threshold; here
each voxel is drawn by itself.  A case is a few blocks for set_blocks, written in one or more steps with an update after each, a parameter set and
the expectation of the model (tests/esdf_independent.py: voxel_marks, column_marks_2d, esdf_blocks_expected, edt_bruteforce):

  a  predicate table: the 64 columns of one block column, each marked by one or two voxels on a threshold of the rule (weight at / around
     esdf_min_weight, distance 0, -0, subnormal, at / around the site limit, ...); site rules 0 and 1
  b  band geometry: a site voxel on the rows kz_lo - 1, kz_lo, kz_hi, kz_hi + 1 of bands of 1, 2, 3, 5 and 63 blocks, with blocks missing,
     below z = 0, with the output slice outside the band; blocks outside the band that must not create a column; the refused bands
  c  re-marking a column whose blocks are written again one at a time
  d  a dirty list of 576 entries (more than two per worker of a 256-worker carrier)
  e  a tilted ground plane: each column's own band, a staircase of sites on every column's kz_hi; the two fall-backs to fixed heights
  f  an occupancy mapper: log-odds 0, the smallest float32 of either sign, +-1 on the rows around the band
  g  the 3-D mode: the table of (a), voxel by voxel; TSDF under both site rules, and occupancy

Voxel size 0.05 m.  Fixed heights are (k + 0.5) voxels, so that floor() of the float32 quotient is k without doubt; under a plane every band quotient
stays 1e-3 voxel or more from an integer (EI.band_margin; float32 evaluation of the plane height and the two additions is off by at most about
2e-6 m within +-2 m of the origin and |h| <= 4 m, i.e. 5e-5 voxel: a 20-fold margin).  Block voxel order z + 8 y + 64 x.
"""
import collections

import numpy as np

import esdf_cases as EC
import esdf_independent as EI

F = np.float32
VOXEL = 0.05
VS = F(VOXEL)
INF = F(np.inf)
TSDF_DT = EI.TSDF_DT

MIN_W = F(0.1)                        # esdf_min_weight as the parameter struct holds it
LIMIT = F(F(2.0) * VS)                # the site limit: float32(esdf_max_site_distance_vox * voxel_size), as the kernel forms it
TRUNC = F(F(4.0) * VS)
SITE_D = F(-0.5) * VS
GOOD_W = F(1.0)
TINY = np.nextafter(F(0), INF)        # the smallest positive float32 (a subnormal)


def up(v):
    return np.nextafter(F(v), INF)


def dn(v):
    return np.nextafter(F(v), -INF)


# name, parameter overrides, ground plane (or None), "tsdf" / "occ", 2 / 3, [(indices [n, 3], voxels [n, 512])] one entry per set_blocks + update,
# block capacity, radius in voxels, and for a refused band the parameter overrides that the update must refuse (else None)
Case = collections.namedtuple("Case", "name kw plane layer dims steps capacity radius refuse")
# what the model expects after a step: the ESDF blocks (sorted tuples), the box (origin, shape in blocks) and over it the dense allocation and marks
Expect = collections.namedtuple("Expect", "blocks origin shape dom site observed inside")


def heights(k_lo, k_hi, k_out):
    """slice heights that put the band on voxel rows k_lo .. k_hi and the output on row k_out: (k + 0.5) voxels each"""
    kw = dict(esdf_slice_min_height=(k_lo + 0.5) * VOXEL, esdf_slice_max_height=(k_hi + 0.5) * VOXEL, esdf_slice_height=(k_out + 0.5) * VOXEL)
    for k, h in zip((k_lo, k_hi, k_out), kw.values()):
        q = float(F(h) / VS)
        assert int(np.floor(q)) == k and abs(q - np.rint(q)) > 0.4, (k, h, q)
    return kw


DEFAULT_BAND = (1, 13, 1)             # the shipped heights 0.09 .. 0.65 m, output at 0.09 m, as rows


def params(M, case, **more):
    kw = dict(heights(*DEFAULT_BAND), **case.kw)
    kw.update(more)
    p = M.default_params(voxel_size=VOXEL, esdf_max_distance_m=EI.distance_for_radius(case.radius, VOXEL), **kw)
    if case.plane is not None:
        for i in range(4):
            p.esdf_ground_plane[i] = float(case.plane[i])
    assert F(p.esdf_min_weight) == MIN_W and F(F(p.esdf_max_site_distance_vox) * F(p.voxel_size)) == LIMIT and F(p.truncation_distance_vox) * VS == TRUNC
    return p, EI.radius_of(p.esdf_max_distance_m, p.voxel_size)[0]


def _block(d, w):
    b = np.zeros((8, 8, 8), TSDF_DT)                       # [x][y][z]
    b["distance"] = d; b["weight"] = w
    return b


def _free():
    return _block(TRUNC, GOOD_W)


def _steps(*writes):
    """each write {key: block [8, 8, 8]} -> (indices, voxels [n, 512])"""
    out = []
    for w in writes:
        keys = sorted(w)
        out.append((np.asarray(keys, np.int32).reshape(-1, 3), np.stack([np.ascontiguousarray(w[k]).reshape(512) for k in keys])))
    return out


def _case(name, writes, kw=None, plane=None, layer="tsdf", dims=2, capacity=1024, radius=3, refuse=None):
    return Case(name, dict(kw or {}), plane, layer, dims, _steps(*writes), capacity, radius, refuse)


# ------------------------------------------------------------------------------------------------ a: the predicate table
# name, the column's voxels (weight, distance), (observed, inside, site under rule 0, site under rule 1) as the rule of SEMANTICS.md gives them
TABLE = [
    ("weight at the minimum", [(MIN_W, SITE_D)], (1, 1, 1, 1)),
    ("weight one float32 below the minimum", [(dn(MIN_W), SITE_D)], (0, 0, 0, 0)),
    ("weight one float32 above the minimum", [(up(MIN_W), SITE_D)], (1, 1, 1, 1)),
    ("weight 0", [(F(0), SITE_D)], (0, 0, 0, 0)),
    ("distance 0.0", [(GOOD_W, F(0.0))], (1, 1, 1, 1)),
    ("distance -0.0", [(GOOD_W, F(-0.0))], (1, 1, 1, 1)),
    ("smallest positive distance", [(GOOD_W, TINY)], (1, 0, 0, 1)),
    ("smallest negative distance", [(GOOD_W, -TINY)], (1, 1, 1, 1)),
    ("+ the site limit", [(GOOD_W, LIMIT)], (1, 0, 0, 1)),
    ("+ one float32 below the limit", [(GOOD_W, dn(LIMIT))], (1, 0, 0, 1)),
    ("+ one float32 above the limit", [(GOOD_W, up(LIMIT))], (1, 0, 0, 0)),
    ("- the site limit", [(GOOD_W, -LIMIT)], (1, 1, 1, 1)),
    ("- one float32 below the limit", [(GOOD_W, -dn(LIMIT))], (1, 1, 1, 1)),
    ("- one float32 above the limit", [(GOOD_W, -up(LIMIT))], (1, 1, 0, 0)),
    ("deeper than the limit", [(GOOD_W, -TRUNC)], (1, 1, 0, 0)),
    ("free space at +truncation", [(GOOD_W, TRUNC)], (1, 0, 0, 0)),
    ("inside and near the surface at different z", [(GOOD_W, -TRUNC), (GOOD_W, -SITE_D)], (1, 1, 0, 1)),
    ("the qualifying voxel just unobserved, another observed", [(dn(MIN_W), SITE_D), (GOOD_W, TRUNC)], (1, 0, 0, 0)),
    ("minimum weight at the limit", [(MIN_W, -LIMIT)], (1, 1, 1, 1)),
    ("distance 0 just unobserved", [(dn(MIN_W), F(0.0))], (0, 0, 0, 0)),
]
TABLE_VOXELS = [v for _, vox, _ in TABLE for v in vox]                     # (g): every voxel of the table by itself


def table_column_entry(c):
    """the table entry of column c = vx + 8 vy of the table's block column"""
    return TABLE[c % len(TABLE)]


def table_rows(c, k_lo=DEFAULT_BAND[0], k_hi=DEFAULT_BAND[1]):
    """the band rows of column c's first and second voxel: every row of the band, and with it every z of both band blocks, carries some entry"""
    n = k_hi - k_lo + 1
    return k_lo + (5 * c) % n, k_lo + (5 * c + 6) % n


def case_table(rule):
    blocks = {(0, 0, 0): _block(SITE_D, F(0)), (0, 0, 1): _block(SITE_D, F(0))}          # weight 0 everywhere else, at a distance that would make a site
    for c in range(64):
        vx, vy = c & 7, c >> 3
        for (w, d), kz in zip(table_column_entry(c)[1], table_rows(c)):
            b = blocks[(0, 0, kz >> 3)]
            b["weight"][vx, vy, kz & 7] = w; b["distance"][vx, vy, kz & 7] = d
    return _case("a-table-rule%d" % rule, [blocks], dict(esdf_site_rule=rule))


def table_expectation(rule):
    """dense [y, x] (site, observed, inside) of the table's block column, from the table's own last column -- not from the model"""
    out = [np.zeros((8, 8), bool) for _ in range(3)]
    for c in range(64):
        o, i, s0, s1 = table_column_entry(c)[2]
        for f, v in zip(out, ((s1 if rule else s0), o, i)):
            f[c >> 3, c & 7] = bool(v)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ b: band geometry
BAND_COLUMNS = {"below": (1, 1), "lo": (5, 1), "hi": (1, 5), "above": (5, 5)}           # (vx, vy) of the column that carries the site voxel
DECOY = (3, 0)                        # a block column with blocks just outside the band only, full of site voxels: it must get no ESDF block


def band_rows(k_lo, k_hi):
    return {"below": k_lo - 1, "lo": k_lo, "hi": k_hi, "above": k_hi + 1}


def case_band(name, k_lo, k_hi, k_out, draw=("below", "lo", "hi", "above"), missing=(), band_blocks=True, refuse=None):
    """Block column (0, 0): observed free space in every allocated block, one site voxel per drawn column on its row; allocated are the band's
    blocks (unless band_blocks is off) without `missing`, and every block that holds a drawn row."""
    rows = band_rows(k_lo, k_hi)
    bz = set(range(k_lo >> 3, (k_hi >> 3) + 1)) if band_blocks else set()
    bz -= set(missing)
    bz |= {rows[d] >> 3 for d in draw}
    assert not set(missing) & bz
    blocks = {(0, 0, z): _free() for z in bz}
    for d in draw:
        vx, vy = BAND_COLUMNS[d]
        blocks[(0, 0, rows[d] >> 3)]["distance"][vx, vy, rows[d] & 7] = SITE_D
    for z in ((k_lo >> 3) - 1, (k_hi >> 3) + 1):
        blocks[DECOY + (z,)] = _block(SITE_D, GOOD_W)
    return _case("b-" + name, [blocks], heights(k_lo, k_hi, k_out), refuse=refuse)


BANDS = {
    "one_block": dict(k_lo=2, k_hi=5, k_out=2),                                            # nz == 1
    "one_row": dict(k_lo=11, k_hi=11, k_out=11),
    "default": dict(k_lo=1, k_hi=13, k_out=1),                                             # nz == 2
    "three_blocks_hole": dict(k_lo=3, k_hi=20, k_out=3, draw=("below", "hi", "above"), missing=(1,)),      # the q >= 2 loop, past a missing block
    "five_blocks_hole": dict(k_lo=5, k_hi=38, k_out=5, draw=("below", "hi", "above"), missing=(2,)),
    "across_zero": dict(k_lo=-5, k_hi=6, k_out=1),
    "below_zero": dict(k_lo=-17, k_hi=-8, k_out=-12),                                      # blocks -3 .. -1: the sites on the last row of -3 and the first of -1
    "slice_outside": dict(k_lo=10, k_hi=13, k_out=27),                                     # the output in block row 3, the band in block row 1
    "63_blocks": dict(k_lo=-248, k_hi=255, k_out=1, draw=("lo", "hi"), band_blocks=False),  # blocks -31 .. 31, only the lowest and the highest allocated
}
# the bands an update refuses (NVBX_E_INVALID, the map untouched): 64 blocks, and the upper height in a block row below the lower one's
REFUSED = {"64_blocks": heights(-256, 255, 1), "max_below_min": heights(13, 1, 1)}


def case_refused(name):
    c = case_band("default", **BANDS["default"])
    return c._replace(name="b-refused-" + name, refuse=REFUSED[name])


# ------------------------------------------------------------------------------------------------ c: re-marking
REMARK_SITE = (2, 3, 10)              # (vx, vy, row): in the upper band block of block column (0, 0)


def _remark_blocks():
    lower = {(bx, 0, 0): _free() for bx in (-1, 0)}
    upper = {(bx, 0, 1): _free() for bx in (-1, 0)}
    upper[(0, 0, 1)]["distance"][REMARK_SITE[0], REMARK_SITE[1], REMARK_SITE[2] & 7] = SITE_D
    return lower, upper


def case_remark():
    """both blocks of the column in one pass (two dirty entries, one column); the lower one again, as it was; the upper one as free space"""
    lower, upper = _remark_blocks()
    return _case("c-remark", [{**lower, **upper}, {(0, 0, 0): lower[(0, 0, 0)]}, {(0, 0, 1): _free()}])


def case_remark_one_at_a_time():
    """the same column from one dirty entry per pass: its first step's result is free space, its second equals case_remark's first"""
    lower, upper = _remark_blocks()
    return _case("c-one-at-a-time", [lower, upper])


# ------------------------------------------------------------------------------------------------ d: a long dirty list
LONG_N = 24
LONG_BAND = (2, 5, 2)


def case_long_list():
    """24 x 24 blocks of one band block row, written in one call: 576 dirty entries.  368 voxels (1 % of the columns) drawn at random (x, y, z)
    carry a site distance; those on the band's rows 2 .. 5 are sites, the others lie above or below the band in the same block."""
    N = 8 * LONG_N
    rng = np.random.default_rng(5)
    flat = rng.choice(N * N, N * N // 100, replace=False)
    z = rng.integers(0, 8, len(flat))
    d = np.full((N, N, 8), TRUNC, F)                                                     # [x, y, z]
    d[flat % N, flat // N, z] = SITE_D
    blocks = {(bx, by, 0): _block(d[8 * bx:8 * bx + 8, 8 * by:8 * by + 8], GOOD_W) for bx in range(LONG_N) for by in range(LONG_N)}
    return _case("d-long-list", [blocks], heights(*LONG_BAND), capacity=4096, radius=2)


# ------------------------------------------------------------------------------------------------ e: ground plane
# h(x, y) = 0.3 x + 0.2 y + 0.075 m: 1.5 voxels at the origin, + 0.3 voxel per column in x, + 0.2 in y -- 3.5 rows across a block; band = h + 1 voxel
# .. h + 5 voxels.  In block column (0, 0) kz_hi runs from 6 to 10: across the block boundary at row 8.  Every quotient ends in .05, .15, ... .95.
PLANE = (-0.3, -0.2, 1.0, -0.075)
PLANE_KW = dict(esdf_use_ground_plane=1, slice_height_above_plane_m=1 * VOXEL, slice_height_thickness_m=4 * VOXEL)
PLANE_COLUMNS = {(0, 0): "hi", (1, 0): "above", (0, 1): "below", (-1, -1): "lo"}         # block column -> the row of its band every column draws a voxel on
PLANE_BOX = ((-1, -1), (3, 3))                                                          # origin (bx, by), shape (nby, nbx)


def _plane_blocks(p):
    """the staircase: in every column of the four block columns one site voxel on the named row of THAT column's band, free space elsewhere;
    allocated are the block rows of EI.block_band and whichever block holds a drawn voxel"""
    origin, shape = PLANE_BOX
    kz_lo, kz_hi = EI.column_bands(p, origin, shape)
    blocks = {}
    for (bx, by), which in PLANE_COLUMNS.items():
        lo, hi = EI.block_band(p, bx, by)
        for z in range(lo, hi + 1):
            blocks[(bx, by, z)] = _free()
        for vx in range(8):
            for vy in range(8):
                y, x = (by - origin[1]) * 8 + vy, (bx - origin[0]) * 8 + vx
                kz = int(band_rows(kz_lo[y, x], kz_hi[y, x])[which])
                blocks.setdefault((bx, by, kz >> 3), _free())["distance"][vx, vy, kz & 7] = SITE_D
    return blocks


def case_plane(M, variant="tilted"):
    """variant: "tilted" (the plane applies), "flat_normal" (n_z == 1e-3: not above it) and "no_thickness": the two fall-backs, which read the
    staircase drawn for the tilted plane through the fixed heights, and "fixed" (the switch off): what both fall-backs must equal."""
    tilted = _case("e-plane-tilted", [], PLANE_KW, PLANE)
    pt = params(M, tilted)[0]
    assert EI.plane_on(pt) and EI.band_margin(pt, *PLANE_BOX) >= 1e-3, "a band quotient of a drawn column or block corner within 1e-3 voxel of an integer"
    blocks = _plane_blocks(pt)
    kw, plane = dict(PLANE_KW), PLANE
    if variant == "flat_normal":
        plane = PLANE[:2] + (float(F(1e-3)),) + PLANE[3:]
    elif variant == "no_thickness":
        kw["slice_height_thickness_m"] = 0.0
    elif variant == "fixed":
        kw["esdf_use_ground_plane"] = 0
    else:
        assert variant == "tilted"
    return _case("e-plane-" + variant, [blocks], kw, plane)


# ------------------------------------------------------------------------------------------------ f: occupancy
LOG_ODDS = [F(0), TINY, -TINY, F(1), F(-1)]


def case_occupancy():
    """log-odds; column c = 5 r + v of block column (0, 0) carries value v on row r of (kz_lo - 1, kz_lo, kz_hi, kz_hi + 1), 0 (unknown) elsewhere"""
    k_lo, k_hi, _ = DEFAULT_BAND
    blocks = {(0, 0, z): np.zeros((8, 8, 8), F) for z in (0, 1)}
    for r, kz in enumerate(band_rows(k_lo, k_hi).values()):
        for v, lo in enumerate(LOG_ODDS):
            c = 5 * r + v
            blocks[(0, 0, kz >> 3)][c & 7, c >> 3, kz & 7] = lo
    return _case("f-occupancy", [blocks], dict(projective_layer_type=1), layer="occ")


# ------------------------------------------------------------------------------------------------ g: 3-D
def case_3d(kind):
    """kind: "rule0" / "rule1" (voxel v of one TSDF block carries TABLE_VOXELS[v % n]) or "occupancy" (LOG_ODDS and -0.0)"""
    if kind == "occupancy":
        vals = LOG_ODDS + [F(-0.0)]
        b = np.array([vals[v % len(vals)] for v in range(512)], F).reshape(8, 8, 8)
        return _case("g-3d-occupancy", [{(0, -1, 2): b}], dict(esdf_mode=1, projective_layer_type=1), layer="occ", dims=3, radius=2)
    b = np.zeros(512, TSDF_DT)
    for v in range(512):
        b["weight"][v], b["distance"][v] = TABLE_VOXELS[v % len(TABLE_VOXELS)]
    return _case("g-3d-" + kind, [{(0, -1, 2): b.reshape(8, 8, 8)}], dict(esdf_mode=1, esdf_site_rule=int(kind[-1])), dims=3, radius=2)


# ------------------------------------------------------------------------------------------------ the catalogue
CASE_NAMES = (["a-table-rule0", "a-table-rule1"] + ["b-" + n for n in BANDS] + ["c-remark", "c-one-at-a-time", "d-long-list"] +
              ["e-plane-" + v for v in ("tilted", "flat_normal", "no_thickness", "fixed")] + ["f-occupancy", "g-3d-rule0", "g-3d-rule1", "g-3d-occupancy"])
REFUSED_NAMES = ["b-refused-" + n for n in REFUSED]
# the cases that run again with the marking pass carried by each launch that can carry it
CARRIER_CASES = ["a-table-rule0", "b-one_block", "b-three_blocks_hole", "b-63_blocks", "d-long-list", "e-plane-tilted"]


def case_by_name(M, name):
    kind, rest = name[0], name[2:]
    if kind == "a":
        return case_table(int(rest[-1]))
    if kind == "b":
        return case_refused(rest[len("refused-"):]) if rest.startswith("refused-") else case_band(rest, **BANDS[rest])
    if kind == "c":
        return case_remark() if rest == "remark" else case_remark_one_at_a_time()
    if kind == "d":
        return case_long_list()
    if kind == "e":
        return case_plane(M, rest[len("plane-"):])
    if kind == "f":
        return case_occupancy()
    return case_3d(rest[len("3d-"):])


# ------------------------------------------------------------------------------------------------ the model's expectation
def case_box(case):
    """(origin, shape in blocks) of everything the case ever writes: 2-D (bx, by), (nby, nbx); 3-D (bx, by, bz), (nbx, nby, nbz)"""
    idx = np.concatenate([s[0] for s in case.steps])
    lo, hi = idx.min(0), idx.max(0)
    if case.dims == 3:
        return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)
    return (int(lo[0]), int(lo[1])), (int(hi[1] - lo[1] + 1), int(hi[0] - lo[0] + 1))


def expectations(case, p):
    """[Expect] after each step of the case, from the model alone: the projective blocks written so far (a later write replaces an earlier one),
    the ESDF blocks the dirty blocks of all steps so far stand for, and the marking rule over those."""
    origin, shape = case_box(case)
    tsdf = {}; esdf = set(); out = []
    for idx, data in case.steps:
        for i, b in zip(idx.tolist(), data):
            tsdf[tuple(i)] = b
        esdf |= EI.esdf_blocks_expected(idx, p)
        keys = sorted(tsdf)
        mask = np.zeros(shape, bool)
        if case.dims == 2:
            for bx, by, _ in esdf:
                mask[by - origin[1], bx - origin[0]] = True
            marks = EI.column_marks_2d(keys, [tsdf[k] for k in keys], p, origin, shape)
        else:
            for k in esdf:
                mask[tuple(k[a] - origin[a] for a in range(3))] = True
            marks = EI.volume_marks_3d(keys, [tsdf[k] for k in keys], p, origin, shape)
        dom = EI.alloc_voxels(mask)
        out.append(Expect(sorted(esdf), origin, shape, dom, *(m & dom for m in marks)))
    return out


# ------------------------------------------------------------------------------------------------ a read-back against the expectation
def in_box(idx, exp, dims):
    """which of the blocks `idx` lie over the expectation's box (in (x, y) for the slice, in all three axes in 3-D)"""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    if dims == 3:
        return ((idx >= np.asarray(exp.origin)) & (idx < np.asarray(exp.origin) + np.asarray(exp.shape))).all(1)
    (ox, oy), (nby, nbx) = exp.origin, exp.shape
    return (idx[:, 0] >= ox) & (idx[:, 0] < ox + nbx) & (idx[:, 1] >= oy) & (idx[:, 1] < oy + nby)


def assert_expected(tag, idx, blocks, p, q, exp, dims, whole_layer=True):
    """An ESDF layer read back (indices, voxels) against the model's expectation, nothing sampled or tolerated: the block set; site / observed /
    inside of every allocated voxel; the squared distance of every allocated voxel == the brute force over the model's sites; valid parents,
    present exactly where a site counts.  whole_layer: the layer holds the expected blocks and no others (else: no others over the box).
    Returns the fields."""
    idx = np.asarray(idx, np.int32).reshape(-1, 3); blocks = np.asarray(blocks).reshape(len(idx), 512)
    keep = in_box(idx, exp, dims)
    assert not whole_layer or keep.all(), (tag, "ESDF blocks outside the drawn box", idx[~keep][:5].tolist())
    got = sorted(tuple(int(v) for v in i) for i in idx[keep])
    assert got == exp.blocks, (tag, "ESDF block set", "only in the map", sorted(set(got) - set(exp.blocks))[:5], "only in the model", sorted(set(exp.blocks) - set(got))[:5])
    if not exp.blocks:
        return None
    if dims == 2:
        f, _ = EI.slice_fields(idx[keep], blocks[keep], p, exp.origin, exp.shape)
    else:
        f, _ = EI.volume_fields(idx[keep], blocks[keep], exp.origin, exp.shape)
    assert np.array_equal(f.dom, exp.dom), (tag, "allocated ESDF voxels")
    for name, have, want in (("is_site", f.site, exp.site), ("observed", f.observed, exp.observed), ("is_inside", f.inside, exp.inside)):
        assert np.array_equal(have, want), (tag, name, "%d marked, %d by the model" % (int(have.sum()), int(want.sum())), "differs at", np.argwhere(have != want)[:6].tolist())
    sq, cnt = EI.edt_bruteforce(exp.site, exp.dom, q)
    bad = exp.dom & (f.sq != sq)
    assert not bad.any(), (tag, "squared distance differs from the brute force at", np.argwhere(bad)[:5].tolist(), f.sq[bad][:5].tolist(), sq[bad][:5].tolist())
    EI.check_parents(exp.site, f.sq, f.parent, exp.dom, q)
    assert np.array_equal((f.parent != 0).any(-1)[exp.dom], ((cnt > 0) & ~exp.site)[exp.dom]), (tag, "a parent exactly where a site counts")
    assert not f.parent[~exp.dom].any()
    return f


# ------------------------------------------------------------------------------------------------ the checker
def checker_write(oracle_mod, o, idx, data):
    """a step's blocks into the checker, which holds log-odds in the distance of its projective layer"""
    for i, b in zip(np.asarray(idx).tolist(), data):
        if b.dtype != oracle_mod.TSDF_DT:
            t = np.zeros(512, oracle_mod.TSDF_DT); t["distance"] = b; b = t
        o.set_block(oracle_mod.L_TSDF, i, np.ascontiguousarray(b))


def checker_steps(oracle_mod, case, p):
    """the case through the CPU checker: yields, after each step's update, its ESDF layer (indices, voxels)"""
    import helpers as H
    o = oracle_mod.OracleMap(H.copy_params(p, oracle_mod.OrcParams))
    for idx, data in case.steps:
        checker_write(oracle_mod, o, idx, data)
        o.update_esdf()
        yield EC.oracle_esdf(oracle_mod, o)
