"""The model of the ESDF marking pass (tests/esdf_independent.py: voxel_marks, column_marks_2d, column_bands, esdf_blocks_expected) and the drawn
cases of tests/esdf_mark_cases.py, validated where they can be, on the CPU: every case goes through the CPU checker, whose observed / is_inside /
is_site on every allocated ESDF voxel and whose ESDF block set must equal the model's (SEMANTICS.md "ESDF 2-D" decides where they differ); and
the cases are held to what they were drawn for, so that none of them is vacuous.  tests/test_gpu_esdf_marking.py then holds the product to the
same expectations.  No GPU."""
import numpy as np
import pytest

import esdf_independent as EI
import esdf_mark_cases as MC

F = np.float32


def _M():
    from isaac_ros_nvblox_amd import mapper as M
    return M


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_model_equals_the_checker(oracle_mod, name):
    """Every step of every case: the checker's ESDF layer meets the model's expectation -- block set, marks, and with them the distances (brute
    force over the model's sites) and parents."""
    M = _M()
    case = MC.case_by_name(M, name)
    p, q = MC.params(M, case)
    exps = MC.expectations(case, p)
    assert len(exps) == len(case.steps) >= 1
    for k, ((oi, ob), exp) in enumerate(zip(MC.checker_steps(oracle_mod, case, p), exps)):
        MC.assert_expected((name, "step", k, "checker"), oi, ob, p, q, exp, case.dims)


def test_predicate_table_is_what_the_rule_says():
    """The model's marks of the table's block column equal the table's own last column, written down from SEMANTICS.md, under both site rules;
    the table holds every threshold it names, and every row of the band (every z of both band blocks) decides some column."""
    M = _M()
    for rule in (0, 1):
        case = MC.case_table(rule)
        p, _ = MC.params(M, case)
        exp = MC.expectations(case, p)[0]
        assert exp.blocks == [(0, 0, 0)] and exp.dom.all()
        for name, have, want in zip(("site", "observed", "inside"), (exp.site, exp.observed, exp.inside), MC.table_expectation(rule)):
            assert np.array_equal(have, want), (rule, name, [MC.table_column_entry(int(y) * 8 + int(x))[0] for y, x in np.argwhere(have != want)])
    s0, s1 = MC.table_expectation(0)[0], MC.table_expectation(1)[0]
    assert (s1 & ~s0).sum() >= 8 and not (s0 & ~s1).any(), "the rules differ on the positive near-surface columns only"
    w = {float(v[0]) for v in MC.TABLE_VOXELS}; d = [v[1] for v in MC.TABLE_VOXELS]
    assert {float(MC.MIN_W), float(MC.dn(MC.MIN_W)), float(MC.up(MC.MIN_W))} <= w
    bits = {int(np.asarray(v, F).view(np.uint32)) for v in d}
    assert {0x00000000, 0x80000000, 0x00000001, 0x80000001} <= bits, "0.0, -0.0 and the smallest float32 of either sign"
    for s in (1, -1):
        assert {float(F(s) * MC.LIMIT), float(F(s) * MC.dn(MC.LIMIT)), float(F(s) * MC.up(MC.LIMIT))} <= {float(v) for v in d}
    rows = {r for c in range(64) for r, _ in zip(MC.table_rows(c), MC.table_column_entry(c)[1])}
    assert rows == set(range(MC.DEFAULT_BAND[0], MC.DEFAULT_BAND[1] + 1))
    assert all(a != b for a, b in map(MC.table_rows, range(64)))


@pytest.mark.parametrize("name", list(MC.BANDS))
def test_band_cases_are_what_they_were_drawn_for(name):
    """The site voxels on kz_lo and kz_hi make sites, those on kz_lo - 1 and kz_hi + 1 do not (every drawn column is observed free space
    otherwise); the decoy column gets no ESDF block; the band spans the blocks the case is named for."""
    M = _M()
    spec = MC.BANDS[name]
    case = MC.case_band(name, **spec)
    p, _ = MC.params(M, case)
    exp = MC.expectations(case, p)[0]
    bz_lo, bz_hi, bz_out, _ = EI.slice_geometry(p)
    assert (bz_lo, bz_hi, bz_out) == (spec["k_lo"] >> 3, spec["k_hi"] >> 3, spec["k_out"] >> 3)
    assert exp.blocks == [(0, 0, bz_out)], "one ESDF block: none for the decoy column, whose dirty blocks lie just outside the band"
    assert any(tuple(i[:2]) == MC.DECOY for i in case.steps[0][0].tolist())
    draw = spec.get("draw", ("below", "lo", "hi", "above"))
    want = np.zeros((8, 8), bool)
    for d in draw:
        vx, vy = MC.BAND_COLUMNS[d]
        want[vy, vx] = d in ("lo", "hi")
    x0 = -exp.origin[0] * 8
    assert np.array_equal(exp.site[:8, x0:x0 + 8], want) and np.array_equal(exp.inside, exp.site) and exp.site.sum() == len(set(draw) & {"lo", "hi"})
    assert exp.observed[:8, x0:x0 + 8].all()
    tsdf_z = sorted(i[2] for i in case.steps[0][0].tolist() if tuple(i[:2]) == (0, 0))
    spans = {"one_block": 1, "one_row": 1, "default": 2, "three_blocks_hole": 3, "five_blocks_hole": 5, "across_zero": 2, "below_zero": 3, "slice_outside": 1, "63_blocks": 63}
    assert bz_hi - bz_lo + 1 == spans[name]
    if "hole" in name:
        assert not set(spec["missing"]) & set(tsdf_z) and bz_lo < min(spec["missing"]) and max(spec["missing"]) < bz_hi and tsdf_z[-1] == bz_hi
    if name == "63_blocks":
        assert tsdf_z == [bz_lo, bz_hi] == [-31, 31]
        rows = MC.band_rows(spec["k_lo"], spec["k_hi"])
        assert rows["lo"] & 7 == 0 and rows["hi"] & 7 == 7, "the first row of the lowest block, the last row of the highest"
    if name in ("across_zero", "below_zero"):
        assert p.esdf_slice_min_height < 0
    if name == "below_zero":
        assert p.esdf_slice_max_height < 0 and spec["k_lo"] & 7 == 7 and spec["k_hi"] & 7 == 0
    if name == "slice_outside":
        assert not bz_lo <= bz_out <= bz_hi


def test_refused_bands_span_what_the_update_refuses():
    M = _M()
    for name in MC.REFUSED_NAMES:
        case = MC.case_by_name(M, name)
        p, _ = MC.params(M, case, **case.refuse)
        bz_lo, bz_hi, _, _ = EI.slice_geometry(p)
        assert (bz_hi - bz_lo + 1 == 64) if "64" in name else (bz_hi < bz_lo), (name, bz_lo, bz_hi)
    p63, _ = MC.params(M, MC.case_by_name(M, "b-63_blocks"))
    assert EI.slice_geometry(p63)[1] - EI.slice_geometry(p63)[0] + 1 == 63


def test_remarking_cases():
    """The site is there after the first pass (two dirty blocks, one column), stays when the lower block is written again as it was, goes with the
    upper block; one dirty block per pass ends where two in one pass do."""
    M = _M()
    a, b = MC.case_remark(), MC.case_remark_one_at_a_time()
    p, _ = MC.params(M, a)
    ea, eb = MC.expectations(a, p), MC.expectations(b, p)
    vx, vy, _ = MC.REMARK_SITE
    x0 = -ea[0].origin[0] * 8
    for k, n in enumerate((1, 1, 0)):
        assert ea[k].site.sum() == n and bool(ea[k].site[vy, x0 + vx]) == bool(n) and ea[k].observed.all() and len(ea[k].blocks) == 2
    assert len(a.steps[0][0]) == 4 and a.steps[1][0].tolist() == [[0, 0, 0]] and a.steps[2][0].tolist() == [[0, 0, 1]]
    assert np.array_equal(a.steps[1][1][0], a.steps[0][1][a.steps[0][0].tolist().index([0, 0, 0])]), "the lower block is written again as it was"
    assert not eb[0].site.any()
    for x, y in zip(ea[0], eb[1]):
        assert np.array_equal(x, y)


def test_long_list_case():
    """576 dirty entries in one pass: however they spread over the list's eight shards, some shard holds 72 or more, over twice the 32 workers
    a 256-worker carrier gives a shard, so the worker stride loops; the drawn voxels lie on, above and below the band."""
    M = _M()
    case = MC.case_long_list()
    p, q = MC.params(M, case)
    exp = MC.expectations(case, p)[0]
    idx, data = case.steps[0]
    assert len(case.steps) == 1 and len(idx) == 576 and case.capacity == 4096 and len(exp.blocks) == 576 and 576 // 8 > 2 * (256 // 8)
    assert EI.cutoff(q)[1] == 2
    drawn = (data["distance"] == MC.SITE_D).reshape(-1, 8, 8, 8)
    per_row = drawn.sum((0, 1, 2))
    assert drawn.sum() == 24 * 24 * 64 // 100 and (per_row > 20).all(), per_row
    assert exp.site.sum() == drawn[..., 2:6].any(-1).sum() and 100 < exp.site.sum() < drawn.sum() and exp.observed.all()


def test_ground_plane_case():
    """Every drawn column's band quotients, and every block corner's, lie 1e-3 voxel or more from an integer; the band moves by 3 rows or more
    across the staircase block and crosses the block boundary at row 8 inside it; the staircase is a site in every column of its block, the
    voxels one row outside the band are none; both fall-backs expect what the fixed heights expect -- not what the plane does."""
    M = _M()
    case = MC.case_plane(M, "tilted")
    p, _ = MC.params(M, case)
    assert EI.plane_on(p)
    origin, shape = MC.case_box(case)
    assert (origin, shape) == MC.PLANE_BOX
    assert EI.band_margin(p, origin, shape) >= 1e-3, EI.band_margin(p, origin, shape)
    kz_lo, kz_hi = EI.column_bands(p, origin, shape)
    assert ((kz_hi - kz_lo) == 4).all()
    blk = lambda a, bx, by: a[(by - origin[1]) * 8:(by - origin[1]) * 8 + 8, (bx - origin[0]) * 8:(bx - origin[0]) * 8 + 8]       # noqa: E731
    hi00 = blk(kz_hi, 0, 0)
    assert hi00.max() - hi00.min() >= 3 and hi00.min() < 8 <= hi00.max(), (hi00.min(), hi00.max())
    assert blk(kz_lo, -1, -1).min() < 0, "a band below z = 0 under the plane"
    exp = MC.expectations(case, p)[0]
    assert sorted(b[:2] for b in exp.blocks) == sorted(MC.PLANE_COLUMNS)
    for (bx, by), which in MC.PLANE_COLUMNS.items():
        assert blk(exp.site, bx, by).all() == (which in ("lo", "hi")) and blk(exp.site, bx, by).any() == (which in ("lo", "hi")), (bx, by, which)
        assert blk(exp.observed, bx, by).all()
    # float32, as the kernel evaluates it, gives the same rows: the condition above is what makes this hold
    vs = F(p.voxel_size); pl = [F(v) for v in p.esdf_ground_plane]
    def centres(o, n):
        k = np.arange(8 * n)
        return ((o + k // 8).astype(F) * (vs * F(8)) + (k % 8).astype(F) * vs) + vs * F(0.5)
    xs, ys = centres(origin[0], shape[1]), centres(origin[1], shape[0])
    assert xs.dtype == F
    t = (pl[0] * xs[None, :] + pl[1] * ys[:, None]) + pl[3]
    h = -(t / pl[2])
    lo = h + F(p.slice_height_above_plane_m)
    assert lo.dtype == F
    assert np.array_equal(np.floor(lo / vs).astype(np.int64), kz_lo) and np.array_equal(np.floor((lo + F(p.slice_height_thickness_m)) / vs).astype(np.int64), kz_hi)
    fixed = MC.case_plane(M, "fixed")
    pf, _ = MC.params(M, fixed)
    want = MC.expectations(fixed, pf)[0]
    assert not EI.plane_on(pf)
    assert want.blocks != exp.blocks or not np.array_equal(want.site, exp.site), "the fixed heights see the staircase differently"
    for variant in ("flat_normal", "no_thickness"):
        c = MC.case_plane(M, variant)
        pv, _ = MC.params(M, c)
        assert pv.esdf_use_ground_plane == 1 and not EI.plane_on(pv)
        got = MC.expectations(c, pv)[0]
        assert got.blocks == want.blocks and all(np.array_equal(x, y) for x, y in zip(got[3:], want[3:])), variant
    assert F(MC.case_plane(M, "flat_normal").plane[2]) == F(1e-3)


def test_occupancy_and_3d_cases():
    """Occupancy: of the twenty drawn columns those with a non-zero value ON a band row are observed, those with a positive one sites; nothing
    else is.  3-D: each voxel by itself -- the voxel that makes a column a site under rule 1 beside a deeper one does so alone here."""
    M = _M()
    case = MC.case_occupancy()
    p, _ = MC.params(M, case)
    exp = MC.expectations(case, p)[0]
    obs = np.zeros((8, 8), bool); site = np.zeros((8, 8), bool)
    for r in (1, 2):                                     # rows kz_lo and kz_hi
        for v, lo in enumerate(MC.LOG_ODDS):
            c = 5 * r + v
            obs[c >> 3, c & 7] = lo != 0; site[c >> 3, c & 7] = lo > 0
    assert exp.blocks == [(0, 0, 0)] and np.array_equal(exp.observed, obs) and np.array_equal(exp.site, site) and np.array_equal(exp.inside, site)
    assert obs.sum() == 8 and site.sum() == 4
    for kind in ("rule0", "rule1", "occupancy"):
        c3 = MC.case_3d(kind)
        p3, _ = MC.params(M, c3)
        e3 = MC.expectations(c3, p3)[0]
        assert e3.blocks == [(0, -1, 2)] and e3.dom.all() and 0 < e3.site.sum() < e3.observed.sum() < 512
        if kind != "occupancy":
            n = len(MC.TABLE_VOXELS)
            flat = [(o, i, s0, s1) for _, vox, (o, i, s0, s1) in MC.TABLE if len(vox) == 1]
            singles = [k for k, (_, vox, _) in enumerate(MC.TABLE) if len(vox) == 1]
            pos = np.cumsum([0] + [len(vox) for _, vox, _ in MC.TABLE])
            for k, (o, i, s0, s1) in zip(singles, flat):
                v = int(pos[k])                          # the first voxel of the block that carries this entry: [x][y][z] = v
                at = (v >> 6, (v >> 3) & 7, v & 7)
                assert v < n and (bool(e3.observed[at]), bool(e3.inside[at]), bool(e3.site[at])) == (bool(o), bool(i), bool(s1 if kind == "rule1" else s0)), (kind, MC.TABLE[k][0])
