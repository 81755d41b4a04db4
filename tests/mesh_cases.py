"""What tests/test_mesh_model.py (CPU) and tests/test_gpu_mesh_drawn.py (GPU) share: TSDF fields DRAWN to reach what a rendered scene never does (all
254 cube cases, the per-block maxima, exact zeros, weights at the threshold, a surface in a block face, huge and subnormal distances, far block
indices, a sphere with an analytic truth), how a field is put into the CPU checker and into a mapper, and the assertions a meshed block meets against
the table-free model (tests/mesh_independent.py).

A field's arrays are [8, 8, 8] in (x, y, z): C order is the voxel order z + 8 y + 64 x of a block."""
import collections
import types

import numpy as np

import helpers as H
import mesh_independent as MI

M = H.M
VOXEL = 0.05
EIGHT = np.array([(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)], np.int32)      # 2 x 2 x 2 blocks around the origin
PRODUCT_LAYERS = types.SimpleNamespace(L_TSDF=M.LAYER_TSDF, L_COLOR=M.LAYER_COLOR)               # (MI.dense_layers asks its module for these two only)

# name, block indices [n, 3], per block: distance f32 [8,8,8], weight f32 [8,8,8], colour (COLOR_DT [8,8,8]) or None; parameter overrides
Field = collections.namedtuple("Field", "name idx dist weight color params")

MIN_W = np.float32(0.1)                     # the default mesh_min_weight, as the float32 the library holds
SPHERE_RADIUS_VOX = 5.3
# Off the lattice, near the common corner of the eight blocks.  Most centres leave a few sliver triangles (the sphere passing close to a lattice
# corner) whose normal is below the length cut-off of MI.expected_normals: 0 to 11 of ~660 vertices among twenty centres tried with the checker;
# this one leaves none under either normal rule, so the sphere's normals are compared without exception.
SPHERE_CENTRE_VOX = (0.1, 0.21, 0.04)
# The checker's worst |distance to the sphere's centre - R| over the sphere field's vertices, measured by tests/test_mesh_model.py
# (test_sphere_field_analytic): 1.1554e-3 m = 0.0231 voxels under both rule pairs.  (Linear interpolation of |x - c| along a unit edge errs by at
# most 1/8 of its second derivative, 1 / (8 R) = 0.0236 voxels.)  The GPU test allows twice the measured value.
SPHERE_CHECKER_WORST_M = 1.16e-3


def _cut(dense, idx, lo):
    out = []
    for i in np.asarray(idx):
        o = (i - lo) * 8
        out.append(np.ascontiguousarray(dense[o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8]))
    return out


def random_colors(rng, idx, without=None):
    """random RGB, colour weight 0 on about 30 % of the voxels (grey 127 there); block `without` has no colour block at all"""
    out = []
    for k in range(len(idx)):
        c = np.zeros((8, 8, 8), M.COLOR_DT)
        for ch in "rgb":
            c[ch] = rng.integers(0, 256, (8, 8, 8), dtype=np.uint8)
        c["weight"] = np.where(rng.random((8, 8, 8)) < 0.3, 0.0, rng.uniform(0.5, 5.0, (8, 8, 8))).astype(np.float32)
        out.append(None if k == without else c)
    return out


def _box(idx):
    idx = np.asarray(idx, np.int32); lo = idx.min(0)
    return idx, lo, tuple(((idx.max(0) - lo + 1) * 8).tolist())


def _random_distance(rng, shape):
    return (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(0.01, 0.2, shape)).astype(np.float32)


def random_field(idx=EIGHT, seed=3, name="random", without_color=5):
    """random sign, |d| in U(0.01, 0.2), w = 1: every cube case"""
    rng = np.random.default_rng(seed)
    idx, lo, shape = _box(idx)
    d = _random_distance(rng, shape)
    return Field(name, idx, _cut(d, idx, lo), _cut(np.ones(shape, np.float32), idx, lo), random_colors(rng, idx, without_color), {})


def checkerboard_field():
    """+-0.1 by the parity of x + y + z: every lattice edge carries a vertex (1944 in a block with all its neighbours, 2048 triangles), every t
    is exactly 0.5 (the colour tie goes to the far end)"""
    rng = np.random.default_rng(4)
    idx, lo, shape = _box(EIGHT)
    g = np.indices(shape).sum(0)
    d = np.where(g % 2 == 0, np.float32(0.1), np.float32(-0.1)).astype(np.float32)
    return Field("checkerboard", idx, _cut(d, idx, lo), _cut(np.ones(shape, np.float32), idx, lo), random_colors(rng, idx, 2), {})


def zeros_field():
    """the random field with 15 % of the distances exactly 0.0 and 5 % exactly -0.0 (both count as outside; t = 0 puts vertices on lattice
    corners: degenerate triangles, zero normals)"""
    rng = np.random.default_rng(5)
    idx, lo, shape = _box(EIGHT)
    d = _random_distance(rng, shape)
    u = rng.random(shape)
    d[u < 0.15] = np.float32(0.0); d[(u >= 0.15) & (u < 0.20)] = np.float32(-0.0)
    assert np.signbit(d[(u >= 0.15) & (u < 0.20)]).all()
    return Field("zeros", idx, _cut(d, idx, lo), _cut(np.ones(shape, np.float32), idx, lo), random_colors(rng, idx, 0), {})


def weights_field():
    """random distances; weights drawn from {the float32 just below mesh_min_weight, mesh_min_weight itself, 1}"""
    rng = np.random.default_rng(6)
    idx, lo, shape = _box(EIGHT)
    d = _random_distance(rng, shape)
    w = rng.choice(np.array([np.nextafter(MIN_W, np.float32(0)), MIN_W, 1.0], np.float32), shape, p=[0.04, 0.48, 0.48]).astype(np.float32)
    return Field("weights", idx, _cut(d, idx, lo), _cut(w, idx, lo), random_colors(rng, idx, 7), {})


def min_weight_zero_field():
    """mesh_min_weight = 0 (the kernel's other neighbour lookup): the random field's distances, 10 % of the weights 0 -- which pass"""
    rng = np.random.default_rng(3)
    idx, lo, shape = _box(EIGHT)
    d = _random_distance(rng, shape)
    w = np.where(np.random.default_rng(7).random(shape) < 0.1, 0.0, 1.0).astype(np.float32)
    return Field("min_weight_zero", idx, _cut(d, idx, lo), _cut(w, idx, lo), random_colors(rng, idx, 5), {"mesh_min_weight": 0.0})


FACE_A, FACE_B = (0, 0, 0), (1, 0, 0)


def face_field():
    """block A all +0.1, block B = A + x all -0.1: the surface lies in the shared face; A has no negative voxel of its own"""
    rng = np.random.default_rng(8)
    idx = np.array([FACE_A, FACE_B], np.int32)
    one = np.ones((8, 8, 8), np.float32)
    return Field("face", idx, [one * np.float32(0.1), one * np.float32(-0.1)], [one, one], random_colors(rng, idx), {})


def _two_valued_field(name, seed, neg, pos, without):
    rng = np.random.default_rng(seed)
    idx, lo, shape = _box(EIGHT)
    d = np.where(rng.random(shape) < 0.5, np.float32(neg), np.float32(pos)).astype(np.float32)
    return Field(name, idx, _cut(d, idx, lo), _cut(np.ones(shape, np.float32), idx, lo), random_colors(rng, idx, without), {})


def huge_field():
    """d in {-1e-30, +1e30}: t is 0 or 1 after rounding (vertices on corners, zero normals), nothing overflows"""
    return _two_valued_field("huge", 9, -1e-30, 1e30, 3)


def subnormal_field():
    """d in {-1e-42, +1e-42}, float32 subnormals: the sign test and the division must not flush them (t = 0.5 exactly)"""
    f = _two_valued_field("subnormal", 10, -1e-42, 1e-42, 4)
    assert all((b != 0).all() and (np.abs(b) < np.finfo(np.float32).tiny).all() for b in f.dist)
    return f


FAR = np.array([(3000, -3000, 3000), (3001, -3000, 3000)], np.int32)


def far_field():
    """two random blocks far from the origin, one index negative: block index arithmetic and the float32 positions out there"""
    return random_field(FAR, seed=11, name="far", without_color=None)


def sphere_centre_m():
    return np.array(SPHERE_CENTRE_VOX, np.float64) * VOXEL


def sphere_field():
    """d = |x - c| - R at the voxel centres, truncated to +-4 voxels; w = 1 where |d| < 4 voxels, else 0 (R = 5.3 voxels: the core is unobserved)"""
    rng = np.random.default_rng(12)
    idx, lo, shape = _box(EIGHT)
    x = (np.stack(np.indices(shape), -1) + lo * 8 + 0.5) * VOXEL
    raw = np.linalg.norm(x - sphere_centre_m(), axis=-1) - SPHERE_RADIUS_VOX * VOXEL
    d = np.clip(raw, -4 * VOXEL, 4 * VOXEL).astype(np.float32)
    w = (np.abs(raw) < 4 * VOXEL).astype(np.float32)
    return Field("sphere", idx, _cut(d, idx, lo), _cut(w, idx, lo), random_colors(rng, idx, 6), {})


FIELDS = {f.__name__[:-len("_field")]: f for f in (random_field, checkerboard_field, zeros_field, weights_field, min_weight_zero_field, face_field,
                                                   huge_field, subnormal_field, far_field, sphere_field)}
RULES_RANDOM = [(a, n) for a in (0, 1, 2) for n in (0, 1)]          # (ambiguity rule, normal rule): all six on the random field
RULES_OTHER = [(0, 0), (1, 1)]                                      # the defaults and one other pair everywhere else
CASES = [("random", a, n) for a, n in RULES_RANDOM] + [(name, a, n) for name in FIELDS if name != "random" for a, n in RULES_OTHER]
CASES.insert(CASES.index(("zeros", 1, 1)), ("zeros", 0, 1))         # (both normal rules under the table the zeros field's shares below were measured with)
# The share of a field's vertices that the length cut-off of MI.expected_normals may keep out of the normal comparison, per normal rule.  The
# zeros field's bounds hold under ambiguity rule 0, where the checker alone excludes 8.6 % and 0.9 % (tests/test_mesh_model.py prints them); which
# vertices fall below the cut-off is a property of the field and the triangle table (under table 1 the checker excludes 4.1 % with normal rule
# 1), so under the other tables a mesh is held to the checker's own share of the same case (assert_normal_shares).
NORMALS_EXCLUDED_MAX = {"zeros": (0.10, 0.02), "random": (0.0, 0.0), "checkerboard": (0.0, 0.0), "sphere": (0.0, 0.0), "far": (0.0, 0.0)}
NORMALS_EXCLUDED_OVER_CHECKER = 0.005                                 # vertices whose length sits at the cut-off, one float32 spacing apart
NORMALS_NOT_COMPARED = ("huge",)


def case_id(c):
    return "%s-a%d-n%d" % c


def params(field, ambiguity_rule=0, normal_rule=0, **kw):
    over = dict(field.params); over.update(kw)
    return M.default_params(voxel_size=VOXEL, mesh_ambiguity_rule=ambiguity_rule, mesh_normal_rule=normal_rule, **over)


def tsdf_blocks(field):
    out = np.zeros((len(field.idx), 512), M.TSDF_DT)
    for k in range(len(field.idx)):
        out[k]["distance"] = field.dist[k].reshape(512); out[k]["weight"] = field.weight[k].reshape(512)
    return out


def color_blocks(field):
    keep = [k for k in range(len(field.idx)) if field.color[k] is not None]
    return field.idx[keep], np.stack([field.color[k].reshape(512) for k in keep]) if keep else np.zeros((0, 512), M.COLOR_DT)


def into_oracle(oracle_mod, pg, field, o=None):
    o = o or oracle_mod.OracleMap(H.copy_params(pg, oracle_mod.OrcParams))
    for i, b in zip(field.idx.tolist(), tsdf_blocks(field)):
        o.set_block(oracle_mod.L_TSDF, i, b)
    for i, b in zip(*color_blocks(field)):
        o.set_block(oracle_mod.L_COLOR, i.tolist(), b)
    return o


def into_mapper(pg, field, block_capacity=1 << 12):
    g = M.Mapper(pg, block_capacity=block_capacity)
    set_blocks(g, field)
    return g


def set_blocks(g, field):
    g.set_blocks(M.LAYER_TSDF, field.idx, tsdf_blocks(field))
    ci, cb = color_blocks(field)
    if len(ci):
        g.set_blocks(M.LAYER_COLOR, ci, cb)


def dense_of(m, oracle_mod=None):
    """A map's own TSDF and colour layers (the checker's with its module, a mapper's without) as the dense arrays MI.expected_block takes."""
    return MI.dense_layers(m, oracle_mod or PRODUCT_LAYERS)


def expected(dense, i, pg):
    ti, lo, d, w, has, col, cw = dense
    return MI.expected_block(np.asarray(i), lo, d, w, has, col, cw, float(pg.voxel_size), float(pg.mesh_min_weight))


def cube_case_histogram(dense, pg):
    """the cube cases among the active cubes of all blocks of a map"""
    ti, lo, d = dense[0], dense[1], dense[2]
    hist = np.zeros(256, np.int64)
    for i in ti:
        hist += MI.cube_cases(MI.lattice(i, lo, d) < 0, expected(dense, i, pg)[3])
    return hist


Stats = collections.namedtuple("Stats", "vertices triangles not_bit_identical normals_compared normals_excluded zero_normals checker_excluded")


def add_stats(a, b):
    return Stats(*[x + y for x, y in zip(a, b)])


NO_STATS = Stats(0, 0, 0, 0, 0, 0, 0)


def assert_block(tag, mb, exp, pg, checker=None, bit_exact=False, compare_normals=True):
    """One meshed block (dict of vertices, normals, colors, triangles) against the model's (edge ids, positions, colours, active cubes):
      1. as many vertices, in the model's order; the triangles of `checker` (the checker's mesh of the block), where given, equal; every triangle's
         three lattice edges share an active cube of the block and every active cube has a triangle,
      2. every coordinate within one float32 spacing of the model's (all bits, with bit_exact),
      3. the model's colours, alpha 255,
      4. normals finite, of length 1 +- 1e-5 or exactly 0; within 2e-4 of the float64 recomputation from the block's own vertices where that one's
         unnormalised length is above the cut-off (compare_normals)."""
    eids, pos, cols, active = exp
    v, t, nrm, c = mb["vertices"], mb["triangles"], mb["normals"], mb["colors"]
    assert len(v) == len(eids) and len(nrm) == len(v) and len(c) == len(v), (tag, "vertex count", len(v), len(eids))
    if checker is not None:
        assert np.array_equal(t, checker["triangles"]), (tag, "triangles differ from the checker's", len(t), len(checker["triangles"]))
    if len(v) == 0:
        assert len(t) == 0 and not active.any(), (tag, "no vertex, yet triangles or active cubes")
        return NO_STATS
    assert t.min() >= 0 and t.max() < len(v), (tag, "triangle index out of range")
    inside, seen = MI.triangle_edge_cubes(eids, t, active)
    assert inside.all(), (tag, "triangles whose three edges share no active cube", np.nonzero(~inside)[0][:5].tolist())
    assert np.array_equal(seen, active), (tag, "active cubes without a triangle", np.argwhere(seen != active)[:5].tolist())
    v = np.ascontiguousarray(v, np.float32); pos = np.ascontiguousarray(pos, np.float32)
    not_bits = int((v.view(np.uint32) != pos.view(np.uint32)).sum())
    off = np.abs(v.astype(np.float64) - pos.astype(np.float64)) > np.spacing(np.abs(pos)).astype(np.float64)
    assert not off.any(), (tag, "vertex position", np.argwhere(off)[:5].tolist(), v[off][:5].tolist(), pos[off][:5].tolist())
    assert not (bit_exact and not_bits), (tag, "coordinates not bit-identical to the model's", not_bits)
    assert np.array_equal(c[:, :3], cols), (tag, "colours", np.argwhere(c[:, :3] != cols)[:5].tolist())
    assert (c[:, 3] == 255).all(), (tag, "alpha")
    assert np.isfinite(nrm).all(), (tag, "a normal is not finite")
    ln = np.linalg.norm(nrm.astype(np.float64), axis=1)
    zero = ~nrm.any(1)
    assert ((np.abs(ln - 1.0) <= 1e-5) | zero).all(), (tag, "a normal is neither of unit length nor exactly 0", ln[(np.abs(ln - 1.0) > 1e-5) & ~zero][:5].tolist())
    n_cmp = n_exc = n_chk = 0
    if compare_normals:
        want, mask = MI.expected_normals(v, t, int(pg.mesh_normal_rule), float(pg.voxel_size))
        err = np.abs(nrm[mask].astype(np.float64) - want[mask]).max(initial=0.0)
        assert err <= 2e-4, (tag, "normals differ from the float64 recomputation by", float(err))
        n_cmp, n_exc = int(mask.sum()), int((~mask).sum())
        if checker is not None:
            n_chk = int((~MI.expected_normals(checker["vertices"], checker["triangles"], int(pg.mesh_normal_rule), float(pg.voxel_size))[1]).sum())
    return Stats(len(v), len(t), not_bits, n_cmp, n_exc, int(zero.sum()), n_chk)


def assert_normal_shares(tag, field_name, ambiguity_rule, normal_rule, stats, against_checker=False):
    """the share of vertices the length cut-off kept out of the normal comparison, against what the field allows (NORMALS_EXCLUDED_MAX) and,
    for a mesh that was compared with the checker's, against the checker's own share"""
    if field_name in NORMALS_EXCLUDED_MAX and stats.vertices:
        share = stats.normals_excluded / stats.vertices
        bound = NORMALS_EXCLUDED_MAX[field_name][normal_rule]
        if ambiguity_rule == 0 or bound == 0.0:
            assert share <= bound, (tag, "share of normals below the length cut-off", share)
        if against_checker:
            assert share <= stats.checker_excluded / stats.vertices + NORMALS_EXCLUDED_OVER_CHECKER, (tag, "share below the cut-off, the checker's", share, stats.checker_excluded / stats.vertices)


def sphere_checks(tag, meshes):
    """The sphere field's mesh against the analytic sphere: meshes = {block: dict(vertices, triangles)}.  Every triangle faces outward (positive dot
    product of its normal with the radial direction at its centroid); the mesh over all blocks is closed -- welded by vertex position, which is
    bit-identical for the two blocks that share a lattice edge here (block sizes and voxel offsets are exact in float32 at these indices), every
    edge has exactly two triangles.  -> the worst |distance to the centre - R| over the vertices, metres."""
    c = sphere_centre_m(); R = SPHERE_RADIUS_VOX * VOXEL
    vs, ts, base = [], [], 0
    for key in sorted(meshes):
        v, t = np.asarray(meshes[key]["vertices"]), np.asarray(meshes[key]["triangles"])
        vs.append(v); ts.append(t.astype(np.int64) + base); base += len(v)
    v = np.concatenate(vs); t = np.concatenate(ts)
    assert len(v) > 300 and len(t) > 600, (tag, "the sphere has no mesh to speak of", len(v), len(t))
    worst = float(np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - R).max())
    p = v.astype(np.float64)[t]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    dots = (fn * (p.mean(1) - c)).sum(1)
    assert (dots > 0).all(), (tag, "triangles facing inward", int((dots <= 0).sum()))
    _, welded = np.unique(v, axis=0, return_inverse=True)
    w = welded.reshape(-1)[t]
    assert (w[:, 0] != w[:, 1]).all() and (w[:, 1] != w[:, 2]).all() and (w[:, 0] != w[:, 2]).all(), (tag, "degenerate triangles")
    e = np.sort(np.concatenate([w[:, [0, 1]], w[:, [1, 2]], w[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all(), (tag, "the welded mesh is not closed: edges by triangle count", np.bincount(counts).tolist())
    return worst
