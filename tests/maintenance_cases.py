"""What tests/test_maintenance_model.py (CPU, against the checker) and tests/test_gpu_maintenance_drawn.py (GPU, against the product) share: the
maps drawn to break decay and clearing, the two sides a drawn map is put through, and the step that applies the model (tests/maintenance_independent.py)
to the map AS READ BACK BEFORE a call and compares it with the read-back after it.

A case is (name, parameter overrides, drawn state, steps, verify).  `verify(trace)` asserts FROM THE MODEL ALONE that the case is not vacuous
(trace = model_trace(case, params): the model run on the drawn state), so the conditions hold on a machine without a GPU.

  A  weight ladder (TSDF decay): 640 lattice blocks with negative indices -- 512 whose sole survivor of the first call is voxel (37 b) % 512 (every
     (lane, register) position of k_decay once) and 128 without a survivor -- plus one block of weights on and around the threshold, two
     blocks that live or die by such a voxel alone, and colour-only blocks.
  B  log-odds ladder (occupancy decay).     C  radius boundary: d2 == r2 stays, the next float32 goes.     D  shape boundary.
"""
import collections

import numpy as np

import maintenance_independent as MM

F = np.float32
VOXEL = 0.05
Case = collections.namedtuple("Case", "name kw state steps verify")
INF = F(np.inf)


def _keys(xs, ys, zs):
    return [(x, y, z) for x in xs for y in ys for z in zs]


def _tsdf(d, w):
    b = np.zeros(512, MM.TSDF_DT); b["distance"] = d; b["weight"] = w
    return b


def _color(rng, weight=1.0):
    c = np.zeros(512, MM.COLOR_DT)
    for f in "rgb":
        c[f] = rng.integers(0, 256, 512)
    c["weight"] = weight
    return c


# ------------------------------------------------------------------------------------------------ A: the weight ladder
DECAY_RUNS = {"dyadic": (0.5, 0.25, (0.5, 1.5, 8.0, 100.0), 0.49), "odd": (0.45, 0.3, (0.7, 1.6, 8.0, 100.0), 0.66)}
DECAY_VARIANTS = {"default": {}, "free": dict(tsdf_set_free_distance_on_decayed=1, tsdf_decayed_free_distance_vox=3.0), "keep": dict(decay_deallocate_decayed_blocks=0),
                  "free_keep": dict(tsdf_set_free_distance_on_decayed=1, tsdf_decayed_free_distance_vox=3.0, decay_deallocate_decayed_blocks=0)}
LADDER_KEYS = _keys(range(-5, 5), range(-4, 4), range(-4, 4))          # 640
SPECIAL, EXACT_ONLY, BELOW_ONLY = (7, -7, 2), (7, -6, 2), (7, -5, 2)
COLOR_ONLY = [(-9, k, 5) for k in range(-4, 4)]


def threshold_weights(f, thr):
    """(exact, below): every float32 w around thr / f with float32(w * f) == thr, and the next float32 below them -- found by stepping"""
    f, thr = F(f), F(thr)
    w = F(thr / f)
    while not F(w * f) < thr:
        w = np.nextafter(w, -INF)
    below = w
    exact = []
    w = np.nextafter(w, INF)
    while F(w * f) == thr:
        exact.append(w); w = np.nextafter(w, INF)
    assert exact, "no float32 weight decays onto the threshold"
    return exact, below


def case_a(run, variant):
    f, thr, live_w, low_max = DECAY_RUNS[run]
    rng = np.random.default_rng(11)
    state = {}
    for b, key in enumerate(LADDER_KEYS):
        w = rng.uniform(0.0, low_max, 512).astype(F)
        w[rng.random(512) < 0.2] = 0
        d = rng.uniform(-0.2, 0.2, 512).astype(F)
        if b < 512:
            w[(37 * b) % 512] = live_w[b % 4]
        state[key] = MM.make_block(tsdf=_tsdf(d, w), color=_color(rng) if b % 3 == 0 else None)
    exact, below = threshold_weights(f, thr)
    w = np.zeros(512, F)
    edge = list(exact) + [below, F(0), F(-0.0), F(1e-40), F(-1.0), INF, F(np.nan)]
    for k in range(512):
        w[k] = edge[k % len(edge)]
    state[SPECIAL] = MM.make_block(tsdf=_tsdf(rng.uniform(-0.2, 0.2, 512).astype(F), w), color=_color(rng))
    for key, v in ((EXACT_ONLY, exact[0]), (BELOW_ONLY, below)):
        w = np.zeros(512, F); w[511] = v                                        # lane 63, register 7
        state[key] = MM.make_block(tsdf=_tsdf(np.full(512, 0.1, F), w))
    for key in COLOR_ONLY:
        state[key] = MM.make_block(color=_color(rng))
    kw = dict(tsdf_decay_factor=f, tsdf_decayed_weight_threshold=thr, **DECAY_VARIANTS[variant])
    steps = [("update_esdf",)] + [("decay_tsdf", False)] * 4
    deallocates = "keep" not in variant

    def verify(trace):
        calls = [t for t in trace if t[0][0] == "decay_tsdf"]
        assert len(calls) == 4
        before = calls[0][1]
        seen = np.zeros(512, bool); none = 0
        for b, key in enumerate(LADDER_KEYS):
            w0 = before[key]["tsdf"]["weight"]
            live = ~((w0 * F(f)).astype(F) < F(thr))
            if b < 512:
                assert live.sum() == 1 and live[(37 * b) % 512], (key, "one survivor, at (37 b) % 512")
                seen[(37 * b) % 512] = True
            else:
                assert not live.any(); none += 1
        assert seen.all(), "every (lane, register) position is the sole survivor of some block"
        assert none >= 100
        last = calls[3][2]
        four = sum(1 for key in LADDER_KEYS if key in last and last[key]["tsdf"] is not None and (~(last[key]["tsdf"]["weight"] < F(thr))).any())
        assert four >= 100, four
        after1 = calls[0][2]
        if deallocates:
            assert BELOW_ONLY not in after1 and EXACT_ONLY in after1 and len(calls[0][3]) >= 100 and len(calls[1][3]) >= 100
        else:
            assert all(len(c[3]) == 0 for c in calls) and BELOW_ONLY in last
        sp = before[SPECIAL]["tsdf"]["weight"]
        assert np.isnan(sp).any() and np.isinf(sp).any() and (MM.bits(sp) == 0x80000000).any() and ((sp > 0) & (sp < F(1e-38))).any() and (sp < 0).any()
        assert SPECIAL in last and np.isnan(last[SPECIAL]["tsdf"]["weight"]).any()
        if "free" in variant:
            n = sum(int(((c[2][k]["tsdf"]["distance"] == F(3.0) * F(VOXEL)) & (c[2][k]["tsdf"]["weight"] == F(thr))).sum()) for c in calls[:1] for k in c[2] if c[2][k]["tsdf"] is not None)
            assert n > 10000, n
        assert all(k in last and last[k]["tsdf"] is None for k in COLOR_ONLY)
    return Case("A-%s-%s" % (run, variant), kw, state, steps, verify)


# ------------------------------------------------------------------------------------------------ B: the log-odds ladder
OCC = dict(projective_layer_type=1, free_region_decay_probability=0.55, occupied_region_decay_probability=0.30)
OCC_VARIANTS = {"default": {}, "to_free": dict(occupancy_decay_to_free=1), "keep": dict(decay_deallocate_decayed_blocks=0)}
OCC_KEYS = _keys(range(0, 5), range(-2, 3), range(0, 2))               # 50


def case_b(variant):
    s_free, s_occ = MM.log_odds(OCC["free_region_decay_probability"]), MM.log_odds(OCC["occupied_region_decay_probability"])
    assert s_free > 0 > s_occ
    up = lambda v: np.nextafter(F(v), INF)                                 # noqa: E731
    dn = lambda v: np.nextafter(F(v), -INF)                                # noqa: E731
    ladder = []
    for s in (-s_occ, -s_free):                                            # +step of the occupied rule, -step of the free rule
        ladder += [s, up(s), dn(s), F(2) * s, up(F(2) * s), dn(F(2) * s)]
    ladder += [F(10), F(-10), F(0), F(-0.0), F(1e-40), F(-1e-40), F(3.3), F(-0.7)]
    ladder = np.asarray(ladder, F)
    state = {}
    for b, key in enumerate(OCC_KEYS):
        kind = b % 5
        if kind == 0:
            v = np.roll(np.resize(ladder, 512), b)
        elif kind == 1:
            v = np.zeros(512, F)                                           # all unknown: deallocated by the first call
        elif kind == 2:
            v = np.zeros(512, F); v[(37 * b) % 512] = -s_occ               # one voxel, exactly one step from 0
        elif kind == 3:
            v = np.zeros(512, F); v[(37 * b) % 512] = F(2) * (-s_free); v[5] = dn(-s_free)      # gone after two calls
        else:
            v = np.zeros(512, F); v[b] = F(10); v[511 - b] = F(-10)
        state[key] = MM.make_block(occ=v)
    kw = dict(OCC, **OCC_VARIANTS[variant])
    steps = [("update_esdf",)] + [("decay_occupancy",)] * 4

    def verify(trace):
        calls = [t for t in trace if t[0][0] == "decay_occupancy"]
        first, last = calls[0], calls[3]
        if variant == "keep":
            assert all(len(c[3]) == 0 for c in calls) and len(last[2]) == len(OCC_KEYS)
        else:
            assert len(first[3]) >= 10 and len(calls[1][3]) >= (10 if variant == "default" else 0) and len(last[2]) >= 10
        b0 = first[1][OCC_KEYS[0]]["occ"]; a0 = first[2][OCC_KEYS[0]]["occ"]
        hit0 = (b0 != 0) & (a0 == 0)
        assert (hit0 & (b0 == -s_occ)).any() and ((b0 == up(-s_occ)) & (a0 > 0)).any(), "a value exactly one step above 0 lands on 0, the next float32 does not"
        assert variant == "to_free" or (hit0 & (b0 == dn(-s_occ))).any(), "the float32 below one step stops at 0"
        if variant == "to_free":
            assert (a0[b0 == dn(-s_occ)] < 0).all() and np.array_equal(MM.bits(a0[b0 < 0]), MM.bits(b0[b0 < 0])), "occupied decays past 0, free is not decayed"
        else:
            assert (hit0 & (b0 == -s_free)).any() and (hit0 & (b0 == up(-s_free))).any() and ((b0 == dn(-s_free)) & (a0 < 0)).any()
        assert (last[2][OCC_KEYS[4]]["occ"] > 0).any()
    return Case("B-" + variant, kw, state, steps, verify)


# ------------------------------------------------------------------------------------------------ C: the radius boundary
RADIUS_KEYS = _keys(range(-4, 5), range(-4, 5), range(-3, 4))           # 567
RADIUS_COLOR_ONLY = [(9, 9, 9), (-9, 2, 1)]


def radius_for(d2):
    """a float32 r with float32(r * r) == d2, or None"""
    r = F(np.sqrt(F(d2)))
    for _ in range(3):
        r = np.nextafter(r, F(0))
    for _ in range(7):
        if F(r * r) == d2:
            return r
        r = np.nextafter(r, INF)
    return None


def search_radius_boundary(keys, voxel_size=VOXEL, lo=0.8, hi=2.2):
    """(centre, r): some block of `keys` has d2 == float32(r * r) and another d2 == the next float32 above it -- searched, not derived: the
    centre's x steps through small float32 values until two blocks mirrored about it come to lie one ulp apart and the lower d2 is a square"""
    for k in range(1, 20000):
        c = (F(k) * F(2.0 ** -27), F(0.13), F(-0.35))
        u = np.unique(MM.block_d2(keys, c, voxel_size))
        for i in np.nonzero(u[1:] == np.nextafter(u[:-1], INF))[0]:
            if lo < u[i] < hi:
                r = radius_for(u[i])
                if r is not None:
                    return tuple(float(v) for v in c), float(r)
    raise AssertionError("no centre / radius with two blocks one ulp apart")


def case_c(run):
    rng = np.random.default_rng(13)
    state = {}
    for b, key in enumerate(RADIUS_KEYS):
        state[key] = MM.make_block(tsdf=_tsdf(rng.uniform(-0.2, 0.2, 512).astype(F), rng.uniform(0.0, 5.0, 512).astype(F)), color=_color(rng) if b % 4 == 0 else None)
    for key in RADIUS_COLOR_ONLY:
        state[key] = MM.make_block(color=_color(rng))
    if run == "boundary":
        c, r = search_radius_boundary(RADIUS_KEYS)
    else:
        c, r = (100.0, 100.0, 100.0), 0.01                                   # everything goes
    steps = [("update_esdf",), ("clear_outside_radius", c, r)]

    def verify(trace):
        t = [x for x in trace if x[0][0] == "clear_outside_radius"][0]
        before, after, cleared = t[1], t[2], t[3]
        assert 512 < len(before) < 700
        gone = {tuple(k) for k in cleared.tolist()}
        assert not gone & set(RADIUS_COLOR_ONLY) and not set(RADIUS_COLOR_ONLY) & set(after), "the colour-only blocks go, and are not reported"
        if run == "boundary":
            r2 = F(F(r) * F(r))
            d2 = MM.block_d2(RADIUS_KEYS, c, VOXEL)
            on, above = d2 == r2, d2 == np.nextafter(r2, INF)
            assert on.any() and above.any()
            assert all(RADIUS_KEYS[i] in after for i in np.nonzero(on)[0]) and all(RADIUS_KEYS[i] in gone for i in np.nonzero(above)[0])
            assert len(after) > 100 and len(gone) > 100
        else:
            assert not after and len(gone) == len(RADIUS_KEYS)
    return Case("C-" + run, {}, state, steps, verify)


# ------------------------------------------------------------------------------------------------ D: the shape boundary
SHAPE_KEYS = _keys(range(-1, 2), range(-1, 2), range(0, 2))             # 18


def _centre(key, v):
    return MM.voxel_centres(key, VOXEL)[v]


def _sphere_on_a_voxel(centre_of):
    """(sphere centre, r, (key, voxel)): a voxel centre at d2 == float32(r * r) exactly from the sphere's centre -- searched over the voxels of a block"""
    c = np.asarray(centre_of, F)
    for key in ((0, 0, 0), (0, 0, 1), (1, 0, 0)):
        p = MM.voxel_centres(key, VOXEL)
        d = [(p[:, a] - c[a]).astype(F) for a in range(3)]
        d2 = (((d[0] * d[0]).astype(F) + (d[1] * d[1]).astype(F)).astype(F) + (d[2] * d[2]).astype(F)).astype(F)
        for v in np.argsort(d2):
            if d2[v] > F(0.01):
                r = radius_for(d2[v])
                if r is not None:
                    return c, r, (key, int(v))
    raise AssertionError("no voxel centre at a float32 square from the sphere's centre")


def case_d(variant, occupancy=False):
    """variant: "on" (the boundary voxels are inside), "off" (radius and faces moved by one float32: they are outside), "none" (no shape)"""
    rng = np.random.default_rng(17)
    state = {}
    for key in SHAPE_KEYS:
        if occupancy:
            state[key] = MM.make_block(occ=rng.uniform(0.5, 3.0, 512).astype(F) * np.where(rng.random(512) < 0.5, F(1), F(-1)))
        else:
            state[key] = MM.make_block(tsdf=_tsdf(rng.uniform(0.01, 0.2, 512).astype(F), rng.uniform(1.0, 5.0, 512).astype(F)), color=_color(rng))
    if not occupancy:
        state[(5, 5, 5)] = MM.make_block(color=_color(rng))
    sc, r, target = _sphere_on_a_voxel((0.1130, 0.0870, 0.2210))
    lo_v, hi_v = ((-1, 0, 0), 2 * 64 + 2 * 8 + 1), ((0, 0, 0), 2 * 64 + 6 * 8 + 5)            # the box: from one voxel centre to another, both faces on centres
    lo, hi = _centre(*lo_v), _centre(*hi_v)
    if variant == "off":
        r = np.nextafter(r, F(0)); lo = np.nextafter(lo, INF); hi = np.nextafter(hi, -INF)
    shapes = [("sphere", tuple(float(v) for v in sc), float(r)), ("aabb", tuple(float(v) for v in lo), tuple(float(v) for v in hi))]
    # fifteen small spheres, the last of them (the 17th shape: the second launch) alone around its voxels
    for k in range(15):
        p = _centre(SHAPE_KEYS[k + 1], (97 * k + 5) % 512)
        shapes.append(("sphere", tuple(float(v) for v in p), 0.06))
    if variant == "none":
        shapes = []
    steps = [("update_esdf",), ("clear_shapes", shapes)]

    def verify(trace):
        t = [x for x in trace if x[0][0] == "clear_shapes"][0]
        before, after = t[1], t[2]
        layer = "occ" if occupancy else "tsdf"

        def reset(key, v, st=after):
            b = st[key][layer]
            return (b[v] == 0) if occupancy else (b["distance"][v] == 0 and b["weight"][v] == 0)
        assert len(t[3]) == 0 and set(after) == set(before)
        if variant == "none":
            for k in before:
                for f in ("tsdf", "occ", "color"):
                    assert (before[k][f] is None) == (after[k][f] is None) and (before[k][f] is None or before[k][f].tobytes() == after[k][f].tobytes()), (k, f)
            return
        assert len(shapes) == 17
        want = variant == "on"
        assert bool(reset(*target)) == want and bool(reset(*lo_v)) == want and bool(reset(*hi_v)) == want, "the boundary voxels"
        inner = ((0, 0, 0), 0 * 64 + 4 * 8 + 2)                                          # well inside the box
        assert reset(*inner)
        both = MM.shape_mask((0, 0, 0), shapes[:1], VOXEL) & MM.shape_mask((0, 0, 0), shapes[1:2], VOXEL)
        assert both.any(), "sphere and box overlap"
        without_last = MM.clear_shapes(before, shapes[:16], VOXEL)[0]
        k17 = SHAPE_KEYS[15]
        m17 = MM.shape_mask(k17, shapes[16:], VOXEL) & ~MM.shape_mask(k17, shapes[:16], VOXEL)
        assert m17.any() and all(reset(k17, v) and not reset(k17, v, without_last) for v in np.nonzero(m17)[0]), "the 17th shape alone resets a voxel"
        n = MM.shape_touched(before, shapes, VOXEL)[1]
        assert 100 < n < 512 * len(SHAPE_KEYS) // 2, n                     # (many voxels reset, most of the map untouched)
    return Case("D-%s%s" % (variant, "-occupancy" if occupancy else ""), dict(OCC) if occupancy else {}, state, steps, verify)


CASE_NAMES = ["A-dyadic-default", "A-dyadic-free", "A-dyadic-keep", "A-dyadic-free_keep", "A-odd-default", "A-odd-free", "B-default", "B-to_free", "B-keep",
              "C-boundary", "C-everything", "D-on", "D-off", "D-none", "D-on-occupancy"]


def case_by_name(name):
    p = name.split("-")
    if p[0] == "A":
        return case_a(p[1], p[2])
    if p[0] == "B":
        return case_b(p[1])
    if p[0] == "C":
        return case_c(p[1])
    return case_d(p[1], occupancy=len(p) > 2)


def params(M, case, **more):
    return M.default_params(voxel_size=VOXEL, **dict(case.kw, **more))


# ------------------------------------------------------------------------------------------------ the model alone


def apply_model(state, step, p, spared=()):
    op = step[0]
    if op == "decay_tsdf":
        return MM.decay_tsdf(state, spared if step[1] else (), p)
    if op == "decay_occupancy":
        return MM.decay_occupancy(state, p)
    if op == "clear_outside_radius":
        return MM.clear_outside_radius(state, step[1], step[2], p.voxel_size)
    if op == "clear_shapes":
        return MM.clear_shapes(state, step[1], p.voxel_size)
    raise ValueError(op)


def model_trace(case, p):
    """[(step, state before, state after, cleared)] of the model on the drawn state (update_esdf, which the model does not know, is skipped)"""
    state = case.state; out = []
    for step in case.steps:
        if step[0] == "update_esdf":
            continue
        new, cleared = apply_model(state, step, p)
        out.append((step, state, new, cleared)); state = new
    return out


# ------------------------------------------------------------------------------------------------ the two sides


def state_from_read(read):
    state = {}

    def blk(key):
        return state.setdefault(tuple(int(v) for v in key), MM.make_block())
    for layer in ("tsdf", "occ", "color"):
        if layer in read:
            idx, vox = read[layer]
            for k, key in enumerate(np.asarray(idx).reshape(-1, 3)):
                blk(key)[layer] = np.array(vox[k], MM.COLOR_DT if layer == "color" else (MM.TSDF_DT if layer == "tsdf" else F)).reshape(512)
    for key in np.asarray(read.get("esdf", ())).reshape(-1, 3):
        blk(key)["esdf"] = True
    return state


def _layer_arrays(state, layer):
    keys = MM.layer_keys(state, layer)
    return np.asarray(keys, np.int32).reshape(-1, 3), [state[k][layer] for k in keys]


class CheckerSide:
    """a drawn map in the CPU checker"""

    def __init__(self, oracle_mod, pg):
        import helpers as H
        self.O = oracle_mod; self.p = pg; self.occ = int(pg.projective_layer_type) == 1
        self.m = oracle_mod.OracleMap(H.copy_params(pg, oracle_mod.OrcParams))

    def draw(self, state):
        O = self.O
        for layer, ol in (("tsdf", O.L_TSDF), ("occ", O.L_TSDF), ("color", O.L_COLOR)):
            idx, vox = _layer_arrays(state, layer)
            for i, b in zip(idx.tolist(), vox):
                if layer == "occ":
                    t = np.zeros(512, O.TSDF_DT); t["distance"] = b; b = t
                self.m.set_block(ol, i, np.ascontiguousarray(b).view(O.TSDF_DT if layer != "color" else O.COLOR_DT))

    def read(self):
        O = self.O; out = {}
        ti = self.m.block_indices(O.L_TSDF)
        tb = [self.m.get_block(O.L_TSDF, i) for i in ti]
        if self.occ:
            out["occ"] = (ti, [b["distance"] for b in tb])
        else:
            out["tsdf"] = (ti, tb)
            ci = self.m.block_indices(O.L_COLOR)
            out["color"] = (ci, [self.m.get_block(O.L_COLOR, i) for i in ci])
        out["esdf"] = self.m.block_indices(O.L_ESDF)
        return out

    def run(self, step):
        op = step[0]
        if op == "update_esdf":
            self.m.update_esdf()
        elif op == "decay_tsdf":
            self.m.decay_tsdf(step[1])
        elif op == "decay_occupancy":
            self.m.decay_occupancy()
        elif op == "clear_outside_radius":
            self.m.clear_outside_radius(step[1], step[2])
        elif op == "clear_shapes":
            self.m.clear_tsdf_inside_shapes(step[1])
        else:
            raise ValueError(op)

    def read_esdf(self):
        idx = self.m.block_indices(self.O.L_ESDF)
        return idx, [self.m.get_block(self.O.L_ESDF, i) for i in idx]

    def take_cleared(self):
        return np.asarray(self.m.take_cleared_blocks(), np.int32).reshape(-1, 3)

    def close(self):
        pass


class ProductSide:
    """a drawn map in the product"""

    def __init__(self, M, pg, capacity=1024, max_capacity=None):
        self.M = M; self.p = pg; self.occ = int(pg.projective_layer_type) == 1
        self.m = M.Mapper(pg, block_capacity=capacity, max_block_capacity=max_capacity)
        self.proj = M.LAYER_OCCUPANCY if self.occ else M.LAYER_TSDF

    def draw(self, state):
        M = self.M
        for layer, ml in (("tsdf", M.LAYER_TSDF), ("occ", M.LAYER_OCCUPANCY), ("color", M.LAYER_COLOR)):
            idx, vox = _layer_arrays(state, layer)
            if len(idx):
                data = np.stack(vox)
                if layer == "occ":
                    t = np.zeros(data.shape, M.OCCUPANCY_DT); t["log_odds"] = data; data = t
                self.m.set_blocks(ml, idx, data)

    def _layer(self, ml):
        idx = np.asarray(self.m.block_indices(ml), np.int32).reshape(-1, 3)
        vox, found = self.m.get_blocks(ml, idx)
        assert found.all(), ("a block that block_indices lists was not found", idx[~found][:5].tolist())
        return idx, vox

    def read(self):
        M = self.M; out = {}
        if self.occ:
            i, v = self._layer(M.LAYER_OCCUPANCY)
            out["occ"] = (i, v["log_odds"])
        else:
            out["tsdf"] = self._layer(M.LAYER_TSDF)
            out["color"] = self._layer(M.LAYER_COLOR)
        out["esdf"] = np.asarray(self.m.block_indices(M.LAYER_ESDF), np.int32).reshape(-1, 3)
        return out

    def run(self, step):
        op = step[0]
        if op == "update_esdf":
            self.m.update_esdf()
        elif op == "decay_tsdf":
            self.m.decay_tsdf(step[1])
        elif op == "decay_occupancy":
            self.m.decay_occupancy()
        elif op == "clear_outside_radius":
            self.m.clear_outside_radius(step[1], step[2])
        elif op == "clear_shapes":
            self.m.clear_tsdf_inside_shapes(step[1])
        else:
            raise ValueError(op)

    def read_esdf(self):
        return self._layer(self.M.LAYER_ESDF)

    def take_cleared(self):
        return np.asarray(self.m.take_cleared_blocks(), np.int32).reshape(-1, 3)

    def close(self):
        self.m.close()


def checked_step(tag, side, step, spared=(), after_hook=None):
    """One call on a side, judged by the model applied to the map as read back before it: block sets, every voxel, the cleared list (and a second
    take of it, which is empty).  Returns the model's state after the call; after_hook(state, cleared, read-back after) runs further checks."""
    if step[0] == "update_esdf":
        side.run(step)
        return state_from_read(side.read())
    before = state_from_read(side.read())
    side.take_cleared()
    side.run(step)
    want, cleared = apply_model(before, step, side.p, spared)
    read = side.read()
    MM.assert_state_equals(tag, want, read)
    got = side.take_cleared()
    assert np.array_equal(got, cleared), (tag, "cleared list", len(got), len(cleared), got[:3].tolist(), cleared[:3].tolist())
    assert len(side.take_cleared()) == 0, (tag, "a second take of the cleared list is not empty")
    if after_hook:
        after_hook(want, before, cleared, read)
    return want


def run_case(case, side, after_hook=None):
    """draw the case, run its steps through checked_step; returns the model's final state"""
    side.draw(case.state)
    state = None
    for k, step in enumerate(case.steps):
        state = checked_step((case.name, k, step[0]), side, step, after_hook=after_hook)
    return state


# ------------------------------------------------------------------------------------------------ the ESDF after deallocation
# A drawn field whose sites lie in the UPPER block row of the z band only (2-D; the lower row is observed free space, so every column stays observed
# whatever happens to the upper row), a first update, ONE maintenance call, a second update.  The truth the ESDF layer is then held to:
#   (i)  the site / observed / inside marks of every ESDF block that exists equal the marking rule applied to the map's own TSDF read-back
#        (2-D: the column rule over the band; 3-D: each voxel by its own TSDF voxel),
#   (ii) squared distances and parents are those of exactly that site set over exactly the existing blocks.
ESDF_OPS_2D = ("decay_dealloc", "decay_set_free", "radius_drops_esdf", "radius_drops_upper_tsdf", "radius_drops_esdf_keeps_upper_tsdf", "shapes_reset_sites")
ESDF_OPS_3D = ("decay_dealloc", "decay_set_free", "radius_drops_esdf", "shapes_reset_sites")
EsdfScene = collections.namedtuple("EsdfScene", "tag params q dims nb state step S N verify")


def esdf_scene(M, op, r, dims, clear_radius_m=0.60):
    import esdf_cases as EC
    import esdf_independent as EI
    kw = dict(tsdf_decay_factor=0.5, tsdf_decayed_weight_threshold=1.0)
    if op == "decay_set_free":
        kw.update(tsdf_set_free_distance_on_decayed=1, tsdf_decayed_free_distance_vox=3.0)
    if dims == 3:
        kw.update(esdf_mode=1)
    pg, q = EC.params(M, r, VOXEL, **kw)
    bs = 8 * VOXEL
    nb = EI.field_blocks_2d(q) if dims == 2 else EI.field_blocks_3d(q)
    cb = nb // 2
    S, N = (cb, cb), (cb + 1, cb)
    if op == "radius_drops_esdf":
        S, N = (nb - 2, cb), (nb - 3, cb)
    site_vox = {S: [(4, 4), (2, 6)], N: [(3, 1)]}                                   # (vx, vy) within the block
    if dims == 2:
        assert EI.slice_geometry(pg)[:3] == (0, 1, 0), "the band is block rows 0..1, the slice in row 0"
        pattern = np.zeros((8 * nb, 8 * nb), bool)
        for (bx, by), vox in site_vox.items():
            for vx, vy in vox:
                pattern[8 * by + vy, 8 * bx + vx] = True
        idx, data = EI.tsdf_blocks_2d(pattern, np.ones((nb, nb), bool), pg)
        data = data.copy()
        data["distance"][idx[:, 2] == 0] = EI._voxel_values(pg)[1]                     # the lower row: free space
        S3, N3 = S + (1,), N + (1,)
        z_of_site = None
    else:
        S, N = S + (cb,), N + (cb,)
        sites = np.zeros((8 * nb,) * 3, bool)
        for b, vox in ((S, [(4, 4, 4), (2, 6, 1)]), (N, [(3, 1, 5)])):
            for v in vox:
                sites[tuple(8 * b[a] + v[a] for a in range(3))] = True
        assert nb <= 7
        idx, data = EI.tsdf_blocks_3d(sites, np.ones((nb,) * 3, bool), pg)
        data = data.copy()
        S3, N3 = S, N
        z_of_site = 4
    data["weight"] = 100.0
    doomed = (idx == np.asarray(S3)).all(1)
    assert doomed.sum() == 1
    first_site = tuple(8 * S[a] + (4, 4, 4)[a] for a in range(dims))                 # voxel coordinates (x, y[, z]) of the site the call removes
    other_site = tuple(8 * S[a] + (2, 6, 1)[a] for a in range(dims))
    if op == "decay_dealloc":
        data["weight"][doomed] = 1.5
        step = ("decay_tsdf", False)
    elif op == "decay_set_free":
        data["weight"][doomed] = np.where(data["distance"][doomed] < 0, 1.5, 100.0)
        step = ("decay_tsdf", False)
    elif op == "radius_drops_esdf":
        c = (0.5 * bs, (cb + 0.5) * bs, 0.5 * bs if dims == 2 else (cb + 0.5) * bs)
        step = ("clear_outside_radius", c, (nb - 2.5) * bs)
    elif op == "radius_drops_upper_tsdf":
        step = ("clear_outside_radius", ((cb + 0.5) * bs, (cb + 0.5) * bs, -0.35), clear_radius_m)
    elif op == "radius_drops_esdf_keeps_upper_tsdf":
        step = ("clear_outside_radius", ((N[0] + 0.5) * bs, (cb + 0.5) * bs, 0.45), 0.447)
    elif op == "shapes_reset_sites":
        p = [(v + 0.5) * VOXEL for v in first_site]
        lo = (p[0] - 0.01, p[1] - 0.01, 0.4 if dims == 2 else p[2] - 0.01); hi = (p[0] + 0.01, p[1] + 0.01, 0.8 if dims == 2 else p[2] + 0.01)
        step = ("clear_shapes", [("aabb", lo, hi)])
    else:
        raise ValueError(op)
    state = {tuple(int(v) for v in i): MM.make_block(tsdf=b) for i, b in zip(idx, data)}

    def at(field, v):
        return bool(field[v[::-1]] if dims == 2 else field[v])                        # 2-D fields are [y, x]

    def verify(before, after):
        """before / after the call and its update: (TSDF keys, ESDF keys, dense is_site field).  The call did what the scene was drawn for."""
        (tb, eb, sb), (ta, ea, sa) = before, after
        E_S, E_N = (S + (0,), N + (0,)) if dims == 2 else (S, N)
        n_s = len(site_vox[S if dims == 2 else S[:2]]); n_all = n_s + 1
        assert S3 in tb and E_S in eb and E_N in eb and int(sb.sum()) == n_all and at(sb, first_site) and at(sb, other_site), "the first update marks the drawn sites"
        if op == "decay_dealloc":
            assert S3 not in ta and E_S in ea and int(sa.sum()) == 1 and not at(sa, first_site)
        elif op == "decay_set_free":
            assert S3 in ta and E_S in ea and int(sa.sum()) == 1
        elif op == "radius_drops_esdf":
            assert E_S not in ea and E_N in ea and int(sa.sum()) == 1
        elif op == "radius_drops_upper_tsdf":
            assert S3 not in ta and S + (0,) in ta and E_S in ea and not at(sa, first_site) and not at(sa, other_site), "no TSDF voxel backs a site of this column any more"
        elif op == "radius_drops_esdf_keeps_upper_tsdf":
            assert S3 in ta and E_S not in ea and E_N in ea and int(sa.sum()) == 1, "the column has no ESDF block until its TSDF is dirtied again"
        elif op == "shapes_reset_sites":
            assert ta == tb and ea == eb and not at(sa, first_site) and at(sa, other_site) and int(sa.sum()) == n_all - 1
    return EsdfScene((op, "r%s" % r, "%dD" % dims), pg, q, dims, nb, state, step, S, N, verify)


def assert_esdf_truth(tag, scene, tsdf, esdf):
    """tsdf / esdf: (indices, voxels) read back from one map.  Returns (TSDF keys, ESDF keys, dense is_site)."""
    import esdf_cases as EC
    import esdf_independent as EI
    nb, dims, pg, q = scene.nb, scene.dims, scene.params, scene.q
    origin, shape = (0,) * dims, (nb,) * dims
    if dims == 2:
        marks = EI.column_marks_2d(tsdf[0], tsdf[1], pg, origin, shape)
        f, _ = EI.slice_fields(esdf[0], esdf[1], pg, origin, shape)
    else:
        marks = EI.volume_marks_3d(tsdf[0], tsdf[1], pg, origin, shape)
        f, _ = EI.volume_fields(esdf[0], esdf[1], origin, shape)
    where = f.dom
    site, obs, ins = (m & where for m in marks)
    for name, got, want in (("is_site", f.site, site), ("observed", f.observed, obs), ("is_inside", f.inside, ins)):
        assert np.array_equal(got, want), (tag, "marks equal the column rule", name, "%d marked, %d by the rule" % (int(got.sum()), int(want.sum())),
                                           np.argwhere(got != want)[:5].tolist(), "squared distance there", f.sq[got != want][:5].tolist())
    if np.array_equal(obs, where) and np.array_equal(ins, site):
        EC.assert_field(tag, f, site, where, q, dims)
    else:                                                                              # (a deallocated 3-D block: allocated, nothing observed)
        sq, cnt = EI.edt_bruteforce(site, where, q)
        bad = where & (f.sq != sq)
        assert not bad.any(), (tag, "squared distance differs from the brute force at", np.argwhere(bad)[:5].tolist(), f.sq[bad][:5].tolist(), sq[bad][:5].tolist())
        EI.check_parents(site, f.sq, f.parent, where, q)
        assert np.array_equal((f.parent != 0).any(-1)[where], ((cnt > 0) & ~site)[where]), (tag, "a parent exactly where a site counts")
    keys = lambda a: {tuple(int(v) for v in i) for i in np.asarray(a).reshape(-1, 3)}                # noqa: E731
    return keys(tsdf[0]), keys(esdf[0]), f.site


def run_esdf_scene(scene, side):
    """draw, update, truth; the call (judged by the model like any other), update, truth; the scene's own conditions.  Returns the ESDF read-back."""
    side.draw(scene.state)
    side.run(("update_esdf",))
    before = assert_esdf_truth(scene.tag + ("first update",), scene, side.read()["tsdf"], side.read_esdf())
    checked_step(scene.tag + (scene.step[0],), side, scene.step)
    side.run(("update_esdf",))
    esdf = side.read_esdf()
    after = assert_esdf_truth(scene.tag + ("after the call",), scene, side.read()["tsdf"], esdf)
    scene.verify(before, after)
    return esdf


# ------------------------------------------------------------------------------------------------ the product only: look-ups, pool and hash conservation
# The tolerance of a point query at a voxel centre (metres), per query: on each axis u = p / vs - 0.5 lands within three float32 spacings of the voxel's
# integer index (the centre is itself three rounded float32 operations, the quotient one more, the float32 voxel size a quarter spacing), so the
# neighbour's share of the interpolant is at most 3 spacings of u per axis and the three axes together move the result by at most
# 3 * 3 * spacing(|u|) * (the largest difference between two drawn distances, 0.4 m): 1.4e-5 m for |u| < 64; 1e-6 m for the interpolant's own rounding.
def query_tolerance(points, voxel_size):
    u = np.abs(np.asarray(points, F) / F(voxel_size)).max(1)
    return 9.0 * np.spacing(u.astype(F)).astype(np.float64) * 0.4 + 1e-6


SHELL = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def lookups(tag, side, state, gone=(), query=True, max_shell=1500):
    """Every way into the map agrees with the model's state: the block count, get_blocks per layer (found with the model's bytes is what
    MM.assert_state_equals checked on side.read(); here: NOT found, with zeros, for the blocks `gone`, for every block that lacks the layer and for a
    shell of never-allocated neighbours), point queries at voxel centres of a sample of live blocks, no overflow."""
    M, g = side.M, side.m
    c = g.counters()
    assert c["blocks_allocated"] == len(state), (tag, "blocks_allocated", c["blocks_allocated"], len(state))
    assert c["capacity_overflow"] == 0, (tag, c)
    shell = sorted({tuple(k[a] + d[a] for a in range(3)) for k in state for d in SHELL} - set(state))
    shell = shell[::max(1, len(shell) // max_shell)]
    probe = sorted(set(tuple(int(v) for v in k) for k in gone) | set(state)) + shell
    layers = (("occ", M.LAYER_OCCUPANCY),) if side.occ else (("tsdf", M.LAYER_TSDF), ("color", M.LAYER_COLOR))
    for name, ml in layers:
        absent = [k for k in probe if k not in state or state[k][name] is None]
        if absent:
            vox, found = g.get_blocks(ml, np.asarray(absent, np.int32))
            assert not found.any(), (tag, name, "found a block that is not there", [absent[i] for i in np.nonzero(found)[0][:5]])
            assert not vox.view(np.uint8).any(), (tag, name, "a block reported not found came back with data")
    if query and not side.occ:
        keys = [k for k in MM.layer_keys(state, "tsdf") if not (state[k]["tsdf"]["weight"] < 0).any() and not np.isnan(state[k]["tsdf"]["weight"]).any()]
        keys = keys[::max(1, len(keys) // 24)]
        rng = np.random.default_rng(len(state))
        if keys:
            v = rng.integers(1, 7, (len(keys), 4, 3))                                   # interior voxels: all eight corners in the block itself
            pts = np.concatenate([MM.voxel_centres(k, side.p.voxel_size)[v[i, :, 0] * 64 + v[i, :, 1] * 8 + v[i, :, 2]] for i, k in enumerate(keys)])
            want = np.concatenate([state[k]["tsdf"]["distance"][v[i, :, 0] * 64 + v[i, :, 1] * 8 + v[i, :, 2]] for i, k in enumerate(keys)])
            d, _, ok = g.query_tsdf(pts, min_weight=0.0)
            d = d.cpu().numpy(); ok = ok.cpu().numpy().astype(bool)
            assert ok.all(), (tag, "a point query inside a live block is invalid", pts[~ok][:3].tolist())
            err = np.abs(d.astype(np.float64) - want.astype(np.float64)); tol = query_tolerance(pts, side.p.voxel_size)
            assert (err <= tol).all(), (tag, "point query against the stored voxel", float(err.max()), float(tol[np.argmax(err)]))
        dead = [k for k in gone if tuple(k) not in state or state[tuple(k)]["tsdf"] is None][:16]
        if len(dead):
            pts = np.stack([MM.voxel_centres(tuple(k), side.p.voxel_size)[3 * 64 + 3 * 8 + 3] for k in dead])
            _, _, ok = g.query_tsdf(pts, min_weight=0.0)
            assert not ok.cpu().numpy().any(), (tag, "a point query inside a deallocated block is valid")


def lookup_hook(side):
    """the after_hook of checked_step that runs `lookups` after every call"""
    def hook(state, before, cleared, read):
        gone = [k for k in before if k not in state or any(before[k][f] is not None and state[k][f] is None for f in ("tsdf", "occ", "color"))]
        lookups(("look-ups", len(state)), side, state, gone)
    return hook


def drawn_blocks(rng, keys, kind, weight):
    """{key: block}: kind "tc" TSDF with colour, "t" TSDF only, "c" colour only; every block its own random voxels, all TSDF weights `weight`"""
    out = {}
    for k in keys:
        t = _tsdf(rng.uniform(-0.2, 0.2, 512).astype(F), np.full(512, weight, F)) if "t" in kind else None
        out[tuple(k)] = MM.make_block(tsdf=t, color=_color(rng) if "c" in kind else None)
    return out


def draw_more(tag, side, state, blocks, gone=()):
    """set_blocks of `blocks` on top of the map; the read-back equals the model's state with those blocks laid over it (a block drawn without a
    layer has none, whatever the slot held before).  Returns the new state."""
    side.draw(blocks)
    new = {k: {f: (v.copy() if isinstance(v, np.ndarray) else v) for f, v in b.items()} for k, b in state.items()}
    for k, b in blocks.items():
        if k in new:
            for f in ("tsdf", "color"):
                if b[f] is not None:
                    new[k][f] = b[f].copy()
        else:
            new[k] = MM.make_block(tsdf=b["tsdf"], color=b["color"])
    MM.assert_state_equals(tag, new, side.read())
    lookups(tag, side, new, gone)
    return new


CONSERVATION_PARAMS = dict(tsdf_decay_factor=0.5, tsdf_decayed_weight_threshold=0.25)
LIVE_W, DOOMED_W = 100.0, 0.4                 # 100 survives five halvings (3.125 >= 0.25), 0.4 dies in the first


def _fresh_keys(n, used, z):
    out = []
    x = 0
    while len(out) < n:
        k = (x % 16 - 8, x // 16 - 8, z)
        if k not in used:
            out.append(k)
        x += 1
    return out


def conservation_rounds(M, rounds=5):
    """A pool of exactly 256 slots, filled to the last one (96 TSDF with colour, 96 TSDF only, 64 colour only: the table at load 1/2), put through
    `rounds` rounds of decay -- which drops the doomed part, about half of the TSDF blocks in the first round and most of the refill in
    the later ones -- and a refill to exactly 256 again at new indices and at some of the dropped ones, with the layers swapped (a dropped
    TSDF-with-colour index comes back as TSDF only, colour-only blocks take recycled slots).  After every call the read-back equals the model, every
    look-up agrees, nothing overflows: a slot freed twice shows as two blocks sharing voxels or as a count that is off, a slot never freed as an
    overflow in the refill, a key the rebuilt table lost as a block not found.  Returns the side (for what the caller adds)."""
    pg = M.default_params(voxel_size=VOXEL, **CONSERVATION_PARAMS)
    side = ProductSide(M, pg, capacity=256, max_capacity=256)
    assert side.m.capacity == 256
    rng = np.random.default_rng(23)
    used = set()
    blocks = {}
    for n, kind, z in ((96, "tc", 0), (96, "t", 1), (64, "c", 2)):
        keys = _fresh_keys(n, used, z); used |= set(keys)
        for j, k in enumerate(keys):
            blocks.update(drawn_blocks(rng, [k], kind, DOOMED_W if j % 2 else LIVE_W))
    state = draw_more(("conservation", "fill"), side, {}, blocks)
    assert len(state) == 256
    hook = lookup_hook(side)
    for r in range(rounds):
        before = state
        state = checked_step(("conservation", r, "decay"), side, ("decay_tsdf", False), after_hook=hook)
        dropped = [k for k in before if k not in state]
        had_colour = [k for k in dropped if before[k]["color"] is not None]
        assert len(dropped) >= 30 and len(had_colour) >= 10, (r, len(dropped), len(had_colour))      # (96 in the first round, 7/8 of each refill after it)
        n = 256 - len(state)
        again = had_colour[:n // 4]                                                    # dropped indices that held colour: back as TSDF only
        fresh = _fresh_keys(n - len(again), used, 3 + r); used |= set(fresh)
        blocks = {}
        for j, k in enumerate(again + fresh[:len(fresh) - len(fresh) // 8]):
            blocks.update(drawn_blocks(rng, [k], "t" if k in again or j % 2 else "tc", LIVE_W if j % 8 == 0 else DOOMED_W))
        blocks.update(drawn_blocks(rng, fresh[len(fresh) - len(fresh) // 8:], "c", 0.0))      # colour only, in recycled slots
        state = draw_more(("conservation", r, "refill"), side, state, blocks, gone=dropped)
        assert len(state) == 256 and all(state[k]["color"] is None for k in again)
    return side, state, rng, used
