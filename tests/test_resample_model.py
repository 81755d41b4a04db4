"""The numpy model of resampling (tests/resample_independent.py) against brute force, against the merge's model and against float64: the
candidate rule is complete over drawn transforms, ratios and tap counts (no destination block outside the candidate set holds a voxel that
would fuse), no source block yields more than 27 candidates, no destination block reaches more than N source blocks per axis; with one voxel
size and one tap the model is merge_independent.merge bit for bit; a plane is reproduced; a voxel fuses iff at least half its taps are valid.
No GPU, no library."""
import itertools

import numpy as np
import pytest

import merge_independent as MI
import resample_independent as RI

F32 = np.float32
pose = MI.pose
VS_S = 0.05
RATIOS = {1.0: 0.05, 1.5: 0.075, 2.0: 0.1, 3.0: 0.15, 4.0: 0.2}
DIAG = float(np.degrees(np.arccos(1.0 / np.sqrt(3.0))))      # 54.7356 deg: the cube diagonal onto an axis


def diagonal_rotations():
    """the block's diagonal (and the other three) turned onto x, y and z: the widest a block gets along an axis -- and a degree to either side"""
    out = []
    for d in ((1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1)):
        for e in np.eye(3):
            axis = np.cross(np.array(d, float), e)
            for da in (0.0, -1.0, 1.0):
                out.append(pose(axis, DIAG + da, [0.013, -0.021, 0.034]))
    return out


def drawn(n=6, seed=5):
    rng = np.random.default_rng(seed)
    out = [pose([0, 0, 1], 0.0, [0, 0, 0]), pose([0, 0, 1], 45.0, [-3.13, 0.77, -1.91]), pose([0, 0, 1], 45.0, [0.0, 0.0, 0.0]),
           pose([1, 2, 3], 54.7, [0.37, -0.21, 0.13])]
    for _ in range(n):
        out.append(pose(rng.normal(size=3), rng.uniform(0.0, 180.0), rng.uniform(-4.0, 4.0, 3)))
    return out


def cluster(rng, origin, n=2, weights=(1.0,), dist=0.15, color=False):
    t, c = {}, {}
    for x, y, z in itertools.product(range(n), repeat=3):
        b = np.zeros(512, MI.TSDF_DT)
        b["distance"] = rng.uniform(-dist, dist, 512).astype(F32); b["weight"] = rng.choice(np.asarray(weights, F32), 512)
        k = (origin[0] + x, origin[1] + y, origin[2] + z)
        t[k] = b
        if color:
            q = np.zeros(512, MI.COLOR_DT)
            for ch in "rgb":
                q[ch] = rng.integers(0, 256, 512)
            q["weight"] = rng.choice(np.array([0.0, 1.0, 2.5], F32), 512)
            c[k] = q
    return t, c


# ---- 1. the derived bounds by brute force
@pytest.mark.parametrize("r", sorted(RATIOS))
def test_no_source_block_has_more_than_27_candidates_and_no_block_reaches_more_than_N(r):
    rng = np.random.default_rng(int(r * 10))
    vd = RATIOS[r]
    widest = {}
    for n in (1, 2, 3, 4):
        N = RI.reach_bound(RI.ratio(vd, VS_S), n)
        assert N ** 3 <= 512
        worst = 0
        for T in drawn() + diagonal_rotations():
            keys = rng.integers(-40, 40, (32, 3))
            lo, hi = RI.candidate_boxes(T, keys, VS_S, vd, n)
            assert ((hi - lo + 1) <= 3).all() and ((hi - lo + 1) >= 1).all(), (r, n)
            blocks = rng.integers(-12, 12, (6, 3))
            got = RI.reach(T, blocks, VS_S, vd, n)
            assert (got <= N).all(), (r, n, int(got.max()), N, T)
            worst = max(worst, int(got.max()))
        widest[n] = (worst, N)
    print("r = %g: largest reach found / N per tap count: %r" % (r, widest))
    assert all(w >= N - 1 for w, N in widest.values()), widest      # (the bound is not loose by more than a block)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("r", sorted(RATIOS))
def test_no_block_outside_the_candidate_set_holds_a_voxel_that_would_fuse(r, n):
    rng = np.random.default_rng(100 + int(r * 10) + n)
    vd = RATIOS[r]
    Ts = [pose([0, 0, 1], 0.0, [0.011, -0.02, 0.003]), pose([0, 0, 1], 45.0, [-1.13, 0.77, -0.91]), diagonal_rotations()[0],
          pose(rng.normal(size=3), rng.uniform(0.0, 180.0), rng.uniform(-2.0, 2.0, 3))]
    for T in Ts[:4 if n < 3 else 3] if n < 4 else Ts[1:3]:      # (the time goes with n^3)
        origin = tuple(int(q) for q in rng.integers(-6, 6, 3))
        src, _ = cluster(rng, origin, n=1 if r < 2 else 2)
        cand = RI.candidates(T, sorted(src), VS_S, vd, n)
        c = np.array(sorted(cand))
        lo, hi = c.min(0) - 1, c.max(0) + 1
        outside = [k for k in itertools.product(*(range(lo[a], hi[a] + 1) for a in range(3))) if k not in cand]
        ro = RI.resample({}, {}, src, {}, T, VS_S, vd, 4 * vd, 5.0, taps=n, blocks=outside)
        bad = [k for k in outside if ro["fused"][k].any()]
        assert not bad, (T, bad[:4])
        # stronger: outside the candidate set no voxel has a single valid tap
        assert not any(ro["valid_taps"][k].any() for k in outside)
        ri = RI.resample({}, {}, src, {}, T, VS_S, vd, 4 * vd, 5.0, taps=n)
        assert ri["candidates"] == sorted(cand) and ri["voxels_fused"] > 0          # (not vacuous: the block's interior does fuse)


# ---- 2. one voxel size, one tap: the merge
def test_with_one_voxel_size_and_one_tap_the_model_is_the_merges_bit_for_bit():
    rng = np.random.default_rng(12)
    src, scol = cluster(rng, (-1, 2, 0), weights=(0.3, 1.0, 2.5, 5e-5), color=True)
    del scol[(-1, 2, 0)]                                                  # a TSDF block without its colour block
    dst, dcol = cluster(rng, (-1, 1, 0), n=3, weights=(0.0, 0.7, 4.9), color=True)
    most = 0
    for T in MI.drawn_transforms(4, seed=2) + [pose([1, 2, 3], 1.5, [0.02, -0.01, 0.017])]:
        for opts in ({}, {"weight_scale": 0.25}, {"merge_color": 0}, {"min_weight": 0.75}):
            a = MI.merge(dst, dcol, src, scol, T, VS_S, 0.2, 5.0, **opts)
            b = RI.resample(dst, dcol, src, scol, T, VS_S, VS_S, 0.2, 5.0, taps=1, **opts)
            assert RI.taps_for(1.0) == 1 and b["taps"] == 1
            for f in ("candidates", "source_blocks", "candidate_blocks", "blocks_allocated", "voxels_fused", "color_voxels_fused", "status", "band"):
                assert a[f] == b[f], f
            assert set(a["tsdf"]) == set(b["tsdf"]) and set(a["color"]) == set(b["color"])
            for k in a["tsdf"]:
                assert a["tsdf"][k].tobytes() == b["tsdf"][k].tobytes(), k
            for k in a["color"]:
                assert a["color"][k].tobytes() == b["color"][k].tobytes(), k
            most = max(most, a["voxels_fused"] if a["color_voxels_fused"] else 0)
    assert most > 200          # (not vacuous: a case fused voxels and blended colours)


def test_a_sum_that_starts_at_minus_zero_is_the_identity_for_one_tap():
    for x in (F32(0.0), F32(-0.0), F32(1.5), F32(-3e-39), F32(np.inf)):
        s = F32(-0.0) + x
        assert s.view(np.uint32) == x.view(np.uint32) and (s / F32(1.0)).view(np.uint32) == x.view(np.uint32)


# ---- 3. a plane
PLANE_F32_F64_M = 3e-7                 # largest |f32 model - f64 mode| on the plane, metres: 2.98e-7 at r 1.5, n 2 (see the test below)
PLANE_TOL = 4 * PLANE_F32_F64_M


@pytest.mark.parametrize("r,n", [(2.0, 2), (4.0, 4), (1.5, 2), (3.0, 3)])
def test_a_plane_is_reproduced(r, n):
    """d = nrm . p - c0 in src, clamped at +-trunc_s, weight 1 everywhere, the normal oblique.  On destination voxels all of whose taps are valid
    and touch no clamped corner the float32 model must give the plane's value at the voxel's centre (the tap lattice is symmetric about it).
    Tolerance: four times the largest difference between the float32 model and its float64 mode (positions, interpolation, reduction and fuse in
    float64 over the same float32 inputs and corners) over these four cases, measured on the CPU: PLANE_F32_F64_M below.  Each case prints
    what it finds and asserts that the recorded figure still covers it."""
    vd = RATIOS[r]
    nrm = np.array([0.36, -0.48, 0.8]); c0 = 3.12
    trunc_s = 4 * VS_S
    centre_blk = np.array([3, -4, 6])                                        # the plane passes through (1.2, -1.6, 2.4)
    keys = [tuple(int(q) for q in centre_blk - 3 + np.array(k)) for k in itertools.product(range(6), repeat=3)]
    src, clamped = {}, {}
    for k in keys:
        p = (8 * np.array(k) + MI.LANE_XYZ + 0.5) * float(F32(VS_S))
        d = p @ nrm - c0
        b = np.zeros(512, MI.TSDF_DT); b["distance"] = np.clip(d, -trunc_s, trunc_s).astype(F32); b["weight"] = 1.0
        q = np.zeros(512, MI.TSDF_DT); q["distance"] = (np.abs(d) >= trunc_s).astype(F32); q["weight"] = 1.0
        src[k] = b; clamped[k] = q
    T = pose([1, 2, 3], 30.0, [0.37, -0.21, 0.13])
    trunc_d = 4 * vd
    a = RI.resample({}, {}, src, {}, T, VS_S, vd, trunc_d, 5.0, taps=n)
    b = RI.resample({}, {}, src, {}, T, VS_S, vd, trunc_d, 5.0, taps=n, dtype=np.float64)
    assert a["candidates"] == b["candidates"]
    cand = np.array(a["candidates"])
    # which voxels touch a clamped corner: the same taps over the indicator field (its interpolant is > 0 iff a clamped corner has a share)
    cnt, ind, _ = RI.reduce_taps(MI._Table(clamped, MI.TSDF_DT), T, cand, VS_S, vd, n, 1e-4)
    T64 = T.astype(np.float64)
    n2 = T64[:3, :3] @ nrm; c2 = c0 + n2 @ T64[:3, 3]
    worst, worst64, seen = 0.0, 0.0, 0
    for i, k in enumerate(a["candidates"]):
        clean = (cnt[i] == n ** 3) & (ind[i] == 0)
        if not clean.any():
            continue
        assert a["fused"][k][clean].all() and (a["valid_taps"][k][clean] == n ** 3).all()
        pD = (8 * np.array(k) + MI.LANE_XYZ + 0.5) * float(F32(vd))
        want = pD @ n2 - c2
        got = a["tsdf"][k]["distance"].astype(np.float64)
        assert (a["tsdf"][k]["weight"][clean] == F32(1.0)).all()               # all taps valid, weight 1 everywhere: the full weight
        worst = max(worst, float(np.abs(got - want)[clean].max()))
        worst64 = max(worst64, float(np.abs(got - b["tsdf"][k]["distance"].astype(np.float64))[clean].max()))
        seen += int(clean.sum())
    print("r %g n %d: %d clean voxels, |f32 - plane| <= %.3g m, |f32 - f64 mode| <= %.3g m" % (r, n, seen, worst, worst64))
    assert seen > (200 if r < 4 else 20)
    assert worst64 <= PLANE_F32_F64_M, worst64
    assert worst <= PLANE_TOL, worst


# ---- 4. at least half the taps
def _grid_source(n_blocks, weak):
    """blocks [0, n_blocks)^3 with weight 1 and distance 0.01 everywhere but the global voxels in `weak` (weight 5e-5)"""
    src = {}
    for k in itertools.product(range(n_blocks), repeat=3):
        b = np.zeros(512, MI.TSDF_DT); b["distance"] = F32(0.01); b["weight"] = F32(1.0)
        src[k] = b
    for v in weak:
        k = tuple(q >> 3 for q in v)
        src[k]["weight"][(v[2] & 7) + 8 * (v[1] & 7) + 64 * (v[0] & 7)] = F32(5e-5)
    return src


def _count_directly(n, stride_g, stride_i, weak, block=(0, 0, 0)):
    """valid taps per voxel of one destination block when tap i of voxel g has the base voxel stride_g g + stride_i i per axis: plain loops"""
    weak = set(weak)
    out = np.zeros(512, np.int64)
    for lane, (vx, vy, vz) in enumerate(MI.LANE_XYZ):
        g = (8 * block[0] + vx, 8 * block[1] + vy, 8 * block[2] + vz)
        for tap in itertools.product(range(n), repeat=3):
            b = [stride_g * g[a] + stride_i * tap[a] for a in range(3)]
            out[lane] += not any((b[0] + i, b[1] + j, b[2] + k) in weak for i, j, k in itertools.product((0, 1), repeat=3))
    return out


HALF_CASES = {
    # n: (r, weak voxel offsets from n g that leave exactly half (rounded up) of the taps valid, one more that takes a further tap)
    3: (3, [(1, 1, 1), (3, 3, 3), (3, 1, 1)], (0, 3, 3)),                # 27 - (8 + 1 + 4) = 14, then 13
    4: (4, [(1, 1, 1), (1, 1, 3), (1, 3, 1), (1, 3, 3)], (4, 4, 4)),      # 64 - 2 * 4 * 4 = 32, then 31
}


@pytest.mark.parametrize("n", [3, 4])
def test_a_voxel_fuses_iff_at_least_half_of_its_taps_are_valid(n):
    """vs_d = n vs_s and a shift of half a source voxel: tap i of voxel g has the base voxel n g + i and t = 0.5 on every axis, so a weak voxel at
    offset a from n g takes the taps i with a - 1 <= i <= a"""
    vs = 0.0625
    r, weak_off, one_more = HALF_CASES[n]
    g = np.array([2, 3, 4])
    T = pose([0, 0, 1], 0.0, [-0.5 * vs] * 3)
    lane = int(g[2] + 8 * g[1] + 64 * g[0])
    got = []
    for offs in (weak_off, weak_off + [one_more]):
        weak = [tuple(int(q) for q in n * g + np.array(o)) for o in offs]
        src = _grid_source(r + 1, weak)
        res = RI.resample({}, {}, src, {}, T, vs, r * vs, 4 * r * vs, 5.0, taps=n, blocks=[(0, 0, 0)])
        want = _count_directly(n, n, 1, weak)
        assert np.array_equal(res["valid_taps"][(0, 0, 0)], want)
        assert np.array_equal(res["fused"][(0, 0, 0)], 2 * want >= n ** 3)
        got.append((int(want[lane]), bool(res["fused"][(0, 0, 0)][lane]), float(res["tsdf"][(0, 0, 0)]["weight"][lane])))
    half = (n ** 3 + 1) // 2
    assert got[0] == (half, True, float(F32(half) / F32(n ** 3))) and got[1] == (half - 1, False, 0.0), got


def test_two_taps_per_axis_on_a_checkerboard_of_taps():
    """r = 4, n = 2, the identity: tap i of voxel g has the base voxel 4 g + 2 i and t = 0.5, the taps' corner cells are disjoint.  Weak base voxels
    on the taps with an odd index sum: 4 of 8 valid everywhere -- every voxel fuses with half the weight; one more weak tap: 3 of 8, not fused"""
    vs = 0.0625
    weak = [(4 * gx + 2 * ix, 4 * gy + 2 * iy, 4 * gz + 2 * iz) for gx, gy, gz in itertools.product(range(8), repeat=3)
            for ix, iy, iz in itertools.product(range(2), repeat=3) if (ix + iy + iz) & 1]
    g = (5, 1, 6)
    lane = g[2] + 8 * g[1] + 64 * g[0]
    for extra, count, fuses in (([], 4, True), ([(4 * g[0] + 1, 4 * g[1] + 1, 4 * g[2] + 1)], 3, False)):      # (a corner of tap (0, 0, 0)'s cell)
        res = RI.resample({}, {}, _grid_source(5, weak + extra), {}, None, vs, 4 * vs, 1.0, 5.0, taps=2, blocks=[(0, 0, 0)])
        want = _count_directly(2, 4, 2, weak + extra)
        assert np.array_equal(res["valid_taps"][(0, 0, 0)], want) and want[lane] == count
        assert bool(res["fused"][(0, 0, 0)][lane]) == fuses
        others = np.arange(512) != lane
        assert (want[others] == 4).all() and res["fused"][(0, 0, 0)][others].all()
        blk = res["tsdf"][(0, 0, 0)]
        assert (blk["weight"][others] == F32(0.5)).all() and (blk["distance"][others] == F32(0.01)).all()
        assert blk["weight"][lane] == (F32(0.5) if fuses else F32(0.0))
