"""The numpy model of map merging (tests/merge_independent.py) against itself and against float64: the candidate rule is complete on drawn
transforms (no destination block outside the candidate set holds a valid sample -- this is what checks the padding margin), the 27-block
bounds hold in both directions, a whole-block translation into an empty map reproduces the source's interior voxels exactly, and the float32
evaluation stays within rounding of the float64 one.  No GPU, no library."""
import numpy as np
import pytest

import merge_independent as MI

F32 = np.float32
pose, drawn_transforms = MI.pose, MI.drawn_transforms
EPS32 = 2.0 ** -23


def cluster(rng, origin, n=2, weights=(1.0,), dist=0.15):
    """n x n x n source blocks at block offset `origin`, distances uniform in +-dist, weights drawn from `weights`"""
    out = {}
    for x in range(n):
        for y in range(n):
            for z in range(n):
                b = np.zeros(512, MI.TSDF_DT)
                b["distance"] = rng.uniform(-dist, dist, 512).astype(F32)
                b["weight"] = rng.choice(np.asarray(weights, F32), 512)
                out[(origin[0] + x, origin[1] + y, origin[2] + z)] = b
    return out


@pytest.mark.parametrize("vs", [0.05, 0.0625])
def test_no_block_outside_the_candidate_set_holds_a_valid_sample(vs):
    rng = np.random.default_rng(11)
    for T in drawn_transforms():
        origin = tuple(int(q) for q in rng.integers(-6, 6, 3))
        src = cluster(rng, origin)
        cand = MI.candidates(T, sorted(src), vs)
        c = np.array(sorted(cand))
        lo, hi = c.min(0) - 1, c.max(0) + 1
        every = [(x, y, z) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)]
        r = MI.merge({}, {}, src, {}, T, vs, 4 * vs, 5.0, blocks=every)
        inside = sum(int(r["fused"][k].any()) for k in every if k in cand)
        outside = [k for k in every if k not in cand and r["fused"][k].any()]
        assert not outside, (T, outside[:4])
        assert inside > 0 and r["voxels_fused"] > 512          # (the check is not vacuous: the interior of the cluster does fuse)
        # hence going over the candidates alone fuses as many voxels as going over every block around them
        assert MI.merge({}, {}, src, {}, T, vs, 4 * vs, 5.0)["voxels_fused"] == r["voxels_fused"]


def test_the_27_block_bounds_hold_in_both_directions():
    rng = np.random.default_rng(5)
    for vs in (0.05, 0.0625, 0.1):
        for T in drawn_transforms(24, seed=9):
            keys = rng.integers(-40, 40, (64, 3))
            lo, hi = MI.candidate_boxes(T, keys, vs)
            assert ((hi - lo + 1) <= 3).all() and ((hi - lo + 1) >= 1).all()
            blocks = rng.integers(-40, 40, (64, 3))
            assert (MI.reach(T, blocks, vs) <= 3).all()


def test_a_whole_block_translation_reproduces_the_interior_exactly():
    """voxel size 2^-4 and weights that are powers of two: every position, quotient and weighted mean is exact"""
    rng = np.random.default_rng(2)
    vs = 0.0625
    src = cluster(rng, (-1, 2, 0), weights=(0.5, 1.0, 2.0, 4.0))
    shift = np.array([2, -1, 3])
    T = pose([0, 0, 1], 0.0, shift * 8 * vs)
    r = MI.merge({}, {}, src, {}, T, vs, 4 * vs, 5.0)
    assert r["status"] == MI.OK and r["blocks_allocated"] == r["candidate_blocks"] == len(r["candidates"])
    seen = 0
    for k, blk in src.items():
        kd = tuple(int(q) for q in np.array(k) + shift)
        assert kd in r["tsdf"]
        got = r["tsdf"][kd]
        # interior: the +1 corners exist, i.e. every voxel but those on a + face of the cluster
        g = 8 * np.array(k) + MI.LANE_XYZ
        interior = np.array([all(tuple((g[l] + o) >> 3) in src for o in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))) for l in range(512)])
        assert np.array_equal(r["fused"][kd], interior)
        assert np.array_equal(got["distance"][interior].view(np.uint32), blk["distance"][interior].view(np.uint32))
        assert np.array_equal(got["weight"][interior].view(np.uint32), blk["weight"][interior].view(np.uint32))
        assert (got["weight"][~interior] == 0).all() and (got["distance"][~interior] == 0).all()
        seen += int(interior.sum())
    assert seen == r["voxels_fused"] == 15 ** 3


def test_float32_stays_within_rounding_of_float64():
    rng = np.random.default_rng(8)
    vs, trunc, mw = 0.05, 0.2, 5.0
    src = cluster(rng, (0, 0, 0), weights=(0.3, 1.0, 2.5))
    dst = cluster(rng, (0, 0, 0), n=3, weights=(0.0, 0.7, 4.9))
    T = pose([1, 2, 3], 30.0, [0.11, -0.07, 0.19])
    a = MI.merge(dst, {}, src, {}, T, vs, trunc, mw)
    b = MI.merge(dst, {}, src, {}, T, vs, trunc, mw, dtype=np.float64)
    assert a["candidates"] == b["candidates"] and a["voxels_fused"] == b["voxels_fused"] > 1000
    # trilinear: 7 lerps of 3 roundings each on values <= trunc (weights: <= 2.5); the fuse: two products, a sum, a quotient
    for k in a["candidates"]:
        assert np.array_equal(a["fused"][k], b["fused"][k])
        assert np.abs(a["tsdf"][k]["distance"].astype(np.float64) - b["tsdf"][k]["distance"]).max() <= 32 * EPS32 * trunc
        assert np.abs(a["tsdf"][k]["weight"].astype(np.float64) - b["tsdf"][k]["weight"]).max() <= 32 * EPS32 * mw
        assert (a["tsdf"][k]["weight"] <= F32(mw)).all() and (np.abs(a["tsdf"][k]["distance"]) <= F32(trunc)).all()
        untouched = ~a["fused"][k]
        before = dst.get(k, np.zeros(512, MI.TSDF_DT))
        assert np.array_equal(a["tsdf"][k][untouched], before[untouched])


def test_options_colour_and_statuses():
    rng = np.random.default_rng(4)
    vs = 0.05
    src = cluster(rng, (0, 0, 0))
    col = {}
    for k in list(src)[:5]:
        c = np.zeros(512, MI.COLOR_DT)
        c["r"] = rng.integers(0, 256, 512); c["g"] = rng.integers(0, 256, 512); c["b"] = rng.integers(0, 256, 512); c["weight"] = rng.choice(np.array([0.0, 1.0, 3.0], F32), 512)
        col[k] = c
    T = pose([0, 1, 0], 10.0, [0.02, 0.01, -0.03])
    r = MI.merge({}, {}, src, col, T, vs, 0.2, 5.0)
    assert 0 < r["color_voxels_fused"] < r["voxels_fused"]
    assert set(r["color"]) == {k for k in r["candidates"] if r["colored"][k].any()}
    for k, c in r["color"].items():
        assert (c["weight"][~r["colored"][k]] == 0).all() and (c["weight"][r["colored"][k]] > 0).all()
    r0 = MI.merge({}, {}, src, col, T, vs, 0.2, 5.0, merge_color=0)
    assert r0["color"] == {} and r0["color_voxels_fused"] == 0 and r0["voxels_fused"] == r["voxels_fused"]
    rq = MI.merge({}, {}, src, col, T, vs, 0.2, 5.0, weight_scale=0.25)
    k = next(k for k in r["candidates"] if r["fused"][k].any())
    assert np.allclose(rq["tsdf"][k]["weight"], 0.25 * r["tsdf"][k]["weight"], rtol=1e-6)
    assert MI.merge({}, {}, {}, {}, T, vs, 0.2, 5.0)["status"] == MI.EMPTY_SOURCE
    weak = {k: v.copy() for k, v in src.items()}
    for v in weak.values():
        v["weight"] = F32(5e-5)
    rn = MI.merge({}, {}, weak, {}, T, vs, 0.2, 5.0)
    assert rn["status"] == MI.NO_OVERLAP and rn["candidate_blocks"] > 0 and all((b["weight"] == 0).all() for b in rn["tsdf"].values())
    assert MI.rotation_ok(T) and not MI.rotation_ok(np.diag([1, 1, -1, 1]).astype(F32)) and not MI.rotation_ok((np.eye(4) * 1.001).astype(F32))
