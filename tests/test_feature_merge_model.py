"""The numpy model of feature merging (tests/feature_merge_independent.py; SEMANTICS.md "Feature merging") held to closed-form cases, on the
CPU: the candidate rule and the 3 x 3 x 3 reach bound by brute force, an identity and a whole-block merge that return the source's bits, the
exact weighted mean of two constant fields, the max_weight clamp.  Nothing of the library is loaded."""
import numpy as np
import pytest

import feature_merge_independent as FM

F32, F16 = np.float32, np.float16
VS = 0.05
pose = FM.pose

TRANSFORMS = {
    "identity": pose([0, 0, 1], 0.0, [0, 0, 0]),
    "whole_blocks": pose([0, 0, 1], 0.0, np.array([2, -1, 1]) * 8 * VS),
    "sub_voxel": pose([0, 0, 1], 0.0, np.array([0.5, -0.25, 0.125]) * VS),
    "small": pose([1, 2, 3], 1.5, [0.03, -0.01, 0.02]),
    "z90": pose([0, 0, 1], 90.0, [0.11, -0.27, 0.4]),
    "general_45": pose([1, 2, 3], 45.0, [0.37, -0.21, 0.13]),
    "general_45_far_negative": pose([3, -1, 2], 45.0, [-6.3, -5.1, -2.2]),
}


def _drawn():
    rng = np.random.default_rng(5)
    out = dict(TRANSFORMS)
    for i in range(8):
        out["drawn%d" % i] = pose(rng.normal(size=3), rng.uniform(0.0, 180.0), rng.uniform(-4.0, 4.0, 3))
    return out


def _hash_block(key, ch, seed=0):
    """per-voxel, per-channel distinct fp16 values and weights in {1, 2, 3}, a function of (block, voxel, channel)"""
    rng = np.random.default_rng([seed, key[0] + 1000, key[1] + 1000, key[2] + 1000])
    return rng.uniform(-4.0, 4.0, (512, ch)).astype(F16), rng.integers(1, 4, 512).astype(F32)


SRC_KEYS = [(x, y, z) for x in (-2, -1, 0) for y in (-1, 0, 1) for z in (-2, -1, 0)]


@pytest.mark.parametrize("name", list(_drawn()))
def test_no_block_outside_the_candidate_set_holds_a_voxel_of_the_source_block(name):
    """brute force: every destination block within four blocks of the source block's image, all 512 voxels each"""
    T = _drawn()[name]
    R_DS, t_DS, _, _ = FM.transforms(T)
    for s in [(0, 0, 0), (-1, -1, -1), (-3, 2, -7), (5, -4, 0)]:
        cand = FM.candidates(T, [s], VS)
        lo, hi = FM.candidate_boxes(T, [s], VS)
        assert ((hi - lo) <= 2).all() and len(cand) <= 27
        centre = R_DS.astype(np.float64) @ ((8.0 * np.array(s) + 4.0) * VS) + t_DS
        c = np.floor(centre / (8 * VS)).astype(np.int64)
        around = np.array([(c[0] + i, c[1] + j, c[2] + k) for i in range(-4, 5) for j in range(-4, 5) for k in range(-4, 5)], np.int64)
        n, ok = FM.source_voxels(T, around, VS)
        hit = (ok & ((n >> 3) == np.array(s)).all(-1)).any(1)
        assert hit.sum() >= 1
        outside = [tuple(b) for b in around[hit].tolist() if tuple(b) not in cand]
        assert not outside, (name, s, outside[:4])


def test_the_voxels_of_one_block_reach_at_most_three_source_blocks_per_axis_and_27_occur():
    rng = np.random.default_rng(9)
    blocks = rng.integers(-40, 40, (64, 3))
    most = 0
    for name, T in _drawn().items():
        r = FM.reach(T, blocks, VS)
        assert (r >= 1).all() and (r <= 3).all(), name
        most = max(most, int(r.prod(1).max()))
        if name.startswith("general_45"):
            assert int(r.prod(1).max()) == 27, name              # where the whole 3 x 3 x 3 table is used
    assert most == 27
    for name in ("identity", "whole_blocks"):
        assert (FM.reach(TRANSFORMS[name], blocks, VS) == 1).all()


@pytest.mark.parametrize("name,shift", [("identity", (0, 0, 0)), ("whole_blocks", (2, -1, 1))])
def test_a_merge_into_a_featureless_twin_returns_the_sources_bits(name, shift):
    ch = 16
    src = {k: _hash_block(k, ch) for k in SRC_KEYS}
    src[(0, 0, 0)][1][5] = 0.0                                     # a voxel of weight 0 inside a flagged block
    have = {tuple(np.add(k, shift)) for k in SRC_KEYS} | {(40, 40, 40)}
    r = FM.merge_features(have, {}, src, TRANSFORMS[name], VS, max_weight=5.0)
    assert r["status"] == FM.OK and r["source_blocks"] == 27 and r["candidate_blocks"] == 27 and r["blocks_flagged"] == 27
    assert r["voxels_fused"] == 27 * 512 - 1 and (40, 40, 40) not in r["feat"]
    for k in SRC_KEYS:
        f, w = r["feat"][tuple(np.add(k, shift))]
        fused = r["fused"][tuple(np.add(k, shift))]
        assert np.array_equal(w, src[k][1]) and np.array_equal(f[fused].view(np.uint16), src[k][0][fused].view(np.uint16))
        assert not f[~fused].any() and not w[~fused].any()
    assert not r["fused"][shift][5] and r["fused"][shift].sum() == 511


def test_the_blend_of_two_constant_fields_is_the_exact_weighted_mean_and_the_weight_is_clamped():
    ch = 8
    key = (-1, 0, 2)
    dst = {key: (np.full((512, ch), 0.5, F16), np.full(512, 1.0, F32))}
    src = {key: (np.full((512, ch), 2.5, F16), np.full(512, 3.0, F32))}
    T = TRANSFORMS["identity"]
    r = FM.merge_features({key}, dst, src, T, VS, max_weight=100.0)
    f, w = r["feat"][key]
    assert (f == F16(2.0)).all() and (w == F32(4.0)).all()         # 0.5 (1 / 4) + 2.5 (3 / 4), every term exact
    assert r["blocks_flagged"] == 0 and r["voxels_fused"] == 512
    r = FM.merge_features({key}, dst, src, T, VS, max_weight=3.5)
    assert (r["feat"][key][0] == F16(2.0)).all() and (r["feat"][key][1] == F32(3.5)).all()
    r = FM.merge_features({key}, dst, src, T, VS, max_weight=100.0, weight_scale=1.0 / 3.0)
    assert (r["feat"][key][1] == F32(1.0) + F32(3.0) * F32(1.0 / 3.0)).all()
    # min_weight above the source's: nothing contributes, nothing is flagged anywhere
    r = FM.merge_features({key}, {}, src, T, VS, max_weight=100.0, min_weight=3.5)
    assert r["status"] == FM.NO_OVERLAP and r["feat"] == {} and r["candidate_blocks"] == 1 and r["blocks_flagged"] == 0
    assert FM.merge_features({key}, dst, {}, T, VS, 100.0)["status"] == FM.EMPTY_SOURCE
    assert dst[key][1][0] == 1.0 and src[key][1][0] == 3.0       # the inputs are not modified
