"""The independent model of feature segmentation (tests/segment_independent.py) on cases whose answer is known in closed form, and its two
implementations (scipy.ndimage.label, a numpy union-find) against each other on the drawn volumes the GPU tests use."""
import numpy as np
import pytest

import segment_independent as SI


def _both(bidx, lab, sc, conn, min_voxels=1):
    a = SI.model(bidx, lab, sc, conn, min_voxels)
    b = SI.model_union_find(bidx, lab, sc, conn, min_voxels)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    return a


def test_parity_checkerboard_is_256_components_under_6_and_one_under_26():
    bidx, lab, _ = SI.cut(SI.checkerboard(), origin_block=(-1, 2, 0))
    c6, k6 = _both(bidx, lab, None, 6)
    c26, k26 = _both(bidx, lab, None, 26)
    assert len(c6) == 256 and all(v[1] == 1 for v in c6.values())
    assert len(c26) == 1
    (low, rec), = c26.items()
    assert low == (-8, 16, 0) and rec[:4] == (0, 256, (-8, 16, 0), (-1, 23, 7))
    assert rec[5] == 0 and rec[6] == low                       # no scores: the peak is 0 at the lowest voxel
    assert (k6 >= 0).sum() == 256 and len(np.unique(k6[k6 >= 0])) == 256 and len(np.unique(k26[k26 >= 0])) == 1


def test_voxels_that_touch_only_across_a_block_corner():
    L = np.full((16, 16, 16), -1, np.int32)
    L[7, 7, 7] = 0; L[8, 8, 8] = 0
    bidx, lab, _ = SI.cut(L, origin_block=(-1, -1, -1), seed=3)
    assert len(_both(bidx, lab, None, 6)[0]) == 2
    c, _ = _both(bidx, lab, None, 26)
    assert list(c.values()) == [(0, 2, (-1, -1, -1), (0, 0, 0), (-1, -1, -1), 0, (-1, -1, -1))]


def test_contacts_across_edges_and_corners_in_every_sign_pattern():
    bidx, lab, _ = SI.cut(SI.contacts(), origin_block=(-2, -2, -2))
    assert len(_both(bidx, lab, None, 6)[0]) == 10 and len(_both(bidx, lab, None, 26)[0]) == 5


def test_an_absent_middle_block_separates_its_two_sides():
    L = np.full((24, 8, 8), -1, np.int32)
    L[:, 4, 4] = 0                                                 # a bar along x through three blocks
    for conn in (6, 26):
        assert len(_both(*SI.cut(L), conn)[0]) == 1
        c, _ = _both(*SI.cut(L, drop=[(1, 0, 0)]), conn)
        assert sorted(v[1:4] for v in c.values()) == [(8, (0, 4, 4), (7, 4, 4)), (8, (16, 4, 4), (23, 4, 4))]


def test_touching_regions_of_different_labels_stay_apart():
    bidx, lab, _ = SI.cut(SI.side_by_side(), origin_block=(-2, -2, -2))
    for conn in (6, 26):
        c, _ = _both(bidx, lab, None, conn)
        assert sorted((v[0], v[1]) for v in c.values()) == [(0, 6 * 16 * 16), (1, 6 * 16 * 16)]


def test_a_peak_tie_picks_the_lowest_voxel_and_compares_as_floats():
    L = np.zeros((8, 8, 16), np.int32)
    S = np.full(L.shape, -1.0, np.float32)
    S[5, 1, 9] = 2.5; S[2, 7, 15] = 2.5; S[2, 7, 3] = 2.5; S[1, 0, 0] = np.nan; S[0, 0, 0] = -0.0
    bidx, lab, sc = SI.cut(L, S, seed=1)
    (low, rec), = _both(bidx, lab, sc, 6)[0].items()
    assert rec[5] == np.float32(2.5).view(np.uint32) and rec[6] == (2, 7, 3)
    S[:] = -0.0; S[3, 3, 3] = 0.0                                  # -0 counts as +0: all tie, the lowest voxel wins
    (low, rec), = _both(*SI.cut(L, S, seed=1), 6)[0].items()
    assert rec[5] == 0 and rec[6] == (0, 0, 0)
    S[:] = np.nan; S[4, 4, 4] = -3.0                               # a NaN counts as -infinity
    (low, rec), = _both(*SI.cut(L, S, seed=1), 6)[0].items()
    assert rec[5] == np.float32(-3.0).view(np.uint32) and rec[6] == (4, 4, 4)


def test_the_threshold_keeps_a_voxel_at_its_threshold():
    lab = np.array([[0, 0, 0, 1, 1, -1, 2]], np.int32); sc = np.array([[0.5, 0.49999997, 0.6, 0.1, -0.2, 0.0, 7.0]], np.float32)
    l2, s2 = SI.threshold(lab, sc, np.array([0.5, 0.0, np.nan], np.float32))
    assert l2.tolist() == [[0, -1, 0, 1, -1, -1, 2]]
    assert s2.tolist() == [[0.5, 0.0, np.float32(0.6), np.float32(0.1), 0.0, 0.0, 7.0]]


@pytest.mark.parametrize("n,blocks", [(8, 1), (24, 27)])
def test_the_serpentine_is_one_component(n, blocks):
    L = SI.serpentine(n)
    half = n // 2
    voxels = half * (half * n + half - 1) + (half - 1)              # per plane: the full rows and their joints; then the joints between planes
    assert int((L == 0).sum()) == voxels
    bidx, lab, _ = SI.cut(L, origin_block=(-2, -2, -2))
    assert len(bidx) == blocks
    for conn in (6, 26):
        (low, rec), = _both(bidx, lab, None, conn)[0].items()
        assert rec[1] == voxels and low == (-16, -16, -16)
    if blocks == 27:                                               # without the middle block it falls apart
        assert len(_both(*SI.cut(L, origin_block=(-2, -2, -2), drop=[(1, 1, 1)]), 6)[0]) > 1


def test_the_u_joins_its_arms_only_in_the_farthest_blocks():
    L = SI.u_shape()
    for conn in (6, 26):
        (low, rec), = _both(*SI.cut(L, origin_block=(-2, -2, -2)), conn)[0].items()
        assert low == (-16, -13, -13) and rec[:2] == (2, 24 + 24 + 15)
        c, _ = _both(*SI.cut(L, origin_block=(-2, -2, -2), drop=[(2, 1, 0)]), conn)      # the joint's middle block taken away: two arms
        assert sorted(v[1] for v in c.values()) == [24 + 3, 24 + 4]                  # (y = 16 .. 18 beside the far arm, y = 4 .. 7 beside the near one)


def test_noise_above_the_percolation_density_has_giants_under_6_and_nearly_one_component_under_26():
    L, s, sq = SI.noise((24, 24, 24))
    bidx, lab, sc = SI.cut(L, sq, origin_block=(-2, -2, -2), seed=7)
    c6, _ = _both(bidx, lab, sc, 6)
    for l in (0, 1):
        sizes = sorted(v[1] for v in c6.values() if v[0] == l)
        print("label %d, connectivity 6: %d components, largest %d voxels" % (l, len(sizes), sizes[-1]))
        assert len(sizes) > 200 and sizes[-1] > 3000
    c26, _ = _both(bidx, lab, sc, 26)
    print("connectivity 26: %d components" % len(c26))
    assert len(c26) <= 6
    # peaks tie on the quantised scores: a giant's peak is the top level, at a voxel that is not simply its lowest one
    giant = max(c6.values(), key=lambda v: v[1])
    assert giant[5] == np.float32(0.25).view(np.uint32)
    for mv in (2, 5):
        c, k = _both(bidx, lab, sc, 6, mv)
        assert c == {key: v for key, v in c6.items() if v[1] >= mv} and 0 < len(c) < len(c6)
