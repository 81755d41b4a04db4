"""The numpy model of frontiers and view gain (tests/frontier_independent.py) against restatements that share nothing with it: a brute-force
dense-array frontier count (pad with unknown, shift six ways, count), scipy.ndimage.label for the clusters, and an analytic scene for the view
gain.  No GPU, no product code."""
import numpy as np
import pytest

import frontier_independent as FI

F32 = np.float32
VS = 0.05
MIN_W = 1e-4
FREE_D = 0.05


def _dense_to_blocks(d, w, origin_block=(0, 0, 0), drop=()):
    """dense float32 volumes [8a, 8b, 8c] indexed [x, y, z] -> {block: TSDF_DT[512]}, the block positions in `drop` left out"""
    nb = [s // 8 for s in d.shape]
    out = {}
    for bx in range(nb[0]):
        for by in range(nb[1]):
            for bz in range(nb[2]):
                if (bx, by, bz) in drop:
                    continue
                v = np.zeros(512, FI.TSDF_DT)
                sl = (slice(8 * bx, 8 * bx + 8), slice(8 * by, 8 * by + 8), slice(8 * bz, 8 * bz + 8))
                v["distance"] = d[sl].reshape(512); v["weight"] = w[sl].reshape(512)
                out[(bx + origin_block[0], by + origin_block[1], bz + origin_block[2])] = v
    return out


def _brute_force(d, w, drop, min_unknown):
    """the frontier rule on the dense volume: -> (frontier mask, nu) over the whole volume"""
    obs = w >= F32(MIN_W)
    for (bx, by, bz) in drop:
        obs[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8] = False        # a block that does not exist
    free = obs & (d > F32(FREE_D))
    unk = np.pad(~obs, 1, constant_values=True).astype(np.int32)
    n = d.shape
    nu = np.zeros(n, np.int32)
    for ax in range(3):
        for sh in (0, 2):
            sl = [slice(1, 1 + n[0]), slice(1, 1 + n[1]), slice(1, 1 + n[2])]
            sl[ax] = slice(sh, sh + n[ax])
            nu += unk[tuple(sl)]
    return free & (nu >= min_unknown), nu


def _volumes():
    rng = np.random.default_rng(11)
    out = {}
    # random classes: a third each of unknown, free, occupied; one block missing
    d = rng.choice(np.array([0.2, 0.0, -0.1, FREE_D], F32), size=(24, 16, 16)).astype(F32)
    w = rng.choice(np.array([0.0, 1.0, 5e-5, 1e-4], F32), size=(24, 16, 16)).astype(F32)
    out["random"] = (d, w, ((1, 1, 0),))
    # a hollow box: occupied walls, free inside, an unobserved core; the space outside the walls unobserved
    d = np.full((24, 24, 24), 0.2, F32); w = np.zeros((24, 24, 24), F32)
    w[4:20, 4:20, 4:20] = 1.0; d[4:20, 4:20, 4:20] = -0.05
    d[5:19, 5:19, 5:19] = 0.2
    w[10:14, 7:17, 10:14] = 0.0
    out["hollow_box"] = (d, w, ())
    out["hollow_box_block_missing"] = (d, w, ((1, 1, 1),))
    # one free voxel in the void
    d = np.zeros((8, 8, 8), F32); w = np.zeros((8, 8, 8), F32)
    d[3, 4, 5] = 0.2; w[3, 4, 5] = 1.0
    out["single_voxel"] = (d, w, ())
    # fully observed: free inside an occupied shell that reaches the border of the volume
    d = np.full((16, 16, 16), -0.02, F32); w = np.ones((16, 16, 16), F32)
    d[1:15, 1:15, 1:15] = 0.3
    out["fully_observed"] = (d, w, ())
    # NaN distances are observed and not free
    d = np.full((8, 8, 8), 0.2, F32); w = np.ones((8, 8, 8), F32)
    d[0, :, :] = np.nan
    out["nan_distance"] = (d, w, ())
    return out


VOLUMES = _volumes()


@pytest.mark.parametrize("name", list(VOLUMES))
@pytest.mark.parametrize("min_unknown", [1, 2, 3, 6])
def test_frontier_set_equals_the_dense_restatement(name, min_unknown):
    d, w, drop = VOLUMES[name]
    origin = (-2, 0, -1)                                    # negative block indices among them
    fr = FI.frontiers(_dense_to_blocks(d, w, origin, drop), MIN_W, FREE_D, min_unknown)
    mask, nu = _brute_force(d.copy(), w.copy(), drop, min_unknown)
    want = {}
    for bx in range(d.shape[0] // 8):
        for by in range(d.shape[1] // 8):
            for bz in range(d.shape[2] // 8):
                sl = (slice(8 * bx, 8 * bx + 8), slice(8 * by, 8 * by + 8), slice(8 * bz, 8 * bz + 8))
                if mask[sl].any():
                    want[(bx + origin[0], by + origin[1], bz + origin[2])] = (np.where(mask[sl], 0, -1).reshape(512), np.where(mask[sl], nu[sl], 0).reshape(512))
    assert set(fr) == set(want)
    for k in want:
        assert np.array_equal(fr[k][0], want[k][0]) and np.array_equal(fr[k][1], want[k][1].astype(F32)), k
    if name == "single_voxel":
        assert (len(fr) == 1 and fr[origin][1].max() == 6 and (fr[origin][0] == 0).sum() == 1)
    if name == "fully_observed":
        assert not fr
    if name == "nan_distance" and min_unknown == 1:
        assert (fr[origin][0].reshape(8, 8, 8)[0] == -1).all() and (fr[origin][0] == 0).sum() == 7 * 64 - 6 * 36      # (x = 1 .. 6, y, z = 1 .. 6 are inside)


def test_box_and_metres():
    d, w, drop = VOLUMES["hollow_box"]
    blocks = _dense_to_blocks(d, w)
    box = FI.box_from_metres(((0.0, 0.0, 0.0), (0.59, 1.19, 0.61)), VS)
    assert box == (0, 0, 0, 11, 23, 12)
    fr = FI.frontiers(blocks, MIN_W, FREE_D, 1, box)
    mask, _ = _brute_force(d.copy(), w.copy(), (), 1)
    mask[12:, :, :] = False; mask[:, :, 13:] = False
    got = np.zeros_like(mask)
    for (bx, by, bz), (lab, _) in fr.items():
        got[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8] = lab.reshape(8, 8, 8) == 0
    assert np.array_equal(got, mask) and mask.any()
    assert FI.box_from_metres(((-0.01, -0.05, -0.051), (0.0, 0.0, 0.0)), VS)[:3] == (-1, -1, -2)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", ["random", "hollow_box", "hollow_box_block_missing", "single_voxel"])
def test_clusters_equal_scipy_label(name, connectivity):
    from scipy import ndimage
    d, w, drop = VOLUMES[name]
    fr = FI.frontiers(_dense_to_blocks(d, w, (0, 0, 0), drop), MIN_W, FREE_D, 1)
    comps, keys = FI.clusters(fr, connectivity, 1)
    mask, nu = _brute_force(d.copy(), w.copy(), drop, 1)
    # (a block without a frontier voxel is not in the list and holds none: it separates nothing that the dense labelling would join)
    cc, k = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    assert len(comps) == k
    sizes = sorted(int(v) for v in np.bincount(cc.ravel())[1:])
    assert sorted(c[1] for c in comps.values()) == sizes
    for low, (label, voxels, mn, mx, sums, peak_bits, peak_xyz) in comps.items():
        member = cc == cc[low]
        xyz = np.argwhere(member)
        assert label == 0 and voxels == len(xyz) and tuple(xyz.min(0)) == mn and tuple(xyz.max(0)) == mx and tuple(xyz.sum(0)) == sums
        best = nu[member].max()
        assert np.uint32(peak_bits).view(F32) == F32(best) and nu[peak_xyz] == best and member[peak_xyz]
    comps5, _ = FI.clusters(fr, connectivity, 5)
    assert len(comps5) == sum(1 for s in sizes if s >= 5)


# ---- view gain on an analytic scene: free space from x = 0 to a slab that starts at voxel 20 (1.0 m), seen straight on from x = 0.01
def _slab_scene(depth_blocks=3):
    out = {}
    for bx in range(depth_blocks):
        for by in range(-2, 2):
            for bz in range(-2, 2):
                v = np.zeros(512, FI.TSDF_DT)
                gx = 8 * bx + FI.OFF[:, 0]
                v["distance"] = np.where(gx >= 20, -0.02, 0.2).astype(F32); v["weight"] = 1.0
                out[(bx, by, bz)] = v
    return out


def _pose_plus_x(o):
    # camera z (forward) = layer +x, camera x (right) = layer -y, camera y (down) = layer -z
    T = np.eye(4, dtype=F32)
    T[:3, 0] = (0, -1, 0); T[:3, 1] = (0, 0, -1); T[:3, 2] = (1, 0, 0); T[:3, 3] = o
    return T


def test_view_gain_straight_on():
    scene = _slab_scene()
    T = _pose_plus_x((0.01, 0.012, 0.013))
    cam = (1000.0, 1000.0, 1.0, 1.0, 2, 2)                  # four rays within 0.03 degrees of the axis: sample k lies in voxel x = k
    assert FI.view_gain(scene, [T], cam, 1, 5.0, VS, MIN_W, FREE_D).tolist() == [[4, 0, 80, 4]]
    # a range that ends before the slab: samples k = 0 .. 15 (t_15 = 0.775 < 0.8 <= t_16), no hit
    assert FI.view_gain(scene, [T], cam, 1, 0.8, VS, MIN_W, FREE_D).tolist() == [[4, 0, 64, 0]]
    # the slab's blocks missing: 16 free samples, then unknown ones to the end of the range (t_k < 1.5: k <= 29)
    assert FI.view_gain(_slab_scene(2), [T], cam, 1, 1.5, VS, MIN_W, FREE_D).tolist() == [[4, 4 * 14, 64, 0]]
    # an empty map: every sample unknown; poses that are not finite or out of range
    bad = T.copy(); bad[1, 3] = np.nan
    far = T.copy(); far[0, 3] = 5e5
    assert FI.view_gain({}, [T, bad, far], cam, 1, 1.5, VS, MIN_W, FREE_D).tolist() == [[4, 120, 0, 0], [-1, 0, 0, 0], [-1, 0, 0, 0]]


def test_view_gain_wide_camera_against_the_analytic_count():
    scene = _slab_scene()
    o = np.array([0.01, 0.012, 0.013])
    cam = (8.0, 8.0, 3.9, 2.9, 8, 6)
    fu, fv, cu, cv, w, h = cam
    want_free = 0
    for r in range(h):
        for c in range(w):
            rx, ry = (c + 0.5 - cu) / fu, (r + 0.5 - cv) / fv
            dx = 1.0 / np.sqrt(rx * rx + ry * ry + 1.0)
            kf = (1.0 - o[0]) / (VS * dx) - 0.5                  # the first sample with x >= 1.0 is k = ceil(kf)
            assert abs(kf - round(kf)) > 1e-3, "a tie: move the camera"
            k_hit = int(np.ceil(kf))
            assert (k_hit + 0.5) * VS * max(abs(rx), abs(ry)) * dx < 0.75      # the ray stays inside the allocated blocks up to its hit
            want_free += k_hit
    got = FI.view_gain(scene, [_pose_plus_x(o)], cam, 1, 5.0, VS, MIN_W, FREE_D)
    assert got.tolist() == [[48, 0, want_free, 48]]
    # subsampling 2: the rays through pixels (2 r, 2 c)
    got2 = FI.view_gain(scene, [_pose_plus_x(o)], cam, 2, 5.0, VS, MIN_W, FREE_D)
    assert got2[0, 0] == 12 and got2[0, 3] == 12 and 0 < got2[0, 2] < want_free
