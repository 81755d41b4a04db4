"""The ESDF of the product on DRAWN site sets, across the whole radius range (tests/esdf_independent.py: the truth, the block writer, the patterns;
tests/test_esdf_model.py validates those on the CPU).

Every case: a fresh Mapper with a small block_capacity, set_blocks of the drawn TSDF, update_esdf(), ALL ESDF blocks read back.  Then
  1. is_site of the slice == the drawn pattern (and observed / inside as drawn),
  2. squared_distance_vox of EVERY allocated ESDF voxel == the brute force, bit for bit,
  3. the parents are valid (independent of any tie rule), non-zero exactly where a site counts,
  4. the same map in the CPU checker gives identical blocks, parents included (the tie rule).
Nothing is sampled, masked out or tolerated.

WHICH LAUNCH carried the transform is asserted from the mapper's launch profile -- by elimination, since a profile names launches, not what rode
in them: the ESDF voxels are written by the distance transform alone, so a correct field with no k_esdf_edt launch was carried by another one.
  (a) stand-alone: k_esdf_edt is in the profile (every test below but the carrier test reads straight after update_esdf: this path).
  (b) in k_mark_view (256-thread workgroups): colour deferral off, update_esdf launches k_esdf_mark and arms the transform, the next depth
      frame carries it; the profile has no k_esdf_edt and, of the two launches of that frame, only k_mark_view holds the transform's code
      (k_integrate_tsdf has none).  Confirmed by elimination.
  (c) in the fused launch (512-thread workgroups): the pipelined order; the profile has no k_esdf_edt and no k_esdf_mark (the marking pass rode in
      k_mark_view, and the transform is armed only after that launch is enqueued), and one k_integrate_tsdf_color.  Confirmed by elimination.
"""
import re

import numpy as np
import pytest

import esdf_cases as EC
import esdf_independent as EI
import helpers as H

pytestmark = pytest.mark.gpu

# the repeats at other voxel sizes run a part of the catalogue: patterns are trimmed there, radii are not
REPEAT_PATTERNS = ("single_centre", "tie_four", "reach+x", "reach-y", "cutoff_inside", "cutoff_outside", "full_row", "random_sparse", "holes")


def _M():
    from isaac_ros_nvblox_amd import mapper as M
    return M


def _capacity(n_blocks):
    cap = 1 << 10
    while cap < n_blocks + n_blocks // 4 + 64:
        cap *= 2
    return cap


def _read(M, g):
    return H.map_state(g, layers=(M.LAYER_ESDF,))["layers"][M.LAYER_ESDF]


def _kernels(g):
    names = {}
    for k, v in g.profile().items():
        m = re.match(r"\s*(?:void\s+)?(k_[a-z_0-9]+)", k)
        if m:
            names[m.group(1)] = names.get(m.group(1), 0) + v["count"]
    return names


def _run_2d(M, oracle_mod, tag, case, pg, q, propagation=False):
    """One drawn 2-D case through the product and the checker; returns the product's fields."""
    where = EI.alloc_voxels(case.alloc)
    idx, data = EI.tsdf_blocks_2d(case.sites, case.alloc, pg)
    g = M.Mapper(pg, block_capacity=_capacity(len(idx)))
    g.set_blocks(M.LAYER_TSDF, idx, data)
    g.update_esdf()
    gi, gb = _read(M, g)
    f, _ = EI.slice_fields(gi, gb, pg, (0, 0), case.alloc.shape)
    if propagation:
        assert np.array_equal(f.dom, where) and np.array_equal(f.site, case.sites), (tag, "sites / allocation")
        ref = EI.numpy_propagation(case.sites, where, EI.cutoff(q)[0])
        bad = where & (f.sq != ref)
        assert not bad.any(), (tag, "differs from numpy_propagation at", np.argwhere(bad)[:5].tolist(), f.sq[bad][:5].tolist(), ref[bad][:5].tolist())
        EI.check_parents(case.sites, f.sq, f.parent, where, q)
        exact, _ = EI.edt_bruteforce(case.sites, where, q)
        EC.assert_propagation_against_exact(tag, case, f.sq, exact, q)
    else:
        EC.assert_field(tag, f, case.sites, where, q, 2)
    o = EC.oracle_map(oracle_mod, pg, idx, data)
    o.update_esdf()
    oi, ob = EC.oracle_esdf(oracle_mod, o)
    EC.assert_same_blocks(tag, gi, gb, oi, ob)
    g.close()
    return f


@pytest.mark.parametrize("r,voxel_size", [(r, EC.VOXEL) for r in EC.RADII_2D] + EC.REPEATS_2D, ids=lambda v: str(v))
def test_exact_transform_on_drawn_patterns(oracle_mod, hip_lib, r, voxel_size):
    """The radius sweep of the exact 2-D transform (stand-alone k_esdf_edt): rb 1 .. 8, the strip of 8 + 2 ri rows up to 134, the 64-bit word
    edges of the row pass (rb 7: ri 49 .. 56, rb 8: ri 57 .. 63), the packing at ri 63, r < 1 (only the sites have a distance) and the last
    accepted radius; three radii again at two other voxel sizes, where the float32 quotient differs."""
    M = _M()
    pg, q = EC.params(M, r, voxel_size)
    n = 0
    for case in EI.patterns_2d(q):
        if voxel_size != EC.VOXEL and case.name not in REPEAT_PATTERNS:
            continue
        _run_2d(M, oracle_mod, (r, voxel_size, case.name), case, pg, q)
        n += 1
    assert n >= len(REPEAT_PATTERNS)


@pytest.mark.parametrize("r", EC.RADII_PROPAGATION, ids=EC.radius_id)
def test_iterative_propagation_on_drawn_patterns(oracle_mod, hip_lib, r):
    """esdf_propagation = 1 on the drawn patterns, the allocation with holes included: == numpy_propagation bit for bit, valid parents, the checker's
    blocks; against the exact brute force as EC.assert_propagation_against_exact states it."""
    M = _M()
    pg, q = EC.params(M, r, EC.VOXEL, esdf_propagation=1)
    for case in EI.patterns_2d(q):
        _run_2d(M, oracle_mod, (r, "propagation", case.name), case, pg, q, propagation=True)


def _blocks_of(idx, data, columns):
    """The rows of (idx, data) whose (bx, by) is one of `columns`."""
    keep = np.array([(int(i[0]), int(i[1])) in columns for i in idx], bool)
    assert keep.any()
    return idx[keep], data[keep]


@pytest.mark.parametrize("r", [9, 57, "57up"], ids=EC.radius_id)
def test_edits_between_updates_2d(oracle_mod, hip_lib, r):
    """The incremental window (dirty AABB + rb) must recompute every voxel a REMOVED site used to own: after a first update the one block that
    holds sites is overwritten with free space, a site appears in a far corner and an unrelated block is overwritten with identical content;
    then the last site goes.  After each update the whole field == the brute force of the NEW site set (a voxel still carrying the removed
    site's distance or parent fails), and == the checker."""
    M = _M()
    pg, q = EC.params(M, r, EC.VOXEL)
    nb = EI.field_blocks_2d(q); N = 8 * nb; cb = nb // 2
    alloc = np.ones((nb, nb), bool); where = EI.alloc_voxels(alloc)
    s0 = np.zeros((N, N), bool); s0[8 * cb + 2, 8 * cb + 5] = True; s0[8 * cb + 7, 8 * cb] = True
    s1 = np.zeros((N, N), bool); s1[8 * (nb - 1) + 6, 3] = True                      # far corner: block (bx 0, by nb - 1)
    s2 = np.zeros((N, N), bool)
    idx, data = EI.tsdf_blocks_2d(s0, alloc, pg)
    g = M.Mapper(pg, block_capacity=_capacity(len(idx)))
    o = EC.oracle_map(oracle_mod, pg, idx, data)
    g.set_blocks(M.LAYER_TSDF, idx, data)

    def update_and_check(tag, sites):
        g.update_esdf(); o.update_esdf()
        gi, gb = _read(M, g)
        f, _ = EI.slice_fields(gi, gb, pg, (0, 0), alloc.shape)
        EC.assert_field((r, tag), f, sites, where, q, 2)
        oi, ob = EC.oracle_esdf(oracle_mod, o)
        EC.assert_same_blocks((r, tag), gi, gb, oi, ob)
        return f

    f0 = update_and_check("first update", s0)
    assert (f0.sq < EI.cutoff(q)[0]).sum() > 100
    i1, d1 = EI.tsdf_blocks_2d(s1, alloc, pg)
    i1, d1 = _blocks_of(i1, d1, {(cb, cb), (0, nb - 1), (nb - 1, 0)})                # sites' block -> free, corner gets a site, an unrelated block as it was
    g.set_blocks(M.LAYER_TSDF, i1, d1); EC.oracle_set(oracle_mod, o, i1, d1)
    update_and_check("a site removed, one added far away", s1)
    i2, d2 = EI.tsdf_blocks_2d(s2, alloc, pg)
    i2, d2 = _blocks_of(i2, d2, {(0, nb - 1)})
    g.set_blocks(M.LAYER_TSDF, i2, d2); EC.oracle_set(oracle_mod, o, i2, d2)
    f2 = update_and_check("the last site removed", s2)
    assert (f2.sq[where] == EI.cutoff(q)[0]).all() and not f2.parent.any()
    g.close()


FAR_CAM = H.SMALL_CAM


def _far_frame(k):
    """A depth + colour frame of a wall 1.03 m in front of a camera 120 m (+ 3 m per k) from the drawn field, looking up through the slice's z band."""
    T = np.eye(4, dtype=np.float32); T[0, 3] = 120.0 + 3.0 * k; T[1, 3] = 1.0; T[2, 3] = -1.0
    return np.full((FAR_CAM[5], FAR_CAM[4]), 1.03, np.float32), np.full((FAR_CAM[5], FAR_CAM[4], 3), 90, np.uint8), T


@pytest.mark.parametrize("r", EC.RADII_CARRIERS, ids=EC.radius_id)
def test_same_field_from_all_three_carriers(oracle_mod, hip_lib, r):
    """The same field out of all three carriers of esdf_edt_worker (module docstring: (a) k_esdf_edt, (b) k_mark_view, 256 threads, (c) the fused
    launch, 512 threads), each asserted from the launch profile.  The far-away frames of (b) and (c) add blocks and sites of their own: the brute
    force runs over the product's full read-back site set, the drawn region's sites are asserted to be the drawn ones, and the drawn region of
    (b) and (c) equals (a)'s -- which the sweep above ties to the checker -- in every field."""
    M = _M()
    pg, q = EC.params(M, r, EC.VOXEL)
    cases = {c.name: c for c in EI.patterns_2d(q)}
    for name in ("random_sparse", "cutoff_inside", "full_row"):
        case = cases[name]
        where = EI.alloc_voxels(case.alloc); N = where.shape[0]
        idx, data = EI.tsdf_blocks_2d(case.sites, case.alloc, pg)
        fields = {}
        for carrier in "abc":
            tag = (r, name, carrier)
            g = M.Mapper(pg, block_capacity=1 << 13)
            if carrier == "b":
                g.set_color_deferral(False)
            g.set_blocks(M.LAYER_TSDF, idx, data)
            g.set_profiling(True)
            if carrier == "a":
                g.update_esdf()
            elif carrier == "b":
                g.update_esdf()
                d, _, T = _far_frame(0); g.integrate_depth(d, T, FAR_CAM)
            else:
                d, rgb, T = _far_frame(0)
                g.integrate_depth(d, T, FAR_CAM); g.integrate_color(rgb, T, FAR_CAM); g.update_esdf()
                d, _, T = _far_frame(1); g.integrate_depth(d, T, FAR_CAM)
            k = _kernels(g)
            if carrier == "a":
                assert k.get("k_esdf_edt", 0) == 1 and not {"k_mark_view", "k_integrate_tsdf_color"} & set(k), (tag, k)
            elif carrier == "b":
                assert k.get("k_esdf_edt", 0) == 0 and k.get("k_esdf_mark", 0) == 1 and k.get("k_mark_view", 0) == 1 and k.get("k_integrate_tsdf", 0) == 1 \
                    and "k_integrate_tsdf_color" not in k, (tag, k)
            else:
                assert k.get("k_esdf_edt", 0) == 0 and k.get("k_esdf_mark", 0) == 0 and k.get("k_mark_view", 0) == 2 and k.get("k_integrate_tsdf_color", 0) == 1 \
                    and k.get("k_integrate_color", 0) == 0, (tag, k)
            g.set_profiling(False)
            gi, gb = _read(M, g)
            f, origin = EI.slice_fields(gi, gb, pg)
            sq, cnt = EI.edt_bruteforce(f.site, f.dom, q)
            bad = f.dom & (f.sq != sq)
            assert not bad.any(), (tag, "differs from the brute force at", np.argwhere(bad)[:5].tolist(), f.sq[bad][:5].tolist(), sq[bad][:5].tolist())
            EI.check_parents(f.site, f.sq, f.parent, f.dom, q)
            assert np.array_equal((f.parent != 0).any(-1)[f.dom], ((cnt > 0) & ~f.site)[f.dom]), tag
            if carrier == "c":
                assert f.dom.sum() > where.sum() and f.site.sum() > case.sites.sum(), (tag, "the far frame's own blocks and sites are in the layer")
            y0, x0 = -origin[1] * 8, -origin[0] * 8
            crop = EI.Fields(*[a[y0:y0 + N, x0:x0 + N] for a in f])
            assert np.array_equal(crop.dom, where) and np.array_equal(crop.site, case.sites), (tag, "the drawn region's sites")
            fields[carrier] = crop
            g.close()
        for carrier in "bc":
            for a, b, what in zip(fields["a"], fields[carrier], EI.Fields._fields):
                assert np.array_equal(a, b), (r, name, carrier, what, "differs from the stand-alone launch's")
    # (a)'s field against the checker: test_exact_transform_on_drawn_patterns, same patterns, same radii


def _run_3d(M, oracle_mod, tag, case, pg, q):
    where = EI.alloc_voxels(case.alloc)
    idx, data = EI.tsdf_blocks_3d(case.sites, case.alloc, pg)
    g = M.Mapper(pg, block_capacity=_capacity(len(idx)))
    g.set_blocks(M.LAYER_TSDF, idx, data)
    g.update_esdf()
    gi, gb = _read(M, g)
    f, _ = EI.volume_fields(gi, gb, (0, 0, 0), case.alloc.shape)
    sq, _ = EC.assert_field(tag, f, case.sites, where, q, 3)
    o = EC.oracle_map(oracle_mod, pg, idx, data)
    o.update_esdf()
    oi, ob = EC.oracle_esdf(oracle_mod, o)
    EC.assert_same_blocks(tag, gi, gb, oi, ob)
    _dense_grid_check(tag, g, pg, sq, case.sites, where)
    g.close()


def _dense_grid_check(tag, g, pg, sq, sites, where):
    """esdf_dense_grid over the whole box == +-sqrt(sq) * voxel_size in float32 from the brute force (inside = the sites), the default elsewhere."""
    dense = g.esdf_dense_grid((0, 0, 0), where.shape, 1000.0)
    want = np.sqrt(sq) * np.float32(pg.voxel_size)
    want = np.where(where, np.where(sites, -want, want), np.float32(1000.0)).astype(np.float32)
    assert dense.shape == want.shape and np.array_equal(dense, want), (tag, "esdf_dense_grid", np.argwhere(dense != want)[:5].tolist())


@pytest.mark.parametrize("r", EC.RADII_3D, ids=EC.radius_id)
def test_exact_transform_3d_on_drawn_patterns(oracle_mod, hip_lib, r):
    """esdf_mode = 1 on drawn 3-D site sets: (2 rb + 3)^3 blocks, capped at 7^3 -- beyond that (r = 20) three axis-aligned strips and one
    diagonal strip through the site block; all three parent components, the flags and esdf_dense_grid against the same truth."""
    M = _M()
    pg, q = EC.params(M, r, EC.VOXEL, esdf_mode=1)
    for case in EI.patterns_3d(q):
        _run_3d(M, oracle_mod, (r, "3d", case.name), case, pg, q)


def test_exact_transform_3d_at_the_top_of_the_range(oracle_mod, hip_lib):
    """r = 63 in 3-D, the sites in one block and only the strips allocated: the 8-bit offset and 16-bit distance fields of the y- and z-pass keys
    at their widest, and the host-sized scratch window of changed blocks + 2 R at its largest per changed block."""
    M = _M()
    pg, q = EC.params(M, 63, EC.VOXEL, esdf_mode=1)
    _run_3d(M, oracle_mod, (63, "3d", "one_block"), EI.one_block_3d(q), pg, q)


def test_edits_between_updates_3d(oracle_mod, hip_lib):
    """The 3-D scratch window (changed blocks + 2 R) after an edit, r = 9: the sites' block overwritten with free space, a site added in a far
    corner block, an unrelated block rewritten as it was; then the last site removed."""
    M = _M()
    r = 9
    pg, q = EC.params(M, r, EC.VOXEL, esdf_mode=1)
    nb = EI.field_blocks_3d(q); N = 8 * nb; cb = nb // 2
    alloc = np.ones((nb, nb, nb), bool); where = EI.alloc_voxels(alloc)
    s0 = np.zeros((N, N, N), bool); s0[8 * cb + 2, 8 * cb + 5, 8 * cb] = True; s0[8 * cb + 7, 8 * cb, 8 * cb + 7] = True
    s1 = np.zeros((N, N, N), bool); s1[3, 8 * (nb - 1) + 6, 8 * (nb - 1) + 1] = True
    s2 = np.zeros((N, N, N), bool)
    idx, data = EI.tsdf_blocks_3d(s0, alloc, pg)
    g = M.Mapper(pg, block_capacity=_capacity(len(idx)))
    o = EC.oracle_map(oracle_mod, pg, idx, data)
    g.set_blocks(M.LAYER_TSDF, idx, data)

    def update_and_check(tag, sites):
        g.update_esdf(); o.update_esdf()
        gi, gb = _read(M, g)
        f, _ = EI.volume_fields(gi, gb, (0, 0, 0), alloc.shape)
        sq, _ = EC.assert_field((r, "3d", tag), f, sites, where, q, 3)
        oi, ob = EC.oracle_esdf(oracle_mod, o)
        EC.assert_same_blocks((r, "3d", tag), gi, gb, oi, ob)
        _dense_grid_check((r, "3d", tag), g, pg, sq, sites, where)
        return f

    def rows(sites, blocks):
        i, d = EI.tsdf_blocks_3d(sites, alloc, pg)
        keep = np.array([tuple(v) in blocks for v in i.tolist()], bool)
        assert keep.sum() == len(blocks)
        return i[keep], d[keep]

    update_and_check("first update", s0)
    i1, d1 = rows(s1, {(cb, cb, cb), (0, nb - 1, nb - 1), (nb - 1, 0, 0)})
    g.set_blocks(M.LAYER_TSDF, i1, d1); EC.oracle_set(oracle_mod, o, i1, d1)
    update_and_check("a site removed, one added far away", s1)
    i2, d2 = rows(s2, {(0, nb - 1, nb - 1)})
    g.set_blocks(M.LAYER_TSDF, i2, d2); EC.oracle_set(oracle_mod, o, i2, d2)
    f2 = update_and_check("the last site removed", s2)
    assert (f2.sq[where] == EI.cutoff(q)[0]).all() and not f2.parent.any()
    g.close()


@pytest.mark.parametrize("r_bad", [64, 100], ids=EC.radius_id)
@pytest.mark.parametrize("mode", [0, 1], ids=["2d", "3d"])
def test_radius_limit(oracle_mod, hip_lib, mode, r_bad):
    """esdf_max_distance_m / voxel_size >= 64 voxels: update_esdf raises NvbxError with the library's message, the map is untouched (TSDF and ESDF
    layers byte-identical to before, an edit still waiting), and after set_params back to a legal radius the next update is correct."""
    M = _M()
    r = 9
    pg, q = EC.params(M, r, EC.VOXEL, esdf_mode=mode)
    if mode == 0:
        case = {c.name: c for c in EI.patterns_2d(q)}["random_sparse"]
        build, fields, dims = EI.tsdf_blocks_2d, lambda i, b: EI.slice_fields(i, b, pg, (0, 0), case.alloc.shape)[0], 2
    else:
        case = EI.patterns_3d(q)[-1]
        build, fields, dims = EI.tsdf_blocks_3d, lambda i, b: EI.volume_fields(i, b, (0, 0, 0), case.alloc.shape)[0], 3
    where = EI.alloc_voxels(case.alloc)
    idx, data = build(case.sites, case.alloc, pg)
    g = M.Mapper(pg, block_capacity=_capacity(len(idx)))
    g.set_blocks(M.LAYER_TSDF, idx, data)
    g.update_esdf()
    EC.assert_field((mode, "before"), fields(*_read(M, g)), case.sites, where, q, dims)
    # an edit that the refused update must leave waiting: one more site in the first allocated block
    sites2 = case.sites.copy()
    first = np.argwhere(where & ~case.sites)[0]
    sites2[tuple(first)] = True
    i2, d2 = build(sites2, case.alloc, pg)
    changed = np.array([not np.array_equal(d2[k], data[k]) for k in range(len(i2))], bool)
    assert np.array_equal(i2, idx) and changed.any()
    g.set_blocks(M.LAYER_TSDF, i2[changed], d2[changed])
    before = H.map_state(g, layers=(M.LAYER_TSDF, M.LAYER_ESDF))
    bad_m = EI.distance_at_least_radius(64, EC.VOXEL) if r_bad == 64 else EI.distance_for_radius(r_bad, EC.VOXEL)
    assert EI.radius_of(bad_m, EC.VOXEL)[0] >= 64
    g.set_params(M.default_params(voxel_size=EC.VOXEL, esdf_max_distance_m=bad_m, esdf_mode=mode))
    for _ in range(2):
        with pytest.raises(M.NvbxError, match="esdf_max_distance_m / voxel_size must be < 64 voxels"):
            g.update_esdf()
    H.assert_same_map(before, g, (mode, r_bad, "the refused update changed the map"))
    g.set_params(pg)
    g.update_esdf()
    EC.assert_field((mode, "after"), fields(*_read(M, g)), sites2, where, q, dims)
    g.close()
