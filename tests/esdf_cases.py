"""What tests/test_esdf_model.py (CPU) and tests/test_gpu_esdf_drawn.py (GPU) share: the radius sweep, the parameters of a case, and how a drawn
case is put through the CPU checker and read back."""
import numpy as np

import esdf_independent as EI
import helpers as H

VOXEL = 0.05
# r = esdf_max_distance_m / voxel_size, as a caller writes it (float32(r * voxel_size); the float32 quotient is what comes out of that: "57" at
# 0.05 m is 56.999996, ri = 56) -- or, by name, a distance searched for its quotient: "57up" the smallest with quotient >= 57 (ri = 57, rb = 8
# with the smallest strip that has it), "below64" the largest with quotient < 64 (the last accepted radius)
RADII_2D = [0.5, 1, 1.5, 2.5, 7, 8, 9, 40, 48, 49, 56, 57, "57up", 62.5, 63, "below64"]
REPEATS_2D = [(2.5, 0.1), (9, 0.1), (63, 0.1), (2.5, 0.02), (9, 0.02), (63, 0.02)]          # the same nominal radius, another float32 quotient
RADII_3D = [1, 2.5, 7, 8, 9, 20]
RADII_PROPAGATION = [2.5, 9, 40, 63]
RADII_CARRIERS = [2.5, 9, 57, 63]


def radius_id(r):
    return "r" + str(r)


def distance_m(r, voxel_size=VOXEL):
    if r == "below64":
        return EI.distance_below_radius(64, voxel_size)
    if r == "57up":
        return EI.distance_at_least_radius(57, voxel_size)
    return EI.distance_for_radius(r, voxel_size)


def params(M, r, voxel_size=VOXEL, **kw):
    """The product's default parameters at this radius; (params, r as the float32 quotient)."""
    p = M.default_params(voxel_size=voxel_size, esdf_max_distance_m=distance_m(r, voxel_size), **kw)
    return p, EI.radius_of(p.esdf_max_distance_m, p.voxel_size)[0]


def oracle_map(oracle_mod, pg, idx, data):
    o = oracle_mod.OracleMap(H.copy_params(pg, oracle_mod.OrcParams))
    oracle_set(oracle_mod, o, idx, data)
    return o


def oracle_set(oracle_mod, o, idx, data):
    for i, b in zip(np.asarray(idx).tolist(), data):
        o.set_block(oracle_mod.L_TSDF, i, b)


def oracle_esdf(oracle_mod, o):
    idx = o.block_indices(oracle_mod.L_ESDF)
    return idx, [o.get_block(oracle_mod.L_ESDF, i) for i in idx]


def assert_same_blocks(tag, idx_a, blocks_a, idx_b, blocks_b):
    """Two read-backs of the ESDF layer hold the same blocks with the same voxels, every field of every voxel (all eight planes of a block), in
    whichever order each lists its blocks."""
    def state(idx, blocks):
        idx = np.asarray(idx, np.int32).reshape(-1, 3)
        order = np.lexsort(idx.T[::-1])
        return {"layers": {H.M.LAYER_ESDF: (idx[order], np.asarray(blocks).reshape(-1, 512)[order])}}
    H.assert_same_map(state(idx_a, blocks_a), state(idx_b, blocks_b), tag, fields={H.M.LAYER_ESDF: H.ESDF_FIELDS})


def assert_field(tag, f, sites, where, r, dims):
    """The four assertions every read-back field meets: (1) the slice's sites are the drawn ones and every allocated voxel is observed, inside
    exactly on the sites; (2) every allocated voxel's squared distance equals the brute force bit for bit; (3) the parents are valid, and
    non-zero exactly where a site counts.  `f`: EI.Fields; sites / where: the drawn pattern and the allocated voxels."""
    assert np.array_equal(f.dom, where), (tag, "allocated ESDF voxels differ from the drawn allocation")
    assert np.array_equal(f.site, sites), (tag, "is_site differs from the drawn pattern", np.argwhere(f.site != sites)[:5].tolist())
    assert np.array_equal(f.observed, where) and np.array_equal(f.inside, sites), (tag, "observed / inside flags")
    sq, cnt = EI.edt_bruteforce(sites, where, r)
    bad = where & (f.sq != sq)
    assert not bad.any(), (tag, "squared distance differs from the brute force at", np.argwhere(bad)[:5].tolist(), f.sq[bad][:5].tolist(), sq[bad][:5].tolist(), int(bad.sum()))
    EI.check_parents(sites, f.sq, f.parent, where, r)
    has_parent = (f.parent != 0).any(-1)
    want_parent = (cnt > 0) & ~sites
    assert np.array_equal(has_parent[where], want_parent[where]), (tag, "a parent exactly where a site counts", np.argwhere(where & (has_parent != want_parent))[:5].tolist())
    assert not f.parent[~where].any() and dims == sites.ndim
    return sq, cnt


def assert_propagation_against_exact(tag, case, sq, exact, r):
    """What iterative propagation owes the exact transform.  A propagated value is always the distance to a real site within the cut-off, so it
    can only OVER-estimate: sq >= exact on every allocated voxel, holes or not.  With ONE site and no holes it is exact: every voxel within the
    cut-off is reached along a staircase of axis steps on which the distance to the site only grows, so no step is cut off.  With several sites
    4-neighbour vector propagation is not exact even on a full field (a site's Voronoi cell need not be 4-connected: the known error of
    sequential / parallel vector distance transforms), so equality is asserted only against numpy_propagation, which restates the definition.
    On the allocation with holes the wall of missing blocks must show: some voxel is over-estimated once the radius reaches across a block
    (ri >= 9)."""
    where = EI.alloc_voxels(case.alloc)
    assert (sq[where] >= exact[where]).all(), (tag, "propagation under-estimates the exact distance")
    if case.name.startswith("single"):
        assert np.array_equal(sq[where], exact[where]), (tag, "one site, no holes: propagation is exact")
    if not case.alloc.all() and EI.cutoff(r)[1] >= 9:
        assert (sq[where] > exact[where]).any(), (tag, "the holes hide nothing from the iterative transform")
