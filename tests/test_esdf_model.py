"""The ESDF truth of tests/esdf_independent.py validated where it can be, on the CPU: the brute force against scipy's exact Euclidean distance
transform, the pattern catalogue against its own design, the block writer against the checker's marking pass -- and the CPU checker's exact
2-D and 3-D updates against the brute force on every drawn pattern at every radius of the GPU sweep (tests/test_gpu_esdf_drawn.py), parents
included.  No GPU."""
import numpy as np
import pytest

import esdf_cases as EC
import esdf_independent as EI


def _M():
    from isaac_ros_nvblox_amd import mapper as M
    return M


def test_radius_table_of_the_sweep():
    """What the float32 quotient makes of the nominal radii: every rb from 1 to 8 and both 64-bit word edges (rb 7, rb 8) are in the sweep; 57 at
    0.05 m lands BELOW 57 (ri 56, rb 7), which is why "57up" is there; the last accepted radius has ri 63 and a max_sq below 4096."""
    got = {}
    for r in EC.RADII_2D:
        q, max_sq, ri = EI.radius_of(EC.distance_m(r), EC.VOXEL)
        got[r] = (ri, EI.radius_blocks(q))
        assert q < 64
    assert got[0.5] == (1, 1) and got[7] == (7, 1) and got[8] == (8, 1) and got[9] == (9, 2) and got[40] == (40, 5)
    assert got[48] == (48, 6) and got[49] == (49, 7) and got[56] == (56, 7) and got[57] == (56, 7) and got["57up"] == (57, 8)
    assert got[62.5] == (62, 8) and got[63] == (63, 8) and got["below64"] == (63, 8)
    q = EI.radius_of(EC.distance_m("below64"), EC.VOXEL)[0]
    assert q == np.nextafter(np.float32(64), np.float32(0)) and np.float32(q * q) < 4096 and np.float32(63 * 63 + 11 * 11) <= np.float32(q * q)
    assert EI.radius_of(EI.distance_at_least_radius(64, EC.VOXEL), EC.VOXEL)[0] >= 64
    quotients = {vs: [EI.radius_of(EC.distance_m(r, vs), vs)[0] for r in (2.5, 9, 63)] for vs in (0.05, 0.1, 0.02)}
    assert quotients[0.02][1] > 9 and quotients[0.05][1] == 9                      # (the repeats do differ)


@pytest.mark.parametrize("r", [0.5, 1, 2.5, 9, 40, 63.999996], ids=EC.radius_id)
def test_bruteforce_against_scipy(r):
    """edt_bruteforce == scipy.ndimage.distance_transform_edt cut off at max_sq, on every pattern of the catalogue (whole field: scipy knows no
    allocation); the count of minimisers against a direct count on a random field."""
    ndi = pytest.importorskip("scipy.ndimage")
    max_sq, ri = EI.cutoff(r)
    for case in EI.patterns_2d(r):
        where = np.ones(case.sites.shape, bool)
        sq, cnt = EI.edt_bruteforce(case.sites, where, r, budget=300_000)            # (a small budget: several chunks)
        d2 = np.rint(ndi.distance_transform_edt(~case.sites) ** 2)
        want = np.where(d2.astype(np.float32) <= max_sq, d2, max_sq).astype(np.float32)
        assert np.array_equal(sq, want), (case.name, np.argwhere(sq != want)[:5].tolist())
        assert np.array_equal(cnt > 0, d2.astype(np.float32) <= max_sq), case.name
    c3 = EI.patterns_3d(min(r, 9))[-1]
    sq3, _ = EI.edt_bruteforce(c3.sites, np.ones(c3.sites.shape, bool), min(r, 9))
    m3 = EI.cutoff(min(r, 9))[0]
    d3 = np.rint(ndi.distance_transform_edt(~c3.sites) ** 2)
    assert np.array_equal(sq3, np.where(d3.astype(np.float32) <= m3, d3, m3).astype(np.float32))


def test_minimiser_count_and_parent_check():
    """The count of minimisers on the tie patterns, and check_parents: it accepts every minimiser, and rejects a parent that is no site, one of
    the wrong length, one beyond ri, a missing one and a spurious one."""
    r = np.float32(9)
    cases = {c.name: c for c in EI.patterns_2d(r)}
    N = cases["tie_four"].sites.shape[0]; c = N // 2
    where = np.ones((N, N), bool)
    for name, n in (("tie_along_y", 2), ("tie_along_x", 2), ("tie_diagonal", 2), ("tie_four", 4), ("cutoff_inside", int(cases["cutoff_inside"].sites.sum())), ("cutoff_outside", 0), ("single_centre", 1)):
        sq, cnt = EI.edt_bruteforce(cases[name].sites, where, r)
        assert cnt[c, c] == n, (name, cnt[c, c])
    sites = cases["tie_four"].sites
    sq, cnt = EI.edt_bruteforce(sites, where, r)
    pts = np.argwhere(sites)
    q = np.argwhere(where)
    for pick in (0, -1):                     # the first and the last minimiser in scan order: two different tie rules, both valid
        parent = np.zeros((N, N, 2), np.int32)
        d = pts[None, :, :] - q[:, None, :]
        d2 = (d * d).sum(-1).astype(np.float32)
        ok = (d2 == sq[where][:, None]) & (sq[where][:, None] < EI.cutoff(r)[0])
        j = np.where(ok.any(1), (ok.argmax(1) if pick == 0 else ok.shape[1] - 1 - ok[:, ::-1].argmax(1)), 0)
        parent[tuple(q.T)] = np.where(ok.any(1)[:, None], d[np.arange(len(q)), j], 0)
        assert EI.check_parents(sites, sq, parent, where, r) > 100
    good = parent
    for what, edit in (("no site", lambda p: p.__setitem__((c, c), (1, 1))), ("missing", lambda p: p.__setitem__((c, c), (0, 0))),
                       ("spurious", lambda p: p.__setitem__((0, 0), (1, 0)))):
        bad = good.copy(); edit(bad)
        with pytest.raises(AssertionError):
            EI.check_parents(sites, sq, bad, where, r)
    # a parent to a real site that lies beyond ri on one axis while the stored distance says otherwise
    lone = np.zeros((N, N), bool); lone[c, c + 10] = True
    sq1 = np.full((N, N), EI.cutoff(r)[0], np.float32); sq1[c, c + 10] = 0; sq1[c, c] = 100
    par = np.zeros((N, N, 2), np.int32); par[c, c] = (0, 10)
    with pytest.raises(AssertionError):
        EI.check_parents(lone, sq1, par, where, r)


@pytest.mark.parametrize("r", EC.RADII_2D, ids=EC.radius_id)
def test_patterns_meet_their_design(r):
    """Every probe of every pattern has the squared distance the pattern was drawn to give it (sites at exactly ri count, at ri + 1 do not; the
    lattice offset just inside the cut-off counts, the one just outside does not), in 2-D and, at the 3-D radii, in 3-D."""
    q = EI.radius_of(EC.distance_m(r), EC.VOXEL)[0]
    max_sq, ri = EI.cutoff(q)
    sets = [EI.patterns_2d(q)] + ([EI.patterns_3d(q), [EI.one_block_3d(q)]] if r in EC.RADII_3D + [63] else [])
    for cases in sets:
        assert len({c.name for c in cases}) == len(cases)
        for case in cases:
            where = EI.alloc_voxels(case.alloc)
            sq, _ = EI.edt_bruteforce(case.sites, where, q)
            for pos, want in case.probes:
                assert where[pos] and sq[pos] == (max_sq if want is None else np.float32(want)), (case.name, pos, sq[pos], want)
            assert case.sites.any() and (not case.name.startswith("random") or case.sites.mean() <= 0.01), case.name
    (ins, s_in), (outs, s_out) = EI.cutoff_offsets(q)
    assert np.float32(s_in) <= max_sq < np.float32(s_out) and max(ins) <= ri


def _oracle_case_2d(oracle_mod, M, case, r, voxel_size, **kw):
    pg, q = EC.params(M, r, voxel_size, **kw)
    idx, data = EI.tsdf_blocks_2d(case.sites, case.alloc, pg)
    o = EC.oracle_map(oracle_mod, pg, idx, data)
    o.update_esdf()
    ei, eb = EC.oracle_esdf(oracle_mod, o)
    f, _ = EI.slice_fields(ei, eb, pg, (0, 0), case.alloc.shape)
    return pg, q, f, o


@pytest.mark.parametrize("r,voxel_size", [(r, EC.VOXEL) for r in EC.RADII_2D] + EC.REPEATS_2D, ids=lambda v: str(v))
def test_oracle_exact_2d_equals_the_brute_force(oracle_mod, r, voxel_size):
    """The checker's exact 2-D update on every drawn pattern: marking gives exactly the drawn sites (the block writer and the checker's marking
    pass agree), every allocated voxel equals the brute force, the parents are valid."""
    M = _M()
    q = EI.radius_of(EC.distance_m(r, voxel_size), voxel_size)[0]
    for case in EI.patterns_2d(q):
        pg, q, f, _ = _oracle_case_2d(oracle_mod, M, case, r, voxel_size)
        EC.assert_field((r, voxel_size, case.name), f, case.sites, EI.alloc_voxels(case.alloc), q, 2)


@pytest.mark.parametrize("r", EC.RADII_PROPAGATION, ids=EC.radius_id)
def test_oracle_propagation_equals_the_numpy_restatement(oracle_mod, r):
    """esdf_propagation = 1 in the checker == numpy_propagation on every drawn pattern, bit for bit, with valid parents; against the brute force
    as EC.assert_propagation_against_exact states it."""
    M = _M()
    q = EI.radius_of(EC.distance_m(r), EC.VOXEL)[0]
    for case in EI.patterns_2d(q):
        pg, q, f, _ = _oracle_case_2d(oracle_mod, M, case, r, EC.VOXEL, esdf_propagation=1)
        where = EI.alloc_voxels(case.alloc)
        ref = EI.numpy_propagation(case.sites, where, EI.cutoff(q)[0])
        assert np.array_equal(f.sq[where], ref[where]), (r, case.name)
        EI.check_parents(case.sites, f.sq, f.parent, where, q)
        exact, _ = EI.edt_bruteforce(case.sites, where, q)
        EC.assert_propagation_against_exact((r, case.name), case, f.sq, exact, q)


def _oracle_case_3d(oracle_mod, M, case, r):
    pg, q = EC.params(M, r, EC.VOXEL, esdf_mode=1)
    idx, data = EI.tsdf_blocks_3d(case.sites, case.alloc, pg)
    o = EC.oracle_map(oracle_mod, pg, idx, data)
    o.update_esdf()
    ei, eb = EC.oracle_esdf(oracle_mod, o)
    f, _ = EI.volume_fields(ei, eb, (0, 0, 0), case.alloc.shape)
    return pg, q, f, o


@pytest.mark.parametrize("r", EC.RADII_3D + [63], ids=EC.radius_id)
def test_oracle_exact_3d_equals_the_brute_force(oracle_mod, r):
    M = _M()
    q = EI.radius_of(EC.distance_m(r), EC.VOXEL)[0]
    for case in ([EI.one_block_3d(q)] if r == 63 else EI.patterns_3d(q)):
        pg, q, f, _ = _oracle_case_3d(oracle_mod, M, case, r)
        EC.assert_field((r, case.name), f, case.sites, EI.alloc_voxels(case.alloc), q, 3)
