"""Decay and clearing of the product on DRAWN maps (tests/maintenance_independent.py: the model; tests/maintenance_cases.py: the maps, the two sides,
the look-ups; tests/test_maintenance_model.py validates both against the CPU checker where there is no GPU).

Every call is judged by the model applied to the map AS READ BACK BEFORE it: the block set of every layer (duplicate-free), every voxel bit for bit
(a NaN as "is NaN"), the cleared list and an empty second take of it.  After every call the look-ups: the block count, get_blocks not finding what
is gone or was never there, point queries through the rebuilt table.  Then what only the product has: a pool of exactly 256 slots filled, decayed
and refilled through more than one turn of the three rotating hash tables, growth across decays, clear() and empty maps, the spared camera view
and its stamps across slot recycling and a LiDAR scan, the 64-blocks-per-wavefront form of k_decay in a child process, the cleared list through
the C ABI -- and the ESDF after a deallocation, held to the marking rule on the map's own TSDF and to the brute-force distances."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import esdf_cases as EC
import helpers as H
import maintenance_cases as MC
import maintenance_independent as MM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120


def _M():
    from isaac_ros_nvblox_amd import mapper as M
    return M


def _capacity(n_blocks):
    cap = 1 << 10
    while cap < n_blocks + n_blocks // 4 + 64:
        cap *= 2
    return cap


# ------------------------------------------------------------------------------------------------ cases A to D
@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_drawn_case_against_the_model(hip_lib, name):
    M = _M()
    case = MC.case_by_name(name)
    case.verify(MC.model_trace(case, MC.params(M, case)))
    side = MC.ProductSide(M, MC.params(M, case))
    look = MC.lookup_hook(side)
    seen = {"esdf": 0, "esdf_gone": 0}

    def hook(state, before, cleared, read):
        seen["esdf"] = max(seen["esdf"], len(MM.layer_keys(before, "esdf")))
        seen["esdf_gone"] += len(set(MM.layer_keys(before, "esdf")) - set(MM.layer_keys(state, "esdf")))
        look(state, before, cleared, read)
    MC.run_case(case, side, after_hook=hook)
    if name[0] in "ABC":
        assert seen["esdf"] >= 20, "the update before the calls made ESDF blocks"
    if name[0] == "C":
        assert seen["esdf_gone"] >= 20, "there are ESDF blocks outside the radius"
    if name == "C-everything":
        assert side.m.counters()["blocks_allocated"] == 0
    side.close()


def test_no_shape_dirties_nothing(hip_lib):
    """clearTsdfInsideShapes with an empty list after both updates have run: the map is unchanged (case D-none above) and nothing becomes dirty --
    the next ESDF update marks no column and the next mesh update meshes no block."""
    M = _M()
    case = MC.case_by_name("D-none")
    side = MC.ProductSide(M, MC.params(M, case))
    side.draw(case.state)
    g = side.m
    g.update_esdf(); g.update_color_mesh()
    assert g.counters()["esdf_columns_marked"] > 0 and g.counters()["mesh_blocks_updated"] > 0
    g.update_esdf(); g.update_color_mesh()
    quiet = g.counters()
    assert quiet["esdf_columns_marked"] == 0 and quiet["mesh_blocks_updated"] == 0, quiet
    MC.checked_step(("no shape",), side, ("clear_shapes", []))
    g.update_esdf(); g.update_color_mesh()
    after = g.counters()
    assert after["esdf_columns_marked"] == 0 and after["mesh_blocks_updated"] == 0, after
    side.close()


# ------------------------------------------------------------------------------------------------ pool and hash conservation
def test_pool_and_hash_conservation(hip_lib):
    """MC.conservation_rounds (five rounds of decay and refill in a pool of exactly 256 slots), then: everything goes under a far, tiny radius --
    no block left -- and the pool refills to exactly 256 without an overflow (a leaked slot would overflow, a slot freed twice would show as two
    blocks sharing voxels); then the maximum capacity is raised, 400 more blocks make the pools grow, and three decays follow with the look-ups
    after each (the rotating tables are re-allocated at the new size)."""
    M = _M()
    side, state, rng, used = MC.conservation_rounds(M)
    g = side.m
    state = MC.checked_step(("everything goes",), side, ("clear_outside_radius", (100.0, 100.0, 100.0), 0.01), after_hook=MC.lookup_hook(side))
    assert not state and g.counters()["blocks_allocated"] == 0
    blocks = {}
    for n, kind, z in ((100, "tc", 20), (100, "t", 21), (56, "c", 22)):
        blocks.update(MC.drawn_blocks(rng, MC._fresh_keys(n, used, z), kind, MC.LIVE_W))
    state = MC.draw_more(("refill after everything went",), side, {}, blocks)
    assert len(state) == 256 and g.capacity == 256 and g.counters()["capacity_overflow"] == 0
    # growth across decays
    g.set_max_capacity(4096)
    more = {}
    keys = MC._fresh_keys(400, used, 30) + MC._fresh_keys(0, used, 31)
    for j, k in enumerate(keys):
        more.update(MC.drawn_blocks(rng, [k], "tc" if j % 2 else "t", (0.4, 0.9, 1.9, 100.0)[j % 4]))      # gone after the 1st / 2nd / 3rd decay / never
    state = MC.draw_more(("growth",), side, state, more)
    assert g.capacity > 256 and len(state) == 656
    for r in range(3):
        n = len(state)
        state = MC.checked_step(("decay after growth", r), side, ("decay_tsdf", False), after_hook=MC.lookup_hook(side))
        assert len(state) <= n - 90, (r, n, len(state))
    side.close()


def test_clear_and_decay_on_empty_maps(hip_lib):
    """clear(), a decay on the empty map, a drawing and a decay: bit-identical to a fresh mapper given the same drawing and one decay."""
    M = _M()
    pg = M.default_params(voxel_size=MC.VOXEL, **MC.CONSERVATION_PARAMS)
    rng = np.random.default_rng(29)
    first = MC.drawn_blocks(rng, MC._fresh_keys(120, set(), 0), "tc", MC.DOOMED_W)
    drawing = {}
    for j, k in enumerate(MC._fresh_keys(150, set(), 1)):
        drawing.update(MC.drawn_blocks(rng, [k], ("tc", "t", "c")[j % 3], MC.DOOMED_W if j % 2 else MC.LIVE_W))
    a = MC.ProductSide(M, pg, capacity=256); b = MC.ProductSide(M, pg, capacity=256)
    a.m.decay_tsdf(False)                                                     # on a map that never held a block
    a.draw(first); a.m.update_esdf(); a.m.decay_tsdf(False)
    a.m.clear()
    assert a.m.counters()["blocks_allocated"] == 0
    MC.checked_step(("decay on the cleared map",), a, ("decay_tsdf", False), after_hook=MC.lookup_hook(a))
    a.draw(drawing); b.draw(drawing)
    cleared = []
    look = MC.lookup_hook(a)

    def hook(state, before, gone, read):
        cleared.append(gone); look(state, before, gone, read)
    state = MC.checked_step(("decay after clear()",), a, ("decay_tsdf", False), after_hook=hook)
    b.m.decay_tsdf(False)
    assert 50 <= len(MM.layer_keys(state, "tsdf")) < 100
    H.assert_same_map(a.m, b.m, "cleared and redrawn against fresh", layers=(M.LAYER_TSDF, M.LAYER_COLOR), min_blocks=50)
    assert len(cleared[0]) >= 40 and np.array_equal(b.take_cleared(), cleared[0])
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ the spared view
WALL_CAM = H.SMALL_CAM
WALL_T = np.eye(4, dtype=np.float32)
SPARED_PARAMS = dict(tsdf_decay_factor=0.5, tsdf_decayed_weight_threshold=4.0)      # one frame leaves weights far below 8: whatever is not spared and not drawn heavy goes
LIDAR = (256, 16, 0.1, -np.deg2rad(15.0), np.deg2rad(15.0))
LIDAR_T = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float32)      # the scan's azimuth sweeps the x-z plane: through the camera's frustum


def _wall_map(rng):
    """blocks around the camera's axis, in front of and behind a wall 1 m away: light ones (gone with the first decay unless spared) and heavy ones"""
    keys = MC._keys(range(-3, 3), range(-3, 3), range(0, 5))
    out = {}
    for j, k in enumerate(keys):
        out.update(MC.drawn_blocks(rng, [k], "tc" if j % 3 == 0 else "t", 1.0 if j % 2 else 100.0))
    return out


def _keyset(a):
    return {tuple(int(v) for v in k) for k in np.asarray(a).reshape(-1, 3)}


def test_spared_view_and_recycled_slots(oracle_mod, hip_lib):
    """A depth frame of a near wall over part of a drawn map: last_view() is the checker's and is the spared set -- after decay_tsdf(True) its blocks
    are bit-identical, the rest follow the model.  Then radius clearing frees some of the viewed blocks, set_blocks draws as many blocks at new
    indices (they take the recycled slots) and decay_tsdf(True) must decay those: a freed slot's camera stamp is reset."""
    M = _M()
    pg = M.default_params(voxel_size=MC.VOXEL, **SPARED_PARAMS)
    rng = np.random.default_rng(31)
    drawn = _wall_map(rng)
    side = MC.ProductSide(M, pg, capacity=1024); chk = MC.CheckerSide(oracle_mod, pg)
    side.draw(drawn); chk.draw(drawn)
    depth = np.full((WALL_CAM[5], WALL_CAM[4]), 1.0, np.float32)
    side.m.integrate_depth(depth, WALL_T, WALL_CAM); chk.m.integrate_depth(depth, WALL_T, WALL_CAM)
    view = side.m.last_view()
    assert _keyset(view) == _keyset(chk.m.last_view()) and len(_keyset(view)) == len(view)
    before = MC.state_from_read(side.read())
    spared = _keyset(view)
    f, thr = np.float32(0.5), np.float32(4.0)
    doomed_if_not_spared = [k for k in spared if not (~((before[k]["tsdf"]["weight"] * f) < thr)).any()]
    assert len(spared & set(drawn)) >= 20 and len(doomed_if_not_spared) >= 20, (len(spared), len(doomed_if_not_spared))
    state = MC.checked_step(("decay, view spared",), side, ("decay_tsdf", True), spared=view, after_hook=MC.lookup_hook(side))
    chk.run(("decay_tsdf", True))
    assert set(MM.layer_keys(state, "tsdf")) == _keyset(chk.m.block_indices(oracle_mod.L_TSDF))
    assert spared <= set(state) and 20 <= len(set(before) - set(state)) and len(set(state) - spared) >= 20, "spared blocks stay, light ones go, heavy ones stay"
    for k in spared:
        assert state[k]["tsdf"].tobytes() == before[k]["tsdf"].tobytes(), (k, "a spared block changed")
    # radius clearing frees viewed blocks; new blocks take their slots
    c, r = (0.0, 0.0, 0.2), 0.75
    before = state
    state = MC.checked_step(("radius clearing",), side, ("clear_outside_radius", c, r), after_hook=MC.lookup_hook(side))
    freed_viewed = [k for k in spared if k not in state]
    assert len(freed_viewed) >= 10 and len(spared & set(state)) >= 5, (len(freed_viewed), len(spared & set(state)))
    new_keys = MC._fresh_keys(len(before) - len(state), set(), 7)
    state = MC.draw_more(("new blocks in recycled slots",), side, state, MC.drawn_blocks(rng, new_keys, "t", 1.0))
    assert side.m.counters()["blocks_allocated"] == len(before)
    state = MC.checked_step(("decay after recycling",), side, ("decay_tsdf", True), spared=view, after_hook=MC.lookup_hook(side))
    assert not set(new_keys) & set(state), "a block in a recycled slot was spared: the freed slot kept its camera stamp"
    assert spared & set(state), "the blocks of the view that stayed are still spared"
    side.close()


def test_camera_view_is_spared_after_a_lidar_scan(oracle_mod, hip_lib):
    """A LiDAR scan over the same blocks follows the camera frame: decay_tsdf(True) still spares the CAMERA's view (k_decay reads the slot's camera
    stamp, not the entry's view stamp, which the scan has re-claimed).  References: the checker's block set, and the model with the camera's view as
    the spared set."""
    M = _M()
    pg = M.default_params(voxel_size=MC.VOXEL, lidar_max_integration_distance_m=5.0, **SPARED_PARAMS)
    rng = np.random.default_rng(31)
    drawn = _wall_map(rng)
    side = MC.ProductSide(M, pg, capacity=2048); chk = MC.CheckerSide(oracle_mod, pg)
    side.draw(drawn); chk.draw(drawn)
    depth = np.full((WALL_CAM[5], WALL_CAM[4]), 1.0, np.float32)
    side.m.integrate_depth(depth, WALL_T, WALL_CAM); chk.m.integrate_depth(depth, WALL_T, WALL_CAM)
    view = side.m.last_view()
    scan = np.full((LIDAR[1], LIDAR[0]), 1.2, np.float32)
    side.m.integrate_lidar_depth(scan, LIDAR_T, LIDAR); chk.m.integrate_lidar_depth(scan, LIDAR_T, LIDAR)
    lidar_view = _keyset(side.m.last_view())
    spared = _keyset(view)
    assert len(spared & lidar_view) >= 10, "the scan re-claims blocks of the camera's view"
    before = MC.state_from_read(side.read())
    state = MC.checked_step(("decay after the scan",), side, ("decay_tsdf", True), spared=view, after_hook=MC.lookup_hook(side))
    chk.run(("decay_tsdf", True))
    assert set(MM.layer_keys(state, "tsdf")) == _keyset(chk.m.block_indices(oracle_mod.L_TSDF))
    assert spared <= set(state) and len(lidar_view - spared - set(state)) >= 10, "the scan's own blocks are not spared"
    for k in spared:
        assert state[k]["tsdf"].tobytes() == before[k]["tsdf"].tobytes(), (k, "a spared block changed")
    side.close()


# ------------------------------------------------------------------------------------------------ many blocks per wavefront
def test_many_blocks_per_wavefront_in_a_child_process(hip_lib):
    """tests/maintenance_child.py with NVBX_DECAY_GRID=1, once: started the way tests/test_gpu_launch_geometry.py starts its child (knob variables
    stripped from the inherited environment, a time limit, a marker on stdout); not started again if it fails or times out."""
    import maintenance_child
    import test_gpu_launch_geometry as LG
    env = {k: v for k, v in os.environ.items() if k not in LG.KNOBS}
    env["NVBX_DECAY_GRID"] = "1"
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maintenance_child.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("the child timed out after %d s:\n%s" % (CHILD_TIMEOUT_S, err[-3000:]))
    print("child: %.1f s" % (time.time() - t0))
    if p.returncode != 0 or maintenance_child.OK_MARKER not in p.stdout:
        why = ("signal %d" % -p.returncode) if p.returncode < 0 else ("exit status %d" % p.returncode)
        pytest.fail("the child failed (%s):\n%s\n%s" % (why, p.stdout[-2000:], p.stderr[-4000:]))


# ------------------------------------------------------------------------------------------------ the cleared list through the C ABI
def test_cleared_list_c_abi_with_a_short_buffer(hip_lib):
    """nvbx_take_cleared_blocks with a buffer smaller than the list returns the count it needs and consumes nothing; with room it returns the whole
    list; the call after that returns 0."""
    M = _M()
    case = MC.case_by_name("B-default")
    side = MC.ProductSide(M, MC.params(M, case))
    side.draw(case.state)
    before = MC.state_from_read(side.read())
    side.m.decay_occupancy()
    _, want = MM.decay_occupancy(before, side.p)
    n = len(want)
    assert n >= 10
    handle = side.m._h
    small = np.full((n - 1, 3), 77, np.int32); full = np.zeros((n, 3), np.int32)
    take = lambda a: hip_lib.nvbx_take_cleared_blocks(handle, a.ctypes.data_as(C.c_void_p), a.shape[0])          # noqa: E731
    assert take(small) == n and (small == 77).all(), "too small: the needed count, nothing written"
    assert take(np.zeros((0, 3), np.int32)) == n
    assert take(full) == n and np.array_equal(full, want)
    assert take(full) == 0
    side.close()


# ------------------------------------------------------------------------------------------------ the ESDF after a deallocation
@pytest.mark.parametrize("dims,r,op", [(2, r, op) for r in (2.5, 9) for op in MC.ESDF_OPS_2D] + [(2, 57, "radius_drops_esdf")] +
                         [(3, r, op) for r in (2.5, 8) for op in MC.ESDF_OPS_3D], ids=str)
def test_esdf_after_deallocation(oracle_mod, hip_lib, dims, r, op):
    """One maintenance call between two ESDF updates (MC.esdf_scene): (i) the marks of every ESDF block that exists equal the marking rule on the
    mapper's own TSDF read-back, (ii) distances and parents are the brute force's for that site set over those blocks, (iii) the layer equals the
    checker's.  "radius_drops_upper_tsdf" is the scene radius clearing used to get wrong: it dropped the upper-row TSDF block that held a column's
    only sites and left the column's surviving ESDF block unmarked for a re-mark, so the slice kept sites at distance 0 that no TSDF voxel backed."""
    M = _M()
    scene = MC.esdf_scene(M, op, r, dims)
    side = MC.ProductSide(M, scene.params, capacity=_capacity(len(scene.state)))
    gi, gb = MC.run_esdf_scene(scene, side)
    chk = MC.CheckerSide(oracle_mod, scene.params)
    oi, ob = MC.run_esdf_scene(scene, chk)
    EC.assert_same_blocks(scene.tag, gi, gb, oi, ob)
    side.close()


def test_esdf_radius_clearing_of_the_upper_row_with_neighbours_left(oracle_mod, hip_lib):
    """the same scene with a radius that leaves 3 x 3 columns of the lower row: the re-marked column's neighbours lose their parents too"""
    M = _M()
    scene = MC.esdf_scene(M, "radius_drops_upper_tsdf", 9, 2, clear_radius_m=0.9)
    side = MC.ProductSide(M, scene.params, capacity=1024)
    gi, gb = MC.run_esdf_scene(scene, side)
    assert len(gi) == 9
    oi, ob = MC.run_esdf_scene(scene, MC.CheckerSide(oracle_mod, scene.params))
    EC.assert_same_blocks(scene.tag, gi, gb, oi, ob)
    side.close()


# ------------------------------------------------------------------------------------------------ the mesh after a decay
def test_mesh_after_a_neighbour_decays_away(oracle_mod, hip_lib):
    """The decay twin of test_gpu_mesh_drawn.py::test_freed_neighbour_slot: blocks A and N = A + x are meshed, N decays away; mesh() holds no geometry
    for N and A's mesh loses its cubes at lattice x = 7 and equals the model without N -- from the dirty list decay filled, and again with full=True.
    (A deallocated block's mesh record is dropped, not listed with zero vertices: the mesh kernel marks the record of a slot without a TSDF block
    invalid and nvbx_mesh_copy leaves it out, as after radius clearing.  What tells a viewer to delete N is the cleared list, asserted here too;
    a listing, where there is one, must be empty.)"""
    import mesh_cases as XC
    M = _M()
    A, N = (0, 0, 0), (1, 0, 0)
    field = XC.random_field(np.array([A, N], np.int32), seed=13, name="pair", without_color=None)
    field = field._replace(weight=[np.full((8, 8, 8), 100.0, np.float32), np.full((8, 8, 8), 1.5, np.float32)])
    pg = XC.params(field, tsdf_decay_factor=0.5, tsdf_decayed_weight_threshold=1.0)
    g = XC.into_mapper(pg, field); o = XC.into_oracle(oracle_mod, pg, field)
    g.update_color_mesh(); o.update_mesh(full=True)
    mesh = g.mesh()
    n_before = len(mesh[A]["vertices"])
    assert set(mesh) == {A, N} and n_before > 400 and XC.expected(XC.dense_of(g), A, pg)[3][7].any(), "A's cubes at x = 7 are meshed while N is there"
    g.decay_tsdf(False); o.decay_tsdf(False)
    assert _keyset(g.block_indices(M.LAYER_TSDF)) == {A} and _keyset(g.take_cleared_blocks()) == {N}
    for full in (False, True):
        g.update_color_mesh(full=full); o.update_mesh(full=True)
        mesh = g.mesh()
        dense = XC.dense_of(g)
        assert not XC.expected(dense, A, pg)[3][7].any()
        assert A in mesh and set(mesh) <= {A, N} and (N not in mesh or (len(mesh[N]["vertices"]) == 0 and len(mesh[N]["triangles"]) == 0)), "no geometry is left for N"
        assert o.mesh_block(np.asarray(N)) is None or len(o.mesh_block(np.asarray(N))["triangles"]) == 0
        XC.assert_block(("pair", "N decayed", full), mesh[A], XC.expected(dense, np.asarray(A), pg), pg, checker=o.mesh_block(np.asarray(A)))
        assert 0 < len(mesh[A]["vertices"]) < n_before and float(mesh[A]["vertices"][:, 0].max()) <= 7.5 * XC.VOXEL + 1e-6
    g.close()
