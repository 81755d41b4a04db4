"""The mesh of the product on DRAWN TSDF fields (tests/mesh_cases.py: the fields, the assertions; tests/mesh_independent.py: the table-free model;
tests/test_mesh_model.py validates both against the CPU checker where there is no GPU).

Every case: a fresh Mapper, set_blocks of the drawn TSDF and colour blocks, update_color_mesh() from the dirty list that set_blocks filled, the mesh
read back; the same on a second mapper with update_color_mesh(full=True).  Per block then
  1. triangles == the checker's, vertex count and order == the model's (evaluated on the mapper's OWN read-back layers),
  2. every coordinate within one float32 spacing of the model's (the count of coordinates that are not bit-identical is printed),
  3. colours == the model's, alpha 255,
  4. normals finite, unit or exactly 0, within 2e-4 of the float64 recomputation from the product's own vertices above the length cut-off,
  5. (sphere) vertices within SPHERE_D_TOL of the analytic sphere, triangles outward, the welded mesh closed,
  6. dirty-list mesh == full-layer mesh bit for bit, a repeated update gives the same read-back,
  7. counters: no overflow, blocks / vertices / triangles == the read-back's totals.
Then the scenarios only the product has: the pre-pass skip at a face plane, a freed neighbour slot, the arena's region limit, pool growth."""
import numpy as np
import pytest

import helpers as H
import mesh_cases as MC

pytestmark = pytest.mark.gpu
M = MC.M

# 2 x the checker's worst radial error on the sphere field: 1.1554e-3 m = 0.0231 voxels, measured by
# tests/test_mesh_model.py::test_sphere_field_analytic and held there within MC.SPHERE_CHECKER_WORST_M = 1.16e-3 m
SPHERE_D_TOL = 2 * MC.SPHERE_CHECKER_WORST_M

ARRAYS = ("vertices", "normals", "colors", "triangles")


def _keys(idx):
    return {tuple(i) for i in np.asarray(idx).reshape(-1, 3).tolist()}


def _assert_same_mesh(tag, a, b):
    """two read-backs of mesh(): the same blocks, all four arrays of every block equal in every bit"""
    assert a.keys() == b.keys(), (tag, sorted(set(a) ^ set(b))[:5])
    for k in a:
        for what in ARRAYS:
            diff = H.array_difference(np.asarray(a[k][what]), np.asarray(b[k][what]))
            assert diff is None, (tag, k, what, diff)


def _check_blocks(tag, g, mesh, o, pg, field_name, want_blocks):
    """every block of `mesh` against the model on g's own layers and against the checker o; -> (summed stats, per block)"""
    dense = MC.dense_of(g)
    assert _keys(dense[0]) == want_blocks and set(mesh) == want_blocks, (tag, "blocks listed", sorted(set(mesh) ^ want_blocks)[:5])
    total, per_block = MC.NO_STATS, {}
    for i in dense[0]:
        key = tuple(i.tolist())
        mo = o.mesh_block(i)
        assert mo is not None, (tag, key)
        s = MC.assert_block(tag + (key,), mesh[key], MC.expected(dense, i, pg), pg, checker=mo, compare_normals=field_name not in MC.NORMALS_NOT_COMPARED)
        per_block[key] = s; total = MC.add_stats(total, s)
    return total, per_block


def _assert_counters(tag, g, mesh):
    c = g.counters()
    assert c["capacity_overflow"] == 0, (tag, c)
    got = (c["mesh_blocks_updated"], c["mesh_vertices"], c["mesh_triangles"])
    want = (len(mesh), sum(len(b["vertices"]) for b in mesh.values()), sum(len(b["triangles"]) for b in mesh.values()))
    assert got == want, (tag, "counters against the read-back", got, want)


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_drawn_field(oracle_mod, hip_lib, case):
    """One drawn field under one (ambiguity rule, normal rule): assertions 1 .. 7 of the module docstring, from the dirty list and from the full
    layer.  The random field runs under all six rule pairs, every other field under the defaults and (1, 1), the zeros field also under (0, 1)."""
    name, a, n = case
    field = MC.FIELDS[name]()
    pg = MC.params(field, a, n)
    o = MC.into_oracle(oracle_mod, pg, field)
    o.update_mesh(full=True)
    blocks = _keys(field.idx)
    states, meshes = {}, {}
    for mode in ("dirty", "full"):
        tag = (name, a, n, mode)
        g = MC.into_mapper(pg, field)
        g.update_color_mesh(full=mode == "full")
        mesh = g.mesh()
        total, _ = _check_blocks(tag, g, mesh, o, pg, name, blocks)
        print("%s a%d n%d %s: %d vertices, %d triangles, %d of %d coordinates not bit-identical to the model, %d zero normals, %d of %d normals below "
              "the cut-off (the checker: %d)" % (name, a, n, mode, total.vertices, total.triangles, total.not_bit_identical, 3 * total.vertices,
                                                 total.zero_normals, total.normals_excluded, total.vertices, total.checker_excluded))
        MC.assert_normal_shares(tag, name, a, n, total, against_checker=name not in MC.NORMALS_NOT_COMPARED)
        _assert_counters(tag, g, mesh)
        if name == "sphere":
            worst = MC.sphere_checks(tag, mesh)
            print("sphere a%d n%d %s: worst radial error %.4e m" % (a, n, mode, worst))
            assert worst <= SPHERE_D_TOL, (tag, worst)
        states[mode] = H.map_state(g, layers=(M.LAYER_TSDF, M.LAYER_COLOR), mesh=True)
        meshes[mode] = mesh
        # the identical update once more (the dirty list filled by the same blocks again; the full layer as it is)
        if mode == "dirty":
            MC.set_blocks(g, field)
        g.update_color_mesh(full=mode == "full")
        H.assert_same_map(states[mode], g, tag + ("a repeated update",))
        _assert_same_mesh(tag + ("a repeated update",), mesh, g.mesh())
        _assert_counters(tag + ("a repeated update",), g, mesh)
        g.close()
    H.assert_same_map(states["dirty"], states["full"], (name, a, n, "dirty list against full layer"), min_blocks={M.LAYER_TSDF: len(blocks)})
    _assert_same_mesh((name, a, n, "dirty list against full layer"), meshes["dirty"], meshes["full"])


def test_face_plane_full_mode(oracle_mod, hip_lib):
    """Block A entirely positive, block B = A + x entirely negative: A has no negative voxel of its own, and the full-layer pre-pass must still
    send it to the meshing path (the negative voxels are its neighbour's).  Then B's weights drop below mesh_min_weight: neither block has an
    observed negative voxel in reach, both are skipped and listed empty."""
    field = MC.face_field()
    pg = MC.params(field)
    g = MC.into_mapper(pg, field)
    o = MC.into_oracle(oracle_mod, pg, field)
    g.update_color_mesh(full=True); o.update_mesh(full=True)
    mesh = g.mesh()
    _check_blocks(("face", "full"), g, mesh, o, pg, "face", {MC.FACE_A, MC.FACE_B})
    A, B = mesh[MC.FACE_A], mesh[MC.FACE_B]
    assert (len(A["vertices"]), len(A["triangles"])) == (64, 98) and len(B["vertices"]) == 0 and len(B["triangles"]) == 0
    x = A["vertices"][:, 0]
    assert (x == x[0]).all() and abs(float(x[0]) - 8 * MC.VOXEL) <= 1e-7          # voxel centre 7.5 + t = 0.5: the face itself
    _assert_counters("face", g, mesh)
    low = MC.Field("face_low", field.idx[1:], field.dist[1:], [np.full((8, 8, 8), np.nextafter(MC.MIN_W, np.float32(0)), np.float32)], [None], {})
    g.set_blocks(M.LAYER_TSDF, low.idx, MC.tsdf_blocks(low)); MC.into_oracle(oracle_mod, pg, low, o)
    g.update_color_mesh(full=True); o.update_mesh(full=True)
    mesh = g.mesh()
    _check_blocks(("face", "B below the weight threshold"), g, mesh, o, pg, "face", {MC.FACE_A, MC.FACE_B})
    assert all(len(mesh[k]["vertices"]) == 0 and len(mesh[k]["triangles"]) == 0 for k in (MC.FACE_A, MC.FACE_B))
    _assert_counters("face, B below the weight threshold", g, mesh)
    g.close()


@pytest.mark.parametrize("min_weight", [0.1, 0.0], ids=["any_slot", "find_slot"])
def test_freed_neighbour_slot(oracle_mod, hip_lib, min_weight):
    """The neighbour lookup of the mesh loads no layer flag when mesh_min_weight > 0: a slot without a TSDF block must read as weight 0, a slot
    that radius clearing freed and a colour-only block took again included.  Blocks A and N = A + x are meshed, N is cleared away, colour-only
    blocks -- one of them at N's own index, the others far off -- take free slots, and the full-layer mesh of A must be the model's without N:
    no cube at lattice x = 7.  With mesh_min_weight = 0 the other lookup (find_slot with the TSDF flag) runs."""
    A, N = (0, 0, 0), (1, 0, 0)
    field = MC.random_field(np.array([A, N], np.int32), seed=13, name="pair", without_color=None)
    pg = MC.params(field, mesh_min_weight=min_weight)
    g = MC.into_mapper(pg, field)
    o = MC.into_oracle(oracle_mod, pg, field)
    g.update_color_mesh(); o.update_mesh(full=True)
    total, per_block = _check_blocks(("pair", min_weight), g, g.mesh(), o, pg, "pair", {A, N})
    assert per_block[A].vertices > 400 and MC.expected(MC.dense_of(g), A, pg)[3][7].any(), "A's cubes at x = 7 are meshed while N is there"
    centre = tuple((np.array(A) + 0.5) * 8 * MC.VOXEL)
    g.clear_outside_radius(centre, 0.2); o.clear_outside_radius(centre, 0.2)
    assert _keys(g.block_indices(M.LAYER_TSDF)) == {A} and _keys(o.block_indices(oracle_mod.L_TSDF)) == {A}
    rng = np.random.default_rng(14)
    new_idx = np.array([N, (40, 41, 42), (41, 41, 42), (-40, 7, 9), (40, -41, 42)], np.int32)
    colour = MC.random_colors(rng, new_idx)
    g.set_blocks(M.LAYER_COLOR, new_idx, np.stack([c.reshape(512) for c in colour]))
    for i, c in zip(new_idx.tolist(), colour):
        o.set_block(oracle_mod.L_COLOR, i, c.reshape(512))
    g.update_color_mesh(full=True); o.update_mesh(full=True)
    mesh = g.mesh()
    dense = MC.dense_of(g)
    after, _ = _check_blocks(("pair", min_weight, "N freed"), g, mesh, o, pg, "pair", {A})
    assert not MC.expected(dense, A, pg)[3][7].any()
    assert 0 < after.vertices < per_block[A].vertices and float(mesh[A]["vertices"][:, 0].max()) <= 7.5 * MC.VOXEL + 1e-6
    _assert_counters(("pair", min_weight, "N freed"), g, mesh)
    g.close()


def test_arena_region_overflow(oracle_mod, hip_lib):
    """The arena's region limit (SEMANTICS.md, Mesh): at block_capacity 256 a region holds 6144 vertices.  The eight checkerboard blocks (13005
    vertices) mesh completely from the dirty list, one block per workgroup and region; under full = True one workgroup meshes all eight into
    region 0, which overflows: capacity_overflow is set, every block is still listed, each block is either complete and exact or entirely empty,
    and mesh() returns.  The same field at capacity 1 << 12 under full = True is complete.  This pins what the kernel does today; measured: three
    blocks, (-1, -1, 0), (-1, 0, -1) and (0, -1, -1), come back complete and the other five empty (which ones follows the slot order)."""
    field = MC.checkerboard_field()
    pg = MC.params(field)
    blocks = _keys(field.idx)
    o = MC.into_oracle(oracle_mod, pg, field)
    o.update_mesh(full=True)
    g = MC.into_mapper(pg, field, block_capacity=256)
    assert g.capacity == 256
    g.update_color_mesh()
    mesh = g.mesh()
    total, _ = _check_blocks(("overflow", "dirty"), g, mesh, o, pg, "checkerboard", blocks)
    assert (total.vertices, total.triangles) == (13005, 13500)
    _assert_counters(("overflow", "dirty"), g, mesh)
    g.update_color_mesh(full=True)
    assert g.counters()["capacity_overflow"] == 1
    mesh = g.mesh()
    assert set(mesh) == blocks
    dense = MC.dense_of(g)
    exact, empty = [], []
    for i in dense[0]:
        key = tuple(i.tolist())
        if len(mesh[key]["vertices"]) == 0 and len(mesh[key]["triangles"]) == 0 and len(mesh[key]["normals"]) == 0 and len(mesh[key]["colors"]) == 0:
            empty.append(key)
        else:
            MC.assert_block(("overflow", "full", key), mesh[key], MC.expected(dense, i, pg), pg, checker=o.mesh_block(i))
            exact.append(key)
    print("arena overflow: complete %s, empty %s" % (exact, empty))
    assert exact and empty, (exact, empty)
    assert sum(len(mesh[k]["vertices"]) for k in exact) <= 6144
    assert g.capacity == 256
    g.close()
    g = MC.into_mapper(pg, field, block_capacity=1 << 12)             # 98304 vertices per region: the full layer fits
    g.update_color_mesh(full=True)
    mesh = g.mesh()
    total, _ = _check_blocks(("overflow", "full at 1 << 12"), g, mesh, o, pg, "checkerboard", blocks)
    assert (total.vertices, total.triangles) == (13005, 13500)
    _assert_counters(("overflow", "full at 1 << 12"), g, mesh)
    g.close()


def test_growth_after_a_drawn_mesh(oracle_mod, hip_lib):
    """The pools and the mesh arenas grow after a drawn mesh (400 far-away all-positive blocks into a mapper of 256): without a new update,
    mesh() returns what it returned before the growth, all four arrays of every block."""
    field = MC.random_field()
    pg = MC.params(field)
    g = MC.into_mapper(pg, field, block_capacity=256)
    g.update_color_mesh()
    before = g.mesh()
    assert g.capacity == 256 and sum(len(b["vertices"]) for b in before.values()) > 6000
    far = np.array([(100 + k % 20, 100 + k // 20, 100) for k in range(400)], np.int32)
    data = np.zeros((400, 512), M.TSDF_DT); data["distance"] = np.float32(0.1); data["weight"] = np.float32(1.0)
    g.set_blocks(M.LAYER_TSDF, far, data)
    assert g.capacity > 256 and g.num_blocks(M.LAYER_TSDF) == 408
    _assert_same_mesh("after the growth", before, g.mesh())
    assert g.counters()["capacity_overflow"] == 0
    g.close()
