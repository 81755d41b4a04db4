"""The drawn mesh fields (tests/mesh_cases.py) through the CPU checker against the table-free model (tests/mesh_independent.py), where there is no
GPU: the truth tests/test_gpu_mesh_drawn.py holds the product to cannot move silently with a change to the checker or to the model, and the
fields keep reaching what they were drawn to reach (all 254 cube cases, the per-block maxima, zero normals, the face plane)."""
import numpy as np
import pytest

import mesh_cases as MC
import mesh_independent as MI


def _mesh_and_check(oracle_mod, field, a, n, **kw):
    """the field through the checker, every block against the model bit for bit; -> (params, checker map, dense layers, meshes, stats, per block)"""
    pg = MC.params(field, a, n, **kw)
    o = MC.into_oracle(oracle_mod, pg, field)
    o.update_mesh(full=True)
    dense = MC.dense_of(o, oracle_mod)
    assert np.array_equal(dense[0], field.idx[np.lexsort(field.idx.T[::-1])])
    meshes, total, per_block = {}, MC.NO_STATS, {}
    for i in dense[0]:
        key = tuple(i.tolist())
        mb = o.mesh_block(i)
        assert mb is not None, (field.name, key, "a TSDF block the full update did not mesh")
        s = MC.assert_block((field.name, a, n, key), mb, MC.expected(dense, i, pg), pg, bit_exact=True, compare_normals=field.name not in MC.NORMALS_NOT_COMPARED)
        meshes[key] = mb; per_block[key] = s; total = MC.add_stats(total, s)
    MC.assert_normal_shares((field.name, a, n), field.name, a, n, total)
    return pg, o, dense, meshes, total, per_block


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_checker_equals_model_on_drawn_fields(oracle_mod, case):
    """Vertex count, order and position (every bit), colours, the topological triangle check and the normals of the checker on every drawn field,
    under the rules the GPU test runs it with; and what each field was drawn for."""
    name, a, n = case
    field = MC.FIELDS[name]()
    pg, o, dense, meshes, total, per_block = _mesh_and_check(oracle_mod, field, a, n)
    hist = MC.cube_case_histogram(dense, pg)
    n_cases = int((hist[1:255] > 0).sum())
    most_v = max(s.vertices for s in per_block.values()); most_t = max(s.triangles for s in per_block.values())
    print("%s a%d n%d: %d vertices, %d triangles (per block at most %d / %d), %d cube cases, %d zero normals, %d of %d normals below the cut-off"
          % (name, a, n, total.vertices, total.triangles, most_v, most_t, n_cases, total.zero_normals, total.normals_excluded, total.vertices))
    assert hist[0] == 0 and hist[255] == 0
    if name in ("random", "min_weight_zero", "zeros", "huge", "subnormal"):
        assert n_cases == 254, (name, "cube cases reached", n_cases)
    if name == "random":
        assert hist[1:255].min() >= 4 and most_v > 900 and most_t > 1400, (int(hist[1:255].min()), most_v, most_t)
    if name == "weights":
        assert n_cases >= 240 and 0 < total.vertices < 6000, (n_cases, total.vertices)
    if name == "checkerboard":
        # every lattice edge that can carry a vertex does: 3 * 9 * 9 * 8 in the block with all seven neighbours, 4 * 512 triangles
        assert (total.vertices, total.triangles, most_v, most_t, n_cases) == (13005, 13500, 1944, 2048, 2), (total, most_v, most_t, n_cases)
        assert per_block[(-1, -1, -1)].vertices == 1944 and per_block[(0, 0, 0)].vertices == 3 * 8 * 8 * 7
    if name in ("zeros", "huge"):
        assert total.zero_normals > (100 if n == 0 else 10), (name, total.zero_normals)      # (a sum of normals vanishes less often than one)
    if name == "face":
        A, B = meshes[MC.FACE_A], meshes[MC.FACE_B]
        assert (len(A["vertices"]), len(A["triangles"])) == (64, 98) and len(B["vertices"]) == 0 and len(B["triangles"]) == 0
        x = A["vertices"][:, 0]
        assert (x == x[0]).all() and abs(float(x[0]) - 8 * MC.VOXEL) <= 1e-7          # voxel centre 7.5 + t = 0.5: the face itself
    if name == "far":
        assert total.vertices > 1000 and most_v > 600
    if name == "min_weight_zero":
        # weight 0 passes a threshold of 0: the same mesh as with every weight 1
        ones = MC.Field(field.name, field.idx, field.dist, [np.ones_like(w) for w in field.weight], field.color, field.params)
        _, _, _, m1, t1, _ = _mesh_and_check(oracle_mod, ones, a, n)
        assert t1[:2] == total[:2] and all(np.array_equal(m1[k]["triangles"], meshes[k]["triangles"]) for k in meshes)


def test_sphere_field_analytic(oracle_mod):
    """The one field with an analytic truth: the checker's mesh of the sphere is closed, faces outward, and its vertices lie within the measured
    bound of the sphere -- the constant the GPU test doubles."""
    field = MC.sphere_field()
    for a, n in MC.RULES_OTHER:
        _, _, _, meshes, total, _ = _mesh_and_check(oracle_mod, field, a, n)
        worst = MC.sphere_checks(("sphere", a, n), meshes)
        print("sphere a%d n%d: %d vertices, %d triangles, worst radial error %.4e m = %.4f voxels" % (a, n, total.vertices, total.triangles, worst, worst / MC.VOXEL))
        assert worst <= MC.SPHERE_CHECKER_WORST_M, worst
        assert worst >= 0.8 * MC.SPHERE_CHECKER_WORST_M, ("the constant is not the measured value any more", worst)


def test_model_helpers_on_hand_made_input():
    """triangle_edge_cubes, expected_normals and cube_cases on inputs small enough to check by hand."""
    def eid(x, y, z, axis):
        return ((x * 9 + y) * 9 + z) * 3 + axis
    # cube (2, 3, 4), corner 0 negative: one triangle on the three edges leaving lattice point (2, 3, 4)
    eids = np.array(sorted([eid(2, 3, 4, 0), eid(2, 3, 4, 1), eid(2, 3, 4, 2)]))
    active = np.zeros((8, 8, 8), bool); active[2, 3, 4] = True
    ok, seen = MI.triangle_edge_cubes(eids, np.array([[0, 1, 2]]), active)
    assert ok.all() and np.array_equal(seen, active)
    # with only a cube active that the three edges do not share, the triangle has no home
    other = np.zeros((8, 8, 8), bool); other[1, 2, 3] = True
    ok, seen = MI.triangle_edge_cubes(eids, np.array([[0, 1, 2]]), other)
    assert not ok.any() and not seen.any()
    # a triangle in the face between cubes (2, 3, 4) and (1, 3, 4): three edges of the lattice square x = 2 -- either cube is a home
    face = np.array(sorted([eid(2, 3, 4, 1), eid(2, 3, 4, 2), eid(2, 4, 4, 2)]))
    both = np.zeros((8, 8, 8), bool); both[1, 3, 4] = True
    ok, seen = MI.triangle_edge_cubes(face, np.array([[0, 1, 2]]), both)
    assert ok.all() and np.array_equal(seen, both)
    # edges on the block's far faces (lattice 8) have fewer cubes around them, none outside 0 .. 7
    c, inside = MI.edge_cubes(np.array([eid(8, 8, 0, 2), eid(0, 0, 0, 0)]))
    assert inside.sum(1).tolist() == [1, 1] and c[0][inside[0]].tolist() == [[7, 7, 0]] and c[1][inside[1]].tolist() == [[0, 0, 0]]
    # normals: two triangles of a unit square in z = 0 and one standing on its edge
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 2]], np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 1]])
    n0, m0 = MI.expected_normals(v, t, 0, 1.0)
    assert np.array_equal(n0, [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 0]]) and m0.all()
    n1, m1 = MI.expected_normals(v, t, 1, 1.0)
    assert np.allclose(n1[0], np.array([0, 2, 2]) / np.sqrt(8)) and np.allclose(n1[1], np.array([0, 2, 1]) / np.sqrt(5)) and np.array_equal(n1[2], [0, 0, 1])
    nz, mz = MI.expected_normals(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), 0, 1.0)
    assert not nz.any() and not mz.any()
    # cube cases: one negative corner at lattice (1, 0, 0) is corner 1 of cube (0, 0, 0) and corner 0 of cube (1, 0, 0)
    neg = np.zeros((9, 9, 9), bool); neg[1, 0, 0] = True
    act = np.zeros((8, 8, 8), bool); act[0, 0, 0] = act[1, 0, 0] = True
    h = MI.cube_cases(neg, act)
    assert h[2] == 1 and h[1] == 1 and h.sum() == 2
