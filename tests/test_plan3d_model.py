"""The cost-volume model of tests/plan3d_independent.py held against three things that do not share its graph or its Dijkstra: a numpy
pull-relaxation (whole-volume sweeps of 26 shifted minima, sharing only the classification), the closed form on an empty volume, and the
properties every path must have.  The random cases of tests/test_gpu_plan3d.py meet their condition here, on the CPU.  The move table and the
step costs the kernels use (csrc/nvbx_plan3d_math.h, compiled with gcc as C) are the model's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plan3d_independent as P3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
F32 = np.float32
BIG = np.int64(P3.UNREACHED)


def _shift(a, d, fill):
    """b[p] = a[p + d] by padding and slicing (not the model's shift)"""
    pad = np.pad(a, 1, constant_values=fill)
    return pad[tuple(slice(1 + c, 1 + c + n) for c, n in zip(d, a.shape))]


def pull_relaxation(vol, sources, o):
    """-> (G int32, sweeps): G(p) = min(G(p), G(q) + c(p, q)) over the 26 neighbours, all voxels at once, until a sweep changes nothing.  The
    corner rule is written out per component here: every proper partial step of the move must land on a traversable voxel."""
    trav, pen = P3.classify(vol, o)
    G = np.full(trav.shape, BIG)
    for p in P3.accepted_sources(trav, sources):
        G[tuple(p)] = 0
    moves = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    ok, base = [], []
    for d in moves:
        m = trav & _shift(trav, d, False)
        for keep in range(1, 7):                                      # the partial steps: keep some components of d, drop others
            e = tuple(c if keep >> i & 1 else 0 for i, c in enumerate(d))
            if e != (0, 0, 0) and e != d:
                m = m & _shift(trav, e, False)
        ok.append(m); base.append({1: 10, 2: 14, 3: 17}[sum(map(abs, d))])
    for sweep in range(1, trav.size + 2):
        new = G.copy()
        for d, m, b in zip(moves, ok, base):
            gq = _shift(G, d, BIG)
            new = np.where(m & (gq != BIG), np.minimum(new, gq + b + pen + _shift(pen, d, 0)), new)
        if np.array_equal(new, G):
            return G.astype(np.int32), sweep
        G = new
    raise AssertionError("no fixed point")


@pytest.fixture(scope="module")
def cases():
    return P3.random_cases()


def test_moves_follow_the_rule():
    assert len(set(P3.MOVES)) == 26 and all(max(map(abs, d)) == 1 for d in P3.MOVES)
    ks = [sum(map(abs, d)) for d in P3.MOVES]
    assert ks == [1] * 6 + [2] * 12 + [3] * 8
    assert P3.MOVES[6:10] == ((1, 1, 0), (1, 0, 1), (1, 0, -1), (1, -1, 0)) and P3.MOVES[18] == (1, 1, 1) and P3.MOVES[25] == (-1, -1, -1)
    assert sorted(P3.between((1, -1, 0))) == [(0, -1, 0), (1, 0, 0)] and len(P3.between((1, 1, -1))) == 6 and P3.between((0, 0, 1)) == []


def test_random_cases_meet_their_condition(cases):
    o = P3.options(**P3.CASE_OPTIONS)
    assert len(cases) == len(P3.RANDOM_SHAPES) * P3.SEEDS_PER_SHAPE
    for shape, seed, vol, sources in cases:
        assert vol.shape == shape and vol.dtype == F32 and sources.shape == (3, 3) and vol.size <= 1 << 15
        assert all(s >= 2 * t for s, t in zip(shape, P3.TILE))
        blocked, unknown, acc, reached = P3.case_shares(vol, sources, o)
        assert 0.1 < blocked < 0.3 and 0.01 < unknown < 0.1 and acc == 3 and reached >= 0.5, (shape, seed, blocked, unknown, acc, reached)
        G, _ = P3.field(vol, sources, o)
        assert (G[sources[:, 0], sources[:, 1], sources[:, 2]] == 0).all()


def test_model_equals_the_pull_relaxation(cases):
    o = P3.options(**P3.CASE_OPTIONS)
    drawn = [(vol, src, o) for _, _, vol, src in cases[::2]] + [P3.line_case(s) + (o,) for s in P3.LINE_SHAPES]
    drawn += [(vol, src, o) for _, vol, src in P3.tile_cases()]
    vol, src = P3.serpentine(8)
    drawn.append((vol, src, P3.options()))
    vol, src, _ = P3.corner_cells()
    drawn.append((vol, src, P3.options()))
    vol, src = P3.special_values_volume()
    drawn += [(vol, src, P3.options(**kw)) for kw in P3.OPTION_SETS]
    for k, (vol, src, opt) in enumerate(drawn):
        G, _ = P3.field(vol, src, opt)
        R, sweeps = pull_relaxation(vol, src, opt)
        assert np.array_equal(G, R), (k, vol.shape, sweeps)


def test_closed_form_on_an_empty_volume():
    vol = np.full((11, 19, 23), F32(5.0))
    for s in ((0, 0, 0), (10, 18, 22), (5, 9, 11), (10, 0, 22)):
        G, acc = P3.field(vol, [s], P3.options())
        off = np.sort(np.stack(np.meshgrid(*[np.abs(np.arange(n) - c) for n, c in zip(vol.shape, s)], indexing="ij"), -1), -1)
        c, b, a = off[..., 0], off[..., 1], off[..., 2]             # a >= b >= c
        assert acc == 1 and np.array_equal(G, (17 * c + 14 * (b - c) + 10 * (a - b)).astype(np.int32))


def test_corner_cells_of_the_gpu_test():
    vol, sources, cells = P3.corner_cells()
    G, acc = P3.field(vol, sources, P3.options())
    assert acc == len(cells) == 76
    for low, far, shut, d in cells:
        k = sum(d)
        assert G[low] == 0
        assert (int(G[far]) == {2: 14, 3: 17}[k]) == (len(shut) == 0), (low, shut, int(G[far]))
        if k == 2:
            assert int(G[far]) == (14, 20, P3.UNREACHED)[len(shut)]
    assert int(G[cells[63][1]]) == P3.UNREACHED                     # all six shut: the far corner touches the source only at a corner
    t = P3.TILE
    assert any(low[i] == t[i] - 1 for low, _, _, _ in cells for i in range(3)) and all(any(low[i] == t[i] - 1 for low, _, _, _ in cells) for i in range(3))


def test_serpentine_of_the_gpu_test():
    vol, src = P3.serpentine(24)
    G, _ = P3.field(vol, src, P3.options())
    reached = G[G != P3.UNREACHED]
    # twelve free planes crossed corner to corner (23 face diagonals each), eleven openings passed through (two axis moves each), one step
    # into the opening of the last slab
    assert int(reached.max()) == 12 * 23 * 14 + 11 * 20 + 10 and len(reached) == 12 * 576 + 12
    far = np.unravel_index(np.argmax(np.where(G == P3.UNREACHED, -1, G)), G.shape)
    p = P3.path(vol, G, far, P3.options())
    assert len(p) == 12 * 23 + 22 + 1 + 1 and p[-1] == (0, 0, 0) and far == (23, 0, 0)


def _check_path(vol, G, start, o, p):
    trav, pen = P3.classify(vol, o)
    assert p[0] == tuple(start) and G[p[-1]] == 0 and all(G[q] != 0 for q in p[:-1])
    total = 0
    for a, b in zip(p[:-1], p[1:]):
        d = tuple(v - u for u, v in zip(a, b))
        assert max(map(abs, d)) == 1 and trav[a] and trav[b] and G[b] < G[a]                 # strictly descending
        for keep in range(1, 7):
            e = tuple(c if keep >> i & 1 else 0 for i, c in enumerate(d))
            if e != (0, 0, 0) and e != d:
                assert trav[tuple(u + v for u, v in zip(a, e))], "a corner was cut"
        total += {1: 10, 2: 14, 3: 17}[sum(map(abs, d))] + int(pen[a]) + int(pen[b])
    assert total == int(G[p[0]])


def test_every_model_path_is_a_cheapest_move_sequence(cases):
    o = P3.options(**P3.CASE_OPTIONS)
    rng = np.random.default_rng(5)
    for shape, seed, vol, sources in cases:
        G, _ = P3.field(vol, sources, o)
        reach = np.argwhere(G != P3.UNREACHED)
        for start in reach[rng.choice(len(reach), 16, replace=False)]:
            p = P3.path(vol, G, start, o)
            assert p, (shape, seed, start)
            _check_path(vol, G, tuple(int(v) for v in start), o, p)
        assert P3.path(vol, G, (-1, 0, 0), o) == [] and P3.path(vol, G, (0, shape[1], 0), o) == [] and P3.path(vol, G, (0, 0, shape[2]), o) == []
        assert P3.path(vol, G, np.argwhere(G == P3.UNREACHED)[0], o) == []
    # a field of another volume: some start finds no neighbour
    (_, _, vol_a, src_a), (_, _, vol_b, _) = cases[0], cases[1]
    Ga, _ = P3.field(vol_a, src_a, o)
    assert any(P3.path(vol_b, Ga, s, o) is None for s in np.argwhere(Ga != P3.UNREACHED))


# ---- the header the kernels take their moves from, compiled as C
def test_the_shared_header_has_the_models_moves_and_step_costs(tmp_path):
    src = tmp_path / "plan3d.c"; so = tmp_path / "plan3d.so"
    src.write_text('#include "nvbx_plan3d_math.h"\n'
                   "static const int MV[26][3] = NVBX_PLAN_MOVES_3D;\n"
                   "int n_moves(void) { return (int)(sizeof(MV) / sizeof(MV[0])); }\n"
                   "int move(int d, int c) { return MV[d][c]; }\n"
                   "int axis_end(void) { return NVBX_PLAN_MOVES_3D_AXIS; }\n"
                   "int face_end(void) { return NVBX_PLAN_MOVES_3D_FACE; }\n"
                   "int max_voxels(void) { return NVBX_PLAN3D_MAX_VOXELS; }\n"
                   "int base(int k) { return nvbx_plan3d_base(k); }\n"
                   "int step(int k, int a, int b) { return nvbx_plan3d_step(k, a, b); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so), "-lm"])
    lib = ctypes.CDLL(str(so))
    assert lib.n_moves() == 26 and lib.axis_end() == 6 and lib.face_end() == 18 and lib.max_voxels() == 1 << 22
    assert tuple(tuple(lib.move(d, c) for c in range(3)) for d in range(26)) == P3.MOVES
    assert [lib.base(k) for k in (1, 2, 3)] == [P3.BASE[k] for k in (1, 2, 3)] == [10, 14, 17]
    assert (lib.step(1, 3, 4), lib.step(2, 0, 0), lib.step(3, 200, 200)) == (17, 14, 417)
    assert 417 * (1 << 22) < 2 ** 31 - 1
