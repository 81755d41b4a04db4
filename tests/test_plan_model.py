"""The cost-field model of tests/plan_independent.py held against three things that do not share its graph or its Dijkstra: a numpy pull-relaxation
(whole-image sweeps of eight shifted minima, sharing only the classification), the octile closed form on an empty image, and the properties every
path must have.  The random cases of tests/test_gpu_plan.py meet their condition here, on the CPU.  The classification the kernels use
(csrc/nvbx_plan_math.h, compiled with gcc as C) gives the model's class words on the edge values, and the two knobs of the call parse as the
others do (csrc/nvbx_knobs.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plan_independent as PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
F32 = np.float32
BIG = np.int64(PI.UNREACHED)


def pull_relaxation(img, sources, o):
    """-> (G int32, sweeps): G(p) = min(G(p), G(q) + c(p, q)) over the eight neighbours, all pixels at once, until a sweep changes nothing"""
    trav, pen = PI.classify(img, o)
    G = np.full(trav.shape, BIG)
    for r, c in PI.accepted_sources(trav, sources):
        G[r, c] = 0
    for sweep in range(1, trav.size + 2):
        new = G.copy()
        for dr, dc in PI.MOVES:
            ok = trav & PI._shift(trav, dr, dc, False)
            if dr and dc:
                ok &= PI._shift(trav, dr, 0, False) & PI._shift(trav, 0, dc, False)
            gq = PI._shift(G, dr, dc, BIG)
            cand = gq + (14 if dr and dc else 10) + pen + PI._shift(pen, dr, dc, 0)
            new = np.where(ok & (gq != BIG), np.minimum(new, cand), new)
        if np.array_equal(new, G):
            return G.astype(np.int32), sweep
        G = new
    raise AssertionError("no fixed point")


@pytest.fixture(scope="module")
def cases():
    return PI.random_cases()


def test_random_cases_meet_their_condition(cases):
    o = PI.options(**PI.CASE_OPTIONS)
    assert len(cases) == len(PI.RANDOM_SHAPES) * PI.SEEDS_PER_SHAPE
    for shape, seed, img, sources in cases:
        assert img.shape == shape and img.dtype == F32 and sources.shape == (3, 2)
        assert PI.case_condition(img, sources, o), (shape, seed)
        G, acc = PI.field(img, sources, o)
        assert acc == 3 and (G[sources[:, 0], sources[:, 1]] == 0).all()
        frac = [(np.abs(img - v) < 1e-6).mean() for v in (PI.BLOCKED, PI.UNKNOWN)]
        assert 0.1 < frac[0] < 0.3 and 0.01 < frac[1] < 0.1, (shape, seed, frac)


def test_model_equals_the_pull_relaxation(cases):
    o = PI.options(**PI.CASE_OPTIONS)
    drawn = [(img, src, o) for _, _, img, src in cases] + [PI.line_case(s) + (o,) for s in PI.LINE_SHAPES]
    img, src = PI.serpentine(24)
    drawn.append((img, src, PI.options()))
    img, src = drawn[0][0], drawn[0][1]
    drawn.append((img, src, PI.options(allow_unknown=1, unknown_penalty=200, **PI.CASE_OPTIONS)))
    drawn.append((img, src, PI.options(allow_unknown=1, unknown_penalty=0, inflation_radius_m=0.0, robot_radius_m=0.0)))
    for k, (img, src, opt) in enumerate(drawn):
        G, _ = PI.field(img, src, opt)
        R, sweeps = pull_relaxation(img, src, opt)
        assert np.array_equal(G, R), (k, img.shape, sweeps)


def test_octile_closed_form_on_an_empty_image():
    img = np.full((37, 53), F32(5.0))
    for r0, c0 in ((0, 0), (36, 52), (17, 31), (36, 0)):
        G, acc = PI.field(img, [(r0, c0)], PI.options())
        dr = np.abs(np.arange(37) - r0)[:, None]; dc = np.abs(np.arange(53) - c0)[None, :]
        assert acc == 1 and np.array_equal(G, (10 * np.maximum(dr, dc) + 4 * np.minimum(dr, dc)).astype(np.int32))


def test_serpentine_of_the_gpu_test():
    img, src = PI.serpentine(96)
    G, _ = PI.field(img, src, PI.options())
    reached = G[G != PI.UNREACHED]
    assert int(reached.max()) == 46550 and len(reached) == 48 * 96 + 48
    far = np.unravel_index(np.argmax(np.where(G == PI.UNREACHED, -1, G)), G.shape)
    p = PI.path(img, G, far, PI.options())
    assert len(p) == 4656 and p[-1] == (0, 0)


def _check_path(img, G, start, o, p):
    trav, pen = PI.classify(img, o)
    assert p[0] == tuple(start) and G[p[-1]] == 0 and all(G[q] != 0 for q in p[:-1])
    total = 0
    for a, b in zip(p[:-1], p[1:]):
        dr, dc = b[0] - a[0], b[1] - a[1]
        assert max(abs(dr), abs(dc)) == 1 and trav[a] and trav[b]
        if dr and dc:
            assert trav[a[0] + dr, a[1]] and trav[a[0], a[1] + dc], "a corner was cut"
        total += (14 if dr and dc else 10) + int(pen[a]) + int(pen[b])
    assert total == int(G[p[0]])


def test_every_model_path_is_a_cheapest_move_sequence(cases):
    o = PI.options(**PI.CASE_OPTIONS)
    rng = np.random.default_rng(5)
    for shape, seed, img, sources in cases:
        G, _ = PI.field(img, sources, o)
        reach = np.argwhere(G != PI.UNREACHED)
        for start in reach[rng.choice(len(reach), 16, replace=False)]:
            p = PI.path(img, G, start, o)
            assert p, (shape, seed, start)
            _check_path(img, G, tuple(int(v) for v in start), o, p)
        assert PI.path(img, G, (-1, 0), o) == [] and PI.path(img, G, (0, shape[1]), o) == []
        blocked = np.argwhere(G == PI.UNREACHED)[0]
        assert PI.path(img, G, blocked, o) == []
    # a field of another image: some start finds no neighbour
    (_, _, img_a, src_a), (_, _, img_b, _) = cases[3], cases[4]
    Ga, _ = PI.field(img_a, src_a, o)
    reach = np.argwhere(Ga != PI.UNREACHED)
    assert any(PI.path(img_b, Ga, s, o) is None for s in reach)


# ---- the header the kernels classify with, compiled as C
def test_the_shared_header_classifies_as_the_model(tmp_path):
    src = tmp_path / "plan.c"; so = tmp_path / "plan.so"
    src.write_text('#include "nvbx_plan_math.h"\n'
                   "void classes(const float* v, int n, const nvbx_cost_options* o, int32_t* k) { for (int i = 0; i < n; i++) k[i] = nvbx_plan_class(v[i], o); }\n"
                   "int step(int d, int a, int b) { return nvbx_plan_step(d, a, b); }\n"
                   "int refused(const nvbx_cost_options* o) { return nvbx_plan_options_problem(o) != 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so), "-lm"])
    lib = ctypes.CDLL(str(so))
    from isaac_ros_nvblox_amd import _lib
    for kw in PI.EDGE_OPTIONS:
        o = PI.options(**kw)
        co = _lib.CostOptions(**{k: v for k, v in o.items()})
        assert lib.refused(ctypes.byref(co)) == 0, kw
        v = PI.edge_values(o)
        k = np.zeros(len(v), np.int32)
        lib.classes(v.ctypes.data_as(ctypes.c_void_p), len(v), ctypes.byref(co), k.ctypes.data_as(ctypes.c_void_p))
        trav, pen = PI.classify(v.reshape(1, -1), o)
        want = np.where(trav[0], pen[0], -1)
        assert np.array_equal(k, want), (kw, [(float(a), int(b), int(c)) for a, b, c in zip(v, k, want) if b != c][:5])
    assert (lib.step(0, 3, 4), lib.step(1, 200, 200)) == (17, 414)
    nan = float("nan")
    for kw in (dict(robot_radius_m=nan), dict(robot_radius_m=-0.1), dict(inflation_radius_m=nan), dict(inflation_radius_m=-1.0), dict(penalty_per_m=nan),
               dict(penalty_per_m=-1.0), dict(unknown_value=nan), dict(max_penalty=-1), dict(max_penalty=201), dict(unknown_penalty=-1), dict(unknown_penalty=201)):
        co = _lib.CostOptions(**PI.options(**kw))
        assert lib.refused(ctypes.byref(co)) == 1, kw


def test_the_two_knobs_parse_like_the_others(tmp_path):
    src = tmp_path / "k.c"; so = tmp_path / "k.so"
    src.write_text('#include "nvbx_knobs.h"\n'
                   "static const char* a; static const char* b;\n"
                   'static const char* look(const char* n) { return !strcmp(n, "NVBX_PLAN_ROUNDS_PER_WAIT") ? a : !strcmp(n, "NVBX_PLAN_TILE_SWEEPS") ? b : "7"; }\n'
                   "int rounds(const char* x, const char* y) { struct nvbx_plan_knobs k; a = x; b = y; nvbx_plan_knobs_read(&k, look); return k.rounds_per_wait; }\n"
                   "int sweeps(const char* x, const char* y) { struct nvbx_plan_knobs k; a = x; b = y; nvbx_plan_knobs_read(&k, look); return k.tile_sweeps; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    for f in (lib.rounds, lib.sweeps):
        f.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    for value, want in ((None, 16), (b"1", 1), (b"64", 64), (b"1024", 1024), (b"0", 16), (b"-3", 16), (b"1025", 16), (b"8x", 16), (b"", 16)):
        assert lib.rounds(value, b"3") == want, value
    for value, want in ((None, 64), (b"1", 1), (b"4096", 4096), (b"0", 64), (b"4097", 64), (b"x", 64)):
        assert lib.sweeps(None, value) == want, value
