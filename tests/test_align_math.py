"""The host/device arithmetic of one alignment step (isaac_ros_nvblox_amd/csrc/nvbx_align_math.h), compiled with g++ into the stand-alone program
tests/cpp/align_math_check.cpp and compared with numpy float64 / long double formulas: the damped Cholesky solve and its pivot rule, the
exponential map against its series, orthonormality under composition.  The same program built with AddressSanitizer and UBSan runs clean.
Nothing is loaded into python, nothing needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import align_independent as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "align_math_check.cpp")
EPS = 2.0 ** -52


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float64).reshape(-1))


def _tri(H):
    return np.asarray(H)[np.triu_indices(6)]


def _spd(rng, cond):
    Qm, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    lam = np.logspace(0, np.log10(cond), 6) * rng.uniform(0.5, 2.0)
    H = (Qm * lam) @ Qm.T
    return (H + H.T) / 2


def _deficient(rng, rank):
    J = rng.normal(size=(rank, 6))
    return J.T @ J


def _solve_longdouble(H, b):
    """Cholesky in long double (64-bit mantissa on x86): the reference the f64 solve is measured against"""
    A_ = np.asarray(H, np.longdouble); L = np.zeros((6, 6), np.longdouble)
    for k in range(6):
        L[k, k] = np.sqrt(A_[k, k] - L[k, :k] @ L[k, :k])
        for i in range(k + 1, 6):
            L[i, k] = (A_[i, k] - L[i, :k] @ L[k, :k]) / L[k, k]
    y = np.zeros(6, np.longdouble); x = np.zeros(6, np.longdouble)
    for i in range(6):
        y[i] = (-np.longdouble(b[i]) - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(5, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def _cases():
    rng = np.random.default_rng(7)
    lines, expect = [], []
    for cond in (1e1, 1e3, 1e6, 1e9):
        for _ in range(8):
            H = _spd(rng, cond); b = rng.normal(size=6)
            lines.append("solve %s %s %s %s" % (_hex(0.0), _hex(1e-12), _hex(_tri(H)), _hex(b))); expect.append(("solve", H, b))
    for rank in (3, 5):
        for _ in range(4):
            H = _deficient(rng, rank); b = rng.normal(size=6)
            lines.append("solve %s %s %s %s" % (_hex(0.0), _hex(1e-9), _hex(_tri(H)), _hex(b))); expect.append(("deficient", H, b))
            lines.append("solve %s %s %s %s" % (_hex(1e-3), _hex(1e-9), _hex(_tri(H)), _hex(b))); expect.append(("damped", H, b))
    for th in (0.0, 1e-12, 1e-8, 1e-4, 1.0, np.pi - 1e-3):
        for _ in range(3):
            ax = rng.normal(size=3); w = ax / np.linalg.norm(ax) * th
            lines.append("exp %s" % _hex(w)); expect.append(("exp", w, th))
    steps = np.concatenate([rng.normal(size=(64, 3)) * 0.1, rng.normal(size=(64, 3)) * 0.2], 1)
    lines.append("compose 64\n" + "\n".join(_hex(s) for s in steps)); expect.append(("compose", steps, None))
    return "\n".join(lines) + "\n", expect


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + [SRC, "-o", str(exe)])
    return str(exe)


def _run(exe, text):
    r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr.decode()[-2000:])
    return [[float.fromhex(t) if i or not t.isalpha() else t for i, t in enumerate(l.split())] for l in r.stdout.decode().splitlines()]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    td = tmp_path_factory.mktemp("align_math")
    text, expect = _cases()
    plain = _run(_build(td, "check", []), text)
    assert len(plain) == len(expect)
    return td, text, expect, plain


def test_cholesky_solve_is_as_accurate_as_the_condition_number_allows(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, H, b), out in zip(expect, got):
        if kind != "solve":
            continue
        ok, worst, x = out[0], out[1], np.array(out[2:8])
        ref = _solve_longdouble(H, b)
        cond = np.linalg.cond(H)
        rel = float(np.linalg.norm((x - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))
        assert ok == 1 and worst > 1e-12
        assert rel <= 64 * cond * EPS, (cond, rel)
        mine, _ = A.solve(H, b, 0.0, 1e-12)
        assert np.linalg.norm(mine - x) / np.linalg.norm(x) <= 64 * cond * EPS       # the numpy model of the tests agrees as well
        seen += 1
    assert seen == 32


def test_pivot_rule_refuses_rank_3_and_rank_5_and_damping_repairs_them(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, H, b), out in zip(expect, got):
        if kind == "deficient":
            assert out[0] == 0 and out[1] <= 1e-9, out[:2]
            assert out[2:8] == [0.0] * 6                      # x is left as it was
            assert A.solve(H, b)[0] is None
            seen += 1
        elif kind == "damped":
            x = np.array(out[2:8])
            assert out[0] == 1
            Ad = H + 1e-3 * np.diag(np.diag(H))
            assert np.linalg.norm(Ad @ x + b) <= 1e-9 * max(1.0, np.linalg.norm(b))
            seen += 1
    assert seen == 16


def test_exponential_map_equals_its_series(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, w, th), out in zip(expect, got):
        if kind != "exp":
            continue
        R = np.array(out[1:10]).reshape(3, 3); V = np.array(out[10:19]).reshape(3, 3)
        Rs, Vs = A.exp_so3_series(w)
        assert np.abs(R - Rs).max() <= 1e-14 and np.abs(V - Vs).max() <= 1e-14, (th, np.abs(R - Rs).max(), np.abs(V - Vs).max())
        Rm, Vm = A.exp_so3(w)
        assert np.abs(R - Rm).max() <= 1e-15 and np.abs(V - Vm).max() <= 1e-15      # the tests' numpy model: the same closed forms
        seen += 1
    assert seen == 18


def test_rotation_stays_orthonormal_over_64_composed_steps(answers):
    _, _, expect, got = answers
    (kind, steps, _), out = expect[-1], got[-1]
    assert kind == "compose"
    R = np.array(out[1:10]).reshape(3, 3); t = np.array(out[10:13])
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(R) - 1.0) <= 1e-13
    T = np.eye(4)
    for s in steps:
        T = A.apply_step(T, s)
    assert np.abs(T[:3, :3] - R).max() <= 1e-12 and np.abs(T[:3, 3] - t).max() <= 1e-12


def test_the_same_program_runs_clean_under_asan_and_ubsan(answers):
    td, text, _, plain = answers
    exe = _build(td, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert _run(exe, text) == plain
