"""The per-edge arithmetic of nvbx_surface_points (isaac_ros_nvblox_amd/csrc/nvbx_surface_math.h), compiled with g++ into the stand-alone program
tests/cpp/surface_math_check.cpp and compared with the numpy model of tests/surface_independent.py on drawn operands: the observed and crossing
tests, the colour end, the position bit for bit, the floor-modulo and the origin filter.  The same program built with AddressSanitizer and UBSan
gives identical output.  Nothing is loaded into python, nothing needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import surface_independent as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "surface_math_check.cpp")
F32 = np.float32


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, F32).reshape(-1))


def _cases():
    rng = np.random.default_rng(27)
    lines, expect = [], []
    special = [0.0, -0.0, 1.0, -1.0, 0.05, -0.05, float("nan"), 1e-4, 0.99e-4]
    edges = [(a, w0, b, w1, mw) for a in special for b in special for w0, w1, mw in ((1.0, 1.0, 1e-4), (1e-4, 0.99e-4, 1e-4), (0.0, 0.0, 0.0), (0.0, 1.0, -1.0))]
    edges += [tuple(rng.uniform(-0.2, 0.2, 2).tolist()[:1] + [rng.uniform(0, 2e-4)] + rng.uniform(-0.2, 0.2, 1).tolist() + [rng.uniform(0, 2e-4), 1e-4]) for _ in range(300)]
    for e in edges:
        lines.append("edge " + _hex(e)); expect.append(("edge", np.asarray(e, F32)))
    for _ in range(600):
        vs = F32(rng.choice([0.05, 0.04, 0.1, 0.0625, 0.2]))
        d0 = F32(rng.uniform(-4, 4) * vs); d1 = F32(-np.sign(d0) * rng.uniform(0, 4) * vs) if rng.random() < 0.9 else F32(0.0)
        b = int(rng.integers(-3000, 3000)); v = int(rng.integers(0, 8))
        lines.append("pos %s %s %s %d %d" % (_hex(vs), _hex(d0), _hex(d1), b, v)); expect.append(("pos", (vs, d0, d1, b, v)))
    for vs, d0, d1, b, v in ((F32(0.05), F32(0.0), F32(0.3), 2, 3), (F32(0.05), F32(-0.0), F32(0.3), -2, 3), (F32(0.05), F32(0.3), F32(0.0), -1 << 20, 0),
                             (F32(0.05), F32(-0.2), F32(0.0), (1 << 20) - 1, 7)):
        lines.append("pos %s %s %s %d %d" % (_hex(vs), _hex(d0), _hex(d1), b, v)); expect.append(("pos", (vs, d0, d1, b, v)))
    for g in list(range(-17, 18)) + [-(1 << 31), (1 << 31) - 1, -8388608, 8388607]:
        for s in (1, 2, 3, 4, 7, 8, 1 << 30):
            lines.append("mod %d %d" % (g, s)); expect.append(("mod", (g, s)))
    for _ in range(400):
        stride = int(rng.choice([1, 1, 2, 3, 5])); use_box = int(rng.random() < 0.6)
        lo = rng.integers(-12, 6, 3); hi = lo + rng.integers(0, 10, 3); g = rng.integers(-14, 16, 3)
        k = [stride, use_box] + lo.tolist() + hi.tolist() + g.tolist()
        lines.append("keep " + " ".join(str(int(x)) for x in k)); expect.append(("keep", (stride, use_box, lo, hi, g)))
    return "\n".join(lines) + "\n", expect


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + [SRC, "-o", str(exe)])
    return str(exe)


def _run(exe, text):
    r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr.decode()[-2000:])
    return [l.split() for l in r.stdout.decode().splitlines()]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    td = tmp_path_factory.mktemp("surface_math")
    text, expect = _cases()
    plain = _run(_build(td, "check", []), text)
    assert len(plain) == len(expect)
    return td, text, expect, plain


def test_observed_crossing_and_colour_end(answers):
    _, _, expect, got = answers
    seen = crossing = 0
    for (kind, e), out in zip(expect, got):
        if kind != "edge":
            continue
        d0, w0, d1, w1, mw = e
        o0 = bool(SI.observed(d0, w0, mw)); o1 = bool(SI.observed(d1, w1, mw))
        cross = o0 and o1 and (bool(d0 <= 0) != bool(d1 <= 0))
        near0 = bool(np.abs(d0) <= np.abs(d1))
        assert [int(x) for x in out[1:4]] == [int(o0), int(o1), int(cross)], e.tolist()
        if not (np.isnan(d0) or np.isnan(d1)):
            assert int(out[4]) == (0 if near0 else 1), e.tolist()
        seen += 1; crossing += cross
    assert seen > 600 and 50 < crossing < seen - 50


def test_positions_bit_for_bit(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, arg), out in zip(expect, got):
        if kind != "pos":
            continue
        vs, d0, d1, b, v = arg
        c = SI.center(b, v, vs); x = F32(c + SI.crossing_offset(d0, d1, vs))
        have = np.array([float.fromhex(out[1]), float.fromhex(out[2])]).astype(F32)
        assert have[0].view(np.uint32) == F32(c).view(np.uint32), arg
        assert have[1].view(np.uint32) == x.view(np.uint32), arg
        seen += 1
    assert seen == 604


def test_floor_modulo_and_origin_filter(answers):
    _, _, expect, got = answers
    for (kind, arg), out in zip(expect, got):
        if kind == "mod":
            g, s = arg
            assert int(out[1]) == g % s, arg                      # (Python's % is the mathematical one)
            assert int(out[1]) == int(SI.floor_mod(g, s)), arg
        elif kind == "keep":
            stride, use_box, lo, hi, g = arg
            want = all(int(x) % stride == 0 for x in g) and (not use_box or all(l <= x <= h for l, x, h in zip(lo, g, hi)))
            assert int(out[1]) == int(want), arg


def test_the_same_program_gives_identical_output_under_asan_and_ubsan(answers):
    td, text, _, plain = answers
    exe = _build(td, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert _run(exe, text) == plain
