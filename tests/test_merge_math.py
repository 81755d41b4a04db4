"""The host/device arithmetic of map merging that is not per-voxel (isaac_ros_nvblox_amd/csrc/nvbx_merge_math.h), compiled with g++ into the
stand-alone program tests/cpp/merge_math_check.cpp and compared with the numpy model of tests/merge_independent.py: the candidate boxes, the
rotation check, the float64 inverse rounded to float32.  The same program built with AddressSanitizer and UBSan gives identical output.
Nothing is loaded into python, nothing needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import merge_independent as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "merge_math_check.cpp")
F32 = np.float32
pose, drawn_transforms = MI.pose, MI.drawn_transforms


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, F32).reshape(-1))


def _bad_rotations():
    out = []
    T = np.eye(4, dtype=F32); T[2, 2] = -1.0; out.append(("mirror", T))
    out.append(("scaled", (np.eye(4) * np.array([1.001, 1.001, 1.001, 1.0])).astype(F32)))
    T = pose([1, 2, 3], 40.0, [0, 0, 0]); T[0, 1] += F32(1e-4); out.append(("sheared", T))
    T = pose([1, 2, 3], 40.0, [0, 0, 0]); T[0, 1] += F32(2e-6); out.append(("within", T))      # inside the 1e-5 bound
    T = np.zeros((4, 4), F32); T[3, 3] = 1; out.append(("zero", T))
    return out


def _cases():
    rng = np.random.default_rng(21)
    lines, expect = [], []
    Ts = drawn_transforms(24, seed=13)
    for T in Ts:
        lines.append("rot " + _hex(T)); expect.append(("rot", T, True))
        lines.append("inv " + _hex(T)); expect.append(("inv", T, None))
    for name, T in _bad_rotations():
        lines.append("rot " + _hex(T)); expect.append(("rot", T, name == "within"))
    for vs in (0.05, 0.0625, 0.1):
        for T in Ts[:12]:
            for s in rng.integers(-60, 60, (8, 3)):
                lines.append("box %s %s %d %d %d" % (_hex(vs), _hex(T), s[0], s[1], s[2])); expect.append(("box", T, (vs, s)))
    # far from the origin: near the end of the addressable range, and beyond it
    far = pose([0, 0, 1], 0.0, [1.0, 2.0, 3.0])
    lines.append("box %s %s %d %d %d" % (_hex(0.05), _hex(far), 1000000, -1000000, 7)); expect.append(("box", far, (0.05, np.array([1000000, -1000000, 7]))))
    lines.append("box %s %s %d %d %d" % (_hex(0.05), _hex(far), 1048575, 1048575, 1048575)); expect.append(("boxfail", far, None))
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
    td = tmp_path_factory.mktemp("merge_math")
    text, expect = _cases()
    plain = _run(_build(td, "check", []), text)
    assert len(plain) == len(expect)
    return td, text, expect, plain


def test_rotation_check(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, T, want), out in zip(expect, got):
        if kind != "rot":
            continue
        ok, err, det = int(out[1]), float.fromhex(out[2]), float.fromhex(out[3])
        e, d = MI.rotation_error(T)
        assert ok == int(want) == int(MI.rotation_ok(T))
        assert abs(err - e) <= 1e-14 and abs(det - d) <= 1e-14
        seen += 1
    assert seen == 27 + 5


def test_the_inverse_is_the_float64_inverse_rounded_once(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, T, _), out in zip(expect, got):
        if kind != "inv":
            continue
        v = np.array([float.fromhex(t) for t in out[1:]])
        R_DS, t_DS, R_SD, t_SD = MI.transforms(T)
        assert np.array_equal(v[:9].astype(F32), R_DS.reshape(-1)) and np.array_equal(v[9:12].astype(F32), t_DS)
        assert np.array_equal(v[12:21].astype(F32).view(np.uint32), R_SD.reshape(-1).view(np.uint32))
        assert np.array_equal(v[21:24].astype(F32).view(np.uint32), t_SD.view(np.uint32))
        # and it is an inverse: within one f32 rounding of the exact one
        exact = -(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))
        assert np.abs(t_SD - exact).max() <= np.abs(exact).max() * 2.0 ** -24 + 1e-45
        seen += 1
    assert seen == 27


def test_candidate_boxes_equal_the_models(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, T, arg), out in zip(expect, got):
        if kind == "box":
            vs, s = arg
            lo, hi = MI.candidate_boxes(T, [s], vs)
            assert int(out[1]) == 1
            assert [int(x) for x in out[2:5]] == list(lo[0]) and [int(x) for x in out[5:8]] == list(hi[0]), (vs, s)
            assert all(0 <= h - l <= 2 for l, h in zip(lo[0], hi[0]))
            seen += 1
        elif kind == "boxfail":
            assert int(out[1]) == 0 and [int(x) for x in out[2:8]] == [0, 0, 0, -1, -1, -1]
    assert seen == 3 * 12 * 8 + 1


def test_the_same_program_gives_identical_output_under_asan_and_ubsan(answers):
    td, text, _, plain = answers
    exe = _build(td, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert _run(exe, text) == plain
