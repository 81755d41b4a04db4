"""The host/device arithmetic of resampling that is not per-voxel (isaac_ros_nvblox_amd/csrc/nvbx_resample_math.h), compiled with g++ into the
stand-alone program tests/cpp/resample_math_check.cpp and compared with the numpy model of tests/resample_independent.py: the ratio check,
the tap count, the reach N, the tap offsets and the candidate boxes.  The same program built with AddressSanitizer and UBSan gives identical
output.  Nothing is loaded into python, nothing needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import merge_independent as MI
import resample_independent as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "resample_math_check.cpp")
F32 = np.float32
VS_S = 0.05
VS_D = (0.05, 0.075, 0.1, 0.15, 0.2)
BAD_PAIRS = ((0.05, 0.1), (0.049, 0.05), (0.2001, 0.05), (0.25, 0.05), (0.0, 0.05), (0.05, 0.0), (-0.1, -0.05), (float("nan"), 0.05))


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, F32).reshape(-1))


def _cases():
    rng = np.random.default_rng(31)
    lines, expect = [], []
    for vd in VS_D + (0.0625, 0.19999):
        for taps in (-1, 0, 1, 2, 3, 4, 5):
            lines.append("ratio %s %s %d" % (_hex(vd), _hex(VS_S), taps)); expect.append(("ratio", (vd, VS_S, taps)))
    for vd, vs in BAD_PAIRS:
        lines.append("ratio %s %s 0" % (_hex(vd), _hex(vs))); expect.append(("bad", (vd, vs)))
    for n in (1, 2, 3, 4):
        lines.append("off %d" % n); expect.append(("off", n))
    Ts = MI.drawn_transforms(10, seed=17)
    for vd in VS_D:
        for n in (1, 2, 3, 4):
            for T in Ts[:8]:
                for s in rng.integers(-60, 60, (3, 3)):
                    lines.append("box %s %s %s %d %d %d %d" % (_hex(VS_S), _hex(vd), _hex(T), n, s[0], s[1], s[2]))
                    expect.append(("box", (T, vd, n, s)))
    far = MI.pose([0, 0, 1], 0.0, [1.0, 2.0, 3.0])
    lines.append("box %s %s %s 1 %d %d %d" % (_hex(VS_S), _hex(VS_S), _hex(far), 1048575, 1048575, 1048575)); expect.append(("boxfail", None))
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
    td = tmp_path_factory.mktemp("resample_math")
    text, expect = _cases()
    plain = _run(_build(td, "check", []), text)
    assert len(plain) == len(expect)
    return td, text, expect, plain


def test_ratio_taps_and_reach(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, arg), out in zip(expect, got):
        if kind == "ratio":
            vd, vs, taps = arg
            r = RI.ratio(vd, vs)
            n = RI.taps_for(r, taps)
            assert int(out[1]) == 1 == int(RI.ratio_ok(vd, vs)) and float.fromhex(out[2]) == r
            assert int(out[3]) == (n or 0) and int(out[4]) == (RI.reach_bound(r, n) if n else 0), arg
            if n:
                assert RI.reach_bound(r, n) ** 3 <= 512
            seen += 1
        elif kind == "bad":
            assert int(out[1]) == 0 == int(RI.ratio_ok(*arg)) and int(out[3]) == 0, arg
    assert seen == 7 * 7
    # the values the semantics quote
    assert [RI.reach_bound(1.0, 1), RI.reach_bound(2.0, 2), RI.reach_bound(4.0, 4), RI.reach_bound(4.0, 1)] == [3, 5, 8, 8]
    assert [RI.taps_for(r) for r in (1.0, 1.5, 2.0, 2.5, 3.0, 4.0)] == [1, 2, 2, 3, 3, 4]
    assert RI.ratio(0.2, 0.05) == 4.0 and RI.ratio(0.1, 0.05) == 2.0          # the float32 voxel sizes share a significand


def test_tap_offsets(answers):
    _, _, expect, got = answers
    for (kind, n), out in zip(expect, got):
        if kind != "off":
            continue
        v = np.array([float.fromhex(t) for t in out[1:]]).astype(F32)
        want = RI.tap_offsets(n)
        assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), n
        assert np.array_equal(v, -v[::-1]), "symmetric about the centre"        # a plane is reproduced where all taps are valid
        assert np.abs(v).max() <= 0.5 * (1.0 - 1.0 / n) + 1e-7
    assert RI.tap_offsets(1).view(np.uint32)[0] == 0                           # + 0.0f: the n = 1 position is the merge's


def test_candidate_boxes_equal_the_models(answers):
    _, _, expect, got = answers
    seen = 0
    for (kind, arg), out in zip(expect, got):
        if kind == "box":
            T, vd, n, s = arg
            lo, hi = RI.candidate_boxes(T, [s], VS_S, vd, n)
            assert int(out[1]) == 1
            assert [int(x) for x in out[2:5]] == list(lo[0]) and [int(x) for x in out[5:8]] == list(hi[0]), (vd, n, s)
            assert all(0 <= h - l <= 2 for l, h in zip(lo[0], hi[0]))
            if vd == VS_S and n == 1:
                ml, mh = MI.candidate_boxes(T, [s], VS_S)
                assert np.array_equal(ml, lo) and np.array_equal(mh, hi)
            seen += 1
        elif kind == "boxfail":
            assert int(out[1]) == 0 and [int(x) for x in out[2:8]] == [0, 0, 0, -1, -1, -1]
    assert seen == 5 * 4 * 8 * 3


def test_the_same_program_gives_identical_output_under_asan_and_ubsan(answers):
    td, text, _, plain = answers
    exe = _build(td, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert _run(exe, text) == plain
