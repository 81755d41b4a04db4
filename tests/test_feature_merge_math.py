"""The candidate box of feature merging (isaac_ros_nvblox_amd/csrc/nvbx_feature_merge_math.h), compiled with g++ into the stand-alone program
tests/cpp/feature_merge_math_check.cpp and compared with the numpy model of tests/feature_merge_independent.py.  The same program built with
AddressSanitizer and UBSan gives identical output.  Nothing is loaded into python, nothing needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import feature_merge_independent as FM
import merge_independent as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "feature_merge_math_check.cpp")
F32 = np.float32


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, F32).reshape(-1))


def _cases():
    rng = np.random.default_rng(31)
    lines, expect = [], []
    Ts = MI.drawn_transforms(12, seed=17) + [FM.pose([1, 2, 3], 45.0, [0.37, -0.21, 0.13]), FM.pose([0, 0, 1], 90.0, [0.11, -0.27, 0.4])]
    for vs in (0.05, 0.0625, 0.1):
        for T in Ts:
            for s in rng.integers(-60, 60, (6, 3)):
                lines.append("fbox %s %s %d %d %d" % (_hex(vs), _hex(T), s[0], s[1], s[2])); expect.append(("box", T, (vs, s)))
    far = FM.pose([0, 0, 1], 0.0, [1.0, 2.0, 3.0])
    lines.append("fbox %s %s %d %d %d" % (_hex(0.05), _hex(far), 1000000, -1000000, 7)); expect.append(("box", far, (0.05, np.array([1000000, -1000000, 7]))))
    lines.append("fbox %s %s %d %d %d" % (_hex(0.05), _hex(far), 1048575, 1048575, 1048575)); expect.append(("boxfail", far, None))
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
    td = tmp_path_factory.mktemp("feature_merge_math")
    text, expect = _cases()
    plain = _run(_build(td, "check", []), text)
    assert len(plain) == len(expect)
    return td, text, expect, plain


def test_candidate_boxes_equal_the_models_and_differ_from_the_merges(answers):
    _, _, expect, got = answers
    seen = differ = 0
    for (kind, T, arg), out in zip(expect, got):
        if kind == "box":
            vs, s = arg
            lo, hi = FM.candidate_boxes(T, [s], vs)
            assert int(out[1]) == 1
            assert [int(x) for x in out[2:5]] == list(lo[0]) and [int(x) for x in out[5:8]] == list(hi[0]), (vs, s)
            assert all(0 <= h - l <= 2 for l, h in zip(lo[0], hi[0]))
            mlo, mhi = MI.candidate_boxes(T, [s], vs)
            differ += int(not (np.array_equal(mlo, lo) and np.array_equal(mhi, hi)))
            seen += 1
        elif kind == "boxfail":
            assert int(out[1]) == 0 and [int(x) for x in out[2:8]] == [0, 0, 0, -1, -1, -1]
    assert seen == 3 * 17 * 6 + 1
    assert differ > 0          # (the cube is not the merge's half-voxel-shifted one)


def test_the_same_program_gives_identical_output_under_asan_and_ubsan(answers):
    td, text, _, plain = answers
    exe = _build(td, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert _run(exe, text) == plain
