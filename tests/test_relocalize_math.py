"""The host arithmetic of the search lattice (isaac_ros_nvblox_amd/csrc/nvbx_relocalize_math.h), compiled with g++ into the stand-alone program
tests/cpp/relocalize_math_check.cpp and compared bit for bit with the numpy tables of tests/relocalize_independent.py: the offset tables, the yaw
matrices, every pose and the indexing; the lattices the header refuses.  The same program built with AddressSanitizer and UBSan runs clean and
prints the same.  Nothing is loaded into python, nothing needs a GPU."""
import os
import subprocess

import numpy as np
import pytest

import relocalize_independent as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "relocalize_math_check.cpp")


def _pose(rng, yaw_only=False):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    if yaw_only:
        ax = np.array([0.0, 0.0, 1.0])
    th = rng.uniform(-np.pi, np.pi)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rng.uniform(-20.0, 20.0, 3)
    return T.astype(np.float32)


def _cases():
    """(T0, half extents, half yaw, steps): the test lattice, one step per axis, 64 steps on an axis, odd and even counts, zero extents, the
    2^20 product; then what the header refuses"""
    rng = np.random.default_rng(11)
    good = [(_pose(rng), (0.4, 0.4, 0.0), np.deg2rad(20.0), (5, 5, 1, 9)),
            (_pose(rng), (0.0, 0.0, 0.0), 0.0, (1, 1, 1, 1)),
            (_pose(rng), (1.0, 0.5, 0.25), np.pi, (64, 1, 1, 2)),
            (_pose(rng), (0.3, 0.7, 0.1), 0.3, (2, 3, 4, 64)),
            (_pose(rng, True), (0.123, 0.0, 2.0), 1e-3, (7, 2, 6, 5)),
            (_pose(rng), (0.0, 0.0, 0.0), 0.5, (3, 3, 1, 4)),
            (np.eye(4, dtype=np.float32), (2.0, 2.0, 0.5), np.pi / 2, (16, 16, 4, 16))]
    bad = [(_pose(rng), (0.4, 0.4, 0.0), 0.1, (0, 5, 1, 9)), (_pose(rng), (0.4, 0.4, 0.0), 0.1, (5, 65, 1, 9)),
           (_pose(rng), (0.4, 0.4, 0.0), 0.1, (5, 5, -1, 9)), (_pose(rng), (0.4, 0.4, 0.0), 0.1, (64, 64, 64, 5)),
           (_pose(rng), (-0.1, 0.4, 0.0), 0.1, (5, 5, 1, 9)), (_pose(rng), (0.4, np.inf, 0.0), 0.1, (5, 5, 1, 9)),
           (_pose(rng), (0.4, 0.4, np.nan), 0.1, (5, 5, 1, 9)), (_pose(rng), (0.4, 0.4, 0.0), -0.1, (5, 5, 1, 9)),
           (_pose(rng), (0.4, 0.4, 0.0), np.nan, (5, 5, 1, 9))]
    good.append((_pose(rng), (0.5, 0.5, 0.5), 1.0, (64, 64, 16, 16)))          # exactly 2^20 (only its head is compared: see the test)
    return good, bad


def _line(T0, he, hy, steps):
    f = np.concatenate([np.asarray(T0, np.float32).reshape(-1), np.asarray(he, np.float32), np.asarray([hy], np.float32)]).view(np.uint32)
    return " ".join("%08x" % v for v in f) + " " + " ".join(str(int(s)) for s in steps)


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + [SRC, "-o", str(exe)])
    return str(exe)


def _run(exe, text):
    r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr.decode()[-2000:])
    return r.stdout.decode().splitlines()


def _u32(line):
    return np.array([int(t, 16) for t in line.split()], np.uint32)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    td = tmp_path_factory.mktemp("relocalize_math")
    good, bad = _cases()
    text = "\n".join(_line(*c) for c in good[:-1] + bad) + "\n"
    return td, text, good, bad, _run(_build(td, "check", []), text)


def test_tables_and_poses_equal_the_numpy_model_bit_for_bit(answers):
    _, _, good, bad, out = answers
    at = 0
    for T0, he, hy, steps in good[:-1]:
        K = int(np.prod(steps))
        assert out[at].split() == ["1", str(K)]
        dx, dy, dz, R = RI.lattice_tables(T0, he, hy, steps)
        for a, tab in enumerate((dx, dy, dz)):
            assert np.array_equal(_u32(out[at + 1 + a]), tab.view(np.uint32)), (steps, a)
            if steps[a] > 1:       # the ends are the half-extent itself (2 h (s - 1) / (s - 1) is exact) and, with an odd count, the middle is an exact 0
                assert tab[0] == -np.float32(he[a]) and tab[-1] == np.float32(he[a]) and (steps[a] % 2 == 0 or tab[steps[a] // 2] == 0.0)
            else:
                assert tab[0] == 0.0
        for w in range(steps[3]):
            assert np.array_equal(_u32(out[at + 4 + w]), R[w].reshape(-1).view(np.uint32)), (steps, w)
        poses = RI.lattice_poses(T0, he, hy, steps)
        got = np.stack([_u32(l) for l in out[at + 4 + steps[3]:at + 4 + steps[3] + K]]).view(np.float32).reshape(K, 4, 4)
        assert np.array_equal(got.view(np.uint32), poses.view(np.uint32)), steps
        at += 4 + steps[3] + K
    for _ in bad:
        assert out[at] == "0"
        at += 1
    assert at == len(out)
    for c in bad:
        assert not RI.lattice_ok(*c[1:])
    for c in good:
        assert RI.lattice_ok(*c[1:])


def test_lattice_indexing_and_geometry():
    """h = ((ix ny + iy) nz + iz) nyaw + iw; with an odd count per axis the middle node is T0 itself; a yaw step turns about the layer's z
    through the sensor origin (the translation does not move), an x step moves along the layer's x"""
    rng = np.random.default_rng(3)
    T0 = _pose(rng)
    he, hy, steps = (0.4, 0.2, 0.1), 0.35, (5, 3, 3, 7)
    P = RI.lattice_poses(T0, he, hy, steps)
    assert len(P) == 5 * 3 * 3 * 7
    seen = set()
    for ix in range(5):
        for iy in range(3):
            for iz in range(3):
                for iw in range(7):
                    h = RI.lattice_index(steps, ix, iy, iz, iw)
                    assert RI.lattice_unravel(steps, h) == (ix, iy, iz, iw)
                    seen.add(h)
    assert seen == set(range(len(P)))
    mid = RI.lattice_index(steps, 2, 1, 1, 3)
    assert np.array_equal(P[mid], T0)
    for iw in range(7):
        assert np.array_equal(P[RI.lattice_index(steps, 2, 1, 1, iw)][:3, 3], T0[:3, 3])
        assert abs(RI.yaw_between(P[RI.lattice_index(steps, 2, 1, 1, iw)], T0) - (-hy + 2 * hy * iw / 6)) < 1e-6
    d = P[RI.lattice_index(steps, 4, 1, 1, 3)][:3, 3] - P[RI.lattice_index(steps, 0, 1, 1, 3)][:3, 3]
    assert np.allclose(d, [0.8, 0.0, 0.0], atol=1e-5)
    R = P[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6


def test_the_largest_lattice_is_accepted_and_written_whole(answers):
    """2^20 poses: the count, the first and the last pose (the whole table would be 16 M numbers of text)"""
    td, _, good, _, _ = answers
    T0, he, hy, steps = good[-1]
    out = _run(os.path.join(str(td), "check"), _line(T0, he, hy, steps) + "\n")
    assert out[0].split() == ["1", str(1 << 20)] and len(out) == 1 + 3 + 16 + (1 << 20)
    dx, dy, dz, R = RI.lattice_tables(T0, he, hy, steps)
    first = _u32(out[20]).view(np.float32).reshape(4, 4); last = _u32(out[-1]).view(np.float32).reshape(4, 4)
    assert np.array_equal(first[:3, :3], R[0]) and np.array_equal(last[:3, :3], R[-1])
    assert np.array_equal(first[:3, 3], T0[:3, 3] + np.array([dx[0], dy[0], dz[0]], np.float32))
    assert np.array_equal(last[:3, 3], T0[:3, 3] + np.array([dx[-1], dy[-1], dz[-1]], np.float32))


def test_the_same_program_runs_clean_under_asan_and_ubsan(answers):
    td, text, _, _, plain = answers
    exe = _build(td, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert _run(exe, text) == plain
