"""The ESDF site-marking pass of the product (csrc/nvbx_esdf_mark.h esdf_mark_entry / esdf_mark_worker, csrc/esdf3d.hip k_esdf3_mark) on the drawn
cases of tests/esdf_mark_cases.py: voxels on every threshold of the predicate, bands of 1 .. 63 blocks with missing blocks and negative heights,
re-marking, a dirty list longer than a carrier's workers, a tilted ground plane, an occupancy mapper, the 3-D mode.  tests/test_esdf_mark_model.py
validates the expectations on the CPU.

Every case: a fresh Mapper, set_blocks, update_esdf, the WHOLE ESDF layer read back.  Then, with nothing sampled or tolerated,
  1. is_site / observed / is_inside of every allocated voxel == the model, and the ESDF block set == the model's,
  2. squared_distance_vox of every allocated voxel == the brute force over the model's site set, the parents valid,
  3. the blocks == the CPU checker's, every field.

WHICH LAUNCH carried the marking pass is asserted from the launch profile, by elimination (a profile names launches, not what rode in them; the
site masks are written by the marking pass alone, so a correct layer with no k_esdf_mark launch had it carried by another one):
  mark   k_esdf_mark, up to 1024 workers: update_esdf straight after set_blocks (every test but the carrier test runs this path).
  color  the 256 riders of k_integrate_color: colour deferral off, a far-away colour frame after the drawn blocks, then update_esdf -- no
         k_esdf_mark, and the only other launch of the colour call, k_sphere_trace, carries riders only in a replay (next line).
  held   the riders behind the sphere-tracing workgroups: colour deferral on, the colour frame and the update both held back and replayed as a
         pair by the read-back -- no k_esdf_mark, no k_esdf_edt: the distance transform rode in k_integrate_color, which carries it only when
         it carries no marking pass; that leaves k_sphere_trace.
  view   the riders of k_mark_view in pipelined order (four workers per workgroup, 1024 to 4096): a far depth frame, the colour frame and the
         update held back, the next far depth frame carries them -- no k_esdf_mark, no k_integrate_color (one k_integrate_tsdf_color).
The frames look at a wall 120 m from the drawn blocks; over the drawn box the layer must equal the model and the `mark` run in every field.
"""
import re

import numpy as np
import pytest

import esdf_cases as EC
import esdf_independent as EI
import esdf_mark_cases as MC
import helpers as H

pytestmark = pytest.mark.gpu

FAR_CAM = H.SMALL_CAM
CARRIERS = ("mark", "color", "held", "view")


def _M():
    from isaac_ros_nvblox_amd import mapper as M
    return M


def _layer(M, case):
    return M.LAYER_OCCUPANCY if case.layer == "occ" else M.LAYER_TSDF


def _write(M, g, case, idx, data):
    if case.layer == "occ":
        t = np.zeros(data.shape, M.OCCUPANCY_DT); t["log_odds"] = data; data = t
    g.set_blocks(_layer(M, case), idx, data)


def _read(M, g):
    return H.map_state(g, layers=(M.LAYER_ESDF,))["layers"][M.LAYER_ESDF]


def _kernels(g):
    names = {}
    for k, v in g.profile().items():
        m = re.match(r"\s*(?:void\s+)?(k_[a-z_0-9]+)", k)
        if m:
            names[m.group(1)] = names.get(m.group(1), 0) + v["count"]
    return names


def _far_frame(k):
    """A depth + colour frame of a wall 1.03 m in front of a camera 120 m (+ 3 m per k) from the drawn blocks."""
    T = np.eye(4, dtype=np.float32); T[0, 3] = 120.0 + 3.0 * k; T[1, 3] = 1.0; T[2, 3] = -1.0
    return np.full((FAR_CAM[5], FAR_CAM[4]), 1.03, np.float32), np.full((FAR_CAM[5], FAR_CAM[4], 3), 90, np.uint8), T


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_marks_equal_the_model_and_the_checker(oracle_mod, hip_lib, name):
    """Every case, every step of it: block set, marks, distances and parents against the model; every field of every block against the checker."""
    M = _M()
    case = MC.case_by_name(M, name)
    p, q = MC.params(M, case)
    exps = MC.expectations(case, p)
    g = M.Mapper(p, block_capacity=case.capacity)
    checker = MC.checker_steps(oracle_mod, case, p)
    for k, ((idx, data), exp) in enumerate(zip(case.steps, exps)):
        _write(M, g, case, idx, data)
        g.update_esdf()
        gi, gb = _read(M, g)
        MC.assert_expected((name, "step", k), gi, gb, p, q, exp, case.dims)
        oi, ob = next(checker)
        EC.assert_same_blocks((name, "step", k, "against the checker"), gi, gb, oi, ob)
    assert g.counters()["capacity_overflow"] == 0
    g.close()


@pytest.mark.parametrize("name", MC.REFUSED_NAMES)
def test_refused_bands_leave_the_map_untouched(oracle_mod, hip_lib, name):
    """A z band of 64 blocks, or one whose upper height lies in a block row below the lower one's: update_esdf fails with NVBX_E_INVALID (-1)
    and the library's message, TSDF and ESDF layers stay as they were with an edit still waiting, and after set_params back to the legal band
    the next update carries the edit out."""
    M = _M()
    case = MC.case_by_name(M, name)
    p, q = MC.params(M, case)
    idx, data = case.steps[0]
    g = M.Mapper(p, block_capacity=case.capacity)
    g.set_blocks(M.LAYER_TSDF, idx, data)
    g.update_esdf()
    MC.assert_expected((name, "before"), *_read(M, g), p, q, MC.expectations(case, p)[0], 2)
    vx, vy = MC.BAND_COLUMNS["hi"]
    k = idx.tolist().index([0, 0, 1])
    edit = data[k].copy().reshape(8, 8, 8)
    assert edit["distance"][vx, vy, 13 & 7] == MC.SITE_D
    edit["distance"][vx, vy, 13 & 7] = MC.TRUNC                                            # the site on kz_hi goes
    g.set_blocks(M.LAYER_TSDF, idx[k:k + 1], edit.reshape(1, 512))
    before = H.map_state(g, layers=(M.LAYER_TSDF, M.LAYER_ESDF))
    g.set_params(MC.params(M, case, **case.refuse)[0])
    for _ in range(2):
        with pytest.raises(M.NvbxError, match=r"nvbx error -1: esdf slice z band must span 1\.\.63 blocks"):
            g.update_esdf()
    H.assert_same_map(before, g, (name, "the refused update changed the map"))
    g.set_params(p)
    g.update_esdf()
    edited = case._replace(steps=case.steps + [(idx[k:k + 1], edit.reshape(1, 512))])
    exp = MC.expectations(edited, p)[1]
    assert exp.site.sum() == 1
    MC.assert_expected((name, "after"), *_read(M, g), p, q, exp, 2)
    g.close()


def _drive(M, g, carrier):
    """update_esdf with the marking pass carried by `carrier`; returns the launches of the profile (reading it carries held-back work out)"""
    g.set_profiling(True)
    d, rgb, T = _far_frame(0)
    if carrier == "mark":
        g.update_esdf()
    elif carrier == "color":
        g.integrate_color(rgb, T, FAR_CAM); g.update_esdf()
    elif carrier == "held":
        g.integrate_color(rgb, T, FAR_CAM); g.update_esdf()
    else:
        g.integrate_depth(d, T, FAR_CAM); g.integrate_color(rgb, T, FAR_CAM); g.update_esdf()
        d1, _, T1 = _far_frame(1); g.integrate_depth(d1, T1, FAR_CAM)
    k = _kernels(g)
    g.set_profiling(False)
    return k


def _assert_carrier(tag, carrier, k):
    n = lambda name: k.get(name, 0)                                                        # noqa: E731
    if carrier == "mark":
        assert n("k_esdf_mark") == 1 and not {"k_mark_view", "k_integrate_color", "k_integrate_tsdf_color", "k_sphere_trace"} & set(k), (tag, k)
    elif carrier == "color":
        assert n("k_esdf_mark") == 0 and n("k_integrate_color") == 1 and n("k_esdf_edt") == 1 and not {"k_mark_view", "k_integrate_tsdf_color"} & set(k), (tag, k)
    elif carrier == "held":
        assert n("k_esdf_mark") == 0 and n("k_esdf_edt") == 0 and n("k_sphere_trace") == 1 and n("k_integrate_color") == 1 and not {"k_mark_view", "k_integrate_tsdf_color"} & set(k), (tag, k)
    else:
        assert n("k_esdf_mark") == 0 and n("k_esdf_edt") == 0 and n("k_mark_view") == 2 and n("k_integrate_tsdf_color") == 1 and n("k_integrate_color") == 0, (tag, k)


@pytest.mark.parametrize("name", MC.CARRIER_CASES)
def test_same_marks_from_all_four_carriers(hip_lib, name):
    """The marking pass of the same drawn blocks carried by each of the four launches that can carry it (module docstring), each asserted from the
    launch profile: over the drawn box the layer equals the model -- block set, marks, distances, parents -- and the `mark` run's in every field."""
    M = _M()
    case = MC.case_by_name(M, name)
    assert len(case.steps) == 1 and case.layer == "tsdf" and case.dims == 2
    p, q = MC.params(M, case)
    exp = MC.expectations(case, p)[0]
    idx, data = case.steps[0]
    fields = {}
    for carrier in CARRIERS:
        tag = (name, carrier)
        g = M.Mapper(p, block_capacity=case.capacity)
        g.set_color_deferral(carrier in ("held", "view"))
        g.set_blocks(M.LAYER_TSDF, idx, data)
        _assert_carrier(tag, carrier, _drive(M, g, carrier))
        gi, gb = _read(M, g)
        assert g.counters()["capacity_overflow"] == 0, tag
        fields[carrier] = MC.assert_expected(tag, gi, gb, p, q, exp, 2, whole_layer=carrier != "view")
        if carrier == "view":
            assert g.num_blocks(M.LAYER_TSDF) > len(idx), (tag, "the far frames' own blocks are in the map")
        g.close()
    for carrier in CARRIERS[1:]:
        for a, b, what in zip(fields["mark"], fields[carrier], EI.Fields._fields):
            assert np.array_equal(a, b), (name, carrier, what, "differs from the stand-alone launch's")
