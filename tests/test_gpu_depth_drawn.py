"""The camera depth frame of the PRODUCT on the drawn frames of tests/depth_cases.py, against the float64 model (tests/tsdf_independent.py
update_block_rules) and against the checker.  Every case runs on a fresh mapper through a single integrate_depth call per frame (the u16 family through
the u16 entry point) and, its last frame together with a second drawn frame from another pose, through one batch launch held against the model applied
in order.  Checked with nothing sampled: the view and the block set equal the checker's; every robust voxel within 1.2e-4 of the model (the contract's
1e-4 to the checker + the checker's 2e-5 to the model); every exact voxel decided as the model decides, and equal in every bit where the expected value
is itself exact (left alone, weight decayed, first observation under constant weighting); every voxel within helpers.TOL of the checker; nothing
non-finite; pre-filled blocks outside the view byte-identical to what was written; no capacity overflow; and for the tap-values family: no voxel that
was observed free, and in front of which no tap measures a surface, ends with a negative distance.  tests/test_depth_model.py holds the checker against
the same model on the CPU and proves the exactness claim."""
import numpy as np
import pytest

import depth_cases as DC
import helpers as H
import test_depth_model as TM
from isaac_ros_nvblox_amd import mapper as M

pytestmark = pytest.mark.gpu
MODEL_TOL = 1.2e-4
BATCH_NAMES = [c.name for c in DC.CASES]


def product_map(g, layer):
    idx, vox = H.map_state(g, layers=(layer,))["layers"][layer]
    out = {}
    for i, b in zip(idx.tolist(), vox):
        v = np.zeros(512, DC.TSDF_DT)
        if layer == M.LAYER_OCCUPANCY:
            v["distance"] = b["log_odds"]
        else:
            v["distance"] = b["distance"]; v["weight"] = b["weight"]
        out[tuple(i)] = v
    return out


def run(oracle_mod, case, frames, batch, tag):
    p = DC.params(M, case)
    occupancy = int(p.projective_layer_type) == 1
    layer = M.LAYER_OCCUPANCY if occupancy else M.LAYER_TSDF
    o, views, before = DC.run_checker(oracle_mod, H, case, p, frames)
    model, robust, exact, report = DC.run_model(case, p, frames, views)
    g = M.Mapper(p, block_capacity=case.capacity)
    if case.prior is not None:
        idx, vox = case.prior
        if occupancy:
            lo = np.zeros(vox.shape, M.OCCUPANCY_DT); lo["log_odds"] = vox["distance"]
            g.set_blocks(layer, idx, lo)
        else:
            g.set_blocks(layer, idx, vox)
    if batch:
        g.integrate_depth_batch([DC.as_metres(d) for d, _ in frames], [T for _, T in frames], [case.cam] * len(frames))
        assert H.idx_set(g.last_view()) == views[-1], tag          # (a batch reports its last camera's view; the block set below holds every camera's)
    else:
        for k, ((image, T), view) in enumerate(zip(frames, views)):
            if k == len(frames) - 1:
                before = product_map(g, layer)              # (the product's own map before the last frame: what a voxel left alone must still hold)
            g.integrate_depth(image, T, case.cam)
            assert H.idx_set(g.last_view()) == view, tag
    got = product_map(g, layer)
    # the model: robust voxels within the tolerance; exact voxels bit for bit where the expectation is exact (a batch hides the map between its frames)
    n_cmp, n_exact, n_all = TM.check_values(case, p, got, model, robust, exact, None if batch else before, report, MODEL_TOL, tag)
    # the checker: every voxel
    want = DC.checker_map(oracle_mod, o)
    assert set(got) == set(want), tag
    for key, b in got.items():
        c = want[key]
        assert np.isfinite(b["distance"]).all() and np.isfinite(b["weight"]).all(), (tag, key)
        d = max(float(np.abs(b["distance"].astype(np.float64) - c["distance"]).max()), float(np.abs(b["weight"].astype(np.float64) - c["weight"]).max()))
        assert d <= H.TOL, (tag, key, d)
    # pre-filled blocks outside every view: the bytes that were written
    if case.prior is not None:
        seen = set().union(*views)
        outside = [k for k, i in enumerate(case.prior[0].tolist()) if tuple(i) not in seen]
        assert outside, tag
        back = np.stack([got[tuple(case.prior[0][k].tolist())] for k in outside])
        written = case.prior[1][outside].copy()
        if occupancy:
            written["weight"] = 0
        diff = H.block_difference(case.prior[0][outside], back, written)
        assert diff is None, (tag, diff)
    assert g.counters()["capacity_overflow"] == 0, tag
    if case.family == "tap-values" and not batch:
        free = DC.stays_free(report)
        keys = [tuple(k) for k in report.block[::512].tolist()]
        now = np.concatenate([got[k] for k in keys])
        assert free.sum() > 1000 and not (now["distance"][free] < 0).any(), (tag, int((now["distance"][free] < 0).sum()))
    return n_cmp, n_exact, n_all


@pytest.mark.parametrize("name", [c.name for c in DC.CASES])
def test_product_against_the_model_on_drawn_frames(oracle_mod, hip_lib, name):
    case = DC.BY_NAME[name]
    n_cmp, n_exact, n_all = run(oracle_mod, case, DC.frames_of(case), False, name)
    print("depth-drawn %s family %s: %d voxels compared, %d exact, %d in view" % (name, case.family, n_cmp, n_exact, n_all))


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_product_batch_of_two_against_the_model_applied_in_order(oracle_mod, hip_lib, name):
    case = DC.BY_NAME[name]
    run(oracle_mod, case, DC.frames_of(case)[-1:] + [DC.batch_partner(case)], True, name + " batch")
