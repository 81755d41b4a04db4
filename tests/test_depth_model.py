"""The checker's camera depth fusion against the float64 model (tests/tsdf_independent.py update_block_rules, tests/view_independent.py) on the drawn
frames of tests/depth_cases.py -- CPU only.  Per case: the same blocks, every robust voxel within 2e-5, every exact voxel decided alike (and, where the
rule leaves the voxel alone or only scales its weight, equal in every bit); the exactness claim of the case module itself (float32 and float64
evaluation of geometry, weights, measured depth and sdf are EQUAL on the exact voxels); every voxel a case was drawn for is there; the view two-sided
against the float64 ray geometry.  tests/test_gpu_depth_drawn.py holds the product against the same model."""
import numpy as np
import pytest

import depth_cases as DC
import helpers as H
import tsdf_independent as TI
import view_independent as V
from isaac_ros_nvblox_amd import mapper as M

F = np.float32
NAMES = [c.name for c in DC.CASES]


def check_values(case, p, got, model, robust, exact, before, report, tol, tag):
    """got / before: {block: voxels [512] of {distance, weight}} after / before the last frame (before = None: no bit-exact expectations);
    -> (voxels compared, exact voxels, voxels of blocks in view)"""
    assert set(got) == set(model), (tag, sorted(set(got) ^ set(model))[:5])
    n_cmp = n_exact = n_all = 0
    for key in sorted(robust):
        ed, ew = model[key]; rob = robust[key]; b = got[key]
        wtol = tol * max(1.0, float(np.max(ew)))
        dd = np.abs(b["distance"].astype(np.float64) - ed); dw = np.abs(b["weight"].astype(np.float64) - ew)
        assert not np.isnan(b["distance"]).any() and not np.isnan(b["weight"]).any(), (tag, key)
        assert dd[rob].max(initial=0.0) <= tol, (tag, key, "distance", int(np.argmax(np.where(rob, dd, 0))), float(dd[rob].max()))
        assert dw[rob].max(initial=0.0) <= wtol, (tag, key, "weight", int(np.argmax(np.where(rob, dw, 0))), float(dw[rob].max()))
        n_cmp += int(rob.sum()); n_exact += int(exact[key].sum()); n_all += 512
    if before is None:
        return n_cmp, n_exact, n_all
    # the last frame, exact voxels: left alone -> the bytes of before; weight decayed / first observation under constant weighting -> the exact value
    keys = [tuple(k) for k in report.block[::512].tolist()]
    zero = np.zeros(512, DC.TSDF_DT)
    prev = np.concatenate([before.get(k, zero) for k in keys]); now = np.concatenate([got[k] for k in keys])
    ex = report.exact
    decays = float(p.invalid_depth_decay_factor) >= 0.0 and int(p.projective_layer_type) == 0
    alone = ex & ((report.rule == TI.OUTSIDE) | (report.rule == TI.REJECTED) | ((report.rule == TI.INVALID) & (not decays)))
    assert np.array_equal(now[alone].view(np.uint64), prev[alone].view(np.uint64)), (tag, "a voxel the rules leave alone changed", int((now[alone] != prev[alone]).sum()))
    touched = ex & ~alone
    if int(p.projective_layer_type) == 0:
        assert (now["weight"][touched & (report.rule == TI.FUSED)] > 0).all(), tag
        dec = touched & (report.rule == TI.INVALID)
        assert np.array_equal(now["weight"][dec], prev["weight"][dec] * F(p.invalid_depth_decay_factor)) and np.array_equal(now["distance"][dec].view(np.uint32), prev["distance"][dec].view(np.uint32)), tag
        first = touched & (report.rule == TI.FUSED) & (report.prev_w == 0) & (int(p.weighting_mode) == 0)
        want = np.clip(report.ds - report.z, -float(p.truncation_distance_vox) * float(p.voxel_size), float(p.truncation_distance_vox) * float(p.voxel_size)).astype(F)
        assert np.array_equal(now["distance"][first], want[first]) and (now["weight"][first] == min(1.0, float(p.max_weight))).all(), tag
    return n_cmp, n_exact, n_all


def check_view(case, p, frames, views, tag):
    for (image, T), view in zip(frames, views):
        org, ends = V.camera_rays(DC.as_metres(image), T, case.cam, float(p.voxel_size), float(p.truncation_distance_vox), float(p.max_integration_distance_m),
                                  int(p.raycast_subsampling_factor))
        bs = float(p.voxel_size) * 8.0
        must = V.blocks_crossed(org, ends, bs, 1e-3)
        assert len(must) > 0 and must <= view, (tag, sorted(must - view)[:5])
        extra = sorted(view - V.blocks_crossed(org, ends, bs, 0.0))
        assert all(V.near_some_ray(extra, org, ends, bs, 1e-3)), (tag, extra[:5])
        if case.family == "range":         # no block beyond the one that holds the cut end point (identity rotation: depth is z)
            assert max(k[2] for k in view) == int(np.floor(ends[:, 2].max() / bs)), tag


def check_targets(case, report):
    for label, (mask, want) in case.targets.items():
        n = int(np.asarray(mask(report)).sum())
        assert (n > 0) if want == "some" else (n == 0), (case.name, label, want, n)


def float32_evaluation(key, image, T, cam, vs, nearest):
    """geometry, bilinear weights, measured depth and sdf of a block's voxels in float32, one rounding per operation"""
    vs = F(vs); bs = F(8.0) * vs
    lin = np.arange(512); vi = [(lin // 64).astype(F), ((lin // 8) % 8).astype(F), (lin % 8).astype(F)]
    pl = [(F(key[a]) * bs + vi[a] * vs) + vs * F(0.5) for a in range(3)]
    T = np.asarray(T, F); d = [pl[a] - T[a, 3] for a in range(3)]
    pc = [(T[0, a] * d[0] + T[1, a] * d[1]) + T[2, a] * d[2] for a in range(3)]
    z = pc[2]; zs = np.where(z > 0, z, F(1.0))
    u = F(cam[0]) * (pc[0] / zs) + F(cam[2]); v = F(cam[1]) * (pc[1] / zs) + F(cam[3])
    img = DC.as_metres(image); rows, cols = img.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if nearest:
            c = np.clip(np.floor(u), 0, cols - 1).astype(np.int64); r = np.clip(np.floor(v), 0, rows - 1).astype(np.int64)
            ds = img[r, c]; ax = ay = np.zeros(512, F)
        else:
            uc, vc = u - F(0.5), v - F(0.5); fx, fy = np.floor(uc), np.floor(vc)
            ax, ay = uc - fx, vc - fy
            x0 = np.clip(fx, 0, max(cols - 2, 0)).astype(np.int64); y0 = np.clip(fy, 0, max(rows - 2, 0)).astype(np.int64)
            x1 = np.minimum(x0 + 1, cols - 1); y1 = np.minimum(y0 + 1, rows - 1)
            top = (F(1.0) - ax) * img[y0, x0] + ax * img[y0, x1]; bot = (F(1.0) - ax) * img[y1, x0] + ax * img[y1, x1]
            ds = (F(1.0) - ay) * top + ay * bot
        sdf = ds - z
    assert all(a.dtype == F for a in (u, v, z, ax, ay, ds, sdf))
    return z, u, v, ax, ay, ds, sdf


def check_exactness(case, p, frames, exact):
    """on the exact voxels the float32 evaluation equals the float64 one: camera depth, pixel coordinates, weights and -- where all four taps are valid -- the
    measured depth and the sdf"""
    n = 0
    nearest = int(p.depth_interp_nearest)
    for image, T in frames:
        for key, ex in exact.items():
            if not ex.any():
                continue
            z32, u32, v32, ax32, ay32, ds32, sdf32 = float32_evaluation(key, image, T, case.cam, p.voxel_size, nearest)
            pc, u, v = TI.voxel_geometry(key, T, case.cam, float(p.voxel_size))
            inside, taps, ds, _ = TI.sample_depth(DC.as_metres(image), u, v, nearest)
            front = ex & (pc[:, 2] > 0)
            assert np.array_equal(z32[ex].astype(np.float64), pc[ex, 2]), (case.name, key)
            assert np.array_equal(u32[front].astype(np.float64), u[front]) and np.array_equal(v32[front].astype(np.float64), v[front]), (case.name, key)
            if not nearest:
                assert np.array_equal(ax32[front].astype(np.float64), ((u - 0.5) - np.floor(u - 0.5))[front]) and np.array_equal(ay32[front].astype(np.float64), ((v - 0.5) - np.floor(v - 0.5))[front])
            m = front & inside & TI.tap_valid(taps).all(0)
            assert np.array_equal(ds32[m].astype(np.float64), ds[m]) and np.array_equal(sdf32[m].astype(np.float64), (ds - pc[:, 2])[m]), (case.name, key)
            n += int(front.sum())
    return n


def checker_against_model(oracle_mod, case, frames, tag):
    p = DC.params(M, case)
    o, views, before = DC.run_checker(oracle_mod, H, case, p, frames)
    model, robust, exact, report = DC.run_model(case, p, frames, views)
    got = DC.checker_map(oracle_mod, o)
    return p, views, model, robust, exact, report, check_values(case, p, got, model, robust, exact, before, report, 2e-5, tag)


@pytest.mark.parametrize("name", NAMES)
def test_checker_against_the_model_on_drawn_frames(oracle_mod, name):
    case = DC.BY_NAME[name]
    frames = DC.frames_of(case)
    p, views, model, robust, exact, report, (n_cmp, n_exact, n_all) = checker_against_model(oracle_mod, case, frames, name)
    check_view(case, p, frames, views, name)
    check_targets(case, report)
    n_proven = check_exactness(case, p, frames, exact)
    if case.exact_depths:
        assert n_exact > 0 and n_proven > 0, (name, n_exact, n_proven)
    if case.family == "oblique":          # the margins may leave out at most 15 % of the voxels of the blocks in view
        assert n_all - n_cmp <= 0.15 * n_all, (name, n_cmp, n_all)
    if case.family == "tap-values":       # no voxel that was observed free, and no tap of which measures a surface in front of it, ends with a negative distance
        free = DC.stays_free(report)
        assert free.sum() > 1000 and not (report.new_d[free] < 0).any(), (name, int((report.new_d[free] < 0).sum()))
    print("depth-model %s family %s: %d voxels compared, %d exact, %d in view (%.1f %% left out)" % (name, case.family, n_cmp, n_exact, n_all, 100.0 * (n_all - n_cmp) / n_all))


@pytest.mark.parametrize("name", [c.name for c in DC.CASES if c.family in ("border", "step", "prior", "oblique", "occupancy", "u16")])
def test_checker_against_the_model_with_a_second_frame_from_another_pose(oracle_mod, name):
    """the frames of the batch-of-two launch (tests/test_gpu_depth_drawn.py), applied in order"""
    case = DC.BY_NAME[name]
    frames = DC.frames_of(case)[-1:] + [DC.batch_partner(case)]
    checker_against_model(oracle_mod, case, frames, name + " + partner")


def test_both_instantiations_and_every_family_occur():
    plain = [DC.is_plain(c.kw) for c in DC.CASES]
    assert any(plain) and not all(plain)
    assert DC.FAMILIES == sorted(["border", "centre-taps", "tap-values", "range", "behind", "sdf-thresholds", "prior", "step", "tiny", "single-ray", "oblique",
                                  "occupancy", "u16"])
    for c in DC.CASES:
        assert c.capacity <= 1 << 12 and all(d.shape[0] <= 48 and d.shape[1] <= 64 for d in c.depths)
