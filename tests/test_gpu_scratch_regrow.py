"""ONE mapper taken through reallocations of its image-sized scratch buffers (dilated depth, synthetic depth, the mask split's nearest-depth
image, the connected-component and dynamic-split arrays): frames at 80x60, 160x120, 320x240 and 80x60 again -- every buffer grows twice on a
buffer that is in use, then serves an image that fits into what it has -- against the CPU oracle fed the same frames.

Bars: the parity suite's (tests/test_gpu_parity.py, smoke()): equal TSDF block index sets, TSDF distance / weight and the ESDF slice within 1e-4;
masks and split depth images bit for bit; colour equal.
"""
import numpy as np
import pytest

import helpers as H
from isaac_ros_nvblox_amd import synthetic as S

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [(60, 80), (120, 160), (240, 320), (60, 80)]          # (rows, cols): grow, grow, grow, fits


def cam_of(rows, cols):
    """90 degree horizontal field of view at every size (helpers.SMALL_CAM at 160x120)."""
    return (cols / 2.0, cols / 2.0, cols / 2.0 - 0.5, rows / 2.0 - 0.5, cols, rows)


def test_image_scratch_regrows_under_one_mapper(oracle_mod, hip_lib):
    from isaac_ros_nvblox_amd import mapper as M
    pg = M.default_params(do_depth_preprocessing=1, depth_preprocessing_num_dilations=1)
    g = M.Mapper(pg, block_capacity=1 << 14); o = oracle_mod.OracleMap(H.copy_params(pg, oracle_mod.OrcParams))
    sc = S.Scene()
    rng = np.random.default_rng(7)
    T_CM_CD = np.eye(4, dtype=np.float32); T_CM_CD[0, 3] = 0.06; T_CM_CD[1, 3] = -0.01      # (the mask camera of test_mask_split_and_human_mapping_parity)
    for k, (rows, cols) in enumerate(SIZES):
        cam = cam_of(rows, cols)
        for j in range(2):
            T = S.trajectory_pose((2 * k + j) * 7, 200)
            d, rgb = S.render(sc, T, cam)
            d = d.copy(); d[rows // 6:rows // 3, cols // 3:cols // 2] = 0.0                  # an invalid region for the dilation to widen
            g.integrate_depth(d, T, cam); o.integrate_depth(d, T, cam)
            assert H.idx_set(g.last_view()) == H.idx_set(o.last_view()), (rows, cols, j)
            g.integrate_color(rgb, T, cam); o.integrate_color(rgb, T, cam)
            sg, so = g.synthetic_depth(), o.synthetic_depth()
            assert sg.shape == so.shape and np.abs(sg - so).max() <= TOL, (rows, cols, j)
            g.update_esdf(); o.update_esdf()
            mask = (rng.random((rows, cols)) < 0.42).astype(np.uint8)                        # the percolation threshold: components of every size
            thr = max(4, rows * cols // 480)
            cg = g.remove_small_components(mask, thr).cpu().numpy(); co = oracle_mod.remove_small_components(mask, thr)
            assert np.array_equal(cg, co) and 0 < co.sum() < mask.sum(), (rows, cols, j)
            un_g, ma_g = g.split_depth_by_mask(d, co, T_CM_CD, cam, cam, 0.25)
            un_o, ma_o = oracle_mod.split_depth_by_mask(d, co, T_CM_CD, cam, cam, 0.25)
            assert np.array_equal(un_g.cpu().numpy(), un_o) and np.array_equal(ma_g.cpu().numpy(), ma_o), (rows, cols, j)
            assert (ma_o > 0).any() and (un_o > 0).any()
    ig = g.block_indices(M.LAYER_TSDF); io = o.block_indices(oracle_mod.L_TSDF)
    assert H.idx_set(ig) == H.idx_set(io) and np.array_equal(ig, io) and len(io) > 100
    bg, found = g.get_blocks(M.LAYER_TSDF, ig)
    assert found.all()
    worst = 0.0
    for n, idx in enumerate(io):
        bo = o.get_block(oracle_mod.L_TSDF, idx)
        worst = max(worst, float(np.abs(bg[n]["distance"] - bo["distance"]).max()), float(np.abs(bg[n]["weight"] - bo["weight"]).max()))
    print("max |tsdf diff| %.3g over %d blocks" % (worst, len(io)))
    assert worst <= TOL
    ic = g.block_indices(M.LAYER_COLOR); ioc = o.block_indices(oracle_mod.L_COLOR)
    assert np.array_equal(ic, ioc) and len(ioc) > 20
    cg_, found = g.get_blocks(M.LAYER_COLOR, ic)
    assert found.all()
    worst_c = 0; worst_w = 0.0
    for n, idx in enumerate(ioc):
        bo = o.get_block(oracle_mod.L_COLOR, idx)
        worst_c = max(worst_c, max(int(np.abs(cg_[n][f].astype(np.int32) - bo[f].astype(np.int32)).max()) for f in ("r", "g", "b")))
        worst_w = max(worst_w, float(np.abs(cg_[n]["weight"] - bo["weight"]).max()))
    print("max colour diff %d LSB, max |colour weight diff| %.3g over %d blocks" % (worst_c, worst_w, len(ioc)))
    assert worst_c == 0 and worst_w <= TOL
    sg, ag = g.esdf_slice_image(); so, ao = o.esdf_slice_image()
    assert sg.shape == so.shape and np.array_equal(ag, ao)
    print("max |esdf slice diff| %.3g, slice %s" % (float(np.abs(sg - so).max()), sg.shape))
    assert np.abs(sg - so).max() <= TOL
    assert g.counters()["capacity_overflow"] == 0


def test_dynamic_split_scratch_regrows_under_one_mapper(oracle_mod, hip_lib):
    """nvbx_dynamic_depth_split on one dynamic-mapping mapper at the four sizes against the three separate calls on a second mapper and against
    the checker, bit for bit (tests/test_gpu_round4.py does this at one size): the static room for 0.8 s at the first two sizes (free voxels become
    high-confidence freespace), then a box in mid-room at the last two."""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    dev = torch.device("cuda", 0)
    fs = dict(projective_layer_type=2, max_integration_distance_m=5.0, invalid_depth_decay_factor=0.8, min_duration_since_occupied_for_freespace_ms=250)
    pg = M.default_params(**fs)
    a = M.Mapper(pg, block_capacity=1 << 14); b = M.Mapper(pg, block_capacity=1 << 14); o = oracle_mod.OracleMap(H.copy_params(pg, oracle_mod.OrcParams))
    eye = np.eye(4, dtype=np.float32)
    static_scene = S.Scene(); moving = S.Scene(box_min=(1.6, -0.3, 0.0), box_max=(2.0, 0.3, 1.3))      # (the scenes of test_dynamic_mapping_parity)
    n_dynamic = 0
    for i in range(16):
        rows, cols = SIZES[i // 4]
        cam = cam_of(rows, cols)
        sc = static_scene if i < 8 else moving
        T = S.trajectory_pose(min(i, 8), 200)
        d, _ = S.render(sc, T, cam, max_range=5.0, color=False)
        d_dev = torch.from_numpy(d).to(dev)
        thr = max(4, rows * cols // 480) if i % 4 != 1 else 0     # (40 at 160x120, as there; one frame per size with the filter off)
        mk_a = torch.empty((rows, cols), dtype=torch.uint8, device=dev); un_a = torch.empty((rows, cols), dtype=torch.float32, device=dev); ma_a = torch.empty_like(un_a)
        a.detect_dynamics_into(d_dev, T, cam, 5.0, mk_a)
        if thr:
            a.remove_small_components_inplace(mk_a, thr)
        a.split_depth_by_mask_into(d_dev, mk_a, eye, cam, cam, 0.25, un_a, ma_a)
        mk_b = torch.empty_like(mk_a); un_b = torch.empty_like(un_a); ma_b = torch.empty_like(un_a)
        b.dynamic_depth_split_into(d_dev, T, cam, 5.0, thr, 0.25, mk_b, un_b, ma_b)
        a.synchronize(); b.synchronize()            # (each mapper owns its stream; the comparisons run on torch's)
        assert torch.equal(mk_a, mk_b) and torch.equal(un_a, un_b) and torch.equal(ma_a, ma_b), i
        mo = o.detect_dynamics(d, T, cam, 5.0)
        if thr:
            mo = oracle_mod.remove_small_components(mo, thr)
        uo, mao = oracle_mod.split_depth_by_mask(d, mo, eye, cam, cam, 0.25)
        assert np.array_equal(mk_b.cpu().numpy(), mo) and np.array_equal(un_b.cpu().numpy(), uo) and np.array_equal(ma_b.cpu().numpy(), mao), i
        n_dynamic += int(mo.sum())
        for m_, un_ in ((a, un_a), (b, un_b)):
            m_.set_time_ms(i * 100); m_.integrate_depth(un_, T, cam)
        o.set_time_ms(i * 100); o.integrate_depth(uo, T, cam)
    assert n_dynamic > 0, n_dynamic                 # the box was detected: the masks compared above were not all empty
