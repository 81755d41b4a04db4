"""Every lanes-per-ray instantiation of the render / ray-cast kernel (render.hip: 8, 4, 2 or 1 lanes march one ray and share its epilogue).
The library picks by ray count -- 8 below 57 600 rays, 4 below 115 200, 2 above -- and NVBX_RENDER_LANES forces a value, read when a mapper is
created: tests/render_lanes_child.py renders the same cases under each setting in a process of its own.  Each setting's results are held
against the colour frame's synthetic depth, the independent model, the colour layer and the point query's gradient, and all settings
against each other bit for bit.  The unforced child covers the by-count choice on a 320 x 240 view (4 lanes) and 134 400 rays (2 lanes);
the 1-lane child also casts more rays than the capped grid holds, so the ray list's grid-stride loop repeats."""
import os
import subprocess
import sys

import numpy as np
import pytest

import render_cases as RC
import render_independent as R
import render_lanes_child as CH

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = ("0", "8", "4", "2", "1")       # 0 = unforced: the by-count choice


@pytest.fixture(scope="module")
def runs(hip_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("lanes")
    procs = {}
    for s in SETTINGS:                      # five small processes side by side
        procs[s] = subprocess.Popen([sys.executable, os.path.join(HERE, "render_lanes_child.py"), str(d / ("l%s.npz" % s))],
                                    env=dict(os.environ, NVBX_RENDER_LANES=s), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for s, p in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (s, log[-3000:])
        out[s] = dict(np.load(d / ("l%s.npz" % s)))
    return out


@pytest.fixture(scope="module")
def model(hip_lib):
    """the independent model's answers for the children's cases, from a map built in this process by the same calls"""
    from isaac_ros_nvblox_amd import mapper as M
    m = M.Mapper(M.default_params(), block_capacity=1 << 13)
    for d, rgb, T in RC.map_frames():
        m.integrate_depth(d, T, RC.CAM); m.integrate_color(rgb, T, RC.CAM)
    m.synchronize()
    tv = RC.product_volume(m, M.LAYER_TSDF, RC.TSDF_FIELDS); cv = RC.product_volume(m, M.LAYER_COLOR, RC.COLOR_FIELDS)
    mp = RC.march_params(m.params)
    out = {}
    for name, cam, pose in (("big", CH.BIG_CAM, "off30"), ("rays", RC.CAM, "off30")):
        o, d, dcz, shape = R.view_rays(RC.NOVEL_POSES[pose], cam, 1)
        t, hit = R.cast(tv, o, d, **mp)
        out[name] = dict(o=o, d=d, dcz=dcz, shape=shape, t=t, hit=hit, tsdf=tv, color=cv, vs=mp["voxel_size"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", SETTINGS)
def test_each_lane_count_against_the_references(runs, model, lanes):
    r = runs[lanes]
    # the colour frame's own synthetic depth
    assert np.array_equal(r["same_pose"], r["synthetic"]) and (r["synthetic"] > 0).mean() > 0.3
    # views against the model's depth; misses are black, normals are unit or zero
    for name in ("view", "big"):
        mo = model["rays" if name == "view" else name]
        depth = r[name + "_depth"]; hit = depth.reshape(-1) > 0
        assert depth.shape == mo["shape"] and np.array_equal(hit, mo["hit"]), (name, int((hit != mo["hit"]).sum()))
        diff = float(np.abs(depth.reshape(-1) - np.where(mo["hit"], mo["t"] * mo["dcz"], 0)).max())
        print("lanes %s %s: max |depth - model| = %g, %d hits" % (lanes, name, diff, int(hit.sum())))
        assert diff <= 1e-4 and hit.mean() > 0.3, diff
        col = r[name + "_color"].reshape(-1, 3); nr = r[name + "_normal"].reshape(-1, 3)
        assert (col[~hit] == 0).all() and (nr[~hit] == 0).all()
        ln = np.linalg.norm(nr[hit].astype(np.float64), axis=1)
        assert np.all((np.abs(ln - 1) <= 1e-6) | (ln == 0)) and (ln > 0).mean() > 0.9
    # the ray list: t, hit against the model; colour against the colour layer; normals against the normalised query gradient
    mo = model["rays"]
    t, hit, col, nr = r["rays_t"], r["rays_hit"], r["rays_color"], r["rays_normal"]
    assert np.array_equal(hit, mo["hit"]) and float(np.abs(t - mo["t"]).max()) <= 1e-4
    assert np.array_equal(col, R.colors(mo["color"], mo["o"], mo["d"], t, hit, mo["vs"]))
    assert (col[hit] != 127).any() and (col[~hit] == 0).all()
    g = r["query_grad"].astype(np.float64); ln = np.linalg.norm(g, axis=1)
    use = hit & r["query_valid"] & (ln > 0)
    assert use.sum() > 5000
    err = float(np.abs(nr[use] - g[use] / ln[use, None]).max())
    print("lanes %s: max |normal - g / |g|| = %g over %d hits" % (lanes, err, int(use.sum())))
    assert err <= 1e-6 and (nr[~use] == 0).all(), err
    # the view of those rays: one march, one epilogue
    assert np.array_equal(r["view_color"].reshape(-1, 3), col) and np.array_equal(r["view_normal"].reshape(-1, 3), nr)
    assert np.array_equal(r["view_depth"].reshape(-1), (t * mo["dcz"]).astype(np.float32))
    # the same rays seven times over (134 400: two lanes per ray when unforced) give the same answers seven times
    for k in ("t", "hit", "color", "normal"):
        assert np.array_equal(r["tiled_" + k], np.tile(r["rays_" + k], (CH.TILES,) + (1,) * (r["rays_" + k].ndim - 1))), k


@pytest.mark.gpu
def test_lane_counts_agree_bit_for_bit(runs):
    base = runs["8"]
    for s in SETTINGS:
        for k in base:
            assert runs[s][k].tobytes() == base[k].tobytes(), (s, k)


@pytest.mark.gpu
def test_ray_list_grid_stride_repeats(runs):
    r = runs["1"]
    assert int(r["stride_rays"]) > CH.STRIDE_WORKGROUPS * 256            # more rays than the capped grid holds at one lane per ray
    assert r["stride_equal"].all(), r["stride_equal"]
