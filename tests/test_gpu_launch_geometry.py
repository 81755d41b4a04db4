"""Launch grids and A/B switches leave the map bit-identical ("a voxel is updated by exactly one lane per frame ... every consumer is
order-free"; 5.1: no result depends on a knob).  Most launches size their grid from a hint -- a count the GPU last wrote to pinned host memory, not
waited for -- and grid-stride over the real count, so whether the paths a short grid takes (the late record fetch past `spec_lanes`, many blocks per
workgroup, k_decay's rounds of 64 blocks per wave with one workgroup, the marking pass's two-level reset with few workers) run in a test is left to
timing.  Here every NVBX_* knob that moves a grid, a rider count or the launch structure is set to small and odd values, one child process per
setting (tests/launch_geometry_child.py: a mapper reads the knobs at creation; a child also keeps a fault to itself), and every snapshot of the scripted schedule must equal the
default run's byte for byte.  The default run is itself run twice (a difference there is a race) and checked against the CPU checker: every
layer, cleared list, slice and mesh (vertices, normals, colours, triangles) of every snapshot, and the point queries against the float64 query model
(tests/query_independent.py) evaluated on the checker's blocks."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers as H
import launch_geometry_child as LG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
CHILD_TIMEOUT_S = 300
KNOBS = ("NVBX_INTEG_GRID", "NVBX_GRID_MARGIN", "NVBX_COLOR_GRID", "NVBX_EDT_RIDERS", "NVBX_PAIR_B_EDT_RIDERS", "NVBX_MARK_RIDERS",
         "NVBX_MARK_TILES_FIRST", "NVBX_DECAY_GRID", "NVBX_ST_LANES", "NVBX_FUSED_TRACE_LANES", "NVBX_FUSE_COLC", "NVBX_DEPTH_PAIR",
         "NVBX_LIDAR_SPARSE", "NVBX_LIDAR_DENSE_LIST", "NVBX_LIDAR_SPARSE_GRID", "NVBX_DEFER_EDT", "NVBX_COLOR_DEFERRAL", "NVBX_LIB")
SETTINGS = [
    {"NVBX_INTEG_GRID": "8"}, {"NVBX_INTEG_GRID": "13"}, {"NVBX_GRID_MARGIN": "0,0"}, {"NVBX_COLOR_GRID": "8"}, {"NVBX_EDT_RIDERS": "8"},
    {"NVBX_PAIR_B_EDT_RIDERS": "8"}, {"NVBX_MARK_RIDERS": "8"}, {"NVBX_MARK_TILES_FIRST": "0"}, {"NVBX_MARK_TILES_FIRST": "1"},
    {"NVBX_DECAY_GRID": "1"}, {"NVBX_ST_LANES": "1"}, {"NVBX_ST_LANES": "2"}, {"NVBX_ST_LANES": "4"}, {"NVBX_FUSED_TRACE_LANES": "4"},
    {"NVBX_FUSE_COLC": "0"}, {"NVBX_DEPTH_PAIR": "0"}, {"NVBX_LIDAR_SPARSE": "0"}, {"NVBX_LIDAR_DENSE_LIST": "0"}, {"NVBX_LIDAR_SPARSE_GRID": "8"},
    {"NVBX_DEFER_EDT": "0"}, {"NVBX_COLOR_DEFERRAL": "0"}, {"NVBX_COLOR_DEFERRAL": "2"},
    # every grid and rider count at its minimum at once
    {"NVBX_INTEG_GRID": "1", "NVBX_GRID_MARGIN": "0,0", "NVBX_COLOR_GRID": "1", "NVBX_EDT_RIDERS": "8", "NVBX_PAIR_B_EDT_RIDERS": "8",
     "NVBX_MARK_RIDERS": "8", "NVBX_DECAY_GRID": "1", "NVBX_ST_LANES": "1", "NVBX_FUSED_TRACE_LANES": "4", "NVBX_LIDAR_SPARSE_GRID": "1"},
    # values the library must refuse (csrc/nvbx_knobs.h: the default instead)
    {"NVBX_EDT_RIDERS": "0", "NVBX_DECAY_GRID": "0", "NVBX_LIDAR_SPARSE_GRID": "0", "NVBX_INTEG_GRID": "-1"},
    {"NVBX_DECAY_GRID": "-5", "NVBX_LIDAR_SPARSE_GRID": "-3", "NVBX_COLOR_GRID": "0", "NVBX_GRID_MARGIN": "-5,-1", "NVBX_MARK_RIDERS": "-8",
     "NVBX_PAIR_B_EDT_RIDERS": "3", "NVBX_ST_LANES": "3", "NVBX_FUSED_TRACE_LANES": "0"},
]
# structural switches: the launch structure must differ from the default run's (else the switch is not being tested); mapper whose counts show it
STRUCTURAL = {"NVBX_FUSE_COLC": "A", "NVBX_DEPTH_PAIR": "A", "NVBX_LIDAR_SPARSE": "E", "NVBX_DEFER_EDT": "A", "NVBX_COLOR_DEFERRAL": "A"}
VARIANT = os.path.join(ROOT, "isaac_ros_nvblox_amd", "variants", "libnvblox_hip_xcd3.so")
_STATE = {"stopped": None, "times": {}}


def _setting_id(s):
    return ",".join("%s=%s" % (k.replace("NVBX_", ""), v) for k, v in sorted(s.items()))


def _run_child(inp, tag, env_extra):
    """One child, waited for.  The first child that does not finish cleanly -- a signal, the time limit, a non-zero exit (a failed check of the hash
    probe, a device error the library reports) -- stops the file: no later lookup starts a process again, of that setting or any other."""
    if _STATE["stopped"]:
        pytest.fail("not started: an earlier child failed (%s)" % _STATE["stopped"])
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    out = os.path.join(os.path.dirname(inp), "out_%s.npz" % tag.replace("=", "_").replace(",", "_"))
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "launch_geometry_child.py"), inp, out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _STATE["stopped"] = "%s timed out" % tag
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("child %s timed out after %d s:\n%s" % (tag, CHILD_TIMEOUT_S, err[-3000:]))
    _STATE["times"][tag] = time.time() - t0
    print("child %s: %.1f s" % (tag, _STATE["times"][tag]))
    if p.returncode != 0 or "LAUNCH_GEOMETRY_CHILD_OK" not in p.stdout:
        why = ("signal %d" % -p.returncode) if p.returncode < 0 else ("exit status %d" % p.returncode)
        _STATE["stopped"] = "%s: %s" % (tag, why)
        pytest.fail("child %s failed (%s):\n%s\n%s" % (tag, why, p.stdout[-2000:], p.stderr[-4000:]))
    return dict(np.load(out))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_geometry")
    inp = str(d / "inputs.npz")
    np.savez(inp, **LG.render_inputs())
    cache = {}
    t0 = time.time()

    def go(tag, env_extra=None):
        if tag not in cache:
            cache[tag] = _run_child(inp, tag, env_extra or {})
        return cache[tag]
    go.inputs = inp
    yield go
    print("launch geometry: %d children, %.1f s in all" % (len(_STATE["times"]), time.time() - t0))
    for tag, s in _STATE["times"].items():
        print("  %6.1f s  %s" % (s, tag))


LAYER_OF = {name: layer for layer, name in H.LAYER_NAMES.items()}


def _assert_same_maps(base, other, tag):
    keys = sorted(k for k in base if not k.startswith("meta/"))
    assert keys == sorted(k for k in other if not k.startswith("meta/")), (tag, set(keys) ^ set(k for k in other if not k.startswith("meta/")))
    for k in keys:
        a, b = base[k], other[k]
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            phase, mapper, what = k.split("/", 2)
            if what.endswith("/bytes"):                                  # the blocks of a layer, in the order of its "/idx" array
                dt = H.LAYER_FIELDS[LAYER_OF[what.split("/")[0]]]
                diff = H.block_difference(base[k[:-len("bytes")] + "idx"], a.view(dt), b.view(dt))
            else:
                diff = H.array_difference(a, b)
            pytest.fail("%s differs from the default run: phase %s, mapper %s, %s: %s" % (tag, phase, mapper, what, diff))


def _launch_counts(out, mapper):
    """Launch counts of the mapper's profile at its last snapshot."""
    keys = sorted(k for k in out if k.startswith("meta/") and k.endswith("/%s/profile" % mapper))
    return json.loads(out[keys[-1]].tobytes().decode())


def test_the_default_run_is_repeatable(run):
    a = run("default"); b = run("default_again")
    _assert_same_maps(a, b, "the second default run")
    assert json.loads(a["meta/growth_frames"].tobytes()) == json.loads(b["meta/growth_frames"].tobytes())
    # the schedule did what it is there for
    cap = a["meta/4_decay_growth/A/capacity"]
    assert cap[0] == 512 and len(cap) >= 3, cap                          # grew before phase 4 and again inside it
    assert a["meta/c2_decay_growth/C/capacity"][-1] >= 2 * a["meta/c1_frames/C/capacity"][-1]
    for ph, m in (("4_decay_growth", "A"), ("5_clear", "A"), ("c2_decay_growth", "C"), ("d2_decay_clear", "D"), ("e2_decay", "E")):
        assert len(a["%s/%s/cleared" % (ph, m)]) > 0, (ph, m, "nothing was deallocated")
    pa = _launch_counts(a, "A")
    assert any("k_integrate_tsdf_color_pair" in k for k in pa) and any("k_integrate_tsdf_color<" in k for k in pa), sorted(pa)
    assert any("k_lidar_sparse" in k for k in _launch_counts(a, "E")), sorted(_launch_counts(a, "E"))


class Checker:
    """The schedule on the CPU checker: a pair is the two calls, a batch the calls one by one, the growth phase as many frames as the GPU took."""

    def __init__(self, oracle_mod, growth_frames):
        from isaac_ros_nvblox_amd import mapper as M
        self.O, self.M, self.growth = oracle_mod, M, growth_frames
        self.m, self.cleared, self.out, self.queries = {}, {}, {}, {}

    def new(self, name):
        kw, _, _ = LG.MAPPERS[name]
        self.m[name] = self.O.OracleMap(H.copy_params(self.M.default_params(**kw), self.O.OrcParams))
        self.cleared[name] = []

    def depth(self, name, d, T):
        self.m[name].integrate_depth(d, T, LG.CAM)

    def color(self, name, rgb, T):
        self.m[name].integrate_color(rgb, T, LG.CAM)

    def esdf(self, name):
        self.m[name].update_esdf()

    def mesh(self, name):
        self.m[name].update_mesh()

    def sync(self, name):
        pass

    def depth_batch(self, name, ds, Ts):
        for d, T in zip(ds, Ts):
            self.depth(name, d, T)

    def color_batch(self, name, rgbs, Ts):
        for c, T in zip(rgbs, Ts):
            self.color(name, c, T)

    def pair(self, a, da, b, db, T):
        self.depth(a, da, T); self.depth(b, db, T)

    def lidar(self, name, img, T):
        self.m[name].integrate_lidar_depth(img, T, LG.LIDAR)

    def decay(self, name):
        o = self.m[name]
        if o.params.projective_layer_type == 1:
            o.decay_occupancy()
        else:
            o.decay_tsdf(True)

    def take_cleared(self, name):
        self.cleared[name].append(self.m[name].take_cleared_blocks())

    def clear_radius(self, name, c, r):
        self.m[name].clear_outside_radius(c, r)

    def clear_shapes(self, name, shapes):
        self.m[name].clear_tsdf_inside_shapes(shapes)

    def grow(self, name, ds, Ts):
        for k in range(self.growth[name]):
            self.depth(name, ds[k], Ts[k])

    def query(self, name, pts):
        """the float64 model of the point queries (tests/query_independent.py) on the checker's own blocks"""
        import query_independent as QI
        o = self.m[name]; p = o.params
        layer_of = {QI.LAYER_TSDF: self.O.L_TSDF, QI.LAYER_ESDF: self.O.L_ESDF}
        dts = {QI.LAYER_TSDF: self.M.TSDF_DT, QI.LAYER_ESDF: self.M.ESDF_DT}

        def get_blocks(layer, keys):
            out = np.zeros((len(keys), 512), dts[layer]); found = np.zeros(len(keys), bool)
            for k, i in enumerate(keys):
                b = o.get_block(layer_of[layer], i)
                if b is not None:
                    out[k] = b; found[k] = True
            return out, found
        td, tg, tv = QI.query(get_blocks, QI.LAYER_TSDF, pts, p.voxel_size, min_weight=p.mesh_min_weight)
        plane = None if p.esdf_mode == 1 else QI.plane_vz(p.esdf_slice_height, p.voxel_size)
        ed, eg, ev = QI.query(get_blocks, QI.LAYER_ESDF, pts, p.voxel_size, plane=plane)
        self.queries[name] = dict(tsdf_d=td, tsdf_g=tg, tsdf_v=tv, esdf_d=ed, esdf_g=eg, esdf_v=ev)

    def snap(self, phase, names, mesh=False):
        O = self.O
        layer_of = dict(tsdf=O.L_TSDF, color=O.L_COLOR, esdf=O.L_ESDF, occupancy=O.L_TSDF)
        for name in names:
            o = self.m[name]
            key = "%s/%s/" % (phase, name)
            layers = LG.MAPPERS[name][2]
            for lay in layers:
                idx = o.block_indices(layer_of[lay])
                self.out[key + lay + "/idx"] = idx
                self.out[key + lay + "/blocks"] = [o.get_block(layer_of[lay], i) for i in idx]
            c = np.concatenate(self.cleared[name] + [np.zeros((0, 3), np.int32)]).reshape(-1, 3)
            self.out[key + "cleared"] = np.unique(c, axis=0) if len(c) else c
            self.cleared[name] = []
            if "esdf" in layers:
                img, aabb = o.esdf_slice_image()
                self.out[key + "slice/img"] = img; self.out[key + "slice/aabb"] = aabb
            if mesh:
                meshes = {}
                for i in o.block_indices(O.L_TSDF):
                    mb = o.mesh_block(i)
                    if mb is not None and len(mb["triangles"]):
                        meshes[tuple(int(v) for v in i)] = mb
                self.out[key + "mesh"] = meshes
            for f, v in self.queries.pop(name, {}).items():
                self.out[key + "query/" + f] = v


def _compare_with_checker(g, o, key_prefix, name):
    M = LG
    layers = M.MAPPERS[name][2]
    for lay in layers:
        ig, io = g[key_prefix + lay + "/idx"], o[key_prefix + lay + "/idx"]
        assert np.array_equal(ig, io), (key_prefix + lay, "block index sets differ", len(ig), len(io),
                                        sorted(set(map(tuple, ig.tolist())) ^ set(map(tuple, io.tolist())))[:5])
        bg = g[key_prefix + lay + "/bytes"].view(H.LAYER_FIELDS[LAYER_OF[lay]]).reshape(-1, 512)
        for k, bo in enumerate(o[key_prefix + lay + "/blocks"]):
            b = bg[k]; where = (key_prefix + lay, tuple(io[k].tolist()))
            if lay == "tsdf":
                for f in ("distance", "weight"):
                    assert np.abs(b[f].astype(np.float64) - bo[f].astype(np.float64)).max() <= TOL, where + (f,)
            elif lay == "occupancy":
                assert np.array_equal(b["log_odds"], bo["distance"]), where
            elif lay == "color":
                assert np.abs(b["weight"].astype(np.float64) - bo["weight"].astype(np.float64)).max() <= TOL, where + ("weight",)
                for f in ("r", "g", "b"):
                    assert np.abs(b[f].astype(np.int32) - bo[f].astype(np.int32)).max() <= 1, where + (f,)
            else:
                for f in H.ESDF_FIELDS:
                    assert np.array_equal(b[f], bo[f]), where + (f,)
    assert np.array_equal(g[key_prefix + "cleared"], o[key_prefix + "cleared"]), (key_prefix, "cleared blocks differ",
                                                                                   len(g[key_prefix + "cleared"]), len(o[key_prefix + "cleared"]))
    if "esdf" in layers:
        sg, so = g[key_prefix + "slice/img"], o[key_prefix + "slice/img"]
        assert sg.shape == so.shape and np.abs(sg - so).max() <= TOL, (key_prefix, "slice")
        assert np.allclose(g[key_prefix + "slice/aabb"], o[key_prefix + "slice/aabb"]), (key_prefix, "slice aabb")
    if key_prefix + "mesh/idx" in g:
        mo = o[key_prefix + "mesh"]
        keys = [tuple(int(v) for v in i) for i in g[key_prefix + "mesh/idx"]]
        # (Mapper.mesh() holds the blocks the LAST update re-meshed; the checker keeps every block's mesh: equal sets on the map's first mesh update)
        only_g = sorted(set(keys) - set(mo))
        assert not only_g, (key_prefix, "mesh blocks the checker does not have", only_g[:5], len(only_g))
        if key_prefix.startswith("3_batch/"):
            assert keys == sorted(mo), (key_prefix, "mesh blocks only on the checker", sorted(set(mo) - set(keys))[:5])
        nv = np.concatenate([[0], np.cumsum(g[key_prefix + "mesh/nv"])]); nt = np.concatenate([[0], np.cumsum(g[key_prefix + "mesh/nt"])])
        for j, k in enumerate(keys):
            v = g[key_prefix + "mesh/vertices"][nv[j]:nv[j + 1]]; t = g[key_prefix + "mesh/triangles"][nt[j]:nt[j + 1]]
            c = g[key_prefix + "mesh/colors"][nv[j]:nv[j + 1]]; nm = g[key_prefix + "mesh/normals"][nv[j]:nv[j + 1]]
            assert np.array_equal(t, mo[k]["triangles"]), (key_prefix, k, "triangles")
            assert v.shape == mo[k]["vertices"].shape and np.abs(v - mo[k]["vertices"]).max() <= TOL, (key_prefix, k, "vertices")
            assert np.abs(nm - mo[k]["normals"]).max() <= 1e-3, (key_prefix, k, "normals")
            assert np.abs(c.astype(int) - mo[k]["colors"].astype(int)).max() <= 1, (key_prefix, k, "colours")
    # point queries against the float64 model on the checker's blocks: validity exact; the TSDF within the layer's 1e-4 (its gradient, a difference
    # of two corners over the voxel size, within 2 * 1e-4 / vs), the ESDF (an exact layer) as tests/test_gpu_query.py holds it
    if key_prefix + "query/tsdf_d" in g:
        vs = float(np.float32(LG.MAPPERS[name][0].get("voxel_size", 0.05)))
        for kind, dtol, gtol in (("tsdf", TOL + 1e-5, 2 * TOL / vs + 1e-4), ("esdf", 1e-5, 1e-4)):
            vg, vo = g[key_prefix + "query/%s_v" % kind].astype(bool), o[key_prefix + "query/%s_v" % kind]
            assert np.array_equal(vg, vo), (key_prefix, kind, "validity differs at", np.nonzero(vg != vo)[0][:5])
            assert vo.sum() > 100, (key_prefix, kind, "too few valid points", int(vo.sum()))
            dd = np.abs(g[key_prefix + "query/%s_d" % kind] - o[key_prefix + "query/%s_d" % kind]).max()
            dg = np.abs(g[key_prefix + "query/%s_g" % kind] - o[key_prefix + "query/%s_g" % kind]).max()
            assert dd <= dtol and dg <= gtol, (key_prefix, kind, "distance / gradient off the model by", dd, dg)


def test_the_default_run_meets_the_checker(run, oracle_mod):
    g = run("default")
    growth = json.loads(g["meta/growth_frames"].tobytes())
    C = Checker(oracle_mod, growth)
    LG.schedule(C, dict(np.load(run.inputs)))
    prefixes = sorted({"/".join(k.split("/")[:2]) + "/" for k in g if not k.startswith("meta/")})
    assert len(prefixes) >= 14, prefixes
    assert "7_query/A/query/tsdf_d" in g and "7_query/A/query/tsdf_d" in C.out
    for p in prefixes:
        _compare_with_checker(g, C.out, p, p.split("/")[1])


@pytest.mark.parametrize("setting", SETTINGS, ids=[_setting_id(s) for s in SETTINGS])
def test_a_knob_setting_leaves_every_snapshot_bit_identical(run, setting):
    base = run("default")
    tag = _setting_id(setting)
    out = run(tag, setting)
    _assert_same_maps(base, out, tag)
    if len(setting) == 1:
        (knob, value), = setting.items()
        if knob in STRUCTURAL and not (knob == "NVBX_COLOR_DEFERRAL" and value == "2"):      # (2 = the default form)
            m = STRUCTURAL[knob]
            assert _launch_counts(out, m) != _launch_counts(base, m), (tag, "the launch structure did not change", _launch_counts(out, m))


def _xcd3_variant():
    srcs = [os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")) if f.endswith((".hip", ".h", ".inc"))]
    if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), "xcd3", "-DNVBX_XCD_CHUNK=3"], stdout=subprocess.DEVNULL)
    return VARIANT


def test_the_xcd_run_length_leaves_every_snapshot_bit_identical(run):
    """-DNVBX_XCD_CHUNK=3 (csrc/nvbx_numbering.h): which workgroup takes which record changes, nothing else may."""
    base = run("default")
    out = run("XCD_CHUNK=3", {"NVBX_LIB": _xcd3_variant()})
    _assert_same_maps(base, out, "XCD_CHUNK=3")
