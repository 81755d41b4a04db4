"""The scripted workload of tests/test_gpu_launch_geometry.py, in a process of its own (a mapper reads the NVBX_* knobs when it is created, so one process
could hold every setting; a process per setting also keeps a fault of one from the others):  python tests/launch_geometry_child.py INPUTS.npz OUT.npz

`schedule` drives five kinds of mapper through one fixed sequence of calls and takes a snapshot of every mapper after every phase (a later decay or
clear could hide an earlier error):
  A   TSDF + colour + 2-D ESDF, colour deferral on (the fused two-launch form), 512 blocks to start with: the pools grow mid-schedule.  Fused frames, a
      close-up frame followed by a wide one (the grid hint falls far short), camera batches, decay -> decay -> growth -> decay, radius and shape
      clearing, the depth pair with an occupancy mapper (Bo) and with a TSDF mapper holding colour and an ESDF update (Bt), point queries.
  C   occupancy + ESDF, decay across a growth.     D   3-D ESDF, decay and radius clearing.     E   LiDAR on the sparse path, ESDF and decay.
The same `schedule` replays on the CPU checker in the test (`Runner` is the GPU side; a pair becomes the two calls there, a batch separate calls).
A snapshot holds, per mapper and layer, the sorted block indices and the raw voxel bytes, the mesh, the ESDF slice and its AABB, the blocks reported
cleared since the last snapshot and the point-query results; the child adds the capacity history and the profile's launch counts.  Every snapshot of
the GPU side also probes the hash: every live block is found through the table, its 26-neighbour shell and the cleared blocks are not."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CAM = (80.0, 80.0, 79.5, 59.5, 160, 120)
LIDAR = (256, 16, 0.1, -np.deg2rad(15.0), np.deg2rad(15.0))
MAX_CAPACITY = 1 << 16
OCC = dict(projective_layer_type=1, free_region_occupancy_probability=0.3, occupied_region_occupancy_probability=0.9,
           unobserved_region_occupancy_probability=0.35, occupied_region_half_width_m=0.2, max_integration_distance_m=5.0)
DECAY = dict(tsdf_decay_factor=0.5, tsdf_decayed_weight_threshold=0.3)
# name -> (parameters, initial block capacity, layers; the first is the one the hash probe walks)
MAPPERS = {
    "A": (dict(DECAY), 512, ("tsdf", "color", "esdf")),
    "Bo": (dict(OCC), 512, ("occupancy",)),
    "Bt": (dict(), 1024, ("tsdf", "color", "esdf")),
    "C": (dict(OCC, free_region_decay_probability=0.55, occupied_region_decay_probability=0.30), 512, ("occupancy", "esdf")),
    "D": (dict(DECAY, esdf_mode=1, esdf_max_distance_m=1.0, max_integration_distance_m=4.0), 1 << 12, ("tsdf", "esdf")),
    "E": (dict(DECAY, voxel_size=0.1, lidar_max_integration_distance_m=20.0, raycast_subsampling_factor=2,
               lidar_nearest_interpolation_max_allowable_dist_to_ray_vox=0.5), 1 << 14, ("tsdf", "esdf")),
}
SHAPES = [("sphere", (1.5, 1.0, 0.6), 0.7), ("aabb", (-3.1, -2.6, -0.1), (-1.2, -0.4, 1.0))]


def render_inputs():
    """Every input of the schedule, rendered once (the parent hands the same file to every child)."""
    import helpers as H
    from isaac_ros_nvblox_amd import synthetic as S
    out = {}

    def put(tag, frames, color=True):
        out[tag + "_d"] = np.stack([f[0] for f in frames]).astype(np.float32)
        out[tag + "_T"] = np.stack([f[2] for f in frames]).astype(np.float32)
        if color:
            out[tag + "_rgb"] = np.stack([f[1] for f in frames]).astype(np.uint8)
    put("room", H.frames(4, CAM, color=True, stride=7))                         # phase 1 (3 frames) + the close-up
    put("wide", H.frames(1, CAM, start=100, color=True))                        # the far side of the room
    put("batch", H.frames(8, CAM, start=30, color=True, stride=5))              # two batches of four
    put("pair", H.frames(3, CAM, start=60, color=True, stride=7))
    put("occ", H.frames(4, CAM, start=10, color=False, stride=9), color=False)
    put("esdf3", H.frames(4, CAM, start=20, color=False, stride=8), color=False)
    # growth: a hall seen from its middle, turning, ranges cut at 3.5 m -- a few hundred new blocks per frame, fewer than the pools' free half
    big = S.Scene(room_min=(-7.0, -6.0, 0.0), room_max=(7.0, 6.0, 3.0))
    grow = []
    for k in range(12):
        T = S.trajectory_pose(k * 17, 200, radius=0.5)
        d, rgb = S.render(big, T, CAM, max_range=3.5)
        grow.append((d, rgb, T))
    put("grow", grow, color=False)
    d = out["room_d"][3].copy()
    keep = np.zeros_like(d); keep[52:68, 72:88] = 1.0
    out["closeup_d"] = (d * keep)[None]
    sc = S.LidarScene(n_boxes=12, extent=40.0)
    out["lidar_T"] = np.stack([S.lidar_pose(i * 7) for i in range(4)]).astype(np.float32)
    out["lidar_d"] = np.stack([S.render_lidar(sc, T, LIDAR, max_range=40.0) for T in out["lidar_T"]]).astype(np.float32)
    rng = np.random.default_rng(7)
    out["query_p"] = (rng.random((2048, 3)) * np.array([6.0, 5.0, 3.0]) + np.array([-3.0, -2.5, 0.0])).astype(np.float32)
    return out


def schedule(R, I):
    """The fixed sequence of calls; R: a runner (GPU or checker), I: the inputs.  R.snap(phase, names) takes the snapshots."""
    cam = CAM
    for name in MAPPERS:
        R.new(name)
    # 1. fused frames: depth + colour + updateEsdf, three times
    for k in range(3):
        R.depth("A", I["room_d"][k], I["room_T"][k]); R.color("A", I["room_rgb"][k], I["room_T"][k]); R.esdf("A")
    R.snap("1_fused", ["A"])
    # 2. a close-up frame (a few blocks in view, the GPU has reported it), then a wide one: the hint falls far short
    R.sync("A")
    R.depth("A", I["closeup_d"][0], I["room_T"][3]); R.color("A", I["room_rgb"][3], I["room_T"][3])
    R.sync("A")
    R.depth("A", I["wide_d"][0], I["wide_T"][0]); R.color("A", I["wide_rgb"][0], I["wide_T"][0]); R.esdf("A")
    R.snap("2_hint_short", ["A"])
    # 3. camera batches (the second depth batch carries the first colour batch), then a mesh
    for b in (0, 4):
        R.depth_batch("A", I["batch_d"][b:b + 4], I["batch_T"][b:b + 4])
        R.color_batch("A", I["batch_rgb"][b:b + 4], I["batch_T"][b:b + 4])
    R.esdf("A"); R.mesh("A")
    R.snap("3_batch", ["A"], mesh=True)
    # 4. decay, decay, frames until the pools have doubled, decay
    R.decay("A"); R.take_cleared("A"); R.decay("A"); R.take_cleared("A")
    R.grow("A", I["grow_d"], I["grow_T"])
    R.decay("A"); R.take_cleared("A"); R.esdf("A")
    R.snap("4_decay_growth", ["A"])
    # 5. clearing
    R.clear_radius("A", (0.0, 0.0, 1.0), 4.0); R.take_cleared("A")
    R.clear_shapes("A", SHAPES); R.take_cleared("A")
    R.esdf("A"); R.mesh("A")
    R.snap("5_clear", ["A"], mesh=True)
    # 6. the depth pair: with an occupancy mapper (nvblox_ros' dynamic / human mapping), then with a TSDF mapper that holds colour and an updateEsdf
    for k in range(3):
        d, T = I["pair_d"][k], I["pair_T"][k]
        fg = d.copy(); fg[:, : cam[4] // 2] = 0.0
        R.color("A", I["pair_rgb"][k], T)
        if k != 1:
            R.esdf("A")
        R.pair("A", d, "Bo", fg, T)
    for k in range(3):
        d, T = I["pair_d"][k], I["pair_T"][k]
        R.color("A", I["pair_rgb"][k], T); R.color("Bt", I["pair_rgb"][k], T)
        R.esdf("Bt")
        if k != 2:
            R.esdf("A")
        R.pair("A", d, "Bt", d, T)
    R.esdf("A"); R.esdf("Bt"); R.esdf("Bo"); R.mesh("A"); R.mesh("Bt")
    R.snap("6_pair", ["A", "Bo", "Bt"], mesh=True)
    # 7. point queries
    R.query("A", I["query_p"])
    R.snap("7_query", ["A"])
    # C: occupancy, decay across a growth
    for k in range(3):
        R.depth("C", I["occ_d"][k], I["occ_T"][k])
    R.esdf("C")
    R.snap("c1_frames", ["C"])
    R.decay("C"); R.take_cleared("C"); R.decay("C"); R.take_cleared("C")
    R.grow("C", I["grow_d"], I["grow_T"])
    R.decay("C"); R.take_cleared("C"); R.esdf("C")
    R.snap("c2_decay_growth", ["C"])
    # D: 3-D ESDF
    for k in range(3):
        R.depth("D", I["esdf3_d"][k], I["esdf3_T"][k])
        if k != 1:
            R.esdf("D")
    R.snap("d1_frames", ["D"])
    R.decay("D"); R.take_cleared("D"); R.decay("D"); R.take_cleared("D"); R.esdf("D")
    R.depth("D", I["esdf3_d"][3], I["esdf3_T"][3])
    T = I["esdf3_T"][3]
    R.clear_radius("D", (float(T[0, 3]), float(T[1, 3]), 1.0), 2.2); R.take_cleared("D"); R.esdf("D")
    R.snap("d2_decay_clear", ["D"])
    # E: LiDAR (sparse path), ESDF, decay
    for k in range(3):
        R.lidar("E", I["lidar_d"][k], I["lidar_T"][k])
    R.esdf("E")
    R.snap("e1_scans", ["E"])
    R.decay("E"); R.take_cleared("E"); R.decay("E"); R.take_cleared("E")
    R.lidar("E", I["lidar_d"][3], I["lidar_T"][3]); R.esdf("E")
    R.snap("e2_decay", ["E"])


def neighbour_shell(idx):
    """The 26-neighbour shell of a set of block indices, minus the set."""
    live = set(map(tuple, idx.tolist()))
    out = set()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if dx or dy or dz:
                    out.update(map(tuple, (idx + np.array([dx, dy, dz], np.int32)).tolist()))
    return np.array(sorted(out - live), np.int32).reshape(-1, 3)


class Runner:
    """The schedule on the GPU: every mapper of the camera part on one stream (the depth pair needs that), LiDAR / occupancy / 3-D ESDF on their own."""

    def __init__(self, torch, stream):
        from isaac_ros_nvblox_amd import mapper as M
        self.M, self.torch, self.stream = M, torch, stream
        self.m, self.cleared, self.capacity, self.queries, self.out = {}, {}, {}, {}, {}
        self.growth_frames = {}

    def new(self, name):
        M = self.M
        kw, cap, _ = MAPPERS[name]
        s = self.stream.cuda_stream if name in ("A", "Bo", "Bt") else None
        g = M.Mapper(M.default_params(**kw), block_capacity=cap, stream=s, max_block_capacity=MAX_CAPACITY)
        g.set_profiling(True)
        self.m[name] = g
        self.cleared[name] = []
        self.capacity[name] = [g.capacity]

    def _cap(self, name):
        c = self.m[name].capacity
        if c != self.capacity[name][-1]:
            self.capacity[name].append(c)

    def depth(self, name, d, T):
        self.m[name].integrate_depth(d, T, CAM); self._cap(name)

    def color(self, name, rgb, T):
        self.m[name].integrate_color(rgb, T, CAM)

    def esdf(self, name):
        self.m[name].update_esdf()

    def mesh(self, name):
        self.m[name].update_color_mesh()

    def sync(self, name):
        self.m[name].synchronize()

    def depth_batch(self, name, ds, Ts):
        self.m[name].integrate_depth_batch(list(ds), list(Ts), [CAM] * len(ds)); self._cap(name)

    def color_batch(self, name, rgbs, Ts):
        self.m[name].integrate_color_batch(list(rgbs), list(Ts), [CAM] * len(rgbs))

    def pair(self, a, da, b, db, T):
        self.m[a].integrate_depth_pair(da, self.m[b], db, T, CAM); self._cap(a); self._cap(b)

    def lidar(self, name, img, T):
        self.m[name].integrate_lidar_depth(img, T, LIDAR); self._cap(name)

    def decay(self, name):
        g = self.m[name]
        if g.params.projective_layer_type == 1:
            g.decay_occupancy()
        else:
            g.decay_tsdf(True)

    def take_cleared(self, name):
        self.cleared[name].append(self.m[name].take_cleared_blocks())

    def clear_radius(self, name, c, r):
        self.m[name].clear_outside_radius(c, r)

    def clear_shapes(self, name, shapes):
        self.m[name].clear_tsdf_inside_shapes(shapes)

    def grow(self, name, ds, Ts):
        """Frames of a larger scene until the pools have doubled (synchronised before each: growth is decided from the free count the GPU last
        reported, so this makes the number of frames the same in every run -- the checker replays that number)."""
        g = self.m[name]
        g.synchronize()
        cap0 = g.capacity
        n = 0
        while g.capacity < 2 * cap0:          # (a frame's first step grows the pools if the count last reported asks for it)
            assert n < len(ds), "%s: the pools did not double (%d -> %d blocks)" % (name, cap0, g.capacity)
            self.depth(name, ds[n], Ts[n]); n += 1
            g.synchronize()
        self.growth_frames[name] = n

    def query(self, name, pts):
        g = self.m[name]
        d, gr, v = g.query_tsdf(pts)
        e, ge, ve = g.query_esdf(pts)
        self.torch.cuda.synchronize()
        self.queries[name] = dict(tsdf_d=d.cpu().numpy(), tsdf_g=gr.cpu().numpy(), tsdf_v=v.cpu().numpy(),
                                  esdf_d=e.cpu().numpy(), esdf_g=ge.cpu().numpy(), esdf_v=ve.cpu().numpy())

    def snap(self, phase, names, mesh=False):
        M = self.M
        layer_of = dict(tsdf=M.LAYER_TSDF, color=M.LAYER_COLOR, esdf=M.LAYER_ESDF, occupancy=M.LAYER_OCCUPANCY)
        for name in names:
            g = self.m[name]
            key = "%s/%s/" % (phase, name)
            layers = MAPPERS[name][2]
            for lay in layers:
                idx = g.block_indices(layer_of[lay])
                blk, found = g.get_blocks(layer_of[lay], idx)
                assert found.all(), (phase, name, lay, "block_indices lists a block the hash does not find", idx[~found][:5])
                self.out[key + lay + "/idx"] = idx
                self.out[key + lay + "/bytes"] = np.frombuffer(blk.tobytes(), np.uint8)
            # hash probe: the live set is found through the table (above); its shell and the cleared blocks are not
            main = layer_of[layers[0]]
            live = g.block_indices(main)
            cleared = np.concatenate(self.cleared[name] + [np.zeros((0, 3), np.int32)]).reshape(-1, 3)
            live_set = set(map(tuple, live.tolist()))
            gone = np.array([c for c in map(tuple, cleared.tolist()) if c not in live_set], np.int32).reshape(-1, 3)
            for what, probe in (("shell", neighbour_shell(live)), ("cleared", gone)):
                if len(probe):
                    _, f = g.get_blocks(main, probe)
                    assert not f.any(), (phase, name, "the hash finds %s blocks that are not live" % what, probe[f][:5])
            self.out[key + "cleared"] = np.unique(cleared, axis=0) if len(cleared) else cleared
            self.cleared[name] = []
            if "esdf" in layers:
                img, aabb = g.esdf_slice_image()
                self.out[key + "slice/img"] = img; self.out[key + "slice/aabb"] = np.asarray(aabb, np.float32)
            if mesh:
                mg = g.mesh()
                keys = sorted(k for k in mg if len(mg[k]["triangles"]))
                self.out[key + "mesh/idx"] = np.array(keys, np.int32).reshape(-1, 3)
                self.out[key + "mesh/nv"] = np.array([len(mg[k]["vertices"]) for k in keys], np.int64)
                self.out[key + "mesh/nt"] = np.array([len(mg[k]["triangles"]) for k in keys], np.int64)
                for f, shape, dt in (("vertices", 3, np.float32), ("normals", 3, np.float32), ("colors", 4, np.uint8), ("triangles", 3, np.int32)):
                    self.out[key + "mesh/" + f] = np.concatenate([mg[k][f] for k in keys] + [np.zeros((0, shape), dt)])
            if name in self.queries:
                for f, v in self.queries.pop(name).items():
                    self.out[key + "query/" + f] = v
            c = g.counters()
            assert c["capacity_overflow"] == 0, (phase, name, "capacity overflow", c["capacity_overflow"])
            self.out["meta/%s/%s/capacity" % (phase, name)] = np.array(self.capacity[name], np.int64)
            self.out["meta/%s/%s/profile" % (phase, name)] = np.frombuffer(json.dumps(
                {k: v["count"] for k, v in g.profile().items()}, sort_keys=True).encode(), np.uint8)


def main(inp, out_path):
    import torch
    I = dict(np.load(inp))
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        R = Runner(torch, stream)
        schedule(R, I)
        R.out["meta/growth_frames"] = np.frombuffer(json.dumps(R.growth_frames, sort_keys=True).encode(), np.uint8)
        torch.cuda.synchronize()
    np.savez(out_path, **R.out)
    for g in R.m.values():
        g.close()
    print("LAUNCH_GEOMETRY_CHILD_OK %d arrays" % len(R.out))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
