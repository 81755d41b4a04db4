"""Round 4: the parity holes behind quoted numbers (VERDICT r03 "next round" 1, 2, 9).

* the camera-BATCH path at 640x480 against the checker -- `nvblox_ros/include/nvblox_ros/nvblox_node.hpp:298-332` feeds up to four cameras through one
  mapper; BASELINE.md quotes 4- and 8-camera figures for a launch shape (2 688 tile workgroups beside 1 200 sphere-tracing riders, 2 / 4 lanes per
  ray, both frame sets in one 4 KiB argument block) that only ran at 160x120 in the tests;
* the sequence bench.py times -- 200 poses, map emptied per loop, colour deferral on, at the headline's drain cadence (one per loop segment) and at
  the block figure's (one per block of K steps) -- compared with the checker at its end, through the very function bench.py prints its `parity` block with;
* the bench line itself (subprocess): `parity.ok`, the mode label, the classic-order figure;
* a repeated-run stress of the fused launches with the replay / carry knobs toggled (the 65a453c race showed in 5 runs of 8).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from isaac_ros_nvblox_amd import synthetic as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rig_frames(n_cams, k, cam):
    sc = S.Scene()
    out = []
    for c in range(n_cams):
        T = S.trajectory_pose(k * 9, 200, yaw_offset_deg=45.0 * c)
        d, rgb = S.render(sc, T, cam, color=True)
        out.append((d, rgb, T))
    return out


@pytest.mark.parametrize("n_cams", [4, 8])
def test_camera_batch_at_640x480_against_the_checker(oracle_mod, hip_lib, n_cams):
    """nvbx_integrate_depth_batch / _color_batch at the size BASELINE.md quotes them for, classic order AND the two-launch pipeline, against the
    checker fed camera after camera (the definition of a batch), every step's last view and the final TSDF / colour / ESDF / slice."""
    import bench
    from isaac_ros_nvblox_amd import mapper as M
    cam = S.REPLICA_LIKE_CAM
    pg = M.default_params(); po = H.copy_params(pg, oracle_mod.OrcParams)
    classic = M.Mapper(pg, block_capacity=1 << 14); piped = M.Mapper(pg, block_capacity=1 << 14); o = oracle_mod.OracleMap(po)
    classic.set_color_deferral(False); piped.set_color_deferral(True); piped.set_profiling(True)
    oracle_mod.set_num_threads(min(8, os.cpu_count() or 1))
    for k in range(4):
        fr = rig_frames(n_cams, k, cam)
        ds, cs, Ts = [f[0] for f in fr], [f[1] for f in fr], [f[2] for f in fr]
        for m_ in (classic, piped):
            m_.integrate_depth_batch(ds, Ts, cam); m_.integrate_color_batch(cs, Ts, cam); m_.update_esdf()
        for d, _, T in fr:
            o.integrate_depth(d, T, cam)
        for _, c, T in fr:
            o.integrate_color(c, T, cam)
        o.update_esdf()
        assert H.idx_set(classic.last_view()) == H.idx_set(o.last_view())              # (classic: queries cost it nothing; the pipelined mapper runs undisturbed)
    prof = piped.profile()            # (a drain: the last batch is replayed)
    fused = sum(v["count"] for k_, v in prof.items() if "k_integrate_tsdf_color" in k_)
    assert fused >= 3, {k_: v["count"] for k_, v in prof.items()}                      # steps 1..3 carried the held-back batch in two launches
    assert H.idx_set(piped.last_view()) == H.idx_set(o.last_view()) and H.idx_set(piped.last_color_view()) == H.idx_set(o.last_color_view())
    H.assert_same_map(classic, piped, "%d cameras" % n_cams)
    for g in (classic, piped):
        r = bench.map_parity(M, g, o, oracle_mod)
        assert r["ok"] and r["blocks"] > 600 and r["color_blocks"] > 100 and r["esdf_blocks"] > 50, r
        assert g.counters()["capacity_overflow"] == 0


def test_the_sequence_the_headline_times_ends_in_the_checkers_map(oracle_mod, hip_lib):
    """bench.py's exploring loop at both of its timings' cadences with the driver's flags (--steps 20 --warmup 5): clear(), the 200 poses of SURVEY 8d
    at 640x480, depth + colour + updateEsdf per frame with colour deferral on (two launches per frame) -- the headline's (from pose 5, one drain per
    loop segment) and the block figure's (from pose 0, a drain after every 20 frames) -- each time then the checker, plain call order."""
    import bench
    from isaac_ros_nvblox_amd import mapper as M
    cam = S.REPLICA_LIKE_CAM
    fr = H.frames(200, cam)
    g = M.Mapper(M.default_params(), block_capacity=1 << 14)
    g.set_color_deferral(True); g.set_profiling(True)

    def gpu_step(k):
        d, rgb, T = fr[k]
        g.integrate_depth(d, T, cam); g.integrate_color(rgb, T, cam); g.update_esdf()

    def checker_step(o, k):
        d, rgb, T = fr[k]
        o.integrate_depth(d, T, cam); o.integrate_color(rgb, T, cam); o.update_esdf()
    r = bench.exploring_parity(M, g, gpu_step, g.synchronize, len(fr), checker_step, len(fr), oracle_mod, first=5)
    assert r["ok"] and r["index_sets_equal"] and r["max_abs_tsdf"] <= 1e-4 and r["blocks"] > 1200 and r["first_pose"] == 5, r
    g.set_profiling(True)                 # (clears the spans: the launch count below is the block cadence's 200 frames)
    r = bench.exploring_parity(M, g, gpu_step, g.synchronize, len(fr), checker_step, 20, oracle_mod)
    assert r["ok"] and r["index_sets_equal"] and r["max_abs_tsdf"] <= 1e-4 and r["blocks"] > 1200, r
    prof = g.profile()
    fused = sum(v["count"] for k_, v in prof.items() if "k_integrate_tsdf_color" in k_)
    assert fused >= 180, {k_: v["count"] for k_, v in prof.items()}                    # 19 of every 20 frames in two launches
    assert g.counters()["capacity_overflow"] == 0


def test_bench_line_carries_parity_and_mode():
    """`python bench.py --steps 20 --warmup 5 --full` (the driver's flags, whole line; CPU baseline shortened): rc 0, one JSON line, `parity.ok`,
    the mode label and the classic-order exploring figure as first-class fields."""
    env = dict(os.environ); env["NVBX_BENCH_MIN_MS"] = "150"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--full", "--cpu-seconds", "1", "--cpu-frames", "4"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["parity"]["ok"] and out["parity"]["index_sets_equal"] and out["parity"]["steps_compared"] == 200, out["parity"]
    assert out["parity"]["first_pose"] == 5 and out["parity"]["drain_every"] == 200, out["parity"]          # (the headline's cadence)
    assert "color_deferral" in out["config"]["mode"] and out["ms_per_step"] > 0
    assert out["ms_per_step_classic_order"] > out["ms_per_step_blocks"] > 0     # (like for like: both block figures)
    assert out["roofline"]["frac"] > 0 and out["cpu_baseline"]["value"] > 0 and out["n_gpus"] == 1


@pytest.mark.parametrize("knobs", [dict(), dict(NVBX_REPLAY_PAIR="0"), dict(NVBX_ESDF_ONLY_CARRY="0"), dict(NVBX_REPLAY_PAIR="0", NVBX_ESDF_ONLY_CARRY="0")],
                         ids=["default", "no_replay_pair", "no_esdf_only_carry", "neither"])
def test_fused_launches_stress_repeated_runs(knobs):
    """The randomised call patterns of tests/test_gpu_pipeline.py (three seeds), twenty repetitions each in ONE process per knob setting (every mapper
    of the process reads the knobs as it is created), bit-identity with the classic mapper asserted in every repetition: an intermittent race between the riders of
    the fused launches shows as a failure in SOME repetition (65a453c: 5 of 8)."""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import functools, oracle, helpers, test_gpu_pipeline as P\n"
        "helpers.frames = functools.lru_cache(maxsize=None)(helpers.frames)      # (the rendered inputs are the same in every repetition)\n"
        "from isaac_ros_nvblox_amd import _lib\n"
        "lib = _lib.load()\n"
        "for rep in range(20):\n"
        "    for seed in (0, 1, 2):\n"
        "        P.test_fused_colour_tsdf_launch_under_irregular_calls(oracle, lib, seed)\n"
        "print('STRESS_OK')\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ); env.update(knobs)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert p.returncode == 0 and "STRESS_OK" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])


def test_bench_gpus_2_starts_itself_and_prints_one_line():
    """`python bench.py --gpus 2` with no WORLD_SIZE: the script starts its two ranks itself (torch.distributed.run).  On a 1-GPU box both ranks share
    device 0 and rendezvous over gloo (NVBX_BENCH_SAME_DEVICE / NVBX_BENCH_BACKEND): a control-flow check of the N > 1 path, not a measurement."""
    env = dict(os.environ); env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    env.update(NVBX_BENCH_SAME_DEVICE="1", NVBX_BENCH_BACKEND="gloo", NVBX_BENCH_MIN_MS="60", OMP_NUM_THREADS="4")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--unique-frames", "8", "--full", "--cpu-seconds", "0.5", "--cpu-frames", "2"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["scaling"] == "weak" and out["parity"]["ok"], out
    assert out["color_deferral"]["enabled"] and out["color_deferral"]["launches_per_frame"] == 2, out["color_deferral"]      # N > 1 ranks take the two-launch pipeline


@pytest.mark.parametrize("cam", [H.SMALL_CAM, S.REPLICA_LIKE_CAM], ids=["160x120", "640x480"])
def test_dynamic_front_end_in_three_launches_equals_the_three_calls_and_the_checker(oracle_mod, hip_lib, cam):
    """nvbx_dynamic_depth_split (detect dynamics -> remove small components -> split, three launches, no memset) against the three separate entry
    points on a second mapper fed the same frames, and against the checker's detect / remove_small_components / split_depth_by_mask: the cleaned
    mask and both depth images bit for bit, every frame -- from the first (no freespace layer yet) to frames with a moving box in view; also
    with the component filter off and with the overlay image.  (A box is one roughly convex blob: for mask SHAPES that need the cross-patch
    rules of k_dyn_detect_union see tests/test_gpu_dynamic_masks.py.)"""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    rows, cols = cam[5], cam[4]
    min_component = 40 if cols == 160 else 640
    dev = torch.device("cuda", 0)
    fs = dict(projective_layer_type=2, max_integration_distance_m=5.0, invalid_depth_decay_factor=0.8, min_duration_since_occupied_for_freespace_ms=250)
    pg = M.default_params(**fs)
    a = M.Mapper(pg, block_capacity=1 << 14); b = M.Mapper(pg, block_capacity=1 << 14); o = oracle_mod.OracleMap(H.copy_params(pg, oracle_mod.OrcParams))
    b.set_profiling(True)
    eye = np.eye(4, dtype=np.float32)
    n_dynamic = 0
    static_scene = S.Scene(); moving = S.Scene(box_min=(1.6, -0.3, 0.0), box_max=(2.0, 0.3, 1.3))      # (the scenes of test_dynamic_mapping_parity)
    for i in range(14):
        # the static room for 0.8 s at 10 Hz from a slowly turning camera (free voxels become high-confidence freespace), then an object in mid-room
        sc = static_scene if i < 8 else moving
        T = S.trajectory_pose(min(i, 8), 200)
        d, _ = S.render(sc, T, cam, max_range=5.0, color=False)
        d_dev = torch.from_numpy(d).to(dev)
        thr = min_component if i != 9 else 0                      # (one frame with the filter off)
        mk_a = torch.empty((rows, cols), dtype=torch.uint8, device=dev); un_a = torch.empty((rows, cols), dtype=torch.float32, device=dev); ma_a = torch.empty_like(un_a)
        a.detect_dynamics_into(d_dev, T, cam, 5.0, mk_a)
        if thr:
            a.remove_small_components_inplace(mk_a, thr)
        a.split_depth_by_mask_into(d_dev, mk_a, eye, cam, cam, 0.25, un_a, ma_a)
        mk_b = torch.empty_like(mk_a); un_b = torch.empty_like(un_a); ma_b = torch.empty_like(un_a)
        ov = torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev) if i % 4 == 0 else None
        b.dynamic_depth_split_into(d_dev, T, cam, 5.0, thr, 0.25, mk_b, un_b, ma_b, ov)
        a.synchronize(); b.synchronize()            # (each mapper owns its stream; the comparisons run on torch's)
        assert torch.equal(mk_a, mk_b) and torch.equal(un_a, un_b) and torch.equal(ma_a, ma_b), i
        mo = o.detect_dynamics(d, T, cam, 5.0)
        if thr:
            mo = oracle_mod.remove_small_components(mo, thr)
        uo, mao = oracle_mod.split_depth_by_mask(d, mo, eye, cam, cam, 0.25)
        assert np.array_equal(mk_b.cpu().numpy(), mo) and np.array_equal(un_b.cpu().numpy(), uo) and np.array_equal(ma_b.cpu().numpy(), mao), i
        if ov is not None:
            red = ov.cpu().numpy()[..., 0] == 255
            assert np.array_equal(red & (d > 0) & (d * 51.0 < 255.0), (ma_b.cpu().numpy() > 0) & (d * 51.0 < 255.0))
        n_dynamic += int(mk_b.sum().item())
        for m_, un_, t_ in ((a, un_a, i * 100), (b, un_b, i * 100)):
            m_.set_time_ms(t_); m_.integrate_depth(un_, T, cam)
        o.set_time_ms(i * 100); o.integrate_depth(uo, T, cam)
    assert n_dynamic > (600 if cols == 160 else 9000), n_dynamic          # the object was detected in several frames (and survived the clean-up)
    prof = b.profile()
    names = {bench_short(k_) for k_ in prof}
    assert "k_dyn_detect_union" in names and "k_dyn_filter_split" in names and not ({"k_detect_dynamics", "k_cc_union", "k_cc_filter", "k_mask_zmin", "k_split_depth"} & names), names
    per_call = sum(v["count"] for k_, v in prof.items() if bench_short(k_) in ("k_dyn_detect_union", "k_cc_count", "k_dyn_filter_split", "k_dyn_init")) / 14.0
    assert per_call <= 3.1, per_call


def bench_short(name):
    import bench
    return bench.short(name)


def test_staged_colour_deferral_survives_a_recycled_colour_buffer(oracle_mod, hip_lib):
    """nvbx_mapper_set_color_deferral(m, 2) -- what nvblox::Mapper::setColorIntegrationDeferred(true) switches on: the held-back frame is copied into
    mapper-owned memory, so a host that refills or scribbles over its ONE colour buffer right after integrateColor returns (a ROS callback,
    nvblox_node.hpp:485-488) still gets the classic result, bit for bit, in two launches per frame.  (Zero-copy deferral, mode 1, would read the
    scribbled buffer: its contract forbids exactly this.)"""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    cam = H.SMALL_CAM
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        pg = M.default_params()
        classic = M.Mapper(pg, block_capacity=1 << 13, stream=stream.cuda_stream); staged = M.Mapper(pg, block_capacity=1 << 13, stream=stream.cuda_stream)
        zero_copy = M.Mapper(pg, block_capacity=1 << 13, stream=stream.cuda_stream)
        classic.set_color_deferral(False)
        staged.set_color_deferral(True, staged=True); staged.set_profiling(True)
        zero_copy.set_color_deferral(True, staged=False)
        buf = torch.empty((cam[5], cam[4], 3), dtype=torch.uint8, device=dev)          # the host's one colour buffer
        noise = torch.randint(0, 255, buf.shape, dtype=torch.uint8, device=dev)
        for k, (d, rgb, T) in enumerate(H.frames(10, cam, stride=7)):
            d_dev = torch.from_numpy(d).to(dev)
            for m_ in (classic, staged, zero_copy):
                m_.integrate_depth(d_dev, T, cam)
                buf.copy_(torch.from_numpy(rgb).to(dev))
                m_.integrate_color(buf, T, cam)
                buf.copy_(noise)                               # recycled before the next call into the mapper
                m_.update_esdf()
        for m_ in (classic, staged, zero_copy):
            m_.synchronize()
    H.assert_same_map(classic, staged, "staged deferral")
    ic = classic.block_indices(M.LAYER_COLOR)
    bc, _ = classic.get_blocks(M.LAYER_COLOR, ic); bz, _ = zero_copy.get_blocks(M.LAYER_COLOR, ic)
    assert not np.array_equal(bc["r"], bz["r"])              # (the test does scribble where it matters: the zero-copy mapper integrated the noise)
    prof = staged.profile()
    assert sum(v["count"] for k_, v in prof.items() if "k_integrate_tsdf_color" in k_) >= 8, {k_: v["count"] for k_, v in prof.items()}


def test_union_step_of_the_index_exchange_rides_in_the_fused_launch(oracle_mod, hip_lib):
    """One camera per GPU with colour deferral on (bench.py --gpus N): the union step of the peers' gathered block lists
    (nvbx_mark_esdf_dirty_gathered_deferred) is held back and rides in the NEXT depth frame's fused TSDF-update launch -- two launches per frame
    for N > 1 as well.  One GPU, a stand-in peer (a second mapper looking the other way, its per-frame block list exported by its own depth pass):
    the map of the rank with the exchange == a mapper without any exchange, bit for bit (re-marking a column from an unchanged TSDF changes no
    voxel), the fused launch ran every frame, no marking launch of its own was needed, and the last update's sweep window reaches the peer's blocks."""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    cam = H.SMALL_CAM
    dev = torch.device("cuda", 0)
    pg = M.default_params()
    plain = M.Mapper(pg, block_capacity=1 << 13); rank0 = M.Mapper(pg, block_capacity=1 << 13); peer = M.Mapper(pg, block_capacity=1 << 13)
    own = H.frames(24, cam, stride=8); other = H.frames(24, cam, stride=8, yaw_offset_deg=180.0)
    for d, rgb, T in own + other:                 # both ranks know the whole room already (the peers' blocks exist locally)
        for m_ in (plain, rank0):
            m_.integrate_depth(d, T, cam)
    for m_ in (plain, rank0):
        m_.update_esdf(); m_.synchronize()
    plain.set_color_deferral(False); rank0.set_color_deferral(True); rank0.set_profiling(True)
    bufs = [torch.zeros((2, 4097, 3), dtype=torch.int32, device=dev) for _ in range(3)]       # three rotating gathered sets, as dist.PipelinedDirtyBlockExchange
    for k in range(12):
        d, rgb, T = own[2 * k]; dp, _, Tp = other[2 * k]
        g = bufs[k % 3]
        peer.set_view_export(g[1]); peer.integrate_depth(dp, Tp, cam); peer.synchronize()     # the peer's message (row 0 = count)
        for m_ in (plain, rank0):
            m_.integrate_depth(d, T, cam)
        rank0.mark_esdf_dirty_gathered(g, 2, 0, 4096, deferred=True)
        for m_ in (plain, rank0):
            m_.integrate_color(rgb, T, cam); m_.update_esdf()
        assert int(g[1, 0, 0].item()) > 50
    prof = rank0.profile()
    fused = sum(v["count"] for k_, v in prof.items() if "k_integrate_tsdf_color" in k_)
    own_launches = sum(v["count"] for k_, v in prof.items() if "k_import_mark_gathered" in k_)       # (only the drain by profile() launches the last step's list on its own)
    assert fused >= 11 and own_launches <= 1, {k_: v["count"] for k_, v in prof.items()}
    # the last update (replayed by the drain above) re-marked the peer's blocks of the step before, dirtied by the last fused launch: they lie
    # behind this camera, so more columns were marked and the sweep window is larger than without the exchange
    c0, c1 = plain.counters(), rank0.counters()
    assert c1["esdf_columns_marked"] > c0["esdf_columns_marked"] and c1["esdf_window_voxels"] > c0["esdf_window_voxels"], (c0, c1)
    H.assert_same_map(plain, rank0, "index exchange in the pipeline", slice=True)


def test_advice_r03_two_updates_in_a_row_and_lidar_then_colour(oracle_mod, hip_lib):
    """(a) Two updateEsdf calls held back with nothing between them stay two updates: the "last update" counters equal the undeferred mapper's.
    (b) One LiDAR scan no longer keeps a camera + LiDAR mapper out of the fused launches for good: the next colour launch repairs every block the
    scan left stale, and the frames after it run in two launches again -- with the classic mapper's map, bit for bit."""
    from isaac_ros_nvblox_amd import mapper as M
    cam = H.SMALL_CAM
    pg = M.default_params(lidar_max_integration_distance_m=6.0)
    a = M.Mapper(pg, block_capacity=1 << 13); b = M.Mapper(pg, block_capacity=1 << 13)
    a.set_color_deferral(False); b.set_color_deferral(True); b.set_profiling(True)
    fr = H.frames(14, cam, stride=6)
    lidar = (128, 16, 0.1, -np.deg2rad(20.0), np.deg2rad(20.0))
    Tl = np.eye(4, dtype=np.float32); Tl[:3, 3] = (-1.0, 0.5, 1.0)
    rng_img = S.Scene().raycast(Tl[:3, 3].astype(float), S.lidar_beam_dirs(lidar).reshape(-1, 3)).reshape(16, 128).astype(np.float32)
    for k, (d, rgb, T) in enumerate(fr):
        for m_ in (a, b):
            m_.integrate_depth(d, T, cam); m_.integrate_color(rgb, T, cam); m_.update_esdf()
            if k == 3:
                m_.update_esdf()                          # a second update right behind the first
        if k == 3:
            ca, cb = a.counters(), b.counters()
            for f in ("esdf_columns_marked", "esdf_blocks_swept", "esdf_window_voxels"):
                assert ca[f] == cb[f], (f, ca[f], cb[f])
        if k == 5:
            for m_ in (a, b):
                m_.integrate_lidar_depth(rng_img, Tl, lidar)
            n_fused_before = sum(v["count"] for k_, v in b.profile().items() if "k_integrate_tsdf_color" in k_)
            b.set_profiling(True)
    prof = b.profile()
    fused_after = sum(v["count"] for k_, v in prof.items() if "k_integrate_tsdf_color" in k_)
    assert n_fused_before >= 3 and fused_after >= 5, (n_fused_before, {k_: v["count"] for k_, v in prof.items()})      # frames 8..13 fused again
    H.assert_same_map(a, b, "camera + LiDAR mapper")


def test_dynamic_mapper_on_its_own_stream_equals_one_stream(oracle_mod, hip_lib):
    """nvbx_mapper_wait_for: the dynamic (occupancy) mapper of a dynamic-mapping frame on a stream of its own, ordered against the static mapper's stream
    with nvbx_mapper_wait_for at the two hand-overs of the split depth image (written on the static mapper's stream, read on the other; two buffers
    in turn).  The same 24 frames -- fused front end, both mappers with colour deferral, decay every 6th frame, nothing in the loop
    waits for the GPU -- as with both mappers on one stream: masks, split images, both maps, freespace and both ESDFs bit for bit."""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    cam = S.REPLICA_LIKE_CAM
    rows, cols = cam[5], cam[4]
    dev = torch.device("cuda", 0)
    s0 = torch.cuda.Stream(dev); s1 = torch.cuda.Stream(dev); s2 = torch.cuda.Stream(dev)
    fs = dict(projective_layer_type=2, max_integration_distance_m=5.0, invalid_depth_decay_factor=0.8, tsdf_decay_factor=0.95,
              min_duration_since_occupied_for_freespace_ms=250)
    occ = dict(projective_layer_type=1, max_integration_distance_m=5.0)
    frames = []
    static_scene = S.Scene(); moving = S.Scene(box_min=(1.6, -0.3, 0.0), box_max=(2.0, 0.3, 1.3))      # (the static room for 0.8 s, then an object in mid-room)
    for i in range(24):
        sc = static_scene if i < 8 else moving
        T = S.trajectory_pose(min(i, 8) + max(0, i - 8) // 4, 200)
        d, rgb = S.render(sc, T, cam, max_range=5.0)
        frames.append((torch.from_numpy(d).to(dev), torch.from_numpy(rgb).to(dev), T))
    torch.cuda.synchronize(dev)

    def run(stream_s, stream_d):
        with torch.cuda.stream(stream_s):
            gs = M.Mapper(M.default_params(**fs), block_capacity=1 << 14, stream=stream_s.cuda_stream)
            gd = M.Mapper(M.default_params(**occ), block_capacity=1 << 13, stream=stream_d.cuda_stream)
            gs.set_color_deferral(True); gd.set_color_deferral(True)
            mask = torch.empty((rows, cols), dtype=torch.uint8, device=dev); un = torch.empty((rows, cols), dtype=torch.float32, device=dev)
            ma2 = [torch.empty_like(un), torch.empty_like(un)]
            kept = []; n_dyn = 0
            for i, (d_dev, rgb_dev, T) in enumerate(frames):
                ma = ma2[i & 1]              # two buffers, as bench.py: frame i + 1's split must not overwrite what the dynamic mapper reads in frame i
                gs.dynamic_depth_split_into(d_dev, T, cam, 5.0, 640, 0.25, mask, un, ma)
                gs.wait_for(gd)              # (the dynamic mapper's frame i - 1 is over before this stream goes on to frame i + 1's split)
                gd.wait_for(gs)              # (`ma` is written)
                gs.set_time_ms(i * 100)
                gs.integrate_depth(un, T, cam); gd.integrate_depth(ma, T, cam)
                gs.integrate_color(rgb_dev, T, cam)
                gs.update_esdf(); gd.update_esdf()
                if i % 6 == 5:
                    gs.decay_tsdf(True); gd.decay_occupancy()
                if i % 4 == 3:
                    kept.append((mask.clone(), ma.clone()))          # (on the static mapper's stream, behind the split that wrote them)
            gs.synchronize(); gd.synchronize(); torch.cuda.synchronize(dev)
            n_dyn = sum(int(m_.sum().item()) for m_, _ in kept)
        return gs, gd, kept, n_dyn

    gs_a, gd_a, kept_a, n_a = run(s0, s0)
    gs_b, gd_b, kept_b, n_b = run(s1, s2)
    assert n_a == n_b and n_a > 9000, (n_a, n_b)
    for (ma_, da_), (mb_, db_) in zip(kept_a, kept_b):
        assert torch.equal(ma_, mb_) and torch.equal(da_, db_)
    H.assert_same_map(gs_a, gs_b, "static mapper", layers=(M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF, M.LAYER_FREESPACE),
                      min_blocks={M.LAYER_FREESPACE: 51}, slice=True)
    H.assert_same_map(gd_a, gd_b, "dynamic mapper", layers=(M.LAYER_OCCUPANCY, M.LAYER_ESDF), min_blocks={M.LAYER_OCCUPANCY: 1}, slice=True)
