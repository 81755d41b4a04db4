"""Time of rendering and ray casts (nvbx_render_view / nvbx_cast_rays) on the bench's room map.

The room map of the 640x480 200-pose loop (synthetic.sequence) is built once and saved; then child processes -- one per setting of
NVBX_RENDER_LANES (read when the child's mapper is created; 0 = the library's choice by ray count), alternating, each under its own time limit -- load the map
and time, after warm-up and over >= --seconds of back-to-back calls each:
  view_160x120_depth       640 x 480 at subsampling 4, depth only -- next to its yardstick `k_sphere_trace`, the stand-alone sphere tracing of
                           integrate_color at the same pose on the same mapper in classic order (set_color_deferral(0)): the same march over
                           the same rays.  The yardstick is timed --yard-reps times (>= 5); their spread is the run-to-run spread to read the
                           difference against.  Both are the mapper's own per-launch event spans (set_profiling), taken in one process.
  view_640x480_depth       subsampling 1, depth only
  view_640x480_all         subsampling 1, depth + colour + normals
  rays_307200              307 200 rays: origins in the observed free space, random unit directions; t + hit
One JSON object per line: us per call (device events around the batch of calls), rays/s, hits, the lanes-per-ray setting.
Usage: python tools/render_bench.py [--lanes 0 8 4 2 1] [--reps 1] [--out FILE] [--map DIR]
(a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/render_bench.py --child DIR, DIR from --map)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POSE_INDEX = 37          # the pose every case renders from: a frame of the loop, so that the yardstick integrates a colour frame AT it


def build_map(d):
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    m = M.Mapper(M.default_params())
    for depth, rgb, T in S.sequence(200, n_frames_in_loop=200):
        m.integrate_depth(depth, T, S.REPLICA_LIKE_CAM); m.integrate_color(rgb, T, S.REPLICA_LIKE_CAM)
    m.synchronize()
    m.save_map(os.path.join(d, "room.nvbx"))
    rng = np.random.default_rng(0); sc = S.Scene(); pts = []
    for i in range(0, 200, 2):          # observed free space: on the camera rays between 20 % and 90 % of the rendered depth
        T = S.trajectory_pose(i).astype(np.float64)
        rays = S.pixel_rays(S.REPLICA_LIKE_CAM).reshape(-1, 3) @ T[:3, :3].T
        t = sc.raycast(T[:3, 3], rays); k = rng.integers(0, len(rays), 3200); k = k[np.isfinite(t[k])][:3072]
        pts.append(T[:3, 3] + rays[k] * (t[k] * rng.uniform(0.2, 0.9, len(k)))[:, None])
    o = np.concatenate(pts)[:307200].astype(np.float32)
    dirs = rng.normal(size=o.shape); dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    np.save(os.path.join(d, "origins.npy"), o); np.save(os.path.join(d, "directions.npy"), dirs)


def timed(fn, seconds, torch):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    calls = max(10, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, calls


def span_us(m, needle):
    p = m.profile()
    ks = [k for k in p if needle in k]
    n = sum(p[k]["count"] for k in ks)
    return (sum(p[k]["total_ms"] for k in ks) * 1e3 / n if n else float("nan")), n


def child(d, seconds, yard_reps):
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    m = M.Mapper(M.default_params()); m.load_map(os.path.join(d, "room.nvbx")); m.set_color_deferral(False); m.synchronize()
    lanes = int(os.environ.get("NVBX_RENDER_LANES", "0") or 0)
    T = S.trajectory_pose(POSE_INDEX)
    rgb = torch.from_numpy(S.render(S.Scene(), T, cam)[1]).cuda()
    o = torch.from_numpy(np.load(os.path.join(d, "origins.npy"))).cuda(); dr = torch.from_numpy(np.load(os.path.join(d, "directions.npy"))).cuda()
    dev = "cuda"
    out4 = (torch.empty((120, 160), device=dev), None, None)
    out1 = (torch.empty((480, 640), device=dev), None, None)
    out1a = (torch.empty((480, 640), device=dev), torch.empty((480, 640, 3), dtype=torch.uint8, device=dev), torch.empty((480, 640, 3), device=dev))
    outr = (torch.empty(len(o), device=dev), torch.empty(len(o), dtype=torch.bool, device=dev), None, None)
    cases = [("view_160x120_depth", 160 * 120, lambda: m.render(T, cam, subsampling=4, color=False, out=out4), lambda: int((out4[0] > 0).sum())),
             ("view_640x480_depth", 640 * 480, lambda: m.render(T, cam, subsampling=1, color=False, out=out1), lambda: int((out1[0] > 0).sum())),
             ("view_640x480_all", 640 * 480, lambda: m.render(T, cam, subsampling=1, out=out1a), lambda: int((out1a[0] > 0).sum())),
             ("rays_307200", len(o), lambda: m.cast_rays(o, dr, out=outr), lambda: int(outr[1].sum()))]
    for name, rays, fn, hits in cases:
        us, calls = timed(fn, seconds, torch)
        rec = {"case": name, "lanes_setting": lanes, "rays": rays, "calls": calls, "us_per_call": round(us, 2), "rays_per_s": round(rays / us * 1e6),
               "hits": hits()}
        if name == "view_160x120_depth":
            # kernel spans of the render launch and of its yardstick, the colour frame's own sphere tracing, in this process
            m.set_profiling(True)
            for _ in range(200):
                fn()
            rec["render_kernel_us"] = round(span_us(m, "k_render")[0], 2)
            m.set_profiling(False)
            yard = []
            for _ in range(max(5, yard_reps)):
                m.set_profiling(True)
                for _ in range(200):
                    m.integrate_color(rgb, T, cam)
                yard.append(round(span_us(m, "k_sphere_trace")[0], 2))
                m.set_profiling(False)
            rec["yardstick_k_sphere_trace_us"] = yard
            rec["yardstick_spread_us"] = round(max(yard) - min(yard), 2)
            sd = m.synthetic_depth()
            rec["equals_synthetic_depth"] = bool(np.array_equal(sd, out4[0].cpu().numpy()))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[0, 8, 4, 2, 1], help="NVBX_RENDER_LANES settings to compare (0 = the library's choice)")
    ap.add_argument("--reps", type=int, default=1, help="alternations over the settings")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--yard-reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--map", default=None, help="directory for the saved map (kept; built only if missing)")
    ap.add_argument("--child", default=None, help="(internal) time one setting on the map in this directory")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.seconds, a.yard_reps)
        return
    d = a.map or tempfile.mkdtemp(prefix="render_bench_")
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(os.path.join(d, "directions.npy")):
        build_map(d)
    lines = []
    for _ in range(a.reps):
        for lanes in a.lanes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d, "--seconds", str(a.seconds), "--yard-reps", str(a.yard_reps)],
                               env=dict(os.environ, NVBX_RENDER_LANES=str(lanes)), capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                sys.exit("render_bench: child with NVBX_RENDER_LANES=%d failed (%d)" % (lanes, r.returncode))
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    print(line, flush=True); lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
