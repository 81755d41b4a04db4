"""What the colour term does to a pose refinement, and what it costs (nvbx_align_depth_color), on tools/align_bench.py's case:
the room map of the 640x480 loop (every second pose of the 200, depth and colour integrated), frame 51 from align_bench's start 3 cm and
1.5 degrees off.

  - the distance from the true pose after 10 and after 40 iterations at color_weight 0, 0.25, 1 and 4 (subsampling 4), with the status, the
    geometric and the colour rmse, and cond(H) of the first linearization;
  - us per accumulate launch with and without the colour term at subsampling 4 and 1, by the library's own per-launch event spans over calls of
    ten working iterations, and us of the whole call by events on torch's stream;
  - with --parent-root DIR (a checkout of the commit before, its library built): the plain align_depth call on this library and on that one in
    alternating child processes, seven runs each in one session; every child imports the package of its own tree and builds the depth-only
    map from the frames this process rendered.
One JSON object per line.  Usage: python tools/align_color_bench.py [--calls 20] [--parent-root DIR] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRAME = 51
WEIGHTS = (0.0, 0.25, 1.0, 4.0)


def rotation_angle(Ra, Rb):
    dR = Ra @ Rb.T
    sk = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.arctan2(np.linalg.norm(sk), (np.trace(dR) - 1.0) / 2.0))


def accumulate_span(m, fn, calls, span_stats):
    m.set_profiling(True)
    for _ in range(calls):
        fn()
    p = m.profile(); m.set_profiling(False)
    acc_us, acc_n = span_stats(p, "k_align_accumulate"); sol_us, sol_n = span_stats(p, "k_align_solve")
    return round(acc_us / max(acc_n, 1), 2), round(sol_us / max(sol_n, 1), 2), [acc_n, sol_n]


def plain_child(a):
    """the plain align_depth call on whichever library the process loaded: one JSON line"""
    import torch
    from align_bench import event_us, perturbed, span_stats          # (helpers only; it puts this tree first on sys.path)
    if a.root:
        sys.path.insert(0, os.path.abspath(a.root))                  # ... and the package comes from the tree that is measured
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    assert not a.root or os.path.abspath(M.__file__).startswith(os.path.abspath(a.root)), M.__file__
    cam = S.REPLICA_LIKE_CAM
    fr = np.load(a.frames)
    m = M.Mapper(M.default_params())
    for d, T in zip(fr["depth"], fr["pose"]):
        m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
    m.synchronize()
    depth = torch.from_numpy(fr["frame_depth"]).cuda()
    T0 = perturbed(fr["frame_pose"], np.random.default_rng(1))
    buf = torch.empty(M.ALIGN_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    rec = {"case": "plain_align_depth", "library": a.tag}
    for s in (4, 1):
        res = m.align_depth(depth, T0, cam, out=buf, subsampling=s)
        rec["s%d_iterations" % s] = res.iterations
        rec["s%d_call_us" % s] = round(event_us(torch, lambda: m.align_depth(depth, T0, cam, out=buf, subsampling=s), a.calls), 2)
        acc, sol, _ = accumulate_span(m, lambda: m.align_depth(depth, T0, cam, out=buf, subsampling=s), a.calls, span_stats)
        rec["s%d_accumulate_span_us" % s] = acc; rec["s%d_solve_span_us" % s] = sol
    m.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built, for the alternating comparison of the plain call")
    ap.add_argument("--root", default=None, help="(internal) the tree a --plain-child imports the package from")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--plain-child", action="store_true", help="(internal) one run of the plain call over --frames")
    ap.add_argument("--frames", default=None)
    ap.add_argument("--tag", default="this")
    a = ap.parse_args()
    if a.plain_child:
        return plain_child(a)
    import torch
    from align_bench import event_us, perturbed, span_stats
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    m = M.Mapper(M.default_params())
    depths, poses = [], []
    for i, (d, rgb, T) in enumerate(S.sequence(200, n_frames_in_loop=200, color=True)):
        if i % 2 == 0:
            m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
            m.integrate_color(torch.from_numpy(rgb).cuda(), T, cam)
            depths.append(d); poses.append(np.asarray(T, np.float32))
    m.flush(); m.synchronize()
    T_true = np.asarray(S.trajectory_pose(FRAME), np.float64)
    depth_np, rgb_np = S.render(S.Scene(), T_true, cam)
    depth = torch.from_numpy(depth_np).cuda(); rgb = torch.from_numpy(rgb_np).cuda()
    T0 = perturbed(T_true, np.random.default_rng(1))
    lines = []

    def emit(rec):
        line = json.dumps(rec); print(line, flush=True); lines.append(line)

    def distance(res):
        return (round(float(np.linalg.norm(res.T64[:3, 3] - T_true[:3, 3])), 5), round(float(np.rad2deg(rotation_angle(res.T64[:3, :3], T_true[:3, :3]))), 4))
    d0 = (round(float(np.linalg.norm(T0[:3, 3].astype(np.float64) - T_true[:3, 3])), 5), round(float(np.rad2deg(rotation_angle(T0[:3, :3].astype(np.float64), T_true[:3, :3]))), 4))
    # 1. where the refinement ends, by weight
    for w in WEIGHTS:
        rec = {"case": "align_depth_color_room_640x480_frame51", "subsampling": 4, "color_weight": w, "start_error_m_deg": d0}
        for k in (10, 40):
            res = m.align_depth_color(depth, rgb, T0, cam, subsampling=4, max_iterations=k, color_weight=w)
            if k == 10:
                rec.update({"cond_H_first": round(float(np.linalg.cond(res.H_first)), 1), "n_valid": res.n_valid_first, "n_color": res.n_color_first,
                            "rmse_first_m": round(res.rmse_first, 5), "color_rmse_first_levels": round(res.color_rmse_first, 3)})
            t, r = distance(res)
            rec["after_%d" % k] = {"status": res.status_name, "iterations": res.iterations, "translation_error_m": t, "rotation_error_deg": r,
                                   "rmse_last_m": round(res.rmse_last, 5), "color_rmse_last_levels": round(res.color_rmse_last, 3),
                                   "last_step_m": float(np.linalg.norm(res.step[:3])), "last_step_rad": float(np.linalg.norm(res.step[3:]))}
        emit(rec)
    plain = m.align_depth(depth, T0, cam, subsampling=4, max_iterations=40)
    t, r = distance(plain)
    emit({"case": "align_depth_room_640x480_frame51", "subsampling": 4, "after_40": {"status": plain.status_name, "iterations": plain.iterations,
                                                                                   "translation_error_m": t, "rotation_error_deg": r}})
    # 2. what the term costs: ten working iterations per call (stop thresholds 0: no call ends early), the same launches with and without colour
    buf = torch.empty(M.ALIGN_RESULT_BYTES, dtype=torch.uint8, device="cuda"); cbuf = torch.empty(M.ALIGN_COLOR_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    for s in (4, 1):
        kw = dict(subsampling=s, max_iterations=10, stop_translation_m=0.0, stop_rotation_rad=0.0)
        calls = {"plain": lambda: m.align_depth(depth, T0, cam, out=buf, **kw),
                 "color": lambda: m.align_depth_color(depth, rgb, T0, cam, out=cbuf, color_weight=1.0, **kw)}
        rec = {"case": "accumulate_cost", "subsampling": s, "pixels": int(depth[::s, ::s].numel()), "iterations_per_call": 10}
        for name, fn in calls.items():
            res = fn()
            assert res.iterations == 10, (name, res.iterations, res.status_name)
            rec[name + "_call_us"] = round(event_us(torch, fn, a.calls), 2)
            acc, sol, n = accumulate_span(m, fn, a.calls, span_stats)
            rec[name + "_accumulate_span_us"] = acc; rec[name + "_solve_span_us"] = sol; rec[name + "_spans_counted"] = n
        emit(rec)
    m.close()
    # 3. the plain call on this library and on the parent's, alternating
    if a.parent_root:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "frames.npz")
            np.savez(path, depth=np.stack(depths), pose=np.stack(poses), frame_depth=depth_np, frame_pose=T_true)
            for run in range(a.runs):
                for tag, root in (("parent", a.parent_root), ("this", ROOT)):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--frames", path, "--tag", tag, "--calls", str(a.calls),
                                          "--root", root], capture_output=True, text=True, timeout=300)
                    if out.returncode != 0:
                        sys.stderr.write(out.stderr[-2000:])
                        raise SystemExit("the %s child of run %d failed with %d" % (tag, run, out.returncode))
                    rec = json.loads(out.stdout.strip().splitlines()[-1]); rec["run"] = run
                    emit(rec)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
