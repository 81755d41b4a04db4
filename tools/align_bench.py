"""Time of a pose refinement (nvbx_align_depth) on the bench's room map, beside the composition a caller builds from the
calls the library already had.

The room map of the 640x480 loop (synthetic.sequence, every second pose of the 200) is built once.  One frame between two map poses is
aligned from a start 3 cm and 1.5 degrees off, at subsampling 4 (19 200 pixels) and 1 (307 200 pixels), max_iterations 10:
  - us per accumulate launch and per solve launch by the library's own per-launch event spans (set_profiling), over a call whose max_iterations
    is the number of iterations the refinement takes, so only working launches are counted;
  - us of the whole call by events on torch's stream, with all ten iterations enqueued (the launches behind the final status return at once)
    and with the working ones only;
  - in the same run, today's composition by the same events: backproject_depth once (it waits for the stream), then per iteration
    nvbx_transform_pointcloud, query_tsdf, the 29 sums in torch float64, a copy to the host, a numpy solve and the next pose from the host --
    for as many iterations as the library's run took;
  - untimed, what the refinement does on this frame with 40 iterations, looser stop thresholds, a Huber threshold, a depth limit and damping.
One JSON object per line.  Usage: python tools/align_bench.py [--calls 20] [--out FILE]
Counters: rocprofv3 --pmc COUNTERS --output-format csv -d DIR -- python tools/align_bench.py --child (a run of its own; the accumulate launches of the two
subsamplings differ by their grid size, 19 200 and 65 536 work-items)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAME = 51


def span_stats(p, needle):
    ks = [k for k in p if needle in k]
    n = sum(p[k]["count"] for k in ks)
    return (sum(p[k]["total_ms"] for k in ks) * 1e3, n)


def event_us(torch, fn, calls):
    """mean us of fn() by events on torch's current stream (the mapper's calls are ordered behind and ahead of it)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


# (hat, exp_so3 and perturbed restate formulas that tests/align_independent.py and csrc/nvbx_align_math.h have too: on purpose -- a tool imports
#  nothing from tests/, and the composition must not call the code it is compared with)
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_so3(w):
    t2 = float(w @ w); th = np.sqrt(t2)
    if th < 1e-8:
        A, B, Cc = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    else:
        A, B, Cc = np.sin(th) / th, 2.0 * np.sin(th / 2) ** 2 / t2, (th - np.sin(th)) / (t2 * th)
    K = hat(w); K2 = np.outer(w, w) - t2 * np.eye(3)
    return np.eye(3) + A * K + B * K2, np.eye(3) + B * K + Cc * K2


def perturbed(T, rng):
    dt = rng.normal(size=3); dt *= 0.03 / np.linalg.norm(dt)
    ax = rng.normal(size=3); ax *= np.deg2rad(1.5) / np.linalg.norm(ax)
    out = np.asarray(T, np.float64).copy()
    out[:3, :3] = exp_so3(ax)[0] @ out[:3, :3]; out[:3, 3] += dt
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="only the map and five calls per subsampling: the program to put behind `rocprofv3 --pmc ... --`")
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    m = M.Mapper(M.default_params())
    for i, (d, _, T) in enumerate(S.sequence(200, n_frames_in_loop=200, color=False)):
        if i % 2 == 0:
            m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
    m.synchronize()
    T_true = S.trajectory_pose(FRAME)
    depth_np, _ = S.render(S.Scene(), T_true, cam, color=False)
    depth = torch.from_numpy(depth_np).cuda()
    T0 = perturbed(T_true, np.random.default_rng(1))
    if a.child:
        for s in (4, 1):
            for _ in range(5):
                m.align_depth(depth, T0, cam, subsampling=s)
        m.synchronize(); m.close()
        return
    buf = torch.empty(M.ALIGN_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    lines = []
    for s in (4, 1):
        res = m.align_depth(depth, T0, cam, out=buf, subsampling=s)
        iters, status, n_valid = res.iterations, res.status_name, res.n_valid
        err_t = float(np.linalg.norm(res.T64[:3, 3] - T_true[:3, 3].astype(np.float64)))
        step = res.step
        # how the refinement behaves on this frame beyond the ten iterations, and under the options made for outliers: status, iterations, distance
        # from the true pose, the last step (one device-to-host copy each; not timed)
        behaviour = {}
        for name, kw in (("max_iterations_40", dict(max_iterations=40)), ("stop_1e-4", dict(max_iterations=40, stop_translation_m=1e-4, stop_rotation_rad=1e-4)),
                         ("huber_0.02", dict(max_iterations=40, huber_delta_m=0.02)), ("max_depth_2.5", dict(max_iterations=40, max_depth_m=2.5)),
                         ("damping_1e-2", dict(max_iterations=40, damping=1e-2))):
            rb = m.align_depth(depth, T0, cam, subsampling=s, **kw)
            behaviour[name] = {"status": rb.status_name, "iterations": rb.iterations, "n_valid": rb.n_valid,
                               "translation_error_m": round(float(np.linalg.norm(rb.T64[:3, 3] - T_true[:3, 3].astype(np.float64))), 5),
                               "last_step_m": float(np.linalg.norm(rb.step[:3])), "last_step_rad": float(np.linalg.norm(rb.step[3:])),
                               "rmse_first": round(rb.rmse_first, 5), "rmse_last": round(rb.rmse_last, 5)}
        call_us = event_us(torch, lambda: m.align_depth(depth, T0, cam, out=buf, subsampling=s), a.calls)
        work_us = event_us(torch, lambda: m.align_depth(depth, T0, cam, out=buf, subsampling=s, max_iterations=iters), a.calls)
        m.set_profiling(True)              # (spans of the working launches only: max_iterations = the iterations the run takes)
        for _ in range(a.calls):
            m.align_depth(depth, T0, cam, out=buf, subsampling=s, max_iterations=iters)
        p = m.profile(); m.set_profiling(False)
        acc_us, acc_n = span_stats(p, "k_align_accumulate"); sol_us, sol_n = span_stats(p, "k_align_solve")
        # the composition: the points once, then the iterations with a host solve each
        masked = torch.zeros_like(depth); masked[::s, ::s] = depth[::s, ::s]
        pts = torch.empty((depth.numel(), 3), dtype=torch.float32, device="cuda"); cnt = C.c_int64()

        def points_once():
            m._check(m.lib.nvbx_backproject_depth(m._h, C.c_void_p(masked.data_ptr()), depth.shape[0], depth.shape[1], C.byref(m._cam(cam)), 0.0,
                                                  C.c_void_p(pts.data_ptr()), pts.shape[0], C.byref(cnt)))
            return pts[:cnt.value]
        x = points_once()
        pl = torch.empty_like(x)
        out = (torch.empty(len(x), dtype=torch.float32, device="cuda"), torch.empty((len(x), 3), dtype=torch.float32, device="cuda"),
               torch.empty(len(x), dtype=torch.bool, device="cuda"))

        def composition():
            xs = points_once()
            T = T0.astype(np.float64)
            for _ in range(iters):
                Tf = np.ascontiguousarray(T.astype(np.float32))
                m._around_torch_stream(lambda: m.lib.nvbx_transform_pointcloud(m._h, Tf.ctypes.data_as(C.c_void_p), C.c_void_p(xs.data_ptr()), len(xs),
                                                                               C.c_void_p(pl.data_ptr())))
                d_, g_, v_ = m.query_tsdf(pl, min_weight=1e-4, unknown_value=0.0, out=out)
                w = v_.double()
                q = pl.double() - torch.from_numpy(Tf[:3, 3].astype(np.float64)).cuda()
                g64 = g_.double()
                J = torch.cat([g64, torch.linalg.cross(q, g64)], 1) * w[:, None]
                r = d_.double() * w
                H = (J.t() @ J).cpu().numpy(); b = (J.t() @ r).cpu().numpy()      # (the host waits here, every iteration)
                xi = np.linalg.solve(H, -b)
                R, V = exp_so3(xi[3:])
                T[:3, :3] = R @ T[:3, :3]; T[:3, 3] += V @ xi[:3]
            return T
        T_comp = composition()
        comp_us = event_us(torch, composition, max(a.calls // 4, 3))
        rec = {"case": "align_depth_room_640x480", "subsampling": s, "pixels": int(depth[::s, ::s].numel()), "n_valid": n_valid, "status": status,
               "iterations": iters, "max_iterations": 10, "translation_error_m": round(err_t, 5),
               "accumulate_span_us": round(acc_us / max(acc_n, 1), 2), "solve_span_us": round(sol_us / max(sol_n, 1), 2), "spans_counted": [acc_n, sol_n],
               "call_working_launches_only_us": round(work_us, 2),
               "call_us": round(call_us, 2), "composition_us": round(comp_us, 2), "composition_over_call": round(comp_us / call_us, 2),
               "composition_pose_difference_m": float(np.linalg.norm(T_comp[:3, 3] - res.T64[:3, 3])),
               "last_step_m": float(np.linalg.norm(step[:3])), "last_step_rad": float(np.linalg.norm(step[3:])), "behaviour": behaviour}
        line = json.dumps(rec); print(line, flush=True); lines.append(line)
    m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
