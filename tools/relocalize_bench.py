"""Time of a relocalisation (nvbx_relocalize_depth) on the bench's room map, beside the composition a caller builds from the
calls the library already had.

The room map of the 640x480 loop (every second pose of the 200) is built once.  One frame between two map poses, at subsampling 8
(4 800 pixels), is searched for in lattices of 256, 4 096 and 32 768 poses over +-0.4 m and +-20 degrees, centred 0.3 m and 15 degrees off
the truth:
  - us of the scoring launch by the library's own per-launch event spans (set_profiling) over score_poses calls on the lattice's poses (one
    launch per call), trilinear queries per second = poses x taken pixels / span, and the launch's least bytes -- the TSDF voxels of the
    blocks the transformed points' base corners fall into, once, plus the taken pixels once -- over span as a share of the HBM peak;
  - the same span with the points never split (one workgroup per pose, plain stores) and always split (a workgroup per 256 points, atomics):
    the A/B behind the launch's choice (NVBX_SCORE_CHUNKS);
  - us of the selection launch by the same spans, and of the whole relocalize_depth call by events on torch's stream;
  - in the same run, today's composition by the same events: a torch [K, n, 3] transform, query_tsdf over it, torch reductions and an arg-max,
    a copy of the winner to the host, then align_depth from it;
  - query_tsdf's own rate on as many uniform points inside the room.
One JSON object per line.  Usage: python tools/relocalize_bench.py [--calls 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAME = 51
SUBSAMPLING = 8
HBM_PEAK = 8.0e12
LATTICES = ((256, (8, 8, 1, 4)), (4096, (16, 16, 1, 16)), (32768, (32, 32, 2, 16)))
HALF_EXTENT, HALF_YAW = (0.4, 0.4, 0.1), float(np.deg2rad(20.0))


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


def off_centre(T, metres=0.3, degrees=15.0):
    yaw = np.deg2rad(degrees); c, s = np.cos(yaw), np.sin(yaw)
    out = np.asarray(T, np.float64).copy()
    out[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ out[:3, :3]
    out[:3, 3] += metres * np.array([np.cos(1.0), np.sin(1.0), 0.0])
    return out.astype(np.float32)


def score_span_us(m, fn, calls):
    for _ in range(3):
        fn()
    m.synchronize()
    m.set_profiling(True)
    for _ in range(calls):
        fn()
    p = m.profile(); m.set_profiling(False)
    us, n = span_stats(p, "k_score_poses")
    return us / max(n, 1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    m = M.Mapper(M.default_params())
    scene = S.Scene()
    for i in range(0, 200, 2):
        T = S.trajectory_pose(i)
        d, _ = S.render(scene, T, cam, color=False)
        m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
        if i % 50 == 0:
            print("# map frame %d" % i, flush=True)
    m.synchronize()
    vs = float(m.params.voxel_size)
    T_true = S.trajectory_pose(FRAME)
    depth_np, _ = S.render(scene, T_true, cam, color=False)
    depth = torch.from_numpy(depth_np).cuda()
    T0 = off_centre(T_true)
    # the taken pixels as a cloud, for the composition and the block count (the library back-projects inside its launches)
    masked = np.zeros_like(depth_np); masked[::SUBSAMPLING, ::SUBSAMPLING] = depth_np[::SUBSAMPLING, ::SUBSAMPLING]
    x = torch.from_numpy(m.backproject_depth(masked, cam)).cuda()
    n = int(x.shape[0])
    buf = torch.empty(M.RELOC_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    lines = []
    for K, steps in LATTICES:
        poses = torch.from_numpy(m.search_lattice(T0, HALF_EXTENT, HALF_YAW, steps)).cuda()
        assert poses.shape[0] == K
        rec_out = torch.empty((K, 3), dtype=torch.int64, device="cuda")
        kw = dict(subsampling=SUBSAMPLING)
        res = m.relocalize_depth(depth, T0, cam, HALF_EXTENT, HALF_YAW, steps, score=kw, align=kw, out=buf)
        status, best, coarse, refined = res.status_name, res.best_index, tuple(res.coarse), tuple(res.refined)
        a_status, a_iters = res.align.status_name, res.align.iterations
        err_t = float(np.linalg.norm(res.align.T64[:3, 3] - T_true[:3, 3].astype(np.float64)))
        score = lambda: m.score_poses(depth, poses, cam=cam, out=rec_out, **kw)
        # (the span is the kernel's; the call by events also holds the memset that zeroes the records of a split launch)
        # (a mapper keeps the knobs it last read: reload_knobs after each change of the environment)
        os.environ.pop("NVBX_SCORE_CHUNKS", None); m.reload_knobs()
        span_us, spans = score_span_us(m, score, a.calls); score_call_us = event_us(torch, score, a.calls)
        try:
            os.environ["NVBX_SCORE_CHUNKS"] = "1"; m.reload_knobs()
            whole_us, _ = score_span_us(m, score, a.calls); whole_call_us = event_us(torch, score, a.calls)
            os.environ["NVBX_SCORE_CHUNKS"] = "1024"; m.reload_knobs()
            split_us, _ = score_span_us(m, score, a.calls); split_call_us = event_us(torch, score, a.calls)
        finally:
            os.environ.pop("NVBX_SCORE_CHUNKS", None); m.reload_knobs()
        # the blocks the launch must read at least: the base corners' blocks of every transformed point, a pose chunk at a time
        keys = []
        for lo in range(0, K, 1024):
            P = poses[lo:lo + 1024].reshape(-1, 4, 4)
            p = torch.einsum("kij,nj->kni", P[:, :3, :3], x) + P[:, None, :3, 3]
            b = torch.floor(p / vs - 0.5).to(torch.int64) >> 3
            keys.append(torch.unique(((b[..., 0] + (1 << 20)) << 42) | ((b[..., 1] + (1 << 20)) << 21) | (b[..., 2] + (1 << 20))))
            del p, b
        blocks = int(torch.unique(torch.cat(keys)).numel())
        least_bytes = blocks * 512 * 8 + n * 4
        reloc = lambda: m.relocalize_depth(depth, T0, cam, HALF_EXTENT, HALF_YAW, steps, score=kw, align=kw, out=buf)
        call_us = event_us(torch, reloc, a.calls)
        m.set_profiling(True)
        for _ in range(a.calls):
            reloc()
        p = m.profile(); m.set_profiling(False)
        sel_us, sel_n = span_stats(p, "k_select_pose")

        def composition():
            P = poses.reshape(-1, 4, 4)
            pts = (torch.einsum("kij,nj->kni", P[:, :3, :3], x) + P[:, None, :3, 3]).reshape(-1, 3)
            d_, _, v_ = m.query_tsdf(pts, min_weight=1e-4, unknown_value=0.0)
            d_ = d_.reshape(K, n); v_ = v_.reshape(K, n)
            inl = (v_ & (d_.abs() <= vs)).sum(1); con = (v_ & (d_ > 2.0 * vs)).sum(1)
            h = int(torch.argmax(inl - con).item())                       # (the host waits here)
            return h, m.align_depth(depth, poses[h].reshape(4, 4).cpu().numpy(), cam, subsampling=SUBSAMPLING)
        h_comp, r_comp = composition()
        comp_us = event_us(torch, composition, max(a.calls // 4, 3))
        # query_tsdf alone, on as many uniform points inside the room
        g = torch.Generator(device="cuda"); g.manual_seed(K)
        rnd = torch.rand((K * n, 3), generator=g, device="cuda") * torch.tensor([6.0, 5.0, 3.0], device="cuda") + torch.tensor([-3.0, -2.5, 0.0], device="cuda")
        qout = (torch.empty(K * n, dtype=torch.float32, device="cuda"), None, None)
        query = lambda: m.query_tsdf(rnd, min_weight=1e-4, unknown_value=0.0, out=qout)
        query_us = event_us(torch, query, max(a.calls // 4, 3))
        del rnd, qout
        queries = K * coarse[0]
        rec = {"case": "relocalize_depth_room_640x480", "poses": K, "steps": list(steps), "subsampling": SUBSAMPLING, "taken_pixels": coarse[0],
               "status": status, "best_index": best, "coarse": list(coarse), "align_status": a_status, "align_iterations": a_iters,
               "refined": list(refined), "translation_error_m": round(err_t, 5),
               "score_span_us": round(span_us, 2), "spans_counted": spans, "queries_per_s": round(queries / (span_us * 1e-6), 0),
               "score_span_never_split_us": round(whole_us, 2), "score_span_always_split_us": round(split_us, 2),
               "score_call_us": round(score_call_us, 2), "score_call_never_split_us": round(whole_call_us, 2),
               "score_call_always_split_us": round(split_call_us, 2),
               "touched_blocks": blocks, "least_bytes": least_bytes, "least_bytes_share_of_hbm_peak": round(least_bytes / (span_us * 1e-6) / HBM_PEAK, 5),
               "select_span_us": round(sel_us / max(sel_n, 1), 2), "call_us": round(call_us, 2),
               "composition_us": round(comp_us, 2), "composition_over_call": round(comp_us / call_us, 2),
               "composition_intermediate_bytes": K * n * 12, "composition_best_index": h_comp,
               "composition_pose_difference_m": float(np.linalg.norm(r_comp.T64[:3, 3] - res.align.T64[:3, 3])),
               "query_tsdf_points": K * n, "query_tsdf_us": round(query_us, 2), "query_tsdf_points_per_s": round(K * n / (query_us * 1e-6), 0)}
        line = json.dumps(rec); print(line, flush=True); lines.append(line)
        del poses, rec_out
        torch.cuda.empty_cache()
    m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
