"""Time of a feature-matching scan (nvbx_match_features) on the bench's room map, beside the composition it replaces.

The room map of the 640x480 loop (synthetic.sequence, every second pose of the 200) is built once per channel count and feature frames (stride 16,
a 30 x 40 grid) are integrated at every eighth of those poses.  Then, for C = 32 and 64 and Q = 1, 32 and 128 random queries, dot metric, with and
without the score matrix: us per scan by the library's own per-launch event spans (set_profiling) and by events on torch's stream around the whole
call; the bytes the scan must move (512 C 2 + 2048 read and 4 KiB written per block, plus 512 Q 4 per block of score matrix where asked for) with
their share of the HBM peak; and, in the same run, the time of today's alternative by the same events on torch's stream: query_features at all
voxel centres of the feature blocks (the points are made beforehand), torch.matmul in f32, then max / argmax over the queries.
One JSON object per line.  Usage: python tools/feature_match_bench.py [--channels 32 64] [--queries 1 32 128] [--calls 50] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12
STRIDE = 16


def span_us(p, needle):
    ks = [k for k in p if needle in k]
    n = sum(p[k]["count"] for k in ks)
    return (sum(p[k]["total_ms"] for k in ks) * 1e3 / n if n else float("nan")), n


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 128])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    frames = [(torch.from_numpy(d).cuda(), T) for d, _, T in (x for i, x in enumerate(S.sequence(200, n_frames_in_loop=200)) if i % 2 == 0)]
    t = np.arange(512)
    off = np.stack([t >> 6, (t >> 3) & 7, t & 7], 1)
    lines = []
    for C in a.channels:
        m = M.Mapper(M.default_params())
        for d, Tf in frames:
            m.integrate_depth(d, Tf, cam)
        m.enable_features(C)
        rng = np.random.default_rng(C)
        for _, Tf in frames[::8]:
            feat = torch.from_numpy(rng.standard_normal((cam[5] // STRIDE, cam[4] // STRIDE, C)).astype(np.float16)).cuda()
            m.integrate_features(feat, Tf, cam, STRIDE)
        idx = m.block_indices(M.LAYER_FEATURE)
        n = len(idx)
        vs = m.params.voxel_size
        pts = torch.from_numpy(((idx[:, None, :].astype(np.float64) * 8 + off[None] + 0.5) * vs).reshape(-1, 3).astype(np.float32)).cuda()
        gathered = torch.empty((n * 512, C), dtype=torch.float16, device="cuda"); gw = torch.empty(n * 512, dtype=torch.float32, device="cuda")
        for Q in a.queries:
            q = torch.from_numpy(rng.standard_normal((Q, C)).astype(np.float16)).cuda()
            qf = q.float().t().contiguous()
            for with_all in (False, True):
                out = (torch.empty((n, 3), dtype=torch.int32, device="cuda"), torch.empty((n, 512), dtype=torch.int32, device="cuda"),
                       torch.empty((n, 512), dtype=torch.float32, device="cuda"),
                       torch.empty((n, 512, Q), dtype=torch.float32, device="cuda") if with_all else None, torch.empty(1, dtype=torch.int64, device="cuda"))

                def scan():
                    m.match_features(q, "dot", 1.0, out=out)

                def composition():
                    m.query_features(pts, out=(gathered, gw))
                    s = torch.matmul(gathered.float(), qf)
                    best, lab = s.max(dim=1)
                    return s, best, lab
                scan_call_us = event_us(torch, scan, a.calls)
                m.set_profiling(True)
                for _ in range(a.calls):
                    scan()
                p = m.profile(); m.set_profiling(False)
                scan_us, cnt = span_us(p, "k_match_features")
                assert int(out[4].item()) == n
                comp_us = event_us(torch, composition, a.calls)
                # the composition's parts, each alone
                gather_us = event_us(torch, lambda: m.query_features(pts, out=(gathered, gw)), a.calls)
                matmul_us = event_us(torch, lambda: torch.matmul(gathered.float(), qf), a.calls)
                s = torch.matmul(gathered.float(), qf)
                argmax_us = event_us(torch, lambda: s.max(dim=1), a.calls)
                del s
                nbytes = n * (512 * C * 2 + 2048 + 4096 + (512 * Q * 4 if with_all else 0))
                rec = {"case": "match_features_room_640x480", "channels": C, "queries": Q, "all_scores": with_all, "metric": "dot", "calls": cnt,
                       "feature_blocks": n, "scan_span_us": round(scan_us, 2), "scan_call_us": round(scan_call_us, 2), "scan_bytes": nbytes,
                       "scan_GBps": round(nbytes / (scan_us * 1e-6) / 1e9, 1), "scan_share_of_hbm_peak": round(nbytes / (scan_us * 1e-6) / HBM_BPS, 4),
                       "composition_us": round(comp_us, 2), "composition_gather_us": round(gather_us, 2), "composition_matmul_f32_us": round(matmul_us, 2),
                       "composition_argmax_us": round(argmax_us, 2), "composition_over_scan_call": round(comp_us / scan_call_us, 2),
                       "scan_not_slower": bool(scan_call_us <= comp_us)}
                line = json.dumps(rec); print(line, flush=True); lines.append(line)
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
