"""Throughput of the interpolated point queries (nvbx_query_points).

The room map of the 640x480 200-pose loop (synthetic.sequence) is built once, for a 3-D ESDF mapper and a default 2-D one, and saved;
the maps are then loaded and the queries timed with device events over >= --seconds of back-to-back calls after warm-up:
  layers: TSDF (3-D mapper), ESDF 3-D, ESDF 2-D;  distributions: coherent (4 096 clusters of points in 0.5 m boxes in the observed
  free space, cluster after cluster) and uniform (over the map's block AABB);  n = 2^20 and 2^24.
One JSON object per case: queries/s, us per call, the algorithmic bytes (12 B in + 17 B out per point + the distinct 8-B corner voxels
of allocated blocks + 16 B per hash probe, one probe per distinct corner block of a point) and their share of 8 TB/s, and the share of
points whose corners lie in 1 / 2 / 4 / 8 blocks.
Usage: python tools/query_bench.py [--n 20 24] [--out FILE] [--maps DIR]
(a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/query_bench.py --maps DIR --n 20, DIR holding the maps of an earlier run)"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VS = 0.05
HBM_BPS = 8e12


def build_maps(d):
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    ms = {"3d": M.Mapper(M.default_params(esdf_mode=1)), "2d": M.Mapper(M.default_params())}
    for depth, rgb, T in S.sequence(200, n_frames_in_loop=200):
        for m in ms.values():
            m.integrate_depth(depth, T, S.REPLICA_LIKE_CAM); m.integrate_color(rgb, T, S.REPLICA_LIKE_CAM)
    for name, m in ms.items():
        m.update_esdf(); m.synchronize()
        m.save_map(os.path.join(d, name + ".nvbx"))
    # coherent cluster centres: points on the camera rays between 20 % and 80 % of the rendered depth (observed free space)
    rng = np.random.default_rng(0); sc = S.Scene(); cent = []
    for i in range(0, 200, 4):
        T = S.trajectory_pose(i).astype(np.float64)
        rays = S.pixel_rays(S.REPLICA_LIKE_CAM).reshape(-1, 3) @ T[:3, :3].T
        t = sc.raycast(T[:3, 3], rays); k = rng.integers(0, len(rays), 200); k = k[np.isfinite(t[k])][:90]
        cent.append(T[:3, 3] + rays[k] * (t[k] * rng.uniform(0.2, 0.8, len(k)))[:, None])
    np.save(os.path.join(d, "centres.npy"), np.concatenate(cent)[:4096].astype(np.float32))


def points(kind, n, m, centres, torch):
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    if kind == "coherent":
        c = torch.from_numpy(centres).cuda()
        per = (n + len(c) - 1) // len(c)
        p = c.repeat_interleave(per, 0)[:n] + (torch.rand((n, 3), device="cuda", generator=g) - 0.5) * 0.5
    else:
        bi = m.block_indices(1)
        lo = torch.tensor(bi.min(0) * 8 * VS, dtype=torch.float32, device="cuda")
        hi = torch.tensor((bi.max(0) + 1) * 8 * VS, dtype=torch.float32, device="cuda")
        p = lo + torch.rand((n, 3), device="cuda", generator=g) * (hi - lo)
    return p.contiguous()


def algorithmic(p, m, plane, torch):
    """(bytes, share of points with 1/2/4/8 corner blocks)"""
    u = p / VS - 0.5
    b = torch.floor(u).to(torch.int64)
    if plane is not None:
        b[:, 2] = plane
    cross = (b & 7) == 7
    if plane is not None:
        cross[:, 2] = False
    nb = 1 << cross.sum(1)
    share = {str(k): float((nb == k).double().mean()) for k in (1, 2, 4, 8)}
    alloc = torch.from_numpy(m.block_indices(1).astype(np.int64)).cuda()
    B = 1 << 21
    akey = torch.sort(((alloc[:, 0] + B) * B + alloc[:, 1] + B) * B + alloc[:, 2] + B).values
    vox = 0
    for k in range(4 if plane is not None else 8):
        c = b + torch.tensor([k & 1, (k >> 1) & 1, k >> 2], device="cuda")
        blk = c >> 3
        key = ((blk[:, 0] + B) * B + blk[:, 1] + B) * B + blk[:, 2] + B
        pos = torch.searchsorted(akey, key).clamp(max=len(akey) - 1)
        live = akey[pos] == key
        ck = ((c[live, 0] + (1 << 23)) << 48) | ((c[live, 1] + (1 << 23)) << 24) | (c[live, 2] + (1 << 23))
        vox = torch.cat([vox, ck]) if torch.is_tensor(vox) else ck
    n_vox = int(torch.unique(vox).numel()) if torch.is_tensor(vox) else 0
    probes = int(nb.sum())
    return len(p) * (12 + 17) + 8 * n_vox + 16 * probes, share


def measure(d, ns, seconds):
    lines = []
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    ms = {}
    for name, mode in (("3d", 1), ("2d", 0)):
        m = M.Mapper(M.default_params(esdf_mode=mode)); m.load_map(os.path.join(d, name + ".nvbx")); m.update_esdf(); m.synchronize()
        ms[name] = m
    centres = np.load(os.path.join(d, "centres.npy"))
    plane2 = int(np.floor(np.float32(ms["2d"].params.esdf_slice_height) / np.float32(VS)))
    for logn in ns:
        n = 1 << logn
        for kind in ("coherent", "uniform"):
            for case, mname, layer, plane in (("tsdf", "3d", 1, None), ("esdf3d", "3d", 4, None), ("esdf2d", "2d", 4, plane2)):
                m = ms[mname]
                p = points(kind, n, m, centres, torch)
                d_ = torch.empty(n, device="cuda"); g_ = torch.empty((n, 3), device="cuda"); v_ = torch.empty(n, dtype=torch.bool, device="cuda")
                q = (lambda: m.query_tsdf(p, out=(d_, g_, v_))) if layer == 1 else (lambda: m.query_esdf(p, out=(d_, g_, v_)))
                for _ in range(5):
                    q()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); q(); e1.record(); torch.cuda.synchronize()
                calls = max(10, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
                e0.record()
                for _ in range(calls):
                    q()
                e1.record(); torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / calls
                nbytes, share = algorithmic(p, m, plane, torch)
                lines.append(json.dumps({"case": case, "dist": kind, "n": n, "calls": calls, "us_per_call": round(us, 2),
                                         "queries_per_s": round(n / us * 1e6), "valid": round(float(v_.float().mean()), 4),
                                         "alg_bytes": nbytes, "alg_frac_8TBs": round(nbytes / (us * 1e-6) / HBM_BPS, 4),
                                         "corner_blocks_share": share}))
                print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20, 24], help="log2 of the point counts")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--maps", default=None, help="directory for the saved maps (kept; built only if missing)")
    a = ap.parse_args()
    d = a.maps or tempfile.mkdtemp(prefix="query_bench_")
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(os.path.join(d, "centres.npy")):
        build_maps(d)
    lines = measure(d, a.n, a.seconds)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
