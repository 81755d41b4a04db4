"""Child process of tests/test_gpu_resample.py: NVBX_RESAMPLE_GRID is read when a mapper is created; every setting resamples the same hand-made
source into the same pre-filled destinations in a process of its own and saves the maps it got.  Usage: python resample_grid_child.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import merge_independent as MI          # noqa: E402

CASES = {"a": (0.075, 2), "b": (0.2, 4)}      # voxel size of the destination, taps


def blocks(rng, keys, weights, color_weights=(0.0, 1.0, 2.5)):
    t, c = {}, {}
    for k in keys:
        b = np.zeros(512, MI.TSDF_DT)
        b["distance"] = rng.uniform(-0.15, 0.15, 512).astype(np.float32); b["weight"] = rng.choice(np.asarray(weights, np.float32), 512)
        q = np.zeros(512, MI.COLOR_DT)
        for ch in "rgb":
            q[ch] = rng.integers(0, 256, 512)
        q["weight"] = rng.choice(np.asarray(color_weights, np.float32), 512)
        t[k] = b; c[k] = q
    return t, c


def upload(M, m, t, c):
    ks = sorted(t)
    m.set_blocks(M.LAYER_TSDF, np.array(ks, np.int32), np.stack([t[k] for k in ks]))
    m.set_blocks(M.LAYER_COLOR, np.array(ks, np.int32), np.stack([c[k] for k in ks]))


def main(out):
    from isaac_ros_nvblox_amd import mapper as M
    rng = np.random.default_rng(77)
    cube = lambda o, n: [(o[0] + x, o[1] + y, o[2] + z) for x in range(n) for y in range(n) for z in range(n)]      # noqa: E731
    st, sc = blocks(rng, cube((-2, -1, -2), 3), (0.5, 1.0, 3.0))
    for b in st.values():
        b["weight"][rng.random(512) < 0.03] = np.float32(5e-5)      # holes: under min_weight
    dt, dc = blocks(rng, cube((-1, -1, -1), 2), (0.0, 4.6, 5.0))
    src = M.Mapper(M.default_params(), device=0, block_capacity=1 << 8)
    upload(M, src, st, sc)
    T = MI.pose([3, -1, 2], 130.0, [0.37, -0.21, 0.13])
    res = {}
    for name, (vd, taps) in CASES.items():
        dst = M.Mapper(M.default_params(voxel_size=vd), device=0, block_capacity=1 << 8)
        upload(M, dst, dt, dc)
        r = dst.resample_from(src, T, taps=taps)
        res["candidates_" + name] = np.int64(r.candidate_blocks); res["fused_" + name] = np.int64(r.voxels_fused)
        res["record_" + name] = r.buffer.cpu().numpy()
        for layer, tag in ((M.LAYER_TSDF, "tsdf"), (M.LAYER_COLOR, "color")):
            idx = np.asarray(dst.block_indices(layer), np.int32).reshape(-1, 3)
            order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
            v, found = dst.get_blocks(layer, idx[order])
            assert found.all()
            res["%s_idx_%s" % (tag, name)] = idx[order]
            res["%s_%s" % (tag, name)] = np.ascontiguousarray(v).view(np.uint8).reshape(len(idx), -1)
        dst.close()
    src.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
