"""Drawn maps for the surface-point and map-registration tests (tests/test_surface_model.py, tests/test_gpu_surface.py), as the block dicts of
tests/surface_independent.py: random fields over chosen blocks, one-crossing blocks, the checkerboard, and the room of planes two mappers are
registered in."""
import numpy as np

import surface_independent as SI

F32 = np.float32
VS = 0.05
TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])


def random_blocks(keys, seed, vs=VS, p_unobserved=0.1, p_nan=0.02, color_keys=(), p_uncoloured=0.3):
    """distances uniform in +-2 voxels, weights 1 but for a drawn share below 1e-4, a few NaN distances; colour where asked"""
    rng = np.random.default_rng(seed)
    out = {}
    for k in keys:
        d = (rng.uniform(-2, 2, (8, 8, 8)) * vs).astype(F32)
        d[rng.random((8, 8, 8)) < p_nan] = np.nan
        w = np.where(rng.random((8, 8, 8)) < p_unobserved, F32(0.5e-4), F32(1.0)).astype(F32)
        out[tuple(k)] = {"d": d, "w": w}
    for k in color_keys:
        b = out.setdefault(tuple(k), {})
        b["rgb"] = rng.integers(1, 256, (8, 8, 8, 3)).astype(np.uint8)
        b["cw"] = np.where(rng.random((8, 8, 8)) < p_uncoloured, F32(0.0), F32(2.0)).astype(F32)
    return out


def one_crossing_block(i):
    """two observed voxels, one edge between them; which edge depends on i"""
    d = np.ones((8, 8, 8), F32); w = np.zeros((8, 8, 8), F32)
    a = i % 7, (i * 3) % 8, (i * 5) % 8          # vx <= 6: the +x neighbour is inside the block
    w[a] = 1.0; w[a[0] + 1, a[1], a[2]] = 1.0
    d[a] = F32(-0.01 - 0.001 * (i % 13)); d[a[0] + 1, a[1], a[2]] = F32(0.02)
    return {"d": d, "w": w}


def checkerboard_block(parity=0):
    vx, vy, vz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    d = np.where(((vx + vy + vz + parity) & 1) == 0, F32(0.03), F32(-0.02)).astype(F32)
    return {"d": d, "w": np.ones((8, 8, 8), F32)}


# ---- the room of planes: a box interior and one slanted plane across a corner
ROOM_HALF = 0.8
ROOM_CUT = 0.9                 # the slanted plane n . x = ROOM_CUT, n = (1, 1, 1) / sqrt 3
ROOM_BAND_VOX = 4.0
ROOM_T = None                  # (set below)


def room_planes():
    """rows (n, c): the room is where c - n . x > 0 for all of them"""
    rows = []
    for a in range(3):
        for s in (1.0, -1.0):
            n = np.zeros(3); n[a] = s
            rows.append((n, ROOM_HALF))
    rows.append((np.ones(3) / np.sqrt(3.0), ROOM_CUT))
    return rows


def room_blocks(T_D_S=None, vs=VS):
    """The room seen from a frame S with p_D = T_D_S p_S (None: the identity), sampled at S's voxel centres in float64: d = the smallest
    c - n . p_D.  A voxel is observed (weight 1) iff |d| <= the band of ROOM_BAND_VOX voxels and every other plane's value is at least the band
    + 4 voxels: two observed voxels that share a cell are then governed by ONE plane (its value grows by at most sqrt 3 vs per cell, the
    others' shrink by as much), so the field is linear wherever a query is valid and the trilinear interpolant is exact."""
    T = np.eye(4) if T_D_S is None else np.asarray(T_D_S, np.float64)
    band = ROOM_BAND_VOX * vs
    nb = int(np.ceil((ROOM_HALF + band + 0.1) / (8 * vs)))
    vx, vy, vz = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    planes = room_planes()
    out = {}
    for bx in range(-nb, nb):
        for by in range(-nb, nb):
            for bz in range(-nb, nb):
                ps = np.stack([(8 * bx + vx + 0.5) * vs, (8 * by + vy + 0.5) * vs, (8 * bz + vz + 0.5) * vs], -1)
                pd = ps @ T[:3, :3].T + T[:3, 3]
                vals = np.stack([c - pd @ n for n, c in planes], -1)
                vals.sort(-1)
                d = vals[..., 0]
                obs = (np.abs(d) <= band) & (vals[..., 1] >= band + 4 * vs)
                if obs.any():
                    out[(bx, by, bz)] = {"d": d.astype(F32), "w": obs.astype(F32)}
    return out


def pose(axis, angle_deg, t):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


ROOM_T = pose([0.3, -0.2, 1.0], 1.5, [0.02, -0.015, 0.0166])      # 3 cm and 1.5 degrees: inside the band of 20 cm
ROOM_ALIGN = dict(max_iterations=12, stop_translation_m=1e-10, stop_rotation_rad=1e-10, min_valid=50)


def dict_get_blocks(blocks):
    """Mapper.get_blocks over a block dict, for tests/query_independent.py"""
    def get(layer, idx):
        idx = np.asarray(idx).reshape(-1, 3)
        out = np.zeros((len(idx), 512), TSDF_DT); found = np.zeros(len(idx), bool)
        for i, k in enumerate(map(tuple, idx.tolist())):
            b = blocks.get(k)
            if b is not None and "d" in b:
                out[i]["distance"] = b["d"].reshape(512); out[i]["weight"] = b["w"].reshape(512); found[i] = True
        return out, found
    return get


def room_model_alignment():
    """The float64 model of tests/align_independent.py on the model's own surface points of the second room, from the identity: -> (its result,
    (translation, angle) distance from ROOM_T, the number of points)"""
    import align_independent as AI
    dst, src = room_blocks(None), room_blocks(ROOM_T)
    pts = SI.surface_rows(src, VS)["points"]
    res = AI.run(AI.full_query(dict_get_blocks(dst), VS, 1e-4), pts, np.eye(4, dtype=F32), ROOM_ALIGN)
    dt, ang, _ = AI.pose_distance(res["T"], ROOM_T)
    return res, (dt, ang), len(pts)
