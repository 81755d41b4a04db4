"""An independent numpy model of change detection (SEMANTICS.md "Change detection"; nvbx_find_changes / nvbx_change_clusters) in float32.

Works on dictionaries {(bx, by, bz): TSDF_DT[512]} of voxels in the order z + 8y + 64x (what Mapper.get_blocks hands out).  The transforms,
the sample positions, the sorted block table and the trilinear rule come from tests/merge_independent.py, another test-side model: the
sample of the reference IS the merge's.  The classes, the nearest rule, the labels, the score, the counters and the status are stated here.
It imports nothing from the product; the component records come from segment_independent."""
import numpy as np

import merge_independent as MI

F32 = np.float32
TSDF_DT = MI.TSDF_DT
OK, EMPTY_MAP, EMPTY_REFERENCE, NO_OVERLAP = 0, 1, 2, 3
APPEARED, REMOVED = 0, 1
TRILINEAR, NEAREST = 0, 1
VOX_LIMIT = 1 << 23                        # addressable voxel indices: [-2^23, 2^23) per axis
LANE_XYZ = MI.LANE_XYZ                     # voxel (x, y, z) of lane t = vx 64 + vy 8 + vz


def classes(d, w, min_weight, free_distance_m, occupied_distance_m):
    """-> (observed, free, occupied) of stored or sampled {d, w}: observed iff w >= min_weight, free iff observed and d > free_distance_m,
    occupied iff observed and d <= occupied_distance_m -- float32 compares, so a NaN d is neither"""
    d = np.asarray(d, F32); w = np.asarray(w, F32)
    with np.errstate(invalid="ignore"):
        obs = w >= F32(min_weight)
        return obs, obs & (d > F32(free_distance_m)), obs & (d <= F32(occupied_distance_m))


def sample_nearest(table, ps, voxel_size, ref_min_weight):
    """the voxel floor(p / vs) per axis in float32 -> (valid, d_ref): valid iff the index is addressable, its block is there and its weight
    >= ref_min_weight"""
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.floor(ps / F32(voxel_size))
        ok = ((n >= -VOX_LIMIT) & (n <= VOX_LIMIT - 1)).all(axis=-1)
    n = np.where(ok[..., None], n, 0.0).astype(np.int64)
    found, rec = table.gather(n)
    with np.errstate(invalid="ignore"):
        valid = ok & found & (rec["weight"] >= F32(ref_min_weight))
    return valid, rec["distance"].astype(F32)


def changes(m_tsdf, ref_tsdf, T_M_R, voxel_size, min_weight=1e-4, ref_min_weight=1e-4, free_distance_m=None, occupied_distance_m=0.0,
            sampling=TRILINEAR, box_vox=None):
    """-> dict: volume {block: (label int32[512], score float32[512])} of the blocks of m with a labelled voxel; per block of m `valid` and
    `d_ref` (bool / float32 [512]; valid only where the voxel is observed and in the box); the result record's fields.
    free_distance_m None or 0: one voxel size.  box_vox: (min x, y, z, max x, y, z) inclusive in global voxel coordinates of m, or None."""
    vs = F32(voxel_size)
    fd = vs if free_distance_m is None or F32(free_distance_m) == 0 else F32(free_distance_m)
    od = F32(occupied_distance_m)
    res = {"volume": {}, "valid": {}, "d_ref": {}, "blocks_scanned": len(m_tsdf), "voxels_compared": 0, "voxels_appeared": 0, "voxels_removed": 0,
           "blocks_changed": 0, "status": OK}
    keys = sorted(m_tsdf)
    if keys:
        table = MI._Table(ref_tsdf, TSDF_DT)
        karr = np.array(keys, np.int64).reshape(-1, 3)
        cur = np.stack([np.asarray(m_tsdf[k], TSDF_DT).reshape(512) for k in keys])
        obs, m_free, m_occ = classes(cur["distance"], cur["weight"], min_weight, fd, od)
        g = 8 * karr[:, None, :] + LANE_XYZ[None]
        inbox = np.ones(obs.shape, bool) if box_vox is None else np.all((g >= np.asarray(box_vox[:3])) & (g <= np.asarray(box_vox[3:])), axis=-1)
        ps = MI.sample_positions(T_M_R, karr, voxel_size)
        with np.errstate(invalid="ignore", over="ignore"):
            if sampling == TRILINEAR:
                valid, d_ref, _, _ = MI.sample(table, ps, voxel_size, ref_min_weight)
            else:
                valid, d_ref = sample_nearest(table, ps, voxel_size, ref_min_weight)
        valid = valid & obs & inbox
        d_ref = np.where(valid, d_ref, F32(0)).astype(F32)
        with np.errstate(invalid="ignore"):                      # a valid sample is classified by the same two thresholds
            r_free = valid & (d_ref > fd); r_occ = valid & (d_ref <= od)
        appeared = m_occ & r_free; removed = m_free & r_occ
        label = np.where(appeared, APPEARED, np.where(removed, REMOVED, -1)).astype(np.int32)
        with np.errstate(invalid="ignore"):
            score = np.where(label >= 0, np.abs(cur["distance"] - d_ref), F32(0)).astype(F32)
        for i, k in enumerate(keys):
            res["valid"][k] = valid[i]; res["d_ref"][k] = d_ref[i]
            if (label[i] >= 0).any():
                res["volume"][k] = (label[i], score[i])
        res["voxels_compared"] = int(valid.sum()); res["voxels_appeared"] = int(appeared.sum()); res["voxels_removed"] = int(removed.sum())
        res["blocks_changed"] = len(res["volume"])
    res["status"] = EMPTY_MAP if not m_tsdf else EMPTY_REFERENCE if not ref_tsdf else NO_OVERLAP if res["voxels_compared"] == 0 else OK
    return res


RESULT_FIELDS = ("blocks_scanned", "voxels_compared", "voxels_appeared", "voxels_removed", "blocks_changed", "status")


def as_lists(volume):
    """{block: (label, score)} -> (block_idx [n, 3] int32, label [n, 512], score [n, 512]) in sorted block order"""
    ks = sorted(volume)
    if not ks:
        return np.zeros((0, 3), np.int32), np.zeros((0, 512), np.int32), np.zeros((0, 512), F32)
    return np.array(ks, np.int32), np.stack([volume[k][0] for k in ks]), np.stack([volume[k][1] for k in ks])


def clusters(volume, connectivity, min_voxels=1, scipy=True):
    """components of the labelled voxels in segment_independent's form: ({lowest voxel: record}, keys [n, 512]) over as_lists(volume);
    scipy.ndimage.label, or the scipy-free union-find"""
    import segment_independent as SI
    idx, lab, sc = as_lists(volume)
    if not len(idx):
        return {}, np.zeros((0, 512), np.int64)
    return (SI.model if scipy else SI.model_union_find)(idx, lab, sc, connectivity, min_voxels)


def labelled_positions(volume, label, voxel_size):
    """centres, float64 metres [n, 3], of the voxels of `volume` that carry `label`"""
    out = [(8 * np.asarray(k, np.int64)[None] + LANE_XYZ[v[0] == label] + 0.5) * float(voxel_size) for k, v in sorted(volume.items())]
    return np.concatenate(out) if out else np.zeros((0, 3))


def move_blocks(tsdf, T, voxel_size, trunc, max_weight=100.0):
    """the blocks of `tsdf` brought into another frame under p_new = T p_old by the merge model into an empty map: {block: TSDF_DT[512]} of the
    blocks that hold a fused voxel"""
    r = MI.merge({}, {}, tsdf, {}, T, voxel_size, trunc, max_weight)
    return {k: v for k, v in r["tsdf"].items() if r["fused"][k].any()}
