"""Shared helpers of the tests: seeded input sequences, the HIP mapper against the CPU oracle within the contract's tolerances (make_pair,
compare_layer, check_all), and two mappers -- or one mapper before and after a call -- holding the same map bit for bit (map_state,
assert_same_map; tests/test_map_compare.py tests these two on the CPU)."""
import numpy as np

from isaac_ros_nvblox_amd import mapper as M, synthetic as S

SMALL_CAM = (80.0, 80.0, 79.5, 59.5, 160, 120)      # 160x120, same 90 deg HFOV as the 640x480 camera


def frames(n, cam=S.REPLICA_LIKE_CAM, start=0, color=True, stride=1, **kw):
    sc = S.Scene()

    def one(i):
        T = S.trajectory_pose(start + i * stride, 200, **kw)
        d, rgb = S.render(sc, T, cam, color=color)
        return (d, rgb, T)
    if n >= 16:          # (numpy releases the GIL in the ray casts: long sequences render on a few threads)
        import os
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            return list(pool.map(one, range(n)))
    return [one(i) for i in range(n)]


def idx_set(a):
    return set(map(tuple, np.asarray(a).reshape(-1, 3).tolist()))


def copy_params(src, dst_cls):
    dst = dst_cls()
    for name, _ in dst_cls._fields_:
        setattr(dst, name, getattr(src, name))
    return dst


def short(name):
    import bench
    return bench.short(name)


# ---- the HIP mapper against the CPU oracle, within the contract's tolerance
TOL = 1e-4


def make_pair(oracle_mod, **kw):
    from isaac_ros_nvblox_amd import mapper as M
    pg = M.default_params(**kw)
    po = copy_params(pg, oracle_mod.OrcParams)
    return M, M.Mapper(pg, block_capacity=1 << 14), oracle_mod.OracleMap(po)


def compare_layer(M, g, o, layer_g, layer_o, fields_exact=(), fields_tol=(), lsb_fields=()):
    ig = g.block_indices(layer_g); io = o.block_indices(layer_o)
    assert idx_set(ig) == idx_set(io), "block index sets differ: only-gpu %s only-oracle %s" % (
        sorted(idx_set(ig) - idx_set(io))[:5], sorted(idx_set(io) - idx_set(ig))[:5])
    assert np.array_equal(ig, io)            # both sorted lexicographically
    bg, found = g.get_blocks(layer_g, ig)
    assert found.all()
    worst = 0.0
    for k, idx in enumerate(io):
        bo = o.get_block(layer_o, idx)
        for f in fields_exact:
            assert np.array_equal(bg[k][f], bo[f]), (f, idx)
        for f in fields_tol:
            d = np.abs(bg[k][f].astype(np.float64) - bo[f].astype(np.float64)).max()
            worst = max(worst, d)
            assert d <= TOL, (f, idx, d)
        for f in lsb_fields:
            d = np.abs(bg[k][f].astype(np.int32) - bo[f].astype(np.int32)).max()
            assert d <= 1, (f, idx, d)
    return len(io), worst


def compare_occupancy(M, g, o, oracle_mod):
    ig = g.block_indices(M.LAYER_OCCUPANCY); io = o.block_indices(oracle_mod.L_TSDF)
    assert np.array_equal(ig, io), (len(ig), len(io))
    bg, found = g.get_blocks(M.LAYER_OCCUPANCY, ig)
    assert found.all()
    for k, idx in enumerate(io):
        assert np.array_equal(bg[k]["log_odds"], o.get_block(oracle_mod.L_TSDF, idx)["distance"]), idx     # adds and compares only: bit-exact
    return len(io), bg


def check_all(M, oracle_mod, g, o, mesh=True):
    compare_layer(M, g, o, M.LAYER_TSDF, oracle_mod.L_TSDF, fields_tol=("distance", "weight"))
    compare_layer(M, g, o, M.LAYER_COLOR, oracle_mod.L_COLOR, fields_tol=("weight",), lsb_fields=("r", "g", "b"))
    assert idx_set(g.block_indices(M.LAYER_ESDF)) == idx_set(o.block_indices(oracle_mod.L_ESDF))
    if len(o.block_indices(oracle_mod.L_ESDF)):
        sg, ag = g.esdf_slice_image(); so, ao = o.esdf_slice_image()
        assert sg.shape == so.shape and np.abs(sg - so).max() <= TOL and np.allclose(ag, ao, atol=1e-6)
    if mesh:
        mg = g.mesh()
        n_tri = 0
        for idx in o.block_indices(oracle_mod.L_TSDF):
            mo = o.mesh_block(idx)
            a = mg.get(tuple(idx))
            if a is None:
                assert mo is None or len(mo["triangles"]) == 0, idx
                continue
            assert np.array_equal(a["triangles"], mo["triangles"]), idx
            if len(mo["vertices"]):
                assert np.abs(a["vertices"] - mo["vertices"]).max() <= TOL
            n_tri += len(mo["triangles"])
        return n_tri
    return 0


# ---- two mappers hold the same map, bit for bit
ESDF_FIELDS = ("squared_distance_vox", "parent_direction", "is_inside", "observed", "is_site")
LAYER_FIELDS = {M.LAYER_TSDF: M.TSDF_DT, M.LAYER_COLOR: M.COLOR_DT, M.LAYER_ESDF: M.ESDF_DT, M.LAYER_OCCUPANCY: M.OCCUPANCY_DT,
                M.LAYER_FREESPACE: M.FREESPACE_DT}
DEFAULT_LAYERS = (M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF)
LAYER_NAMES = {M.LAYER_TSDF: "tsdf", M.LAYER_COLOR: "color", M.LAYER_ESDF: "esdf", M.LAYER_OCCUPANCY: "occupancy",
               M.LAYER_FREESPACE: "freespace", M.LAYER_FEATURE: "feature"}


def _read_layer(m, layer):
    idx = np.asarray(m.block_indices(layer), np.int32).reshape(-1, 3)
    if layer == M.LAYER_FEATURE:
        f, w, found = m.feature_blocks(idx)
        blocks = np.zeros(w.shape, np.dtype([("features", f.dtype, f.shape[2:]), ("weight", w.dtype)]))
        blocks["features"] = f; blocks["weight"] = w
    else:
        blocks, found = m.get_blocks(layer, idx)
    assert np.all(found), ("layer %s: a block that block_indices lists was not found" % LAYER_NAMES[layer], idx[~np.asarray(found, bool)][:5].tolist())
    return idx, np.asarray(blocks).reshape(len(idx), 512)


def _read_slice(m):
    img, aabb = m.esdf_slice_image()
    return np.asarray(img), np.asarray(aabb)


def _read_mesh(m):
    return {k: (np.asarray(v["vertices"]), np.asarray(v["triangles"])) for k, v in m.mesh().items()}


def map_state(m, layers=None, slice=False, mesh=False):
    """One mapper read back into plain numpy: per layer the index array as block_indices returned it (not sorted) and every voxel of those
    blocks; on request the ESDF slice (image, AABB) and the mesh of the last update (per block: vertices, triangles).  The feature layer, read
    through feature_blocks, is held as voxels of (features, weight).  Nothing in the result changes when the mapper goes on working: every read
    call of a mapper returns arrays of its own, so nothing is copied here."""
    state = {"layers": {layer: _read_layer(m, layer) for layer in layers or DEFAULT_LAYERS}}
    if slice:
        state["slice"] = _read_slice(m)
    if mesh:
        state["mesh"] = _read_mesh(m)
    return state


def _raw(a):
    """the bytes of every element: [..., itemsize] uint8"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


def _same_bytes(a, b):
    """two arrays of one shape and type hold the same bytes (compared in the widest words their size allows)"""
    a, b = (np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in (a, b))
    word = next(w for w in (np.uint64, np.uint32, np.uint16, np.uint8) if a.size % np.dtype(w).itemsize == 0)
    return np.array_equal(a.view(word), b.view(word))


def _any_per_voxel(x):
    """[n, 512, ...] -> [n, 512]"""
    return x.reshape(x.shape[:2] + (-1,)).any(-1) if x.size else np.zeros(x.shape[:2], bool)


def _float_fields(dt, names):
    return [f for f in names if dt[f].base.kind == "f"]


def block_difference(idx, a, b, fields=None):
    """Where two read-backs [n, 512] of the blocks `idx` first differ in the bytes of a field (all fields, `pad` included, unless named): the
    block, the field and the first few differing voxels (z + 8y + 64x) with both values.  None if they do not differ."""
    a = np.asarray(a).reshape(-1, 512); b = np.asarray(b).reshape(-1, 512)
    if a.shape != b.shape or (fields is None and a.dtype != b.dtype):
        return "read-backs of %s %s and of %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
    if fields is None and _same_bytes(a, b):
        return None
    for f in fields or a.dtype.names:
        bad = _any_per_voxel(_raw(a[f]) != _raw(b[f]))
        if bad.any():
            k = int(np.argmax(bad.any(1)))
            v = np.nonzero(bad[k])[0][:4]
            return "block %s, field %s, voxels %s: %s vs %s (%d voxels of %d blocks differ in this field)" % (
                tuple(np.asarray(idx[k]).tolist()), f, v.tolist(), a[k][f][v].tolist(), b[k][f][v].tolist(), int(bad.sum()), int(bad.any(1).sum()))
    return None


def _nan_report(idx, blocks, fields):
    for f in _float_fields(blocks.dtype, fields or blocks.dtype.names):
        if blocks.size and np.isnan(blocks[f].min()):                   # (the minimum of an array that holds a NaN is NaN)
            bad = _any_per_voxel(np.isnan(blocks[f]))
            k = int(np.argmax(bad.any(1)))
            return "block %s, field %s, voxels %s hold a NaN" % (tuple(idx[k].tolist()), f, np.nonzero(bad[k])[0][:4].tolist())
    return None


def array_difference(a, b):
    """first element at which two arrays differ in shape, type or bits, both values; NaNs count as a difference from anything"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "%s %s vs %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
    bad = (_raw(a) != _raw(b)).any(-1)
    if a.dtype.kind == "f":
        bad |= np.isnan(a) | np.isnan(b)
    if not bad.any():
        return None
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return "element %s: %s vs %s" % (at, a[at].tolist(), b[at].tolist())


def assert_same_map(a, b, tag="", layers=None, fields=None, min_blocks=None, slice=False, mesh=False):
    """Two mappers or two states (map_state), or one of each, hold the same map bit for bit: per layer the same index array in the same order, the
    same voxel bytes (`pad` included) and no NaN in a float field on either side; slice and mesh, where asked for and where both states have
    them, equal in every bit.  A mapper is read here, one layer at a time (a whole map of each side at once is memory the tests need not hold).
    fields = {layer: names} narrows a layer to those fields; min_blocks (a number, or {layer: number}): every compared layer holds at least that
    many blocks.  A failure names the tag, the layer and the blocks only one side has, or the block, field, voxels and values."""
    for given in (x for x in (a, b) if isinstance(x, dict)):      # a mapper beside a state is read as that state was
        layers, slice, mesh = layers or tuple(given["layers"]), "slice" in given, "mesh" in given

    def both(part, read):
        return [(x[part] if part in x else None) if isinstance(x, dict) else read(x) for x in (a, b)]
    where = ("%s: " % (tag,)) if tag != "" else ""
    for layer in layers or DEFAULT_LAYERS:
        name = where + "layer " + LAYER_NAMES[layer]
        (ia, va), (ib, vb) = [x["layers"][layer] if isinstance(x, dict) else _read_layer(x, layer) for x in (a, b)]
        if not np.array_equal(ia, ib):
            only_a, only_b = sorted(idx_set(ia) - idx_set(ib)), sorted(idx_set(ib) - idx_set(ia))
            if only_a or only_b:
                raise AssertionError("%s: %d and %d blocks, only in the first %s, only in the second %s" % (name, len(ia), len(ib), only_a[:5], only_b[:5]))
            k = int(np.argmax((ia != ib).any(1)))
            raise AssertionError("%s: the same %d blocks in another order, position %d holds %s and %s" % (name, len(ia), k, ia[k].tolist(), ib[k].tolist()))
        need = min_blocks.get(layer, 0) if isinstance(min_blocks, dict) else (min_blocks or 0)
        assert len(ia) >= need, "%s: %d blocks, at least %d are wanted" % (name, len(ia), need)
        names = (fields or {}).get(layer)
        for v in (va, vb):
            nan = _nan_report(ia, v, names)
            assert nan is None, "%s: %s" % (name, nan)
        diff = block_difference(ia, va, vb, names)
        assert diff is None, "%s: %s" % (name, diff)
    sa, sb = both("slice", _read_slice) if slice else (None, None)
    if sa is not None and sb is not None:
        for what, x, y in zip(("slice image, pixel (row, column)", "slice AABB"), sa, sb):
            diff = array_difference(x, y)
            assert diff is None, "%s%s: %s" % (where, what, diff)
    ma, mb = both("mesh", _read_mesh) if mesh else (None, None)
    if ma is not None and mb is not None:
        assert ma.keys() == mb.keys(), "%smesh: %d and %d blocks, on one side only %s" % (where, len(ma), len(mb), sorted(set(ma) ^ set(mb))[:5])
        for k in ma:
            for what, x, y in zip(("vertex", "triangle"), ma[k], mb[k]):
                diff = array_difference(x, y)
                assert diff is None, "%smesh block %s, %s: %s" % (where, k, what, diff)
