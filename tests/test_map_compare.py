"""tests/helpers.py map_state / assert_same_map on a stand-in mapper backed by dicts: equal maps pass; a missing block, another order, one flipped bit in
any field of any layer (`pad` included), a NaN shared by both sides, a slice pixel, the slice AABB, a mesh vertex, a listed block that is not found and
too few blocks all fail, and the failure names what was planted."""
import copy

import numpy as np
import pytest

import helpers as H
from helpers import M

BLOCKS = [(0, 0, 0), (0, 1, -2), (3, 0, 1)]
PLANT_BLOCK, PLANT_VOXEL = (0, 1, -2), 3 + 8 * 5 + 64 * 2
ALL_LAYERS = tuple(H.LAYER_FIELDS)
FIELDS = [(layer, f) for layer in ALL_LAYERS for f in H.LAYER_FIELDS[layer].names]


class DictMapper:
    """block_indices / get_blocks / esdf_slice_image / mesh of a mapper, over dicts a test can edit; like a mapper's, every call returns new arrays"""

    def __init__(self, seed=1):
        rng = np.random.default_rng(seed)
        self.order = {layer: list(BLOCKS) for layer in ALL_LAYERS}
        self.blocks = {}
        for layer, dt in H.LAYER_FIELDS.items():
            for b in BLOCKS:
                v = np.zeros(512, dt)
                for f in dt.names:
                    v[f] = rng.standard_normal(v[f].shape) if dt[f].base.kind == "f" else rng.integers(0, 100, v[f].shape)
                self.blocks[layer, b] = v
        self.hidden = set()                      # (layer, block): listed, but get_blocks does not find it
        self.slice = (rng.standard_normal((6, 9)).astype(np.float32), np.arange(6, dtype=np.float32))
        self.meshes = {b: dict(vertices=rng.standard_normal((7, 3)).astype(np.float32), triangles=np.arange(6, dtype=np.int32).reshape(2, 3),
                               normals=np.zeros((7, 3), np.float32), colors=np.zeros((7, 4), np.uint8)) for b in BLOCKS[:2]}

    def block_indices(self, layer):
        return np.array(self.order[layer], np.int32).reshape(-1, 3)

    def get_blocks(self, layer, indices):
        keys = [tuple(i) for i in np.asarray(indices).reshape(-1, 3).tolist()]
        out = np.zeros((len(keys), 512), H.LAYER_FIELDS[layer]); found = np.zeros(len(keys), bool)
        for k, b in enumerate(keys):
            if (layer, b) in self.blocks and (layer, b) not in self.hidden:
                out[k] = self.blocks[layer, b]; found[k] = True
        return out, found

    def esdf_slice_image(self):
        return self.slice[0].copy(), self.slice[1].copy()

    def mesh(self):
        return copy.deepcopy(self.meshes)

    def flip_bit(self, layer, field):
        raw = self.blocks[layer, PLANT_BLOCK][field][PLANT_VOXEL:PLANT_VOXEL + 1].view(np.uint8)      # (a view: the block itself changes)
        raw[0] ^= 1


@pytest.fixture()
def pair():
    a = DictMapper()
    return a, copy.deepcopy(a)


def fails(a, b, *named, **kw):
    with pytest.raises(AssertionError) as e:
        H.assert_same_map(a, b, "planted", **kw)
    msg = str(e.value)
    for n in ("planted",) + named:
        assert str(n) in msg, (n, msg)
    return msg


def test_equal_maps_pass_as_mappers_states_or_one_of_each(pair):
    a, b = pair
    H.assert_same_map(a, b)
    H.assert_same_map(a, b, layers=ALL_LAYERS, min_blocks=3, slice=True, mesh=True)
    sa = H.map_state(a, ALL_LAYERS, slice=True, mesh=True)
    H.assert_same_map(sa, H.map_state(b, ALL_LAYERS, slice=True, mesh=True))
    H.assert_same_map(sa, b); H.assert_same_map(b, sa)
    assert set(sa["layers"]) == set(ALL_LAYERS) and set(H.map_state(a)["layers"]) == {M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF}
    assert "slice" not in H.map_state(a) and "mesh" not in H.map_state(a)


def test_a_state_does_not_follow_the_mapper(pair):
    a, b = pair
    before = H.map_state(a, slice=True, mesh=True)
    a.flip_bit(M.LAYER_TSDF, "weight"); a.slice[0][0, 0] += 1; a.meshes[BLOCKS[0]]["vertices"][0, 0] += 1; a.order[M.LAYER_ESDF].reverse()
    H.assert_same_map(before, b)
    fails(before, a, "layer tsdf")


@pytest.mark.parametrize("side", [0, 1])
def test_a_block_on_one_side_only(pair, side):
    a, b = pair
    pair[side].order[M.LAYER_COLOR].remove(PLANT_BLOCK)
    msg = fails(a, b, "layer color", PLANT_BLOCK, "only in the %s [(0, 1, -2)]" % ("second", "first")[side])
    assert "3 and 2" in msg or "2 and 3" in msg


def test_the_same_blocks_in_another_order(pair):
    a, b = pair
    b.order[M.LAYER_ESDF] = [BLOCKS[0], BLOCKS[2], BLOCKS[1]]
    fails(a, b, "layer esdf", "another order", "position 1", list(BLOCKS[1]), list(BLOCKS[2]))


@pytest.mark.parametrize("layer,field", FIELDS, ids=["%s-%s" % (H.LAYER_NAMES[l], f) for l, f in FIELDS])
def test_one_flipped_bit_in_any_field(pair, layer, field):
    a, b = pair
    b.flip_bit(layer, field)
    va, vb = a.blocks[layer, PLANT_BLOCK][field][PLANT_VOXEL], b.blocks[layer, PLANT_BLOCK][field][PLANT_VOXEL]
    fails(a, b, "layer " + H.LAYER_NAMES[layer], "block %s" % (PLANT_BLOCK,), "field %s," % field, "voxels [%d]" % PLANT_VOXEL, "%s vs %s" % ([va.tolist()], [vb.tolist()]),
          layers=ALL_LAYERS)
    if field == "pad":                           # fields= narrows a layer to the named fields: the only way past a difference in `pad`
        H.assert_same_map(a, b, layers=ALL_LAYERS, fields={layer: [f for f in H.LAYER_FIELDS[layer].names if f != "pad"]})
        fails(a, b, "field pad", layers=ALL_LAYERS, fields={layer: ["pad"]})


@pytest.mark.parametrize("layer,field", [(l, f) for l, f in FIELDS if H.LAYER_FIELDS[l][f].base.kind == "f"])
def test_a_nan_at_the_same_voxel_on_both_sides(pair, layer, field):
    a, b = pair
    for m in (a, b):
        m.blocks[layer, PLANT_BLOCK][field][PLANT_VOXEL] = np.nan
    assert a.blocks[layer, PLANT_BLOCK].tobytes() == b.blocks[layer, PLANT_BLOCK].tobytes()
    fails(a, b, "layer " + H.LAYER_NAMES[layer], "block %s" % (PLANT_BLOCK,), "field %s," % field, "voxels [%d]" % PLANT_VOXEL, "NaN", layers=ALL_LAYERS)


def test_slice_and_mesh(pair):
    a, b = pair
    H.assert_same_map(a, b, slice=True, mesh=True)
    b.slice[0][4, 7] = np.nextafter(b.slice[0][4, 7], np.float32(9))
    fails(a, b, "slice image", "(4, 7)", "%s vs %s" % (a.slice[0][4, 7].tolist(), b.slice[0][4, 7].tolist()), slice=True)
    H.assert_same_map(a, b, mesh=True)                                    # (not asked for: not compared)
    a, b = DictMapper(), DictMapper()
    b.slice[1][5] += 1
    fails(a, b, "slice AABB", "(5,)", "5.0 vs 6.0", slice=True)
    a, b = DictMapper(), DictMapper()
    b.meshes[BLOCKS[1]]["vertices"][6, 2] *= 2
    fails(a, b, "mesh block %s" % (BLOCKS[1],), "vertex", "(6, 2)", mesh=True)
    a, b = DictMapper(), DictMapper()
    b.meshes[BLOCKS[0]]["triangles"][1, 0] = 0
    fails(a, b, "mesh block %s" % (BLOCKS[0],), "triangle", "(1, 0)", "3 vs 0", mesh=True)
    a, b = DictMapper(), DictMapper()
    del b.meshes[BLOCKS[1]]
    fails(a, b, "mesh", BLOCKS[1], mesh=True)
    a, b = DictMapper(), DictMapper()
    for m in (a, b):
        m.meshes[BLOCKS[0]]["vertices"][2, 1] = np.nan                    # equal bits, and still no pass
    fails(a, b, "mesh block %s" % (BLOCKS[0],), "(2, 1)", mesh=True)


def test_a_listed_block_that_is_not_found(pair):
    a, b = pair
    b.hidden.add((M.LAYER_TSDF, PLANT_BLOCK))
    for read in (lambda: H.assert_same_map(a, b), lambda: H.map_state(b)):
        with pytest.raises(AssertionError) as e:
            read()
        assert "layer tsdf" in str(e.value) and "not found" in str(e.value) and str(list(PLANT_BLOCK)) in str(e.value), str(e.value)


def test_min_blocks(pair):
    a, b = pair
    H.assert_same_map(a, b, min_blocks=3); H.assert_same_map(a, b, min_blocks={M.LAYER_COLOR: 3})
    fails(a, b, "layer tsdf", "3 blocks", "at least 4", min_blocks=4)
    fails(a, b, "layer color", "at least 4", min_blocks={M.LAYER_COLOR: 4})
    for m in (a, b):
        for layer in ALL_LAYERS:
            m.order[layer] = []
    H.assert_same_map(a, b, layers=ALL_LAYERS)                            # two empty maps are equal ...
    fails(a, b, "layer tsdf", "0 blocks", min_blocks=1)                   # ... and pass no guard
