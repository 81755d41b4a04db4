"""CPU checks of the point queries: the float64 model (tests/query_independent.py) on hand-made blocks with exact expectations, and
that the C header, the façade header and the device helpers still compile (nothing here needs a GPU)."""
import os
import subprocess

import numpy as np
import pytest

import query_independent as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
ESDF_DT = np.dtype([("squared_distance_vox", "<f4"), ("parent_direction", "<i4", (3,)),
                    ("is_inside", "u1"), ("observed", "u1"), ("is_site", "u1"), ("pad", "u1")])
VS = 0.0625          # a power of two: voxel centres and block faces are exact in f32


class FakeLayer:
    """get_blocks over a dict {block index: 512 voxels in the reference order z + 8y + 64x}"""

    def __init__(self, dt):
        self.dt, self.blocks = dt, {}

    def get_blocks(self, layer, idx):
        out = np.zeros((len(idx), 512), self.dt); found = np.zeros(len(idx), bool)
        for r, k in enumerate(map(tuple, np.asarray(idx))):
            if k in self.blocks:
                out[r] = self.blocks[k]; found[r] = True
        return out, found


def linear_tsdf(blocks, slope, offset, weight=1.0):
    f = FakeLayer(TSDF_DT)
    for bi in blocks:
        v = np.zeros(512, TSDF_DT)
        x, y, z = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")       # [x][y][z] -> z + 8y + 64x
        g = (np.stack([x, y, z], -1) + 8 * np.asarray(bi)).reshape(-1, 3)
        centre = (g + 0.5) * VS
        v["distance"] = (centre @ np.asarray(slope) + offset).astype(np.float32)
        v["weight"] = weight
        f.blocks[tuple(bi)] = v
    return f


ALL = [(x, y, z) for x in (-2, -1, 0, 1) for y in (-2, -1, 0, 1) for z in (-2, -1, 0, 1)]


def test_linear_field_is_reproduced_with_its_slope():
    slope = np.array([0.25, -0.5, 0.125]); f = linear_tsdf(ALL, slope, 0.125)
    rng = np.random.default_rng(3)
    p = rng.uniform(-1.5 * 8 * VS, 1.5 * 8 * VS, (2000, 3)).astype(np.float32)
    d, g, ok = Q.query(f.get_blocks, Q.LAYER_TSDF, p, VS, min_weight=0.5)
    assert ok.all()
    np.testing.assert_allclose(d, p.astype(np.float64) @ slope + 0.125, atol=1e-6)
    np.testing.assert_allclose(g, np.broadcast_to(slope, g.shape), atol=1e-6)


def test_voxel_centres_block_faces_and_negative_coordinates():
    slope = np.array([1.0, 2.0, -3.0]); f = linear_tsdf(ALL, slope, 0.0)
    # voxel centres (t = 0 exactly): the voxel's own value; block faces (b & 7 == 7 on every axis): 8 blocks
    pts = np.array([[(-9 + 0.5) * VS, (3 + 0.5) * VS, (-1 + 0.5) * VS], [0.0, 0.0, 0.0], [-8 * VS, -8 * VS, -8 * VS],
                    [8 * VS, -8 * VS, 8 * VS]], np.float32)
    d, g, ok = Q.query(f.get_blocks, Q.LAYER_TSDF, pts, VS)
    assert ok.all()
    np.testing.assert_allclose(d, pts.astype(np.float64) @ slope, atol=1e-12)
    assert list(Q.corner_block_counts(pts, VS)) == [4, 8, 8, 8]      # (a voxel centre still has the corners b + 1: -9 and -1 end a block)
    b, t, _ = Q.corner_coordinates(pts, VS)
    assert b[0].tolist() == [-9, 3, -1] and t[0].tolist() == [0.0, 0.0, 0.0]
    assert b[1].tolist() == [-1, -1, -1] and t[1].tolist() == [0.5, 0.5, 0.5]


def test_one_missing_or_under_weight_corner_makes_the_point_invalid():
    slope = np.array([1.0, 0.0, 0.0]); f = linear_tsdf(ALL, slope, 0.0)
    p = np.array([[0.0, 0.0, 0.0]], np.float32)           # corners (-1..0)^3: 8 blocks
    assert Q.query(f.get_blocks, Q.LAYER_TSDF, p, VS, min_weight=0.5)[2].all()
    blk = f.blocks[(0, -1, 0)].copy(); f.blocks[(0, -1, 0)]["weight"][0 + 8 * 7 + 64 * 0] = 0.25      # corner (0, -1, 0)
    d, g, ok = Q.query(f.get_blocks, Q.LAYER_TSDF, p, VS, min_weight=0.5, unknown_value=7.0)
    assert not ok[0] and d[0] == 7.0 and (g[0] == 0).all()
    assert Q.query(f.get_blocks, Q.LAYER_TSDF, p, VS, min_weight=0.25)[2][0]          # weight >= min_weight counts
    f.blocks[(0, -1, 0)] = blk; del f.blocks[(-1, -1, -1)]
    assert not Q.query(f.get_blocks, Q.LAYER_TSDF, p, VS)[2][0]


def test_esdf_plane_ignores_z_and_signs_inside_voxels():
    f = FakeLayer(ESDF_DT)
    for bi in [(x, y, 1) for x in (-1, 0) for y in (-1, 0)]:
        v = np.zeros(512, ESDF_DT)
        x, y, z = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
        gx = (x + 8 * bi[0]).reshape(-1)
        v["squared_distance_vox"] = (gx.astype(np.float64) ** 2).astype(np.float32)
        v["is_inside"] = gx < 0; v["observed"] = 1
        f.blocks[bi] = v
    # distance = +-|gx| * VS = gx * VS (a linear field in x through the voxel centres' indices)
    p = np.array([[0.3 * VS, 0.7 * VS, z] for z in (-5.0, 0.0, 123.0)], np.float32)
    d, g, ok = Q.query(f.get_blocks, Q.LAYER_ESDF, p, VS, plane=9)
    assert ok.all() and np.ptp(d) == 0 and np.ptp(g, axis=0).max() == 0
    np.testing.assert_allclose(d, (0.3 - 0.5) * VS, atol=1e-12)
    np.testing.assert_allclose(g[0], [1.0, 0.0, 0.0], atol=1e-12)
    assert not Q.query(f.get_blocks, Q.LAYER_ESDF, p, VS, plane=20)[2].any()       # plane in no block
    assert not Q.query(f.get_blocks, Q.LAYER_ESDF, p, VS)[2].any()                  # 3-D: z corners absent


def test_points_beyond_the_addressable_range_are_invalid():
    f = linear_tsdf([(0, 0, 0)], [0, 0, 0], 0.0)
    p = np.array([[2.0 ** 23 * VS, 0, 0], [-(2.0 ** 23 + 2) * VS, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], np.float32)
    assert not Q.query(f.get_blocks, Q.LAYER_TSDF, p, VS)[2].any()
    assert Q.plane_vz(0.09, 0.05) == 1 and Q.plane_vz(-0.01, 0.05) == -1


def test_device_helpers_cross_compile(tmp_path):
    """a caller's kernel using nvbx_dev_interpolate_* builds for gfx950 (hipcc -c; no GPU needed)"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is missing")
    src = tmp_path / "helpers.hip"
    src.write_text(r'''
#include "nvblox_hip_device.h"
__global__ void k(nvbx_device_view v, const float* p, int n, float* d, float* g, uint8_t* ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ok[i] = nvbx_dev_interpolate_tsdf(v, p + 3 * i, 0.1f, 1000.0f, &d[2 * i], g + 3 * i);
  ok[i] |= nvbx_dev_interpolate_esdf(v, p + 3 * i, 1, 1000.0f, &d[2 * i + 1], nullptr) << 1;
}
''')
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + INC, "-c",
                           str(src), "-o", str(tmp_path / "helpers.o")])


def test_c_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "nvblox_hip_device.h"\nint main(void) { int (*f)(nvbx_mapper*, uint32_t, const float*, int64_t, float, float, float*, float*, uint8_t*) = nvbx_query_points; (void)f; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + INC, "-c", str(src), "-o", str(tmp_path / "c99.o")])


def test_interpolator_facade_compiles_with_gxx(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text(r'''
#include "nvblox/interpolation/interpolation_3d.h"
#include "nvblox/nvblox.h"
void f(const nvblox::TsdfLayer& t, const nvblox::EsdfLayer& e, const float* p_dev, float* d_dev, float* g_dev, uint8_t* v_dev) {
  nvblox::Interpolator in;
  std::vector<nvblox::Vector3f> pts{{0.f, 0.f, 0.f}};
  std::vector<float> d; std::vector<bool> ok;
  in.interpolateOnGPU(pts, t, &d, &ok);
  in.interpolateOnGPU(pts, e, &d, &ok);
  in.interpolateOnGPU(p_dev, 1, t, d_dev, g_dev, v_dev);
  in.interpolateOnGPU(p_dev, 1, e, d_dev, nullptr, nullptr);
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I" + INC, "-I/opt/rocm/include",
                           "-c", str(src), "-o", str(tmp_path / "facade.o")])
