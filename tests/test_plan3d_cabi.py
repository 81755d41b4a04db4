"""The cost-volume entry points exist: libnvblox_hip.so exports them, the ctypes mirror carries them with the header's argument lists, the
Python methods are there with their defaults, and the host-only helpers (voxel lists, metres to voxels) do what they say.  No compute calls."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nvblox_hip.h")
NAMES = {"nvbx_cost_volume": 10, "nvbx_trace_paths_3d": 12}


def test_library_exports_the_cost_volume_calls(hip_lib):
    for s in NAMES:
        assert hasattr(hip_lib, s), "libnvblox_hip.so does not export %s" % s


def test_ctypes_mirror_carries_the_calls_with_the_headers_argument_lists():
    from isaac_ros_nvblox_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for s, n_args in NAMES.items():
        assert s in _lib.SIGNATURES, "ctypes mirror lacks %s" % s
        res, args = _lib.SIGNATURES[s]
        decl = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S)
        assert decl, "the header does not declare %s" % s
        params = [p.strip() for p in decl.group(2).split(",")]
        assert res is C.c_int and decl.group(1) == "int" and len(args) == len(params) == n_args, s
        for p, a in zip(params, args):
            if "nvbx_cost_options" in p:
                assert a == C.POINTER(_lib.CostOptions), (s, p, a)
            elif "*" in p:
                assert a is C.c_void_p, (s, p, a)                       # a pointer
            else:
                assert a is kinds[p.split()[0]], (s, p, a)               # a scalar of the header's type
    names = [p.split()[-1].lstrip("*") for p in re.search(r"nvbx_cost_volume\s*\((.*?)\)", txt, flags=re.S).group(1).split(",")]
    assert names == ["m", "volume_dev", "nx", "ny", "nz", "options", "sources_xyz_dev", "n_sources", "cost_dev", "accepted_dev"]
    names = [p.split()[-1].lstrip("*") for p in re.search(r"nvbx_trace_paths_3d\s*\((.*?)\)", txt, flags=re.S).group(1).split(",")]
    assert names == ["m", "volume_dev", "nx", "ny", "nz", "options", "cost_dev", "starts_xyz_dev", "n_starts", "path_xyz_dev", "capacity", "length_dev"]


def test_python_mapper_has_the_methods_and_their_defaults():
    from isaac_ros_nvblox_amd import mapper as M
    for name in ("cost_volume", "trace_paths_3d", "esdf_dense_grid_device", "volume_voxels", "esdf_dense_grid", "cost_options"):
        assert callable(getattr(M.Mapper, name, None)), name
    p = inspect.signature(M.Mapper.cost_volume).parameters
    assert list(p)[1:3] == ["volume_dev", "sources_xyz"] and p["out"].default is None and p["accepted"].default is None
    assert p["options"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(M.Mapper.trace_paths_3d).parameters
    assert list(p)[1:5] == ["volume_dev", "field", "starts_xyz", "capacity"] and p["out"].default is None and p["options"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(M.Mapper.esdf_dense_grid_device).parameters
    assert list(p)[1:] == ["min_vox", "size_vox", "default_value", "out"] and p["out"].default is None
    assert list(inspect.signature(M.Mapper.volume_voxels).parameters)[1:] == ["points_xyz", "min_vox"]
    assert list(inspect.signature(M.Mapper.esdf_dense_grid).parameters)[1:] == ["min_vox", "size_vox", "default_value"]      # unchanged


def test_voxel_lists_are_coerced_like_pixel_lists():
    import torch
    from isaac_ros_nvblox_amd import _args
    cpu = torch.device("cpu")
    v = _args.voxels3([(1, 2, 3), (4, 5, 6)], cpu)
    assert v.dtype == torch.int32 and tuple(v.shape) == (2, 3) and v.is_contiguous() and v.tolist() == [[1, 2, 3], [4, 5, 6]]
    assert tuple(_args.voxels3(np.zeros((0, 3), np.int64), cpu).shape) == (0, 3)
    t = torch.arange(12, dtype=torch.int32).reshape(3, 4)[:, :3]
    assert _args.voxels3(t, cpu).is_contiguous() and _args.voxels3(t, cpu).tolist() == t.tolist()
    for bad in (torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32), torch.zeros(6, dtype=torch.int32)):
        with pytest.raises(ValueError):
            _args.voxels3(bad, cpu, "sources_xyz")


def test_volume_voxels_is_floor_of_metres_over_the_voxel_size_minus_the_box_corner():
    from isaac_ros_nvblox_amd import mapper as M

    class Stub:                                                         # the method reads the voxel size only: no mapper, no device
        params = M.default_params()
    vs = np.float32(Stub.params.voxel_size)
    pts = np.array([(0.0, 0.0, 0.0), (0.051, -0.001, 1.5), (-0.05, 0.0499, 0.1), (3.2, -3.2, 0.3)], np.float32)
    got = M.Mapper.volume_voxels(Stub, pts, (-8, 0, 4))
    want = np.floor(pts / vs).astype(np.int64) - np.array([-8, 0, 4])
    assert got.dtype == np.int32 and got.shape == (4, 3) and np.array_equal(got, want)
    assert got[0].tolist() == [8, 0, -4] and got[1].tolist() == [9, -1, 26]
