"""csrc/nvbx_knobs.h: the NVBX_* environment knobs of the launch geometry and the A/B switches, compiled from the shipped header with gcc and checked on
the CPU.  A missing, malformed or out-of-range value must give the default: a knob that yields a zero grid or zero riders drops work (NVBX_EDT_RIDERS=0
never ran a held-back distance transform, NVBX_DECAY_GRID=0 made every k_decay workgroup a table-clearing rider); a negative one was cast to unsigned for
the launch.  Rider counts come out as multiples of 8.  And every read of these knobs in the library goes through the header."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")

FUNCS = ("integ_grid", "color_grid", "edt_riders", "pair_b_edt_riders", "mark_riders", "mark_tiles_first", "decay_grid", "st_lanes",
         "fused_trace_lanes", "lidar_sparse_grid", "color_deferral", "switch")


@pytest.fixture(scope="module")
def knobs(tmp_path_factory):
    d = tmp_path_factory.mktemp("knobs")
    src = d / "knobs.c"
    body = ['#include "nvbx_knobs.h"']
    body += ["int k_%s(const char* s) { return nvbx_knob_%s(s); }" % (f, f) for f in FUNCS]
    body += ["void k_grid_margin(const char* s, int* p, int* b) { nvbx_knob_grid_margin(s, p, b); }"]
    src.write_text("\n".join(body) + "\n")
    so = d / "knobs.so"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    for f in FUNCS:
        getattr(lib, "k_" + f).argtypes = [ctypes.c_char_p]
        getattr(lib, "k_" + f).restype = ctypes.c_int
    lib.k_grid_margin.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]

    def call(name, value):
        arg = None if value is None else value.encode()
        if name == "grid_margin":
            p, b = ctypes.c_int(-99), ctypes.c_int(-99)
            lib.k_grid_margin(arg, ctypes.byref(p), ctypes.byref(b))
            return (p.value, b.value)
        return getattr(lib, "k_" + name)(arg)
    return call


# (knob, value -> what the library uses); None = unset
CASES = {
    "integ_grid": {None: 0, "13": 13, "8": 8, "1": 1, "1048576": 1048576, "0": 0, "-1": 0, "1048577": 0, "abc": 0, "8x": 0, "": 0, "99999999999999999999": 0},
    "color_grid": {None: 1024, "8": 8, "1": 1, "0": 1024, "-3": 1024, " ": 1024, "4.5": 1024},
    "edt_riders": {None: 256, "8": 8, "12": 16, "256": 256, "65536": 65536, "0": 256, "7": 256, "-8": 256, "65537": 256, "x": 256},
    "pair_b_edt_riders": {None: 64, "8": 8, "9": 16, "64": 64, "0": 64, "4": 64, "-16": 64},
    "mark_riders": {None: 0, "8": 8, "5": 8, "17": 24, "0": 0, "-1": 0, "65537": 0},
    "mark_tiles_first": {None: -1, "0": 0, "1": 1, "2": -1, "-1": -1, "yes": -1},
    "decay_grid": {None: 4096, "1": 1, "4096": 4096, "0": 4096, "-5": 4096, "1048577": 4096},
    "st_lanes": {None: 0, "1": 1, "2": 2, "4": 4, "8": 8, "0": 0, "3": 0, "16": 0, "-2": 0},
    "fused_trace_lanes": {None: 8, "4": 4, "8": 8, "5": 8, "0": 8, "16": 8},
    "lidar_sparse_grid": {None: 2048, "8": 8, "1": 1, "0": 2048, "-1": 2048},
    "color_deferral": {None: -1, "0": 0, "1": 1, "2": 2, "3": -1, "-1": -1, "x": -1},
    "switch": {None: 1, "0": 0, "1": 1, "2": 1, "-1": 1, "": 1, "off": 1},
    "grid_margin": {None: (25, 64), "0,0": (0, 0), "10": (10, 64), "50,8": (50, 8), "-5,-1": (25, 64), "50,abc": (50, 64), ",7": (25, 7),
                    "0": (0, 64), "x,0": (25, 0), "10001,0": (25, 0), "1" * 40 + ",3": (25, 3)},
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_knob_mapping(knobs, name):
    for value, want in CASES[name].items():
        assert knobs(name, value) == want, (name, value, knobs(name, value), want)


def test_rider_counts_are_multiples_of_eight_and_grids_positive(knobs):
    for v in range(-20, 300):
        s = str(v)
        for name in ("edt_riders", "pair_b_edt_riders"):
            r = knobs(name, s)
            assert r >= 8 and r % 8 == 0, (name, s, r)
        r = knobs("mark_riders", s)
        assert r == 0 or (r >= 8 and r % 8 == 0 and r >= v), (s, r)
        for name in ("color_grid", "decay_grid", "lidar_sparse_grid"):
            assert knobs(name, s) >= 1, (name, s)
        assert knobs("integ_grid", s) >= 0


# every knob of the header and the name the library reads it by
READS = {"NVBX_INTEG_GRID": "integ_grid", "NVBX_GRID_MARGIN": "grid_margin", "NVBX_COLOR_GRID": "color_grid", "NVBX_EDT_RIDERS": "edt_riders",
         "NVBX_PAIR_B_EDT_RIDERS": "pair_b_edt_riders", "NVBX_MARK_RIDERS": "mark_riders", "NVBX_MARK_TILES_FIRST": "mark_tiles_first",
         "NVBX_DECAY_GRID": "decay_grid", "NVBX_ST_LANES": "st_lanes", "NVBX_FUSED_TRACE_LANES": "fused_trace_lanes", "NVBX_FUSE_COLC": "switch",
         "NVBX_DEPTH_PAIR": "switch", "NVBX_LIDAR_SPARSE": "switch", "NVBX_LIDAR_DENSE_LIST": "switch", "NVBX_LIDAR_SPARSE_GRID": "lidar_sparse_grid",
         "NVBX_DEFER_EDT": "switch", "NVBX_COLOR_DEFERRAL": "color_deferral"}


def test_the_library_reads_these_knobs_through_the_header_only():
    seen = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")) or f == "nvbx_knobs.h":
            continue
        for line in open(os.path.join(CSRC, f)):
            for var in re.findall(r'getenv\("(NVBX_[A-Z_]+)"\)', line):
                if var in READS:
                    assert "nvbx_knob_%s(getenv(\"%s\")" % (READS[var], var) in line, (f, line.strip())
                    seen[var] = seen.get(var, 0) + 1
    assert seen == {v: 1 for v in READS}, seen
