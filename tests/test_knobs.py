"""csrc/nvbx_knobs.h: the NVBX_* environment knobs of the launch geometry and the A/B switches, compiled from the shipped header with gcc and checked on
the CPU.  A missing, malformed or out-of-range value must give the default: a knob that yields a zero grid or zero riders drops work (NVBX_EDT_RIDERS=0
never ran a held-back distance transform, NVBX_DECAY_GRID=0 made every k_decay workgroup a table-clearing rider); a negative one was cast to unsigned for
the launch.  Rider counts come out as multiples of 8.  nvbx_knobs_read fills one mapper's struct and names every variable in one place; the library reads
the environment there and for the process-wide frame pool, nowhere else, and keeps no knob in a static."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_ros_nvblox_amd", "csrc")

FUNCS = ("integ_grid", "color_grid", "edt_riders", "pair_b_edt_riders", "mark_riders", "mark_tiles_first", "decay_grid", "st_lanes",
         "fused_trace_lanes", "lidar_sparse_grid", "color_deferral", "switch", "score_chunks", "view_grid_reach", "view_grid_max_mb",
         "max_blocks", "frame_pool_max")

# the fields of struct nvbx_knobs: (field, the variable that reaches it, what all-unset gives, a value to set, what the field then holds)
FIELDS = (
    ("fuse_colc", "NVBX_FUSE_COLC", 1, "0", 0), ("depth_pair", "NVBX_DEPTH_PAIR", 1, "0", 0), ("lidar_sparse", "NVBX_LIDAR_SPARSE", 1, "0", 0),
    ("lidar_dense_list", "NVBX_LIDAR_DENSE_LIST", 1, "0", 0), ("lidar_view_grid", "NVBX_LIDAR_VIEW_GRID", 1, "0", 0),
    ("defer_edt", "NVBX_DEFER_EDT", 1, "0", 0), ("replay_pair", "NVBX_REPLAY_PAIR", 1, "0", 0), ("esdf_only_carry", "NVBX_ESDF_ONLY_CARRY", 1, "0", 0),
    ("color_deferral", "NVBX_COLOR_DEFERRAL", -1, "1", 1), ("mark_tiles_first", "NVBX_MARK_TILES_FIRST", -1, "0", 0),
    ("integ_grid", "NVBX_INTEG_GRID", 0, "13", 13), ("color_grid", "NVBX_COLOR_GRID", 1024, "9", 9), ("decay_grid", "NVBX_DECAY_GRID", 4096, "3", 3),
    ("lidar_sparse_grid", "NVBX_LIDAR_SPARSE_GRID", 2048, "17", 17), ("grid_margin_pct", "NVBX_GRID_MARGIN", 25, "50", 50),
    ("grid_margin_blocks", "NVBX_GRID_MARGIN", 64, ",7", 7), ("edt_riders", "NVBX_EDT_RIDERS", 256, "12", 16),
    ("pair_b_edt_riders", "NVBX_PAIR_B_EDT_RIDERS", 64, "9", 16), ("mark_riders", "NVBX_MARK_RIDERS", 0, "17", 24), ("st_lanes", "NVBX_ST_LANES", 0, "2", 2),
    ("fused_trace_lanes", "NVBX_FUSED_TRACE_LANES", 8, "4", 4), ("render_lanes", "NVBX_RENDER_LANES", 0, "1", 1),
    ("score_chunks", "NVBX_SCORE_CHUNKS", 0, "5", 5), ("view_grid_reach", "NVBX_VIEW_GRID_REACH", 0, "6", 6),
    ("view_grid_max_mb", "NVBX_VIEW_GRID_MAX_MB", 128, "1", 1), ("max_blocks", "NVBX_MAX_BLOCKS", 0, "4096", 4096),
)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("knobs")
    src = d / "knobs.c"
    body = ['#include "nvbx_knobs.h"']
    body += ["int k_%s(const char* s) { return nvbx_knob_%s(s); }" % (f, f) for f in FUNCS]
    body += ["void k_grid_margin(const char* s, int* p, int* b) { nvbx_knob_grid_margin(s, p, b); }"]
    # nvbx_knobs_read against a fake lookup: one variable set at a time, every name asked for is written down
    body += ["static const char* set_name; static const char* set_value; static char asked[4096];",
             "static const char* fake_lookup(const char* name) {",
             "  strcat(asked, name); strcat(asked, \" \");",
             "  return set_name && strcmp(name, set_name) == 0 ? set_value : NULL; }",
             "static struct nvbx_knobs K;",
             "const char* read_with(const char* name, const char* value) { set_name = name; set_value = value; asked[0] = 0; nvbx_knobs_read(&K, fake_lookup); return asked; }",
             "int knobs_size(void) { return (int)sizeof(struct nvbx_knobs); }"]
    body += ["int get_%s(void) { return K.%s; }" % (f[0], f[0]) for f in FIELDS]
    src.write_text("\n".join(body) + "\n")
    so = d / "knobs.so"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    for f in FUNCS:
        getattr(lib, "k_" + f).argtypes = [ctypes.c_char_p]
        getattr(lib, "k_" + f).restype = ctypes.c_int
    lib.k_grid_margin.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.read_with.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.read_with.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope="module")
def knobs(lib):
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
    # NVBX_LIDAR_VIEW_GRID, NVBX_REPLAY_PAIR, NVBX_ESDF_ONLY_CARRY: "switch" above ("abc" was off under atoi: now the default, on)
    "score_chunks": {None: 0, "1": 1, "64": 64, "1024": 1024, "0": 0, "1025": 0, "-1": 0, "x": 0},
    "view_grid_reach": {None: 0, "1": 1, "12": 12, "1048576": 1048576, "0": 0, "-4": 0, "1048577": 0, "3 ": 0, "far": 0},
    "view_grid_max_mb": {None: 128, "1": 1, "64": 64, "1048576": 1048576, "0": 128, "-1": 128, "1048577": 128, "64MB": 128, "": 128},
    "max_blocks": {None: 0, "1": 1, "4096": 4096, "2147483647": 2147483647, "0": 0, "-4096": 0, "2147483648": 0, "4k": 0, "99999999999999999999": 0},
    "frame_pool_max": {None: 8, "2": 2, "3": 3, "8": 8, "65536": 65536, "1": 2, "0": 2, "-7": 2, "65537": 8, "many": 8, "": 8, "2x": 8,
                       "-99999999999999999999": 8},
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
        for name in ("color_grid", "decay_grid", "lidar_sparse_grid", "view_grid_max_mb"):
            assert knobs(name, s) >= 1, (name, s)
        assert knobs("frame_pool_max", s) >= 2, s
        for name in ("integ_grid", "view_grid_reach", "max_blocks", "score_chunks"):
            assert knobs(name, s) >= 0, (name, s)


def _header_names():
    """The NVBX_* names nvbx_knobs_read looks up, as the header's text has them."""
    text = open(os.path.join(CSRC, "nvbx_knobs.h")).read()
    body = text[text.index("static inline void nvbx_knobs_read("):]
    return re.findall(r'lookup\("(NVBX_[A-Z_]+)"\)', body)


def test_knobs_read_gives_the_defaults_and_each_name_reaches_its_own_field(lib):
    assert lib.knobs_size() == 4 * len(FIELDS)      # (no field the table above does not know)

    def read(name, value):
        asked = lib.read_with(name.encode() if name else None, value.encode() if value else None).decode().split()
        return asked, {f[0]: getattr(lib, "get_" + f[0])() for f in FIELDS}
    asked, defaults = read(None, None)
    assert defaults == {f[0]: f[2] for f in FIELDS}
    # every variable is asked for once per read, and the header's text names it once
    names = sorted({f[1] for f in FIELDS})
    assert sorted(asked) == names and sorted(_header_names()) == names
    for field, var, _, value, want in FIELDS:
        _, got = read(var, value)
        assert got == dict(defaults, **{field: want}), (var, value)
    # a malformed value of any variable leaves every field at its default
    for var in names:
        assert read(var, "1x")[1] == defaults, var


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            yield f, open(os.path.join(CSRC, f)).read()


def test_the_library_reads_these_knobs_through_the_header_only():
    # the environment is read in two places: the mapper's knob read (mapper.hip, through nvbx_knobs_read) and the process-wide frame pool's pool_max()
    sites = [(f, line.strip()) for f, text in _sources() for line in text.splitlines() if "getenv" in line]
    assert len(sites) == 2, sites
    assert sites[0][0] == "frames.hip" and 'nvbx_knob_frame_pool_max(getenv("NVBX_FRAME_POOL_MAX"))' in sites[0][1], sites[0]
    assert sites[1][0] == "mapper.hip" and "nvbx_knobs_read(&m->knobs," in sites[1][1], sites[1]
    # ... and no knob is frozen in a static: nothing static is initialised from a parser of the header or from the mapper's struct
    for f, text in _sources():
        for line in text.splitlines():
            if re.search(r"\bstatic\b[^;(]*=[^;]*(nvbx_knob|knobs\b)", line):
                raise AssertionError((f, line.strip()))
    # outside the header, NVBX_* variable names appear as string literals nowhere but at the frame pool's read
    for f, text in _sources():
        if f != "nvbx_knobs.h":
            assert [n for n in re.findall(r'"(NVBX_[A-Z_]+)"', text) if n != "NVBX_FRAME_POOL_MAX"] == [], f


def test_the_design_document_lists_exactly_the_variables_the_library_reads():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 5.1 Environment switches of the library"):text.index("## 6. Multi-GPU")]
    listed = set()
    for row in section.splitlines():
        if row.startswith("| `NVBX_"):
            listed |= set(re.findall(r"`(NVBX_[A-Z_]+)`", row.split("|")[1]))
    assert listed == set(_header_names()) | {"NVBX_FRAME_POOL_MAX"}, listed ^ (set(_header_names()) | {"NVBX_FRAME_POOL_MAX"})
