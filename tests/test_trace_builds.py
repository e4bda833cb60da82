"""tests/trace_builds.py — the tests' rule for "which kernel was that launch" — pinned to the library's rule
(csrc/pt_geom_plan.hpp hierarchy_staging, grid_staging and walk_lds_room through tests/geom_plan_shim.cpp; the table of kernels,
its rows and columns, csrc/pt_trace_table.hpp through tests/trace_table_shim.cpp).  A kernel audit is worth what its naming is
worth: a restatement of the staging arithmetic or of the table that drifts from the library's would let a test believe it
reached a kernel that never ran.  CPU only."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import pytest

import trace_builds as tb
from ray_tracer_webgl_amd import abi
from test_geom_plan import shim  # noqa: F401  (the fixture that compiles and loads the shim)


def lib_hierarchy(lib, n_nodes, n_slots, room):
    b = C.c_uint64()
    return lib.gp_hierarchy_staging(n_nodes, n_slots, room, C.byref(b)), b.value


def lib_grid(lib, n_cells, n_entries, room, cells_build, fit):
    b = C.c_uint64()
    return lib.gp_grid_staging(n_cells, n_entries, room, cells_build, fit, C.byref(b)), b.value


def test_the_room_is_the_librarys(shim):
    assert tb.WALK_LDS_ROOM == shim.gp_walk_lds_room() == 102336
    assert tb.WALK_LDS_MAX == 163776 and tb.MAX_SPHERES_LDS == 10232


def hierarchy_sweep(room):
    """(n_nodes, n_slots) over both thresholds +- 2 records — nodes and slots fit: ((n + 1) 2 + s) 16 <= room, the nodes fit:
    (n + 1) 16 <= room — with the other count at its corners, and the corners of the 16-bit limits"""
    rec = room // 16
    out = set()
    for d in range(-2, 3):
        # all-in-LDS threshold, at a few splits between nodes and slots (slots come in fours; odd counts too: the rule is arithmetic)
        for n in (0, 1, 15, 255, 1597, rec // 2 - 3, rec // 2 - 2, rec // 2 - 1):
            s = rec - 2 * (n + 1) + d
            if s >= 0:
                out.add((n, s))
        for s in (0, 4, 516, 3200, rec - 2):
            n2 = rec - s + d * 2
            for n in (n2 // 2 - 1, n2 // 2, (n2 + 1) // 2 - 1):
                if n >= 0:
                    out.add((n, s))
        # nodes-in-LDS threshold, whatever the slots
        for s in (0, 4, 12792, 12800, 0xFFFC, 0xFFFF):
            out.add((rec - 1 + d, s))
    for n, s in itertools.product((0, 1, rec // 2, rec, 0xFFFE), (0, 4, rec, 0xFFFC, 0xFFFF)):
        out.add((n, s))
    return sorted(out)


def test_hierarchy_rows_follow_the_librarys_staging(shim):
    room = shim.gp_walk_lds_room()
    kinds = set()
    for n, s in hierarchy_sweep(room):
        want = lib_hierarchy(shim, n, s, room)
        assert tb.hierarchy_staging(n, s) == want, (n, s, want)
        kinds.add(want[0])
    assert kinds == {0, 1, 2}
    # the thresholds themselves: the last record that fits and the first that does not
    rec = room // 16
    assert tb.hierarchy_staging(rec // 2 - 1, 0) == (0, room) and tb.hierarchy_staging(rec // 2 - 1, 1)[0] == 1
    assert tb.hierarchy_staging(1597, 3200) == (0, room) and tb.hierarchy_staging(1597, 3201)[0] == 1
    assert tb.hierarchy_staging(rec - 1, 0xFFFF) == (1, room) and tb.hierarchy_staging(rec, 0xFFFF) == (2, 0)
    # another room: the rule, not this room's numbers
    for n, s in ((10, 20), (10, 21), (41, 4), (42, 0), (42, 4), (63, 0), (64, 0)):
        assert tb.hierarchy_staging(n, s, 1024) == lib_hierarchy(shim, n, s, 1024)


@pytest.mark.parametrize("cells_build", [0, 1])
@pytest.mark.parametrize("fit", [0, 1, 2])
def test_grid_builds_follow_the_librarys_staging(shim, cells_build, fit):
    room = shim.gp_walk_lds_room()
    rec = room // 16
    cases = set()
    for d in range(-2, 3):
        for cells in (1, 4, 5, 256, 5400, 4 * (rec // 2)):
            cell_recs = (cells + 3) // 4
            if rec - cell_recs + d >= 0:
                cases.add((cells, rec - cell_recs + d))   # cells and entries fit / do not
        for entries in (0, 1, 798, 19482, 0xFFFF, 200000):
            cases.add((4 * (rec + d), entries))           # the cell records alone fit / do not
            cases.add((4 * (rec + d) - 3, entries))
    for cells, entries in itertools.product((1, 4 * rec, 4 * rec + 1, 31000, 1 << 20), (0, 1, rec, rec + 1, 130000)):
        cases.add((cells, entries))
    kinds = set()
    for cells, entries in sorted(cases):
        want = lib_grid(shim, cells, entries, room, cells_build, fit)
        assert tb.grid_staging(cells, entries, room, bool(cells_build), fit) == want, (cells, entries, want)
        kinds.add(want[0])
    assert kinds == ({1, 2, 3} if not cells_build and fit != 1 else {2, 3})


class Stats:
    """the fields of PtStats row_of reads"""

    def __init__(self, path, n, nodes=0, slots=0, entries=0, build=0, flat=0):
        self.geometry_path, self.n_spheres, self.bvh_nodes, self.bvh_slots = path, n, nodes, slots
        self.grid_entries, self.grid_kernel_build, self.grid_walk_flat = entries, build, flat


ROWS = [
    (Stats(abi.PT_GEOM_LDS, 9), "list_lds", None),
    (Stats(abi.PT_GEOM_LDS, 10232), "list_lds", None),
    (Stats(abi.PT_GEOM_SCALAR, 10232), "scalar", None),
    (Stats(abi.PT_GEOM_SCALAR, 10233), "scalar_nolds", None),
    (Stats(abi.PT_GEOM_SMALL, 12), "small_t0", "small_count"),
    (Stats(abi.PT_GEOM_SMALL, 9), "small_t1", "small_count"),
    (Stats(abi.PT_GEOM_SMALL, 10), "small_t2", "small_count"),
    (Stats(abi.PT_GEOM_SMALL, 11), "small_t3", "small_count"),
    (Stats(abi.PT_GEOM_BVH, 484, 255, 516), "bvh", "bvh_count"),                # config 2
    (Stats(abi.PT_GEOM_BVH, 10001, 5243, 10492), "bvh_nodes", None),            # config 5 (tests/test_geom_plan.py)
    (Stats(abi.PT_GEOM_BVH, 3037, 1597, 3200), "bvh", "bvh_count"),
    (Stats(abi.PT_GEOM_BVH, 3038, 1603, 3212), "bvh_nodes", None),
    (Stats(abi.PT_GEOM_BVH, 12224, 6395, 12792), "bvh_nodes", None),
    (Stats(abi.PT_GEOM_BVH, 12225, 6396, 12800), "bvh_gmem", None),
    (Stats(abi.PT_GEOM_GRID, 484, entries=798, build=1, flat=1), "grid", "grid_count"),
    (Stats(abi.PT_GEOM_GRID, 1501, entries=3000, build=1, flat=0), "grid_layers", "grid_layers_count"),
    (Stats(abi.PT_GEOM_GRID, 10001, entries=19482, build=2), "grid_cells", "grid_cells_count"),
    (Stats(abi.PT_GEOM_GRID, 60001, entries=130000, build=3), "grid_gmem", None),
]


def test_rows_twins_and_the_columns_with_one_grid_build():
    for st, row, twin in ROWS:
        assert tb.row_of(st) == row and tb.twin_of(row) == twin, (row, twin)
        assert tb.build_of(st, "_rr") == ("grid" if row == "grid_layers" else row) + "_rr"
    assert sorted(r for _, r, _ in ROWS) != [] and {r for _, r, _ in ROWS} == set(tb.ROWS) and len(tb.ROWS) == 14
    assert {t for _, _, t in ROWS if t} == set(tb.TWINS) and len(tb.TWINS) == 5
    # a launch that leaves PtStats.geometry_path alone names its path itself
    assert tb.row_of(Stats(abi.PT_GEOM_LDS, 484, 255, 516), path=abi.PT_GEOM_BVH) == "bvh"
    for bad in (Stats(abi.PT_GEOM_AUTO, 9), Stats(abi.PT_GEOM_SMALL, 17), Stats(abi.PT_GEOM_BVH, 484), Stats(abi.PT_GEOM_GRID, 484, entries=798),
                Stats(abi.PT_GEOM_GRID, 484, entries=798, build=2, flat=1)):
        with pytest.raises(AssertionError):
            tb.row_of(bad)


# ---- the table itself (csrc/pt_trace_table.hpp through tests/trace_table_shim.cpp): which symbol sits in which cell, built for
# ---- how many waves, and the row, the column and the ring layout of a launch

TABLE_SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trace_table_shim.cpp")
REPORTED = (abi.BUILD_PLAIN, abi.BUILD_ROULETTE, abi.BUILD_TWIN, abi.BUILD_DEBUG_OVERLAY, abi.BUILD_FEATURES)
# the ray-query and radiance-query builds: columns of the table, not values pt_last_trace_build ever reports (no abi constant)
BUILD_QRY, BUILD_RAD = 5, 6
COLUMNS = REPORTED + (BUILD_QRY, BUILD_RAD)
DOORS = (0, 1, 2, 3)  # csrc/pt_trace_table.hpp Door: none, pt_render_features, pt_query_rays, pt_query_radiance


@pytest.fixture(scope="module")
def table():
    so = os.path.join(tempfile.mkdtemp(prefix="trace_table_"), "libtrace_table_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", TABLE_SHIM, "-o", so])
    lib = C.CDLL(so)
    IP = C.POINTER(C.c_int)
    lib.tt_shape.restype, lib.tt_shape.argtypes = None, [IP]
    lib.tt_objects.restype, lib.tt_objects.argtypes = C.c_int, [IP]
    lib.tt_cell.restype, lib.tt_cell.argtypes = C.c_char_p, [C.c_int, C.c_int, IP]
    lib.tt_row.restype, lib.tt_row.argtypes = C.c_int, [C.c_int, C.c_uint32, C.c_int, C.c_uint32]
    lib.tt_build.restype, lib.tt_build.argtypes = C.c_int, [C.c_int] * 4
    lib.tt_door_build.restype, lib.tt_door_build.argtypes = C.c_int, [C.c_int]
    lib.tt_reads_ring_layout.restype, lib.tt_reads_ring_layout.argtypes = C.c_int, [C.c_int, C.c_int]
    return lib


def lib_cell(lib, row, build):
    """(name, object, id, waves) of a cell"""
    out = (C.c_int * 3)()
    return (lib.tt_cell(row, build, out).decode(),) + tuple(out)


def lib_row(lib, st):
    """the library's row for the launch the `Stats` describe: the staging kind as the library's own staging rule gives it (pinned
    above), a flat grid as one layer along y"""
    kind = 0
    if st.geometry_path == abi.PT_GEOM_BVH:
        kind = tb.hierarchy_staging(st.bvh_nodes, st.bvh_slots)[0]
    if st.geometry_path == abi.PT_GEOM_GRID:
        kind = st.grid_kernel_build
    return lib.tt_row(st.geometry_path, st.n_spheres, kind, 1 if st.grid_walk_flat else 3)


def test_every_case_names_the_librarys_cell_in_every_column(table):
    assert len(ROWS) == 18
    for st, _, _ in ROWS:
        r, row = lib_row(table, st), tb.row_of(st)
        plain = "" if row == "list_lds" else "_" + row
        twin = tb.twin_of(row)
        want = {
            abi.BUILD_PLAIN: plain,
            abi.BUILD_TWIN: "_" + twin if twin else plain,
            abi.BUILD_ROULETTE: "_" + tb.build_of(st, "_rr"),
            abi.BUILD_DEBUG_OVERLAY: "_" + tb.build_of(st, "_dbg"),
            abi.BUILD_FEATURES: "_" + tb.build_of(st, "_feat"),
            BUILD_QRY: "_" + tb.build_of(st, "_qry"),
            BUILD_RAD: "_" + tb.build_of(st, "_rad"),
        }
        if row == "list_lds":  # no roulette, overlay, feature, query or radiance build: the plain kernel in every column
            want = dict.fromkeys(COLUMNS, "")
        for col in COLUMNS:
            assert lib_cell(table, r, col)[0] == "pt_trace_kernel" + want[col], (row, col)


def waves_of(name):
    """the waves per SIMD a kernel is built for, by its family (csrc/pt_kernel_args.h PT_WAVES_*)"""
    stem = name[len("pt_trace_kernel"):]
    if stem == "":
        return 6
    if stem == "_grid_cells_count":
        return 4
    return 7 if stem.startswith(("_scalar", "_small")) else 6


def test_the_whole_table(table):
    shape = (C.c_int * 2)()
    table.tt_shape(shape)
    assert tuple(shape) == (14, 7) == (len(tb.ROWS), len(COLUMNS))
    ids = (C.c_int * 16)()
    n_objects = table.tt_objects(ids)
    assert n_objects == 7 and list(ids[:7]) == [10, 4, 17, 12, 12, 12, 12]  # main, small, extra, debug, features, query, radiance
    cells = {(r, c): lib_cell(table, r, c) for r in range(14) for c in COLUMNS}
    by_name = {}
    for name, obj, kid, waves in cells.values():
        assert name.startswith("pt_trace_kernel") and waves == waves_of(name), (name, waves)
        assert by_name.setdefault(name, (obj, kid)) == (obj, kid), name   # one kernel, one object and id
    assert len(by_name) == 79 == 55 + 12 + 12 == sum(ids[:7])
    assert len(set(by_name.values())) == 79                                # ... and one id, one kernel
    # every id of every object is used by some cell
    assert set(by_name.values()) == {(obj, kid) for obj in range(7) for kid in range(ids[obj])}
    assert {n for n, _, _, w in cells.values() if w == 4} == {"pt_trace_kernel_grid_cells_count"}
    # the names are the tests' names: every plain row, twin and variant of tests/trace_builds.py, nothing else
    variants = sorted({"grid" if r == "grid_layers" else r for r in tb.ROWS if r != "list_lds"})
    want = {"pt_trace_kernel"} | {"pt_trace_kernel_" + r for r in tb.ROWS if r != "list_lds"} | {"pt_trace_kernel_" + t for t in tb.TWINS}
    want |= {"pt_trace_kernel_%s%s" % (v, s) for v in variants for s in ("_rr", "_dbg", "_feat", "_qry", "_rad")}
    assert set(by_name) == want and len(variants) == 12
    # the ring layout: the two-axis walk's two kernels
    ring = [(r, c) for r in range(14) for c in COLUMNS if table.tt_reads_ring_layout(r, c)]
    assert sorted(cells[rc][0] for rc in ring) == ["pt_trace_kernel_grid", "pt_trace_kernel_grid_count"] and len(ring) == 2
    assert sorted(c for _, c in ring) == [abi.BUILD_PLAIN, abi.BUILD_TWIN]


def test_column_precedence(table):
    """features > overlay > roulette > count-work > plain"""
    for feat, dbg, rr, count in itertools.product((0, 1), repeat=4):
        want = (abi.BUILD_FEATURES if feat else abi.BUILD_DEBUG_OVERLAY if dbg else abi.BUILD_ROULETTE if rr
                else abi.BUILD_TWIN if count else abi.BUILD_PLAIN)
        assert table.tt_build(feat, dbg, rr, count) == want, (feat, dbg, rr, count)
    assert REPORTED == (0, 1, 2, 3, 4)


def test_a_door_names_its_own_column(table):
    """no door: the plain column (a render launch's comes from its options, above); each entry point's door: its own"""
    assert [table.tt_door_build(d) for d in DOORS] == [abi.BUILD_PLAIN, abi.BUILD_FEATURES, BUILD_QRY, BUILD_RAD]
    assert COLUMNS == (0, 1, 2, 3, 4, 5, 6)
