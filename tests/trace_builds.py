"""Which trace kernel a launch was: the row of kTraceKernels (csrc/pt_trace_table.hpp), read from PtStats after the launch.

One place for the arithmetic that decides what a walk kernel stages in the LDS (csrc/pt_geom_plan.hpp hierarchy_staging and
grid_staging, the sizes of csrc/pt_kernel_args.h), so that the tests which audit the kernels they reached — the plain builds and
the measuring twins (test_gpu_plain_builds.py), the roulette, overlay and feature builds (test_gpu_roulette_exact.py,
test_gpu_overlay.py, test_gpu_features.py), the hierarchy at its thresholds (test_gpu_hierarchy_edges.py) — name a launch by one
rule.  tests/test_trace_builds.py pins that rule to the library's, on the CPU."""
from ray_tracer_webgl_amd import abi

# csrc/pt_kernel_args.h: the longest list a workgroup stages, PT_LDS_ENTRIES of it, the parked path state of 1024 lanes
MAX_SPHERES_SMALL = 16
MAX_SPHERES_LDS = 10232
PARK_STRIDE = 15
WALK_LDS_MAX = (((MAX_SPHERES_LDS + 7) & ~7) + 4) * 16
# csrc/pt_geom_plan.hpp walk_lds_room: what a walk kernel may stage beside a 1024-thread workgroup's parked state
WALK_LDS_ROOM = WALK_LDS_MAX - PARK_STRIDE * 4 * 1024

ROWS = ["list_lds", "scalar", "scalar_nolds", "small_t0", "small_t1", "small_t2", "small_t3", "bvh", "bvh_nodes", "bvh_gmem",
        "grid", "grid_layers", "grid_cells", "grid_gmem"]
TWINS = ["small_count", "bvh_count", "grid_count", "grid_layers_count", "grid_cells_count"]


def hierarchy_bytes_all(n_nodes, n_slots):
    """PT_BVH_LDS_BYTES32: fp32 nodes (two records each, and the spare node) and the slots"""
    return ((n_nodes + 1) * 2 + n_slots) * 16


def hierarchy_bytes_nodes(n_nodes):
    """PT_BVH_LDS_BYTES16: the packed nodes and the spare node"""
    return (n_nodes + 1) * 16


def hierarchy_staging(n_nodes, n_slots, room=WALK_LDS_ROOM):
    """(row past `bvh`, bytes staged): 0 = nodes and slots in the LDS, 1 = the nodes, 2 = nothing"""
    if hierarchy_bytes_all(n_nodes, n_slots) <= room:
        return 0, hierarchy_bytes_all(n_nodes, n_slots)
    if hierarchy_bytes_nodes(n_nodes) <= room:
        return 1, hierarchy_bytes_nodes(n_nodes)
    return 2, 0


def grid_staging(n_cells, n_entries, room=WALK_LDS_ROOM, cells_build=False, fit_state=0):
    """(PtStats.grid_kernel_build, bytes staged): 1 = cell records and entries in the LDS, 2 = the cell records, 3 = nothing"""
    need_cells = (n_cells + 3) // 4 * 16
    need_all = need_cells + n_entries * 16
    if need_all <= room and not cells_build and fit_state != 1:
        return 1, need_all
    return (2, need_cells) if need_cells <= room else (3, 0)


def row_of(st, path=None):
    """the row of kTraceKernels the last launch of the context behind `st` (PtStats) was; `path`: the geometry path of a launch
    that leaves PtStats.geometry_path as it finds it (pt_render_features)"""
    path, n = st.geometry_path if path is None else path, st.n_spheres
    if path == abi.PT_GEOM_LDS:
        assert n <= MAX_SPHERES_LDS
        return "list_lds"
    if path == abi.PT_GEOM_SMALL:
        assert n <= MAX_SPHERES_SMALL
        return "small_t%d" % (n & 3)
    if path == abi.PT_GEOM_SCALAR:
        return "scalar" if n <= MAX_SPHERES_LDS else "scalar_nolds"
    if path == abi.PT_GEOM_BVH:
        assert st.bvh_nodes > 0
        return ("bvh", "bvh_nodes", "bvh_gmem")[hierarchy_staging(st.bvh_nodes, st.bvh_slots)[0]]
    if path == abi.PT_GEOM_GRID:  # as the library reports its grid_staging and grid_walk_flat
        assert st.grid_entries > 0 and st.grid_kernel_build in (1, 2, 3)
        if st.grid_kernel_build == 1:
            return "grid" if st.grid_walk_flat else "grid_layers"
        assert st.grid_walk_flat == 0
        return ("grid_cells", "grid_gmem")[st.grid_kernel_build - 2]
    raise AssertionError("no trace kernel for geometry path %d" % path)


def twin_of(row):
    """the measuring twin that runs for `row` under PT_OPT_COUNT_WORK; None where the plain kernel runs then"""
    assert row in ROWS, row
    if row.startswith("small_t"):
        return "small_count"
    return row + "_count" if row in ("bvh", "grid", "grid_layers", "grid_cells") else None


def build_of(st, suffix, path=None):
    """the kernel of a column that has ONE grid build for the rows `grid` and `grid_layers` (roulette, overlay, features, ray queries, radiance
    queries)"""
    row = row_of(st, path)
    return ("grid" if row == "grid_layers" else row) + suffix
