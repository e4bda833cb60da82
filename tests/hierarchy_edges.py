"""The hierarchy (PT_GEOM_BVH, csrc/pt_bvh.hpp) at the sizes where what a walk kernel stages in the LDS changes, and at the
16-bit limits of its links, leaf numbers and per-lane queues.

The scenes are prefixes of ONE field: the ground and the first M spheres of scenes.field_spheres(64000), seen by config 5's
camera.  Whether a prefix's hierarchy fits the LDS is not monotone in M (a sphere more can make a leaf less), so the edges
are found by search and kept as constants:

  M_BVH_FULL     nodes and slots staged (pt_trace_kernel_bvh), within 1 KiB of the room beside the parked state
  M_NODES_FIRST  the next prefix above it that does not fit: the smallest scene of pt_trace_kernel_bvh_nodes
  M_NODES_FULL   the nodes staged (pt_trace_kernel_bvh_nodes), within 1 KiB of the room
  M_GMEM_FIRST   the next prefix above it whose nodes do not fit: the smallest scene of pt_trace_kernel_bvh_gmem
  M_LIMIT        still gets a hierarchy, with at least 0xffff - 64 slots
  M_OVER         a prefix above it that gets none (pt_build_bvh: PT_ERR_NOT_READY)

tests/test_bvh.py checks on the CPU that each constant still has its property under the builder as it stands; when the builder
changes, that test fails and this file is to be run as a script,

    python tests/hierarchy_edges.py

which derives the constants again with pt_build_bvh (sizes only; a coarse scan, then every prefix around each edge) and prints
them.  The suite never runs the search: at 63 000 spheres a build takes a tenth of a second."""
import ctypes as C
import os
import sys

import numpy as np

if __name__ == "__main__":  # (as a script: the package lies one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_tracer_webgl_amd import _lib, abi, scenes  # noqa: E402
from trace_builds import WALK_LDS_ROOM, hierarchy_bytes_all, hierarchy_bytes_nodes, hierarchy_staging  # noqa: E402

N_FIELD = 64000
NEAR_BYTES = 1024  # "fills the room": staged bytes >= WALK_LDS_ROOM - NEAR_BYTES
NEAR_SLOTS = 64    # "at the limit": n_slots >= MAX_SLOTS - NEAR_SLOTS
MAX_NODES, MAX_SLOTS = 0xFFFE, 0xFFFF

M_BVH_FULL = 3036  # 1597 nodes, 3200 slots: 102 336 bytes staged, the room to the byte
M_NODES_FIRST = 3037  # 1603 nodes, 3212 slots
M_NODES_FULL = 12223  # 6393 nodes, 12 792 slots: 102 304 bytes of nodes staged
M_GMEM_FIRST = 12224  # 6397 nodes, 12 800 slots
M_LIMIT = 62991  # 32 761 nodes, 65 528 slots
M_OVER = 63005  # 0x10000 slots and more: no hierarchy

EDGES = ["M_BVH_FULL", "M_NODES_FIRST", "M_NODES_FULL", "M_GMEM_FIRST", "M_LIMIT", "M_OVER"]
ROW_AT = {"M_BVH_FULL": "bvh", "M_NODES_FIRST": "bvh_nodes", "M_NODES_FULL": "bvh_nodes", "M_GMEM_FIRST": "bvh_gmem",
          "M_LIMIT": "bvh_gmem"}

_field = []


def field():
    """the ground and the 64 000 spheres every prefix is taken from (made once)"""
    if not _field:
        _field.append(scenes.field_spheres(N_FIELD))
    return _field[0]


def prefix(m):
    """the ground and the first m spheres of the field: scenes.field_spheres(m)"""
    assert 0 < m <= N_FIELD
    return field()[:m + 1].copy()


def scene(m, width, height, spp, n_passes, max_depth):
    """prefix m under config 5's camera"""
    sc = scenes.config5(width, height, spp, n_passes, max_depth, n=16)
    sc.spheres = prefix(m)
    sc.note = "%d-sphere field" % m
    return sc


def sizes(m):
    """(n_nodes, n_slots) of prefix m's hierarchy, or None where pt_build_bvh builds none"""
    lib = _lib.load()
    ptr, _, keep = abi.spheres_as_ctypes(field())
    counts = np.zeros(5, np.uint32)
    rc = lib.pt_build_bvh(ptr, m + 1, None, 0, None, 0, None, 0, None, counts.ctypes.data_as(C.c_void_p), None, 0, None, None, 0)
    if rc == abi.PT_ERR_NOT_READY:
        return None
    assert rc == abi.PT_OK, rc
    return int(counts[0]), int(counts[1])


def properties(m):
    """what the constants claim, for prefix m: {"kind": 0 / 1 / 2 or None without a hierarchy, "bytes", "n_nodes", "n_slots"}"""
    s = sizes(m)
    if s is None:
        return {"kind": None, "bytes": 0, "n_nodes": 0, "n_slots": 0}
    kind, staged = hierarchy_staging(*s)
    return {"kind": kind, "bytes": staged, "n_nodes": s[0], "n_slots": s[1]}


def holds(name, m):
    """does prefix m (and, for the FIRST edges, every prefix between it and the edge below) have the property of `name`?"""
    p = properties(m)
    if name == "M_BVH_FULL":
        return p["kind"] == 0 and p["bytes"] == hierarchy_bytes_all(p["n_nodes"], p["n_slots"]) >= WALK_LDS_ROOM - NEAR_BYTES
    if name == "M_NODES_FIRST":
        return p["kind"] == 1 and m > M_BVH_FULL and all(properties(k)["kind"] == 0 for k in range(M_BVH_FULL + 1, m))
    if name == "M_NODES_FULL":
        return p["kind"] == 1 and p["bytes"] == hierarchy_bytes_nodes(p["n_nodes"]) >= WALK_LDS_ROOM - NEAR_BYTES
    if name == "M_GMEM_FIRST":
        return p["kind"] == 2 and m > M_NODES_FULL and all(properties(k)["kind"] == 1 for k in range(M_NODES_FULL + 1, m))
    if name == "M_LIMIT":
        return p["kind"] == 2 and MAX_SLOTS - NEAR_SLOTS <= p["n_slots"] <= MAX_SLOTS and p["n_nodes"] <= MAX_NODES
    if name == "M_OVER":
        return p["kind"] is None and m > M_LIMIT
    raise KeyError(name)


def _search():
    """a coarse scan for where the kind changes, then every prefix around the change"""
    coarse, local = 128, 384
    kinds = {}

    def kind(m):
        if m not in kinds:
            kinds[m] = properties(m)
        return kinds[m]

    def first_change(start, was):
        m = start
        while m <= N_FIELD and kind(m)["kind"] == was:
            m += coarse
        assert m <= N_FIELD, "no prefix up to %d leaves kind %r" % (N_FIELD, was)
        return m

    def around(m):
        return range(max(16, m - local - coarse), min(N_FIELD, m + local) + 1)

    out = {}
    # the fullest prefix of a kind near the kind's end (of equals the longest), then the first prefix above it of the next kind
    at = 1024
    for was, full, first in ((0, "M_BVH_FULL", "M_NODES_FIRST"), (1, "M_NODES_FULL", "M_GMEM_FIRST")):
        at = first_change(at, was)
        best = max((m for m in around(at) if kind(m)["kind"] == was), key=lambda m: (kind(m)["bytes"], m))
        assert kind(best)["bytes"] >= WALK_LDS_ROOM - NEAR_BYTES, (full, best, kind(best))
        out[full] = best
        out[first] = next(m for m in range(best + 1, N_FIELD) if kind(m)["kind"] != was)
        assert kind(out[first])["kind"] == was + 1
    at = first_change(at, 2)
    best = max((m for m in around(at) if kind(m)["kind"] == 2), key=lambda m: (kind(m)["n_slots"], m))
    assert kind(best)["n_slots"] >= MAX_SLOTS - NEAR_SLOTS, ("M_LIMIT", best, kind(best))
    out["M_LIMIT"] = best
    out["M_OVER"] = next(m for m in range(best + 1, N_FIELD) if kind(m)["kind"] is None)
    return out, kinds


if __name__ == "__main__":
    found, seen = _search()
    print("room %d bytes; %d prefixes built" % (WALK_LDS_ROOM, len(seen)))
    for name in EDGES:
        p = seen[found[name]]
        print("%s = %d  # %s" % (name, found[name], "no hierarchy" if p["kind"] is None else
                                 "%d nodes, %d slots, kind %d, %d bytes staged" % (p["n_nodes"], p["n_slots"], p["kind"], p["bytes"])))
