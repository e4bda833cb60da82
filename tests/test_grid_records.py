"""The device form of a grid cell record and the ring layout of a one-layer grid (csrc/pt_grid_records.hpp), on the CPU.

The host grid keeps `first | count << 24` (pt_grid.hpp, and everything that exports it).  The kernels read a record derived
from it at upload: `first` in 23 bits and a 9-bit field — the 4-bit valid mask of the only round of a cell of at most four
entries, or 256 | count with "long" as the sign bit.  Checked through a shim compiled from the header itself:

  (a) decode-after-encode is the host record's (first, count), for every count 0 ... 255 and `first` at 0, 1, mid-range and the
      largest value an entry array the host accepts (`fits`) can give it;
  (b) the (base, mask) of every round a lane runs on the new record — both the way the kernels' four-entry path takes it and
      through the general functions, for G = 4, 3, 2 — is the sequence the parent's decode of the host record gave;
  (c) the host's check: which entry arrays fit the 23-bit field;
  (d) the ring layout on grids built by the library's own builder: every real cell's padded index and back, every ring index
      the "outside" record, no real cell reading as outside.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ray_tracer_webgl_amd import abi, scenes
from test_bvh import random_field

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "grid_records_shim.cpp")
ENTRY_LIMIT = (1 << 23) - 8  # an entry array must be shorter than this (ptrec::kEntryLimit)
_LIB = []


def shim():
    if not _LIB:
        so = os.path.join(tempfile.mkdtemp(prefix="grid_records_"), "libgrid_records_shim.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-DPT_DEV_KNOBS", SHIM_SRC, "-o", so])
        lib = C.CDLL(so)
        u32, vp = C.c_uint32, C.c_void_p
        for name, res, args in (("rec_from_host", u32, [u32]), ("rec_to_host", u32, [u32]), ("rec_none", u32, []),
                                ("rec_fits", C.c_int, [u32]), ("rec_rounds", u32, [u32, u32, C.c_int, vp, vp, u32]),
                                ("ring_cells", C.c_uint64, [u32, u32]), ("ring_index", u32, [u32, u32, u32]),
                                ("ring_outside", u32, []), ("ring_layout", None, [vp, u32, u32, vp]),
                                ("records_build_grid", C.c_int, [C.POINTER(abi.PtSphere), u32, C.c_double, vp, vp, C.c_size_t])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB.append(lib)
    return _LIB[0]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_rounds(first, count, G):
    """the parent's leaf round on `first | count << 24` (pt_grid_walk.hpp before the device record): base, mask, the rest"""
    pend = first | (count << 24)
    out = []
    while (pend >> 24) != 0:
        base, left = pend & 0xFFFFFF, pend >> 24
        out.append((base, (1 << G) - 1 if left >= G else (1 << left) - 1))
        pend = (base + G) | ((left - G) << 24) if left > G else 0
    return out


def device_rounds(rec, G, fast):
    base = np.zeros(256, np.uint32)
    mask = np.zeros(256, np.uint32)
    n = shim().rec_rounds(rec, G, int(fast), _vp(base), _vp(mask), 256)
    assert n <= 256
    return [(int(base[k]), int(mask[k])) for k in range(n)]


def firsts(count):
    # 0, 1, mid-range, and the largest first of a cell of `count` entries in the longest array the host accepts
    return (0, 1, 4_000_003, ENTRY_LIMIT - 1 - count)


def test_decode_after_encode_is_the_host_record():
    lib = shim()
    assert lib.rec_none() == 1 << 23
    for count in range(256):
        for first in firsts(count):
            host = first | (count << 24)
            rec = lib.rec_from_host(host)
            assert lib.rec_to_host(rec) == host, (first, count, hex(rec))
            assert (rec >= lib.rec_none()) == (count != 0)       # `has` / an empty cell
            assert (rec >> 31 != 0) == (count > 4)               # "long" is the sign bit
            if count <= 4:
                assert rec >> 23 == (1 << count) - 1             # the valid mask of the cell's only round


@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 8, 9, 17, 255])
def test_the_rounds_of_the_counts_that_change_path(count):
    """no round / one short round / exactly four / a long cell with a short rest (5, 8: rests 1, 4), with a long rest first (9, 17),
    the format's longest"""
    lib = shim()
    for first in firsts(count):
        rec = lib.rec_from_host(first | (count << 24))
        want = host_rounds(first, count, 4)
        assert len(want) == (count + 3) // 4
        assert device_rounds(rec, 4, True) == want, (first, count)
        assert device_rounds(rec, 4, False) == want, (first, count)


def test_the_rounds_of_every_count():
    lib = shim()
    for count in range(256):
        for first in firsts(count):
            rec = lib.rec_from_host(first | (count << 24))
            assert device_rounds(rec, 4, True) == host_rounds(first, count, 4), (first, count)
            for G in (4, 3, 2):
                got = device_rounds(rec, G, False)
                assert got == host_rounds(first, count, G), (first, count, G)
                assert all(b + G <= (1 << 23) - 1 for b, _ in got)  # every base, and the entries read from it, inside the field


def test_which_entry_arrays_fit():
    lib = shim()
    assert lib.rec_fits(0) and lib.rec_fits(794) and lib.rec_fits(ENTRY_LIMIT - 1)
    assert not lib.rec_fits(ENTRY_LIMIT) and not lib.rec_fits(1 << 23) and not lib.rec_fits(1 << 24)


# ---- the ring layout ------------------------------------------------------------------------------------------------

def _flat_field(n, seed, ex, ez, r=0.2):
    """n spheres of one size on a plane, centres in [0, ex] x [0, ez]"""
    s = random_field(n, seed, extent=1.0, rmax=r, giants=0)
    rng = np.random.default_rng(seed)
    s["center"][:, 0] = rng.uniform(0.0, ex, n).astype(np.float32)
    s["center"][:, 1] = np.float32(r)
    s["center"][:, 2] = rng.uniform(0.0, ez, n).astype(np.float32)
    s["radius"][:] = np.float32(r)
    return s


def built(spheres, want_n, scales):
    """the library's builder (ptgrid::build) on `spheres`, with the first cell-edge scale of `scales` that gives want_n cells"""
    lib = shim()
    ptr, n, keep = abi.spheres_as_ctypes(spheres)
    tried = []
    for sc in scales:
        n3 = np.zeros(3, np.uint32)
        cells = np.zeros(1 << 16, np.uint32)
        rc = lib.records_build_grid(ptr, n, float(sc), _vp(n3), _vp(cells), cells.size)
        tried.append((sc, rc, tuple(int(v) for v in n3)))
        if rc == 0 and tuple(int(v) for v in n3) == want_n:
            return cells[:int(n3[0]) * int(n3[1]) * int(n3[2])].copy()
    raise AssertionError("no grid of %s cells: %s" % (want_n, tried))


RING_GRIDS = {
    "1x1x1": lambda: built(_flat_field(40, 3, 1.0, 1.0), (1, 1, 1), (8.0, 12.0, 19.0)),
    "2x1x3": lambda: built(_flat_field(60, 4, 4.0, 6.0), (2, 1, 3), np.arange(1.0, 6.0, 0.125)),
    "config2": lambda: built(scenes.config2(96, 54, 2, 2, 12).spheres, (16, 1, 16), (0.0,)),
}
RING_N = {"1x1x1": (1, 1), "2x1x3": (2, 3), "config2": (16, 16)}


@pytest.mark.parametrize("name", sorted(RING_GRIDS))
def test_the_ring_layout_holds_every_real_cell_inside_a_border_of_outside_records(name):
    lib = shim()
    cells = RING_GRIDS[name]()
    nx, nz = RING_N[name]
    assert cells.size == nx * nz and (cells >> 24).sum() > 0
    n_ring = lib.ring_cells(nx, nz)
    assert n_ring == (nx + 2) * (nz + 2)
    ring = np.full(n_ring, 0xDEADBEEF, np.uint32)
    lib.ring_layout(_vp(cells), nx, nz, _vp(ring))
    outside = lib.ring_outside()
    real = np.zeros(n_ring, bool)
    # every real cell — each side's last cell among them — to its padded index and back
    for cz in range(nz):
        for cx in range(nx):
            k = lib.ring_index(nx, cx, cz)
            assert k == (cz + 1) * (nx + 2) + (cx + 1) and 0 < k < n_ring and not real[k]
            real[k] = True
            assert (k % (nx + 2) - 1, k // (nx + 2) - 1) == (cx, cz)
            host = int(cells[cz * nx + cx])
            rec = int(ring[k])
            assert rec != outside, (cx, cz)                       # no real cell ends a walk
            if host >> 24:
                assert rec == lib.rec_from_host(host) and lib.rec_to_host(rec) == host
            else:                                                 # an empty cell: no entries; its first is free (1 where it was 0)
                assert rec < lib.rec_none() and rec in (host, 1) and (rec == host or host == 0)
    for cx, cz in ((0, 0), (nx - 1, 0), (0, nz - 1), (nx - 1, nz - 1)):
        assert real[lib.ring_index(nx, cx, cz)]
    # the border, the corner at index 0 included: the outside record, and one step from a side's last cell lands on it
    assert real.sum() == nx * nz and not real[0]
    assert np.all(ring[~real] == outside)
    row = nx + 2
    for cz in range(nz):
        assert not real[lib.ring_index(nx, 0, cz) - 1] and not real[lib.ring_index(nx, nx - 1, cz) + 1]
    for cx in range(nx):
        assert not real[lib.ring_index(nx, cx, 0) - row] and not real[lib.ring_index(nx, cx, nz - 1) + row]


def test_the_encoder_under_address_and_undefined_behaviour_sanitizers():
    """tests/grid_records_main.cpp: a stand-alone program (its own main) over the same counts, built with
    -fsanitize=address,undefined and run as a child; nothing sanitized is loaded into this process"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "grid_records_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(HERE, "grid_records_main.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and "grid records: ok" in out.stdout, out.stdout[-2000:]
