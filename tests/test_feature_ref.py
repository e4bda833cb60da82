"""tests/feature_ref.py (the restatement the GPU feature tests compare against) pinned to the oracle by another route: its
uuid plane equals ora_first_hit_map — the oracle's own loop over pixel centres, which shares no Python with it — on every
pixel, and its band rows come out as pt_band_row says."""
import numpy as np
import pytest

import feature_ref as F
from ray_tracer_webgl_amd import abi, scenes

CASES = {"default": lambda: scenes.default_scene(320, 176, spp=1, max_depth=8), "cover": lambda: scenes.config2(96, 54, 1, 1, 8)}
_PLANES = {}


def planes_of(name):
    if name not in _PLANES:
        sc = CASES[name]()
        _PLANES[name] = (sc, F.planes(sc.spheres, sc.params))
    return _PLANES[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_uuid_plane_equals_the_first_hit_map(ora, name):
    sc, pl = planes_of(name)
    want = F.first_hit_map(sc.spheres, sc.params)
    ids = pl["ids"]
    assert ids.shape == (sc.params.height, sc.params.width, 4) and ids.dtype == np.int32
    assert np.array_equal(ids[..., 1], want)
    hit = want >= 0
    assert hit.any() and (~hit).any()
    # ... and the record hangs together: list index <-> uuid <-> type, +0 where the contract says +0, t > 0 on a hit
    idx = ids[..., 0]
    assert np.array_equal(idx >= 0, hit) and np.array_equal(sc.spheres["uuid"][idx[hit]], want[hit])
    assert np.array_equal(ids[..., 2][hit], sc.spheres["type"][idx[hit]]) and (ids[..., 2][~hit] == -1).all()
    assert set(np.unique(ids[..., 3]).tolist()) <= {0, 1} and (ids[..., 3][~hit] == 0).all()
    assert (pl["albedo"][..., 3][hit] > 0).all()
    assert np.array_equal(pl["albedo"][..., :3][hit], sc.spheres["albedo"][idx[hit]])
    for k in ("normal", "point"):
        assert not pl[k][~hit].view(np.uint32).any() and not pl[k][..., 3].view(np.uint32).any()
    assert not pl["albedo"][..., 3][~hit].view(np.uint32).any()
    sky = pl["albedo"][..., :3][~hit]  # the sky gradient: white towards (0.5, 0.7, 1.0), blue never below the others
    assert (sky > 0.49).all() and (sky <= 1.0).all() and (sky[:, 2] >= sky[:, 1]).all() and (sky[:, 1] >= sky[:, 0]).all()


def test_black_background_misses_are_zero(ora):
    sc = CASES["default"]()
    p = sc.params.copy()
    p.width, p.height, p.background_mode = 40, 22, abi.PT_BG_BLACK
    pl = F.planes(sc.spheres, p)
    miss = pl["ids"][..., 1] < 0
    assert miss.any() and not pl["albedo"][miss].view(np.uint32).any()


def test_band_rows_come_out_as_pt_band_row_says(ora, lib):
    sc, whole = planes_of("cover")
    h = sc.params.height
    seen = []
    for r in range(3):
        p = sc.params.copy()
        p.band_rows, p.band_index, p.band_count = 4, r, 3
        n = lib.pt_local_rows(h, 4, r, 3)
        ys = [lib.pt_band_row(4, r, 3, l) for l in range(n)]
        assert F.owned_rows(p) == ys
        pl = F.planes(sc.spheres, p)
        for k in whole:
            assert pl[k].shape[0] == n
            assert np.array_equal(pl[k].view(np.uint32), whole[k][ys].view(np.uint32)), (r, k)
        seen += ys
    assert sorted(seen) == list(range(h))
