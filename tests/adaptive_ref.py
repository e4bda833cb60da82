"""A plain restatement of adaptive sampling (include/ptrace.h pt_render_adaptive) on top of tests/error_ref.py:
the selection rule, the loop with its per-tile masked fold, and the stable partition of the tile table
(tests/test_adaptive_ref.py on the CPU, tests/test_gpu_adaptive.py on the device).

TEST INFRASTRUCTURE ONLY.  The fold, the tile records and the host sums are error_ref's; what is added here:

    THE SELECTION RULE, on the host in double, one IEEE operation per statement, from the records and tallies pt_error_stats has
    just copied — E, M, C = sum_e2, sum_m2, pixels_counted; per tile t: e_t = the record's sum e, c_t its counted lanes,
    short_t its pixels with !(n >= 2):
        tau = (double)target;  t2 = tau * tau;  b = t2 * M;  Cd = (double)C;
        per tile t:  lhs = (double)e_t * Cd;  rhs = b * (double)c_t;  active_t = short_t > 0 || lhs > rhs;
    A tile is active while its mean squared standard error per counted pixel is above the per-pixel share that meets the
    frame target, if every tile meets it.  A tile with no counted and no short pixel is never active: sampling cannot help
    it (it lies outside the image or holds non-finite radiance).

    the loop: `act` starts from a look at the state the call finds (a fresh estimate: every pixel short, all tiles); per round
    k = min(passes_per_round, max_passes - done), the passes done ... done + k - 1 of the uninterrupted frame are folded into
    the pixels of the active tiles only, done += k, and a look follows: the stats are taken,
    reached = rel_error <= target && pixels_short == 0, `act` is selected anew; stop when reached, when done >= max_passes,
    when no tile is active.

    the partition: the tiles of `base` whose flag is set, in their order in `base`, then the others in theirs.
"""
import numpy as np

import error_ref as E

F = np.float32


def tile_shape(rows, width):
    return (rows + 7) // 8, (width + 7) // 8


def select(state, target):
    """The rule on a state: bool flags of shape (tiles_y * tiles_x,), tile index order."""
    rec, tal = E.tiles(state)
    s = E.stats(state)
    rec = rec.reshape(-1, 4)
    tau = np.float64(F(target))
    t2 = tau * tau
    b = t2 * np.float64(s["sum_m2"])
    cd = np.float64(s["pixels_counted"])
    with np.errstate(all="ignore"):
        lhs = rec[:, 0].astype(np.float64) * cd
        rhs = b * rec[:, 2].astype(np.float64)
        return (tal["short"] > 0) | (lhs > rhs)


def pixel_mask(flags, rows, width):
    """(rows, width) bool: the pixels of the flagged tiles."""
    ty, tx = tile_shape(rows, width)
    m = np.asarray(flags, bool).reshape(ty, tx)
    return np.repeat(np.repeat(m, 8, axis=0), 8, axis=1)[:rows, :width]


def masked_fold(state, accum, passes, flags):
    """error_ref.fold of `passes` into the pixels of the flagged tiles; every other pixel keeps its bits."""
    rows, width = state.shape[:2]
    m = pixel_mask(flags, rows, width)
    st, acc = E.fold(state, accum, passes)
    return np.where(m[..., None, None], st, state), np.where(m[..., None], acc, accum)


def partition(base, flags):
    """Stable partition of the tile table `base` by flags[tile]."""
    base = np.asarray(base, np.uint32)
    f = np.asarray(flags, bool)[base]
    return np.concatenate([base[f], base[~f]]).astype(np.uint32)


def predicted(passes, passes_per_round, target, max_passes, state=None, accum=None, first=0):
    """What pt_render_adaptive does, on pass sums obtained elsewhere (passes[p] = pass p of the uninterrupted frame; the call
    starts at pass `first` on `state` / `accum`, zeros when None).  Returns a dict: `rounds` = per round {first, k, active (the
    flags the round ran with), partial}, `state`, `accum`, `stats` (error_ref.stats of the last look plus passes_rendered and
    reached), `adaptive` (the fields of PtAdaptiveStats), `flags` (the selection after the last look), `count` (per pixel, the
    passes its tile was active for during this call), `next` (first + passes rendered)."""
    rows, width = passes[0].shape[:2]
    st = E.empty_state(rows, width) if state is None else state.copy()
    acc = np.zeros((rows, width, 4), np.float32) if accum is None else accum.copy()
    ty, tx = tile_shape(rows, width)
    n_tiles = ty * tx
    inside = pixel_mask(np.ones(n_tiles, bool), rows, width)
    per_tile = E._lanes(inside, False).sum(axis=1)          # in-image pixels of each tile
    spp = int(passes[0][..., 3].max())
    count = np.zeros((rows, width), np.int64)
    rounds = []
    ad = {"rounds": 0, "partial_rounds": 0, "tiles": n_tiles, "tiles_active": 0, "tile_passes": 0, "samples": 0}
    done = 0
    while True:
        s = E.stats(st)
        s["passes_rendered"] = done
        s["reached"] = int(s["rel_error"] <= float(F(target)) and s["pixels_short"] == 0)
        act = select(st, target)
        ad["tiles_active"] = int(act.sum())
        if s["reached"] or done >= max_passes or not act.any():
            return {"rounds": rounds, "state": st, "accum": acc, "stats": s, "adaptive": ad, "flags": act, "count": count,
                    "next": first + done}
        k = min(passes_per_round, max_passes - done)
        partial = not act.all()
        st, acc = masked_fold(st, acc, passes[first + done:first + done + k], act)
        count += k * pixel_mask(act, rows, width)
        rounds.append({"first": first + done, "k": k, "active": act.copy(), "partial": partial})
        ad["rounds"] += 1
        ad["partial_rounds"] += int(partial)
        ad["tile_passes"] += int(act.sum()) * k
        ad["samples"] += int(per_tile[act].sum()) * k * spp
        done += k


def same_adaptive(ad, ref):
    """A PtAdaptiveStats against predicted()['adaptive']."""
    for k in ("rounds", "partial_rounds", "tiles", "tiles_active", "tile_passes", "samples"):
        if int(getattr(ad, k)) != int(ref[k]):
            return "%s: %r vs %r" % (k, int(getattr(ad, k)), int(ref[k]))
    return ""
