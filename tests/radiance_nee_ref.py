"""The records of include/ptrace.h pt_query_radiance_nee, restated: tests/radiance_ref.records with ora_ray_color replaced by
tests/nee_ref.py's Restatement.path(o, d, seed, acc) — one path of the PT_OPT_NEXT_EVENT estimator from the caller's ray, which
starts with a throughput of one, depth 0 and sampled = False (the caller's ray is a path's FIRST segment: an emissive sphere
it hits adds its emission).  The batch, the place, the pixel centre and the seed are radiance_ref's; `acc`, the pass's running
sum, is carried over the samples_per_pixel chained paths of a pass — every term goes into it where it arises, the order in
which a render launch's per-item sum receives them — and is then added to the record.  TEST INFRASTRUCTURE ONLY.

light_sample=False is the scaffold: the plain estimator, radiance_ref.records' own bits (tests/test_radiance_nee_ref.py)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import nee_ref
import query_ref as Q
import radiance_ref as RR
from feature_ref import owned_rows
from oracle import oracle

F = np.float32


class _Counting(nee_ref.Restatement):
    """the restatement, which also counts the shadow segments whose closest hit is a sphere that is no light: occluded for
    certain (path() counts a shadow segment just before it asks for that segment's hit)"""

    def __init__(self, spheres, params, light_sample=True):
        super().__init__(spheres, params, light_sample=light_sample)
        self.occluded = 0
        self._shadow_seen = 0

    def _hit_world(self, o, d):
        hit = super()._hit_world(o, d)
        if self.shadow_segments != self._shadow_seen:
            self._shadow_seen = self.shadow_segments
            if hit and self.index_of[int(self._hit.index)] not in self.light_of_index:
                self.occluded += 1
        return hit


def records(spheres, params, origins, directions, n_passes, light_sample=True, per_sample=None, info=None):
    """((n, 4) float32 {sum r, g, b, samples}, segments, shadow segments): the record of every ray under the list `spheres` and
    the uniforms `params`; the segments are the path segments plus the shadow segments.  per_sample: a dict that receives, per
    valid ray index, the list of every sample's own term sum (3 float64, in pass and sample order), for variances.  info: a
    dict that receives "occluded", the shadow segments that ended on a sphere that is no light."""
    L = oracle.load()
    p = params.copy()
    o_all = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d_all = np.ascontiguousarray(directions, F).reshape(-1, 3)
    assert o_all.shape == d_all.shape and n_passes >= 1
    ok = Q.valid(o_all, d_all)
    rows, w = owned_rows(p), int(p.width)
    B = len(rows) * w
    spp = int(p.samples_per_pixel)
    out = np.zeros((len(o_all), 4), F)
    n_sph = len(nee_ref.as_numpy(spheres))

    def some(indices):
        """the records of these rays into `out` (every ray is independent of every other): (segments, shadow segments, of them occluded)"""
        r = _Counting(spheres, p, light_sample=light_sample)  # (its ctypes buffers are one thread's)
        for i in indices:
            b, j = divmod(int(i), B)
            px, ly = j % w, j // w
            vx, vy = L.ora_v_position(px, p.width), L.ora_v_position(int(rows[ly]), p.height)
            o, d = [F(x) for x in o_all[i]], [F(x) for x in d_all[i]]
            rec = np.zeros(4, F)
            terms = []
            with np.errstate(all="ignore"):
                for k in range(n_passes):
                    seed = F(L.ora_init_seed(vx, vy, float(RR.u_time(p, int(p.first_pass) + b * n_passes + k))))
                    acc = [F(0.0), F(0.0), F(0.0)]
                    for _ in range(spp):
                        before = [float(v) for v in acc]
                        seed = r.path(o, d, seed, acc)
                        terms.append([float(acc[c]) - before[c] for c in range(3)])
                    for c in range(3):
                        rec[c] = rec[c] + acc[c]
                    rec[3] = rec[3] + F(spp)
            out[i] = rec
            if per_sample is not None:
                per_sample[int(i)] = terms
        return r.segments, r.shadow_segments, r.occluded

    todo = np.flatnonzero(ok)  # an invalid ray: {+0, +0, +0, +0}, no segment
    workers = min(16, os.cpu_count() or 1) if len(todo) * n_sph * n_passes * spp > 2_000_000 else 1
    if workers > 1:
        with ThreadPoolExecutor(workers) as pool:
            parts = list(pool.map(some, [todo[k::workers] for k in range(workers)]))
    else:
        parts = [some(todo)]
    if info is not None:
        info["occluded"] = sum(part[2] for part in parts)
    return out, sum(part[0] for part in parts), sum(part[1] for part in parts)


def gather(spheres, params, kind, positions, normals, D, n_passes, light_sample=True):
    """((n, 4 or 28) float32 records, segments, shadow segments, the n * D radiance records): pt_gather_irradiance_nee /
    pt_bake_probes_nee by their defining sentence — tests/gather_ref.py's rays, the records above, tests/gather_ref.py's reduce"""
    import gather_ref as G

    positions = np.asarray(positions, F).reshape(-1, 3)
    n = len(positions)
    normals = np.zeros((n, 3), F) if normals is None else np.asarray(normals, F).reshape(-1, 3)
    o, d = G.rays(kind, positions, normals, D)
    rec, seg, shadow = records(spheres, params, o, d, n_passes, light_sample=light_sample)
    out = np.zeros((n, 28 if kind == G.PROBE else 4), F)
    for i in range(n):
        if G.item_valid(kind, positions[i], normals[i]):
            out[i] = G.reduce_item(kind, rec[i * D:(i + 1) * D], D)
    return out, seg, shadow, rec


raw = RR.raw
has_nan = RR.has_nan
