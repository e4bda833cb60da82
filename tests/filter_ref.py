"""A plain restatement of the variance-guided filtered read-out (include/ptrace.h pt_resolve_filtered), built on
error_ref.pixel_error and independent of the kernel; tests/test_filter_ref.py holds it to its properties on the CPU,
tests/test_gpu_filter.py compares pt_filter_kernel with it bit for bit.

TEST INFRASTRUCTURE ONLY.  np.float32 throughout, one IEEE operation per statement, nothing fused; numpy's float32 `/` and sqrt
are correctly rounded.  The state array has the shape (rows, width, 2, 4) (error_ref).

    per pixel: (se, m, known) = the read-out of §4.8b (pixel_error)
               counted = known && finite se && finite m     (the tile kernel's "counted")
               v.c = se.c * se.c
    once:      k2 = kappa * kappa
    rows p may look at: band_count <= 1: all local rows
                        otherwise: the local rows ly with ly / band_rows == y_p / band_rows
                        (p's own chunk of consecutive image rows; local rows of different chunks
                        are not neighbours in the image)
    centre p = (x, y) not counted:
        f = m                                   (0 where unknown, non-finite stays non-finite)
        cnt = 0
    centre p counted:
        sum = {+0, +0, +0}
        cnt = +0
        for dy = -R .. R ascending, for dx = -R .. R ascending:
            q = (x + dx, y + dy)
            skip unless 0 <= q.x < width, q.y is a row p may look at, and q is counted
            if (dx, dy) != (0, 0):
                d.c = m_p.c - m_q.c
                d2.c = d.c * d.c
                t = (d2.r + d2.g) + d2.b
                s.c = v_p.c + v_q.c
                u = (s.r + s.g) + s.b
                rhs = k2 * u
                skip unless t <= rhs            (a NaN on either side skips)
            sum.c = sum.c + m_q.c
            cnt = cnt + 1.0f
        f.c = sum.c / cnt
    gamma != 0: f.c = sqrtf(f.c)                (every pixel)
    out = {f.r, f.g, f.b, cnt}                  (.a = accepted taps, 0 for an uncounted centre)
"""
import numpy as np

import error_ref as E

F = np.float32
MAX_RADIUS = 4
KAPPA_DEFAULT = 2.0


def counted(state):
    """(se, m, counted) of a state: the tile kernel's "counted" per pixel."""
    se, m, known = E.pixel_error(state)
    return se, m, known & np.isfinite(se).all(axis=-1) & np.isfinite(m).all(axis=-1)


def chunk_of_rows(rows, band_rows):
    """The chunk index of every local row: ly // band_rows, or 0 everywhere for a context that is no band (band_rows 0 / None)."""
    ly = np.arange(rows)
    return ly // int(band_rows) if band_rows else np.zeros(rows, np.int64)


def filtered(state, radius, kappa=KAPPA_DEFAULT, gamma=False, band_rows=0):
    """pt_resolve_filtered of `state`: (rows, width, 4) float32 {f.r, f.g, f.b, accepted taps}.  `band_rows`: the chunk height of a
    band context (band_count > 1), 0 for a context that owns the whole image."""
    st = E._f32(state)
    rows, width = st.shape[:2]
    R = int(radius)
    assert 0 <= R <= MAX_RADIUS
    se, m, cntd = counted(st)
    chunk = chunk_of_rows(rows, band_rows)
    ys, xs = np.arange(rows)[:, None], np.arange(width)[None, :]
    with np.errstate(all="ignore"):
        v = se * se
        k2 = F(kappa) * F(kappa)
        total = np.zeros((rows, width, 3), np.float32)
        cnt = np.zeros((rows, width), np.float32)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
                cy, cx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, width - 1)
                cy, cx = np.broadcast_arrays(cy, cx)
                ok = cntd & inside & (chunk[cy] == chunk[ys]) & cntd[cy, cx]
                m_q, v_q = m[cy, cx], v[cy, cx]
                if (dx, dy) != (0, 0):
                    d = m - m_q
                    d2 = d * d
                    t = d2[..., 0] + d2[..., 1]
                    t = t + d2[..., 2]
                    s = v + v_q
                    u = s[..., 0] + s[..., 1]
                    u = u + s[..., 2]
                    rhs = k2 * u
                    ok = ok & (t <= rhs)
                added = total + m_q
                total = np.where(ok[..., None], added, total)
                cnt = np.where(ok, cnt + F(1.0), cnt)
        mean = total / cnt[..., None]
        f = np.where(cntd[..., None], mean, m)
        if gamma:
            f = np.sqrt(f)
    out = np.empty((rows, width, 4), np.float32)
    out[..., :3] = f
    out[..., 3] = cnt
    assert total.dtype == np.float32 and cnt.dtype == np.float32 and f.dtype == np.float32
    return out


def ordinary_state(width, rows, seed=13):
    """Every pixel counted: mean uniform in [0.5, 8), M2 uniform in [0, 4), n = 8, k = 32."""
    rng = np.random.default_rng(seed)
    st = E.empty_state(rows, width)
    st[..., 0, :3] = rng.uniform(0.5, 8.0, (rows, width, 3)).astype(np.float32)
    st[..., 0, 3] = 8.0
    st[..., 1, :3] = rng.uniform(0.0, 4.0, (rows, width, 3)).astype(np.float32)
    st[..., 1, 3] = 32.0
    return st


def squared_error(image, reference):
    """Sum over pixels and channels of (image - reference)^2, in double."""
    d = np.asarray(image, np.float64)[..., :3] - np.asarray(reference, np.float64)[..., :3]
    return float((d * d).sum())
