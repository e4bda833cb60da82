"""A plain restatement of the patch-wise filtered read-out (include/ptrace.h pt_resolve_filtered_patch), built on
error_ref.pixel_error and filter_ref's counted / chunk_of_rows and independent of the kernel; tests/test_patch_filter_ref.py holds
it to its properties on the CPU, tests/test_gpu_patch_filter.py compares pt_filter_patch_kernel with it bit for bit.

TEST INFRASTRUCTURE ONLY.  np.float32 throughout, one IEEE operation per statement, nothing fused; numpy's float32 `/` and sqrt
are correctly rounded.  The state array has the shape (rows, width, 2, 4) (error_ref).  R = radius, P = patch.

    patch-wise test: (se, m, known), counted, v.c, k2 and the rows p may look at are pt_resolve_filtered's (§4.8d)
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
                T = +0
                U = +0
                for oy = -P .. P ascending, for ox = -P .. P ascending:
                    a = (x + ox, y + oy), b = (q.x + ox, q.y + oy)
                    skip unless 0 <= a.x < width, 0 <= b.x < width, a.y and b.y are rows p may look at, a and b are counted
                    d.c = m_a.c - m_b.c
                    d2.c = d.c * d.c
                    t = (d2.r + d2.g) + d2.b
                    s.c = v_a.c + v_b.c
                    u = (s.r + s.g) + s.b
                    T = T + t
                    U = U + u
                rhs = k2 * U
                skip unless T <= rhs            (a NaN on either side skips)
            sum.c = sum.c + m_q.c
            cnt = cnt + 1.0f
        f.c = sum.c / cnt
    gamma != 0: f.c = sqrtf(f.c)                (every pixel)
    out = {f.r, f.g, f.b, cnt}                  (.a = accepted taps of the patch-wise test, 0 for an uncounted centre)
"""
import numpy as np

import error_ref as E
import filter_ref as FR

F = np.float32
MAX_RADIUS = FR.MAX_RADIUS
MAX_PATCH = 1
KAPPA_DEFAULT = 1.5


def filtered(state, radius, patch=MAX_PATCH, kappa=KAPPA_DEFAULT, gamma=False, band_rows=0):
    """pt_resolve_filtered_patch of `state`: (rows, width, 4) float32 {f.r, f.g, f.b, accepted taps}.  `band_rows`: the chunk
    height of a band context (band_count > 1), 0 for a context that owns the whole image."""
    st = E._f32(state)
    rows, width = st.shape[:2]
    R, P = int(radius), int(patch)
    assert 0 <= R <= MAX_RADIUS and 0 <= P <= MAX_PATCH
    se, m, cntd = FR.counted(st)
    chunk = FR.chunk_of_rows(rows, band_rows)
    ys, xs = np.arange(rows)[:, None], np.arange(width)[None, :]

    def look(ddx, ddy):
        """The texel at p + (ddx, ddy) for every p: (inside the image, in a row p may look at and counted; its clipped row and
        column indices)."""
        ty, tx = ys + ddy, xs + ddx
        inside = (tx >= 0) & (tx < width) & (ty >= 0) & (ty < rows)
        cy, cx = np.broadcast_arrays(np.clip(ty, 0, rows - 1), np.clip(tx, 0, width - 1))
        return inside & (chunk[cy] == chunk[ys]) & cntd[cy, cx], cy, cx

    with np.errstate(all="ignore"):
        v = se * se
        k2 = F(kappa) * F(kappa)
        total = np.zeros((rows, width, 3), np.float32)
        cnt = np.zeros((rows, width), np.float32)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                q_ok, qy, qx = look(dx, dy)
                ok = cntd & q_ok
                m_q = m[qy, qx]
                if (dx, dy) != (0, 0):
                    T = np.zeros((rows, width), np.float32)
                    U = np.zeros((rows, width), np.float32)
                    for oy in range(-P, P + 1):
                        for ox in range(-P, P + 1):
                            a_ok, ay, ax = look(ox, oy)
                            b_ok, by, bx = look(dx + ox, dy + oy)
                            d = m[ay, ax] - m[by, bx]
                            d2 = d * d
                            t = d2[..., 0] + d2[..., 1]
                            t = t + d2[..., 2]
                            s = v[ay, ax] + v[by, bx]
                            u = s[..., 0] + s[..., 1]
                            u = u + s[..., 2]
                            both = a_ok & b_ok
                            T = np.where(both, T + t, T)
                            U = np.where(both, U + u, U)
                    rhs = k2 * U
                    ok = ok & (T <= rhs)
                    assert T.dtype == np.float32 and U.dtype == np.float32 and rhs.dtype == np.float32
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
