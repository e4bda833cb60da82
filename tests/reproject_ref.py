"""Temporal reprojection (include/ptrace.h pt_reproject, pt_reproject_constants) restated in numpy: the host
constants in float64, the per-pixel statement list in fp32, one IEEE operation per numpy operation.  TEST INFRASTRUCTURE ONLY.

Everything is vectorised over the frame: a statement of the contract is one numpy operation on float32 arrays (numpy adds,
subtracts, multiplies and divides float32 correctly rounded and fuses nothing), a `done` / `skip` is a mask.  Values computed
for pixels that are already done are garbage and never read.
"""
import numpy as np

from ray_tracer_webgl_amd import abi

F = np.float32


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def constants(prev, tolerance_px):
    """out16 of pt_reproject_constants as a float32 array, or None where the call returns PT_ERR_INVALID.  Python floats are
    IEEE doubles: each line below is one operation (or one per component)."""
    tol = float(F(tolerance_px))
    if not np.isfinite(tol) or tol < 0.0 or prev.width == 0:
        return None
    O = [float(x) for x in prev.camera_origin]
    Hh = [float(x) for x in prev.horizontal]
    V = [float(x) for x in prev.vertical]
    L = [float(x) for x in prev.lower_left_corner]
    with np.errstate(all="ignore"):
        e = [np.float64(L[c]) - np.float64(O[c]) for c in range(3)]
        Hh = [np.float64(x) for x in Hh]
        V = [np.float64(x) for x in V]
        n = _cross(Hh, V)
        en = _dot(e, n)
        vn = _cross(V, n)
        da = _dot(Hh, vn)
        nh = _cross(n, Hh)
        db = _dot(V, nh)
        if en == 0.0 or da == 0.0 or db == 0.0:
            return None
        N = [n[c] / en for c in range(3)]
        A = [vn[c] / da for c in range(3)]
        B = [nh[c] / db for c in range(3)]
        ea, eb = _dot(e, A), _dot(e, B)
        w = np.float64(prev.width)
        k = ((np.float64(tol) * np.float64(tol)) * _dot(Hh, Hh)) / (w * w)
        out = np.array(O + N + A + B + [ea, eb, k, 0.0], dtype=np.float64).astype(np.float32)
    if not np.all(np.isfinite(out)):
        return None
    return out


def band_of(p):
    """(band_rows, band_index, band_count) as the kernel reads them: (0, 0, 1) for a context that is no band"""
    if p.band_count <= 1 or p.band_rows == 0:
        return 0, 0, 1
    return int(p.band_rows), int(p.band_index), int(p.band_count)


def local_row_of(y, p):
    """image rows y (int array) -> (owned by this band, local row): the inverse of pt_band_row"""
    br, bi, bc = band_of(p)
    if bc <= 1:
        return np.ones(y.shape, bool), y
    chunk = y // br
    return (chunk % bc) == bi, (chunk // bc) * br + y % br


def _dot32(w, n):
    return (w[0] * n[0] + w[1] * n[1]) + w[2] * n[2]


def reproject(cur_ids, cur_pnt, hist_ids, hist_pnt, acc, prev, params, cap_diffuse, cap_other, tolerance_px):
    """(out, tallies): out (local_rows, width, 4) float32 — what pt_reproject leaves in the accumulation — and
    {"pixels", "pixels_hit", "pixels_kept", "samples_kept"}.  Planes and acc are (local_rows, width, 4) of the band `params`
    describes; prev: the history view's PtParams.  None where the constants are refused."""
    K = constants(prev, tolerance_px)
    if K is None:
        return None
    ids = np.ascontiguousarray(cur_ids, np.int32)
    Pn = np.ascontiguousarray(cur_pnt, np.float32)
    hids = np.ascontiguousarray(hist_ids, np.int32)
    hpnt = np.ascontiguousarray(hist_pnt, np.float32)
    acc = np.ascontiguousarray(acc, np.float32)
    rows, width = ids.shape[:2]
    height = int(params.height)
    assert width == int(params.width) and rows == abi.local_rows(height, params.band_rows, params.band_index, params.band_count)
    O, N, A, B = K[0:3], K[3:6], K[6:9], K[9:12]
    ea, eb, k = K[12], K[13], K[14]
    out = np.zeros((rows, width, 4), np.float32)
    with np.errstate(all="ignore"):
        live = ids[..., 0] >= 0
        w = [Pn[..., c] - O[c] for c in range(3)]
        lam = _dot32(w, N)
        live &= lam > 0
        ws, wt = _dot32(w, A), _dot32(w, B)
        s = ws / lam
        s = s - ea
        t = wt / lam
        t = t - eb
        wf, hf = F(width), F(height)
        fx = s * wf
        fx = fx - F(0.5)
        fy = t * hf
        fy = fy - F(0.5)
        live &= (fx > F(-1)) & (fx < wf) & (fy > F(-1)) & (fy < hf)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0 = np.where(live, x0f, F(0)).astype(np.int64)
        y0 = np.where(live, y0f, F(0)).astype(np.int64)
        lam2 = lam * lam
        rhs = k * lam2
        cap = np.where(ids[..., 2] == abi.PT_DIFFUSE, F(cap_diffuse), F(cap_other)).astype(np.float32)
        sm = [np.zeros((rows, width), np.float32) for _ in range(3)]
        cnt = np.zeros((rows, width), np.float32)
        wsum = np.zeros((rows, width), np.float32)
        one = F(1)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = x0 + dx, y0 + dy
                ok = live & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                owned, lq = local_row_of(np.where(ok, qy, 0), params)
                ok &= owned
                lq = np.where(ok, lq, 0)
                qxs = np.where(ok, qx, 0)
                assert lq.max(initial=0) < max(rows, 1)
                h_i, h_p, a = hids[lq, qxs], hpnt[lq, qxs], acc[lq, qxs]
                ok &= (h_i[..., 0] == ids[..., 0]) & (h_i[..., 3] == ids[..., 3])
                d = [h_p[..., c] - Pn[..., c] for c in range(3)]
                d2 = _dot32(d, d)
                ok &= d2 <= rhs
                ok &= a[..., 3] > 0
                wx = ax if dx else one - ax
                wy = ay if dy else one - ay
                g = wx * wy
                ok &= g > 0
                for c in range(3):
                    m = a[..., c] / a[..., 3]
                    gm = g * m
                    sm[c] = np.where(ok, sm[c] + gm, sm[c])
                ga = g * a[..., 3]
                cnt = np.where(ok, cnt + ga, cnt)
                wsum = np.where(ok, wsum + g, wsum)
        live &= wsum > 0
        nq = cnt / wsum
        nq = np.floor(nq)
        nq = np.where(nq > cap, cap, nq)
        live &= nq >= 1
        for c in range(3):
            col = sm[c] / wsum
            out[..., c] = np.where(live, col * nq, F(0))
        out[..., 3] = np.where(live, nq, F(0))
    kept = out[..., 3] > 0
    tallies = {"pixels": rows * width, "pixels_hit": int((ids[..., 0] >= 0).sum()), "pixels_kept": int(kept.sum()),
               "samples_kept": int(out[..., 3][kept].astype(np.int64).sum())}
    return out, tallies


def flight_params(p0, k):
    """frame k of the flight the quality figures are measured on: origin offset (0.02 k, 0, -0.01 k), yaw + 0.5 degrees x k;
    the clock advances by 1000 per frame so that every frame's samples are new ones"""
    import ctypes as C

    from ray_tracer_webgl_amd._lib import load

    lib = load()
    cam = abi.PtCameraIn()
    assert lib.pt_default_camera(p0.width, p0.height, C.byref(cam)) == 0
    cam.camera_origin = abi.d3(cam.camera_origin[0] + 0.02 * k, cam.camera_origin[1], cam.camera_origin[2] - 0.01 * k)
    cam.yaw_degrees = cam.yaw_degrees + 0.5 * k
    p = p0.copy()
    assert lib.pt_camera_from_state(C.byref(cam), C.byref(p)) == 0
    p.time = p0.time + 1000.0 * k
    return p


def footprint_rows(cur_pnt, prev, params, tolerance_px=1.0):
    """(live, y0) per pixel: whether the projection lands in the history frame and the lower image row of its four taps — what
    the band test needs to say which pixels gather from a row another band owns"""
    K = constants(prev, tolerance_px)
    Pn = np.ascontiguousarray(cur_pnt, np.float32)
    with np.errstate(all="ignore"):
        w = [Pn[..., c] - K[c] for c in range(3)]
        lam = _dot32(w, K[3:6])
        s = _dot32(w, K[6:9]) / lam - K[12]
        t = _dot32(w, K[9:12]) / lam - K[13]
        wf, hf = F(params.width), F(params.height)
        fx, fy = s * wf - F(0.5), t * hf - F(0.5)
        live = (lam > 0) & (fx > F(-1)) & (fx < wf) & (fy > F(-1)) & (fy < hf)
        y0 = np.where(live, np.floor(fy), F(0)).astype(np.int64)
    return live, y0


CLASSES = ("plain", "miss", "behind", "outside_x", "outside_y", "nan", "inf", "ninf", "huge", "huge_ahead", "other_index",
           "other_face", "other_depth", "left_rim", "right_rim", "bottom_rim", "top_rim", "centre", "hist_nan", "hist_miss",
           "acc_empty", "acc_nan", "acc_inf")


def hand_frame(params, seed=7):
    """A hand-made full-height frame with every operand class of the contract, for the view `params` (which is also the
    history view: the surfaces stand still, the current pixels look at them from sub-pixel offsets).  Returns a dict of
    full-height arrays — cur_ids, cur_pnt, hist_ids, hist_pnt, acc, (h, w, 4) each — and "cls", the class index per pixel
    (CLASSES).  The surface under history pixel (x, y) is the point at depth 2 along that pixel's central ray; its sphere index
    changes every 8 columns and 4 rows, so taps straddle index borders too."""
    rng = np.random.default_rng(seed)
    w, h = int(params.width), int(params.height)
    O = np.array(list(params.camera_origin), np.float64)
    Hh = np.array(list(params.horizontal), np.float64)
    V = np.array(list(params.vertical), np.float64)
    e = np.array(list(params.lower_left_corner), np.float64) - O
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))

    def point(px, py, depth):
        s, t = (px + 0.5) / w, (py + 0.5) / h
        d = e[None, None, :] + s[..., None] * Hh[None, None, :] + t[..., None] * V[None, None, :]
        return O[None, None, :] + np.asarray(depth, np.float64)[..., None] * d

    def ids_at(px, py):
        idx = ((px.astype(np.int64) // 8) + (py.astype(np.int64) // 4)) % 5
        out = np.zeros(px.shape + (4,), np.int32)
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = idx, idx + 100, idx % 3, 1 - (idx == 4)
        return out

    two = np.full((h, w), 2.0)
    hist_pnt = np.zeros((h, w, 4), np.float32)
    hist_pnt[..., :3] = point(xs, ys, two)
    hist_ids = ids_at(xs, ys)
    counts = rng.choice(np.array([1, 3, 17, 40, 100], np.float32), size=(h, w))
    acc = np.zeros((h, w, 4), np.float32)
    acc[..., :3] = rng.random((h, w, 3), dtype=np.float32) * counts[..., None]
    acc[..., 3] = counts
    cls = rng.choice(len(CLASSES), size=(h, w), p=[0.4] + [0.6 / (len(CLASSES) - 1)] * (len(CLASSES) - 1))
    is_ = lambda name: cls == CLASSES.index(name)
    ox = rng.uniform(-0.5, 0.5, (h, w))
    oy = rng.uniform(-0.5, 0.5, (h, w))
    ox[is_("centre")] = 0.0
    oy[is_("centre")] = 0.0
    px, py, depth = xs + ox, ys + oy, two.copy()
    px[is_("outside_x")] = np.where(rng.random((h, w)) < 0.5, -1.75, w + 0.75)[is_("outside_x")]
    py[is_("outside_y")] = np.where(rng.random((h, w)) < 0.5, -1.75, h + 0.75)[is_("outside_y")]
    px[is_("left_rim")], px[is_("right_rim")] = -0.25, w - 0.75      # fx in (-1, 0) / (width - 1, width): one tap column outside
    py[is_("bottom_rim")], py[is_("top_rim")] = -0.25, h - 0.75
    depth[is_("behind")] = -2.0
    depth[is_("other_depth")] = 2.6
    cur_pnt = np.zeros((h, w, 4), np.float32)
    cur_pnt[..., :3] = point(px, py, depth)
    # the ids of the surface the pixel looks at: those of the history pixel its projection rounds to
    cur_ids = ids_at(np.clip(np.rint(px), 0, w - 1), np.clip(np.rint(py), 0, h - 1))
    cur_ids[is_("miss")] = (-1, -1, -1, 0)
    cur_ids[is_("other_index"), 0] = 9   # (an index no history texel carries)
    cur_ids[is_("other_face"), 3] ^= 1
    cur_pnt[is_("nan"), 1] = np.nan
    cur_pnt[is_("inf"), 0] = np.inf
    cur_pnt[is_("ninf"), 2] = -np.inf
    cur_pnt[is_("huge"), :3] = 1e30
    ahead = e + 0.5 * Hh + 0.5 * V   # the view's central ray: 1e30 along it projects to the middle of the frame
    cur_pnt[is_("huge_ahead"), :3] = (O + 1e30 * ahead / np.linalg.norm(ahead)).astype(np.float32)
    hist_pnt[is_("hist_nan"), 0] = np.nan
    hist_ids[is_("hist_miss")] = (-1, -1, -1, 0)
    acc[is_("acc_empty")] = 0.0
    acc[is_("acc_nan"), 0] = np.nan
    acc[is_("acc_inf"), 1] = np.inf
    return {"cur_ids": cur_ids, "cur_pnt": cur_pnt, "hist_ids": hist_ids, "hist_pnt": hist_pnt, "acc": acc, "cls": cls}


# ------------------------------------------------------------------------------------------------ the shared header on the CPU
def build_shim(directory):
    """tests/reproject_plan_shim.cpp compiled into `directory`: csrc/pt_reproject_plan.hpp and csrc/pt_reproject.hpp, the header
    the kernel runs per thread, behind ctypes.  -ffp-contract=off as in the library's own build."""
    import ctypes as C
    import os
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    so = os.path.join(directory, "libreproject_plan_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                           os.path.join(here, "reproject_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    lib.reproject_plan_constants.restype = C.c_int
    lib.reproject_plan_constants.argtypes = [fp, C.c_uint32, C.c_float, fp]
    lib.reproject_plan_frame.restype = None
    lib.reproject_plan_frame.argtypes = [C.POINTER(C.c_uint32), fp, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp]
    return lib


def camera12(prev):
    return np.array(list(prev.camera_origin) + list(prev.horizontal) + list(prev.vertical) + list(prev.lower_left_corner), np.float32)


def frame6(params, rows):
    br, bi, bc = band_of(params)
    return np.array([params.width, params.height, rows, br, bi, bc], np.uint32)


def _aligned(a, dtype):
    """a C-contiguous copy whose data is 16-byte aligned (the header's texels are alignas(16))"""
    a = np.ascontiguousarray(a, dtype)
    buf = np.empty(a.nbytes + 16, np.uint8)
    off = (-buf.ctypes.data) % 16
    out = buf[off:off + a.nbytes].view(dtype).reshape(a.shape)
    out[...] = a
    return out


def shim_reproject(shim, cur_ids, cur_pnt, hist_ids, hist_pnt, acc, prev, params, cap_diffuse, cap_other, tolerance_px):
    """reproject() through the C++ header: the out array, or None where the constants are refused"""
    import ctypes as C

    fp = C.POINTER(C.c_float)
    k16 = np.zeros(16, np.float32)
    cam = camera12(prev)
    if not shim.reproject_plan_constants(cam.ctypes.data_as(fp), int(prev.width), float(tolerance_px), k16.ctypes.data_as(fp)):
        return None
    arrs = [_aligned(cur_ids, np.int32), _aligned(cur_pnt, np.float32), _aligned(hist_ids, np.int32), _aligned(hist_pnt, np.float32),
            _aligned(acc, np.float32)]
    out = _aligned(np.zeros(arrs[1].shape, np.float32), np.float32)
    f6 = frame6(params, arrs[0].shape[0])
    shim.reproject_plan_frame(f6.ctypes.data_as(C.POINTER(C.c_uint32)), k16.ctypes.data_as(fp), float(cap_diffuse), float(cap_other),
                              *[a.ctypes.data_as(C.c_void_p) for a in arrs], out.ctypes.data_as(C.c_void_p))
    return np.array(out)


def write_main_file(path, cur_ids, cur_pnt, hist_ids, hist_pnt, acc, prev, params, cap_diffuse, cap_other, tolerance_px):
    """one frame in the layout tests/reproject_main.cpp reads, with this module's constants and output as the expectation"""
    K = constants(prev, tolerance_px)
    rows = np.asarray(cur_ids).shape[0]
    with open(path, "wb") as f:
        f.write(frame6(params, rows).tobytes())
        f.write(camera12(prev).tobytes())
        f.write(np.array([tolerance_px, cap_diffuse, cap_other], np.float32).tobytes())
        f.write((K if K is not None else np.zeros(16, np.float32)).tobytes())
        f.write(np.array([1 if K is None else 0], np.uint32).tobytes())
        if K is None:
            out = np.zeros(np.asarray(cur_pnt).shape, np.float32)
        else:
            out, _ = reproject(cur_ids, cur_pnt, hist_ids, hist_pnt, acc, prev, params, cap_diffuse, cap_other, tolerance_px)
        for a, dt in ((cur_ids, np.int32), (cur_pnt, np.float32), (hist_ids, np.int32), (hist_pnt, np.float32), (acc, np.float32),
                      (out, np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def same_floats(got, ref):
    """bit patterns equal, except where both sides are NaN"""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return got.shape == ref.shape and bool(np.all((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))))


def first_difference(got, ref):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    if got.shape != ref.shape:
        return "shapes %s vs %s" % (got.shape, ref.shape)
    bad = np.argwhere(~((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))))
    if len(bad) == 0:
        return "equal"
    i = tuple(bad[0])
    return "%d of %d values differ, first at %s: %r vs %r" % (len(bad), got.size, i, got[i], ref[i])
