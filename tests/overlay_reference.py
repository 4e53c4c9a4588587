"""The overlay rule, stated independently of csrc/zr_overlay.h: numpy float32 for the transform, the clip, the projection and the depth
(every fma evaluated exactly and rounded once), Python integers for the walk.  tests/test_overlay_cpu.py holds the library's host
statement (zr_frame_overlay) to it byte for byte, tests/test_gpu_overlay.py the kernels.

A segment, in list order: ca, cb = PVM * (p, 1) (zr_mat4_point's expressions); nothing drawn when a component is not finite; the
two-point polygon clipped against z >= 0, 4w + x, 4w - x, 4w + y, 4w - y, w - z (>= 0 inside), the outside end replaced by
lerp(in, out, d_in / (d_in - d_out)); w > 0 at both ends; project() with its snap to 1/256 pixel, clamped to the frame's centre +- 2^23;
the walk along the major axis (|dX| >= |dY|: X), half-open in the major coordinate; the depth interpolated in fp32 and clamped between
the ends'; the test against the frame's depth; the highlight's blend."""
import numpy as np

F = np.float32
GUARD = F(4.0)
REACH = 1 << 23
XRAY = 1
MAX_SEGMENTS = 16384
SEGMENT = np.dtype([("a", "<f4", 3), ("b", "<f4", 3), ("rgba", "u1", 4), ("flags", "<u4")])
DEFAULT_STYLE = {"depth_bias": 0.0, "hidden_opacity": 0}


def segments(rows):
    """rows (ax, ay, az, bx, by, bz, r, g, b, a[, flags]) -> a SEGMENT array"""
    out = np.zeros(len(rows), dtype=SEGMENT)
    for i, s in enumerate(rows):
        out[i]["a"], out[i]["b"], out[i]["rgba"], out[i]["flags"] = s[0:3], s[3:6], s[6:10], s[10] if len(s) > 10 else 0
    return out


def fma(a, b, c):
    """fl32(a * b + c), rounded once.  In float64 the product of two float32 is exact and the sum s is rounded to 53 bits, with the
    error e recovered exactly (TwoSum); s rounds to float32 as the exact value does unless s is the midpoint of two neighbouring
    float32 and e is not 0: then e says which side the exact value lies on."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        up = np.nextafter(r, F(np.inf)).astype(np.float64)
        dn = np.nextafter(r, F(-np.inf)).astype(np.float64)
        live = np.isfinite(s) & np.isfinite(e) & (e != 0)
        go_up = live & (s == (r64 + up) * 0.5) & (e > 0)
        go_dn = live & (s == (r64 + dn) * 0.5) & (e < 0)
        r = np.where(go_up, up.astype(np.float32), np.where(go_dn, dn.astype(np.float32), r))
    return r.astype(np.float32)


def mat4_mul(A, B):
    """zr_mat4_mul: column-major 4 x 4, C = A * B in fp32, every fma explicit"""
    A, B = np.asarray(A, dtype=np.float32).reshape(16), np.asarray(B, dtype=np.float32).reshape(16)
    out = np.zeros(16, dtype=np.float32)
    for c in range(4):
        for r in range(4):
            out[c * 4 + r] = fma(A[12 + r], B[c * 4 + 3], fma(A[8 + r], B[c * 4 + 2], fma(A[4 + r], B[c * 4 + 1], F(A[r] * B[c * 4 + 0]))))
    return out


def pvm_of(proj, view, model):
    """proj * view * model, left to right (the frame's PVM)"""
    return mat4_mul(mat4_mul(proj, view), model)


def mat4_point(m, p):
    """m (16,), p (n, 3) -> (n, 4)"""
    m = np.asarray(m, dtype=np.float32).reshape(16)
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([fma(m[8 + k], p[:, 2], fma(m[4 + k], p[:, 1], m[k] * p[:, 0])) + m[12 + k] for k in range(4)], axis=1).astype(np.float32)


def _plane(c, k):
    x, y, z, w = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    with np.errstate(all="ignore"):
        return (z, fma(GUARD, w, x), fma(GUARD, w, -x), fma(GUARD, w, y), fma(GUARD, w, -y), w - z)[k]


def _lerp(a, b, t):
    with np.errstate(all="ignore"):
        return np.stack([fma(t, b[:, k] - a[:, k], a[:, k]) for k in range(4)], axis=1)


def _snap(f):
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(f, F(-2147483648.0)), F(2147483520.0)).astype(np.int64)


def project(c, hw, hh):
    """project() of the rasteriser: (n, 4) clip -> X, Y (int64, 1/256 pixel), z (float32)"""
    hw, hh = F(hw), F(hh)
    with np.errstate(all="ignore"):
        rw = F(1.0) / c[:, 3]
        nx, ny = c[:, 0] * rw, c[:, 1] * rw
        xs, ys = fma(nx, hw, hw), fma(ny, hh, hh)
        X = _snap(np.floor(fma(xs, F(256.0), F(0.5))))
        Y = _snap(np.floor(fma(ys, F(256.0), F(0.5))))
        return X, Y, (c[:, 2] * rw).astype(np.float32)


def setup(pvm, W, H, seg):
    """steps 1 - 4's set-up of every segment -> a list of None (draws nothing) or dict(Xa, Ya, Xb, Yb ints, za, zb float32, ymajor)"""
    n = len(seg)
    if n == 0:
        return []
    ca, cb = mat4_point(pvm, seg["a"]), mat4_point(pvm, seg["b"])
    alive = np.isfinite(ca).all(axis=1) & np.isfinite(cb).all(axis=1)
    for k in range(6):
        da, db = _plane(ca, k), _plane(cb, k)
        ia, ib = da >= 0, db >= 0                       # (NaN: outside)
        alive &= ia | ib
        with np.errstate(all="ignore"):
            nb = _lerp(ca, cb, da / (da - db))          # a inside, b outside
            na = _lerp(cb, ca, db / (db - da))          # b inside, a outside
        cb = np.where((ia & ~ib)[:, None], nb, cb).astype(np.float32)
        ca = np.where((ib & ~ia)[:, None], na, ca).astype(np.float32)
    alive &= (ca[:, 3] > 0) & (cb[:, 3] > 0)
    hw, hh = F(0.5) * F(W), F(0.5) * F(H)
    Xa, Ya, za = project(ca, hw, hh)
    Xb, Yb, zb = project(cb, hw, hh)
    out = []
    for i in range(n):
        if not alive[i]:
            out.append(None)
            continue
        xa, xb = (min(max(int(v), 128 * W - REACH), 128 * W + REACH) for v in (Xa[i], Xb[i]))
        ya, yb = (min(max(int(v), 128 * H - REACH), 128 * H + REACH) for v in (Ya[i], Yb[i]))
        a, b = (xa, ya, za[i]), (xb, yb, zb[i])
        dX, dY = xb - xa, yb - ya
        if dX == 0 and dY == 0:
            out.append(None)
            continue
        ymajor = not abs(dX) >= abs(dY)
        if (dY if ymajor else dX) < 0:
            a, b = b, a
        out.append({"Xa": a[0], "Ya": a[1], "za": F(a[2]), "Xb": b[0], "Yb": b[1], "zb": F(b[2]), "ymajor": ymajor})
    return out


def pixels(rec, W, H):
    """step 4: the pixels one record covers -> (xs, ys, k, dM) int64 arrays; k = the centre's distance from the first end along the
    major axis, dM the major delta"""
    if rec is None:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, 0
    Ma, Mb, Na, Nb = (rec["Ya"], rec["Yb"], rec["Xa"], rec["Xb"]) if rec["ymajor"] else (rec["Xa"], rec["Xb"], rec["Ya"], rec["Yb"])
    mlim, nlim = (H, W) if rec["ymajor"] else (W, H)
    dM, dN = Mb - Ma, Nb - Na
    ms, ns, ks = [], [], []
    m = max(0, -((128 - Ma) // 256))                    # the first pixel whose centre 256 m + 128 is >= Ma
    while m < mlim and 256 * m + 128 < Mb:
        k = 256 * m + 128 - Ma
        c = (Na + (2 * k * dN + dM) // (2 * dM)) >> 8
        if 0 <= c < nlim:
            ms.append(m); ns.append(c); ks.append(k)
        m += 1
    ms, ns, ks = (np.asarray(v, dtype=np.int64) for v in (ms, ns, ks))
    return (ns, ms, ks, dM) if rec["ymajor"] else (ms, ns, ks, dM)


def depth_of(rec, k, dM):
    """step 5 over the pixels of one record"""
    za, zb = F(rec["za"]), F(rec["zb"])
    with np.errstate(all="ignore"):
        t = k.astype(np.float32) / F(dM)
        d = fma(t, zb - za, za)
        return np.fmin(np.fmax(d, np.fmin(za, zb)), np.fmax(za, zb)).astype(np.float32)


def blend(p, q, a):
    return (p * (255 - a) + q * a + 127) // 255


def overlay(frame, depth, pvm, seg, style=None, classes=None):
    """frame (H, W, 4) uint8, depth (H, W) float32, pvm (16,) float32, seg a SEGMENT array, style a dict depth_bias / hidden_opacity ->
    (H, W, 4) uint8.  classes: a dict that receives (H, W) bool planes "visible" and "hidden" - the pixels some non-XRAY segment passed
    / failed the depth test at - and "drawn", the pixels any segment covered"""
    st = dict(DEFAULT_STYLE, **(style or {}))
    bias, hidden = F(st["depth_bias"]), int(st["hidden_opacity"])
    H, W = depth.shape
    assert frame.dtype == np.uint8 and frame.shape == (H, W, 4) and depth.dtype == np.float32 and 0 <= hidden <= 255
    out = frame.astype(np.int64)
    if classes is not None:
        classes.update({k: np.zeros((H, W), dtype=bool) for k in ("visible", "hidden", "drawn")})
    for rec, s in zip(setup(pvm, W, H, seg), seg):
        xs, ys, k, dM = pixels(rec, W, H)
        if xs.size == 0:
            continue
        d = depth_of(rec, k, dM)
        with np.errstate(all="ignore"):
            passed = (d - bias) <= depth[ys, xs]        # (NaN: False)
        xray = bool(int(s["flags"]) & XRAY)
        vis = np.ones(xs.size, dtype=bool) if xray else passed
        a0 = int(s["rgba"][3])
        a = np.where(vis, a0, (a0 * hidden + 127) // 255).astype(np.int64)
        for ch in range(3):
            out[ys, xs, ch] = blend(out[ys, xs, ch], int(s["rgba"][ch]), a)
        if classes is not None:
            classes["drawn"][ys, xs] = True
            if not xray:
                classes["visible"][ys[passed], xs[passed]] = True
                classes["hidden"][ys[~passed], xs[~passed]] = True
    return out.astype(np.uint8)
