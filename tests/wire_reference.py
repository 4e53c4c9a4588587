"""The wireframe rule in exact rationals: a second statement, written from DESIGN.md section 5, "Wireframe", not from csrc/zr_wire.h.

A pixel (x, y) of a W x H frame was won by a triangle with the float32 clip-space corners (xk, yk, wk), k = 0, 1, 2.
    Hk = (W/2 (xk + wk), H/2 (yk + wk), wk)
    for the edges (0,1), (1,2), (2,0):  l = Ha x Hb,  s = lx (x + 1/2) + ly (y + 1/2) + lz,  n2 = lx^2 + ly^2
    on the wire iff for some edge  n2 > 0  and  s^2 <= r^2 n2,  r = width_256 / 512
Here every value is a fractions.Fraction of the float32 inputs: nothing is rounded.  The float64 statement of the product rounds each
operation; a pixel-edge pair whose s^2 lies within 2^-30, relative, of r^2 n2 without meeting it exactly is UNDECIDED (the two
statements may differ there), an exact tie is decided by the <= and is on.

An edge one of whose corners has a non-finite component has no rational value.  For such an edge this file follows the text's float64
operation order in Python floats (IEEE binary64, like the product's): "a NaN anywhere compares false", and an infinity behaves as IEEE
arithmetic makes it behave.

The blend is the highlight's: floor((p (255 - a) + q a + 127) / 255) per colour channel, A stays.
"""
import math
from fractions import Fraction

import numpy as np

EDGES = ((0, 1), (1, 2), (2, 0))
UNDECIDED_REL = Fraction(1, 1 << 30)
ON, OFF, UNDECIDED = 1, 0, 2


def _finite(c):
    return all(math.isfinite(float(v)) for v in c)


def _screen(c, W, H, num):
    """Hk of one corner; num: Fraction (exact) or float (IEEE)"""
    x, y, w = (num(float(v)) for v in c)
    return (num(W) / 2 * (x + w), num(H) / 2 * (y + w), w)


def _line(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def triangle_lines(corners, W, H):
    """The three edges' lines of one triangle (corners: 3 x (x, y, w) float32): per edge ('exact', (lx, ly, lz)) in Fractions, or
    ('ieee', (lx, ly, lz)) in floats where a corner of the edge is not finite"""
    out = []
    for a, b in EDGES:
        if _finite(corners[a]) and _finite(corners[b]):
            out.append(("exact", _line(_screen(corners[a], W, H, Fraction), _screen(corners[b], W, H, Fraction))))
        else:
            out.append(("ieee", _line(_screen(corners[a], W, H, float), _screen(corners[b], W, H, float))))
    return out


def edge_verdict(line, x, y, width_256):
    """ON / OFF / UNDECIDED for one pixel-edge pair, and whether it is an exact tie"""
    kind, (lx, ly, lz) = line
    if kind == "ieee":
        px, py, r = x + 0.5, y + 0.5, width_256 / 512.0
        s = (lx * px + ly * py) + lz
        n2 = lx * lx + ly * ly
        return (ON if (n2 > 0.0 and s * s <= (r * r) * n2) else OFF), False
    px, py, r = Fraction(2 * x + 1, 2), Fraction(2 * y + 1, 2), Fraction(width_256, 512)
    n2 = lx * lx + ly * ly
    if n2 <= 0:
        return OFF, False
    ss, lim = (lx * px + ly * py + lz) ** 2, r * r * n2
    if ss == lim:
        return ON, True
    if abs(ss - lim) <= UNDECIDED_REL * lim:
        return UNDECIDED, False
    return (ON if ss < lim else OFF), False


def pixel_verdict(lines, x, y, width_256):
    """(verdict of the pixel, its undecided pairs, its exact ties): ON if some edge is ON; else UNDECIDED if some edge is; else OFF"""
    vs = [edge_verdict(l, x, y, width_256) for l in lines]
    und, ties = sum(1 for v, _ in vs if v == UNDECIDED), sum(1 for _, t in vs if t)
    if any(v == ON for v, _ in vs):
        return ON, und, ties
    return (UNDECIDED if und else OFF), und, ties


def blend(p, q, a):
    return (p * (255 - a) + q * a + 127) // 255


def blend_pixel(px, rgba):
    """px, rgba: 4 uint8 each -> the pixel with R, G, B blended at opacity rgba[3]; A stays"""
    return [blend(int(px[k]), int(rgba[k]), int(rgba[3])) for k in range(3)] + [int(px[3])]


def frame(img, prim, corners, style, selected=None):
    """The whole frame: img (H, W, 4) uint8, prim (H, W) uint32, corners (n, 3, 3) float32, style a dict (rgba, width_256, flags),
    selected n flags or None -> (expected (H, W, 4) uint8, verdict (H, W) of ON / OFF / UNDECIDED, dict of counts).  An UNDECIDED pixel's
    expected bytes are the input's."""
    H, W = prim.shape
    n = len(corners)
    only = (style["flags"] & 1) != 0 and selected is not None
    out = np.array(img, dtype=np.uint8, copy=True)
    verdict = np.zeros((H, W), dtype=np.uint8)
    stats = {"pairs": 0, "undecided_pairs": 0, "ties": 0}
    lines = {}
    for y in range(H):
        for x in range(W):
            p = int(prim[y, x])
            if p >= n or (only and not selected[p]):
                continue
            if p not in lines:
                lines[p] = triangle_lines(corners[p], W, H)
            v, und, ties = pixel_verdict(lines[p], x, y, style["width_256"])
            stats["pairs"] += 3; stats["undecided_pairs"] += und; stats["ties"] += ties
            verdict[y, x] = v
            if v == ON:
                out[y, x] = blend_pixel(img[y, x], style["rgba"])
    return out, verdict, stats
