"""What tests/test_overlay_cpu.py (the host statement, on the CPU oracle's frames) and tests/test_gpu_overlay.py (the kernels, on the
renderer's) share: the shapes, the scene and cameras (tests/highlight_cases.py's), the styles and the segment lists.

A list is built for one frame: its segments are placed in SCREEN terms - through a pixel, along a tile seam, across a frame edge, at an
NDC depth - and taken back to the space of a non-instanced vertex through the float64 inverse of the frame's PVM.  Where a snapped end
lands to the last 1/256 pixel is for the rule to say; every check compares with tests/overlay_reference.py on the same floats.
Every list but "empty" starts with the PROBES: a line in front of everything (NDC depth 0.1), one behind all geometry but in front of
the cleared depth (0.99999: hidden behind geometry, visible over a cleared pixel) and an XRAY line."""
import numpy as np

import highlight_cases as hc
import overlay_reference as ovr

SHAPES = [(66, 34), (257, 131)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
CAMERAS = hc.CAMERAS
STYLES = {"default": {"depth_bias": 0.0, "hidden_opacity": 0}, "biased": {"depth_bias": 1e-4, "hidden_opacity": 96}}
LIST_CAPACITY = 256                # records k_overlay_apply's LDS list holds
MANY = 600                         # segments through one tile: above the capacity twice over, so the list flushes
FRONT, BEHIND = 0.1, 0.99999       # NDC depths: ahead of every surface / behind every surface, ahead of the cleared 1.0

RED, BLUE, GREEN, WHITE, YELLOW = (255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 255), (255, 220, 0)


class Placer:
    """screen -> the space the segments are given in, for one frame's PVM (16 floats, column-major)"""

    def __init__(self, pvm, W, H):
        self.W, self.H = W, H
        self.M = np.asarray(pvm, dtype=np.float64).reshape(4, 4).T      # (row, column)
        self.inv = np.linalg.inv(self.M)

    def point(self, sx, sy, z):
        """the point that projects to pixel coordinates (sx, sy) at NDC depth z"""
        p = self.inv @ np.array([2.0 * sx / self.W - 1.0, 2.0 * sy / self.H - 1.0, z, 1.0])
        return p[:3] / p[3]

    def ray(self, sx, sy, s):
        """along the pixel's ray: s = 0 on the near plane, 1 on the far plane; s_eye(sx, sy) < 0 is the eye"""
        n, f = self.point(sx, sy, 0.0), self.point(sx, sy, 1.0)
        return n + s * (f - n)

    def s_eye(self, sx, sy):
        n, f = self.point(sx, sy, 0.0), self.point(sx, sy, 1.0)
        wn, wf = (self.M @ np.append(n, 1.0))[3], (self.M @ np.append(f, 1.0))[3]
        return -wn / (wf - wn)

    def seg(self, p1, p2, z1, z2, rgb, a=255, flags=0):
        return tuple(self.point(p1[0], p1[1], z1)) + tuple(self.point(p2[0], p2[1], z2)) + tuple(rgb) + (a, flags)

    def seg_rays(self, p1, s1, p2, s2, rgb, a=255, flags=0):
        return tuple(self.ray(p1[0], p1[1], s1)) + tuple(self.ray(p2[0], p2[1], s2)) + tuple(rgb) + (a, flags)


def probes(P):
    W, H = P.W, P.H
    return [P.seg((1.3, 2.2), (W - 1.7, H - 2.6), FRONT, FRONT, YELLOW, 200),
            P.seg((0.4, H - 1.5), (W - 0.6, 0.5), BEHIND, BEHIND, GREEN, 128),
            P.seg((W * 0.5, 0.5), (W * 0.5 + 3.0, H - 0.5), BEHIND, FRONT, WHITE, 90, ovr.XRAY)]


def lists(pvm, W, H):
    """name -> SEGMENT array, for one frame"""
    P = Placer(pvm, W, H)
    rng = np.random.default_rng(W * 1000 + H)
    cx, cy = W * 0.5, H * 0.5
    L = {}
    # axis-aligned, diagonal and steep; ends on pixel centres and on pixel borders; both directions
    L["slopes"] = [P.seg((2.5, 5.5), (W - 3.5, 5.5), FRONT, BEHIND, RED), P.seg((W - 3.0, 8.0), (3.0, 8.0), BEHIND, FRONT, BLUE, 128),
                   P.seg((7.5, 1.5), (7.5, H - 1.5), FRONT, FRONT, GREEN), P.seg((9.0, H - 2.0), (9.0, 2.0), BEHIND, BEHIND, WHITE, 128),
                   P.seg((3.5, 3.5), (3.5 + H - 8, H - 4.5), FRONT, BEHIND, RED, 128), P.seg((W - 4.5, 3.5), (W - 4.5 - (H - 8), H - 4.5), BEHIND, FRONT, BLUE),
                   P.seg((20.25, 1.75), (27.6, H - 2.3), FRONT, BEHIND, YELLOW), P.seg((40.1, H - 1.2), (36.3, 0.7), BEHIND, BEHIND, GREEN, 128),
                   P.seg((1.0, 12.3), (W - 1.0, 15.9), BEHIND, BEHIND, WHITE), P.seg((W - 2.0, 20.7), (2.0, 17.2), FRONT, FRONT, RED, 128)]
    # along the x = 32 and y = 32 tile seams, on either side and on them; through tile corners
    seams = [P.seg((31.5, 0.5), (31.5, H - 0.5), BEHIND, BEHIND, RED), P.seg((32.0, 0.5), (32.0, H - 0.5), FRONT, FRONT, BLUE, 128),
             P.seg((32.5, H - 0.5), (32.5, 0.5), BEHIND, FRONT, GREEN), P.seg((0.5, 31.5), (W - 0.5, 31.5), BEHIND, BEHIND, YELLOW),
             P.seg((W - 0.5, 32.0), (0.5, 32.0), FRONT, BEHIND, WHITE, 128), P.seg((0.5, 32.5), (W - 0.5, 32.5), BEHIND, BEHIND, RED, 128),
             P.seg((22.0, 22.0), (42.0, 42.0), BEHIND, BEHIND, BLUE), P.seg((42.0, 22.0), (22.0, 42.0), FRONT, FRONT, GREEN, 128),
             P.seg((54.0, 22.0), (74.0, 42.0), BEHIND, BEHIND, YELLOW), P.seg((63.5, 31.5), (64.5, 32.5), FRONT, FRONT, RED)]
    L["seams"] = seams
    # wholly off-screen (inside the guard band); crossing each frame edge
    L["edges"] = [P.seg((W + 10.0, 3.0), (W + 50.0, H - 3.0), FRONT, FRONT, RED), P.seg((-40.0, -30.0), (-5.0, -2.0), FRONT, FRONT, RED),
                  P.seg((3.0, H + 5.0), (W - 3.0, H + 9.0), BEHIND, BEHIND, RED), P.seg((-20.0, cy - 3.0), (cx, cy + 2.0), BEHIND, BEHIND, BLUE),
                  P.seg((cx, cy - 4.0), (W + 25.0, cy + 5.0), FRONT, BEHIND, GREEN, 128), P.seg((cx - 6.0, -15.0), (cx + 4.0, cy), BEHIND, BEHIND, YELLOW),
                  P.seg((cx + 9.0, cy), (cx - 2.0, H + 30.0), BEHIND, FRONT, WHITE), P.seg((-9.0, -7.0), (W + 11.0, H + 6.0), BEHIND, BEHIND, RED, 128)]
    # the near plane, the camera's own plane, the far plane
    e1, e2 = P.s_eye(5.0, 4.0), P.s_eye(W - 6.0, H - 5.0)
    L["near_far"] = [P.seg_rays((5.0, 4.0), 0.5 * e1, (W - 6.0, H - 5.0), 0.4, RED),                  # crosses the near plane (w > 0, z < 0 at the first end)
                     P.seg_rays((5.0, H - 4.0), 3.0 * e1, (W - 6.0, 5.0), 0.6, BLUE, 128),            # from behind the camera
                     P.seg_rays((5.0, 4.0), 2.0 * e1, (W - 6.0, H - 5.0), 3.0 * e2, GREEN),          # wholly behind the camera
                     P.seg_rays((8.0, cy), 0.5 * e1, (W - 8.0, cy + 2.0), 0.25 * e2, GREEN),          # wholly between the eye and the near plane
                     P.seg_rays((4.0, cy + 6.0), 0.5, (W - 4.0, cy - 7.0), 1.5, YELLOW),              # crosses the far plane
                     P.seg_rays((4.0, 3.0), 1.2, (W - 4.0, 9.0), 2.5, WHITE)]                        # wholly beyond it
    # past the guard band (NDC beyond +-4), one end or both
    L["guard"] = [P.seg((-6.0 * W, cy - 11.0), (cx, cy + 3.0), BEHIND, BEHIND, RED), P.seg((cx, 2.0), (9.0 * W, H - 2.0), FRONT, BEHIND, BLUE, 128),
                  P.seg((cx - 5.0, -7.0 * H), (cx + 5.0, 8.0 * H), BEHIND, BEHIND, GREEN), P.seg((-5.0 * W, -5.0 * H), (6.0 * W, 6.5 * H), BEHIND, FRONT, YELLOW),
                  P.seg((-9.0 * W, 4.0), (-5.0 * W, 9.0), FRONT, FRONT, WHITE)]
    # zero length, NaN and infinite coordinates
    z = P.seg((cx, cy), (cx, cy), FRONT, FRONT, RED)
    ok = P.seg((3.0, 3.0), (W - 3.0, H - 3.0), FRONT, FRONT, RED)
    bad = []
    for k, v in ((0, np.nan), (4, np.nan), (2, np.inf), (3, -np.inf), (5, np.inf)):
        s = list(ok); s[k] = v; bad.append(tuple(s))
    L["degenerate"] = [z, z[:3] + tuple(P.point(cx + 0.001, cy, FRONT)) + z[6:]] + bad
    # opacity 0, 128, 255, visible and hidden
    L["opacity"] = [P.seg((2.0, 10.0 + 3 * i), (W - 2.0, 11.0 + 3 * i), d, d, c, a) for i, (a, d, c) in
                    enumerate(((0, FRONT, RED), (128, FRONT, RED), (255, FRONT, RED), (0, BEHIND, BLUE), (128, BEHIND, BLUE), (255, BEHIND, BLUE)))]
    # the order rule: red then blue, blue then red, half-transparent, crossing at one pixel
    r = P.seg((cx - 4.0, cy + 0.5), (cx + 5.0, cy + 0.5), FRONT, FRONT, RED, 128)
    b = P.seg((cx + 0.5, cy - 4.0), (cx + 0.5, cy + 5.0), FRONT, FRONT, BLUE, 128)
    L["order_rb"], L["order_br"] = [r, b], [b, r]
    # MANY segments through one tile (the second of the first row where there is one), half-transparent: the LDS list flushes, order holds
    x0 = 32.0 if W > 64 else 0.0
    many = []
    for i in range(MANY):
        p1 = (x0 + rng.uniform(0.0, 32.0), rng.uniform(0.0, min(32.0, H)))
        p2 = (x0 + rng.uniform(0.0, 32.0), rng.uniform(0.0, min(32.0, H)))
        many.append(P.seg(p1, p2, (FRONT, BEHIND)[i % 2], (BEHIND, FRONT, BEHIND)[i % 3], (RED, BLUE, GREEN, YELLOW)[i % 4], (128, 77, 255, 30)[i % 4], i % 5 == 0))
    L["many"] = many
    # the cap: short segments all over the frame
    big = []
    for i in range(ovr.MAX_SEGMENTS):
        p1 = (rng.uniform(-2.0, W + 2.0), rng.uniform(-2.0, H + 2.0))
        p2 = (p1[0] + rng.uniform(-5.0, 5.0), p1[1] + rng.uniform(-5.0, 5.0))
        big.append(P.seg(p1, p2, rng.uniform(0.05, BEHIND), rng.uniform(0.05, BEHIND), tuple(int(v) for v in rng.integers(0, 256, 3)), int(rng.integers(0, 256)), i % 7 == 0))
    out = {k: ovr.segments(probes(P) + v) for k, v in L.items()}
    out["max"] = ovr.segments(big)
    assert len(out["max"]) == ovr.MAX_SEGMENTS and len(out["many"]) > 2 * LIST_CAPACITY
    out["empty"] = ovr.segments([])
    return out


LIST_NAMES = ("slopes", "seams", "edges", "near_far", "guard", "degenerate", "opacity", "order_rb", "order_br", "many", "max", "empty")
GPU_LISTS = ("slopes", "seams", "edges", "near_far", "guard", "degenerate", "opacity", "order_rb", "order_br", "many")      # (max, empty: tests of their own)
