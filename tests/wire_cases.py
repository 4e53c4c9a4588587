"""The table tests/test_wire_cpu.py holds engine.frame_wire to tests/wire_reference.py on.  A case is one small frame: a winner plane,
the primitives' clip-space corners, a style and, for some, the selection flags.  The host statement tests a pixel against the lines of
whatever triangle its winner names, inside it or not, so a frame whose every pixel names one triangle probes that triangle's lines over
the whole frame.

Classes (a case's `cls`):
  random      random triangles, w in [0.5, 4], two per frame, winners drawn at random among them, "beyond n_prims" and "none"
  wneg        a corner behind the eye (w < 0)
  tie_axis    dyadic axis-aligned edges placed so that pixel centres lie EXACTLY r from the line (s^2 = r^2 n2: the <= decides, on)
  tie_345     dyadic edges of direction (3, 4) / (4, -3): n2 = 25 L^2 is a square, so exact ties exist off the axes too
  dyadic_45   dyadic 45-degree edges.  (No pixel can tie exactly here: s^2 = r^2 n2 needs (dx - dy)^2 = 2 r^2 with dx - dy and r dyadic.
              The class is kept for its exact arithmetic right beside the threshold.)
  coincident  two or all three projected corners coincide: n2 = 0, no wire from that edge
  subpixel    triangles smaller than a pixel
  nonfinite   NaN and infinite corner components
  selected    ZR_WIRE_SELECTED with flags (only flagged primitives get a wire), and with no flags given (every primitive does)
  beyond      winners at or above n_prims, 0xFFFFFFFF among them: never a wire
Every width of WIDTHS occurs in the classes random, tie_axis and tie_345."""
import numpy as np

WIDTHS = (1, 256, 1024, 4096)
CLASSES = ("random", "wneg", "tie_axis", "tie_345", "dyadic_45", "coincident", "subpixel", "nonfinite", "selected", "beyond")
NONE = 0xFFFFFFFF


def _case(cls, name, W, H, corners, prim, width, rng, flags=0, selected=None, rgba=None):
    corners = np.asarray(corners, dtype=np.float32).reshape(-1, 3, 3)
    img = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    if rgba is None:
        rgba = tuple(int(v) for v in rng.integers(0, 256, size=3)) + (int(rng.choice([255, 255, 128, 1, 0])),)
    return {"cls": cls, "name": name, "W": W, "H": H, "corners": corners, "prim": np.asarray(prim, dtype=np.uint32).reshape(H, W), "img": img,
            "style": {"rgba": rgba, "width_256": width, "flags": flags}, "selected": selected}


def _clip(sx, sy, w, W, H):
    """the clip-space (x, y, w) whose homogeneous screen position is (sx w, sy w, w): x = (2 sx / W - 1) w"""
    return [(2.0 * sx / W - 1.0) * w, (2.0 * sy / H - 1.0) * w, w]


def cases():
    rng = np.random.default_rng(20261021)
    out = []
    # random: two triangles per frame
    for width in WIDTHS:
        for rep in range(2):
            W, H = 24, 16
            w = rng.uniform(0.5, 4.0, size=(2, 3))
            xy = rng.uniform(-1.5, 1.5, size=(2, 3, 2)) * w[..., None]
            corners = np.concatenate([xy, w[..., None]], axis=2)
            prim = rng.choice(np.array([0, 1, 2, NONE], dtype=np.uint32), size=(H, W), p=[0.45, 0.45, 0.05, 0.05])
            out.append(_case("random", "random_w%d_%d" % (width, rep), W, H, corners, prim, width, rng))
    # wneg: one corner behind the eye
    for width in (256, 1024):
        W, H = 20, 12
        corners = [[[-0.5, -0.6, 1.0], [0.7, -0.2, 2.0], [0.3, 0.9, -0.75]], [[0.1, 0.2, -1.5], [-0.8, 0.4, 1.0], [0.5, -0.9, 1.25]]]
        prim = (np.arange(W * H).reshape(H, W) // 7 % 2).astype(np.uint32)
        out.append(_case("wneg", "wneg_w%d" % width, W, H, corners, prim, width, rng))
    # tie_axis: a vertical line at screen x = X0 and a horizontal one at y = Y0, both dyadic, with pixel centres exactly r away
    for width in WIDTHS:
        W, H = 32, 32
        r = width / 512.0
        X0, Y0 = 10.5 + r, 6.5 + r                                             # the centres of column 10 and of row 6 lie exactly r away
        corners = [[_clip(X0, 1.0, 1.0, W, H), _clip(X0, 30.0, 2.0, W, H), _clip(X0, 16.0, 0.5, W, H)],      # all three on x = X0 (n2 > 0, one line)
                   [_clip(2.0, Y0, 1.0, W, H), _clip(29.0, Y0, 4.0, W, H), _clip(31.0, 31.0, 1.0, W, H)]]
        prim = (np.arange(W * H).reshape(H, W) % 2).astype(np.uint32)
        out.append(_case("tie_axis", "tie_axis_w%d" % width, W, H, corners, prim, width, rng))
    # tie_345: the line 4 (px - X0) - 3 (py - Y0) = 0; |4 dx - 3 dy| = 5 r at pixel centres for suitable dyadic (X0, Y0)
    for width in WIDTHS:
        W, H = 32, 32
        r = width / 512.0
        # centre (i + 1/2, j + 1/2): 4 i - 3 j + 1/2 - (4 X0 - 3 Y0) = +-5 r; with Y0 = 0 and 4 X0 = 1/2 - 5 r + 4 k the centres with 4 i - 3 j = 4 k tie
        X0 = (0.5 - 5.0 * r) / 4.0 + 10.0
        a, b = (X0 + 3.0 * 2.0, 4.0 * 2.0), (X0 + 3.0 * 7.0, 4.0 * 7.0)         # two points of the line through (X0, 0) along (3, 4)
        corners = [[_clip(a[0], a[1], 1.0, W, H), _clip(b[0], b[1], 2.0, W, H), _clip(a[0] + 4.0, a[1] - 3.0, 1.0, W, H)]]      # third corner: along (4, -3) from a
        out.append(_case("tie_345", "tie_345_w%d" % width, W, H, corners, np.zeros((H, W), dtype=np.uint32), width, rng))
    # dyadic_45
    for width in (256, 1024):
        W, H = 16, 16
        corners = [[_clip(2.0, 1.0, 1.0, W, H), _clip(13.0, 12.0, 2.0, W, H), _clip(13.0, 1.0, 0.5, W, H)],
                   [_clip(1.25, 12.75, 1.0, W, H), _clip(12.25, 1.75, 1.0, W, H), _clip(1.25, 1.75, 1.0, W, H)]]
        prim = (np.arange(W * H).reshape(H, W) // 3 % 2).astype(np.uint32)
        out.append(_case("dyadic_45", "dyadic_45_w%d" % width, W, H, corners, prim, width, rng))
    # coincident: c0 == c1 (edge 0-1 has n2 = 0; the other two are one line), all three equal (no wire), equal after projection only
    W, H = 16, 12
    p, q = _clip(4.0, 3.0, 1.0, W, H), _clip(12.0, 9.0, 2.0, W, H)
    corners = [[p, p, q], [p, p, p], [_clip(4.0, 3.0, 1.0, W, H), _clip(4.0, 3.0, 2.0, W, H), q]]
    prim = (np.arange(W * H).reshape(H, W) % 3).astype(np.uint32)
    out.append(_case("coincident", "coincident", W, H, corners, prim, 256, rng))
    # subpixel
    for width in (1, 256):
        W, H = 12, 10
        corners = [[_clip(5.4, 4.4, 1.0, W, H), _clip(5.7, 4.5, 1.5, W, H), _clip(5.5, 4.7, 0.75, W, H)],
                   [_clip(7.51, 2.49, 1.0, W, H), _clip(7.52, 2.5, 1.0, W, H), _clip(7.5, 2.52, 1.0, W, H)]]
        prim = (np.arange(W * H).reshape(H, W) % 2).astype(np.uint32)
        out.append(_case("subpixel", "subpixel_w%d" % width, W, H, corners, prim, width, rng))
    # nonfinite
    W, H = 12, 8
    nan, inf = float("nan"), float("inf")
    corners = [[[nan, 0.0, 1.0], [0.5, 0.5, 1.0], [-0.5, 0.25, 1.0]], [[0.0, 0.0, inf], [0.5, 0.5, 1.0], [-0.5, 0.25, 1.0]],
               [[inf, -0.5, 1.0], [0.5, -inf, 1.0], [-0.5, 0.25, 1.0]], [[0.25, 0.5, nan], [nan, nan, nan], [0.0, 0.0, 1.0]]]
    prim = (np.arange(W * H).reshape(H, W) % 4).astype(np.uint32)
    out.append(_case("nonfinite", "nonfinite", W, H, corners, prim, 1024, rng))
    # selected: with flags, and with the style's flag but no flags given
    W, H = 20, 14
    w = rng.uniform(0.5, 2.0, size=(4, 3))
    xy = rng.uniform(-1.0, 1.0, size=(4, 3, 2)) * w[..., None]
    corners = np.concatenate([xy, w[..., None]], axis=2)
    prim = rng.integers(0, 4, size=(H, W)).astype(np.uint32)
    out.append(_case("selected", "selected_flags", W, H, corners, prim, 1024, rng, flags=1, selected=np.array([1, 0, 0, 7], dtype=np.uint8)))
    out.append(_case("selected", "selected_none_flagged", W, H, corners, prim, 1024, rng, flags=1, selected=np.zeros(4, dtype=np.uint8)))
    out.append(_case("selected", "selected_absent", W, H, corners, prim, 1024, rng, flags=1, selected=None))
    out.append(_case("selected", "flags_without_the_style_bit", W, H, corners, prim, 1024, rng, flags=0, selected=np.array([1, 0, 0, 1], dtype=np.uint8)))
    # beyond
    W, H = 9, 7
    prim = np.array([1, 2, 1000, NONE, 0x80000000, 1, 1], dtype=np.uint32)[np.arange(W * H) % 7].reshape(H, W)
    out.append(_case("beyond", "beyond", W, H, [[_clip(1.0, 1.0, 1.0, W, H), _clip(8.0, 2.0, 1.0, W, H), _clip(3.0, 6.0, 1.0, W, H)]], prim, 4096, rng))
    out.append(_case("beyond", "no_prims", 5, 3, np.zeros((0, 3, 3)), np.zeros((3, 5), dtype=np.uint32), 256, rng))
    # frames of one row, one column, one pixel
    for W, H in ((1, 1), (1, 9), (9, 1)):
        out.append(_case("random", "thin_%dx%d" % (W, H), W, H, [[_clip(0.25, 0.0, 1.0, W, H), _clip(0.75, H, 2.0, W, H), _clip(W, 0.5, 1.0, W, H)]],
                         np.zeros((H, W), dtype=np.uint32), 256, rng))
    return out
