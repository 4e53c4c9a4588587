"""The numpy statement of highlighting a selection, written from the rule alone (include/zelda_render.h, "highlighting a selection"):

    M(x, y) = 1 iff the winner at (x, y) is a scene primitive whose slot is in the set (0 outside the frame)
    M = 1:                                        R, G, B blended with fill
    M = 0, some M = 1 within |dx|, |dy| <= r:     R, G, B blended with outline
    else, and A always:                           unchanged
    blend(p, q, a) = floor((p (255 - a) + q a + 127) / 255)

It imports nothing of csrc/."""
import numpy as np

RADII = tuple(range(9))
DEFAULT = {"outline": (255, 160, 0, 255), "fill": (255, 160, 0, 0), "radius": 2}
# the four styles of the tests, less the radius: opaque, half-opaque, fill on, everything transparent
STYLES = {
    "opaque": {"outline": (255, 160, 0, 255), "fill": (255, 160, 0, 0)},
    "half": {"outline": (10, 200, 255, 128), "fill": (0, 0, 0, 0)},
    "fill": {"outline": (255, 255, 255, 127), "fill": (40, 90, 250, 77)},
    "clear": {"outline": (255, 0, 0, 0), "fill": (0, 255, 0, 0)},
}


def style(name, radius):
    return dict(STYLES[name], radius=radius)


def blend(p, q, a):
    """per channel, on int64 arrays or ints"""
    return (p * (255 - a) + q * a + 127) // 255


def slots_of(object_plane, slot_base):
    """(H, W, 2) {object, instance} (all ones = none) -> (H, W) int64 slot, -1 = none; slot_base[o] = object o's first slot"""
    obj = object_plane[..., 0].astype(np.int64)
    none = object_plane[..., 0] == 0xFFFFFFFF
    base = np.asarray(slot_base, dtype=np.int64)
    return np.where(none, -1, base[np.where(none, 0, obj)] + object_plane[..., 1].astype(np.int64))


def mask_of(object_plane, the_set, slot_base):
    """M as (H, W) bool: the_set is a flag per slot"""
    s = slots_of(object_plane, slot_base)
    flags = np.asarray(the_set) != 0
    return np.where(s >= 0, flags[np.maximum(s, 0)], False) if flags.size else np.zeros(s.shape, dtype=bool)


def dilate(mask, r):
    """some M = 1 within |dx| <= r, |dy| <= r: shifted ORs over a zero-padded mask"""
    H, W = mask.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    pad[r:r + H, r:r + W] = mask
    out = np.zeros((H, W), dtype=bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + H, dx:dx + W]
    return out


def highlight(frame, mask, st):
    """frame (H, W, 4) uint8, mask (H, W) non-zero = highlighted, st a dict outline / fill / radius -> (H, W, 4) uint8"""
    mask = np.asarray(mask) != 0
    r = int(st["radius"])
    assert 0 <= r <= 8 and frame.dtype == np.uint8 and frame.shape[:2] == mask.shape
    ring = dilate(mask, r) & ~mask
    out = frame.copy()
    rgb = frame[..., :3].astype(np.int64)
    for where, colour in ((mask, st["fill"]), (ring, st["outline"])):
        q = np.array(colour[:3], dtype=np.int64)
        mixed = blend(rgb, q[None, None, :], int(colour[3])).astype(np.uint8)
        out[..., :3] = np.where(where[..., None], mixed, out[..., :3])
    return out
