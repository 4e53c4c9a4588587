"""The numpy statement of the scaled forms' filter (zr_frame_downscale, zr_read_color_scaled, zr_copy_frame_scaled_async, the deltas of a
scaled frame), written from the rule alone and independent of csrc/zr_scale.h: the table is computed here from the float64 formula.

T[c] = floor(65535 * L(c / 255) + 1/2), L the sRGB EOTF.  Output pixel (X, Y) at scale s covers the frame pixels X s <= x < min(W, (X + 1) s),
Y s <= y < min(H, (Y + 1) s), n of them.  R, G, B each: S = the block's sum of T[p]; the result is the number of k in 1..255 with
2 S >= (T[k - 1] + T[k]) n.  A: floor((2 sum + n) / (2 n)).  All of it in int64.
"""
import numpy as np

SCALES = tuple(range(1, 9))


def eotf(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def table_real():
    """65535 * L(c / 255), float64, before rounding"""
    return 65535.0 * eotf(np.arange(256, dtype=np.float64) / 255.0)


def table():
    return np.floor(table_real() + 0.5).astype(np.int64)


T = table()
MID = T[:-1] + T[1:]                     # MID[k - 1] = T[k - 1] + T[k], k = 1 .. 255


def extent(w, h, s):
    return -(-w // s), -(-h // s)


def _block_sums(plane, s):
    """plane (H, W) int64 -> (Hd, Wd) sums over the s x s blocks, the missing pixels of edge blocks counting 0"""
    h, w = plane.shape
    wd, hd = extent(w, h, s)
    pad = np.zeros((hd * s, wd * s), dtype=np.int64)
    pad[:h, :w] = plane
    return pad.reshape(hd, s, wd, s).sum(axis=(1, 3))


def downscale(img, s):
    """img (H, W, 4) uint8 -> (ceil(H / s), ceil(W / s), 4) uint8"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4 and 1 <= s <= 8
    h, w = img.shape[:2]
    n = _block_sums(np.ones((h, w), dtype=np.int64), s)
    out = np.zeros(n.shape + (4,), dtype=np.uint8)
    for ch in range(3):
        two_s = 2 * _block_sums(T[img[:, :, ch]], s)
        out[:, :, ch] = (two_s[:, :, None] >= MID[None, None, :] * n[:, :, None]).sum(axis=2)
    a = _block_sums(img[:, :, 3].astype(np.int64), s)
    out[:, :, 3] = (2 * a + n) // (2 * n)
    return out


def tie_block(k):
    """the 2 x 2 block {k - 1, k - 1, k, k} in every channel: it sits exactly on threshold k and yields k"""
    return np.array([[k - 1, k - 1], [k, k]], dtype=np.uint8)[:, :, None].repeat(4, axis=2)


def tie_image(w, h, shift=0):
    """the 255 tie blocks tiled across a w x h frame, block (bx, by) that of k = 1 + (bx + by * ceil(w / 2) + shift) % 255"""
    img = np.zeros((h, w, 4), dtype=np.uint8)
    nx = -(-w // 2)
    for by in range(-(-h // 2)):
        for bx in range(nx):
            k = 1 + (bx + by * nx + shift) % 255
            blk = tie_block(k)
            y, x = 2 * by, 2 * bx
            img[y:y + 2, x:x + 2] = blk[:min(2, h - y), :min(2, w - x)]
    return img


def digest(buf):
    """FNV-1a over bytes, 64 bits: what tests/frame_scale_check.cpp prints"""
    hsh = 0xCBF29CE484222325
    for b in np.asarray(buf, dtype=np.uint8).reshape(-1).tolist():
        hsh = ((hsh ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return hsh
