"""The statement of the tile codec (include/zelda_render.h, "delivering changes, compressed") in numpy: a 32 x 32 RGBA8 tile as a record,
a record as a tile, a delivery as a stream of records and what a client does with one.  Written from the format's text, not from the
library: left / upper prediction per channel, zigzag, 64 groups of 64 values (8 x 8 block x channel), a width per group, bit planes.

A tile is (32, 32, 4) uint8 indexed [y, x, channel], as tests/frame_delta_reference.py cuts it (0 outside the frame)."""
import numpy as np

import frame_delta_reference as fdr

TILE = 32
RAW_BYTES = 8 + TILE * TILE * 4          # a mode-1 record, and the longest record there is: 4 104
MODE_CODED, MODE_RAW = 0, 1


class Malformed(ValueError):
    pass


def zigzag(tile):
    """-> (32, 32, 4) uint8: the zigzagged residual of every value against its predictor (left; in column 0 the one above; (0, 0): 0)"""
    t = tile.astype(np.int32)
    pred = np.empty_like(t)
    pred[:, 1:] = t[:, :-1]
    pred[1:, 0] = t[:-1, 0]
    pred[0, 0] = t[0, 0]
    r = (t - pred) & 255
    return np.where(r < 128, 2 * r, 2 * (255 - r) + 1).astype(np.uint8)


def unzigzag(p00, z):
    """the tile whose zigzagged residuals are z (z[0, 0] is not looked at) and whose pixel (0, 0) is p00"""
    z = z.astype(np.int32)
    r = np.where(z & 1, 255 - (z >> 1), z >> 1)
    r[0, 0] = np.asarray(p00, dtype=np.int32)
    col0 = np.cumsum(r[:, 0], axis=0) & 255                   # down column 0 from pixel (0, 0)
    r[:, 0] = col0
    return (np.cumsum(r, axis=1) & 255).astype(np.uint8)       # along every row from its column 0


def groups(z):
    """(32, 32, 4) -> (64, 64): group g = (by * 4 + bx) * 4 + channel, value i = block pixel (i & 7, i >> 3)"""
    return z.reshape(4, 8, 4, 8, 4).transpose(0, 2, 4, 1, 3).reshape(64, 64)


def ungroups(g):
    return g.reshape(4, 4, 4, 8, 8).transpose(0, 3, 1, 4, 2).reshape(TILE, TILE, 4)


def widths(z):
    """-> 64 ints: the bit length of each group's largest value"""
    return [int(m).bit_length() for m in groups(z).max(axis=1)]


def encode_tile(tile):
    """-> the tile's record as bytes"""
    tile = np.ascontiguousarray(tile, dtype=np.uint8)
    assert tile.shape == (TILE, TILE, 4)
    z = zigzag(tile)
    b = widths(z)
    coded = 40 + 8 * sum(b)
    head = bytes(tile[0, 0])
    if coded > RAW_BYTES:
        return head + np.array([RAW_BYTES // 8, MODE_RAW], dtype="<u2").tobytes() + tile.tobytes()
    nib = bytes(b[2 * k] | (b[2 * k + 1] << 4) for k in range(32))
    out = [head, np.array([coded // 8, MODE_CODED], dtype="<u2").tobytes(), nib]
    for vals, bits in zip(groups(z), b):
        for k in range(bits):                                  # word k: bit i = bit k of value i
            out.append(np.packbits((vals >> k) & 1, bitorder="little").tobytes())
    rec = b"".join(out)
    assert len(rec) == coded
    return rec


def decode_record(rec):
    """-> (tile, mode); Malformed where the record contradicts itself"""
    rec = bytes(rec)
    if len(rec) < 8 or len(rec) % 8:
        raise Malformed("length %d" % len(rec))
    p00 = np.frombuffer(rec, dtype=np.uint8, count=4)
    words, mode = (int(v) for v in np.frombuffer(rec, dtype="<u2", count=2, offset=4))
    if words * 8 != len(rec):
        raise Malformed("length word %d in a record of %d bytes" % (words, len(rec)))
    if mode == MODE_RAW:
        if len(rec) != RAW_BYTES:
            raise Malformed("raw record of %d bytes" % len(rec))
        return np.frombuffer(rec, dtype=np.uint8, offset=8).reshape(TILE, TILE, 4).copy(), mode
    if mode != MODE_CODED:
        raise Malformed("mode %d" % mode)
    if len(rec) < 40 or len(rec) > RAW_BYTES:
        raise Malformed("coded record of %d bytes" % len(rec))
    nib = np.frombuffer(rec, dtype=np.uint8, count=32, offset=8)
    b = np.stack([nib & 15, nib >> 4], axis=1).reshape(64).astype(int)
    if (b > 8).any() or 40 + 8 * int(b.sum()) != len(rec):
        raise Malformed("widths %s in a record of %d bytes" % (b.tolist(), len(rec)))
    g = np.zeros((64, 64), dtype=np.uint8)
    at = 40
    for k, bits in enumerate(b):
        for plane in range(bits):
            g[k] |= np.unpackbits(np.frombuffer(rec, dtype=np.uint8, count=8, offset=at), bitorder="little") << plane
            at += 8
    return unzigzag(p00, ungroups(g)), mode


def encode_stream(frame, tiles):
    """The records of `tiles` (ascending) of an (H, W, 4) frame -> (offsets uint32[n + 1], stream uint8[offsets[n]], records in mode 1)"""
    recs = [encode_tile(fdr.tile_pixels(frame, int(t))) for t in tiles]
    offsets = np.zeros(len(recs) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(r) for r in recs])
    raw = sum(1 for r in recs if r[6] == MODE_RAW)
    return offsets, np.frombuffer(b"".join(recs), dtype=np.uint8).copy(), raw


def delta(delivered, frame, full=False):
    """One packed delivery -> (tiles, offsets, stream, raw_tiles): tests/frame_delta_reference.py's list, each listed tile as its record"""
    tiles, _ = fdr.delta(delivered, frame, full)
    return (tiles,) + encode_stream(frame, tiles)


def apply(client, tiles, offsets, stream):
    """The client's side: every record decoded, its pixels inside the frame replace the copy's, in place (nothing is written when any
    part of the delivery is malformed)"""
    H, W = client.shape[:2]
    nx, ny = fdr.tile_grid(W, H)
    tiles, offsets = np.asarray(tiles).astype(np.int64), np.asarray(offsets).astype(np.int64)
    if len(offsets) != len(tiles) + 1 or offsets[0] != 0 or (np.diff(offsets) <= 0).any() or offsets[-1] > len(stream):
        raise Malformed("offsets")
    if (tiles >= nx * ny).any() or (np.diff(tiles) <= 0).any():
        raise Malformed("tiles")
    pixels = [decode_record(bytes(stream[offsets[k]:offsets[k + 1]]))[0] for k in range(len(tiles))]
    return fdr.apply(client, tiles, pixels)


def tile_of_widths(rng, b, p00=None):
    """A tile whose 64 groups have exactly the widths b (a list of 64, or one int for all): residuals drawn below 2^b, one of each group
    at least 2^(b - 1), turned into pixels by inverse prediction"""
    b = [b] * 64 if isinstance(b, int) else list(b)
    g = np.zeros((64, 64), dtype=np.uint8)
    for k, bits in enumerate(b):
        if bits:
            g[k] = rng.integers(0, 1 << bits, size=64)
            g[k, 1 + int(rng.integers(0, 63))] |= 1 << (bits - 1)      # (value 0 of groups 0..3 is pixel (0, 0): its residual is 0)
    z = ungroups(g)
    z[0, 0] = 0
    tile = unzigzag(rng.integers(0, 256, size=4) if p00 is None else p00, z)
    assert widths(zigzag(tile)) == b
    return tile


# What a synthetic tile can be: every width 0..8 in all groups, the longest coded record (widths summing to 508), the shortest raw one
# (509), random bytes (raw) and one colour (40 bytes)
KINDS = list(range(9)) + ["sum508", "sum509", "random", "constant"]


def tile_of_kind(rng, kind):
    if kind == "sum508":
        return tile_of_widths(rng, [8] * 63 + [4])
    if kind == "sum509":
        return tile_of_widths(rng, [8] * 63 + [5])
    if kind == "random":
        return rng.integers(0, 256, size=(TILE, TILE, 4), dtype=np.uint8)
    if kind == "constant":
        return np.broadcast_to(rng.integers(0, 256, size=4, dtype=np.uint8), (TILE, TILE, 4)).copy()
    return tile_of_widths(rng, kind)


def synthetic_frame(W, H, step):
    """An (H, W, 4) frame whose tile t is of kind KINDS[(step + t) % 13], cut at the frame's edge: over steps 0 .. synthetic_steps - 1 tile 0
    (whole, or the frame's least cut one) is of every kind but the last, and no tile is of the same kind twice in a row"""
    nx, ny = fdr.tile_grid(W, H)
    rng = np.random.default_rng(1000 * step + W)
    big = np.zeros((ny * TILE, nx * TILE, 4), dtype=np.uint8)
    for t in range(nx * ny):
        big[t // nx * TILE:t // nx * TILE + TILE, t % nx * TILE:t % nx * TILE + TILE] = tile_of_kind(rng, KINDS[(step + t) % len(KINDS)])
    return np.ascontiguousarray(big[:H, :W])


def synthetic_steps(W, H):
    nx, ny = fdr.tile_grid(W, H)
    return max(1, len(KINDS) + 1 - nx * ny)
