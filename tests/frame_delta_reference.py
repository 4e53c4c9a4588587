"""The statement of a delivery (include/zelda_render.h, "delivering changes") in numpy: which 32 x 32 tiles of a frame differ from what
was delivered last, their pixels packed tile by tile, and what a client does with them."""
import numpy as np

TILE = 32


def tile_grid(W, H):
    """(tiles_x, tiles_y)"""
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tile_pixels(frame, t):
    """Tile t of an (H, W, 4) uint8 frame as (32, 32, 4): tile pixel (x, y) = frame pixel (tx*32 + x, ty*32 + y), 0 outside the frame"""
    H, W = frame.shape[:2]
    tx, ty = t % tile_grid(W, H)[0], t // tile_grid(W, H)[0]
    out = np.zeros((TILE, TILE, 4), dtype=np.uint8)
    part = frame[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
    out[:part.shape[0], :part.shape[1]] = part
    return out


def delta(delivered, frame, full=False):
    """-> (tiles uint32[n] ascending, pixels uint8[n, 32, 32, 4]): the tiles in which any byte of any pixel inside the frame differs
    (every tile when `full`), in increasing t = ty * ceil(W/32) + tx"""
    assert delivered.shape == frame.shape and frame.dtype == np.uint8 and frame.shape[2] == 4
    H, W = frame.shape[:2]
    nx, ny = tile_grid(W, H)
    tiles = [t for t in range(nx * ny)
             if full or not np.array_equal(tile_pixels(delivered, t), tile_pixels(frame, t))]
    pixels = np.zeros((len(tiles), TILE, TILE, 4), dtype=np.uint8)
    for k, t in enumerate(tiles):
        pixels[k] = tile_pixels(frame, t)
    return np.asarray(tiles, dtype=np.uint32), pixels


def apply(client, tiles, pixels):
    """The client's side: every listed tile's pixels inside the frame replace the copy's, in place"""
    H, W = client.shape[:2]
    nx, _ = tile_grid(W, H)
    for k, t in enumerate(np.asarray(tiles).tolist()):
        tx, ty = t % nx, t // nx
        h, w = min(TILE, H - ty * TILE), min(TILE, W - tx * TILE)
        client[ty * TILE:ty * TILE + h, tx * TILE:tx * TILE + w] = pixels[k][:h, :w]
    return client


def untile(tiles, pixels, W, H):
    """A full delivery as a frame"""
    return apply(np.zeros((H, W, 4), dtype=np.uint8), tiles, pixels)


def padding_is_zero(tiles, pixels, W, H):
    """every slot's pixels outside the frame are 0"""
    nx, _ = tile_grid(W, H)
    for k, t in enumerate(np.asarray(tiles).tolist()):
        tx, ty = t % nx, t // nx
        h, w = min(TILE, H - ty * TILE), min(TILE, W - tx * TILE)
        if pixels[k][h:].any() or pixels[k][:, w:].any():
            return False
    return True
