"""tests/qb3_mosaic.py -- the mosaic contract of include/qb3x.h in plain numpy: a W x H raster as a grid of tw x th tiles.

grid(W, H, tw, th)      (tx, ty): tiles a row, rows of tiles
cut(raster, tw, th)     the tiles, tile k = j * tx + i at index k: pixel (x, y) of it is raster pixel
                        (min(i * tw + x, W - 1), min(j * th + y, H - 1)) -- edge tiles repeat the last column and row
paste(tiles, W, H)      the raster back: tile k's pixels at (i * tw, j * th), clipped to W x H
"""
import numpy as np


def grid(W, H, tw, th):
    if not (W and H and tw and th):
        return 0, 0
    return -(-W // tw), -(-H // th)


def cut(raster, tw, th):
    """raster: (H, W, bands).  Returns (tx * ty, th, tw, bands), contiguous."""
    H, W, b = raster.shape
    tx, ty = grid(W, H, tw, th)
    tiles = np.empty((tx * ty, th, tw, b), dtype=raster.dtype)
    for j in range(ty):
        ys = np.minimum(np.arange(j * th, j * th + th), H - 1)
        for i in range(tx):
            xs = np.minimum(np.arange(i * tw, i * tw + tw), W - 1)
            tiles[j * tx + i] = raster[ys][:, xs]
    return tiles


def paste(tiles, W, H):
    """tiles: (n, th, tw, bands) in the order of cut.  Returns (H, W, bands)."""
    n, th, tw, b = tiles.shape
    tx, ty = grid(W, H, tw, th)
    assert n == tx * ty
    raster = np.empty((H, W, b), dtype=tiles.dtype)
    for j in range(ty):
        for i in range(tx):
            h, w = min(th, H - j * th), min(tw, W - i * tw)
            raster[j * th:j * th + h, i * tw:i * tw + w] = tiles[j * tx + i, :h, :w]
    return raster
