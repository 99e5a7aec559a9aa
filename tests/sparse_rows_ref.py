"""NumPy restatement of the list builders of csrc/sparse_rows.hip (clx_changed_rows, clx_changed_tiles).  No device, no
libclx, no 64-bit words: boolean arrays, one OR per window offset, np.flatnonzero per chunk.  Everything here is exact;
the lists are SORTED (the kernels append in no particular order: a test sorts what it got)."""

import numpy as np


def out_extents(shape, window):
    """(OD, OH, OW) of a valid (KD, KH, KW) window over (ID, IH, IW)"""
    return tuple(n - k + 1 for n, k in zip(shape, window))


def changed_rows_ref(clean, noisy, window, chunk):
    """clean (C, ID, IH, IW), noisy (T, C, ID, IH, IW), window (KD, KH, KW) -> (want, lists):
    want (T, OD, OH, OW) bool: some input pixel of the output pixel's window differs from the clean image in some channel
    (numpy's != : a NaN differs from itself, -0.0 equals 0.0);
    lists[k]: the sorted int64 entries of chunk k, (copy inside the chunk) * npix_out + raster(oz, oy, ox); its length is
    the chunk's count."""
    clean, noisy = np.asarray(clean), np.asarray(noisy)
    assert clean.ndim == 4 and noisy.ndim == 5 and noisy.shape[1:] == clean.shape, (clean.shape, noisy.shape)
    T = noisy.shape[0]
    diff = (noisy != clean[None]).any(axis=1)                                    # (T, ID, IH, IW)
    kd, kh, kw = window
    od, oh, ow = out_extents(clean.shape[1:], window)
    assert min(od, oh, ow) >= 1 and chunk >= 1
    want = np.zeros((T, od, oh, ow), bool)
    for dz in range(kd):
        for dy in range(kh):
            for dx in range(kw):
                want |= diff[:, dz:dz + od, dy:dy + oh, dx:dx + ow]
    return want, _chunk_lists(want.reshape(T, -1), chunk)


def changed_tiles_ref(want, WH, WW, tile, chunk):
    """want (T, 1, OH, OW) or (T, OH, OW) bool (changed_rows_ref), a valid (WH, WW) convolution over it in tile x tile
    output tiles -> (changed, lists): changed (T, th, tw) bool: some row of the tile's (tile + WH - 1) x (tile + WW - 1)
    input window, clipped at the bottom and right edge, is changed; lists[k]: the sorted entries of chunk k,
    (copy inside the chunk) * th * tw + ty * tw + tx."""
    want = np.asarray(want, bool)
    if want.ndim == 4:
        assert want.shape[1] == 1, "2-D only"
        want = want[:, 0]
    T, OH, OW = want.shape
    assert 1 <= WH <= OH and 1 <= WW <= OW and tile >= 1 and chunk >= 1
    th, tw = -(-(OH - WH + 1) // tile), -(-(OW - WW + 1) // tile)
    changed = np.zeros((T, th, tw), bool)
    for ty in range(th):
        for tx in range(tw):
            y0, x0 = ty * tile, tx * tile
            changed[:, ty, tx] = want[:, y0:min(y0 + tile + WH - 1, OH), x0:min(x0 + tile + WW - 1, OW)].any(axis=(1, 2))
    return changed, _chunk_lists(changed.reshape(T, -1), chunk)


def _chunk_lists(flags, chunk):
    T = flags.shape[0]
    return [np.flatnonzero(flags[k * chunk:(k + 1) * chunk].reshape(-1)).astype(np.int64)
            for k in range(-(-T // chunk))]


def changed_rows_loops(clean, noisy, window, chunk):
    """changed_rows_ref pixel by pixel, in plain Python: what the tests check the reference against"""
    T, C, ID, IH, IW = noisy.shape
    kd, kh, kw = window
    od, oh, ow = ID - kd + 1, IH - kh + 1, IW - kw + 1
    lists = [[] for _ in range(-(-T // chunk))]
    for t in range(T):
        for oz in range(od):
            for oy in range(oh):
                for ox in range(ow):
                    hit = False
                    for c in range(C):
                        for dz in range(kd):
                            for dy in range(kh):
                                for dx in range(kw):
                                    a = float(clean[c, oz + dz, oy + dy, ox + dx])
                                    b = float(noisy[t, c, oz + dz, oy + dy, ox + dx])
                                    hit = hit or a != b
                    if hit:
                        lists[t // chunk].append((t % chunk) * od * oh * ow + (oz * oh + oy) * ow + ox)
    return lists


def changed_tiles_loops(want, WH, WW, tile, chunk):
    """changed_tiles_ref row by row, in plain Python, from the definition: output tile (ty, tx) covers the output pixels
    [ty * tile, ty * tile + tile) x [tx * tile, ...) that exist; output pixel (y, x) reads rows (y + i, x + j)"""
    T, OH, OW = want.shape
    oh2, ow2 = OH - WH + 1, OW - WW + 1
    th, tw = (oh2 + tile - 1) // tile, (ow2 + tile - 1) // tile
    lists = [[] for _ in range(-(-T // chunk))]
    for t in range(T):
        for ty in range(th):
            for tx in range(tw):
                hit = False
                for y in range(ty * tile, min(ty * tile + tile, oh2)):
                    for x in range(tx * tile, min(tx * tile + tile, ow2)):
                        for i in range(WH):
                            for j in range(WW):
                                hit = hit or bool(want[t, y + i, x + j])
                if hit:
                    lists[t // chunk].append((t % chunk) * th * tw + ty * tw + tx)
    return lists
