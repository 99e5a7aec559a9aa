"""The skeleton stage's definitions (include/clx.h, "skeleton" stage) restated in NumPy on whole maps: the reference of
tests/test_cpu_skeleton.py, tests/test_gpu_skeleton.py and tests/test_gpu_skeleton_stage.py.  No device, no cellulus_amd."""

import numpy as np

DIST_INF = 1 << 30
# P2 .. P9 = N, NE, E, SE, S, SW, W, NW as (dy, dx), N at y - 1
NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))
WORDS = ("pixels", "face_links", "diag_links", "blocks", "ends", "junctions", "isolated", "d2_sum", "d2_min", "d2_max")


def noise_map(shape, seed, block=12, sigma=2.0, labels=5):
    """Objects of smoothed noise -- blobs with necks, branches and holes -- cut into territories of ``block`` pixels with
    random labels in [1, labels], so that objects of different labels touch.  int32; a 3-D shape is made slice by slice."""
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    out = np.zeros((int(np.prod(shape[:-2], dtype=int)),) + shape[-2:], dtype=np.int32)
    Y, X = shape[-2:]
    for z in range(len(out)):
        smooth = ndimage.gaussian_filter(rng.random((Y + 8, X + 8)), sigma)[4:-4, 4:-4]
        cells = rng.integers(1, labels + 1, size=(Y // block + 1, X // block + 1))
        territory = np.kron(cells, np.ones((block, block), dtype=np.int64))[:Y, :X]
        out[z] = np.where(smooth > np.median(smooth), territory, 0)
    return out.reshape(shape)


def disc(radius, label=1, margin=2):
    n = 2 * radius + 1 + 2 * margin
    yy, xx = np.indices((n, n))
    return np.where((yy - n // 2) ** 2 + (xx - n // 2) ** 2 <= radius ** 2, label, 0).astype(np.int32)


def serpentine(shape, width=5, gap=3, label=1):
    """a band of ``width`` pixels that runs left to right and back over the whole map, ``gap`` background rows between its
    passes"""
    Y, X = shape
    out = np.zeros(shape, dtype=np.int32)
    period, k = width + gap, 0
    for y0 in range(1, Y - width, period):
        out[y0:y0 + width, 1:X - 1] = label
        if y0 + period + width < Y:                      # the turn, at alternating ends
            xs = slice(X - 1 - width, X - 1) if k % 2 == 0 else slice(1, 1 + width)
            out[y0:y0 + period + width, xs] = label
        k += 1
    return out


def _slices(a):
    """a 2-D or 3-D map as [Z][Y][X]: every slice is a map of its own"""
    a = np.asarray(a)
    assert a.ndim in (2, 3)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def shifted(a, dy, dx):
    """b[z, y, x] = a[z, y + dy, x + dx], 0 where that lies outside the slice: rows and slices never wrap"""
    Y, X = a.shape[1:]
    b = np.zeros_like(a)
    ys, xs = slice(max(0, -dy), min(Y, Y - dy)), slice(max(0, -dx), min(X, X - dx))
    yd, xd = slice(max(0, dy), min(Y, Y + dy)), slice(max(0, dx), min(X, X + dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[:, ys, xs] = a[:, yd, xd]
    return b


def thin(labels, iterations=None):
    """Whole-map synchronous thinning -> (the state after ``iterations`` iterations as a map in the shape and dtype of
    ``labels``, the pixels each iteration deleted).  ``iterations=None``: up to and including the first iteration that deletes
    nothing, so the list ends in 0 and the map is the skeleton."""
    labels = np.asarray(labels)
    lab = _slices(labels)
    alive = lab != 0
    same = [alive & (shifted(lab, dy, dx) == lab) for dy, dx in NEIGHBOURS]
    deleted = []
    while iterations is None or len(deleted) < iterations:
        n = 0
        for sub in (1, 2):
            p2, p3, p4, p5, p6, p7, p8, p9 = (s & shifted(alive, dy, dx) for s, (dy, dx) in zip(same, NEIGHBOURS))
            c = ((~p2 & (p3 | p4)).astype(int) + (~p4 & (p5 | p6)).astype(int) + (~p6 & (p7 | p8)).astype(int)
                 + (~p8 & (p9 | p2)).astype(int))
            n1 = (p9 | p2).astype(int) + (p3 | p4).astype(int) + (p5 | p6).astype(int) + (p7 | p8).astype(int)
            n2 = (p2 | p3).astype(int) + (p4 | p5).astype(int) + (p6 | p7).astype(int) + (p8 | p9).astype(int)
            nn = np.minimum(n1, n2)
            m = (p2 | p3 | ~p5) & p4 if sub == 1 else (p6 | p7 | ~p9) & p8
            gone = alive & (c == 1) & (nn >= 2) & (nn <= 3) & ~m
            alive = alive & ~gone
            n += int(gone.sum())
        deleted.append(n)
        if iterations is None and n == 0:
            break
    return np.where(alive, lab, 0).astype(labels.dtype).reshape(labels.shape), deleted


def skeleton(labels):
    return thin(labels)[0]


def census(skel, dist_sq=None, nid=None):
    """-> (words int64 (nid, 10) in the order of ``WORDS``, the bad bits).  ``nid=None``: the largest label + 1."""
    lab = _slices(skel).astype(np.int64)
    if nid is None:
        nid = max(int(lab.max()) + 1, 1) if lab.size else 1
    bad = 0
    outside = (lab < 0) | (lab >= nid)
    if outside.any():
        bad |= 1
        lab = np.where(outside, 0, lab)
    obj = lab != 0

    def same(dy, dx):
        return obj & (shifted(lab, dy, dx) == lab)

    e, s, w, n = same(0, 1), same(1, 0), same(0, -1), same(-1, 0)
    se, sw, nw, ne = same(1, 1) & ~s & ~e, same(1, -1) & ~s & ~w, same(-1, -1) & ~n & ~w, same(-1, 1) & ~n & ~e
    degree = sum(v.astype(int) for v in (e, s, w, n, se, sw, nw, ne))

    def count(mask):
        return np.bincount(lab[mask], minlength=nid).astype(np.int64)

    words = np.zeros((nid, 10), dtype=np.int64)
    words[:, 0] = count(obj)
    words[:, 1] = count(e) + count(s)
    words[:, 2] = count(se) + count(sw)
    words[:, 3] = count(e & s & same(1, 1))
    words[:, 4] = count(obj & (degree == 1))
    words[:, 5] = count(obj & (degree >= 3))
    words[:, 6] = count(obj & (degree == 0))
    words[:, 8], words[:, 9] = DIST_INF, -1
    if dist_sq is not None:
        d = _slices(dist_sq).astype(np.int64)
        ok = obj & (d >= 0) & (d < DIST_INF)
        if (obj & ~ok).any():
            bad |= 2
        for label in np.unique(lab[ok]):                 # Python-int sums
            values = d[ok & (lab == label)]
            words[label, 7:] = sum(int(v) for v in values), int(values.min()), int(values.max())
    return words, bad
