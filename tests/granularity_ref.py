"""NumPy restatement of the granularity stage's definitions (include/clx.h, cellulus_amd/granularity.py), written from them:
erosion / dilation by shifted views with an explicit inside set, reconstruction by dilation twice -- the whole-map update
iterated to its fixed point, and a max-heap flood over (value, pixel) -- and the granular spectrum with Python-int sums.
Nothing here has tiles, rounds or scans but ``row_by_clamps``, which restates the clamp algebra of the kernel's row scan."""

import heapq

import numpy as np

MAX_LEVEL = 65535


def inside_of(shape, mask):
    return np.ones(shape, bool) if mask is None else np.asarray(mask) != 0


def shifted(a, axis, d, fill):
    """b[p] = a[p + d * e_axis], ``fill`` where that lies beyond the map: rows and slices never wrap"""
    out = np.full_like(a, fill)
    src, dst = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    src[axis], dst[axis] = (slice(d, None), slice(0, -d)) if d > 0 else (slice(0, d), slice(-d, None))
    out[tuple(dst)] = a[tuple(src)]
    return out


def cleaned(values, inside):
    """-> (int64 values with 0 on outside pixels and where an inside value leaves [0, 65535], whether one did)"""
    v = np.asarray(values).astype(np.int64)
    bad = inside & ((v < 0) | (v > MAX_LEVEL))
    return np.where(inside & ~bad, v, 0), bool(bad.any())


def ref_morph(image, mask=None, op=0, steps=1):
    """``steps`` steps of erosion (``op`` 0) or dilation (1) -> (out int32, the bad bit)"""
    image = np.asarray(image)
    inside = inside_of(image.shape, mask)
    v, bad = cleaned(image, inside)
    neutral = 0 if op else MAX_LEVEL
    pick = np.maximum if op else np.minimum
    cur = np.where(inside, v, neutral)
    for _ in range(steps):
        nxt = cur.copy()
        for axis in range(image.ndim):
            for d in (-1, 1):
                nxt = pick(nxt, shifted(cur, axis, d, neutral))
        cur = np.where(inside, nxt, neutral)                 # an outside pixel keeps the neutral value: nothing passes through it
    return np.where(inside, cur, 0).astype(np.int32), int(bad)


def ball_footprint(nd, k):
    """the L1 ball of radius k as a boolean footprint"""
    grid = np.indices((2 * k + 1,) * nd) - k
    return np.abs(grid).sum(axis=0) <= k


def _start(marker, image, mask):
    image = np.asarray(image)
    inside = inside_of(image.shape, mask)
    m, bad_m = cleaned(marker, inside)
    v, bad_v = cleaned(image, inside)
    return np.minimum(m, v), v, int(bad_m) | int(bad_v) << 1


def ref_reconstruct_sweeps(marker, image, mask=None):
    """the update of the whole map iterated until nothing changes -> (out int32, the bad bits, the sweeps that changed it)"""
    r, v, bad = _start(marker, image, mask)
    sweeps = 0
    while True:
        nxt = r.copy()
        for axis in range(r.ndim):
            for d in (-1, 1):
                nxt = np.maximum(nxt, shifted(r, axis, d, 0))
        nxt = np.minimum(nxt, v)                             # v is 0 on outside pixels: they stay 0 and conduct nothing
        if np.array_equal(nxt, r):
            return r.astype(np.int32), bad, sweeps
        r, sweeps = nxt, sweeps + 1


def ref_reconstruct(marker, image, mask=None):
    """a flood from the highest value down: a pixel is final when it leaves the heap -> (out int32, the bad bits)"""
    r, v, bad = _start(marker, image, mask)
    shape = r.shape
    r, v = r.reshape(-1).copy(), v.reshape(-1)
    strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
    heap = [(-int(r[p]), int(p)) for p in np.flatnonzero(r > 0)]
    heapq.heapify(heap)
    while heap:
        neg, p = heapq.heappop(heap)
        if -neg < r[p]:
            continue
        rest = p
        for axis, stride in enumerate(strides):
            c, rest = divmod(rest, stride)
            for d in (-1, 1):
                if 0 <= c + d < shape[axis]:
                    q = p + d * stride
                    cand = min(-neg, int(v[q]))
                    if cand > r[q]:
                        r[q] = cand
                        heapq.heappush(heap, (-cand, q))
    return r.reshape(shape).astype(np.int32), bad


def clamp_then(a, b):
    """the clamp x -> min(hi, max(lo, x)) ``a = (lo, hi)`` followed by the clamp ``b``, as one clamp"""
    return min(b[1], max(b[0], a[0])), min(b[1], max(b[0], a[1]))


def row_by_clamps(r, image, carry):
    """r[q] <- min(I[q], max(r[q], r[q - 1])) along a row, ``carry`` before the first pixel, by an inclusive doubling scan over
    the clamps (r[q], I[q]) the way a wave makes it"""
    f = [(int(lo), int(hi)) for lo, hi in zip(r, image)]
    d = 1
    while d < len(f):
        f = [clamp_then(f[q - d], f[q]) if q >= d else f[q] for q in range(len(f))]
        d *= 2
    return [min(hi, max(lo, int(carry))) for lo, hi in f]


def row_serial(r, image, carry):
    out = []
    for lo, hi in zip(r, image):
        carry = min(int(hi), max(int(lo), int(carry)))
        out.append(carry)
    return out


def object_sums(labels, values):
    """-> (the labels present, ascending; the sum of ``values`` over each as a Python int)"""
    labels = np.asarray(labels)
    ids = np.unique(labels[labels > 0]).astype(np.int64)
    return ids, [int(np.asarray(values, dtype=np.int64)[labels == i].sum()) for i in ids]


def ref_spectrum(labels, levels, scales, background=0):
    """-> (ids, S): S[i] the list of the objects' sums of r_i as Python ints, i = 0 .. scales"""
    g = np.asarray(levels).astype(np.int64)
    if background:
        g = g - ref_morph(ref_morph(g, None, 0, background)[0], None, 1, background)[0]
    ids, s0 = object_sums(labels, g)
    sums, e = [s0], g
    for _ in range(scales):
        e = ref_morph(e, None, 0, 1)[0]
        sums.append(object_sums(labels, ref_reconstruct(e, g)[0])[1])
    return ids, sums


def ref_columns(sums, k=0):
    """the columns from exact fractions, one rounding each"""
    from fractions import Fraction

    table = {}
    for i in range(1, len(sums) + 1):
        num = sums[i - 1] if i == len(sums) else [a - b for a, b in zip(sums[i - 1], sums[i])]
        name = f"granularity_residual_c{k}" if i == len(sums) else f"granularity_{i}_c{k}"
        table[name] = np.array([float(Fraction(100 * n, s0)) if s0 else float("nan") for n, s0 in zip(num, sums[0])], dtype=np.float64)
    return table


def blob_image(shape, centres, sigmas, peak=200.0, floor=10.0):
    """float64 image: a flat floor and a Gaussian blob of height ``peak`` and width sigma at every centre"""
    grid = np.indices(shape).astype(np.float64)
    image = np.full(shape, floor)
    for centre, sigma in zip(centres, sigmas):
        d2 = sum((g - c) ** 2 for g, c in zip(grid, centre))
        image += peak * np.exp(-d2 / (2.0 * sigma * sigma))
    return image


def quadrant_scene(size=96, small=1.5, large=5.0):
    """(labels, image): four square objects, one a quadrant; objects 1 and 2 hold blobs of width ``small``, 3 and 4 of ``large``"""
    labels = np.zeros((size, size), np.int32)
    half, centres, sigmas = size // 2, [], []
    for n, (y0, x0) in enumerate(((0, 0), (0, half), (half, 0), (half, half))):
        labels[y0 + 3:y0 + half - 3, x0 + 3:x0 + half - 3] = n + 1
        sigma = small if n < 2 else large
        step = 10 if n < 2 else 20
        for cy in range(y0 + 10, y0 + half - 8, step):
            for cx in range(x0 + 10, x0 + half - 8, step):
                centres.append((cy, cx))
                sigmas.append(sigma)
    return labels, blob_image((size, size), centres, sigmas)


def serpentine(shape):
    """bool map of a corridor one pixel wide: the even rows, joined at alternating ends by one pixel of the odd row between"""
    Y, X = shape
    path = np.zeros(shape, bool)
    path[::2] = True
    for y in range(1, Y - 1, 2):
        path[y, X - 1 if (y // 2) % 2 == 0 else 0] = True
    return path


def random_levels(rng, shape, top=50):
    return rng.integers(0, top, size=shape).astype(np.int32)
