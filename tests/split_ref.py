"""Restatements the split stage is compared with, written from the definitions (cellulus_amd/split.py's docstring), not from the
kernels: the ascent under the total order, the roots, the passes, the merge and the piece table.

Two forms of the device's half.  ``loops_*``: plain Python loops over pixels and neighbours, the definitions word for word,
for small maps.  ``ref_*``: NumPy over shifted views of the padded map, for the one large map and the stage tests; the tests
compare the two on the small cases.  The merge is restated with tuples as keys and dicts, and its depth test
(``ref_shallower``) with Fractions between integer brackets of the square roots, so nothing of ``merge_basins``' algebra is
shared.  The fixtures (discs, ellipses, balls, blob maps) are here too."""

import itertools
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from inscribed_ref import DIST_INF, ref_distance_sq

NONE = -1
DEPTHS = (0, Fraction(1, 4), Fraction(1, 2), 1, Fraction(3, 2), 2, 3, 5, 1000)


def offsets(nd):
    """the 8 / 26 neighbour offsets as (dz, dy, dx), in raster order"""
    zs = (-1, 0, 1) if nd == 3 else (0,)
    return [o for o in itertools.product(zs, (-1, 0, 1), (-1, 0, 1)) if o != (0, 0, 0)]


def forward(nd):
    """the 4 / 13 offsets that come after the pixel in raster order"""
    return [o for o in offsets(nd) if o > (0, 0, 0)]


def _as3(a):
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def _valid(labels, dist_sq):
    """-> (labels int64 with the pixels that are no object pixels as 0, dist int64, info bit 1 as the value 2), all 3-D"""
    lab, d = _as3(labels).astype(np.int64), _as3(dist_sq).astype(np.int64)
    out = (lab != 0) & ((d < 0) | (d > DIST_INF))
    return np.where(out, 0, lab), d, 2 * int(out.any())


# ------------------------------------------------------------------ plain loops
def loops_basins(labels, dist_sq):
    """-> (root int64 in the shape of labels, NONE where no object pixel is; summits ascending; info[0] without bit 2)"""
    nd = np.asarray(labels).ndim
    lab, d, info = _valid(labels, dist_sq)
    Z, Y, X = lab.shape
    idx = lambda z, y, x: (z * Y + y) * X + x                 # noqa: E731
    key = lambda z, y, x: (int(d[z, y, x]), -idx(z, y, x))    # noqa: E731
    up = {}
    for z, y, x in itertools.product(range(Z), range(Y), range(X)):
        if lab[z, y, x] == 0:
            continue
        best = (z, y, x)
        for dz, dy, dx in offsets(nd):
            q = (z + dz, y + dy, x + dx)
            if 0 <= q[0] < Z and 0 <= q[1] < Y and 0 <= q[2] < X and lab[q] == lab[z, y, x] and key(*q) > key(*best):
                best = q
        up[z, y, x] = best
    root = np.full(lab.shape, NONE, dtype=np.int64)
    for p in up:
        q = p
        while up[q] != q:
            assert key(*up[q]) > key(*q)
            q = up[q]
        root[p] = idx(*q)
    summits = np.array(sorted(idx(*p) for p in up if up[p] == p), dtype=np.int64)
    return root.reshape(np.asarray(labels).shape), summits, info


def loops_passes(labels, dist_sq, root):
    """-> {(rootA, rootB): pass} with rootA < rootB"""
    nd = np.asarray(labels).ndim
    lab, d, _ = _valid(labels, dist_sq)
    r = _as3(root)
    Z, Y, X = lab.shape
    out = {}
    for z, y, x in itertools.product(range(Z), range(Y), range(X)):
        if r[z, y, x] == NONE:
            continue
        for dz, dy, dx in forward(nd):
            q = (z + dz, y + dy, x + dx)
            if not (0 <= q[0] < Z and 0 <= q[1] < Y and 0 <= q[2] < X) or r[q] == NONE:
                continue
            if lab[q] == lab[z, y, x] and r[q] != r[z, y, x]:
                pair = (min(int(r[q]), int(r[z, y, x])), max(int(r[q]), int(r[z, y, x])))
                out[pair] = max(out.get(pair, 0), int(min(d[q], d[z, y, x])))
    return out


# ------------------------------------------------------------------ shifted views
def _shifted(a, offset, fill):
    """a[p + offset], `fill` outside the map"""
    padded = np.pad(a, 1, constant_values=fill)
    return padded[tuple(slice(1 + o, 1 + o + n) for o, n in zip(offset, a.shape))]


def ref_up(labels, dist_sq):
    """-> (up as flat raster indices, a pixel that is no object pixel pointing at itself; which pixels are object pixels, flat;
    info[0] without bit 2)"""
    nd = np.asarray(labels).ndim
    lab, d, info = _valid(labels, dist_sq)
    index = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    key = np.where(lab != 0, (d << 32) | (0xFFFFFFFF - index), -1)
    best, up = key.copy(), index.copy()
    for o in offsets(nd):
        k = np.where(_shifted(lab, o, 0) == lab, _shifted(key, o, -1), -1)
        take = k > best
        best, up = np.where(take, k, best), np.where(take, _shifted(index, o, 0), up)
    return up.reshape(-1), lab.reshape(-1) != 0, info


def ref_basins(labels, dist_sq):
    """loops_basins' results from shifted views and pointer doubling"""
    up, obj, info = ref_up(labels, dist_sq)
    index = np.arange(len(up), dtype=np.int64)
    summits = np.flatnonzero(obj & (up == index))
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        up = nxt
    return np.where(obj, up, NONE).reshape(np.asarray(labels).shape), summits, info


def ref_passes(labels, dist_sq, root):
    """loops_passes' table as sorted rows -> (rootA, rootB, pass) int64"""
    nd = np.asarray(labels).ndim
    lab, d, _ = _valid(labels, dist_sq)
    r = _as3(root).astype(np.int64)
    rows = []
    for o in forward(nd):
        rq, lq, dq = _shifted(r, o, NONE), _shifted(lab, o, 0), _shifted(d, o, 0)
        hit = (r != NONE) & (rq != NONE) & (lq == lab) & (rq != r)
        rows.append(np.stack([np.minimum(r, rq)[hit], np.maximum(r, rq)[hit], np.minimum(d, dq)[hit]], axis=1))
    rows = np.concatenate(rows)
    if not len(rows):
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    rows = rows[np.lexsort((-rows[:, 2], rows[:, 1], rows[:, 0]))]          # the largest value of a pair first
    first = np.r_[True, (rows[1:, 0] != rows[:-1, 0]) | (rows[1:, 1] != rows[:-1, 1])]
    return rows[first, 0], rows[first, 1], rows[first, 2]


def passes_of(table):
    """loops_passes' dict as ref_passes' rows"""
    rows = sorted((a, b, v) for (a, b), v in table.items())
    return tuple(np.array([r[k] for r in rows], dtype=np.int64) for k in range(3))


# ------------------------------------------------------------------ the merge
def ref_shallower(a, b, depth):
    """sqrt(a) - sqrt(b) < depth for integers a >= b >= 0 and a Fraction depth: the roots between integer brackets
    isqrt(v 4^k) / 2^k <= sqrt(v) <= (isqrt(v 4^k) + 1) / 2^k, refined until they decide.  Equality (only possible where both are
    squares or equal, which is decided exactly first) does not merge"""
    depth = Fraction(depth)
    ra, rb = math.isqrt(a), math.isqrt(b)
    if a == b or (ra * ra == a and rb * rb == b):
        return ra - rb < depth
    for k in range(0, 400, 8):
        lo_a, lo_b = math.isqrt(a << (2 * k)), math.isqrt(b << (2 * k))
        scale = 1 << k
        if Fraction(lo_a + 1 - lo_b, scale) < depth:                        # an upper bound of the difference
            return True
        if Fraction(lo_a - lo_b - 1, scale) >= depth:                       # a lower bound
            return False
    raise AssertionError("the brackets did not decide")


def ref_merge(summits, summit_labels, summit_d2, passes, depth):
    """the merge rule, word for word -> ({summit: piece id}, [per piece (parent, top, top_d2, pass_d2 or None)])"""
    label = {int(s): int(v) for s, v in zip(summits, summit_labels)}
    d2 = {int(s): int(v) for s, v in zip(summits, summit_d2)}
    key = lambda s: (d2[s], -s)                               # noqa: E731
    cluster = {s: s for s in label}                           # summit -> a representative
    members = {s: [s] for s in label}
    top = {s: s for s in label}
    rows = sorted((-int(v), int(a), int(b)) for a, b, v in zip(*passes))
    for minus, a, b in rows:
        assert a < b
        ca, cb = cluster[a], cluster[b]
        if ca == cb:
            continue
        lo, hi = (ca, cb) if key(top[ca]) < key(top[cb]) else (cb, ca)
        if ref_shallower(d2[top[lo]], -minus, depth):
            for s in members[lo]:
                cluster[s] = hi
            members[hi] += members.pop(lo)
            del top[lo]                                       # hi's top is the higher one already
    order = sorted(members, key=lambda c: (label[top[c]], top[c]))
    number = {c: i + 1 for i, c in enumerate(order)}
    piece = {s: number[cluster[s]] for s in label}
    best = {}
    for minus, a, b in rows:
        if piece[a] != piece[b]:
            for c in (piece[a], piece[b]):
                best[c] = max(best.get(c, -1), -minus)
    return piece, [(label[top[c]], top[c], d2[top[c]], best.get(i + 1)) for i, c in enumerate(order)]


def ref_split(labels, depth=1, edge=False, basins=ref_basins, passes=ref_passes):
    """-> (the new map int64, the piece table as split_table gives it, the number of summits)"""
    labels = np.asarray(labels)
    shape = labels.shape
    dist = ref_distance_sq(labels, edge)
    root, summits, _ = basins(labels, dist)
    flat_lab, flat_d = labels.reshape(-1), dist.reshape(-1)
    piece, rows = ref_merge(summits, flat_lab[summits], flat_d[summits], passes(labels, dist, root), depth)
    id_of = np.zeros(labels.size + 1, dtype=np.int64)         # the last entry serves NONE
    for s, i in piece.items():
        id_of[s] = i
    new = id_of[root.reshape(-1)].reshape(shape)
    n = len(rows)
    area = np.bincount(new.reshape(-1), minlength=n + 1)[1:]
    per_parent = {}
    for parent, _, _, _ in rows:
        per_parent[parent] = per_parent.get(parent, 0) + 1
    table = {"label": np.arange(1, n + 1, dtype=np.int64), "parent": np.array([r[0] for r in rows], dtype=np.int64)}
    where = np.unravel_index(np.array([r[1] for r in rows], dtype=np.int64), shape) if n else (np.zeros(0, np.int64),) * len(shape)
    for axis, c in zip("zyx"[3 - len(shape):], where):
        table[f"summit_{axis}"] = np.asarray(c, dtype=np.int64)
    # the square root of an integer below 2^53 in IEEE arithmetic is the correctly rounded one
    table["summit_radius"] = np.array([math.sqrt(r[2]) for r in rows], dtype=np.float64)
    table["pass_radius"] = np.array([math.nan if r[3] is None else math.sqrt(r[3]) for r in rows], dtype=np.float64)
    table["pieces_of_parent"] = np.array([per_parent[r[0]] for r in rows], dtype=np.int64)
    table["area"] = area.astype(np.int64)
    return new, table, len(summits)


def same_partition(a, b):
    """whether two label maps cut the same pixels into the same sets, whatever the numbering"""
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    if not np.array_equal(a > 0, b > 0):
        return False
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def coarsens(coarse, fine):
    """whether every piece of `fine` lies in one piece of `coarse`"""
    pairs = np.unique(np.stack([np.asarray(fine).reshape(-1), np.asarray(coarse).reshape(-1)], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs)


# ------------------------------------------------------------------ fixtures
def disc(shape, centre, radius, label=1, into=None):
    """a digital disc / ball of an integer radius: the pixels whose distance from `centre` rounds to at most `radius`,
    |p - c|² <= radius² + radius (for integers the same as |p - c| < radius + 1/2)"""
    lab = np.zeros(shape, dtype=np.int32) if into is None else into
    grid = np.indices(shape)
    lab[sum((g - c) ** 2 for g, c in zip(grid, centre)) <= radius * radius + radius] = label
    return lab


def ellipse(shape, centre, length, width, angle):
    """a digital ellipse `length` x `width` pixels across, its long axis turned by `angle` (radians from x towards y): as the
    disc's radius its semi-axes get the half pixel, length / 2 + 1/2 and width / 2 + 1/2"""
    a, b = length / 2 + 0.5, width / 2 + 0.5
    y, x = np.indices(shape).astype(np.float64)
    dy, dx = y - centre[0], x - centre[1]
    u, v = dx * math.cos(angle) + dy * math.sin(angle), -dx * math.sin(angle) + dy * math.cos(angle)
    return ((u / a) ** 2 + (v / b) ** 2 <= 1.0).astype(np.int32)


def two_discs(distance, radius=8):
    lab = disc((2 * radius + 5, 2 * radius + distance + 5), (radius + 2, radius + 2), radius)
    return disc(lab.shape, (radius + 2, radius + 2 + distance), radius, into=lab)


def two_balls(distance, radius=6):
    shape = (2 * radius + 3, 2 * radius + 3, 2 * radius + distance + 3)
    lab = disc(shape, (radius + 1, radius + 1, radius + 1), radius)
    return disc(shape, (radius + 1, radius + 1, radius + 1 + distance), radius, into=lab)


def noise_blobs(seed, shape=(64, 80), sigma=3.0):
    """a thresholded Gaussian-filtered noise image, its 4-connected components as labels: blobs with necks, and objects of
    different labels that touch at corners"""
    image = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    return ndimage.label(image > 0)[0].astype(np.int32)


def serpentine(size):
    """one object one pixel wide that winds through a size x size map: every second row, joined at alternating ends"""
    lab = np.zeros((size, size), dtype=np.int32)
    lab[::2] = 1
    for k, y in enumerate(range(1, size - 1, 2)):
        lab[y, -1 if k % 2 == 0 else 0] = 1
    return lab
