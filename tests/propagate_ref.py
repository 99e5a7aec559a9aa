"""The propagate stage's definitions restated twice, neither the kernel's tiles nor its rounds: a heap Dijkstra on the key
(cost, id) in plain loops (ref_propagate), and the Jacobi relaxation key[q] = min(key[q], key[p] + step(p, q)) over shifted
views of the whole map, iterated until nothing changes (ref_propagate_sweeps, for maps too large for the loops).  Both -> (owner
int32, cost int32, info bits).  The fixtures of the tests live here too: a serpentine corridor, seeded dots, a ridge image."""

import heapq
import itertools

import numpy as np

from nearest_ref import dots_map  # noqa: F401  (the seeds of the tests: small boxes with distinct ids)

COST_INF = 1 << 30
MAX_WEIGHT = 65535


def offsets(nd):
    """the 8 / 26 neighbour offsets with the chamfer weight of each: 3 face, 4 edge, 5 corner"""
    return [(d, 2 + sum(v != 0 for v in d)) for d in itertools.product((-1, 0, 1), repeat=nd) if any(d)]


def _roles(seeds, mask, weight, nid):
    """-> (ids int64 with the out-of-range ones 0, source, enterable, weight int64 with the out-of-range ones 0, info)"""
    ids = np.asarray(seeds).astype(np.int64)
    bad = (ids < 0) | (ids >= nid)
    ids = np.where(bad, 0, ids)
    seed = ids > 0
    allowed = np.ones(ids.shape, bool) if mask is None else np.asarray(mask) != 0
    w = np.zeros(ids.shape, np.int64) if weight is None else np.asarray(weight).astype(np.int64)
    assert allowed.shape == ids.shape == w.shape
    wbad = (w < 0) | (w > MAX_WEIGHT)
    info = int(bad.any()) | 2 * int((wbad & (allowed | seed)).any())
    return ids, seed & ~wbad, allowed & ~seed & ~wbad, np.where(wbad, 0, w), info


def _limit(limit):
    return COST_INF - 1 if limit is None or limit < 0 else int(limit)


def ref_propagate(seeds, mask=None, weight=None, nid=None, reg=1, limit=None):
    """heap Dijkstra on (cost, id): a key only grows along a path, so the first time a pixel leaves the heap with its current
    key that key is final"""
    nid = int(np.max(seeds)) + 1 if nid is None else nid
    ids, source, enter, w, info = _roles(seeds, mask, weight, nid)
    shape, lim, steps = ids.shape, _limit(limit), offsets(ids.ndim)
    cost, owner = np.full(shape, COST_INF, np.int64), np.zeros(shape, np.int64)
    heap = []
    for p in zip(*np.nonzero(source)):
        cost[p], owner[p] = 0, ids[p]
        heap.append((0, int(ids[p]), p))
    heapq.heapify(heap)
    while heap:
        c, i, p = heapq.heappop(heap)
        if (c, i) != (cost[p], owner[p]):
            continue
        for d, a in steps:
            q = tuple(x + y for x, y in zip(p, d))
            if any(x < 0 or x >= n for x, n in zip(q, shape)) or not enter[q]:
                continue
            nc = c + reg * a + abs(int(w[p]) - int(w[q]))
            if nc <= lim and (nc, i) < (cost[q], owner[q]):
                cost[q], owner[q] = nc, i
                heapq.heappush(heap, (nc, i, q))
    return owner.astype(np.int32), cost.astype(np.int32), info


def ref_propagate_sweeps(seeds, mask=None, weight=None, nid=None, reg=1, limit=None, max_sweeps=None):
    """the Jacobi relaxation on int64 keys (cost << 32) | id over shifted views"""
    nid = int(np.max(seeds)) + 1 if nid is None else nid
    ids, source, enter, w, info = _roles(seeds, mask, weight, nid)
    lim, steps, none = _limit(limit), offsets(ids.ndim), COST_INF << 32
    key = np.where(source, ids, none)
    wide = np.pad(w, 1)
    sweeps = 0
    while True:
        padded = np.pad(key, 1, constant_values=none)
        best = key.copy()
        for d, a in steps:
            view = tuple(slice(1 + v, 1 + v + n) for v, n in zip(d, key.shape))
            cand = padded[view] + ((reg * a + np.abs(w - wide[view])) << 32)
            best = np.minimum(best, np.where((cand >> 32) <= lim, cand, none))
        new = np.where(enter, best, key)
        if np.array_equal(new, key):
            break
        key, sweeps = new, sweeps + 1
        assert max_sweeps is None or sweeps <= max_sweeps, "ref_propagate_sweeps: more sweeps than the caller expects"
    return (key & 0xFFFFFFFF).astype(np.int32), (key >> 32).astype(np.int32), info


def serpentine(shape):
    """uint8 mask of a corridor one pixel wide through a 2-D map: the even rows, joined at alternating ends by one pixel of
    the odd row between them (rows two apart are no neighbours, so the only way is along the corridor)"""
    Y, X = shape
    mask = np.zeros(shape, np.uint8)
    mask[::2] = 1
    for y in range(1, Y - 1, 2):
        mask[y, X - 1 if (y // 2) % 2 == 0 else 0] = 1
    return mask


def ridge_image(shape=(9, 15), column=7, open_rows=2, height=200):
    """int32 grey levels: 0 but for a wall `height` high in `column` that leaves the last `open_rows` rows open"""
    image = np.zeros(shape, np.int32)
    image[:shape[0] - open_rows, column] = height
    return image


def random_case(rng, nd):
    """-> (seeds, mask or None, weight or None, reg): a random small map, shapes 3 .. 11 an axis"""
    shape = tuple(int(v) for v in rng.integers(3, 12, size=nd))
    seeds = np.where(rng.random(shape) < 0.08, rng.integers(1, 6, size=shape), 0).astype(np.int32)
    if not seeds.any():
        seeds[tuple(int(rng.integers(0, s)) for s in shape)] = 3
    mask = (rng.random(shape) < 0.75).astype(np.uint8) if rng.random() < 0.7 else None
    weight = rng.integers(0, int(rng.choice([2, 4, 300])), size=shape).astype(np.int32) if rng.random() < 0.7 else None
    return seeds, mask, weight, int(rng.integers(0, 3))


def ref_propagate_table(seeds, owner, cost, mask=None):
    """the columns of propagate_table from one mask per object"""
    from fractions import Fraction

    seeds, owner, cost = np.asarray(seeds), np.asarray(owner), np.asarray(cost).astype(np.int64)
    nd = seeds.ndim
    label = np.unique(seeds[seeds > 0]).astype(np.int64)
    allowed = np.ones(seeds.shape, bool) if mask is None else np.asarray(mask) != 0
    unreached = int((allowed & (owner == 0)).sum())
    cols = {name: [] for name in ["seed_area", "area", "reach_cost"] + [f"reach_{x}" for x in "zyx"[3 - nd:]] + ["cost_mean", "unreached"]}
    for i in label:
        mine = owner == i
        c = cost[mine]
        cols["seed_area"].append(int((seeds == i).sum()))
        cols["area"].append(int(mine.sum()))
        cols["reach_cost"].append(int(c.max()))
        first = np.argwhere(mine & (cost == c.max()))[0]
        for x, v in zip("zyx"[3 - nd:], first):
            cols[f"reach_{x}"].append(int(v))
        cols["cost_mean"].append(float(Fraction(int(c.sum()), int(mine.sum()))))
        cols["unreached"].append(unreached)
    table = {"label": label}
    table.update({name: np.array(v, dtype=np.float64 if name == "cost_mean" else np.int64) for name, v in cols.items()})
    return table
