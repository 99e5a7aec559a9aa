"""The expand stage's definitions restated in NumPy / SciPy, none of the kernels' passes: the nearest object of every pixel as
the minimum of (d², id) over ALL pairs of a pixel and an object pixel in int64 (ref_nearest, small maps), or over the k nearest
object pixels a k-d tree returns, with the proof that no tie was cut off (ref_nearest_tree, large maps); the zones' numbers
as one mask per object, the adjacency as shifted comparisons (contacts_ref), Fractions rounded once for the floats."""

from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree

from coloc_ref import round_sqrt
from contacts_ref import ref_contacts

DIST_INF = 1 << 30
MASK = (1 << 32) - 1


def _objects(labels, nid):
    """-> (coordinates of every pixel int64 (npix, nd), coordinates of the object pixels (m, nd), their ids (m), bad)"""
    lab = np.asarray(labels).astype(np.int64)
    flat = lab.reshape(-1)
    coords = np.indices(lab.shape).reshape(lab.ndim, -1).T.astype(np.int64)
    obj = (flat > 0) & (flat < nid)
    return coords, coords[obj], flat[obj], int(((flat < 0) | (flat >= nid)).any())


def _finish(keys, shape, limit_sq):
    dist, nearest = keys >> 32, keys & MASK
    if limit_sq >= 0:
        beyond = dist > limit_sq
        dist, nearest = np.where(beyond, DIST_INF, dist), np.where(beyond, 0, nearest)
    return nearest.astype(np.int32).reshape(shape), dist.astype(np.int32).reshape(shape)


def ref_nearest(labels, nid, limit_sq=-1):
    """-> (nearest int32, dist_sq int32, bad): over all pairs; a map for which pixels x object pixels stays small"""
    shape = np.asarray(labels).shape
    coords, q, ids, bad = _objects(labels, nid)
    keys = np.full(len(coords), DIST_INF << 32, dtype=np.int64)
    step = max(1, (1 << 22) // max(1, len(q)))
    for at in range(0, len(coords) if len(q) else 0, step):
        d2 = ((coords[at:at + step, None, :] - q[None, :, :]) ** 2).sum(axis=2)
        keys[at:at + step] = ((d2 << 32) | ids[None, :]).min(axis=1)
    return _finish(keys, shape, limit_sq) + (bad,)


def ref_nearest_tree(labels, nid, limit_sq=-1, k=12):
    """the same from the k nearest object pixels of a k-d tree, their d² recomputed in integers; asserts that the k-th lies
    strictly farther than the winner, so that no object pixel at the winner's distance was left out"""
    shape = np.asarray(labels).shape
    coords, q, ids, bad = _objects(labels, nid)
    if len(q) == 0:
        return _finish(np.full(len(coords), DIST_INF << 32, dtype=np.int64), shape, limit_sq) + (bad,)
    k = min(k, len(q))
    _, at = cKDTree(q.astype(np.float64)).query(coords.astype(np.float64), k=k)
    at = at.reshape(len(coords), k)
    d2 = ((coords[:, None, :] - q[at]) ** 2).sum(axis=2)
    keys = ((d2 << 32) | ids[at]).min(axis=1)
    assert k == len(q) or (d2.max(axis=1) > (keys >> 32)).all(), "ref_nearest_tree: k candidates may have cut a tie off"
    return _finish(keys, shape, limit_sq) + (bad,)


def ref_edge_faces(zones, nid):
    """the faces of every id to the outside of the image, int64 (nid)"""
    zones = np.asarray(zones)
    out = np.zeros(nid, dtype=np.int64)
    for axis in range(zones.ndim):
        for at in (0, zones.shape[axis] - 1):
            out += np.bincount(np.take(zones, at, axis=axis).reshape(-1), minlength=nid)
    return out


def ref_zone_table(labels, limit_sq=-1, nearest=ref_nearest):
    """-> (object table, pair table) as zone_table gives them, from one mask per object"""
    labels = np.asarray(labels)
    nd, nid = labels.ndim, int(labels.max()) + 1 if labels.size else 1
    zones, dist, _ = nearest(labels, nid, limit_sq)
    label = np.unique(labels[labels > 0]).astype(np.int64)
    keys, counts = ref_contacts(zones, nd) if len(label) else (np.zeros(0, np.uint64), np.zeros(0, np.int64))
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(MASK)).astype(np.int64)
    edge = ref_edge_faces(zones, nid)
    cols = {name: [] for name in ["area", "zone_area", "zone_fraction", "zone_reach"] + [f"zone_reach_{x}" for x in "zyx"[3 - nd:]]
            + ["zone_dist_sq_mean", "num_neighbours", "zone_border", "zone_border_open"]}
    for i in label:
        mine = zones == i
        d = dist[mine].astype(np.int64)
        area, zone_area = int((labels == i).sum()), int(mine.sum())
        cols["area"].append(area)
        cols["zone_area"].append(zone_area)
        cols["zone_fraction"].append(float(Fraction(area, zone_area)))
        cols["zone_reach"].append(round_sqrt(Fraction(int(d.max()))))
        first = np.argwhere(mine & (dist == d.max()))[0]                  # argwhere lists in raster order
        for x, c in zip("zyx"[3 - nd:], first):
            cols[f"zone_reach_{x}"].append(int(c))
        cols["zone_dist_sq_mean"].append(float(Fraction(int(d.sum()), zone_area)))
        others = ((a == i) | (b == i)) & (a > 0)
        cols["num_neighbours"].append(int(others.sum()))
        cols["zone_border"].append(int(counts[others].sum()))
        cols["zone_border_open"].append(int(counts[(a == 0) & (b == i)].sum()) - int(edge[i]))
    floats = ("zone_fraction", "zone_reach", "zone_dist_sq_mean")
    table = {"label": label}
    table.update({name: np.array(v, dtype=np.float64 if name in floats else np.int64) for name, v in cols.items()})
    return table, {"label_a": a, "label_b": b, "faces": counts}


def dots_map(shape, n, seed, size=2):
    """seeded label map of n small boxes (up to `size` pixels a side) with distinct ids 1 .. n, later ones on top: from a formula
    of the seed alone"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.int32)
    for i in range(1, n + 1):
        corner = [int(rng.integers(0, s)) for s in shape]
        lab[tuple(slice(c, c + int(rng.integers(1, size + 1))) for c in corner)] = i
    return lab
