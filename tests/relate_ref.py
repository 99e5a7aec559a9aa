"""The relate stage's definitions restated in plain NumPy, none of the kernels' or the host module's passes: np.unique over the
stacked pairs for the overlaps, a loop over the objects with one mask each for parents, tables and clearance, Fractions
rounded once for the floats."""

import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from coloc_ref import round_sqrt

DIST_INF = 1 << 30
ALL_ONES = (1 << 64) - 1


def blob_map(shape, n, seed, scale=4):
    """seeded label map of n ellipsoids that may cover one another, on background; semi-axes up to extent / scale"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.int32)
    grid = np.indices(shape).astype(np.float64)
    for i in range(1, n + 1):
        centre = [rng.uniform(0, s) for s in shape]
        radius = [rng.uniform(1.0, max(2.0, s / scale)) for s in shape]
        lab[sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radius)) <= 1.0] = i
    return lab


def clamp(labels, nid):
    """labels as int64, out-of-range ones as 0 -> (flat map, whether there was one)"""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    out = (lab < 0) | (lab >= nid)
    return np.where(out, 0, lab), bool(out.any())


def ref_overlaps(a, b, nid_a, nid_b):
    """-> (keys uint64 sorted, counts int64, info[0] without bit 2)"""
    fa, bad_a = clamp(a, nid_a)
    fb, bad_b = clamp(b, nid_b)
    keep = (fa > 0) | (fb > 0)
    if not keep.any():
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), int(bad_a) | 2 * int(bad_b)
    pairs, counts = np.unique(np.stack([fa[keep], fb[keep]], axis=1), axis=0, return_counts=True)
    pairs = pairs.reshape(-1, 2)
    keys = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    return keys, counts.astype(np.int64), int(bad_a) | 2 * int(bad_b)


def ref_parents(a, b):
    """-> (label, parent, overlap) int64 of every id of a: the b > 0 under most of its pixels, the smallest among equals"""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    label = np.unique(a[a > 0])
    parent, overlap = [], []
    for i in label:
        under = b[a == i]
        under = under[under > 0]
        count = np.bincount(under) if len(under) else np.zeros(1, np.int64)
        j = int(np.argmax(count))                               # the first maximum: the smallest id
        parent.append(j)
        overlap.append(int(count[j]) if j else 0)
    return label, np.array(parent, np.int64), np.array(overlap, np.int64)


def ref_clearance(a, b, dist_sq, parent, nid_a):
    """-> (rows: nid_a lists of 3 Python ints, bad)"""
    fa, bad_a = clamp(a, nid_a)
    fb = np.asarray(b).astype(np.int64).reshape(-1)
    d = np.asarray(dist_sq).astype(np.int64).reshape(-1)
    parent = np.asarray(parent).astype(np.int64)
    rows, bad_d = [[0, ALL_ONES, 0] for _ in range(nid_a)], False
    for i in range(1, nid_a):
        if parent[i] <= 0:
            continue
        p = np.flatnonzero((fa == i) & (fb == parent[i]))
        wrong = (d[p] < 0) | (d[p] > DIST_INF)
        bad_d |= bool(wrong.any())
        p = p[~wrong]
        if len(p):
            rows[i] = [len(p), min((int(d[q]) << 32) | int(q) for q in p), int(d[p].sum())]
    return rows, int(bad_a) | 2 * int(bad_d)


def clearance_words(rows):
    return np.array([[v & ALL_ONES for v in r] for r in rows], dtype=np.uint64).reshape(-1, 3)


def _centroid(mask):
    pts = np.argwhere(mask)
    return [Fraction(int(pts[:, k].sum()), len(pts)) for k in range(mask.ndim)]


def ref_relate(children, parents, clearance=False, edge=False):
    """-> (child table, parent table) as dicts of arrays, one mask pass per object"""
    a, b = np.asarray(children).astype(np.int64), np.asarray(parents).astype(np.int64)
    nd = a.ndim
    label, parent, overlap = ref_parents(a, b)
    child = {k: [] for k in ("label", "area", "parent", "overlap", "fraction_inside", "outside", "num_parents", "parent_centroid_distance")}
    if clearance:
        child.update({k: [] for k in ["clearance"] + [f"clearance_{x}" for x in "zyx"[3 - nd:]] + ["depth_sq_mean"]})
        pad = np.pad(b, 1) if edge else b
    for i, j, n in zip(label, parent, overlap):
        m = a == i
        area = int(m.sum())
        under = b[m]
        child["label"].append(int(i)); child["area"].append(area); child["parent"].append(int(j)); child["overlap"].append(int(n))
        child["fraction_inside"].append(int(n) / area)
        child["outside"].append(int((under == 0).sum()))
        child["num_parents"].append(len(np.unique(under[under > 0])))
        if j:
            ca, cb = _centroid(m), _centroid(b == j)
            child["parent_centroid_distance"].append(round_sqrt(sum((x - y) ** 2 for x, y in zip(ca, cb))))
        else:
            child["parent_centroid_distance"].append(math.nan)
        if clearance:
            inside = m & (b == j) if j else np.zeros_like(m)
            if not inside.any():
                values = [math.nan] + [-1] * nd + [math.nan]
            elif (pad == j).all():
                first = np.argwhere(inside)[0]
                values = [math.inf] + [int(v) for v in first] + [math.inf]
            else:
                d = ndimage.distance_transform_edt(pad == j)
                d2 = np.rint(d * d).astype(np.int64)
                d2 = d2[(slice(1, -1),) * nd] if edge else d2
                least = int(d2[inside].min())
                first = np.argwhere(inside & (d2 == least))[0]                  # argwhere lists in raster order
                values = [round_sqrt(least)] + [int(v) for v in first] + [int(d2[inside].sum()) / int(inside.sum())]
            for k, v in zip(list(child)[-(nd + 2):], values):
                child[k].append(v)
    table = {k: [] for k in ("label", "area", "num_children", "children_area", "children_fraction", "tertiary_area")}
    for j in np.unique(b[b > 0]):
        m = b == j
        area, covered = int(m.sum()), int((m & (a > 0)).sum())
        table["label"].append(int(j)); table["area"].append(area); table["num_children"].append(int((parent == j).sum()))
        table["children_area"].append(covered); table["children_fraction"].append(covered / area); table["tertiary_area"].append(area - covered)
    floats = ("fraction_inside", "parent_centroid_distance", "clearance", "depth_sq_mean", "children_fraction")
    return tuple({k: np.array(v, dtype=np.float64 if k in floats else np.int64) for k, v in t.items()} for t in (child, table))
