"""Restatement of the measure stage's texture quantities for the tests (no kernel, no cellulus_amd import).

Counts: the grey-level co-occurrence counts of include/clx.h's clx_region_cooccurrence from shifted views of the whole map,
one direction at a time, with np.add.at: vectorised and independent of any bounding box or slab (a box only enters where
a test asks what a stale or wrong one gives).  Levels: the formula of clx.h in float64, in its order of operations.
Features: Haralick's thirteen per object, straight from the definitions, in fractions.Fraction; the entropies are math.fsum
over terms ``x log2 x`` with ``x`` the float64 nearest to the exact probability."""

import math
from fractions import Fraction

import numpy as np

FEATURES = ("asm", "contrast", "correlation", "variance", "idm", "sum_average", "sum_variance", "sum_entropy", "entropy",
            "difference_variance", "difference_entropy", "info_correlation_1", "info_correlation_2")
RATIONAL = ("asm", "contrast", "correlation", "variance", "sum_average", "sum_variance", "difference_variance")


def directions(nd):
    """the offsets of {-1, 0, 1}^nd lexicographically greater than zero, ascending"""
    out = []
    for code in range(3 ** nd):
        d = tuple(code // 3 ** (nd - 1 - a) % 3 - 1 for a in range(nd))
        if d > (0,) * nd:
            out.append(d)
    assert out == sorted(out) and len(out) == (3 ** nd - 1) // 2
    return out


def levels_of(raw, lo, hi, levels):
    """-> (level int64, finite bool) per pixel; the level of a non-finite pixel is meaningless"""
    v = np.asarray(raw).astype(np.float64)
    finite = np.isfinite(v)
    if hi == lo:
        return np.zeros(v.shape, dtype=np.int64), finite
    with np.errstate(all="ignore"):
        f = np.floor((np.where(finite, v, lo) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * np.float64(levels))
        lev = np.where(f >= 0, np.minimum(f, levels - 1), 0.0)
    return lev.astype(np.int64), finite


def ref_cooccurrence(labels, raw, nid, ids, lo, hi, levels, distance, bbox=None):
    """-> dict(counts int32 (nrows, ndir, levels, levels), seen int64 (nrows), bad int32 (1)).
    bbox (nid, 6) inclusive zmin ymin xmin zmax ymax xmax: only pixels p inside the box of their id are visited, and an id
    whose box does not lie inside the map has no pixel; None: every pixel is visited."""
    labels = np.asarray(labels).astype(np.int64)
    nd = labels.ndim
    dirs = directions(nd)
    shape = labels.shape
    lev, finite = levels_of(raw, lo, hi, levels)
    in_range = (labels >= 0) & (labels < nid)
    obj = in_range & (labels > 0)
    bad = int((~in_range).any()) | (2 if (obj & ~finite).any() else 0)
    visited = obj.copy()
    if bbox is not None:
        box = np.asarray(bbox).astype(np.int64).reshape(nid, 6)
        full = (1,) * (3 - nd) + shape
        ok = np.ones(nid, dtype=bool)
        for a in range(3):
            ok &= (box[:, a] >= 0) & (box[:, a] <= box[:, 3 + a]) & (box[:, 3 + a] < full[a])
        l = np.where(obj, labels, 0)
        visited &= ok[l]
        for a, c in zip(range(3 - nd, 3), np.indices(shape)):
            visited &= (c >= box[l, a]) & (c <= box[l, 3 + a])
    usable = visited & finite
    table = np.zeros((nid, len(dirs), levels, levels), dtype=np.int64)
    for k, d in enumerate(dirs):
        src, dst = [], []
        for a in range(nd):
            o = d[a] * distance
            n = shape[a]
            if abs(o) >= n:
                break
            src.append(slice(max(0, -o), n - max(0, o)))
            dst.append(slice(max(0, o), n - max(0, -o)))
        else:
            src, dst = tuple(src), tuple(dst)
            pair = usable[src] & obj[dst] & finite[dst] & (labels[src] == labels[dst])
            np.add.at(table, (labels[src][pair], k, lev[src][pair], lev[dst][pair]), 1)
    per_id = np.bincount(labels[visited], minlength=nid)[:nid]
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    counts = np.zeros((len(ids), len(dirs), levels, levels), dtype=np.int32)
    seen = np.zeros(len(ids), dtype=np.int64)
    good = (ids >= 1) & (ids < nid)
    counts[good] = table[ids[good]]
    seen[good] = per_id[ids[good]]
    return dict(counts=counts, seen=seen, bad=np.array([bad], dtype=np.int32))


def _entropy(probabilities):
    """-Σ x log2 x over Fractions, zero terms contributing 0: fsum of float terms"""
    return -math.fsum(float(x) * math.log2(float(x)) for x in probabilities if x > 0)


def direction_features(C):
    """the thirteen features of one (levels, levels) count matrix with at least one pair -> dict; Fractions for the
    rational ones (idm among them), floats for the entropies and the two information measures"""
    L = len(C)
    S = [[int(C[i][j]) + int(C[j][i]) for j in range(L)] for i in range(L)]
    T = sum(map(sum, S))
    assert T > 0
    p = {(i, j): Fraction(S[i][j], T) for i in range(L) for j in range(L) if S[i][j]}
    px = [sum((v for (i, _), v in p.items() if i == a), Fraction(0)) for a in range(L)]
    mu = sum(i * px[i] for i in range(L))
    var = sum((i - mu) ** 2 * px[i] for i in range(L))
    p_sum = [sum((v for (i, j), v in p.items() if i + j == k), Fraction(0)) for k in range(2 * L - 1)]
    p_diff = [sum((v for (i, j), v in p.items() if abs(i - j) == k), Fraction(0)) for k in range(L)]
    f = {}
    f["asm"] = sum(v * v for v in p.values())
    f["contrast"] = sum(k * k * p_diff[k] for k in range(L))
    f["correlation"] = (sum(i * j * v for (i, j), v in p.items()) - mu * mu) / var if var else Fraction(1)
    f["variance"] = var
    f["idm"] = sum(v / (1 + (i - j) ** 2) for (i, j), v in p.items())
    f["sum_average"] = sa = sum(k * p_sum[k] for k in range(2 * L - 1))
    f["sum_variance"] = sum((k - sa) ** 2 * p_sum[k] for k in range(2 * L - 1))
    f["sum_entropy"] = _entropy(p_sum)
    f["entropy"] = hxy = _entropy(p.values())
    da = sum(k * p_diff[k] for k in range(L))
    f["difference_variance"] = sum((k - da) ** 2 * p_diff[k] for k in range(L))
    f["difference_entropy"] = _entropy(p_diff)
    hx = _entropy(px)
    hxy1 = -math.fsum(float(v) * math.log2(float(px[i] * px[j])) for (i, j), v in p.items())
    hxy2 = -math.fsum(float(px[i] * px[j]) * math.log2(float(px[i] * px[j])) for i in range(L) for j in range(L) if px[i] and px[j])
    f["info_correlation_1"] = (hxy - hxy1) / hx if hx else 0.0
    f["info_correlation_2"] = math.sqrt(max(0.0, 1.0 - 2.0 ** (-2.0 * (hxy2 - hxy))))
    f["_hx"], f["_hxy"], f["_hxy1"], f["_hxy2"] = hx, hxy, hxy1, hxy2             # for the error bars of the tests
    return f


def object_features(C):
    """(ndir, levels, levels) counts of one object -> (pairs, {feature: float, NaN without any pair}, per-direction dicts)"""
    per_dir = [direction_features(M) for M in C if int(np.sum(M)) > 0]
    pairs = int(np.sum(C))
    out = {}
    for name in FEATURES:
        vals = [d[name] for d in per_dir]
        if not vals:
            out[name] = math.nan
        elif isinstance(vals[0], Fraction):
            out[name] = float(sum(vals, Fraction(0)) / len(vals))
        else:
            out[name] = math.fsum(vals) / len(vals)
    return pairs, out, per_dir


def ref_columns(counts):
    """(n, ndir, levels, levels) -> dict of pairs (int64) and the thirteen float64 columns"""
    rows = [object_features(C) for C in np.asarray(counts)]
    cols = {"pairs": np.array([r[0] for r in rows], dtype=np.int64)}
    for name in FEATURES:
        cols[name] = np.array([r[1][name] for r in rows], dtype=np.float64)
    return cols


def ref_bbox(labels, nid):
    """inclusive boxes (nid, 6) as clx_region_moments leaves them: max < min for an absent id"""
    labels = np.asarray(labels)
    nd = labels.ndim
    box = np.zeros((nid, 6), dtype=np.int32)
    box[:, :3] = 0x7FFFFFFF
    box[:, 3:] = -1
    for i in np.unique(labels):
        if 0 < i < nid:
            idx = np.argwhere(labels == i)
            box[i, :3 - nd] = 0
            box[i, 3:6 - nd] = 0
            box[i, 3 - nd:3] = idx.min(axis=0)
            box[i, 6 - nd:] = idx.max(axis=0)
    return box
