"""NumPy restatement of clx_region_order_stats and of the quantile / MAD columns of region_table, for the order
statistics tests.  Keys: the order-preserving 64-bit keys of clx_inst_stats / clx_region_intensity, restated.  Selection: a
plain np.sort of every object's keys (or values).  Columns: NumPy's default ("linear") quantile with the index and the
interpolation in Fractions, one rounding at the end -- np.quantile itself rounds (n - 1) q and is not the definition."""

import math
from fractions import Fraction

import numpy as np

F32, F64, I32 = 0, 1, 2         # clx_raw_type
BAD_LABEL, BAD_VALUE, BAD_AREA, BAD_RANK = 1, 2, 4, 8
ABSENT = np.uint64(0xFFFFFFFFFFFFFFFF)


def raw_type_of(raw):
    return {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}[np.asarray(raw).dtype]


def order_key(values):
    """uint64 keys of a float32, float64 or int32 array: a < b as numbers  <=>  key(a) < key(b) as unsigned integers
    (-0.0 sorts below +0.0); float32 and int32 keys lie in the low 32 bits"""
    v = np.ascontiguousarray(values)
    if v.dtype == np.int32:
        return (v.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    if v.dtype == np.float32:
        b = v.view(np.uint32)
        return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32).astype(np.uint64)
    assert v.dtype == np.float64, v.dtype
    b = v.view(np.uint64)
    top = np.uint64(1 << 63)
    return np.where(b & top, ~b, b | top).astype(np.uint64)


def decode_key(keys, raw_type):
    """the inverse of order_key"""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    if raw_type == I32:
        return (k.astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)
    if raw_type == F32:
        k = k.astype(np.uint32)
        return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)
    top = np.uint64(1 << 63)
    return np.where(k & top, k & ~top, ~k).astype(np.uint64).view(np.float64)


def pixel_keys(labels, raw, nid, centre=None):
    """-> (ids, keys) of the pixels with an id in [1, nid), in raster order"""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    v = np.asarray(raw).reshape(-1)
    inside = (lab >= 1) & (lab < nid)
    ids, v = lab[inside], v[inside]
    if centre is not None:
        v = np.abs(v.astype(np.float64) - np.asarray(centre, dtype=np.float64)[ids])     # one float64 subtraction
    return ids, order_key(v)


def sorted_keys(labels, raw, nid, centre=None):
    """-> {id: sorted uint64 keys} for the present ids in [1, nid)"""
    ids, keys = pixel_keys(labels, raw, nid, centre)
    order = np.lexsort((keys, ids))
    ids, keys = ids[order], keys[order]
    cuts = np.flatnonzero(np.diff(ids)) + 1
    return {int(part_ids[0]): part for part_ids, part in zip(np.split(ids, cuts), np.split(keys, cuts)) if len(part)}


def ref_order_stats(labels, raw, nid, rank, area=None, centre=None):
    """-> (out uint64 (nid, nq), bad).  rank (nid, nq); area: what the caller claims (default: the truth).  Rows of ids whose
    claimed area is not the truth, or that hold a non-finite value, are unspecified: the caller leaves them out."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    v = np.asarray(raw).reshape(-1)
    rank = np.asarray(rank).astype(np.uint64)
    nq = rank.shape[1]
    truth = np.bincount(lab[(lab >= 1) & (lab < nid)], minlength=nid)
    claimed = truth if area is None else np.asarray(area).astype(np.int64)
    bad = 0
    if ((lab < 0) | (lab >= nid)).any():
        bad |= BAD_LABEL
    inside = (lab >= 1) & (lab < nid)
    if v.dtype.kind == "f" and not np.isfinite(v[inside]).all():
        bad |= BAD_VALUE
    if (claimed[1:] != truth[1:]).any():
        bad |= BAD_AREA
    out = np.full((nid, nq), ABSENT, dtype=np.uint64)
    for i, keys in sorted_keys(labels, raw, nid, centre).items():
        for c in range(nq):
            r = int(rank[i, c])
            if r < min(claimed[i], len(keys)):
                out[i, c] = keys[r]
    present = claimed > 0
    present[0] = False
    if (rank[present] >= claimed[present].astype(np.uint64)[:, None]).any():
        bad |= BAD_RANK
    return out, bad


def exact_quantile(sorted_values, q):
    """NumPy's default quantile of an ascending array of finite numbers with the index (n - 1) q, q the float64 it is, and
    the interpolation computed in Fractions: one correctly rounded float64"""
    n = len(sorted_values)
    h = Fraction(float(q)) * (n - 1)
    lo = math.floor(h)
    hi = math.ceil(h)
    number = (lambda x: Fraction(int(x))) if np.asarray(sorted_values).dtype.kind in "ui" else (lambda x: Fraction(float(x)))
    a, b = number(sorted_values[lo]), number(sorted_values[hi])
    return float(a + (b - a) * (h - lo))


def ref_columns(labels, raw, quantiles, mad):
    """-> {name: float64 (objects)} for one channel, names without the _c{k} suffix: "intensity_q<repr(q)>" per quantile and
    "intensity_mad"; objects = the ids present in labels, ascending"""
    lab = np.asarray(labels).reshape(-1)
    v = np.asarray(raw).reshape(-1)
    ids = np.unique(lab[lab > 0])
    cols = {f"intensity_q{float(q)!r}": [] for q in quantiles}
    if mad:
        cols["intensity_mad"] = []
    for i in ids:
        s = np.sort(v[lab == i])
        for q in quantiles:
            cols[f"intensity_q{float(q)!r}"].append(exact_quantile(s, q))
        if mad:
            median = exact_quantile(s, 0.5)
            cols["intensity_mad"].append(exact_quantile(np.sort(np.abs(s.astype(np.float64) - median)), 0.5))
    return {k: np.array(c, dtype=np.float64) for k, c in cols.items()}
