"""A restatement of clx_region_weighted and clx_region_border_intensity and of the columns formed from them, shared by the
weighted / border tests.  Quantisation: coloc_ref.ref_q (clx_region_intensity's q).  Sums: Python ints (object arrays under
np.add.at).  Columns: Fractions of those ints, rounded ONCE: a ratio by Fraction.__float__, a square root by coloc_ref's
round_sqrt (an 80-digit Decimal root whose float is then proved, in exact arithmetic, to be the nearest one)."""

import math
from fractions import Fraction

import numpy as np

from coloc_ref import M64, ref_q, round_sqrt

NW, NB = 21, 7
BAD_LABEL, BAD_VALUE = 1, 2
NO_PEAK = M64
AXES = ("z", "y", "x")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))     # zz yy xx zy zx yx
MOMENTS = ("sum_qz", "sum_qy", "sum_qx", "sum_qzz", "sum_qyy", "sum_qxx", "sum_qzy", "sum_qzx", "sum_qyx")


def ref_keys(raw):
    """region_sums.h's order keys of the values as uint64"""
    raw = np.ascontiguousarray(raw).reshape(-1)
    if raw.dtype == np.int32:
        return (raw.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    bits, top = (raw.view(np.uint32), np.uint32(1 << 31)) if raw.dtype == np.float32 else (raw.view(np.uint64), np.uint64(1 << 63))
    return np.where(bits & top, ~bits, bits | top).astype(np.uint64)


def _shape3(labels):
    labels = np.asarray(labels)
    return (1,) * (3 - labels.ndim) + labels.shape


def _counted(labels, raw, nid, shift):
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    in_range = (lab >= 0) & (lab < nid)
    bad = 0 if in_range.all() else BAD_LABEL
    obj = in_range & (lab > 0)
    q, fits = ref_q(raw, shift, lab.size)
    return lab, obj, q, fits, bad


def ref_max_keys(labels, raw, nid, shift=0):
    """clx_region_intensity's vkey[:, 1]: the largest key over the counted pixels of every id, 0 where there is none"""
    lab, obj, _, fits, _ = _counted(labels, raw, nid, shift)
    ok = obj & fits
    out = np.zeros(nid, dtype=np.uint64)
    np.maximum.at(out, lab[ok], ref_keys(raw)[ok])
    return out


def ref_weighted(labels, raw, nid, shift=0, peak_keys=None, small=False):
    """-> (rows: nid lists [n, Σq, peak, nine sums] of Python ints, bad); labels 2-D or 3-D.  small=True: int64 sums, for maps
    whose values and extents are so small that no sum reaches 2^63 (asserted)"""
    shape = _shape3(labels)
    lab, obj, q, fits, bad = _counted(labels, raw, nid, shift)
    if (obj & ~fits).any():
        bad |= BAD_VALUE
    ok = obj & fits
    ids = lab[ok]
    dt = np.int64 if small else object
    assert not small or int(np.abs(q).max(initial=0)) * max(shape) ** 2 * max(1, len(ids)) < 2 ** 63
    qo = q[ok].astype(dt)
    coords = [c.reshape(-1)[ok].astype(dt) for c in np.indices(shape)]
    cols = []
    for v in [np.ones(len(ids), dtype=dt), qo] + [qo * c for c in coords] + [qo * coords[a] * coords[b] for a, b in PAIRS]:
        acc = np.zeros(nid, dtype=dt)
        np.add.at(acc, ids, v)
        cols.append([int(x) for x in acc])
    peak = np.full(nid, NO_PEAK, dtype=np.uint64)
    if peak_keys is not None:
        hit = ok & (ref_keys(raw) == np.asarray(peak_keys, dtype=np.uint64)[np.where(ok, lab, 0)])
        np.minimum.at(peak, lab[hit], np.flatnonzero(hit).astype(np.uint64))
    cols.insert(2, [int(x) for x in peak])
    return [list(r) for r in zip(*cols)], bad


def weighted_words(rows):
    """rows of 12 Python ints -> uint64 (n, 21): clx_region_weighted's layout, two's complement"""
    out = np.zeros((len(rows), NW), dtype=np.uint64)
    for i, r in enumerate(rows):
        for w in range(3):
            out[i, w] = r[w] & M64
        for p in range(9):
            v = r[3 + p]
            assert -(1 << 127) <= v < (1 << 127)
            out[i, 3 + 2 * p] = v & M64
            out[i, 4 + 2 * p] = (v >> 64) & M64
    return out


def ref_border_mask(labels, nid, nd):
    """bool, in the shape of labels: object pixels (ids in [1, nid)) with a face neighbour of another value or none"""
    labels = np.asarray(labels)
    shape = _shape3(labels)
    lab = labels.reshape(shape).astype(np.int64)
    lab = np.where((lab < 0) | (lab >= nid), 0, lab)
    padded = np.full(tuple(s + 2 for s in shape), -1, dtype=np.int64)
    padded[1:-1, 1:-1, 1:-1] = lab
    border = np.zeros(shape, bool)
    for axis in range(3 - nd, 3):
        for step in (0, 2):
            window = [slice(1, -1)] * 3
            window[axis] = slice(step, shape[axis] + step)
            border |= padded[tuple(window)] != lab
    return (border & (lab > 0)).reshape(labels.shape)


def ref_border(labels, raw, nid, nd, shift=0, small=False):
    """-> (rows: nid lists [border pixels, counted, Σq, min key, max key, Σq²] of Python ints, bad); small as in ref_weighted"""
    lab, obj, q, fits, bad = _counted(labels, raw, nid, shift)
    border = ref_border_mask(labels, nid, nd).reshape(-1)
    if (border & ~fits).any():
        bad |= BAD_VALUE
    ok = border & fits
    keys = ref_keys(raw)
    dt = np.int64 if small else object
    assert not small or int(np.abs(q).max(initial=0)) ** 2 * max(1, int(ok.sum())) < 2 ** 63
    qo = q[ok].astype(dt)
    nb, nc, sq, sqq = (np.zeros(nid, dtype=dt) for _ in range(4))
    np.add.at(nb, lab[border], 1)
    np.add.at(nc, lab[ok], 1)
    np.add.at(sq, lab[ok], qo)
    np.add.at(sqq, lab[ok], qo * qo)
    kmin, kmax = np.full(nid, M64, dtype=np.uint64), np.zeros(nid, dtype=np.uint64)
    np.minimum.at(kmin, lab[ok], keys[ok])
    np.maximum.at(kmax, lab[ok], keys[ok])
    return [[int(v) for v in r] for r in zip(nb, nc, sq, kmin, kmax, sqq)], bad


def border_words(rows):
    """rows of 6 Python ints -> uint64 (n, 7): clx_region_border_intensity's layout"""
    out = np.zeros((len(rows), NB), dtype=np.uint64)
    for i, r in enumerate(rows):
        for w in range(5):
            out[i, w] = r[w] & M64
        assert 0 <= r[5] < (1 << 127)
        out[i, 5], out[i, 6] = r[5] & M64, r[5] >> 64
    return out


def _scaled(v, e):
    with np.errstate(over="ignore", under="ignore"):
        return float(np.ldexp(np.float64(v), e))


def _frac(num, den):
    return float(Fraction(num, den)) if den else math.nan


def ref_weighted_columns(area, sum1, rows, shift, nd, k, shape):
    """the weighted columns of channel k as lists: rows of 12 Python ints of the same objects as area (n) and sum1 (n, 3)"""
    shape = (1,) * (3 - nd) + tuple(int(s) for s in shape)
    axes = range(3 - nd, 3)
    out = {f"intensity_sum_c{k}": []}
    out.update({f"centroid_weighted_{AXES[a]}_c{k}": [] for a in axes})
    out.update({f"cov_weighted_{AXES[a]}{AXES[b]}_c{k}": [] for a, b in PAIRS if a >= 3 - nd})
    out[f"mass_displacement_c{k}"] = []
    out.update({f"intensity_peak_{AXES[a]}_c{k}": [] for a in axes})
    for A, s1, r in zip(area, sum1, rows):
        A, s1 = int(A), [int(v) for v in s1]
        Q, peak, m1, m2 = r[1], r[2], r[3:6], r[6:12]
        out[f"intensity_sum_c{k}"].append(_scaled(float(Q), -shift))
        for a in axes:
            out[f"centroid_weighted_{AXES[a]}_c{k}"].append(_frac(m1[a], Q))
        for p, (a, b) in enumerate(PAIRS):
            if a >= 3 - nd:
                out[f"cov_weighted_{AXES[a]}{AXES[b]}_c{k}"].append(_frac(Q * m2[p] - m1[a] * m1[b], Q * Q))
        d2 = sum((Fraction(s1[a], A) - Fraction(m1[a], Q)) ** 2 for a in axes) if Q else None
        out[f"mass_displacement_c{k}"].append(round_sqrt(d2) if Q else math.nan)
        assert peak != NO_PEAK
        where = np.unravel_index(peak, shape)
        for a in axes:
            out[f"intensity_peak_{AXES[a]}_c{k}"].append(int(where[a]))
    return out


def ref_border_columns(rows, shift, dtype, k):
    """the border columns of channel k (the pixel count apart): lists of floats, and arrays of the raw dtype for the minimum and
    the maximum; rows of 6 Python ints; dtype: the raw channel's"""
    from cellulus_amd.segment import _decode_keys

    raw_type = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2}[np.dtype(dtype)]
    out = {f"intensity_border_{name}_c{k}": [] for name in ("sum", "mean", "std")}
    for _, n, s, _, _, ss in rows:
        out[f"intensity_border_sum_c{k}"].append(_scaled(float(s), -shift))
        out[f"intensity_border_mean_c{k}"].append(_scaled(_frac(s, n), -shift))
        out[f"intensity_border_std_c{k}"].append(_scaled(round_sqrt(Fraction(n * ss - s * s, n * n)), -shift) if n else math.nan)
    keys = np.array([[r[3], r[4]] for r in rows], dtype=np.uint64).reshape(-1, 2)
    values = _decode_keys(keys, raw_type)
    out[f"intensity_border_min_c{k}"] = values[:, 0].copy()      # in the raw dtype
    out[f"intensity_border_max_c{k}"] = values[:, 1].copy()
    return out
