"""A restatement of clx_region_products and of the columns formed from it, shared by the colocalization tests.
Quantisation: clx_region_intensity's q (np.rint of an exact scaling, the per-pixel bound 2^62 >> bit_length(npix)).  Classes:
q >= thr per id.  Sums: Python ints (object arrays under np.add.at), or int64 where the caller says the values are small
enough for it.  Columns: Fractions of those ints, rounded ONCE: a ratio by Fraction.__float__, a square root by a 80-digit
Decimal root whose float is then checked, in exact arithmetic, to be the nearest one."""

import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

NW = 20
BAD_LABEL, BAD_VALUE = 1, 2
SUMS = ("n", "sum_a", "sum_b", "n_both", "sum_a_above", "sum_b_above", "sum_a_both", "sum_b_both")
SQUARES = ("sum_aa", "sum_bb", "sum_ab", "sum_aa_both", "sum_bb_both", "sum_ab_both")
M64 = (1 << 64) - 1


def ref_q(raw, shift, npix):
    """-> (q int64, fits bool) per value; q is 0 where it does not fit"""
    raw = np.ascontiguousarray(raw).reshape(-1)
    if raw.dtype.kind in "ui":
        return raw.astype(np.int64), np.ones(raw.shape, bool)
    bound = float(2 ** 62 >> int(npix).bit_length())
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = np.rint(np.ldexp(raw.astype(np.float64), int(shift)))
        fits = np.abs(t) <= bound                            # False for NaN
    return np.where(fits, t, 0.0).astype(np.int64), fits


def ref_products(labels, raw_a, raw_b, nid, shift_a=0, shift_b=0, thr_a=None, thr_b=None, small=False):
    """-> (rows: list of nid lists of 14 Python ints in the order SUMS + SQUARES, bad).  small=True: int64 sums, for maps whose
    values are so small that no sum reaches 2^63 (asserted)"""
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    npix = lab.size
    in_range = (lab >= 0) & (lab < nid)
    bad = 0 if in_range.all() else BAD_LABEL
    ok = in_range & (lab > 0)
    qa, fa = ref_q(raw_a, shift_a, npix)
    qb, fb = ref_q(raw_b, shift_b, npix)
    if (ok & ~(fa & fb)).any():
        bad |= BAD_VALUE
    ok &= fa & fb
    ids, a, b = lab[ok], qa[ok], qb[ok]
    assert (thr_a is None) == (thr_b is None)
    if thr_a is None:
        ua = ub = np.ones(ids.shape, bool)
    else:
        ua, ub = a >= np.asarray(thr_a, dtype=np.int64)[ids], b >= np.asarray(thr_b, dtype=np.int64)[ids]
    both = ua & ub
    if small:
        m = int(max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)))
        assert m * m * max(1, len(ids)) < 2 ** 63
        dt = np.int64
    else:
        dt = object
    a, b = a.astype(dt), b.astype(dt)
    one = np.ones(len(ids), dtype=dt)
    terms = [(one, None), (a, None), (b, None), (one, both), (a, ua), (b, ub), (a, both), (b, both),
             (a * a, None), (b * b, None), (a * b, None), (a * a, both), (b * b, both), (a * b, both)]
    cols = []
    for v, mask in terms:
        acc = np.zeros(nid, dtype=dt)
        if mask is None:
            np.add.at(acc, ids, v)
        else:
            np.add.at(acc, ids[mask], v[mask])
        cols.append([int(x) for x in acc])
    return [list(r) for r in zip(*cols)], bad


def words_of(rows):
    """rows of 14 Python ints -> uint64 (n, 20): clx_region_products' layout, two's complement"""
    out = np.zeros((len(rows), NW), dtype=np.uint64)
    for i, r in enumerate(rows):
        for w in range(8):
            out[i, w] = r[w] & M64
        for p in range(6):
            v = r[8 + p]
            assert -(1 << 127) <= v < (1 << 127)
            out[i, 8 + 2 * p] = v & M64
            out[i, 9 + 2 * p] = (v >> 64) & M64
    return out


def table_of(rows):
    """rows of 14 Python ints -> the dict of cellulus_amd.measure.product_table"""
    t = {}
    for w, name in enumerate(SUMS):
        t[name] = np.array([r[w] for r in rows], dtype=np.int64)
    for p, name in enumerate(SQUARES):
        t[name] = np.empty(len(rows), dtype=object)
        t[name][:] = [r[8 + p] for r in rows]
    return t


def round_sqrt(x):
    """the float64 nearest to sqrt(x), x a non-negative Fraction: a Decimal root to 80 digits, then the proof in exact
    arithmetic that x lies between the squares of the midpoints to the two neighbouring floats"""
    x = Fraction(x)
    assert x >= 0
    if x == 0:
        return 0.0
    getcontext().prec = 80
    r = float((Decimal(x.numerator) / Decimal(x.denominator)).sqrt())
    assert 0.0 < r < math.inf
    lo = (Fraction(r) + Fraction(math.nextafter(r, 0.0))) / 2
    hi = (Fraction(r) + Fraction(math.nextafter(r, math.inf))) / 2
    assert lo * lo <= x <= hi * hi, "round_sqrt: the Decimal root rounded to the wrong float"
    return r


def _scaled(v, e):
    with np.errstate(over="ignore", under="ignore"):
        return float(np.ldexp(np.float64(v), e))


def ref_columns(rows, shift_a=0, shift_b=0, j=0, k=1):
    """every column of one pair from rows of 14 Python ints, as lists of floats: the std of both channels and the seven
    colocalization columns, each a Fraction rounded once and scaled by an exact power of two; NaN for a zero denominator"""
    nan = math.nan
    out = {name: [] for name in [f"intensity_std_c{j}", f"intensity_std_c{k}"] + [f"coloc_{q}_c{j}_c{k}" for q in (
        "pearson", "slope", "overlap", "k1", "k2", "manders1", "manders2")]}
    pair = f"c{j}_c{k}"
    for n, A, B, nb, a_above, b_above, aT, bT, aa, bb, ab, aaT, bbT, abT in rows:
        Va, Vb, C = n * aa - A * A, n * bb - B * B, n * ab - A * B
        out[f"intensity_std_c{j}"].append(_scaled(round_sqrt(Fraction(Va, n * n)), -shift_a) if n else nan)
        if k != j:
            out[f"intensity_std_c{k}"].append(_scaled(round_sqrt(Fraction(Vb, n * n)), -shift_b) if n else nan)
        sign = lambda v: -1.0 if v < 0 else 1.0
        out[f"coloc_pearson_{pair}"].append(sign(C) * round_sqrt(Fraction(C * C, Va * Vb)) if Va * Vb else nan)
        out[f"coloc_slope_{pair}"].append(_scaled(float(Fraction(C, Va)), shift_a - shift_b) if Va else nan)
        out[f"coloc_overlap_{pair}"].append(sign(abT) * round_sqrt(Fraction(abT * abT, aaT * bbT)) if aaT * bbT else nan)
        out[f"coloc_k1_{pair}"].append(_scaled(float(Fraction(abT, aaT)), shift_a - shift_b) if aaT else nan)
        out[f"coloc_k2_{pair}"].append(_scaled(float(Fraction(abT, bbT)), shift_b - shift_a) if bbT else nan)
        out[f"coloc_manders1_{pair}"].append(float(Fraction(aT, a_above)) if a_above else nan)
        out[f"coloc_manders2_{pair}"].append(float(Fraction(bT, b_above)) if b_above else nan)
    return out


def ref_thresholds(qmax, f):
    """ceil(f * qmax) per object, f as the exact value of the float"""
    return np.array([math.ceil(Fraction(float(f)) * int(q)) for q in qmax], dtype=np.int64)


def same_floats(a, b):
    """equal as float64 arrays, NaN matching NaN, -0.0 matching 0.0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
