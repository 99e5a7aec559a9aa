"""The host side of the radial distribution, without a device: the ring and wedge rules of tests/radial_ref.py (what the
kernel is compared with) against their float formulas away from the ties and by hand on them, radial_columns against a
restatement in Fractions, the argument checks, the declarations."""

import ctypes
import math
import os
import re
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

from cellulus_amd.measure import MAX_RINGS, RADIAL_TABLE_BYTES, _check_radial, radial_columns
from radial_ref import (DIST_INF, ref_distance_sq, ref_inscribed, ref_radial, ref_rings, ref_wedge, ring_absolute, ring_relative,
                        rows_of_all)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.mark.parametrize("rings", [1, 2, 3, 4, 7, 32])
def test_ring_rule_against_the_float_formula(rings):
    D2 = np.repeat(np.arange(1, 4097, dtype=np.int64), 16)
    # every d2 for D2 <= 64, and 16 spread over [1, D2] above that (the ends among them)
    pairs = [(d, D) for D in range(1, 65) for d in range(1, D + 1)]
    steps = np.linspace(0.0, 1.0, 16)
    d2 = np.rint(1 + steps[None, :] * (np.arange(1, 4097)[:, None] - 1)).astype(np.int64).reshape(-1)
    d2 = np.concatenate([d2, np.array([p[0] for p in pairs], dtype=np.int64)])
    D2 = np.concatenate([D2, np.array([p[1] for p in pairs], dtype=np.int64)])
    got = ref_rings(d2, D2, rings, 0)
    f = rings * np.sqrt(d2 / D2)
    clear = np.abs(f - np.rint(f)) >= 1e-9
    assert clear.sum() > len(f) // 2 or rings == 1
    assert np.array_equal(got[clear], (np.ceil(f) - 1).astype(np.int64)[clear])
    assert got.min() >= 0 and got.max() <= rings - 1
    # on the ties the inequality decides: rings * sqrt(d2 / D2) an integer m puts the pixel in ring m - 1
    for d, D in ((1, 4), (4, 16), (9, 16), (16, 16), (1, 1024), (DIST_INF, DIST_INF), (1, DIST_INF)):
        f2 = Fraction(d * rings * rings, D)
        want = next(k for k in range(rings) if f2 <= (k + 1) ** 2)
        assert ring_relative(d, D, rings) == want == int(ref_rings([d], [D], rings, 0)[0])
    some = np.random.default_rng(rings).integers(0, len(d2), 300)
    assert [ring_relative(d2[i], D2[i], rings) for i in some] == got[some].tolist()


@pytest.mark.parametrize("rings", [1, 2, 3, 4, 7, 32])
def test_ring_rule_over_all_pairs_up_to_4096(rings):
    """every (d2, D2) with d2 <= D2 <= 4096, about 8.4 million pairs, vectorised.  Where rings * sqrt(d2 / D2) is within 1e-9 of
    an integer m it IS m: its square is a ratio with a denominator of at most 4096, so it misses m^2 by 1 / 4096 or not at all"""
    D = np.arange(1, 4097, dtype=np.int64)
    for lo in range(1, 4097, 512):
        d = np.arange(lo, lo + 512, dtype=np.int64)
        dd, DD = np.meshgrid(d, D, indexing="ij")
        ok = dd <= DD
        got = ref_rings(dd[ok], DD[ok], rings, 0)
        f = rings * np.sqrt(dd[ok] / DD[ok])
        clear = np.abs(f - np.rint(f)) >= 1e-9
        assert np.array_equal(got[clear], (np.ceil(f) - 1).astype(np.int64)[clear])
        tie = ~clear                                       # there f is an integer up to rounding: ring = that integer - 1
        assert np.array_equal(got[tie], (np.rint(f) - 1).astype(np.int64)[tie])


def test_absolute_rings():
    d2 = np.arange(1, 2000, dtype=np.int64)
    for width, rings in ((1, 4), (2, 4), (3, 7), (7, 32), (32768, 2)):
        got = ref_rings(d2, None, rings, width)
        f = np.sqrt(d2) / width
        want = np.minimum(rings - 1, np.ceil(np.where(np.abs(f - np.rint(f)) < 1e-9, np.rint(f), f)) - 1).astype(np.int64)
        assert np.array_equal(got, want)
        assert [ring_absolute(v, width, rings) for v in d2[:200]] == got[:200].tolist()
    assert ring_absolute(DIST_INF, 32768, 32) == 0 and ring_absolute(DIST_INF, 1, 32) == 31 and ring_absolute(DIST_INF - 1, 32767, 3) == 1


def _square():
    labels = np.zeros((12, 13), np.int32)
    labels[2:10, 3:11] = 1
    return labels


def _tables(labels, rings, width, wedges=1, raw=None, shift=0):
    labels = np.asarray(labels)
    nid = int(labels.max()) + 1
    dist = ref_distance_sq(labels, 0)
    ins, bad = ref_inscribed(labels, dist, nid)
    assert bad == 0
    row, nrows = rows_of_all(nid)
    count, isum, bad = ref_radial(labels, dist, raw, nid, ins, row, nrows, rings, width, wedges, shift)
    assert bad == 0
    return count, isum


def test_square_by_hand():
    """an 8 x 8 square in background: its pixels lie at distances 1, 2, 3, 4 from the background in 28, 20, 12, 4 pixels"""
    labels = _square()
    assert _tables(labels, 4, 0)[0][0, :, 0].tolist() == [28, 20, 12, 4]           # every layer's edge is a ring's edge: ties
    assert _tables(labels, 2, 0)[0][0, :, 0].tolist() == [48, 16]                  # d = 2 is the tie: rim
    assert _tables(labels, 1, 0)[0][0, :, 0].tolist() == [64]
    assert _tables(labels, 4, 1)[0][0, :, 0].tolist() == [28, 20, 12, 4]
    assert _tables(labels, 4, 2)[0][0, :, 0].tolist() == [48, 16, 0, 0]            # thinner than 4 rings of 2: empty rings
    assert _tables(labels, 4, 3)[0][0, :, 0].tolist() == [60, 4, 0, 0]
    assert _tables(labels, 3, 1)[0][0, :, 0].tolist() == [28, 20, 16]              # the last ring takes what lies deeper
    # wedges: the centre is the first pixel at distance 4, (5, 6); every pixel lands in one wedge of its ring
    count, _ = _tables(labels, 4, 0, 8)
    assert count.sum() == 64 and count[0].sum(axis=1).tolist() == [28, 20, 12, 4]
    yy, xx = np.nonzero(labels)
    want = np.bincount(ref_wedge(yy - 5, xx - 6), minlength=8)
    assert count[0].sum(axis=0).tolist() == want.tolist() and (want > 0).all()


def test_wedge_table():
    r = np.arange(-40, 41)
    dy, dx = (v.reshape(-1) for v in np.meshgrid(r, r, indexing="ij"))
    got = ref_wedge(dy, dx)
    theta = np.degrees(np.arctan2(dy, dx)) % 360.0
    off = np.abs(theta / 45.0 - np.rint(theta / 45.0)) > 1e-9
    assert off.sum() > 6000 and np.array_equal(got[off], np.floor(theta[off] / 45.0).astype(np.int64))
    # a ray belongs to the wedge that starts at it
    for n in (1, 2, 37):
        rays = [(0, n), (n, n), (n, 0), (n, -n), (0, -n), (-n, -n), (-n, 0), (-n, n)]
        assert [int(ref_wedge(y, x)) for y, x in rays] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert int(ref_wedge(0, 0)) == 0
    # one step off a ray, on either side
    assert [int(ref_wedge(y, x)) for y, x in ((-1, 9), (1, 9), (8, 9), (9, 8), (9, 1), (9, -1))] == [7, 0, 0, 1, 1, 2]
    assert [int(ref_wedge(y, x)) for y, x in ((1, -9), (-1, -9), (-9, -8), (-8, -9), (-9, -1), (-9, 1))] == [3, 4, 5, 4, 5, 6]


# ---------------------------------------------------------------------------------------------------------


def _correctly_rounded(got, exact):
    """`got` is a float64 nearest to the Fraction `exact`: no neighbour is nearer"""
    got = float(got)
    assert math.isfinite(got)
    err = abs(Fraction(got) - exact)
    return all(err <= abs(Fraction(math.nextafter(got, side)) - exact) for side in (-math.inf, math.inf))


def _cv_exact(sums, counts):
    """(cv as a Decimal of 60 digits or None, largest |wedge mean| / |mean of wedge means|) from exact wedge means"""
    getcontext().prec = 60
    m = [Fraction(int(s), int(c)) for s, c in zip(sums, counts) if c]
    if not m:
        return None, None
    mu = sum(m) / len(m)
    if mu == 0:
        return None, None
    var = sum((v - mu) ** 2 for v in m) / len(m)
    cv = (Decimal(var.numerator) / Decimal(var.denominator)).sqrt() / (Decimal(mu.numerator) / Decimal(mu.denominator))
    return cv, float(max(abs(v) for v in m) / abs(mu))


def _check_columns(area, count, isum, shift, nd, k):
    cols = radial_columns(area, count, isum, shift, nd, k)
    n, rings, W = count.shape
    names = [f"radial_{q}_r{j}_c{k}" for j in range(rings) for q in ("mean", "frac", "meanfrac") + (("cv",) if W == 8 else ())]
    assert list(cols) == names and all(v.dtype == np.float64 and v.shape == (n,) for v in cols.values())
    worst = 0.0
    for i in range(n):
        S = [sum(int(v) for v in isum[i, j]) for j in range(rings)]
        N = [sum(int(v) for v in count[i, j]) for j in range(rings)]
        total, A = sum(S), int(area[i])
        for j in range(rings):
            mean, frac, meanfrac = (cols[f"radial_{q}_r{j}_c{k}"][i] for q in ("mean", "frac", "meanfrac"))
            if N[j] == 0:
                assert math.isnan(mean) and math.isnan(meanfrac)
            else:
                assert _correctly_rounded(mean, Fraction(S[j], N[j]) / Fraction(2) ** shift)
            if total == 0:
                assert math.isnan(frac) and math.isnan(meanfrac)
            else:
                assert _correctly_rounded(frac, Fraction(S[j], total))
                if N[j]:
                    assert _correctly_rounded(meanfrac, Fraction(S[j] * A, total * N[j]))
            if W == 8:
                got = cols[f"radial_cv_r{j}_c{k}"][i]
                want, spread = _cv_exact(isum[i, j], count[i, j])
                if want is None:
                    assert math.isnan(got)
                    continue
                # The bar, from the operations.  u = 2^-53, w <= 8 occupied wedges, M the largest |wedge mean|, mu their mean.
                # Every wedge mean is one rounding: off by at most u M.  Their float sum (w - 1 adds of partial sums below
                # w M) and its division are off by at most (w + 2) u M together, so every deviation d = m - mu carries at
                # most u M + (w + 2) u M + u |d| <= (w + 5) u M, |d| <= 2 M.  The root mean square moves by no more than the
                # largest change of a deviation (it is a norm), and its own w squarings, w - 1 adds, division and root add
                # at most (w + 4) u relative to a value below 2 M: (3 w + 13) u M for the standard deviation.  The quotient
                # by mu adds cv (w + 2) u M / |mu| for mu's error and u cv for its rounding.  First order in u; 1 % on top
                # covers the second-order terms while M / |mu| < 2^20, which is asserted.
                w = sum(1 for c in count[i, j] if c)
                assert spread < 2 ** 20
                bar = 1.01 * (3 * w + 13 + (w + 3) * abs(float(want))) * U * spread
                err = abs(Decimal(float(got)) - want)
                assert err <= Decimal(bar), (i, j, float(err), bar)
                worst = max(worst, float(err) / bar)
    return cols, worst


def test_radial_columns_against_fractions():
    rng = np.random.default_rng(5)
    n, rings = 40, 5
    for W, nd in ((1, 2), (1, 3), (8, 2)):
        count = rng.integers(0, 60, size=(n, rings, W)).astype(np.int64)
        count[rng.random(count.shape) < 0.25] = 0              # empty wedges and (for W == 1) empty rings
        count[:, 0, 0] += 1                                    # no empty object
        count[3, 1:] = 0                                       # an object of one ring
        count[6, 1, 0] = 2
        area = count.sum(axis=(1, 2))
        for shift, scale in ((0, 1000), (7, 10 ** 6), (-3, 50), (40, 2 ** 58 // 4096)):
            mean = rng.integers(scale // 2, scale, size=(n, rings, W))      # positive wedge means: M / |mu| stays small
            isum = np.where(count > 0, count * mean + rng.integers(0, 7, size=count.shape), 0).astype(np.int64)
            _, worst = _check_columns(area, count, isum, shift, nd, 2)
            assert worst <= 1.0
        # negative and mixed sums, an object whose sum is zero
        isum = np.where(count > 0, rng.integers(-10 ** 9, 10 ** 9, size=count.shape), 0).astype(np.int64)
        isum[5] = 0
        isum[6] = 0
        isum[6, 0, 0], isum[6, 1, 0] = 5, -5                   # sums that cancel: means, but no shares
        assert isum[6].sum() == 0
        cols = radial_columns(area, count, isum, 3, nd, 0)
        assert np.isnan(cols["radial_frac_r0_c0"][[5, 6]]).all() and np.isnan(cols["radial_meanfrac_r0_c0"][[5, 6]]).all()
        assert cols["radial_mean_r0_c0"][5] == 0.0 and cols["radial_mean_r1_c0"][6] == -5 / int(count[6, 1].sum()) / 8
        for i in range(n):
            if isum[i].sum() != 0:
                total = int(isum[i].sum())
                for j in range(rings):
                    assert _correctly_rounded(cols[f"radial_frac_r{j}_c0"][i], Fraction(int(isum[i, j].sum()), total))
                    if count[i, j].sum():
                        assert _correctly_rounded(cols[f"radial_meanfrac_r{j}_c0"][i],
                                                  Fraction(int(isum[i, j].sum()) * int(area[i]), total * int(count[i, j].sum())))
                        assert _correctly_rounded(cols[f"radial_mean_r{j}_c0"][i], Fraction(int(isum[i, j].sum()), 8 * int(count[i, j].sum())))
        # invariants: the fractions of an object add up to 1 within one rounding each and (rings - 1) adds; the areas add up
        frac = np.stack([cols[f"radial_frac_r{j}_c0"] for j in range(rings)], axis=1)
        ok = ~np.isnan(frac).any(axis=1)
        assert ok.sum() >= n - 2
        assert (np.abs(frac[ok].sum(axis=1) - 1.0) <= (2 * rings - 1) * U * np.abs(frac[ok]).sum(axis=1)).all()
        areas = radial_columns(area, count, nd=nd)
        assert list(areas) == [f"radial_area_r{j}" for j in range(rings)] and all(v.dtype == np.int64 for v in areas.values())
        assert np.array_equal(sum(areas.values()), area)


def test_radial_columns_conventions_by_hand():
    count = np.array([[[3], [1], [0]], [[2], [0], [0]]], dtype=np.int64)
    isum = np.array([[[30], [-10], [0]], [[8], [0], [0]]], dtype=np.int64)
    c = radial_columns([4, 2], count, isum, 1, 3, 0)
    assert c["radial_mean_r0_c0"].tolist() == [5.0, 2.0] and c["radial_mean_r1_c0"][0] == -5.0
    assert c["radial_frac_r0_c0"].tolist() == [1.5, 1.0] and c["radial_frac_r1_c0"].tolist() == [-0.5, 0.0]
    assert c["radial_meanfrac_r0_c0"].tolist() == [2.0, 1.0] and c["radial_meanfrac_r1_c0"][0] == -2.0
    for name in ("radial_mean_r2_c0", "radial_meanfrac_r2_c0"):
        assert np.isnan(c[name]).all()                         # an empty ring has no mean
    assert c["radial_frac_r2_c0"].tolist() == [0.0, 0.0]       # but a share: none of the object's sum
    assert np.isnan(c["radial_mean_r1_c0"][1]) and np.isnan(c["radial_meanfrac_r1_c0"][1])
    # big sums: Python integers, no int64 product overflows
    big = radial_columns([2 ** 31], np.array([[[2 ** 30], [2 ** 30]]]), np.array([[[2 ** 61], [2 ** 61 - 2 ** 31]]]), 0, 2, 1)
    assert _correctly_rounded(big["radial_meanfrac_r1_c1"][0], Fraction((2 ** 61 - 2 ** 31) * 2 ** 31, (2 ** 62 - 2 ** 31) * 2 ** 30))
    # wedges: equal wedge means give cv 0; one occupied wedge gives 0; none gives NaN; a zero mean of means gives NaN
    cnt = np.zeros((4, 1, 8), np.int64)
    s = np.zeros((4, 1, 8), np.int64)
    cnt[0, 0], s[0, 0] = [1, 2, 3, 4, 5, 6, 7, 8], [3, 6, 9, 12, 15, 18, 21, 24]
    cnt[1, 0, 5], s[1, 0, 5] = 9, 77
    cnt[2, 0, :2], s[2, 0, :2] = [2, 2], [8, -8]
    cnt[3, 0, :2], s[3, 0, :2] = [1, 1], [1, 3]                 # means 1 and 3: mu 2, std 1
    cv = radial_columns(cnt.sum(axis=(1, 2)), cnt, s, 5, 2, 0)["radial_cv_r0_c0"]
    assert cv[0] == 0.0 and cv[1] == 0.0 and np.isnan(cv[2]) and cv[3] == 0.5
    with pytest.raises(ValueError, match="count must have shape"):
        radial_columns([8], np.ones((1, 1, 8), np.int64), np.ones((1, 1, 8), np.int64), 0, 3, 0)
    with pytest.raises(AssertionError, match="add up"):
        radial_columns([5], np.ones((1, 2, 1), np.int64))
    for nd, W in ((2, 1), (2, 8), (3, 1)):
        e = radial_columns(np.zeros(0, np.int64), np.zeros((0, 3, W), np.int64), np.zeros((0, 3, W), np.int64), 0, nd, 1)
        assert len(e) == 3 * (4 if W == 8 else 3) and all(v.shape == (0,) and v.dtype == np.float64 for v in e.values())


def test_restatement_end_to_end_on_the_square():
    """rings thinner than the object leave inner rings empty in absolute mode: NaN means, zero shares, areas that add up"""
    labels = _square()
    raw = (np.arange(labels.size, dtype=np.float64).reshape(labels.shape) - 70.0) / 8.0
    count, isum = _tables(labels, 4, 2, 1, raw, 3)
    assert count[0, :, 0].tolist() == [48, 16, 0, 0]
    cols = radial_columns([64], count, isum, 3, 2, 0)
    inner = labels.astype(bool) & (ref_distance_sq(labels, 0) > 4)
    assert cols["radial_mean_r1_c0"][0] == raw[inner].mean() and cols["radial_mean_r0_c0"][0] == raw[labels.astype(bool) & ~inner].mean()
    assert np.isnan(cols["radial_mean_r2_c0"][0]) and np.isnan(cols["radial_meanfrac_r3_c0"][0]) and cols["radial_frac_r2_c0"][0] == 0.0
    assert abs(sum(cols[f"radial_frac_r{j}_c0"][0] for j in range(4)) - 1.0) <= 8 * U * sum(abs(cols[f"radial_frac_r{j}_c0"][0]) for j in range(4))
    assert sum(v[0] for v in radial_columns([64], count).values()) == 64


def test_argument_checks():
    assert _check_radial(4, None, False, 2) == (4, 0, 1) and _check_radial(32, 32768, True, 2) == (32, 32768, 8)
    assert _check_radial(np.int64(1), np.int32(1), False, 3) == (1, 1, 1) and MAX_RINGS == 32 and RADIAL_TABLE_BYTES >= 1 << 20
    for rings in (0, -1, 33, 2.5, True):
        with pytest.raises(ValueError, match="rings"):
            _check_radial(rings, None, False, 2)
    for width in (0, -3, 32769, 1.5, False):
        with pytest.raises(ValueError, match="width"):
            _check_radial(4, width, False, 2)
    with pytest.raises(ValueError, match="wedges need a 2-D map"):
        _check_radial(4, None, True, 3)


def test_symbol_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+clx_region_radial\s*\(", text), "clx_region_radial is not declared in include/clx.h"
    assert hasattr(ctypes.CDLL(_clx.LIB_PATH), "clx_region_radial"), "clx_region_radial is not exported"
    assert len(_clx.PROTOTYPES["clx_region_radial"][1]) == 20


def test_cli_accepts_radial_flags():
    from click.testing import CliRunner

    from cellulus_amd.cli import measure

    text = CliRunner().invoke(measure, ["--help"]).output
    for flag in ("--radial", "--radial-rings", "--radial-width", "--radial-wedges"):
        assert flag in text
    for args in (["--radial-rings", "0"], ["--radial-rings", "33"], ["--radial-width", "0"], ["--radial-width", "32769"]):
        result = CliRunner().invoke(measure, [__file__, "--radial"] + args)
        assert result.exit_code == 2 and "Invalid value" in result.output
