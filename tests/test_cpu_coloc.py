"""The host side of the intensity standard deviation and the colocalization columns, without a device: products_columns
against the restatement in Fractions of tests/coloc_ref.py and by hand, against NumPy's float64 formulas within a bar derived
from their rounding, the threshold rule at its ties, the argument checks, the declarations."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

from cellulus_amd.measure import (coloc_thresholds, channel_products, product_table, products_columns, quantised, region_table)
from coloc_ref import (SQUARES, SUMS, ref_columns, ref_products, ref_thresholds, round_sqrt, same_floats, table_of, words_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _rows(a, b, thr_a=None, thr_b=None, labels=None):
    """rows of the restatement for int64 'channels' a and b (one object unless labels are given) -> rows from id 1 up"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    labels = np.ones(a.shape, np.int64) if labels is None else np.asarray(labels)
    nid = int(labels.max()) + 1
    rows, bad = ref_products(labels, a, b, nid, 0, 0, thr_a, thr_b)
    assert bad == 0
    return rows[1:]


def _assert_columns(rows, shift_a, shift_b, j, k):
    got = products_columns(table_of(rows), shift_a, shift_b, j, k, std=True, colocalization=True)
    want = ref_columns(rows, shift_a, shift_b, j, k)
    assert list(got) == list(want)
    for name in want:
        assert got[name].dtype == np.float64 and same_floats(got[name], want[name]), (name, got[name], want[name])
    return got


@pytest.mark.parametrize("seed", range(4))
def test_products_columns_equal_the_fraction_restatement(seed):
    rng = np.random.default_rng(seed)
    n, nid = 700, 13
    labels = rng.integers(0, nid, size=n)
    mag = (2 ** 20, 2 ** 40, 2 ** 49, 2 ** 55)[seed]                 # squares up to 2^110: sums far above 2^64; Σa stays in int64
    a = rng.integers(-mag, mag, size=n)
    b = np.where(rng.random(n) < 0.7, -a // 3 + rng.integers(-mag // 8, mag // 8, size=n), rng.integers(-mag, mag, size=n))
    thr_a = rng.integers(-mag // 2, mag // 2, size=nid)
    thr_b = rng.integers(-mag // 2, mag // 2, size=nid)
    rows = _rows(a, b, thr_a, thr_b, labels)
    if seed:
        assert max(abs(r[8]) for r in rows) > 2 ** 64
    assert any(r[10] < 0 for r in rows) and any(r[13] < 0 for r in rows)       # negative cross sums
    for shift_a, shift_b in ((0, 0), (5, -3), (-1022, 1023), (40, 40)):
        _assert_columns(rows, shift_a, shift_b, 0, 1)
    _assert_columns(rows, 3, 9, 2, 5)
    # the words of the device layout decode to the same table
    t = product_table(words_of(rows))
    for w, name in enumerate(SUMS + SQUARES):
        assert [int(v) for v in t[name]] == [r[w] for r in rows], name
    assert all(t[name].dtype == np.int64 for name in SUMS) and all(t[name].dtype == object for name in SQUARES)


def test_conventions_by_hand():
    a = np.array([3, -7, 12, 5, 0, 9, 9, -2])
    c = _assert_columns(_rows(a, 2 * a + 3), 0, 0, 0, 1)
    assert c["coloc_pearson_c0_c1"][0] == 1.0 and c["coloc_slope_c0_c1"][0] == 2.0
    assert c["intensity_std_c1"][0] == 2.0 * c["intensity_std_c0"][0]
    c = _assert_columns(_rows(a, -a), 0, 0, 0, 1)
    assert c["coloc_pearson_c0_c1"][0] == -1.0 and c["coloc_slope_c0_c1"][0] == -1.0 and c["coloc_overlap_c0_c1"][0] == -1.0
    # the shifts: b = 2 a + 3 read as a / 2^4 and b / 2^6 has a quarter of the slope, and the std scale with their channel
    c = _assert_columns(_rows(a, 2 * a + 3), 4, 6, 0, 1)
    assert c["coloc_slope_c0_c1"][0] == 0.5 and c["coloc_pearson_c0_c1"][0] == 1.0
    # a constant channel: no correlation, no slope on it, std exactly 0
    const = _assert_columns(_rows(a, np.full(len(a), 7)), 0, 0, 0, 1)
    assert math.isnan(const["coloc_pearson_c0_c1"][0]) and const["intensity_std_c1"][0] == 0.0 and const["coloc_slope_c0_c1"][0] == 0.0
    flipped = _assert_columns(_rows(np.full(len(a), 7), a), 0, 0, 0, 1)
    assert math.isnan(flipped["coloc_pearson_c0_c1"][0]) and math.isnan(flipped["coloc_slope_c0_c1"][0])
    # A 2 x 2 object:  a = 1 2 / 3 4,  b = 2 1 / 4 3,  thresholds 2 and 2.
    #   n = 4, A = B = 10, Σaa = Σbb = 30, Σab = 2 + 2 + 12 + 12 = 28;  Va = Vb = 4 * 30 - 100 = 20,  C = 4 * 28 - 100 = 12
    #   std = sqrt(20 / 16),  pearson = 12 / 20,  slope = 12 / 20
    #   above a: the pixels 2 3 4 (Σa = 9);  above b: those with b = 2 4 3 (Σb = 9);  both: the bottom row, (3, 4) and (4, 3)
    #   n_both = 2, Σa_T = Σb_T = 7, Σaa_T = Σbb_T = 25, Σab_T = 24:  overlap = k1 = k2 = 24 / 25,  manders1 = manders2 = 7 / 9
    rows = _rows([1, 2, 3, 4], [2, 1, 4, 3], [0, 2], [0, 2])
    assert rows == [[4, 10, 10, 2, 9, 9, 7, 7, 30, 30, 28, 25, 25, 24]]
    c = _assert_columns(rows, 0, 0, 0, 1)
    assert c["intensity_std_c0"][0] == c["intensity_std_c1"][0] == math.sqrt(1.25)
    assert c["coloc_pearson_c0_c1"][0] == 0.6 and c["coloc_slope_c0_c1"][0] == 0.6
    assert c["coloc_overlap_c0_c1"][0] == c["coloc_k1_c0_c1"][0] == c["coloc_k2_c0_c1"][0] == 0.96
    assert c["coloc_manders1_c0_c1"][0] == c["coloc_manders2_c0_c1"][0] == 7 / 9
    # no pixel above both: the conditioned columns have no denominator
    none = _assert_columns(_rows([1, 2, 3, 4], [2, 1, 4, 3], [0, 5], [0, 5]), 0, 0, 0, 1)
    for q in ("overlap", "k1", "k2", "manders1", "manders2"):
        assert math.isnan(none[f"coloc_{q}_c0_c1"][0])
    # which columns are formed, and in which order
    t = table_of(rows)
    assert list(products_columns(t, j=1, k=2)) == [f"coloc_{q}_c1_c2" for q in ("pearson", "slope", "overlap", "k1", "k2", "manders1", "manders2")]
    assert list(products_columns(t, j=3, k=3, std=True, colocalization=False)) == ["intensity_std_c3"]
    empty = products_columns(table_of([]), std=True)
    assert len(empty) == 9 and all(v.shape == (0,) and v.dtype == np.float64 for v in empty.values())


def test_round_sqrt_of_the_restatement():
    assert round_sqrt(4) == 2.0 and round_sqrt(2) == math.sqrt(2.0) and round_sqrt(0) == 0.0
    from fractions import Fraction
    assert round_sqrt(Fraction(1, 10 ** 40)) == 1e-20 and round_sqrt(Fraction(2 ** 200 + 1)) == 2.0 ** 100


def test_against_numpy_float64():
    """uint8-valued objects against np.std and np.corrcoef in float64.  The bars, from float64's own rounding of those formulas
    (u = EPS / 2 a rounding, n pixels, d = x - mean):
    np.std: the mean carries at most n u mean|x| (a sum of n terms, one division); subtracting it from every pixel shifts all d
    by that COMMON error, which the sum of squares sees only to second order (Σ d = 0), plus one rounding per d; the squares,
    their sum of n terms, the division and the root add at most n + 4 roundings to the variance, half of that to its root.
    So |np.std - σ| <= n EPS (1 + κ) σ with κ = mean|x| / σ the condition of the subtraction, a generous cover of
    (n + 4) u / 2 + (n u κ)^2.  The column itself is the correctly rounded σ, u more, inside the same cover.
    np.corrcoef: the covariance Σ da db has the same roundings on every term, at most (n + 4) u Σ|da db| in all, and
    Σ|da db| <= sqrt(Σ da² Σ db²) (Cauchy-Schwarz), so its share of r errs by at most (n + 4) u; the two variances under the
    root add (n + 4) u |r| together.  So |np.corrcoef - r| <= n EPS (1 + |r|) (1 + κa + κb) covers it, the last factor for the
    two subtractions."""
    rng = np.random.default_rng(5)
    checked = 0
    for trial in range(40):
        n = int(rng.integers(16, 400))
        a = rng.integers(0, 256, size=n)
        b = np.clip(a * rng.uniform(-1, 1) + rng.integers(0, 256, size=n) * rng.uniform(0, 1), 0, 255).astype(np.int64)
        if trial % 5 == 0:
            a = a // 64 + 250                                     # a large mean over a small spread: κ is large
        if a.min() == a.max() or b.min() == b.max():
            continue
        cols = products_columns(table_of(_rows(a, b)), std=True)
        fa, fb = a.astype(np.float64), b.astype(np.float64)
        for col, x in ((cols["intensity_std_c0"][0], fa), (cols["intensity_std_c1"][0], fb)):
            want = np.std(x)
            kappa = np.abs(x).mean() / want
            assert abs(col - want) <= n * EPS * (1.0 + kappa) * want, (trial, col, want)
        r = float(np.corrcoef(fa, fb)[0, 1])
        ka, kb = np.abs(fa).mean() / np.std(fa), np.abs(fb).mean() / np.std(fb)
        assert abs(cols["coloc_pearson_c0_c1"][0] - r) <= n * EPS * (1.0 + abs(r)) * (1.0 + ka + kb), (trial, cols["coloc_pearson_c0_c1"][0], r)
        checked += 1
    assert checked >= 30


def test_threshold_rule_at_its_ties():
    # f * qmax an integer: the threshold IS that integer and a pixel at it is above (q >= thr)
    assert coloc_thresholds([200, 8, -8], 0.25).tolist() == [50, 2, -2]
    assert coloc_thresholds([100], 0.15).tolist() == [15]          # the float 0.15 lies below 3/20: ceil(14.99999999999999944) = 15
    assert coloc_thresholds([100], 0.15000000000000002).tolist() == [16]       # the next float lies above 3/20
    assert coloc_thresholds([3, 2 ** 62, -(2 ** 62), 0], 0.0).tolist() == [0, 0, 0, 0]
    assert coloc_thresholds([3, 2 ** 62, -(2 ** 62), 0], 1.0).tolist() == [3, 2 ** 62, -(2 ** 62), 0]
    assert coloc_thresholds([7], 0.5).tolist() == [4] and coloc_thresholds([-7], 0.5).tolist() == [-3]
    rng = np.random.default_rng(2)
    q = [int(v) for v in rng.integers(-2 ** 62, 2 ** 62, size=200)]
    for f in (0.15, 0.5, 1 / 3, 5e-324, 1.0 - 2.0 ** -53):
        assert np.array_equal(coloc_thresholds(q, f), ref_thresholds(q, f))
    assert coloc_thresholds([], 0.3).shape == (0,) and coloc_thresholds([], 0.3).dtype == np.int64
    for f in (-0.1, 1.5, math.nan, math.inf):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            coloc_thresholds([1], f)
    # the classes that follow: with thr = f * qmax an integer, the pixel at the threshold counts
    rows = _rows([50, 49, 200, 51], [8, 8, 8, 8], [0, 50], [0, 8])
    assert rows[0][3] == 3 and rows[0][4] == 301
    # the quantised maximum the thresholds are taken of
    assert quantised(np.array([1.5, -2.5, 0.25], np.float32), 1) == [3, -5, 0] and quantised(np.array([7, -9], np.int32), 12) == [7, -9]


def test_argument_checks_before_the_device():
    """every one of these is raised before a device is looked for: on a machine without one the device error would come first"""
    labels = np.ones((4, 5), np.int32)
    one = np.ones((4, 5), np.float32)
    two = np.ones((2, 4, 5), np.float32)
    with pytest.raises(ValueError, match="need raw"):
        region_table(labels, std=True)
    with pytest.raises(ValueError, match="need raw"):
        region_table(labels, colocalization=True)
    for raw in (one, one[None]):
        with pytest.raises(ValueError, match="at least 2 raw channels"):
            region_table(labels, raw, colocalization=True)
    for f in (-0.01, 1.01, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="coloc_threshold"):
            region_table(labels, two, colocalization=True, coloc_threshold=f)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            channel_products(labels, two, threshold=f)
    with pytest.raises(ValueError, match="raw is needed"):
        channel_products(labels, None)
    for j, k in ((0, 2), (-1, 1), (2, 0)):
        with pytest.raises(ValueError, match="channels"):
            channel_products(labels, two, j, k)
    with pytest.raises(ValueError, match="channels"):
        channel_products(labels, one)                             # one channel has no channel 1
    with pytest.raises(ValueError, match="raw has shape"):
        channel_products(labels, np.ones((2, 4, 6), np.float32))


def test_symbol_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+clx_region_products\s*\(", text), "clx_region_products is not declared in include/clx.h"
    assert hasattr(ctypes.CDLL(_clx.LIB_PATH), "clx_region_products"), "clx_region_products is not exported"
    assert len(_clx.PROTOTYPES["clx_region_products"][1]) == 13
    assert _clx.load().clx_abi_version() == 13


def test_entry_point_refuses_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def products(raw_type=0, npix=64, nid=4, **ptrs):
        p = dict(labels=some, raw_a=some, raw_b=some, thr_a=some, thr_b=some, out=some, bad=some)
        p.update(ptrs)
        return lib.clx_region_products(p["labels"], p["raw_a"], p["raw_b"], raw_type, npix, nid, 0, 0, p["thr_a"], p["thr_b"], p["out"],
                                       p["bad"], null)

    refused = [(lambda k=k: products(**{k: null}), "null pointer") for k in ("labels", "raw_a", "raw_b", "out", "bad", "thr_a", "thr_b")] + [
        (lambda: products(raw_type=3), "raw_type"), (lambda: products(raw_type=-1), "raw_type"),
        (lambda: products(nid=0), "nid"), (lambda: products(nid=-2), "nid"), (lambda: products(nid=2 ** 24 + 1), "nid"),
        (lambda: products(npix=0), "npix"), (lambda: products(npix=-5), "npix"), (lambda: products(npix=2 ** 32), "npix"),
        (lambda: products(thr_a=null, thr_b=null, raw_a=null), "null pointer"),
    ]
    for i, (call, word) in enumerate(refused):
        assert call() == -1, f"case {i} was not refused"
        message = lib.clx_last_error().decode()
        assert message.startswith("clx_region_products") and word in message, f"case {i}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="thr_a and thr_b"):
        _clx.call("clx_region_products", some, some, some, 0, 64, 4, 0, 0, some, null, some, some, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import measure

    text = CliRunner().invoke(measure, ["--help"]).output
    for flag in ("--std", "--colocalization", "--coloc-threshold"):
        assert flag in text
    for args in (["--coloc-threshold", "-0.1"], ["--coloc-threshold", "1.5"], ["--coloc-threshold", "x"]):
        result = CliRunner().invoke(measure, [__file__, "--colocalization"] + args)
        assert result.exit_code == 2 and "Invalid value" in result.output
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(measure, [__file__, "--std", "--colocalization", "--coloc-threshold", "0.25"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output
