"""CPU tier of the measure stage's texture columns (no kernel is launched): cellulus_amd.measure.texture_columns against the
Fraction restatement (tests/texture_ref.py) on co-occurrence counts the restatement makes from the fixture maps, hand-worked
cases, invariants, the level formula at its bin edges, the C-ABI row and the command's options.

Error bars (u = 2^-53, γ(n) = n u / (1 - n u), the standard bound for n float64 operations in a chain or a sum):

  rational features (asm, contrast, correlation, variance, sum_average, sum_variance, difference_variance): per direction
  texture_columns holds the exact integer numerator and denominator, converts each to float64 and divides: 3 roundings.
  The column adds at most ndir of them and divides by their number: ndir more.  The restatement rounds once.  So
  |column - restatement| <= γ(ndir + 4) max_k |f_k| over the per-direction values f_k.

  idm: p₋(k) is one rounding of an exact ratio, the division by 1 + k² one more, the sum over the L levels γ(L - 1) of a sum
  of non-negative terms: γ(L + 1), then the mean as above: γ(L + ndir + 3) max_k idm_k.

  entropies (sum_entropy, entropy, difference_entropy): a term is x log2 x with x one rounding of the exact probability.
  d/dx (x log2 x) = log2 x + log2 e, so the rounding of x moves the term by at most u (|x log2 x| + x log2 e); log2 is
  taken as accurate to one ulp (2u relative), the product rounds once: u (4 |x log2 x| + x log2 e) per term, on either side
  (the restatement forms its terms the same way and sums them exactly).  The n non-zero terms are each at most log2(e)/e in
  magnitude and the x sum to 1, so one direction is off by at most (8u + γ(n) + u) n log2(e)/e + 2u log2 e =: bar_H(n),
  the γ(n) for texture_columns' sum in any order and the last u for the restatement's rounding of its exact sum.  The mean
  over the directions adds γ(ndir + 2) max_k |f_k|.

  HXY1 and HXY2 are sums of n terms w log2(px(i) px(j)): the weight w (p or px(i) px(j)) carries up to 3 roundings, the
  logarithm of the product is formed from one or two logarithms of once-rounded marginals: at most 6u of the term's
  magnitude and 3u w log2 e per side.  The terms sum to HXY1 resp. HXY2 in magnitude (all have one sign) and the weights to 1:
  bar_X(n, H) = (12u + γ(n) + u) H + 6u log2 e.
  info_correlation_1 = A / B, A = HXY - HXY1, B = HX: |Δ| <= (e_A + |f| e_B) / (B - e_B) + 2u |f| with
  e_A = bar_H + bar_X + u |A| and e_B = bar_H(L).
  info_correlation_2 = sqrt(g), g = 1 - 2^(-2 d), d = HXY2 - HXY with e_d = bar_X + bar_H + u |d|: 2^(-2d) has the slope
  2 ln 2 2^(-2d), so e_g = 2 ln 2 2^(-2 (d - e_d)) e_d + 8u (exp2 to one ulp of a value near at most 1 and the subtraction, on
  either side); sqrt: e_g / sqrt(g) + 2u where g >= 4 e_g (the mean-value bound with g - e_g >= 3g/4 > g/4), else both
  values lie in [0, sqrt(g + e_g)].
No bar is tuned to a run."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

from texture_ref import FEATURES, RATIONAL, directions, levels_of, object_features, ref_columns, ref_cooccurrence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LOG2E = math.log2(math.e)
TERM = LOG2E / math.e                   # max of |x log2 x| on [0, 1]
SETTINGS = [(8, 1), (8, 3), (32, 1), (32, 3)]


def gamma(n):
    return n * U / (1.0 - n * U)


def bar_h(n):
    return (9.0 * U + gamma(n)) * n * TERM + 2.0 * U * LOG2E


def bar_x(n, h):
    return (13.0 * U + gamma(n)) * abs(h) + 6.0 * U * LOG2E


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: (g[f"{name}/labels"], g[f"{name}/raw"]) for name in ("2d", "2d_edge", "3d")}


G = _fixture()
_COUNTS = {}


def fixture_counts(name, levels, distance):
    """(ids, counts) of a fixture map over the range of its object pixels, computed once and left unchanged"""
    key = (name, levels, distance)
    if key not in _COUNTS:
        labels, raw = G[name]
        nid = int(labels.max()) + 1
        ids = np.unique(labels[labels > 0])
        lo, hi = float(raw[labels > 0].min()), float(raw[labels > 0].max())
        counts = ref_cooccurrence(labels, raw, nid, ids, lo, hi, levels, distance)["counts"]
        counts.setflags(write=False)
        _COUNTS[key] = (ids, counts)
    return _COUNTS[key]


def column_bars(C):
    """the bars of the module docstring for one object's (ndir, L, L) counts -> {feature: bar}, from the restatement's exact
    per-direction values"""
    ndir, L = C.shape[0], C.shape[1]
    _, _, per_dir = object_features(C)
    live = [np.asarray(M) for M in C if int(np.sum(M)) > 0]
    bars = {}
    if not per_dir:
        return {name: 0.0 for name in FEATURES}
    top = {name: max(abs(float(d[name])) for d in per_dir) for name in FEATURES}
    for name in RATIONAL:
        bars[name] = gamma(ndir + 4) * top[name]
    bars["idm"] = gamma(L + ndir + 3) * top["idm"]
    worst = {name: 0.0 for name in ("sum_entropy", "entropy", "difference_entropy", "info_correlation_1", "info_correlation_2")}
    for d, M in zip(per_dir, live):
        S = M.astype(np.int64) + M.T.astype(np.int64)
        n_p = int(np.count_nonzero(S))
        n_x = int(np.count_nonzero(S.sum(axis=1)))
        ii, jj = np.nonzero(S)
        worst["entropy"] = max(worst["entropy"], bar_h(n_p))
        worst["sum_entropy"] = max(worst["sum_entropy"], bar_h(len(set((ii + jj).tolist()))))
        worst["difference_entropy"] = max(worst["difference_entropy"], bar_h(len(set(abs(ii - jj).tolist()))))
        hx, hxy, hxy1, hxy2 = d["_hx"], d["_hxy"], d["_hxy1"], d["_hxy2"]
        if hx:
            f = d["info_correlation_1"]
            e_a = bar_h(n_p) + bar_x(n_p, hxy1) + U * abs(hxy - hxy1)
            e_b = bar_h(n_x)
            assert hx > 2.0 * e_b
            worst["info_correlation_1"] = max(worst["info_correlation_1"], (e_a + abs(f) * e_b) / (hx - e_b) + 2.0 * U * abs(f))
        dd = hxy2 - hxy
        e_d = bar_x(n_x * n_x, hxy2) + bar_h(n_p) + U * abs(dd)
        e_g = 2.0 * math.log(2.0) * 2.0 ** (-2.0 * (dd - e_d)) * e_d + 8.0 * U
        g = max(0.0, 1.0 - 2.0 ** (-2.0 * dd))
        e_f = e_g / math.sqrt(g) + 2.0 * U if g >= 4.0 * e_g else math.sqrt(g + e_g)
        worst["info_correlation_2"] = max(worst["info_correlation_2"], e_f)
    for name, b in worst.items():
        bars[name] = b + gamma(ndir + 2) * top[name]
    return bars


@pytest.mark.parametrize("levels,distance", SETTINGS)
@pytest.mark.parametrize("name", sorted(G))
def test_columns_against_fraction_restatement(name, levels, distance):
    from cellulus_amd.measure import TEXTURE_FEATURES, texture_columns

    assert TEXTURE_FEATURES == FEATURES
    nd = G[name][0].ndim
    ids, counts = fixture_counts(name, levels, distance)
    got = texture_columns(counts, nd)
    want = ref_columns(counts)
    assert list(got) == ["pairs"] + list(FEATURES)
    assert got["pairs"].dtype == np.int64 and np.array_equal(got["pairs"], want["pairs"])
    for r in range(len(ids)):
        bars = column_bars(counts[r])
        for f in FEATURES:
            g, w = got[f][r], want[f][r]
            assert got[f].dtype == np.float64
            if math.isnan(w):
                assert math.isnan(g), (name, ids[r], f)
            else:
                assert abs(g - w) <= bars[f], (name, int(ids[r]), f, g, w, bars[f])
                if f in RATIONAL:
                    assert bars[f] <= 1e-12 * max(1.0, abs(w))      # the derived bar of a rational feature is a few ulps


def test_fixture_exercises_the_nan_and_missing_direction_rules():
    """among the fixture's maps and settings there are objects with an empty direction and objects with no pair at all"""
    some_empty = none_at_all = 0
    for name in G:
        for levels, distance in SETTINGS:
            _, counts = fixture_counts(name, levels, distance)
            n_dir = (counts.sum(axis=(2, 3)) > 0).sum(axis=1)
            some_empty += int(((n_dir > 0) & (n_dir < counts.shape[1])).sum())
            none_at_all += int((n_dir == 0).sum())
    assert some_empty > 0 and none_at_all > 0


def _cols(counts, nd=2):
    from cellulus_amd.measure import texture_columns

    return texture_columns(np.asarray(counts), nd)


def _counts_of(labels, raw, levels, distance=1, lo=None, hi=None):
    labels = np.asarray(labels)
    raw = np.asarray(raw)
    nid = int(labels.max()) + 1
    ids = np.unique(labels[labels > 0])
    lo = float(raw[labels > 0].min()) if lo is None else lo
    hi = float(raw[labels > 0].max()) if hi is None else hi
    return ids, ref_cooccurrence(labels, raw, nid, ids, lo, hi, levels, distance)["counts"]


def test_constant_object():
    labels = np.zeros((6, 7), np.int32)
    labels[1:5, 2:6] = 1
    _, counts = _counts_of(labels, np.full((6, 7), 3.5), 8)          # hi == lo: every pixel at level 0
    assert counts[0, :, 0, 0].tolist() == [12, 9, 12, 9] and counts.sum() == 42
    c = _cols(counts)
    assert c["pairs"].tolist() == [42]
    # p = 1 in one cell: every sum below is one exact term
    want = dict(asm=1.0, contrast=0.0, correlation=1.0, variance=0.0, idm=1.0, sum_average=0.0, sum_variance=0.0, sum_entropy=0.0,
                entropy=0.0, difference_variance=0.0, difference_entropy=0.0, info_correlation_1=0.0, info_correlation_2=0.0)
    for f in FEATURES:
        assert c[f][0] == want[f], f


def test_two_level_checkerboard():
    yy, xx = np.indices((6, 6))
    raw = ((yy + xx) % 2).astype(np.float64)
    labels = np.ones((6, 6), np.int32)
    _, counts = _counts_of(labels, raw, 2)
    # axial directions (0,1), (1,0): 30 pairs each, all between unequal levels, 15 each way; diagonals: 25 pairs between
    # equal levels, 13 at level 0 ((y + x) even) and 12 at level 1 along (1,1); 12 and 13 along (1,-1)
    assert counts[0, 0].tolist() == [[0, 15], [15, 0]] and counts[0, 2].tolist() == [[0, 15], [15, 0]]
    assert counts[0, 3].tolist() == [[13, 0], [0, 12]] and counts[0, 1].tolist() == [[12, 0], [0, 13]]
    c = _cols(counts)
    assert c["pairs"].tolist() == [110]
    # axial: p(0,1) = p(1,0) = 1/2: asm 1/2, contrast 1, μ = 1/2, σ² = 1/4, correlation (0 - 1/4) / (1/4) = -1, entropy 1 bit
    # diagonal (1,1): p(0,0) = 13/25, p(1,1) = 12/25: asm (169 + 144) / 625, contrast 0, μ = 12/25, σ² = 156/625,
    # correlation (12/25 - 144/625) / (156/625) = 1
    assert c["asm"][0] == pytest.approx((0.5 + 0.5 + 2 * 313 / 625) / 4, rel=4 * U)
    assert c["contrast"][0] == 0.5
    assert c["correlation"][0] == 0.0
    assert c["variance"][0] == pytest.approx((0.25 + 0.25 + 2 * 156 / 625) / 4, rel=4 * U)
    # sum_average is 2 μ: 1 and 1 along the axes, 24/25 along (1,1) and 26/25 along (1,-1), where the levels swap
    assert c["sum_average"][0] == pytest.approx(1.0, rel=4 * U)
    h = -(13 / 25 * math.log2(13 / 25) + 12 / 25 * math.log2(12 / 25))
    assert c["entropy"][0] == pytest.approx((1 + 1 + 2 * h) / 4, rel=1e-15)
    assert c["difference_entropy"][0] == 0.0 and c["difference_variance"][0] == 0.0
    # axial: px = (1/2, 1/2), HX = 1, HXY = 1, HXY1 = 2: (1 - 2) / 1 = -1.  diagonal: HXY = HX = h, HXY1 = 2h: -1
    assert c["info_correlation_1"][0] == pytest.approx(-1.0, rel=1e-15)


def test_two_pixel_object():
    labels = np.array([[0, 0, 0], [0, 1, 1], [0, 0, 0]], np.int32)
    raw = np.array([[9, 9, 9], [9, 0, 7], [9, 9, 9]], np.float64)
    _, counts = _counts_of(labels, raw, 8)
    want = np.zeros((1, 4, 8, 8), np.int32)
    want[0, 0, 0, 7] = 1                                              # the one pair, along (0, 1), from level 0 to level 7
    assert np.array_equal(counts, want)
    c = _cols(counts)
    # S has 1 at (0,7) and (7,0), T = 2: p = 1/2 twice.  Only one direction has a pair: the mean is over it alone
    assert c["pairs"].tolist() == [1]
    assert c["asm"][0] == 0.5 and c["contrast"][0] == 49.0 and c["variance"][0] == 12.25 and c["correlation"][0] == -1.0
    assert c["idm"][0] == 1.0 / 50.0 and c["sum_average"][0] == 7.0 and c["sum_variance"][0] == 0.0
    assert c["entropy"][0] == 1.0 and c["sum_entropy"][0] == 0.0 and c["difference_entropy"][0] == 0.0
    assert c["difference_variance"][0] == 0.0 and c["info_correlation_1"][0] == -1.0
    assert c["info_correlation_2"][0] == math.sqrt(1.0 - 2.0 ** -2.0)  # HXY2 = 2, HXY = 1
    # a one-pixel object: no pair in any direction, NaN everywhere
    one = _cols(np.zeros((1, 4, 8, 8), np.int64))
    assert one["pairs"].tolist() == [0] and all(math.isnan(one[f][0]) for f in FEATURES)
    assert all(len(v) == 0 for v in _cols(np.zeros((0, 4, 8, 8), np.int32)).values())
    assert _cols(np.zeros((0, 13, 8, 8), np.int32), 3)["pairs"].dtype == np.int64


def test_python_int_route_agrees_with_int64(monkeypatch):
    from cellulus_amd import measure, measure_columns

    _, counts = fixture_counts("2d", 8, 1)
    a = measure.texture_columns(counts, 2)
    monkeypatch.setattr(measure_columns, "_TEXTURE_INT64_MAX_T", 0)          # every numerator as Python ints
    b = measure.texture_columns(counts, 2)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    # counts whose numerators do not fit int64: 2N = 2^31 in one cell pair
    big = np.zeros((1, 4, 2, 2), np.int64)
    big[0, 0, 0, 1] = 2 ** 30
    monkeypatch.undo()
    c = measure.texture_columns(big, 2)
    assert c["asm"][0] == 0.5 and c["contrast"][0] == 1.0 and c["correlation"][0] == -1.0 and c["pairs"][0] == 2 ** 30


def test_invariants():
    labels, raw = G["2d"]
    ids, counts = fixture_counts("2d", 8, 1)
    S = counts.astype(np.int64) + counts.transpose(0, 1, 3, 2)
    assert np.array_equal(S, S.transpose(0, 1, 3, 2))
    # pairs: the same-object pixel pairs over the four directions, counted without the levels
    same = 0
    per_object = np.zeros(int(labels.max()) + 1, np.int64)
    for dy, dx in directions(2):
        a = labels[:labels.shape[0] - dy, max(0, -dx):labels.shape[1] - max(0, dx)]
        b = labels[dy:, max(0, dx):labels.shape[1] - max(0, -dx)]
        hit = (a == b) & (a > 0)
        same += int(hit.sum())
        per_object += np.bincount(a[hit], minlength=len(per_object))
    cols = _cols(counts)
    assert int(cols["pairs"].sum()) == same and np.array_equal(cols["pairs"], per_object[ids])
    lo, hi = float(raw[labels > 0].min()), float(raw[labels > 0].max())
    # a permutation of the object ids permutes the rows
    perm = np.arange(int(labels.max()) + 1)
    perm[1:] = np.random.default_rng(5).permutation(perm[1:])
    ids2, counts2 = _counts_of(perm[labels], raw, 8, 1, lo, hi)
    cols2 = _cols(counts2)
    order = np.searchsorted(ids2, perm[ids])
    for k in cols:
        assert np.array_equal(cols[k], cols2[k][order], equal_nan=True), k
    # mirroring the map swaps directions ((1,-1) with (1,1)) and transposes matrices, but S and the set of directions with
    # a pair are what they were: the rational numerators are the same integers, so those columns are EQUAL; the others are
    # sums of the same terms in another order
    _, counts3 = _counts_of(labels[:, ::-1], raw[:, ::-1], 8, 1, lo, hi)
    assert np.array_equal(counts3[:, 0], counts[:, 0].transpose(0, 2, 1)) and np.array_equal(counts3[:, 1], counts[:, 3])
    cols3 = _cols(counts3)
    for k in cols:
        if k in RATIONAL or k == "pairs":
            assert np.allclose(cols[k], cols3[k], rtol=gamma(4), atol=0, equal_nan=True), k
        else:
            assert np.allclose(cols[k], cols3[k], rtol=0, atol=2 * max(column_bars(c)[k] for c in counts), equal_nan=True), k


def test_level_formula_at_bin_edges():
    lo, hi = -1.5, 6.5                                               # a range of 8: with 8 levels the edges are integers + 0.5
    v = np.array([lo, lo + 1.0, np.nextafter(lo + 1.0, -np.inf), hi, np.nextafter(hi, -np.inf), hi + 100.0, lo - 100.0, 2.5])
    lev, finite = levels_of(v, lo, hi, 8)
    assert lev.tolist() == [0, 1, 0, 7, 7, 7, 0, 4] and finite.all()              # v == hi: floor gives 8, clamped to 7
    assert levels_of(v, 3.0, 3.0, 8)[0].tolist() == [0] * 8                       # hi == lo
    lev, finite = levels_of(np.array([np.nan, np.inf, -np.inf, 1.0]), 0.0, 2.0, 4)
    assert finite.tolist() == [False, False, False, True] and lev[3] == 2
    # every edge of 32 levels over [0, 1]: v = k / 32 is exact and lands in level k
    assert levels_of(np.arange(33) / 32.0, 0.0, 1.0, 32)[0].tolist() == list(range(32)) + [31]


def test_directions():
    from cellulus_amd.measure import texture_directions

    assert directions(2) == [(0, 1), (1, -1), (1, 0), (1, 1)] == texture_directions(2)
    assert directions(3) == texture_directions(3) and len(directions(3)) == 13 and directions(3)[0] == (0, 0, 1)


def test_symbol_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    assert _build.PER_FILE_FLAGS["region_texture.hip"] == ["-ffp-contract=off"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, restype in (("clx_region_cooccurrence", "int"), ("clx_region_cooccurrence_workspace", "size_t")):
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (restype, name), text)
        assert m, f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == len(m.group(1).split(","))
    assert len(_clx.PROTOTYPES["clx_region_cooccurrence"][1]) == 21
    size = _clx.load().clx_region_cooccurrence_workspace
    assert size(0, 1) == 0 and size(1 << 31, 1) == 0 and size(100, -1) == 0
    assert size(100, 0) == 104 + 8 + 8 and size(100, 10) == 104 + 88 + 8


def test_cli_and_arguments():
    from click.testing import CliRunner

    from cellulus_amd import cli
    from cellulus_amd.measure import _check_texture

    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and "--texture " in res.output and "--texture-levels" in res.output and "--texture-distance" in res.output
    for bad in ((1, 1, None), (33, 1, None), (8, 0, None), (8, 65, None), (8, 1, (1.0, 0.0)), (8, 1, (0.0, math.inf))):
        with pytest.raises(ValueError, match="^region_table: texture"):
            _check_texture(*bad)
    assert _check_texture(32, 64, (0, 0)) == (32, 64, (0.0, 0.0))
