"""CPU tier of the measure stage's order statistics (no kernel is launched): the rank and interpolation arithmetic behind
the quantile columns against Fractions written out here and, where NumPy's own index arithmetic is exact, against
np.quantile / np.median with ==; the restatement the GPU tests compare with (tests/order_ref.py); argument validation; the
C-ABI symbols and the command's flags."""

import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from order_ref import F32, F64, I32, decode_key, exact_quantile, order_key, ref_columns, ref_order_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREAS = [1, 2, 3, 4, 5, 64, 65, 1000]
QS = [0, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.999, 1]


def test_quantile_ranks_against_fractions():
    from cellulus_amd.measure import quantile_ranks

    for q in QS:
        lo, hi, t = quantile_ranks(AREAS, q)
        assert lo.dtype == np.int64 and hi.dtype == np.int64 and len(t) == len(AREAS)
        for n, a, b, w in zip(AREAS, lo, hi, t):
            h = Fraction(float(q)) * (n - 1)                 # the float64 q, exactly; no rounding anywhere
            assert isinstance(w, Fraction) and a + w == h and 0 <= w < 1, (n, q)
            assert 0 <= a <= b <= n - 1 and b - a == (0 if w == 0 else 1), (n, q)
    # written out: 0.1 as a float64 is 3602879701896397 / 2^55, a little above 1/10
    tenth = Fraction(3602879701896397, 2 ** 55)
    lo, hi, t = quantile_ranks([1, 2, 11, 1000], 0.1)
    assert lo.tolist() == [0, 0, 1, 99] and hi.tolist() == [0, 1, 2, 100]      # 10 * 0.1 is just above 1: ranks 1 and 2
    assert t == [0, tenth, 10 * tenth - 1, 999 * tenth - 99]
    lo, hi, t = quantile_ranks([1, 2, 3, 4, 5, 64, 65, 1000], 0.5)
    assert lo.tolist() == [0, 0, 1, 1, 2, 31, 32, 499] and hi.tolist() == [0, 1, 1, 2, 2, 32, 32, 500]
    assert t == [0, Fraction(1, 2), 0, Fraction(1, 2), 0, Fraction(1, 2), 0, Fraction(1, 2)]
    lo, hi, t = quantile_ranks([4, 5, 65], 0.75)
    assert lo.tolist() == [2, 3, 48] and hi.tolist() == [3, 3, 48] and t == [Fraction(1, 4), 0, 0]
    third = Fraction(float(1 / 3))
    lo, hi, t = quantile_ranks([4, 1000], 1 / 3)
    assert lo.tolist() == [0, 332] and hi.tolist() == [1, 333] and t == [3 * third, 999 * third - 332]    # 1/3 rounds down
    for q, want in ((0, [0] * 8), (1, [n - 1 for n in AREAS])):
        lo, hi, t = quantile_ranks(AREAS, q)
        assert lo.tolist() == want and hi.tolist() == want and t == [0] * 8
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            quantile_ranks([3], q)
    with pytest.raises(ValueError):
        quantile_ranks([3, 0], 0.5)


def test_quantile_columns_against_fractions():
    from cellulus_amd.measure import quantile_columns, quantile_ranks

    # by hand: 1 + (4 - 1) / 3 = 2; 2^53 + (2^53 + 2 - 2^53) / 2 = 2^53 + 1 -> rounds to even, 2^53; 0.1f + 0 = 0.1f
    got = quantile_columns(np.array([1, 2 ** 53, -7], np.int64), np.array([4, 2 ** 53 + 2, -7], np.int64),
                           [Fraction(1, 3), Fraction(1, 2), 0])
    assert got.dtype == np.float64 and got.tolist() == [2.0, float(2 ** 53), -7.0]
    f = np.float32(0.1)
    got = quantile_columns(np.array([f, f], np.float32), np.array([f, np.float32(0.3)], np.float32), [Fraction(1, 2), Fraction(1, 4)])
    assert got.tolist() == [float(f), float(Fraction(float(f)) + (Fraction(float(np.float32(0.3))) - Fraction(float(f))) / 4)]
    # one rounding: a + (b - a) t in float64 arithmetic gives another number here
    a, b, t = 1.0, 1.0 + 2.0 ** -52, Fraction(1, 3)
    assert quantile_columns([a], [b], [t])[0] == float(Fraction(a) + (Fraction(b) - Fraction(a)) * t) == 1.0
    assert quantile_columns(np.zeros(0), np.zeros(0), []).shape == (0,)
    # the whole chain on sorted data, against the restatement and the Fractions written out
    rng = np.random.default_rng(1)
    for n in AREAS:
        for values in (rng.integers(-50, 50, n).astype(np.int32), rng.normal(size=n).astype(np.float32), rng.normal(size=n) * 1e-3):
            s = np.sort(values)
            for q in QS:
                lo, hi, t = quantile_ranks([n], q)
                h = Fraction(float(q)) * (n - 1)
                number = (lambda x: Fraction(int(x))) if s.dtype.kind == "i" else (lambda x: Fraction(float(x)))
                want = float(number(s[lo[0]]) + (number(s[hi[0]]) - number(s[lo[0]])) * (h - lo[0]))
                got = quantile_columns(s[lo], s[hi], t)[0]
                assert got == want == exact_quantile(s, q), (n, q, s.dtype)


def test_against_numpy_where_numpy_is_exact():
    """integer-valued raw and q in {0, 0.5, 1} or (n - 1) q an integer: the value is an order statistic or the midpoint of
    two integers, and both of NumPy's interpolation branches are exact there.  Elsewhere np.quantile rounds (n - 1) q."""
    from cellulus_amd.measure import quantile_columns, quantile_ranks

    rng = np.random.default_rng(2)
    for n in AREAS + [5, 9, 17, 101]:
        v = rng.integers(0, 65536, n)
        for values in (v.astype(np.int32), v.astype(np.float32), v.astype(np.float64)):
            s = np.sort(values)
            qs = [0.0, 0.5, 1.0] + [q for q in (0.25, 0.75, 0.125) if ((n - 1) * Fraction(q)).denominator == 1]
            for q in qs:
                lo, hi, t = quantile_ranks([n], q)
                assert quantile_columns(s[lo], s[hi], t)[0] == np.quantile(values, q) == exact_quantile(s, q), (n, q)
            lo, hi, t = quantile_ranks([n], 0.5)
            median = quantile_columns(s[lo], s[hi], t)[0]
            assert median == np.median(values)
            dev = np.sort(np.abs(values.astype(np.float64) - median))
            assert quantile_columns(dev[lo], dev[hi], t)[0] == np.median(np.abs(values - np.median(values)))
    lab = np.repeat(np.arange(1, 5), 25).reshape(10, 10)
    raw = rng.integers(0, 4096, lab.shape).astype(np.int32)
    cols = ref_columns(lab, raw, (0.0, 0.5, 1.0), True)
    for row, i in enumerate(range(1, 5)):
        v = raw[lab == i]
        assert cols["intensity_q0.5"][row] == np.median(v) and cols["intensity_q0.0"][row] == v.min() and cols["intensity_q1.0"][row] == v.max()
        assert cols["intensity_mad"][row] == np.median(np.abs(v - np.median(v)))


def test_restatement_keys_and_flags():
    f = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    for values, raw_type in ((f, F32), (f.astype(np.float64), F64), (np.array([-2 ** 31, -1, 0, 1, 2 ** 31 - 1], np.int32), I32)):
        k = order_key(values)
        assert k.dtype == np.uint64 and (np.diff(k.astype(object)) > 0).all()        # strictly ascending, -0.0 below +0.0
        assert decode_key(k, raw_type).tobytes() == values.tobytes()
        assert raw_type == F64 or (k >> np.uint64(32) == 0).all()
    assert order_key(np.array([0.0], np.float32))[0] == 0x80000000 and order_key(np.array([0], np.int32))[0] == 0x80000000
    lab = np.array([[1, 1, 2, 0], [2, 1, 5, -1]])
    raw = np.array([[3.0, 1.0, 7.0, np.nan], [5.0, 2.0, 9.0, 9.0]], np.float32)
    rank = np.array([[0, 0], [0, 2], [1, 1], [0, 0]], np.uint64)
    out, bad = ref_order_stats(lab, raw, 4, rank)
    assert bad == 1 and decode_key(out[1], F32).tolist() == [1.0, 3.0] and decode_key(out[2], F32).tolist() == [7.0, 7.0]
    assert (out[3] == 0xFFFFFFFFFFFFFFFF).all()
    rank[1, 1] = 3
    out, bad = ref_order_stats(lab, raw, 4, rank)
    assert bad == 1 | 8 and out[1, 1] == 0xFFFFFFFFFFFFFFFF
    out, bad = ref_order_stats(lab, raw, 6, np.zeros((6, 1), np.uint64), centre=np.array([0, 2.5, 0, 0, 0, 9.0]))
    assert bad == 1 and decode_key(out[1], F64).tolist() == [0.5] and decode_key(out[5], F64).tolist() == [0.0]
    raw[0, 0] = np.inf
    assert ref_order_stats(lab, raw, 6, np.zeros((6, 1), np.uint64))[1] == 1 | 2
    assert ref_order_stats(lab, raw, 6, np.zeros((6, 1), np.uint64), area=[0, 3, 3, 0, 0, 1])[1] == 1 | 2 | 4


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    raw = open(os.path.join(ROOT, "include", "clx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, restype, nargs in (("clx_region_order_workspace", "size_t", 2), ("clx_region_order_stats", "int", 16),
                                 ("clx_region_order_phase", "int", 17)):
        assert re.search(r"\b%s\s+%s\s*\(" % (restype, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs
    # the workspace size is host arithmetic: at least the key buffer and a cursor per id; 0 for an argument out of range
    size = _clx.load().clx_region_order_workspace
    assert size(-1, 4) == 0 and size(10, 0) == 0 and size(10, 2 ** 24 + 1) == 0 and size(2 ** 32, 4) == 0
    assert size(0, 1) > 0 and size(0, 1) % 8 == 0
    for total, nid in ((1, 2), (1000, 7), (2 ** 20, 2 ** 24)):
        assert size(total, nid) >= 8 * total + 8 * nid and size(total, nid) % 8 == 0
    assert size(2 ** 20, 5) <= 3 * 8 * 2 ** 20               # the histograms of long segments stay a fraction of the keys


def test_cli_accepts_quantiles_and_mad():
    from click.testing import CliRunner

    from cellulus_amd import cli

    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and "--quantiles" in res.output and "--mad" in res.output and "--inscribed" in res.output
    res = CliRunner().invoke(cli.measure, ["--quantiles", "0.25,0.5,0.75", "--mad", "--inscribed", "--hull", "--topology",
                                           "--contacts", "missing.toml"])
    assert res.exit_code != 0 and "does not exist" in res.output        # the flags parse; the file is what is wrong
    res = CliRunner().invoke(cli.measure, ["--quantiles", "0.25;0.5", __file__])
    assert res.exit_code != 0 and "--quantiles" in res.output


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx, measure

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    raw = np.ones((4, 5), np.float32)
    for quantiles in ((0.5, float("nan")), (-0.25,), (1.0000001,), (0.5, 0.25, 0.5), tuple(np.linspace(0, 1, 17))):
        with pytest.raises(ValueError, match="^region_table:.*quantile"):
            measure.region_table(good, raw, device=fake, quantiles=quantiles)
    with pytest.raises(ValueError, match="^region_table:.*need raw"):
        measure.region_table(good, device=fake, quantiles=(0.5,))
    with pytest.raises(ValueError, match="^region_table:.*need raw"):
        measure.region_table(good, device=fake, mad=True)
    # 16 distinct quantiles pass this check; the next one (the labels) fails
    with pytest.raises(TypeError, match="^region_table: labels"):
        measure.region_table(good.astype(np.float32), raw, device=fake, quantiles=tuple(np.linspace(0, 1, 16)), mad=True)
