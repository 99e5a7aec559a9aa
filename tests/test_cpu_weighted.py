"""The host side of the weighted and border columns without a device: weighted_columns / border_intensity_columns against the
restatement of tests/weighted_ref.py bit for bit and against scipy.ndimage exactly, the restatement's border pixels against a
binary erosion, the corner cases, and the plumbing (declarations, prototypes, options, argument checks)."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from cellulus_amd.measure import (NO_PEAK, border_intensity, border_intensity_columns, border_table, intensity_shift, region_table,
                                  weighted_columns, weighted_moments, weighted_table)
from coloc_ref import same_floats
from weighted_ref import (border_words, ref_border, ref_border_columns, ref_border_mask, ref_max_keys, ref_weighted,
                          ref_weighted_columns, weighted_words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 5), (7, 129), (33, 31), (5, 4, 37), (9, 130)]


def _permutation_case(shape, seed):
    """ids 0..6 at random and raw a permutation of 0..npix-1 as float32: every maximum is unique"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 7, size=shape).astype(np.int32)
    present = min(6, labels.size)
    labels.reshape(-1)[:present] = np.arange(1, present + 1)     # every id is there
    raw = rng.permutation(labels.size).astype(np.float32).reshape(shape)
    return labels, raw


def _moments(labels, ids):
    """area (n) and Σz Σy Σx (n, 3) of the objects ids, as clx_region_moments gives them"""
    shape = (1,) * (3 - labels.ndim) + labels.shape
    coords = np.indices(shape).reshape(3, -1)
    flat = labels.reshape(-1)
    area = np.array([(flat == i).sum() for i in ids], dtype=np.int64)
    sum1 = np.array([[int(c[flat == i].sum()) for c in coords] for i in ids], dtype=np.uint64).reshape(len(ids), 3)
    return area, sum1


def _host_weighted(labels, raw, shift, k=0):
    """the host columns from the restatement's words, and the restatement's own columns"""
    nid = int(labels.max()) + 1
    ids = np.unique(labels[labels > 0])
    rows, bad = ref_weighted(labels, raw, nid, shift, ref_max_keys(labels, raw, nid, shift))
    assert bad == 0
    area, sum1 = _moments(labels, ids)
    table = weighted_table(weighted_words(rows)[ids])
    got = weighted_columns(area, sum1, table, shift, labels.ndim, k, labels.shape)
    want = ref_weighted_columns(area, sum1, [rows[i] for i in ids], shift, labels.ndim, k, labels.shape)
    return ids, got, want


def _assert_same(got, want):
    assert list(got) == list(want)
    for name in want:
        if got[name].dtype == np.float64:
            assert same_floats(got[name], want[name]), (name, got[name][:4], want[name][:4])
        else:
            assert got[name].tolist() == list(want[name]), name


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_weighted_columns_equal_restatement_and_scipy(shape):
    labels, raw = _permutation_case(shape, 5)
    shift = intensity_shift(float(raw.max()), labels.size)
    ids, got, want = _host_weighted(labels, raw, shift)
    _assert_same(got, want)
    nd = len(shape)
    axes = "zyx"[3 - nd:]
    assert list(got) == (["intensity_sum_c0"] + [f"centroid_weighted_{a}_c0" for a in axes]
                         + [f"cov_weighted_{p}_c0" for p in (("yy", "xx", "yx") if nd == 2 else ("zz", "yy", "xx", "zy", "zx", "yx"))]
                         + ["mass_displacement_c0"] + [f"intensity_peak_{a}_c0" for a in axes])
    assert all(got[f"intensity_peak_{a}_c0"].dtype == np.int64 for a in axes)
    # scipy's centre of mass is one correctly rounded division of exactly representable sums here: EQUAL
    with np.errstate(invalid="ignore"):
        centres = ndimage.center_of_mass(raw.astype(np.float64), labels, ids)
    peaks = ndimage.maximum_position(raw, labels, ids)
    checked = 0
    for row, (c, p) in enumerate(zip(centres, peaks)):
        for a, axis in enumerate(axes):
            if np.isnan(c[a]):                               # the one pixel of value 0 alone in its object
                assert np.isnan(got[f"centroid_weighted_{axis}_c0"][row])
            else:
                assert got[f"centroid_weighted_{axis}_c0"][row] == c[a], (row, axis)
            assert got[f"intensity_peak_{axis}_c0"][row] == p[a]
            checked += 1
    assert checked == len(ids) * nd
    sums = ndimage.sum_labels(raw.astype(np.float64), labels, ids)
    assert np.array_equal(got["intensity_sum_c0"], sums)
    # the displacement is the distance between the two centroids, loosely in float64
    plain = np.array(ndimage.center_of_mass(np.ones(shape), labels, ids))
    ok = ~np.isnan(np.array(centres)).any(axis=1)
    assert np.allclose(got["mass_displacement_c0"][ok], np.linalg.norm(plain - np.array(centres), axis=1)[ok], rtol=1e-9, atol=1e-12)


def test_scipy_comparison_covers_68_coordinates():
    labels = [_permutation_case(s, 5)[0] for s in SHAPES]
    assert sum(len(np.unique(lab[lab > 0])) * lab.ndim for lab in labels) == 68


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_border_restatement_equals_erosion_and_columns(shape):
    labels, raw = _permutation_case(shape, 6)
    nd = len(shape)
    nid = int(labels.max()) + 1
    mask = ref_border_mask(labels, nid, nd)
    structure = ndimage.generate_binary_structure(nd, 1)
    for i in range(1, nid):
        m = labels == i
        assert np.array_equal(mask & m, m & ~ndimage.binary_erosion(m, structure, border_value=0)), i
    ids = np.unique(labels[labels > 0])
    for channel in (raw, raw.astype(np.float64) * 0.37 - 11.0, (raw.astype(np.int32) - labels.size // 2)):
        shift = 0 if channel.dtype.kind == "i" else intensity_shift(float(np.abs(channel).max()), labels.size)
        rows, bad = ref_border(labels, channel, nid, nd, shift)
        assert bad == 0
        table = border_table(border_words(rows)[ids])
        raw_type = {"float32": 0, "float64": 1, "int32": 2}[channel.dtype.name]
        got = border_intensity_columns(table, shift, raw_type, 3)
        _assert_same(got, ref_border_columns([rows[i] for i in ids], shift, channel.dtype, 3))
        pixels = border_intensity_columns(table)
        assert list(pixels) == ["intensity_border_pixels"] and pixels["intensity_border_pixels"].dtype == np.int64
        for row, i in enumerate(ids):
            v = channel[mask & (labels == i)]
            assert pixels["intensity_border_pixels"][row] == v.size
            assert got["intensity_border_min_c3"][row] == v.min() and got["intensity_border_max_c3"][row] == v.max()
            assert got["intensity_border_min_c3"].dtype == channel.dtype
            assert np.isclose(got["intensity_border_mean_c3"][row], v.astype(np.float64).mean(), rtol=1e-6, atol=1e-6)
            assert np.isclose(got["intensity_border_std_c3"][row], v.astype(np.float64).std(), rtol=1e-6, atol=1e-4)
            assert np.isclose(got["intensity_border_sum_c3"][row], v.astype(np.float64).sum(), rtol=1e-6, atol=1e-4)


def test_corner_cases():
    # Σq = 0: NaN in every float column but the sum; the peak is still there
    labels = np.array([[1, 1, 0], [2, 2, 2]], np.int32)
    raw = np.array([[3.0, -3.0, 9.0], [0.0, 0.0, 0.0]], np.float32)
    ids, got, want = _host_weighted(labels, raw, 2)
    _assert_same(got, want)
    assert got["intensity_sum_c0"].tolist() == [0.0, 0.0]
    for name in ("centroid_weighted_y_c0", "centroid_weighted_x_c0", "cov_weighted_yy_c0", "cov_weighted_yx_c0", "mass_displacement_c0"):
        assert np.isnan(got[name]).all(), name
    assert got["intensity_peak_y_c0"].tolist() == [0, 1] and got["intensity_peak_x_c0"].tolist() == [0, 0]    # ties: the first pixel
    # negative weights: the centroid may leave the object, the "covariance" may be negative; exact all the same
    raw = np.array([[3.0, -1.0, 9.0], [-2.0, -4.0, 1.0]], np.float32)
    ids, got, want = _host_weighted(labels, raw, 0)
    _assert_same(got, want)
    assert got["centroid_weighted_x_c0"].tolist() == [-0.5, -2 / -5] and got["cov_weighted_xx_c0"][0] == (2 * -1 - 1) / 4
    assert got["intensity_sum_c0"].tolist() == [2.0, -5.0] and got["intensity_peak_x_c0"].tolist() == [0, 2]
    # a one-pixel object: displacement 0, covariance 0, and its border is itself
    one = np.zeros((3, 4, 5), np.int32)
    one[1, 2, 3] = 1
    raw = np.full(one.shape, 2.5, np.float64)
    ids, got, want = _host_weighted(one, raw, 7)
    _assert_same(got, want)
    assert got["mass_displacement_c0"].tolist() == [0.0] and all(got[f"cov_weighted_{p}_c0"].tolist() == [0.0] for p in ("zz", "yy", "xx", "zy", "zx", "yx"))
    assert [got[f"centroid_weighted_{a}_c0"][0] for a in "zyx"] == [1.0, 2.0, 3.0] == [got[f"intensity_peak_{a}_c0"][0] for a in "zyx"]
    rows, _ = ref_border(one, raw, 2, 3, 7)
    cols = border_intensity_columns(border_table(border_words(rows)[1:]), 7, 1, 0)
    assert border_intensity_columns(border_table(border_words(rows)[1:]))["intensity_border_pixels"].tolist() == [1]
    assert [cols[f"intensity_border_{n}_c0"][0] for n in ("sum", "mean", "std", "min", "max")] == [2.5, 2.5, 0.0, 2.5, 2.5]
    # a shift at both clamps: float64 values near the ends of the exponent range (intensity_shift itself reaches the upper
    # clamp only; the lower one is what region_table's first pass over a channel with non-finite background uses)
    labels = np.array([[1, 1, 1, 2, 2]], np.int32)
    m = np.array([[4.0, 12.0, -4.0, 12.0, 12.0]])
    assert intensity_shift(12 * 2.0 ** -1020, 5) == 1023
    for raw, shift in ((m * 2.0 ** -1020, 1023), (m * 2.0 ** 1020, -1022)):
        ids, got, want = _host_weighted(labels, raw, shift)
        _assert_same(got, want)
        assert got["centroid_weighted_x_c0"].tolist() == [1 / 3, 3.5] and got["intensity_sum_c0"][0] == raw[0, 1]
        rows, _ = ref_border(labels, raw, 3, 2, shift)
        cols = border_intensity_columns(border_table(border_words(rows)[1:]), shift, 1, 0)
        _assert_same(cols, ref_border_columns(rows[1:], shift, raw.dtype, 0))
        assert cols["intensity_border_mean_c0"].tolist() == [raw[0, 0], raw[0, 3]] and cols["intensity_border_std_c0"][1] == 0.0
    # no peak under a present object is an internal error
    words = weighted_words([[1, 5, NO_PEAK, 0, 0, 0, 0, 0, 0, 0, 0, 0]])
    with pytest.raises(RuntimeError, match="internal error"):
        weighted_columns([1], [[0, 0, 0]], weighted_table(words), 0, 2, 0, (1, 1))
    # no objects: every column is there, empty, in its dtype
    empty = weighted_columns([], np.zeros((0, 3)), weighted_table(np.zeros((0, 21), np.uint64)), 0, 3, 1, (2, 2, 2))
    assert all(len(v) == 0 for v in empty.values()) and empty["intensity_peak_z_c1"].dtype == np.int64 and empty["cov_weighted_zy_c1"].dtype == np.float64
    empty = border_intensity_columns(border_table(np.zeros((0, 7), np.uint64)), 0, 0, 2)
    assert all(len(v) == 0 for v in empty.values()) and empty["intensity_border_min_c2"].dtype == np.float32
    assert math.isnan(border_intensity_columns(border_table(border_words([[2, 0, 0, NO_PEAK, 0, 0]])), 0, 2, 0)["intensity_border_mean_c0"][0])


def test_tables_decode_signed_128_bit_words():
    rows = [[7, -5, 3, -1, 2 ** 100, -2 ** 100, 2 ** 64, -2 ** 64, 2 ** 127 - 1, -2 ** 127, 0, -2 ** 63]]
    t = weighted_table(weighted_words(rows))
    assert list(t) == ["n", "sum_q", "peak", "sum_qz", "sum_qy", "sum_qx", "sum_qzz", "sum_qyy", "sum_qxx", "sum_qzy", "sum_qzx", "sum_qyx"]
    assert [int(t[k][0]) for k in t] == rows[0] and t["n"].dtype == np.int64 and t["sum_qz"].dtype == object
    b = border_table(border_words([[9, 8, -7, 5, 2 ** 64 - 2, 2 ** 90 + 1]]))
    assert [int(b[k][0]) for k in b] == [9, 8, -7, 5, 2 ** 64 - 2, 2 ** 90 + 1] and list(b) == ["pixels", "n", "sum_q", "key_min", "key_max", "sum_qq"]


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name in ("clx_region_weighted", "clx_region_border_intensity"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == 12 and _clx.PROTOTYPES[name][0] is ctypes.c_int
    assert _clx.load().clx_abi_version() == 13


def test_entry_points_refuse_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def weighted(raw_type=0, Z=1, Y=8, X=8, nid=4, **ptrs):
        p = dict(labels=some, raw=some, keys=some, out=some, bad=some)
        p.update(ptrs)
        return lib.clx_region_weighted(p["labels"], p["raw"], raw_type, Z, Y, X, nid, 0, p["keys"], p["out"], p["bad"], null)

    def border(raw_type=0, nd=2, Z=1, Y=8, X=8, nid=4, **ptrs):
        p = dict(labels=some, raw=some, out=some, bad=some)
        p.update(ptrs)
        return lib.clx_region_border_intensity(p["labels"], p["raw"], raw_type, nd, Z, Y, X, nid, 0, p["out"], p["bad"], null)

    common = [(dict(raw_type=3), "raw_type"), (dict(raw_type=-1), "raw_type"), (dict(nid=0), "nid"), (dict(nid=2 ** 24 + 1), "nid"),
              (dict(Y=0), "shape"), (dict(X=-4), "shape")]
    cases = [("clx_region_weighted", weighted, [({k: null}, "null pointer") for k in ("labels", "raw", "out", "bad")] + common
              + [(dict(Z=0), "shape"), (dict(Z=2 ** 12, Y=2 ** 10, X=2 ** 10), "2^32")]),
             ("clx_region_border_intensity", border, [({k: null}, "null pointer") for k in ("labels", "raw", "out", "bad")] + common
              + [(dict(nd=3, Z=0), "shape"), (dict(nd=3, Z=2 ** 12, Y=2 ** 10, X=2 ** 10), "2^32"), (dict(nd=1), "nd"), (dict(nd=4), "nd"),
                 (dict(nd=2, Z=3), "nd == 2")])]
    for who, call, refused in cases:
        for kw, word in refused:
            assert call(**kw) == -1, f"{who}{kw} was not refused"
            message = lib.clx_last_error().decode()
            assert message.startswith(who) and word in message, f"{who}{kw}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="clx_region_weighted.*nid"):
        _clx.call("clx_region_weighted", some, some, 0, 1, 8, 8, 0, 0, null, some, some, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import measure

    text = CliRunner().invoke(measure, ["--help"]).output
    assert "--weighted" in text and "--border-intensity" in text
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(measure, [__file__, "--weighted", "--border-intensity"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx, measure

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    labels = np.ones((4, 5), np.int32)
    one = np.ones((4, 5), np.float32)
    for flags in (dict(weighted=True), dict(border_intensity=True), dict(weighted=True, border_intensity=True)):
        with pytest.raises(ValueError, match="^region_table: weighted and border_intensity need raw"):
            region_table(labels, device=fake, **flags)
    for helper, who in ((weighted_moments, "weighted_moments"), (border_intensity, "border_intensity")):
        with pytest.raises(ValueError, match=f"^{who}: raw is needed"):
            helper(labels, None, device=fake)
        for k in (1, -1):
            with pytest.raises(ValueError, match=f"^{who}: channel k"):
                helper(labels, one, k, device=fake)
        with pytest.raises(ValueError, match=f"^{who}: raw has shape"):
            helper(labels, np.ones((2, 4, 6), np.float32), device=fake)
    with pytest.raises(TypeError, match="^region_table: labels"):
        region_table(labels.astype(np.float32), one, device=fake, weighted=True, border_intensity=True)
    # the new arguments are the last two of all three signatures
    import inspect

    for f in (measure.region_table, measure._region_table, measure.measure):
        assert list(inspect.signature(f).parameters)[-2:] == ["weighted", "border_intensity"]
