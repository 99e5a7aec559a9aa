"""The expand stage without a device: the restatements of tests/nearest_ref.py against scipy's distance transform and against
each other, the limit's rounding, zone_columns by hand, and the plumbing (declarations, prototypes, refusals, the command's
options, argument checks before any device)."""

import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy import ndimage

from cellulus_amd.expand import _limit_sq, expand_labels, expand_stage, nearest_object, zone_columns, zone_table
from nearest_ref import DIST_INF, dots_map, ref_nearest, ref_nearest_tree, ref_zone_table
from relate_ref import blob_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = {"blobs_2d": blob_map((23, 31), 7, 3, 6), "dots_2d": dots_map((30, 26), 12, 4), "blobs_3d": blob_map((6, 11, 13), 5, 5, 5),
         "dots_3d": dots_map((5, 9, 12), 6, 6), "one_pixel": np.pad(np.ones((1, 1), np.int32), ((4, 2), (0, 7)))}


def unique_nearest(labels):
    """where exactly one OBJECT is nearest: the smallest and the largest id at the smallest distance agree"""
    lab = np.asarray(labels).astype(np.int64)
    nid = int(lab.max()) + 1
    low, dist, _ = ref_nearest(lab, nid)
    high, dist_high, _ = ref_nearest(np.where(lab > 0, nid - lab, 0), nid)           # the ids reversed: the largest wins
    assert np.array_equal(dist, dist_high)
    return low == np.where(high > 0, nid - high, 0)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_restatement_agrees_with_scipy(name):
    labels = SMALL[name]
    nid = int(labels.max()) + 1
    nearest, dist, bad = ref_nearest(labels, nid)
    edt, indices = ndimage.distance_transform_edt(labels == 0, return_indices=True)
    assert bad == 0 and np.array_equal(dist, np.rint(edt ** 2).astype(np.int64))
    theirs = labels[tuple(indices)]
    unique = unique_nearest(labels)
    assert np.array_equal(nearest[unique], theirs[unique]) and (nearest <= theirs).all() and (nearest > 0).all()
    assert np.array_equal(nearest[labels > 0], labels[labels > 0]) and (dist[labels > 0] == 0).all()
    assert unique.sum() > labels.size // 2


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("limit_sq", [-1, 0, 9])
def test_tree_restatement_equals_all_pairs(name, limit_sq):
    labels = SMALL[name].copy()
    labels.flat[3], labels.flat[-2] = -1, int(labels.max()) + 1            # out of range: background, and reported
    nid = int(labels.max())
    want = ref_nearest(labels, nid, limit_sq)
    got = ref_nearest_tree(labels, nid, limit_sq)
    assert want[2] == got[2] == 1 and np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    if limit_sq >= 0:
        assert ((want[1] <= limit_sq) == (want[0] > 0)).all() and (want[1][want[0] == 0] == DIST_INF).all()
    zeros = np.zeros((4, 5), np.int32)
    for f in (ref_nearest, ref_nearest_tree):
        nearest, dist, bad = f(zeros, 1, limit_sq)
        assert bad == 0 and (nearest == 0).all() and (dist == DIST_INF).all()


def test_limit_sq_at_the_edges():
    def admits(limit, offset):
        return sum(c * c for c in offset) <= _limit_sq(limit, "test")

    assert admits(5, (3, 4)) and admits(5, (5, 0)) and not admits(5, (4, 4))
    assert admits(5.0, (3, 4)) and admits(Fraction(5), (0, 5)) and admits(np.float32(5), (3, 4)) and admits(np.int64(5), (4, 3))
    assert admits(math.sqrt(2), (1, 1))                       # the float above the root: its square is above 2
    assert math.sqrt(2) ** 2 > 2 and Fraction(math.sqrt(2)) ** 2 > 2
    below = np.nextafter(math.sqrt(2), 0)
    assert not admits(below, (1, 1)) and admits(below, (1, 0))
    assert not admits(0, (1, 0)) and not admits(0.0, (0, 1)) and admits(0, (0, 0))
    assert _limit_sq(None, "test") == -1 and _limit_sq(0.999, "test") == 0 and _limit_sq(32767.99, "test") == 2 ** 30 - 656
    assert _limit_sq(32767, "test") == 32767 ** 2 and _limit_sq(Fraction(65535, 2), "test") == 2 ** 30 - 32768
    for bad in (32768, 32768.0, 1e300):
        with pytest.raises(ValueError, match="^test: the square of limit must be below 2\\^30"):
            _limit_sq(bad, "test")
    for bad in (-1, -1e-300, Fraction(-1, 3)):
        with pytest.raises(ValueError, match="^test: limit must be >= 0"):
            _limit_sq(bad, "test")
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="^test: limit must be finite"):
            _limit_sq(bad, "test")
    for bad in ("3", True, 1j, [3]):
        with pytest.raises(TypeError, match="^test: limit must be a real number"):
            _limit_sq(bad, "test")


def test_zone_columns_by_hand():
    # two single pixels in a 3 x 7 map, ids 1 at (1, 1) and 2 at (1, 5): column 3 is equidistant and goes to 1
    #   zones: columns 0 .. 3 -> 1 (12 pixels), columns 4 .. 6 -> 2 (9 pixels); they share 3 faces
    #   d² in zone 1: row 1 has 1 0 1 4, rows 0 and 2 have 2 1 2 5; in zone 2: 1 0 1 and 2 1 2
    rows = [[5, 3, 6 + 10 + 10], [2, 4, 2 + 5 + 5]]
    pairs = ([0, 1, 0], [2, 2, 1], [3 + 3 + 3, 3, 4 + 4 + 3])                       # unsorted; a == 0: here all towards the outside
    table, pair = zone_columns([1, 2], [1, 1], [12, 9], rows, *pairs, [11, 9], (3, 7))
    assert list(table) == ["label", "area", "zone_area", "zone_fraction", "zone_reach", "zone_reach_y", "zone_reach_x",
                           "zone_dist_sq_mean", "num_neighbours", "zone_border", "zone_border_open"]
    assert table["label"].tolist() == [1, 2] and table["area"].tolist() == [1, 1] and table["zone_area"].tolist() == [12, 9]
    assert table["zone_fraction"].tolist() == [1 / 12, 1 / 9] and table["zone_reach"].tolist() == [math.sqrt(5), math.sqrt(2)]
    assert table["zone_reach_y"].tolist() == [0, 0] and table["zone_reach_x"].tolist() == [3, 4]
    assert table["zone_dist_sq_mean"].tolist() == [26 / 12, 12 / 9]
    assert table["num_neighbours"].tolist() == [1, 1] and table["zone_border"].tolist() == [3, 3]
    assert table["zone_border_open"].tolist() == [0, 0]
    assert all(table[k].dtype == (np.float64 if k in ("zone_fraction", "zone_reach", "zone_dist_sq_mean") else np.int64) for k in table)
    assert list(pair) == ["label_a", "label_b", "faces"]
    assert [pair[k].tolist() for k in pair] == [[0, 0, 1], [1, 2, 2], [11, 9, 3]]
    labels = np.zeros((3, 7), np.int32)
    labels[1, 1], labels[1, 5] = 1, 2
    want = ref_zone_table(labels)
    for got_t, want_t in zip((table, pair), want):
        assert list(got_t) == list(want_t) and all(np.array_equal(got_t[k], want_t[k]) and got_t[k].dtype == want_t[k].dtype for k in want_t)
    # with a limit of 1 the zones are crosses of 5 pixels and 12 faces, 3 of them towards the outside, the others open
    table, _ = zone_columns([1, 2], [1, 1], [5, 5], [[1, 1, 4], [1, 5, 4]], [0, 0], [1, 2], [12, 12], [3, 3], (3, 7))
    assert table["zone_border_open"].tolist() == [9, 9] and table["num_neighbours"].tolist() == [0, 0]
    assert all(np.array_equal(table[k], ref_zone_table(labels, 1)[0][k]) for k in table)
    # one rounding: a ratio whose double division differs from dividing the rounded operands
    area, zone_area = 2 ** 53 + 1, 3
    table, _ = zone_columns([1], [area], [area * zone_area], [[0, 0, 0]], [], [], [], [0], (2, 2))
    assert table["zone_fraction"][0] == float(Fraction(area, area * zone_area)) == 1 / 3
    # empty tables have the columns, 3-D ones the z column
    none = np.zeros(0, np.int64)
    table, pair = zone_columns(none, none, none, np.zeros((0, 3), np.int64), none, none, none, none, (4, 5, 6))
    assert list(table)[4:8] == ["zone_reach", "zone_reach_z", "zone_reach_y", "zone_reach_x"] and len(table) == 12
    assert all(len(c) == 0 for t in (table, pair) for c in t.values()) and table["zone_reach"].dtype == np.float64
    with pytest.raises(ValueError, match="^zone_columns: shape must have 2 or 3"):
        zone_columns(none, none, none, np.zeros((0, 3), np.int64), none, none, none, none, (20,))
    with pytest.raises(ValueError, match="^zone_columns: needs increasing labels"):
        zone_columns([1], [4], [3], [[0, 0, 0]], [], [], [], [0], (2, 2))
    with pytest.raises(ValueError, match="^zone_columns: the pairs and edge_faces"):
        zone_columns([1], [4], [4], [[0, 0, 0]], [0], [1], [3], [8], (2, 2))
    with pytest.raises(ValueError, match="^zone_columns: the pairs need"):
        zone_columns([1], [4], [4], [[0, 0, 0]], [1], [3], [3], [8], (2, 2))


@pytest.mark.parametrize("name,limit_sq", [("dots_2d", -1), ("dots_2d", 10), ("dots_3d", -1), ("blobs_3d", 4)])
def test_zone_restatement_is_consistent(name, limit_sq):
    labels = SMALL[name]
    table, pair = ref_zone_table(labels, limit_sq)
    zones, dist, _ = ref_nearest(labels, int(labels.max()) + 1, limit_sq)
    assert table["zone_area"].sum() == (zones > 0).sum() and (table["zone_area"] >= table["area"]).all()
    assert (table["zone_border_open"] >= 0).all() and (table["zone_border_open"].sum() > 0) == bool((zones == 0).any())
    assert table["num_neighbours"].sum() == 2 * (pair["label_a"] > 0).sum()
    if limit_sq >= 0:
        assert (table["zone_reach"] <= math.sqrt(limit_sq)).all()


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, kind, restype, nargs in (("clx_label_nearest", "int", ctypes.c_int, 13),
                                       ("clx_label_nearest_workspace", "size_t", ctypes.c_size_t, 1)):
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs and _clx.PROTOTYPES[name][0] is restype
    lib = _clx.load()
    assert lib.clx_abi_version() == 13
    assert lib.clx_label_nearest_workspace(0) == 0 and lib.clx_label_nearest_workspace(2 ** 32) == 0 and lib.clx_label_nearest_workspace(-5) == 0
    assert lib.clx_label_nearest_workspace(1) == 8 and lib.clx_label_nearest_workspace(2 ** 32 - 1) == 8 * (2 ** 32 - 1)


def test_entry_point_refuses_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def nearest(nd=2, Z=1, Y=8, X=8, nid=4, limit_sq=-1, nbytes=None, **ptrs):
        p = dict(labels=some, nearest=some, dist_sq=some, bad=some, workspace=some)
        p.update(ptrs)
        nbytes = 8 * Z * Y * X if nbytes is None else nbytes
        return lib.clx_label_nearest(p["labels"], nd, Z, Y, X, nid, limit_sq, p["nearest"], p["dist_sq"], p["bad"], p["workspace"], nbytes,
                                     null)

    refused = [({k: null}, "null pointer") for k in ("labels", "nearest", "dist_sq", "bad", "workspace")] + [
        (dict(nd=1), "nd"), (dict(nd=4), "nd"), (dict(nd=2, Z=2), "Z == 1"),
        (dict(Y=0), "shape"), (dict(X=-1), "shape"), (dict(nd=3, Z=0), "shape"),
        (dict(nid=0), "nid"), (dict(nid=-1), "nid"), (dict(nid=2 ** 24 + 1), "nid"),
        (dict(limit_sq=-2), "limit_sq"), (dict(limit_sq=2 ** 30), "limit_sq"), (dict(limit_sq=2 ** 31 - 1), "limit_sq"),
        (dict(Y=65536, X=65536, nbytes=2 ** 40), "Z * Y * X"), (dict(nd=3, Z=2, Y=46341, X=46341, nbytes=2 ** 40), "Z * Y * X"),
        (dict(Y=2, X=32769), "(X-1)^2"), (dict(Y=23172, X=23172), "(X-1)^2"), (dict(nd=3, Z=23172, Y=23172, X=2), "(X-1)^2"),
        (dict(nbytes=8 * 64 - 1), "workspace_bytes"), (dict(nbytes=0), "workspace_bytes"),
        (dict(workspace=ctypes.c_void_p(4098)), "aligned"), (dict(workspace=ctypes.c_void_p(4097)), "aligned")]
    for kw, word in refused:
        assert nearest(**kw) == -1, f"clx_label_nearest{kw} was not refused"
        message = lib.clx_last_error().decode()
        assert message.startswith("clx_label_nearest:") and word in message, f"{kw}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="clx_label_nearest.*limit_sq"):
        _clx.call("clx_label_nearest", some, 2, 1, 8, 8, 4, -7, some, some, some, some, 512, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import expand as expand_cli

    text = CliRunner().invoke(expand_cli, ["--help"]).output
    assert all(option in text for option in ("--source", "--distance", "--output", "--neighbours", "--limit"))
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(expand_cli, [__file__, "--source", "nuclei", "--distance", "7.5", "--output", "cells", "--neighbours",
                                             "--limit", "20"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output
    result = CliRunner().invoke(expand_cli, [__file__, "--neighbours"])
    assert result.exit_code == 2 and "--source" in result.output
    result = CliRunner().invoke(expand_cli, [__file__, "--source", "nuclei", "--distance", "-1", "--output", "cells"])
    assert result.exit_code == 2 and "--distance" in result.output
    text = open(os.path.join(ROOT, "pyproject.toml")).read() + open(os.path.join(ROOT, "cellulus_amd", "infer.py")).read()
    assert "expand" not in text                               # no console script, and infer() does not run the stage


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    monkeypatch.setattr(_clx, "load", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    entries = ((nearest_object, "nearest_object", "limit", lambda m, v=None: dict(labels=m, limit=v, device=fake)),
               (zone_table, "zone_table", "limit", lambda m, v=None: dict(labels=m, limit=v, device=fake)),
               (expand_labels, "expand_labels", "distance", lambda m, v=1: dict(labels=m, distance=v, device=fake)))
    for f, who, name, kw in entries:
        for floats in (good.astype(np.float32), torch.ones(4, 5), good.astype(bool), torch.ones(4, 5, dtype=torch.bool)):
            with pytest.raises(TypeError, match=f"^{who}: labels must be integers"):
                f(**kw(floats))
        for shape in ((20,), (1, 1, 4, 5)):
            with pytest.raises(ValueError, match=f"^{who}: labels must be 2-D or 3-D"):
                f(**kw(np.ones(shape, np.int32)))
        with pytest.raises(TypeError, match=f"^{who}: labels must be an array or a tensor"):
            f(**kw([[1, 2]]))
        for bad, kind in ((-1, ValueError), (math.nan, ValueError), (32768, ValueError), ("2", TypeError)):
            with pytest.raises(kind, match=f"^{who}: .*{name}"):
                f(**kw(good, bad))
        with pytest.raises(ValueError, match=f"^{who}: label ids must lie in"):
            f(**kw(good - 2))
    with pytest.raises(TypeError, match="^expand_labels: distance must be a real number"):
        expand_labels(good, None, device=fake)
    for kw in (dict(source="", neighbours=True), dict(source=None, neighbours=True), dict(source="nuclei"),
               dict(source="nuclei", output="nuclei", distance=3), dict(source="nuclei", output="", distance=3),
               dict(source="nuclei", output="cells"), dict(source="nuclei", distance=3, neighbours=True),
               dict(source="nuclei", output="cells", distance=3, limit=4), dict(source="nuclei", output="cells", distance=-3),
               dict(source="nuclei", neighbours=True, limit=1e6), dict(source="nuclei", output="cells", distance=math.inf)):
        with pytest.raises(ValueError, match="^expand_stage: "):
            expand_stage(None, **kw)


def test_cpu_device_raises():
    from cellulus_amd._clx import ClxError

    labels = np.ones((4, 5), np.int32)
    for call in (lambda: nearest_object(labels, device="cpu"), lambda: expand_labels(labels, 2, device=torch.device("cpu")),
                 lambda: zone_table(labels, 3, device="cpu")):
        with pytest.raises(ClxError, match="no CPU path"):
            call()
