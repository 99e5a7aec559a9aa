"""The host side of the relate stage without a device: assign_parents / relate_columns against the restatement of
tests/relate_ref.py bit for bit and against a 6 x 6 example whose numbers stand here, tertiary_labels, and the plumbing
(declarations, prototypes, refusals, the command's options, argument checks before any device)."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from cellulus_amd.relate import assign_parents, label_overlaps, relate, relate_columns, relate_stage, tertiary_labels
from coloc_ref import same_floats
from inscribed_ref import ref_distance_sq
from relate_ref import ALL_ONES, blob_map, clearance_words, ref_clearance, ref_overlaps, ref_parents, ref_relate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILDREN = np.array([[1, 1, 0, 0, 2, 2],
                     [1, 1, 0, 0, 2, 2],
                     [0, 3, 3, 3, 0, 0],
                     [0, 3, 3, 3, 0, 0],
                     [4, 4, 0, 0, 5, 5],
                     [4, 4, 0, 0, 5, 5]], np.int32)
PARENTS = np.array([[1, 1, 1, 0, 0, 0],
                    [1, 1, 1, 0, 0, 0],
                    [1, 1, 2, 2, 0, 6],
                    [3, 3, 2, 2, 0, 6],
                    [3, 3, 0, 0, 4, 5],
                    [3, 3, 0, 0, 4, 5]], np.int32)


def moments(labels):
    """(label, area, Σz Σy Σx) of the objects present, as clx_region_moments gives them"""
    labels = np.asarray(labels)
    coords = np.indices((1,) * (3 - labels.ndim) + labels.shape).reshape(3, -1)
    flat = labels.reshape(-1)
    ids = np.unique(flat[flat > 0]).astype(np.int64)
    area = np.array([(flat == i).sum() for i in ids], dtype=np.int64)
    sum1 = np.array([[int(c[flat == i].sum()) for c in coords] for i in ids], dtype=np.uint64).reshape(len(ids), 3)
    return ids, area, sum1


def host_tables(children, parents, clearance=False, edge=False):
    """relate_columns fed with the restatement's integers"""
    nid_a, nid_b = int(children.max()) + 1, int(parents.max()) + 1
    keys, counts, flags = ref_overlaps(children, parents, nid_a, nid_b)
    assert flags == 0
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    rows = None
    if clearance:
        label, parent, _ = assign_parents(a, b, counts)
        table = np.zeros(nid_a, np.int64)
        table[label] = parent
        words, bad = ref_clearance(children, parents, ref_distance_sq(parents, edge), table, nid_a)
        assert bad == 0
        rows = clearance_words(words)[label].view(np.int64)          # as the device words arrive: int64 views
    return relate_columns(a, b, counts, moments(children), moments(parents), children.shape, rows)


def assert_same_tables(got, want):
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for name in w:
            assert g[name].dtype == w[name].dtype, (name, g[name].dtype)
            if w[name].dtype == np.float64:
                assert same_floats(g[name], w[name]), (name, g[name], w[name])
            else:
                assert np.array_equal(g[name], w[name]), (name, g[name], w[name])


def _random_maps(shape, seed, na=9, nb=6):
    return blob_map(shape, na, seed), blob_map(shape, nb, seed + 100)


def test_by_hand_6x6():
    child, parent = host_tables(CHILDREN, PARENTS, clearance=True)
    assert child["label"].tolist() == [1, 2, 3, 4, 5] and child["area"].tolist() == [4, 4, 6, 4, 4]
    assert child["parent"].tolist() == [1, 0, 2, 3, 4]          # 3 lies across 1, 2 and 3; 5 ties between 4 and 5: the smaller id
    assert child["overlap"].tolist() == [4, 0, 4, 4, 2]
    assert child["fraction_inside"].tolist() == [1.0, 0.0, 4 / 6, 1.0, 0.5]
    assert child["outside"].tolist() == [0, 4, 0, 0, 0] and child["num_parents"].tolist() == [1, 0, 3, 1, 2]
    d = child["parent_centroid_distance"]
    assert d[0] == math.sqrt(18) / 8 and math.isnan(d[1]) and d[2:].tolist() == [0.5, 0.5, 0.5]
    c = child["clearance"]
    assert c[0] == math.sqrt(2) and math.isnan(c[1]) and c[2:].tolist() == [1.0, 1.0, 1.0]
    assert child["clearance_y"].tolist() == [1, -1, 2, 4, 4] and child["clearance_x"].tolist() == [1, -1, 2, 1, 4]
    m = child["depth_sq_mean"]
    assert m[0] == 4.5 and math.isnan(m[1]) and m[2:].tolist() == [1.0, 2.5, 1.0]
    assert parent["label"].tolist() == [1, 2, 3, 4, 5, 6] and parent["area"].tolist() == [8, 4, 6, 2, 2, 2]
    assert parent["num_children"].tolist() == [1, 1, 1, 1, 0, 0]                # 5 holds half of child 5 but is not its parent
    assert parent["children_area"].tolist() == [5, 4, 5, 2, 2, 0]
    assert parent["children_fraction"].tolist() == [5 / 8, 1.0, 5 / 6, 1.0, 1.0, 0.0]
    assert parent["tertiary_area"].tolist() == [3, 0, 1, 0, 0, 2]
    assert list(child) == ["label", "area", "parent", "overlap", "fraction_inside", "outside", "num_parents",
                           "parent_centroid_distance", "clearance", "clearance_y", "clearance_x", "depth_sq_mean"]
    assert list(parent) == ["label", "area", "num_children", "children_area", "children_fraction", "tertiary_area"]
    assert_same_tables((child, parent), ref_relate(CHILDREN, PARENTS, clearance=True))
    plain = host_tables(CHILDREN, PARENTS)
    assert list(plain[0]) == list(child)[:8] and all(np.array_equal(plain[0][k], child[k], equal_nan=True) for k in plain[0])
    t = tertiary_labels(CHILDREN, PARENTS)
    assert t.dtype == PARENTS.dtype and np.array_equal(t, np.where(CHILDREN > 0, 0, PARENTS))
    assert [int((t == j).sum()) for j in range(1, 7)] == parent["tertiary_area"].tolist()
    tt = tertiary_labels(torch.from_numpy(CHILDREN), torch.from_numpy(PARENTS.astype(np.int64)))
    assert tt.dtype == torch.int64 and np.array_equal(tt.numpy(), t)


@pytest.mark.parametrize("shape,edge", [((23, 31), False), ((23, 31), True), ((6, 11, 13), False), ((6, 11, 13), True), ((1, 1), True)])
def test_columns_equal_restatement(shape, edge):
    children, parents = _random_maps(shape, 7 + len(shape))
    assert_same_tables(host_tables(children, parents, clearance=True, edge=edge), ref_relate(children, parents, True, edge))
    assert_same_tables(host_tables(children, parents), ref_relate(children, parents))


def test_assign_parents_ties_and_orphans():
    # rows in any order; a: 1 ties 7 / 3 / 9 at 5 pixels, 2 has background only, 4 one parent, 6 a larger later row
    a = [1, 4, 1, 2, 1, 6, 0, 6, 1, 0]
    b = [7, 2, 3, 0, 9, 1, 5, 8, 0, 3]
    n = [5, 1, 5, 9, 5, 2, 4, 3, 50, 6]
    label, parent, overlap = assign_parents(a, b, n)
    assert label.tolist() == [1, 2, 4, 6] and parent.tolist() == [3, 0, 2, 8] and overlap.tolist() == [5, 0, 1, 3]
    assert label.dtype == parent.dtype == overlap.dtype == np.int64
    empty = assign_parents([], [], [])
    assert all(len(v) == 0 and v.dtype == np.int64 for v in empty)
    for shape, seed in (((23, 31), 3), ((6, 11, 13), 4)):
        children, parents = _random_maps(shape, seed)
        keys, counts, _ = ref_overlaps(children, parents, 10, 7)
        got = assign_parents(keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF), counts)
        assert all(np.array_equal(g, w) for g, w in zip(got, ref_parents(children, parents)))
    with pytest.raises(ValueError, match="^assign_parents: ids_a, ids_b and pixels"):
        assign_parents([1], [1, 2], [3])
    with pytest.raises(ValueError, match="^assign_parents: ids must be"):
        assign_parents([1], [1], [0])


def test_corner_cases_of_the_tables():
    # no children / no parents / nothing at all: every column is there, in its dtype
    zeros = np.zeros((4, 5), np.int32)
    for children, parents in ((zeros, PARENTS[:4, :5]), (CHILDREN[:4, :5], zeros), (zeros, zeros)):
        got = host_tables(children, parents, clearance=True)
        assert_same_tables(got, ref_relate(children, parents, True))
        assert len(got[0]["label"]) == len(np.unique(children)) - 1 and len(got[1]["label"]) == len(np.unique(parents)) - 1
    # a parent that fills a map without an edge to measure to: inf; with the edge: the distance to it
    full = np.ones((3, 4), np.int32)
    kid = np.zeros((3, 4), np.int32)
    kid[1, 1:3] = 2
    child, _ = host_tables(kid, full, clearance=True)
    assert child["clearance"].tolist() == [math.inf] and child["depth_sq_mean"].tolist() == [math.inf]
    assert child["clearance_y"].tolist() == [1] and child["clearance_x"].tolist() == [1]
    child, _ = host_tables(kid, full, clearance=True, edge=True)
    assert child["clearance"].tolist() == [2.0] and child["depth_sq_mean"].tolist() == [4.0]
    # rows that do not belong to the moments, and clearance rows that do not belong to the rows
    ids = moments(CHILDREN), moments(PARENTS)
    with pytest.raises(ValueError, match="^relate_columns: the overlap rows and the moments"):
        relate_columns([1], [1], [4], *ids, (6, 6))
    keys, counts, _ = ref_overlaps(CHILDREN, PARENTS, 6, 7)
    a, b = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    with pytest.raises(ValueError, match="^relate_columns: clearance has 2 rows"):
        relate_columns(a, b, counts, *ids, (6, 6), np.zeros((2, 3), np.int64))
    wrong = np.array([[0, ALL_ONES, 0]] * 5, np.uint64)
    with pytest.raises(ValueError, match="^relate_columns: the clearance rows and the overlap rows"):
        relate_columns(a, b, counts, *ids, (6, 6), wrong)
    with pytest.raises(ValueError, match="^relate_columns: shape must have 2 or 3"):
        relate_columns(a, b, counts, *ids, (36,))


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, nargs in (("clx_label_overlaps", 10), ("clx_region_clearance", 9)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs and _clx.PROTOTYPES[name][0] is ctypes.c_int
    assert _clx.load().clx_abi_version() == 13


def test_entry_points_refuse_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def overlaps(npix=64, nid_a=4, nid_b=4, capacity=1024, **ptrs):
        p = dict(a=some, b=some, keys=some, counts=some, info=some)
        p.update(ptrs)
        return lib.clx_label_overlaps(p["a"], p["b"], npix, nid_a, nid_b, capacity, p["keys"], p["counts"], p["info"], null)

    def clearance(npix=64, nid_a=4, **ptrs):
        p = dict(a=some, b=some, dist_sq=some, parent=some, out=some, bad=some)
        p.update(ptrs)
        return lib.clx_region_clearance(p["a"], p["b"], p["dist_sq"], p["parent"], npix, nid_a, p["out"], p["bad"], null)

    npix = [(dict(npix=0), "npix"), (dict(npix=-1), "npix"), (dict(npix=2 ** 32), "npix")]
    cases = [("clx_label_overlaps", overlaps, [({k: null}, "null pointer") for k in ("a", "b", "keys", "counts", "info")] + npix
              + [(dict(nid_a=0), "nid_a"), (dict(nid_a=2 ** 24 + 1), "nid_a"), (dict(nid_b=0), "nid_b"), (dict(nid_b=2 ** 24 + 1), "nid_b"),
                 (dict(nid_b=-3), "nid_b")]
              + [(dict(capacity=c), "capacity") for c in (0, 512, 1025, 3072, 2 ** 29, -1024)]),
             ("clx_region_clearance", clearance, [({k: null}, "null pointer") for k in ("a", "b", "dist_sq", "parent", "out", "bad")] + npix
              + [(dict(nid_a=0), "nid_a"), (dict(nid_a=-1), "nid_a"), (dict(nid_a=2 ** 24 + 1), "nid_a")])]
    for who, call, refused in cases:
        for kw, word in refused:
            assert call(**kw) == -1, f"{who}{kw} was not refused"
            message = lib.clx_last_error().decode()
            assert message.startswith(who) and word in message, f"{who}{kw}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="clx_label_overlaps.*capacity"):
        _clx.call("clx_label_overlaps", some, some, 64, 4, 4, 1000, some, some, some, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import relate as relate_cli

    text = CliRunner().invoke(relate_cli, ["--help"]).output
    assert all(option in text for option in ("--children", "--parents", "--clearance", "--tertiary"))
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(relate_cli, [__file__, "--children", "nuclei", "--parents", "cells", "--clearance", "--tertiary", "cyto"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output
    result = CliRunner().invoke(relate_cli, [__file__, "--children", "nuclei"])
    assert result.exit_code == 2 and "--parents" in result.output


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for f, who, kw in ((relate, "relate", dict(device=fake)), (relate, "relate", dict(device=fake, clearance=True)),
                       (label_overlaps, "label_overlaps", dict(device=fake)), (tertiary_labels, "tertiary_labels", {})):
        with pytest.raises(ValueError, match=f"^{who}: .* has shape"):
            f(good, np.ones((4, 6), np.int32), **kw)
        with pytest.raises(ValueError, match=f"^{who}: .* has shape"):
            f(torch.ones(4, 5, dtype=torch.int32), np.ones((5, 4), np.int32), **kw)
        for floats in (good.astype(np.float32), torch.ones(4, 5), good.astype(bool)):
            with pytest.raises(TypeError, match=f"^{who}: .* must be integers"):
                f(good, floats, **kw)
            with pytest.raises(TypeError, match=f"^{who}: .* must be integers"):
                f(floats, good, **kw)
        for shape in ((20,), (1, 1, 4, 5)):
            with pytest.raises(ValueError, match=f"^{who}: .* must be 2-D or 3-D"):
                f(np.ones(shape, np.int32), np.ones(shape, np.int32), **kw)
        with pytest.raises(TypeError, match=f"^{who}: .* must be an array or a tensor"):
            f([[1, 2]], good, **kw)
    for kw in (dict(children="", parents="cells"), dict(children="nuclei", parents=None), dict(children="x", parents="x"),
               dict(children="nuclei", parents="cells", tertiary="cells"), dict(children="nuclei", parents="cells", tertiary="")):
        with pytest.raises(ValueError, match="^relate_stage: "):
            relate_stage(None, **kw)
