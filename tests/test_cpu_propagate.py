"""The propagate stage without a device: the two restatements of tests/propagate_ref.py against each other and against
hand-worked maps, the properties that follow from the definitions (transpose, limit, renumbering, connectedness), image_levels
and propagate_columns by hand, the symbols of the library, and every refusal that needs no device."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from propagate_ref import (COST_INF, dots_map, offsets, random_case, ref_propagate, ref_propagate_sweeps, ref_propagate_table,
                           ridge_image, serpentine)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = (None, 0, 7, 12)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def cases(seed, n):
    rng = np.random.default_rng(seed)
    return [random_case(rng, nd) for nd in (2, 3) for _ in range(n)]


def test_restatements_agree():
    for seeds, mask, weight, reg in cases(5, 12):
        for limit in LIMITS:
            a = ref_propagate(seeds, mask, weight, reg=reg, limit=limit)
            assert same(a, ref_propagate_sweeps(seeds, mask, weight, reg=reg, limit=limit))
            assert ((a[0] == 0) == (a[1] == COST_INF)).all() and np.array_equal(a[0][seeds > 0], seeds[seeds > 0])
            if limit is not None:
                assert (a[1][a[0] > 0] <= limit).all()


def test_transpose_limit_and_renumbering():
    for seeds, mask, weight, reg in cases(6, 8):
        whole = ref_propagate(seeds, mask, weight, reg=reg)
        turned = ref_propagate(seeds.T, None if mask is None else mask.T, None if weight is None else weight.T, reg=reg)
        assert np.array_equal(turned[0].T, whole[0]) and np.array_equal(turned[1].T, whole[1])
        for limit in (0, 7, 12):
            cut = ref_propagate(seeds, mask, weight, reg=reg, limit=limit)
            beyond = whole[1] > limit
            assert np.array_equal(cut[0], np.where(beyond, 0, whole[0])) and np.array_equal(cut[1], np.where(beyond, COST_INF, whole[1]))
        renumbered = ref_propagate(np.where(seeds > 0, 3 * seeds + 2, 0), mask, weight, reg=reg)      # monotone
        assert np.array_equal(renumbered[0], np.where(whole[0] > 0, 3 * whole[0] + 2, 0)) and np.array_equal(renumbered[1], whole[1])


def test_every_reached_pixel_has_a_parent_of_its_owner():
    for seeds, mask, weight, reg in cases(7, 8):
        owner, cost, _ = ref_propagate(seeds, mask, weight, reg=reg)
        w = np.zeros(seeds.shape, np.int64) if weight is None else weight.astype(np.int64)
        for q in zip(*np.nonzero((owner > 0) & (seeds == 0))):
            assert mask is None or mask[q]
            parents = []
            for d, a in offsets(seeds.ndim):
                p = tuple(x - y for x, y in zip(q, d))
                if all(0 <= x < n for x, n in zip(p, seeds.shape)) and owner[p] == owner[q]:
                    parents.append(int(cost[p]) + reg * a + abs(int(w[p]) - int(w[q])))
            assert int(cost[q]) in parents, q


def test_row_with_a_weight_jump_by_hand():
    seeds = np.array([[1, 0, 0, 0, 0, 0, 2]], np.int32)
    weight = np.array([[5, 5, 5, 9, 9, 9, 9]], np.int32)
    for ref in (ref_propagate, ref_propagate_sweeps):
        owner, cost, info = ref(seeds, None, weight, reg=1)
        # from the left: 3, 6, then 9 + 4 = 13; from the right: 3, 6, 9, then 12 + 4 = 16
        assert owner.tolist() == [[1, 1, 1, 2, 2, 2, 2]] and cost.tolist() == [[0, 3, 6, 9, 6, 3, 0]] and info == 0
        owner, cost, _ = ref(seeds, None, None, reg=1)                    # flat: the middle is a tie, the smaller id wins
        assert owner.tolist() == [[1, 1, 1, 1, 2, 2, 2]] and cost.tolist() == [[0, 3, 6, 9, 6, 3, 0]]
        owner, cost, _ = ref(seeds, np.array([[0, 1, 1, 0, 1, 1, 1]], np.uint8), weight, reg=2, limit=6)
        assert owner.tolist() == [[1, 1, 0, 0, 0, 2, 2]] and cost.tolist() == [[0, 6, COST_INF, COST_INF, COST_INF, 6, 0]]


def test_cube_corner_by_hand():
    seeds = np.zeros((3, 3, 3), np.int32)
    seeds[0, 0, 0] = 4
    for reg in (1, 3):
        for ref in (ref_propagate, ref_propagate_sweeps):
            owner, cost, _ = ref(seeds, None, None, reg=reg)
            assert (owner == 4).all() and cost[1, 1, 1] == 5 * reg and cost[2, 2, 2] == 10 * reg
            assert cost[0, 0, 1] == 3 * reg and cost[0, 1, 1] == 4 * reg and cost[2, 1, 0] == 7 * reg
    only = np.zeros((2, 2, 2), np.uint8)
    only[1, 1, 1] = 1                                                     # the far corner is the only allowed pixel
    owner, cost, _ = ref_propagate(seeds[:2, :2, :2], only, None, reg=7)
    assert owner[1, 1, 1] == 4 and cost[1, 1, 1] == 35 and (owner > 0).sum() == 2


def test_bad_ids_and_weights():
    seeds = np.array([[1, 0, 9, 0, 0, 2]], np.int32)
    owner, cost, info = ref_propagate(seeds, None, None, nid=3)
    assert info == 1 and owner.tolist() == [[1, 1, 1, 2, 2, 2]] and cost.tolist() == [[0, 3, 6, 6, 3, 0]]       # entered, as label 0
    for value in (-1, 65536):
        weight = np.zeros((1, 6), np.int32)
        weight[0, 2] = value
        owner, cost, info = ref_propagate(seeds, None, weight, nid=3)
        assert info == 3 and owner.tolist() == [[1, 1, 0, 2, 2, 2]] and cost[0, 2] == COST_INF
        weight[0, 2], weight[0, 5] = 0, value                            # under a seed: no source
        owner, cost, info = ref_propagate(seeds, None, weight, nid=10)
        assert info == 2 and owner.tolist() == [[1, 1, 9, 9, 9, 0]]
        hidden = np.ones((1, 6), np.uint8)
        hidden[0, 5] = 0
        owner, cost, info = ref_propagate(np.array([[1, 0, 0, 0, 0, 0]], np.int32), hidden, weight, nid=3)
        assert info == 0 and owner.tolist() == [[1, 1, 1, 1, 1, 0]]      # neither allowed nor a seed: the weight does not count


def test_fixtures():
    mask = serpentine((9, 12))
    seeds = np.zeros((9, 12), np.int32)
    seeds[0, 0] = 1
    owner, cost, _ = ref_propagate(seeds, mask, None, reg=1)
    assert np.array_equal(owner > 0, mask > 0) and same((owner, cost, 0), ref_propagate_sweeps(seeds, mask, None, reg=1))
    # four rows of the corridor end to end, at least 10 face steps each: far more than the 8 face steps straight down
    assert cost[0, 11] == 33 and cost[2, 11] == 37 and cost[8, 0] >= 4 * 30 and cost[8, 11] == cost[mask > 0].max() == cost[8, 0] + 31
    image = ridge_image()
    seeds = np.zeros(image.shape, np.int32)
    seeds[2, 5] = 1
    assert ref_propagate(seeds, None, image, reg=1)[1][2, 9] == 34                    # round the wall: 2 x (2 corners + 3 faces)
    assert ref_propagate(seeds, None, image, reg=100)[1][2, 9] == 12 * 100 + 400      # across it: 4 faces, up 200 and down 200
    assert dots_map((9, 9), 4, 3).max() == 4


def test_image_levels():
    from cellulus_amd.propagate import image_levels

    image = np.array([[0.0, 0.24999, 0.25, 0.5, 0.75, 0.99999, 1.0]])
    assert image_levels(image, 4).tolist() == [[0, 0, 1, 2, 3, 3, 3]] and image_levels(image, 4).dtype == np.int32
    assert image_levels(image, 2).tolist() == [[0, 0, 0, 1, 1, 1, 1]]
    assert image_levels(image * 8 - 3, 4).tolist() == [[0, 0, 1, 2, 3, 3, 3]]
    assert image_levels(image, 4, value_range=(0, 2)).tolist() == [[0, 0, 0, 1, 1, 1, 2]]
    assert image_levels(image, 4, value_range=(0.5, 0.75)).tolist() == [[0, 0, 0, 0, 3, 3, 3]]     # outside the range: the nearest level
    assert not image_levels(np.full((3, 4), 7.5), 16).any() and not image_levels(image, 4, value_range=(2, 2)).any()
    for dtype, levels in ((np.uint8, 256), (np.uint16, 65536), (np.int32, 1000)):
        whole = np.random.default_rng(3).integers(0, levels, size=(5, 6)).astype(dtype)
        assert np.array_equal(image_levels(whole, levels, value_range=(0, levels)), whole)
        assert np.array_equal(image_levels(torch.from_numpy(whole.astype(np.int64)), levels, value_range=(0, levels)), whole)
    where = np.array([[0, 1, 1, 1, 0, 0, 0]])
    assert image_levels(image, 2, where=where).tolist() == [[0, 0, 0, 1, 1, 1, 1]]                 # lo, hi = 0.24999, 0.5
    holes = image.copy()
    holes[0, 0], holes[0, 6] = math.nan, math.inf
    assert image_levels(holes, 2, where=where).tolist() == [[0, 0, 0, 1, 1, 1, 0]]                 # outside where: level 0
    with pytest.raises(ValueError, match="^image_levels: image has non-finite values under where"):
        image_levels(holes, 2)
    with pytest.raises(ValueError, match="^image_levels: image has non-finite values under where"):
        image_levels(holes, 2, where=np.array([[1, 1, 0, 0, 0, 0, 0]]))
    for levels in (1, 0, 65537, -4):
        with pytest.raises(ValueError, match="^image_levels: levels must lie in"):
            image_levels(image, levels)
    with pytest.raises(TypeError, match="^image_levels: levels must be an integer"):
        image_levels(image, 4.0)
    with pytest.raises(ValueError, match="^image_levels: where has shape"):
        image_levels(image, 4, where=np.ones((7, 1)))
    with pytest.raises(ValueError, match="^image_levels: value_range"):
        image_levels(image, 4, value_range=(1, 0))
    with pytest.raises(TypeError, match="^image_levels: image must be real"):
        image_levels(image.astype(complex), 4)


def test_propagate_columns_by_hand():
    from cellulus_amd.propagate import propagate_columns

    table = propagate_columns([2, 5], [1, 3], [4, 3], [[9, 7, 18], [0, 11, 0]], 6, (3, 5))
    assert list(table) == ["label", "seed_area", "area", "reach_cost", "reach_y", "reach_x", "cost_mean", "unreached"]
    assert table["label"].tolist() == [2, 5] and table["seed_area"].tolist() == [1, 3] and table["area"].tolist() == [4, 3]
    assert table["reach_cost"].tolist() == [9, 0] and table["reach_y"].tolist() == [1, 2] and table["reach_x"].tolist() == [2, 1]
    assert table["cost_mean"].tolist() == [4.5, 0.0] and table["unreached"].tolist() == [6, 6]
    assert all(table[k].dtype == (np.float64 if k == "cost_mean" else np.int64) for k in table)
    table = propagate_columns([1], [2], [3], [[10, 59, 10]], 0, (3, 4, 5))
    assert list(table)[4:7] == ["reach_z", "reach_y", "reach_x"] and [table[f"reach_{a}"][0] for a in "zyx"] == [2, 3, 4]
    assert table["cost_mean"][0] == 10 / 3
    none = np.zeros(0, np.int64)
    empty = propagate_columns(none, none, none, np.zeros((0, 3)), 0, (4, 5))
    assert len(empty) == 8 and all(len(c) == 0 for c in empty.values()) and empty["cost_mean"].dtype == np.float64
    # the restatement's table of a small map equals the columns fed from its maps
    seeds = dots_map((8, 9), 3, 5)
    mask = (np.random.default_rng(2).random((8, 9)) < 0.8).astype(np.uint8)
    owner, cost, _ = ref_propagate(seeds, mask)
    want = ref_propagate_table(seeds, owner, cost, mask)
    label = want["label"]
    rows = []
    for i in label:
        c = np.where(owner == i, cost, -1)
        rows.append([c.max(), int(np.argmax(c.reshape(-1))), int(cost[owner == i].sum())])
    got = propagate_columns(label, [(seeds == i).sum() for i in label], [(owner == i).sum() for i in label], rows,
                            ((mask != 0) & (owner == 0)).sum(), seeds.shape)
    assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)
    with pytest.raises(ValueError, match="^propagate_columns: shape must have 2 or 3"):
        propagate_columns(none, none, none, np.zeros((0, 3)), 0, (20,))
    with pytest.raises(ValueError, match="^propagate_columns: needs increasing labels"):
        propagate_columns([1], [3], [2], [[0, 0, 0]], 0, (4, 5))
    with pytest.raises(ValueError, match="^propagate_columns: a row of the reach"):
        propagate_columns([1], [1], [2], [[3, 20, 3]], 0, (4, 5))
    with pytest.raises(ValueError, match="^propagate_columns: seed_area, area and rows"):
        propagate_columns([1, 2], [1], [2], [[3, 2, 3]], 0, (4, 5))
    with pytest.raises(ValueError, match="^propagate_columns: unreached"):
        propagate_columns([1], [1], [2], [[3, 2, 3]], -1, (4, 5))


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    raw = open(os.path.join(ROOT, "include", "clx.h")).read()
    assert re.search(r"#define\s+CLX_COST_INF\s+CLX_DIST_INF", raw)
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, kind, restype, nargs in (("clx_label_propagate", "int", ctypes.c_int, 18),
                                       ("clx_label_propagate_workspace", "size_t", ctypes.c_size_t, 4)):
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs and _clx.PROTOTYPES[name][0] is restype
    lib = _clx.load()
    assert lib.clx_abi_version() == 13
    size = lib.clx_label_propagate_workspace
    for bad in ((1, 1, 8, 8), (4, 1, 8, 8), (2, 2, 8, 8), (2, 1, 0, 8), (3, 0, 8, 8), (2, 1, 8, -1), (2, 1, 65536, 65536), (3, 2, 46341, 46341)):
        assert size(*bad) == 0, bad
    head = 4 * (16 + 64)
    assert size(2, 1, 1, 1) == head + 8 + 2 * 4 and size(2, 1, 16, 64) == head + 8 * 1024 + 2 * 4
    assert size(2, 1, 17, 65) == head + 8 * 17 * 65 + 2 * 4 and size(2, 1, 33, 129) == head + 8 * 33 * 129 + 2 * 12
    assert size(3, 8, 8, 16) == head + 8 * 1024 + 2 * 4 and size(3, 9, 9, 17) == head + 8 * 9 * 9 * 17 + 2 * 8
    assert size(2, 1, 65535, 65537) == head + 8 * (2 ** 32 - 1) + 2 * 4096 * 1025         # 2^32 - 1 pixels


def test_entry_point_refuses_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def propagate(nd=2, Z=1, Y=8, X=8, nid=4, reg=1, limit=-1, rounds=8, resume=0, nbytes=2 ** 20, **ptrs):
        p = dict(seeds=some, mask=some, weight=some, owner=some, cost=some, info=some, workspace=some)
        p.update(ptrs)
        return lib.clx_label_propagate(p["seeds"], p["mask"], p["weight"], nd, Z, Y, X, nid, reg, limit, rounds, resume, p["owner"], p["cost"],
                                       p["info"], p["workspace"], nbytes, null)

    exact = int(lib.clx_label_propagate_workspace(2, 1, 8, 8))
    refused = [({k: null}, "null pointer") for k in ("seeds", "owner", "cost", "info", "workspace")]
    refused += [(dict(nd=1), "nd"), (dict(nd=4), "nd"), (dict(Z=2), "Z == 1"), (dict(Y=0), "shape"), (dict(X=-1), "shape"), (dict(nd=3, Z=0), "shape"),
                (dict(Y=65536, X=65536, nbytes=2 ** 40), "Z * Y * X"), (dict(nd=3, Z=2, Y=46341, X=46341, nbytes=2 ** 40), "Z * Y * X"),
                (dict(nid=0), "nid"), (dict(nid=2 ** 24 + 1), "nid"), (dict(reg=-1), "reg"), (dict(reg=65536), "reg"),
                (dict(limit=-2), "limit"), (dict(limit=2 ** 30), "limit"), (dict(rounds=0), "rounds"), (dict(rounds=65), "rounds"),
                (dict(rounds=-3), "rounds"), (dict(resume=2), "resume"), (dict(resume=-1), "resume"),
                (dict(nbytes=exact - 1), "workspace_bytes"), (dict(nbytes=0), "workspace_bytes"),
                (dict(workspace=ctypes.c_void_p(4098)), "aligned"), (dict(workspace=ctypes.c_void_p(4097)), "aligned")]
    for kw, word in refused:
        assert propagate(**kw) == -1, f"clx_label_propagate{kw} was not refused"
        message = lib.clx_last_error().decode()
        assert message.startswith("clx_label_propagate:") and word in message, f"{kw}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="clx_label_propagate.*rounds"):
        _clx.call("clx_label_propagate", some, null, null, 2, 1, 8, 8, 4, 1, -1, 100, 0, some, some, some, some, 2 ** 20, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import propagate as propagate_cli

    text = CliRunner().invoke(propagate_cli, ["--help"]).output
    assert all(option in text for option in ("--seeds", "--output", "--mask", "--channel", "--levels", "--regularisation", "--limit"))
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(propagate_cli, [__file__, "--seeds", "nuclei", "--output", "cells", "--mask", "fg", "--channel", "0", "--levels", "64",
                                                "--regularisation", "2", "--limit", "300"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output
    result = CliRunner().invoke(propagate_cli, [__file__, "--seeds", "nuclei"])
    assert result.exit_code == 2 and "--output" in result.output
    for option, value in (("--levels", "1"), ("--regularisation", "-1"), ("--regularisation", "65536"), ("--limit", "-1"), ("--channel", "-1")):
        result = CliRunner().invoke(propagate_cli, [__file__, "--seeds", "nuclei", "--output", "cells", option, value])
        assert result.exit_code == 2 and option in result.output
    text = open(os.path.join(ROOT, "cellulus_amd", "propagate.py")).read()
    assert 'from .cli import propagate as _command' in text


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.propagate import geodesic_owner, propagate_labels, propagate_stage, propagate_table

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    monkeypatch.setattr(_clx, "load", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for f, who in ((geodesic_owner, "geodesic_owner"), (propagate_labels, "propagate_labels"), (propagate_table, "propagate_table")):
        for floats in (good.astype(np.float32), torch.ones(4, 5), good.astype(bool), torch.ones(4, 5, dtype=torch.bool)):
            with pytest.raises(TypeError, match=f"^{who}: labels must be integers"):
                f(floats, device=fake)
        for shape in ((20,), (1, 1, 4, 5)):
            with pytest.raises(ValueError, match=f"^{who}: labels must be 2-D or 3-D"):
                f(np.ones(shape, np.int32), device=fake)
        with pytest.raises(TypeError, match=f"^{who}: labels must be an array or a tensor"):
            f([[1, 2]], device=fake)
        with pytest.raises(ValueError, match=f"^{who}: label ids must lie in"):
            f(good - 2, device=fake)
        with pytest.raises(ValueError, match=f"^{who}: mask has shape"):
            f(good, mask=np.ones((5, 4)), device=fake)
        with pytest.raises(TypeError, match=f"^{who}: mask must be an array or a tensor"):
            f(good, mask=[[1]], device=fake)
        for bad, kind in ((-1, ValueError), (65536, ValueError), (1.0, TypeError), (None, TypeError), (True, TypeError), ("1", TypeError)):
            with pytest.raises(kind, match=f"^{who}: regularisation must"):
                f(good, regularisation=bad, device=fake)
        for bad, kind in ((-1, ValueError), (2 ** 30, ValueError), (7.5, TypeError), (False, TypeError)):
            with pytest.raises(kind, match=f"^{who}: limit must"):
                f(good, limit=bad, device=fake)
    with pytest.raises(ValueError, match="^geodesic_owner: weight has shape"):
        geodesic_owner(good, weight=np.ones((5, 4), np.int32), device=fake)
    with pytest.raises(TypeError, match="^geodesic_owner: weight must be integers"):
        geodesic_owner(good, weight=np.ones((4, 5)), device=fake)
    for value in (-1, 65536):
        with pytest.raises(ValueError, match="^geodesic_owner: weight must lie in"):
            geodesic_owner(good, weight=np.full((4, 5), value, np.int64), device=fake)
    with pytest.raises(ValueError, match="^propagate_labels: image has shape"):
        propagate_labels(good, image=np.ones((5, 4)), device=fake)
    with pytest.raises(ValueError, match="^image_levels: image has non-finite"):
        propagate_labels(good, image=np.full((4, 5), np.nan), device=fake)
    with pytest.raises(ValueError, match="^image_levels: levels must lie in"):
        propagate_table(good, image=np.ones((4, 5)), levels=1, device=fake)
    for kw in (dict(seeds="", output="cells"), dict(seeds=None, output="cells"), dict(seeds="nuclei", output="nuclei"),
               dict(seeds="nuclei", output=""), dict(seeds="nuclei", output=None), dict(seeds="nuclei", output="fg", mask="fg"),
               dict(seeds="nuclei", output="cells", mask=""), dict(seeds="nuclei", output="cells", channel=-1),
               dict(seeds="nuclei", output="cells", levels=1), dict(seeds="nuclei", output="cells", regularisation=-1),
               dict(seeds="nuclei", output="cells", limit=2 ** 30)):
        with pytest.raises(ValueError, match="^propagate_stage: "):
            propagate_stage(None, **kw)
    with pytest.raises(TypeError, match="^propagate_stage: limit must be"):
        propagate_stage(None, "nuclei", "cells", limit=1.5)


def test_cpu_device_raises():
    from cellulus_amd._clx import ClxError
    from cellulus_amd.propagate import geodesic_owner, propagate_labels, propagate_table

    seeds = np.ones((4, 5), np.int32)
    for call in (lambda: geodesic_owner(seeds, device="cpu"), lambda: propagate_labels(seeds, device=torch.device("cpu")),
                 lambda: propagate_table(seeds, device="cpu")):
        with pytest.raises(ClxError, match="no CPU path"):
            call()
