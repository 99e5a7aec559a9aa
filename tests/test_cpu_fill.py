"""The fill stage without a device: the restatement of tests/fill_ref.py against scipy's binary_fill_holes (the subset relation
on random maps, equality on isolated objects), planewise against the 2-D restatement slice by slice, the maps worked by hand,
hole_columns and fill_columns by hand, the symbols of the library, and every refusal that needs no device."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from fill_ref import (HAND, comb_hole, discs_map, hand_result, random_map, ref_fill_table, ref_hole_table, ref_holes, serpentine_hole,
                      spiral_hole)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_fill(labels):
    """the union over L of binary_fill_holes(labels == L) & (labels == 0)"""
    filled = np.zeros(labels.shape, bool)
    for i in np.unique(labels[labels != 0]):
        filled |= ndimage.binary_fill_holes(labels == i) & (labels == 0)
    return filled


def test_filled_pixels_are_a_subset_of_scipys():
    strict = 0
    for seed in range(60):
        shape = [(23, 31), (40, 17), (7, 13, 18), (9, 9, 9)][seed % 4]
        labels = random_map(shape, seed, block=[4, 5, 3][seed % 3], knock=[0.2, 0.1, 0.3][seed % 3])
        out, rows, info = ref_holes(labels)
        ours, theirs = (out != 0) & (labels == 0), scipy_fill(labels)
        assert not (ours & ~theirs).any(), seed
        assert np.array_equal(out[labels != 0], labels[labels != 0]) and info[1] == ours.sum() == rows[:, 2].sum()
        strict += bool((theirs & ~ours).any())
    assert strict > 0                                                    # nested labels and gaps between two occur


def test_equal_to_scipy_on_isolated_objects():
    holes = 0
    for seed in range(12):
        labels = discs_map([(48, 56), (9, 40, 44)][seed % 2], seed)
        out, rows, info = ref_holes(labels)
        assert np.array_equal((out != 0) & (labels == 0), scipy_fill(labels)), seed
        assert info[0] == len(rows) > 10 and not rows[:, 3].any()
        holes += len(rows)
    assert holes > 500


def test_planewise_is_the_2d_restatement_slice_by_slice():
    for seed in range(8):
        labels = random_map((5, 19, 23), 100 + seed, block=3)
        for max_size in (None, 2):
            out, rows, info = ref_holes(labels, max_size, planewise=True)
            slices = [ref_holes(labels[z], max_size) for z in range(labels.shape[0])]
            assert np.array_equal(out, np.stack([s[0] for s in slices]))
            stacked = np.concatenate([s[1] + [z * 19 * 23, 0, 0, 0] for z, s in enumerate(slices)])
            assert np.array_equal(rows, stacked) and info == [sum(s[2][k] for s in slices) for k in range(4)]
    deep = random_map((6, 12, 12), 7, block=3)
    assert ref_holes(deep)[2] != ref_holes(deep, planewise=True)[2]


@pytest.mark.parametrize("name", sorted(HAND))
def test_maps_worked_by_hand(name):
    labels, planewise, out, rows, info = hand_result(name)
    got = ref_holes(labels, planewise=planewise)
    assert np.array_equal(got[0], out) and got[0].dtype == np.int32
    assert np.array_equal(got[1], rows) and got[2] == info


def test_size_cap_by_hand():
    labels, _, out, rows, info = hand_result("one_side_each")            # one hole of 3 pixels
    for max_size, kept in ((2, 1), (3, 0), (4, 0), (0, 1), (None, 0), (-1, 0)):
        got = ref_holes(labels, max_size)
        assert np.array_equal(got[0], labels if kept else out)
        assert got[1].tolist() == [[24, 1, 3, kept]] and got[2] == [1, 0 if kept else 3, 6, 0]


def test_long_chains_are_one_hole():
    for m in (serpentine_hole(), comb_hole(), spiral_hole()):
        out, rows, info = ref_holes(m)
        assert (out == 1).all() and rows.tolist() == [[int(np.flatnonzero(m == 0)[0]), 1, int((m == 0).sum()), 0]] and info[2] == 1
    assert (serpentine_hole() == 0).sum() == 10 * 148 + 9 and (spiral_hole(41) == 0).sum() > 400


def test_tables_of_the_restatement():
    labels, _, _, _, _ = hand_result("one_side_each")
    holes = ref_hole_table(labels, 2)
    assert list(holes) == ["owner", "first_y", "first_x", "area", "filled"] and [c.tolist() for c in holes.values()] == [[1], [3], [3], [3], [0]]
    table = ref_fill_table(labels, 2)
    assert [table[k].tolist() for k in table] == [[1], [36], [36], [0], [0], [3], [1]]
    table = ref_fill_table(labels)
    assert [table[k].tolist() for k in table] == [[1], [36], [39], [1], [3], [3], [0]]
    assert list(ref_hole_table(hand_result("cavity")[0]))[1:4] == ["first_z", "first_y", "first_x"]


def test_columns_by_hand():
    from cellulus_amd.fill import fill_columns, hole_columns

    holes = hole_columns([24, 7], [1, 9], [3, 1], [1, 0], (7, 7))
    assert list(holes) == ["owner", "first_y", "first_x", "area", "filled"]
    assert [c.tolist() for c in holes.values()] == [[1, 9], [3, 1], [3, 0], [3, 1], [0, 1]] and all(c.dtype == np.int64 for c in holes.values())
    deep = hole_columns([62], [4], [2], [0], (5, 5, 5))
    assert [deep[f"first_{a}"][0] for a in "zyx"] == [2, 2, 2] and len(deep) == 6
    empty = hole_columns([], [], [], [], (4, 5))
    assert len(empty) == 5 and all(len(c) == 0 and c.dtype == np.int64 for c in empty.values())
    table = fill_columns([2, 5, 9], [10, 20, 30], [5, 9, 5, 5], [4, 1, 7, 2], [0, 0, 1, 0])
    assert list(table) == ["label", "area_before", "area", "holes_filled", "filled_area", "largest_hole", "holes_kept"]
    assert [c.tolist() for c in table.values()] == [[2, 5, 9], [10, 20, 30], [10, 26, 31], [0, 2, 1], [0, 6, 1], [0, 7, 1], [0, 1, 0]]
    assert all(c.dtype == np.int64 for c in table.values())
    none = np.zeros(0, np.int64)
    assert all(len(c) == 0 for c in fill_columns(none, none, none, none, none).values())
    # the restatement's tables of a random map equal the columns fed from its rows
    labels = random_map((30, 41), 3)
    for max_size in (None, 1):
        rows = ref_holes(labels, max_size)[1]
        want = ref_fill_table(labels, max_size)
        got = fill_columns(want["label"], want["area_before"], rows[:, 1], rows[:, 2], rows[:, 3])
        assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)
        want = ref_hole_table(labels, max_size)
        got = hole_columns(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], labels.shape)
        assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want) and len(rows) > 3
    with pytest.raises(ValueError, match="^hole_columns: shape must have 2 or 3"):
        hole_columns([], [], [], [], (20,))
    with pytest.raises(ValueError, match="^hole_columns: first, owner, area and kept"):
        hole_columns([1, 2], [1], [1], [0], (4, 5))
    for bad in (([20], [1], [1], [0]), ([3], [0], [1], [0]), ([3], [1], [0], [0]), ([3], [1], [1], [2])):
        with pytest.raises(ValueError, match="^hole_columns: needs first pixels"):
            hole_columns(*bad, (4, 5))
    with pytest.raises(ValueError, match="^fill_columns: needs increasing labels"):
        fill_columns([2, 2], [1, 1], [], [], [])
    with pytest.raises(ValueError, match="^fill_columns: a hole needs an owner"):
        fill_columns([2, 5], [1, 1], [3], [1], [0])
    with pytest.raises(ValueError, match="^fill_columns: label and area_before"):
        fill_columns([2, 5], [1], [], [], [])


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    raw = open(os.path.join(ROOT, "include", "clx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, kind, restype, nargs in (("clx_label_holes", "int", ctypes.c_int, 14), ("clx_label_holes_workspace", "size_t", ctypes.c_size_t, 4)):
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs and _clx.PROTOTYPES[name][0] is restype
    lib = _clx.load()
    assert lib.clx_abi_version() == 13
    size = lib.clx_label_holes_workspace
    for bad in ((1, 1, 8, 8), (4, 1, 8, 8), (2, 2, 8, 8), (2, 1, 0, 8), (3, 0, 8, 8), (2, 1, 8, -1), (2, 1, 32768, 65536), (3, 2, 32768, 32768)):
        assert size(*bad) == 0, bad
    assert size(2, 1, 1, 1) == 16 and size(2, 1, 17, 65) == 16 * 17 * 65 and size(3, 9, 9, 17) == 16 * 9 * 9 * 17
    assert size(2, 1, 32768, 65535) == 16 * 32768 * 65535                 # 2^31 - 32768 pixels
    # the definitions stand word for word in the header and in the design document
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.3p" in design
    for phrase in ("surrounded by a single object", "REACHES THE BORDER", "FACE neighbours"):
        assert phrase in raw and phrase in design, phrase


def test_entry_point_refuses_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, other, null = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(0)

    def holes(nd=2, Z=1, Y=8, X=8, planewise=0, max_size=-1, capacity=4, nbytes=2 ** 20, **ptrs):
        p = dict(labels=some, out=other, holes=some, info=some, workspace=some)
        p.update(ptrs)
        return lib.clx_label_holes(p["labels"], nd, Z, Y, X, planewise, max_size, capacity, p["out"], p["holes"], p["info"], p["workspace"],
                                   nbytes, null)

    exact = int(lib.clx_label_holes_workspace(2, 1, 8, 8))
    refused = [({k: null}, "null pointer") for k in ("labels", "out", "info", "workspace")]
    refused += [(dict(holes=null), "null holes"), (dict(nd=1), "nd"), (dict(nd=4), "nd"), (dict(Z=2), "Z == 1"), (dict(Y=0), "shape"),
                (dict(X=-1), "shape"), (dict(nd=3, Z=0), "shape"), (dict(planewise=1), "planewise"), (dict(planewise=2, nd=3), "planewise"),
                (dict(planewise=-1), "planewise"), (dict(Y=32768, X=65536, nbytes=2 ** 40), "Z * Y * X"),
                (dict(nd=3, Z=2, Y=32768, X=32768, nbytes=2 ** 40), "Z * Y * X"), (dict(max_size=-2), "max_size"), (dict(capacity=-1), "capacity"),
                (dict(nbytes=exact - 1), "workspace_bytes"), (dict(nbytes=0), "workspace_bytes"),
                (dict(workspace=ctypes.c_void_p(4098)), "aligned"), (dict(workspace=ctypes.c_void_p(4097)), "aligned"),
                (dict(out=some), "in-place")]
    for kw, word in refused:
        assert holes(**kw) == -1, f"clx_label_holes{kw} was not refused"
        message = lib.clx_last_error().decode()
        assert message.startswith("clx_label_holes:") and word in message, f"{kw}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="clx_label_holes.*max_size"):
        _clx.call("clx_label_holes", some, 2, 1, 8, 8, 0, -5, 0, other, null, some, some, 2 ** 20, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import fill as fill_cli

    text = CliRunner().invoke(fill_cli, ["--help"]).output
    assert all(option in text for option in ("--source", "--output", "--max-size", "--planewise"))
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(fill_cli, [__file__, "--source", "cells", "--output", "solid", "--max-size", "30", "--planewise"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output
    result = CliRunner().invoke(fill_cli, [__file__, "--source", "cells"])
    assert result.exit_code == 2 and "--output" in result.output
    result = CliRunner().invoke(fill_cli, [__file__, "--source", "cells", "--output", "solid", "--max-size", "-1"])
    assert result.exit_code == 2 and "--max-size" in result.output
    assert 'from .cli import fill as _command' in open(os.path.join(ROOT, "cellulus_amd", "fill.py")).read()


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.fill import fill_holes, fill_stage, fill_table, hole_table

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    monkeypatch.setattr(_clx, "load", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for f, who in ((fill_holes, "fill_holes"), (hole_table, "hole_table"), (fill_table, "fill_table")):
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
        with pytest.raises(ValueError, match=f"^{who}: label ids must lie in"):
            f(good.astype(np.int64) << 24, device=fake)
        for bad, kind in ((-1, ValueError), (2 ** 63, ValueError), (1.0, TypeError), (True, TypeError), ("1", TypeError)):
            with pytest.raises(kind, match=f"^{who}: max_size must"):
                f(good, max_size=bad, device=fake)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(TypeError, match=f"^{who}: planewise must be a bool"):
                f(good, planewise=bad, device=fake)
        with pytest.raises(ValueError, match=f"^{who}: planewise needs a 3-D map"):
            f(good, planewise=True, device=fake)
    for kw in (dict(source="", output="solid"), dict(source=None, output="solid"), dict(source="cells", output="cells"),
               dict(source="cells", output=""), dict(source="cells", output=None), dict(source="cells", output="solid", max_size=-1)):
        with pytest.raises(ValueError, match="^fill_stage: "):
            fill_stage(None, **kw)
    with pytest.raises(TypeError, match="^fill_stage: max_size must be"):
        fill_stage(None, "cells", "solid", max_size=1.5)
    with pytest.raises(TypeError, match="^fill_stage: planewise must be"):
        fill_stage(None, "cells", "solid", planewise=1)


def test_cpu_device_raises():
    from cellulus_amd._clx import ClxError
    from cellulus_amd.fill import fill_holes, fill_table, hole_table

    labels = np.ones((4, 5), np.int32)
    for call in (lambda: fill_holes(labels, device="cpu"), lambda: hole_table(labels, device=torch.device("cpu")),
                 lambda: fill_table(labels, device="cpu")):
        with pytest.raises(ClxError, match="no CPU path"):
            call()
