"""The split stage without a device: the two forms of the restatement (tests/split_ref.py) against each other, the properties
of the definitions on discs, ellipses, balls and blob maps, merge_basins and its exact depth test against the restatement's
bracketed square roots, merge_basins and split_columns by hand, and the plumbing (declarations, prototypes, refusals of the
entry points and of the host functions before any device, the command's options)."""

import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy import ndimage

from cellulus_amd.split import basin_passes, basins, merge_basins, shallower, split_columns, split_labels, split_stage, split_table
from inscribed_ref import DIST_INF, ref_distance_sq
from split_ref import (DEPTHS, coarsens, disc, ellipse, loops_basins, loops_passes, noise_blobs, passes_of, ref_basins, ref_merge,
                       ref_passes, ref_shallower, ref_split, same_partition, serpentine, two_balls, two_discs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELLIPSES = {"16x5": ellipse((25, 25), (12, 12), 16, 5, 0.4), "18x6": ellipse((25, 25), (12, 12), 18, 6, 1.1)}


def pieces(labels, depth):
    return len(ref_split(labels, depth)[1]["label"])


def integer_maps(shape, seed, labels=3, top=6):
    """a random label map with a random `distance` map, as the ABI admits it: many basins on a tiny image, many ties"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, labels + 1, size=shape).astype(np.int32), rng.integers(0, top, size=shape).astype(np.int32)


SMALL = {"ellipse": lambda: (ELLIPSES["18x6"], None), "discs": lambda: (two_discs(11), None), "balls": lambda: (two_balls(9), None),
         "blobs": lambda: (noise_blobs(3, (30, 41), 2.0), None), "serpentine": lambda: (serpentine(13), None),
         "integers_2d": lambda: integer_maps((9, 11), 1), "integers_3d": lambda: integer_maps((3, 5, 6), 2, top=3),
         "flat": lambda: (np.ones((4, 7), np.int32), np.full((4, 7), 5, np.int32))}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_loops_equal_shifted_views(name):
    labels, dist = SMALL[name]()
    if dist is None:
        dist = ref_distance_sq(labels, False)
    else:
        dist.flat[5], dist.flat[-3] = -1, DIST_INF + 1          # out of range: no object pixel there, and reported
    want_root, want_summits, want_info = loops_basins(labels, dist)
    root, summits, info = ref_basins(labels, dist)
    assert np.array_equal(root, want_root) and np.array_equal(summits, want_summits) and info == want_info
    want = passes_of(loops_passes(labels, dist, want_root))
    got = ref_passes(labels, dist, root)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    flat = root.reshape(-1)
    assert np.array_equal(flat[summits], summits) and np.array_equal(np.unique(flat[flat >= 0]), summits)
    assert ((flat >= 0) == ((labels.reshape(-1) != 0) & (dist.reshape(-1) >= 0) & (dist.reshape(-1) <= DIST_INF))).all()
    d = dist.reshape(-1)
    assert (got[2] <= np.minimum(d[got[0]], d[got[1]])).all()


def test_single_shapes():
    whole = disc((23, 23), (11, 11), 9)
    assert ref_split(whole, 0)[2] == 1 and all(pieces(whole, d) == 1 for d in DEPTHS)
    for name, summits in (("16x5", 4), ("18x6", 5)):
        assert ref_split(ELLIPSES[name], 0)[2] == summits == pieces(ELLIPSES[name], 0)
        assert all(pieces(ELLIPSES[name], d) == 1 for d in DEPTHS if d >= Fraction(1, 2))


def test_two_discs_and_two_balls():
    near, far, merged = two_discs(11), two_discs(14), two_discs(6)
    assert all(pieces(near, d) == 2 for d in DEPTHS if d <= Fraction(3, 2)) and pieces(near, 2) == 1
    assert all(pieces(far, d) == 2 for d in DEPTHS if d <= 3) and pieces(far, 1000) == 1
    assert all(pieces(merged, d) == 1 for d in DEPTHS if d >= 1)
    new = ref_split(near, 1)[0]
    assert new[10, 4] == 1 and new[10, 27] == 2 and set(np.unique(new)) == {0, 1, 2}        # numbered by the summits' raster index
    balls = two_balls(9)
    assert all(pieces(balls, d) == 2 for d in DEPTHS if d <= 1) and pieces(balls, 2) == 1


@pytest.mark.parametrize("seed", range(12))
def test_blob_maps(seed):
    labels = noise_blobs(seed)
    full = np.ones((3, 3), dtype=bool)
    dist = ref_distance_sq(labels, False)
    root, summits, _ = ref_basins(labels, dist)
    a, b, height = ref_passes(labels, dist, root)
    flat_d, flat_lab = dist.reshape(-1), labels.reshape(-1)
    assert (height <= np.minimum(flat_d[a], flat_d[b])).all() and (height >= 1).all() and len(summits) > labels.max()
    components = sum(ndimage.label(labels == v, structure=full)[1] for v in range(1, labels.max() + 1))
    before = None
    for depth in DEPTHS:
        new, table, nsummits = ref_split(labels, depth)
        n = len(table["label"])
        assert np.array_equal(new > 0, labels > 0) and nsummits == len(summits)
        for i in range(1, n + 1):                                # every piece is 8-connected and lies in one object
            assert ndimage.label(new == i, structure=full)[1] == 1 and len(np.unique(labels[new == i])) == 1
        assert before is None or coarsens(new, before)
        before = new
        # the product's merge gives the restatement's pieces
        piece, rows = merge_basins(flat_lab[summits], flat_d[summits], summits, np.stack([a, b, height], axis=1), depth)
        want_piece, want_rows = ref_merge(summits, flat_lab[summits], flat_d[summits], (a, b, height), depth)
        assert piece.tolist() == [want_piece[int(s)] for s in summits]
        assert [tuple(int(rows[k][i]) for k in ("parent", "top", "top_d2", "pass_d2")) for i in range(n)] == \
               [(r[0], r[1], r[2], -1 if r[3] is None else r[3]) for r in want_rows]
        if depth == 0:
            assert n == len(summits)
        if depth == 1000:
            assert n == components


def test_depth_test_is_exact():
    depths = [Fraction(0), Fraction(1, 4), Fraction(1), Fraction(3, 2), Fraction(2), Fraction(7, 3), Fraction(math.sqrt(2)), Fraction(1000)]
    for a in range(0, 70):
        for b in range(0, a + 1):
            for depth in depths:
                assert shallower(a, b, depth) == ref_shallower(a, b, depth), (a, b, depth)
    # ties do not merge
    assert not shallower(25, 9, Fraction(2)) and shallower(25, 9, Fraction(2) + Fraction(1, 10 ** 30))
    assert not shallower(49, 49, Fraction(0)) and shallower(49, 49, Fraction(1, 10 ** 30)) and not shallower(2, 1, Fraction(0))
    # where a float of the difference rounds to the depth: sqrt(2^30) - sqrt(2^30 - 1) = 2^-16 + 2^-48 + ...
    tiny = Fraction(1, 2 ** 16)
    assert not shallower(2 ** 30, 2 ** 30 - 1, tiny) and shallower(2 ** 30, 2 ** 30 - 1, tiny + Fraction(1, 2 ** 47))
    assert ref_shallower(2 ** 30, 2 ** 30 - 1, tiny) is False and ref_shallower(2 ** 30, 2 ** 30 - 1, tiny + Fraction(1, 2 ** 47)) is True
    assert math.sqrt(2 ** 30) - math.sqrt(2 ** 30 - 1) == float(tiny)          # the rounded difference cannot tell
    # a float depth is taken exactly as the binary fraction it is
    from cellulus_amd.split import _depth
    assert _depth(0.1, "test") == Fraction(0.1) > Fraction(1, 10) and _depth(np.float32(0.1), "test") == Fraction(float(np.float32(0.1)))
    assert shallower(121, 100, _depth(1.0 + 1e-15, "test")) and not shallower(121, 100, _depth(1.0, "test"))
    with pytest.raises(ValueError, match="^shallower: needs"):
        shallower(4, 9, Fraction(1))


def test_merge_and_columns_by_hand_on_a_chain():
    # three basins in a row under label 7: A (index 12, D 100), B (index 40, D 36), C (index 90, D 100); passes A-B 25, B-C 25
    summits, labels, d2 = [12, 40, 90], [7, 7, 7], [100, 36, 100]
    passes = [[12, 40, 25], [40, 90, 25]]
    # depth 1: sqrt 36 - sqrt 25 = 1 is not below it: nothing merges
    piece, rows = merge_basins(labels, d2, summits, passes, 1)
    assert piece.tolist() == [1, 2, 3] and rows["top"].tolist() == [12, 40, 90] and rows["pass_d2"].tolist() == [25, 25, 25]
    # depth 3/2: B merges, and among the equal passes (12, 40) comes before (40, 90): into A.  Then {A, B} against C: C's top
    # has the larger index, so it is the lower one, and sqrt 100 - sqrt 25 = 5 refuses
    for given in (passes, passes[::-1]):                          # the order of the rows given does not matter
        piece, rows = merge_basins(labels, d2, summits, given, Fraction(3, 2))
        assert piece.tolist() == [1, 1, 2] and rows["top"].tolist() == [12, 90] and rows["top_d2"].tolist() == [100, 100]
        assert rows["parent"].tolist() == [7, 7] and rows["pass_d2"].tolist() == [25, 25]
    # with the equal passes swapped in index order B goes the other way
    piece, _ = merge_basins(labels, d2, [12, 40, 90], [[12, 90, 1], [40, 90, 25], [12, 40, 24]], Fraction(3, 2))
    assert piece.tolist() == [1, 2, 2]
    # depth 6 merges everything into A, the smaller index among the equal tops
    piece, rows = merge_basins(labels, d2, summits, passes, 6)
    assert piece.tolist() == [1, 1, 1] and rows["top"].tolist() == [12] and rows["pass_d2"].tolist() == [-1]
    # pieces are numbered by (label, raster index of the top), whatever the heights
    piece, rows = merge_basins([9, 2, 9, 2], [4, 9, 16, 1], [3, 5, 8, 20], [[3, 8, 4], [5, 20, 1]], 0)
    assert piece.tolist() == [3, 1, 4, 2] and rows["parent"].tolist() == [2, 2, 9, 9] and rows["top"].tolist() == [5, 20, 3, 8]
    assert rows["pass_d2"].tolist() == [1, 1, 4, 4]

    piece, rows = merge_basins(labels, d2, summits, passes, Fraction(3, 2))
    table = split_columns(rows["parent"], rows["top"], rows["top_d2"], rows["pass_d2"], [30, 20], (10, 10))
    assert list(table) == ["label", "parent", "summit_y", "summit_x", "summit_radius", "pass_radius", "pieces_of_parent", "area"]
    assert table["label"].tolist() == [1, 2] and table["parent"].tolist() == [7, 7] and table["summit_y"].tolist() == [1, 9]
    assert table["summit_x"].tolist() == [2, 0] and table["summit_radius"].tolist() == [10.0, 10.0]
    assert table["pass_radius"].tolist() == [5.0, 5.0] and table["pieces_of_parent"].tolist() == [2, 2] and table["area"].tolist() == [30, 20]
    assert all(table[k].dtype == (np.float64 if k.endswith("radius") else np.int64) for k in table)
    table = split_columns([7, 8], [12, 90], [2, 3], [-1, 2], [5, 6], (2, 5, 10))
    assert list(table)[2:5] == ["summit_z", "summit_y", "summit_x"] and table["summit_z"].tolist() == [0, 1]
    assert table["summit_radius"].tolist() == [math.sqrt(2), math.sqrt(3)] and math.isnan(table["pass_radius"][0])
    assert table["pass_radius"][1] == math.sqrt(2) and table["pieces_of_parent"].tolist() == [1, 1]
    none = np.zeros(0, np.int64)
    empty = split_columns(none, none, none, none, none, (4, 5))
    assert len(empty) == 8 and all(len(c) == 0 for c in empty.values()) and empty["summit_radius"].dtype == np.float64
    with pytest.raises(ValueError, match="^split_columns: shape must have 2 or 3"):
        split_columns(none, none, none, none, none, (20,))
    with pytest.raises(ValueError, match="^split_columns: needs tops inside"):
        split_columns([1], [100], [4], [-1], [3], (10, 10))
    with pytest.raises(ValueError, match="^merge_basins: a pass needs"):
        merge_basins(labels, d2, summits, [[12, 41, 25]], 1)
    with pytest.raises(ValueError, match="^merge_basins: a pass needs"):
        merge_basins([7, 8, 7], d2, summits, [[12, 40, 25]], 1)
    with pytest.raises(ValueError, match="^merge_basins: a pass needs"):
        merge_basins(labels, d2, summits, [[12, 40, 37]], 1)
    with pytest.raises(ValueError, match="^merge_basins: needs increasing summits"):
        merge_basins(labels, d2, [12, 90, 40], [], 1)


def test_restated_table_on_the_two_discs():
    new, table, nsummits = ref_split(two_discs(11), 1)
    assert nsummits == 2 and table["label"].tolist() == [1, 2] and table["parent"].tolist() == [1, 1]
    assert table["summit_y"].tolist() == [10, 10] and table["summit_x"].tolist() == [10, 21] and table["pieces_of_parent"].tolist() == [2, 2]
    assert table["area"].sum() == (new > 0).sum() and (table["summit_radius"] > table["pass_radius"]).all()
    whole = ref_split(two_discs(11), 2)[1]
    assert whole["label"].tolist() == [1] and math.isnan(whole["pass_radius"][0]) and whole["area"].tolist() == [int((new > 0).sum())]
    assert same_partition(ref_split(two_discs(11), 2)[0], two_discs(11))


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, kind, restype, nargs in (("clx_label_basins", "int", ctypes.c_int, 13), ("clx_basin_passes", "int", ctypes.c_int, 12),
                                       ("clx_basin_relabel", "int", ctypes.c_int, 10),
                                       ("clx_label_basins_workspace", "size_t", ctypes.c_size_t, 1)):
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs and _clx.PROTOTYPES[name][0] is restype
    lib = _clx.load()
    assert lib.clx_abi_version() == 13
    assert lib.clx_label_basins_workspace(0) == 0 and lib.clx_label_basins_workspace(2 ** 32) == 0 and lib.clx_label_basins_workspace(-5) == 0
    assert lib.clx_label_basins_workspace(1) == 64 + 4 and lib.clx_label_basins_workspace(2 ** 32 - 1) == 64 + 4 * (2 ** 32 - 1)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """the checks come before any launch and no pointer is followed: they run without a device"""
    from cellulus_amd import _clx

    lib = _clx.load()
    some, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def label_basins(nd=2, Z=1, Y=8, X=8, capacity=16, nbytes=None, **ptrs):
        p = dict(labels=some, dist_sq=some, root=some, summits=some, info=some, workspace=some)
        p.update(ptrs)
        nbytes = 64 + 4 * Z * Y * X if nbytes is None else nbytes
        return lib.clx_label_basins(p["labels"], p["dist_sq"], nd, Z, Y, X, capacity, p["root"], p["summits"], p["info"], p["workspace"],
                                    nbytes, null)

    def basin_passes_(nd=2, Z=1, Y=8, X=8, capacity=1024, **ptrs):
        p = dict(labels=some, dist_sq=some, root=some, keys=some, values=some, info=some)
        p.update(ptrs)
        return lib.clx_basin_passes(p["labels"], p["dist_sq"], p["root"], nd, Z, Y, X, capacity, p["keys"], p["values"], p["info"], null)

    def basin_relabel(npix=64, n=3, nbytes=None, **ptrs):
        p = dict(root=some, summits=some, ids=some, out=some, bad=some, workspace=some)
        p.update(ptrs)
        nbytes = 64 + 4 * max(npix, 0) if nbytes is None else nbytes
        return lib.clx_basin_relabel(p["root"], npix, p["summits"], p["ids"], n, p["out"], p["bad"], p["workspace"], nbytes, null)

    shapes = [(dict(nd=1), "nd"), (dict(nd=4), "nd"), (dict(nd=2, Z=2), "Z == 1"), (dict(Y=0), "shape"), (dict(X=-1), "shape"),
              (dict(nd=3, Z=0), "shape"), (dict(Y=65536, X=65536), "Z * Y * X"), (dict(nd=3, Z=2, Y=46341, X=46341), "Z * Y * X")]
    cases = {
        "clx_label_basins": (label_basins, [({k: null}, "null pointer") for k in ("labels", "dist_sq", "root", "summits", "info", "workspace")]
                             + [(dict(kw, nbytes=2 ** 40), word) for kw, word in shapes]
                             + [(dict(capacity=0), "capacity"), (dict(capacity=-4), "capacity"), (dict(capacity=2 ** 30 + 1), "capacity"),
                                (dict(nbytes=64 + 4 * 64 - 1), "workspace_bytes"), (dict(nbytes=0), "workspace_bytes"),
                                (dict(workspace=ctypes.c_void_p(4098)), "aligned"), (dict(workspace=ctypes.c_void_p(4097)), "aligned")]),
        "clx_basin_passes": (basin_passes_, [({k: null}, "null pointer") for k in ("labels", "dist_sq", "root", "keys", "values", "info")]
                             + shapes + [(dict(capacity=512), "capacity"), (dict(capacity=1025), "capacity"), (dict(capacity=3000), "capacity"),
                                         (dict(capacity=2 ** 29), "capacity"), (dict(capacity=0), "capacity"), (dict(capacity=-1024), "capacity")]),
        "clx_basin_relabel": (basin_relabel, [({k: null}, "null pointer") for k in ("root", "summits", "ids", "out", "bad", "workspace")]
                              + [(dict(npix=0), "npix"), (dict(npix=-3), "npix"), (dict(npix=2 ** 32, nbytes=2 ** 40), "npix"),
                                 (dict(n=-1), "n must"), (dict(n=2 ** 30 + 1), "n must"), (dict(nbytes=64 + 4 * 64 - 1), "workspace_bytes"),
                                 (dict(workspace=ctypes.c_void_p(4098)), "aligned")]),
    }
    for name, (call, refused) in cases.items():
        for kw, word in refused:
            assert call(**kw) == -1, f"{name}{kw} was not refused"
            message = lib.clx_last_error().decode()
            assert message.startswith(name + ":") and word in message, f"{kw}: {message!r} does not name {word!r}"
    with pytest.raises(_clx.ClxError, match="clx_basin_passes.*capacity"):
        _clx.call("clx_basin_passes", some, some, some, 2, 1, 8, 8, 1000, some, some, some, null)


def test_cli_accepts_the_options():
    from click.testing import CliRunner

    from cellulus_amd.cli import split as split_cli

    text = CliRunner().invoke(split_cli, ["--help"]).output
    assert all(option in text for option in ("--source", "--output", "--depth", "--edge"))
    # accepted: the parse succeeds and the command goes on to read its file as a config, where this file fails
    result = CliRunner().invoke(split_cli, [__file__, "--source", "cells", "--output", "pieces", "--depth", "1.5", "--edge"])
    assert result.exit_code == 1 and "Invalid value" not in result.output and "No such option" not in result.output
    result = CliRunner().invoke(split_cli, [__file__, "--source", "cells"])
    assert result.exit_code == 2 and "--output" in result.output
    result = CliRunner().invoke(split_cli, [__file__, "--source", "cells", "--output", "pieces", "--depth", "-1"])
    assert result.exit_code == 2 and "--depth" in result.output
    text = open(os.path.join(ROOT, "cellulus_amd", "split.py")).read()
    assert 'from .cli import split as _command' in text


def test_arguments_checked_before_any_device(monkeypatch):
    from cellulus_amd import _clx

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    monkeypatch.setattr(_clx, "load", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for f, who in ((basins, "basins"), (basin_passes, "basin_passes"), (split_labels, "split_labels"), (split_table, "split_table")):
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
    for f, who in ((split_labels, "split_labels"), (split_table, "split_table")):
        for bad, kind in ((-1, ValueError), (-1e-300, ValueError), (math.nan, ValueError), (math.inf, ValueError), ("2", TypeError),
                          (None, TypeError), (True, TypeError), (1j, TypeError)):
            with pytest.raises(kind, match=f"^{who}: depth must be"):
                f(good, bad, device=fake)
    with pytest.raises(TypeError, match="^merge_basins: depth must be"):
        merge_basins([1], [4], [0], [], "1")
    for kw in (dict(source="", output="pieces"), dict(source=None, output="pieces"), dict(source="cells", output="cells"),
               dict(source="cells", output=""), dict(source="cells", output=None), dict(source="cells", output="pieces", depth=-1),
               dict(source="cells", output="pieces", depth=math.inf), dict(source="cells", output="pieces", depth=math.nan)):
        with pytest.raises(ValueError, match="^split_stage: "):
            split_stage(None, **kw)
    with pytest.raises(TypeError, match="^split_stage: depth must be"):
        split_stage(None, "cells", "pieces", depth="deep")


def test_cpu_device_raises():
    from cellulus_amd._clx import ClxError

    labels = np.ones((4, 5), np.int32)
    for call in (lambda: basins(labels, device="cpu"), lambda: basin_passes(labels, device=torch.device("cpu")),
                 lambda: split_labels(labels, 2, device="cpu"), lambda: split_table(labels, device="cpu")):
        with pytest.raises(ClxError, match="no CPU path"):
            call()
