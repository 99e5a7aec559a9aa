"""CPU tier of the measure stage's convex hull quantities (no kernel is launched): the restatement the GPU tests compare
with (tests/hull_ref.py) against scipy.spatial.ConvexHull (qhull), the host arithmetic behind the columns, the C-ABI
symbol and the command's flag.

Against qhull: at coordinates below 2^12 a polygon's doubled area is below 2^25 and qhull's float64 sum of it is wrong by
many orders less than 0.5, so its rounding must be A2; squared distances of integer points are exact in float64, so the
largest over qhull's vertices must EQUAL F2; the minimum width is recomputed in fractions.Fraction over qhull's edges
(a collinear point that qhull might keep splits an edge without changing its line, so the minimum is the same)."""

import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

from hull_ref import corner_points, hull_integers_2d, max_sq_distance, ref_hull, shapes, strict_hull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = shapes()


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))[f"{name}/labels"]


def _maps():
    m = {f"golden_{name}": _golden(name) for name in ("2d", "2d_edge", "3d")}
    m.update({name: labels for name, (labels, _) in SHAPES.items()})
    slabs = np.zeros((5, 6, 8), np.int32)
    slabs[1, 1:4, 2:6] = 1
    slabs[2, 1:4, 2:6] = 2
    slabs[4, 0:2, 0:3] = 3
    m["3d_slabs"] = slabs
    m["3d_one_voxel"] = np.ones((1, 1, 1), np.int32)
    return m


MAPS = _maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_restatement_against_qhull(name):
    labels = MAPS[name]
    nd = labels.ndim
    got = ref_hull(labels, nd)
    assert labels.max() < 2 ** 12 and max(labels.shape) < 2 ** 12
    ids = np.unique(labels)
    for i in ids[ids > 0]:
        corners = corner_points(np.argwhere(labels == i))
        hull = ConvexHull(corners.astype(np.float64))
        pts = hull.points[hull.vertices]
        d = pts[:, None, :] - pts[None, :, :]
        assert float((d * d).sum(axis=2).max()) == float(got[i, 2]), (name, i)       # integers in float64: exact
        if nd == 3:
            assert got[i].tolist() == [0, 0, got[i, 2], 0, 0]
            continue
        a2 = int(got[i, 0])
        assert round(2 * hull.volume) == a2 and abs(2 * hull.volume - a2) < 0.5, (name, i, hull.volume)   # 2-D: volume is the area
        verts = [(int(p[0]), int(p[1])) for p in pts]                               # in order around the hull in 2-D
        assert set(strict_hull(corners)) <= set(verts) and got[i, 1] == len(strict_hull(corners)) <= len(verts)
        widths = []
        for k in range(len(verts)):
            a, b = verts[k], verts[(k + 1) % len(verts)]
            e = (b[0] - a[0], b[1] - a[1])
            c = max(abs(e[0] * (v[1] - a[1]) - e[1] * (v[0] - a[0])) for v in verts)
            widths.append(Fraction(c * c, e[0] * e[0] + e[1] * e[1]))
        assert min(widths) == Fraction(int(got[i, 3]) ** 2, int(got[i, 4])), (name, i)
    absent = np.setdiff1d(np.arange(len(got)), ids[ids > 0])
    assert not got[absent].any()


def test_restatement_by_hand():
    square = [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert hull_integers_2d(square) == [2, 4, 2, 1, 1]                              # one pixel
    assert ref_hull(SHAPES["one_pixel"][0], 2)[1].tolist() == [2, 4, 2, 1, 1]
    assert ref_hull(SHAPES["bar_1x40"][0], 2)[1].tolist() == [80, 4, 1601, 40, 1600]
    assert ref_hull(SHAPES["fills_the_image_13x21"][0], 2)[3].tolist() == [2 * 13 * 21, 4, 13 ** 2 + 21 ** 2, 13 * 21, 21 ** 2]
    assert ref_hull(SHAPES["checkerboard_one_id_15x15"][0], 2)[1].tolist() == [450, 4, 450, 225, 225]      # the box
    # 16 x 16: the box less the two half-pixel triangles at the unset corners; the narrowest is across an edge of length 15
    assert ref_hull(SHAPES["checkerboard_one_id_16x16"][0], 2)[1].tolist() == [512 - 2, 6, 512, 15 * 16, 15 ** 2]
    # the concave side does not matter: L, C and ring of one box have the hull of the box or of the L's five corners
    assert ref_hull(SHAPES["C"][0], 2)[2].tolist() == ref_hull(SHAPES["ring"][0], 2)[3].tolist() == [200, 4, 200, 100, 100]
    assert ref_hull(SHAPES["C_open_left"][0], 2)[2].tolist() == [200, 4, 200, 100, 100]
    assert ref_hull(SHAPES["L"][0], 2)[1, :2].tolist() == [200 - 7 * 7, 5]
    # the staircase under the diagonal of a 12 x 12 square: 12 steps whose outer corners are collinear, whose inner are inside
    tri = ref_hull(SHAPES["staircase_triangle_12"][0], 2)[1]
    assert tri[:3].tolist() == [144 + 2 * 12 - 1, 5, 288]                            # the triangle and the strip of the first step
    # the trapezoid on a 1 x 12 strip: area 12 + (4 + 12) / 2; both parallel edges are 2 apart, c = 2 * 4 over the short one,
    # 2 * 12 over the long one: the short one wins
    assert ref_hull(SHAPES["trapezoid_tie"][0], 2)[1].tolist() == [2 * 12 + (4 + 12), 6, 12 ** 2 + 1, 8, 16]
    assert max_sq_distance(corner_points(np.zeros((1, 3), np.int64))) == 3          # one voxel
    flat = _golden("2d")
    f2, f3 = ref_hull(flat, 2), ref_hull(flat[None], 3)
    present = f2[:, 2] > 0
    assert np.array_equal(f3[present, 2], f2[present, 2] + 1)                        # one more unit along z, at right angles


def test_hull_columns_by_hand():
    from cellulus_amd.measure import hull_columns

    names = ["area_convex", "solidity", "feret_diameter_max", "feret_diameter_min", "hull_vertices"]
    # one pixel; a 2 x 4 rectangle; the staircase under the diagonal of a 3 x 3 square (6 pixels; its hull is the triangle
    # under the line through the steps' outer corners less the tip above the first row: doubled area 9 + 3 + 3 - 1); the two
    # candidates of the trapezoid's tie
    stairs = np.array([[1, 0, 0], [1, 1, 0], [1, 1, 1]], np.int32)
    a2, nv, f2, c, l2 = ref_hull(stairs, 2)[1].tolist()
    assert (a2, nv, f2) == (9 + 3 + 3 - 1, 5, 18)
    rows = [[2, 4, 2, 1, 1], [16, 4, 20, 8, 16], [a2, nv, f2, c, l2], [40, 6, 145, 8, 16], [40, 6, 145, 24, 144]]
    cols = hull_columns([1, 8, 6, 16, 16], rows, 2)
    assert list(cols) == names
    assert cols["area_convex"].tolist() == [1.0, 8.0, a2 / 2, 20.0, 20.0]
    assert cols["solidity"].tolist() == [1.0, 1.0, 12 / a2, 32 / 40, 32 / 40]
    assert cols["feret_diameter_max"].tolist() == [math.sqrt(2.0), math.sqrt(20.0), math.sqrt(18.0), math.sqrt(145.0), math.sqrt(145.0)]
    assert cols["feret_diameter_min"][:2].tolist() == [1.0, 2.0]
    assert cols["feret_diameter_min"][2] == pytest.approx(c / math.sqrt(l2), rel=2.0 ** -51)
    assert cols["feret_diameter_min"][3] == cols["feret_diameter_min"][4] == 2.0      # equal ratios: the same width exactly
    assert cols["hull_vertices"].tolist() == [4, 4, 5, 6, 6] and cols["hull_vertices"].dtype == np.int64
    assert all(cols[k].dtype == np.float64 for k in names[:4])
    # one rounding from exact integers, also where the integers exceed 2^53
    big = hull_columns([3], [[2 ** 60 + 2, 4, 2 ** 61 + 1, 2 ** 31 - 1, (2 ** 30 - 1) ** 2 + 1]], 2)
    assert big["area_convex"][0] == float(2 ** 59 + 1) and big["solidity"][0] == 6 / (2 ** 60 + 2)
    for got, exact_sq in ((big["feret_diameter_max"][0], Fraction(2 ** 61 + 1)),
                          (big["feret_diameter_min"][0], Fraction((2 ** 31 - 1) ** 2, (2 ** 30 - 1) ** 2 + 1))):
        lo, hi = Fraction(np.nextafter(got, 0.0)), Fraction(np.nextafter(got, np.inf))
        g = Fraction(got)
        assert ((g + lo) / 2) ** 2 <= exact_sq <= ((g + hi) / 2) ** 2                # the nearest float64 to the root
    c3 = hull_columns([1, 5], [[0, 0, 3, 0, 0], [0, 0, 50, 0, 0]], 3)
    assert list(c3) == ["feret_diameter_max"] and c3["feret_diameter_max"].tolist() == [math.sqrt(3.0), math.sqrt(50.0)]
    for nd, want in ((2, names), (3, ["feret_diameter_max"])):
        e = hull_columns(np.zeros(0, np.int64), np.zeros((0, 5), np.int64), nd)
        assert list(e) == want and all(len(v) == 0 for v in e.values())
        assert all(e[k].dtype == (np.int64 if k == "hull_vertices" else np.float64) for k in want)


def test_symbol_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, restype, nargs in (("clx_region_hull", "int", 14), ("clx_region_hull_workspace", "size_t", 1)):
        assert re.search(r"\b%s\s+%s\s*\(" % (restype, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs
    comment = open(os.path.join(ROOT, "include", "clx.h")).read()
    assert "NOT scikit-image's" in comment
    # the workspace size is host arithmetic: it grows with the rows and refuses a negative count
    size = _clx.load().clx_region_hull_workspace
    assert size(-1) == 0 and size(0) > 0 and size(1000) >= 8 * 1000 and size(2000) == 2 * size(1000)


def test_cli_accepts_hull_flag():
    from click.testing import CliRunner

    from cellulus_amd import cli

    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and "--hull" in res.output and "--topology" in res.output and "--contacts" in res.output
    res = CliRunner().invoke(cli.measure, ["--hull", "--topology", "--contacts", "missing.toml"])
    assert res.exit_code != 0 and "does not exist" in res.output        # the flags parse; the file is what is wrong


def test_hull_has_no_cpu_path_and_checks_labels_first(monkeypatch):
    from cellulus_amd import _clx, measure
    from cellulus_amd._clx import ClxError

    labels = torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ClxError, match="no CPU path"):
        measure.region_table(labels, device="cpu", hull=True)
    with pytest.raises(ClxError, match="no CPU path"):
        measure.region_table(labels.numpy(), device=torch.device("cpu"), boundary=True, topology=True, hull=True)

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for bad, error in ((good.astype(np.float32), TypeError), (good - 2, ValueError), (good.astype(np.int64) << 24, ValueError),
                       (np.ones(5, np.int32), ValueError)):
        with pytest.raises(error):
            measure.region_table(bad, device=fake, hull=True)
