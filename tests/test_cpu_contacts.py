"""CPU tier of the measure stage's boundary quantities (no kernel is launched): the host arithmetic behind the boundary
columns, the C-ABI symbols, the command's flag, the refusals that need no device — and the restatements the GPU tests
compare with (tests/contacts_ref.py), on the fixture's maps."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from contacts_ref import ref_boundary_columns, ref_contacts, ref_perimeter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT2 = math.sqrt(2.0)


def test_perimeter_from_classes():
    from cellulus_amd.measure import perimeter_from_classes

    classes = [[1, 0, 0, 0], [12, 12, 0, 0], [5, 0, 5, 0], [9, 2, 3, 4], [0, 0, 0, 0], [2 ** 40, 2 ** 40, 0, 0]]
    got = perimeter_from_classes(classes)
    assert got.dtype == np.float64
    want = [0.0, 12.0, 5 * SQRT2, 2 + 3 * SQRT2 + 4 * (1 + SQRT2) / 2, 0.0, float(2 ** 40)]
    assert np.allclose(got, want, rtol=1e-15, atol=0)
    assert got[0] == 0.0 and got[1] == 12.0                             # a one-pixel object; weight 1 is exact
    assert perimeter_from_classes(np.zeros((0, 4), np.uint64)).shape == (0,)


def test_boundary_columns_by_hand_2d():
    """Counts as of a 6 x 8 map: object 2 touches 3 along 2 faces and 5 along 1; 3 reaches the last column; 9 is one
    pixel in a corner and touches no object."""
    from cellulus_amd.measure import boundary_columns

    present = [2, 3, 5, 9]
    bbox = [[0, 1, 1, 0, 2, 3], [0, 1, 4, 0, 2, 7], [0, 3, 2, 0, 4, 2], [0, 5, 0, 0, 5, 0]]
    a = [0, 0, 0, 0, 2, 2]
    b = [2, 3, 5, 9, 3, 5]
    faces = [7, 10, 5, 4, 2, 1]
    classes = [[6, 6, 0, 0], [8, 8, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]]
    c = boundary_columns(present, bbox, (6, 8), a, b, faces, classes, 2)
    assert list(c) == ["boundary_faces", "contact_faces", "num_neighbours", "touches_border", "border_pixels", "perimeter"]
    assert c["boundary_faces"].tolist() == [10, 12, 6, 4]
    assert c["contact_faces"].tolist() == [3, 2, 1, 0]
    assert c["num_neighbours"].tolist() == [2, 1, 1, 0]
    assert c["touches_border"].tolist() == [0, 1, 0, 1]                  # 3: xmax == 7; 9: ymax == 5 and xmin == 0
    assert c["border_pixels"].tolist() == [6, 8, 2, 1]
    assert c["perimeter"].tolist() == [6.0, 8.0, 0.0, 0.0]
    assert all(v.dtype == np.int64 for k, v in c.items() if k != "perimeter")


def test_boundary_columns_lonely_edge_only_empty_and_3d():
    from cellulus_amd.measure import boundary_columns

    # one object with no neighbours at all (only background around it), away from the edge
    c = boundary_columns([4], [[0, 2, 2, 0, 3, 3]], (9, 9), [0], [4], [8], [[4, 4, 0, 0]], 2)
    assert [c[k].tolist() for k in c] == [[8], [0], [0], [0], [4], [4.0]]
    # an object that fills the image: it touches only the edge
    c = boundary_columns([1], [[0, 0, 0, 0, 2, 4]], (3, 5), [0], [1], [16], [[12, 12, 0, 0]], 2)
    assert [c[k].tolist() for k in c] == [[16], [0], [0], [1], [12], [12.0]]
    # an empty table keeps its columns
    for nd, shape in ((2, (4, 4)), (3, (2, 4, 4))):
        e = boundary_columns([], np.zeros((0, 6)), shape, [], [], [], np.zeros((0, 4)) if nd == 2 else None, nd)
        assert all(len(v) == 0 for v in e.values())
        assert ("perimeter" in e) == (nd == 2) and "boundary_faces" in e
    # 3-D: the z extent counts for touches_border, and there is no perimeter
    c = boundary_columns([1, 2], [[0, 1, 1, 0, 2, 2], [1, 1, 1, 2, 2, 2]], (4, 5, 5), [0, 0, 1], [1, 2, 2], [12, 20, 4], None, 3)
    assert list(c) == ["boundary_faces", "contact_faces", "num_neighbours", "touches_border"]
    assert c["boundary_faces"].tolist() == [16, 24] and c["contact_faces"].tolist() == [4, 4]
    assert c["num_neighbours"].tolist() == [1, 1] and c["touches_border"].tolist() == [1, 0]
    # in 2-D the z entries of the bounding box (always 0) are not looked at
    c = boundary_columns([1], [[0, 1, 1, 0, 1, 1]], (3, 3), [0], [1], [4], [[1, 0, 0, 0]], 2)
    assert c["touches_border"].tolist() == [0]


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name in ("clx_region_contacts", "clx_region_perimeter"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES
    assert len(_clx.PROTOTYPES["clx_region_contacts"][1]) == 11
    assert len(_clx.PROTOTYPES["clx_region_perimeter"][1]) == 7


def test_cli_accepts_contacts_flag():
    from click.testing import CliRunner

    from cellulus_amd import cli

    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and "--contacts" in res.output
    res = CliRunner().invoke(cli.measure, ["--contacts", "missing.toml"])
    assert res.exit_code != 0 and "does not exist" in res.output        # the flag parses; the file is what is wrong


def test_contact_pairs_has_no_cpu_path():
    from cellulus_amd._clx import ClxError
    from cellulus_amd.measure import contact_pairs, region_table

    labels = torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ClxError, match="no CPU path"):
        contact_pairs(labels, device="cpu")
    with pytest.raises(ClxError, match="no CPU path"):
        contact_pairs(labels.numpy(), device=torch.device("cpu"))
    with pytest.raises(ClxError, match="no CPU path"):
        region_table(labels, device="cpu", boundary=True)
    if not torch.cuda.is_available():
        with pytest.raises(ClxError, match="no CPU path"):
            contact_pairs(labels)


def test_bad_labels_raise_before_any_device_call(monkeypatch):
    """The type and range checks come before the first entry point: with `_clx.call` replaced nothing may reach it."""
    from cellulus_amd import _clx, measure

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for bad, error in ((good.astype(np.float32), TypeError), (good.astype(bool), TypeError), (good - 2, ValueError),
                       (good.astype(np.int64) << 24, ValueError), (np.ones(5, np.int32), ValueError),
                       (np.ones((2, 2, 2, 2), np.int32), ValueError)):
        with pytest.raises(error):
            measure.contact_pairs(bad, device=fake)
        with pytest.raises(error):
            measure.region_table(bad, device=fake, boundary=True)
    for bad in (torch.ones(4, 5), torch.ones(4, 5, dtype=torch.bool)):
        with pytest.raises(TypeError):
            measure.contact_pairs(bad, device=fake)


def test_pair_capacity():
    from cellulus_amd.measure import MAX_CAPACITY, MIN_CAPACITY, _pair_capacity

    assert (MIN_CAPACITY, MAX_CAPACITY) == (1 << 10, 1 << 28)
    for objects in (0, 1, 127, 128, 129, 6400, 100000, 2 ** 24 - 1):
        c = _pair_capacity(objects)
        assert c & (c - 1) == 0 and c >= 1024 and c >= 8 * objects and (c == 1024 or c < 16 * objects)


# ------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("name,pairs,between,faces", [("2d", 29, 15, 489), ("2d_edge", 3, 0, 322), ("3d", 13, 4, 489)])
def test_restatements_on_the_fixture_maps(name, pairs, between, faces):
    """The fixture's maps exercise what they should: distinct pairs, object-object pairs and faces in all."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    labels = g[f"{name}/labels"]
    keys, counts = ref_contacts(labels, labels.ndim)
    assert len(keys) == pairs and int(((keys >> np.uint64(32)) > 0).sum()) == between and int(counts.sum()) == faces
    assert np.all(keys[1:] > keys[:-1]) and np.all((keys >> np.uint64(32)) < (keys & np.uint64(0xFFFFFFFF)))
    cols, (a, b, n) = ref_boundary_columns(labels)
    assert np.array_equal(cols["boundary_faces"] - cols["contact_faces"], [int(n[(a == 0) & (b == i)].sum()) for i in np.unique(labels)[1:]])
    assert cols["contact_faces"].sum() == 2 * n[a > 0].sum()
    if name == "2d_edge":
        classes, perimeter = ref_perimeter(labels, int(labels.max()) + 1)
        assert perimeter[2] == 34.41421356237309 and perimeter[3] == 136.0 and perimeter[7] == 0.0
        assert classes[7].tolist() == [1, 0, 0, 0]


def test_restatements_by_hand():
    one = np.ones((1, 1), np.int32)
    assert [v.tolist() for v in ref_contacts(one, 2)] == [[1], [4]]
    assert [v.tolist() for v in ref_contacts(one, 3)] == [[1], [6]]
    two = np.array([[1, 1, 2], [0, 2, 2]], np.int32)
    keys, counts = ref_contacts(two, 2)
    assert keys.tolist() == [1, 2, (1 << 32) | 2] and counts.tolist() == [4, 6, 2]
    keys, counts = ref_contacts(np.array([[1, 5, -3], [9, 2, 2]]), 2, nid=3)        # 5, -3 and 9 become background
    assert keys.tolist() == [1, 2] and counts.tolist() == [4, 6]
    rect = np.zeros((9, 11), np.int32)
    rect[2:6, 3:10] = 1
    classes, perimeter = ref_perimeter(rect, 2)
    assert classes[1].tolist() == [18, 18, 0, 0] and perimeter[1] == 18.0            # 2 (h + w) - 4
    diag = np.eye(6, dtype=np.int32)
    classes, perimeter = ref_perimeter(diag, 2)
    assert classes[1].tolist() == [6, 0, 4, 0]                                       # the ends have code 11: weight 0
