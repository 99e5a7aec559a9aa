"""CPU tier of the measure stage's inscribed circle / ball (no kernel is launched): the restatement the GPU tests compare
with (tests/inscribed_ref.py: scipy's distance transform per object on a crop) against all pixel pairs in NumPy, the host
arithmetic behind the columns, the C-ABI symbols and the command's flag."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from inscribed_ref import DIST_INF, brute_distance_sq, ref_distance_sq, ref_inscribed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES_2D = ["inscribed_radius", "inscribed_centre_y", "inscribed_centre_x", "distance_sq_mean"]
NAMES_3D = ["inscribed_radius", "inscribed_centre_z", "inscribed_centre_y", "inscribed_centre_x", "distance_sq_mean"]


def _small_maps():
    rng = np.random.default_rng(5)
    maps = []
    for trial in range(40):
        nd = 2 + trial % 2
        shape = tuple(int(v) for v in rng.integers(1, 7 if nd == 3 else 13, size=nd))
        lab = rng.integers(0, int(rng.integers(1, 5)) + 1, size=shape)
        if trial % 8 == 0:
            lab[:] = 3                                                  # one value everywhere: the INF map
        if trial % 8 == 1:
            lab = lab - 2                                               # negative values are objects too
        maps.append(lab)
    return maps


@pytest.mark.parametrize("edge", [0, 1])
def test_restatement_against_all_pixel_pairs(edge):
    for lab in _small_maps():
        want = brute_distance_sq(lab, edge)
        got = ref_distance_sq(lab, edge)
        assert np.array_equal(got, want), (lab.tolist(), got.tolist(), want.tolist())
        assert ((got == 0) == (lab == 0)).all()
        if len(np.unique(lab)) == 1 and lab.flat[0] != 0 and not edge:
            assert (got == DIST_INF).all()
        else:
            assert got.max() < DIST_INF


def test_restatement_by_hand():
    square = np.zeros((7, 7), np.int32)
    square[1:6, 1:6] = 1
    d = ref_distance_sq(square, 0)
    assert d[3, 3] == 9 and d[1, 1] == 1 and d[2, 2] == 4 and d[0, 0] == 0
    full = np.ones((5, 5), np.int32)
    assert (ref_distance_sq(full, 0) == DIST_INF).all()
    assert ref_distance_sq(full, 1).tolist() == [[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 4, 9, 4, 1], [1, 4, 4, 4, 1], [1, 1, 1, 1, 1]]
    # two half planes: a binary transform (distance to the background) would see no candidate at all here
    halves = np.ones((4, 6), np.int32)
    halves[:, 3:] = 2
    assert ref_distance_sq(halves, 0)[0].tolist() == [9, 4, 1, 1, 4, 9]
    assert ref_distance_sq(halves, 1)[0].tolist() == [1, 1, 1, 1, 1, 1] and ref_distance_sq(halves, 1)[1].tolist() == [1, 4, 1, 1, 4, 1]
    # Z == 1 with z counted: the padding is one step away from every pixel
    assert (ref_distance_sq(full[None], 1) == 1).all() and (ref_distance_sq(full[None], 0) == DIST_INF).all()
    out, bad = ref_inscribed(np.array([[1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]]), np.array([[1, 4, 4, 4, 4, 1], [1, 4, 4, 4, 4, 1]]), 3)
    assert out.tolist() == [[0, 0, 0], [4, 1, 36], [0, 0, 0]] and bad == 0          # the tie goes to the smallest index


def test_inscribed_columns_by_hand():
    from cellulus_amd import measure
    from cellulus_amd.measure import inscribed_columns

    assert measure.DIST_INF == DIST_INF
    # a one-pixel object at (2, 3); the 5 x 5 square of a 5 x 5 map under edge=True (D2 = 9 at its centre, index 12; Σd² from
    # the restatement); the INF row; D2 = 2 somewhere
    square = ref_distance_sq(np.ones((5, 5), np.int32), 1)
    assert square[2, 2] == 9 == square.max() and int(square.sum()) == 16 + 8 * 4 + 9
    cols = inscribed_columns([1, 25, 25, 7], [[1, 2 * 5 + 3, 1], [9, 12, 57], [DIST_INF, 0, 25 * DIST_INF], [2, 24, 9]], (5, 5), 2)
    assert list(cols) == NAMES_2D
    assert cols["inscribed_radius"].tolist() == [1.0, 3.0, math.inf, math.sqrt(2.0)]
    assert cols["inscribed_centre_y"].tolist() == [2, 2, 0, 4] and cols["inscribed_centre_x"].tolist() == [3, 2, 0, 4]
    assert cols["distance_sq_mean"].tolist() == [1.0, 57 / 25, math.inf, 9 / 7]
    assert all(cols[k].dtype == (np.int64 if "centre" in k else np.float64) for k in NAMES_2D)
    # centres unravelled in 3-D: index (z * Y + y) * X + x in a 4 x 5 x 6 map
    c3 = inscribed_columns([10, 3], [[16, (3 * 5 + 4) * 6 + 5, 40], [5, (1 * 5 + 0) * 6 + 2, 7]], (4, 5, 6), 3)
    assert list(c3) == NAMES_3D
    assert [c3[f"inscribed_centre_{a}"].tolist() for a in "zyx"] == [[3, 1], [4, 0], [5, 2]]
    assert c3["inscribed_radius"].tolist() == [4.0, math.sqrt(5.0)] and c3["distance_sq_mean"].tolist() == [4.0, 7 / 3]
    # one rounding from exact integers where the sum exceeds 2^53
    big = inscribed_columns([3], [[(1 << 30) - 1, 0, (1 << 61) + 1]], (2, 2), 2)
    assert big["distance_sq_mean"][0] == ((1 << 61) + 1) / 3 and big["inscribed_radius"][0] == math.sqrt((1 << 30) - 1)
    for nd, shape, want in ((2, (3, 3), NAMES_2D), (3, (2, 3, 3), NAMES_3D)):
        e = inscribed_columns(np.zeros(0, np.int64), np.zeros((0, 3), np.int64), shape, nd)
        assert list(e) == want and all(len(v) == 0 for v in e.values())
        assert all(e[k].dtype == (np.int64 if "centre" in k else np.float64) for k in want)


def test_symbols_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    raw = open(os.path.join(ROOT, "include", "clx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    for name, restype, nargs in (("clx_label_distance_workspace", "size_t", 1), ("clx_label_distance_sq", "int", 10),
                                 ("clx_region_inscribed", "int", 7)):
        assert re.search(r"\b%s\s+%s\s*\(" % (restype, name), text), f"{name} is not declared in include/clx.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _clx.PROTOTYPES and len(_clx.PROTOTYPES[name][1]) == nargs
    assert re.search(r"#define\s+CLX_DIST_INF\s+\(1 << 30\)", text)
    assert _clx.load().clx_abi_version() == 13
    # the workspace size is host arithmetic: one int32 map, 0 for a pixel count out of range
    size = _clx.load().clx_label_distance_workspace
    assert size(-1) == 0 and size(0) == 0 and size(1) == 4 and size(1000) == 4000
    assert size(2 ** 32 - 1) == 4 * (2 ** 32 - 1) and size(2 ** 32) == 0


def test_cli_accepts_inscribed_flag():
    from click.testing import CliRunner

    from cellulus_amd import cli

    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and "--inscribed" in res.output and "--hull" in res.output
    res = CliRunner().invoke(cli.measure, ["--inscribed", "--hull", "--topology", "--contacts", "missing.toml"])
    assert res.exit_code != 0 and "does not exist" in res.output        # the flags parse; the file is what is wrong


def test_no_cpu_path_and_labels_checked_first(monkeypatch):
    from cellulus_amd import _clx, measure
    from cellulus_amd._clx import ClxError

    labels = torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ClxError, match="no CPU path"):
        measure.label_distance_sq(labels, device="cpu")
    with pytest.raises(ClxError, match="no CPU path"):
        measure.region_table(labels.numpy(), device=torch.device("cpu"), inscribed=True, edge=True)

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for bad, error in ((good.astype(np.float32), TypeError), (good - 2, ValueError), (good.astype(np.int64) << 24, ValueError),
                       (np.ones(5, np.int32), ValueError)):
        with pytest.raises(error, match="^label_distance_sq:"):
            measure.label_distance_sq(bad, device=fake)
        with pytest.raises(error, match="^region_table:"):
            measure.region_table(bad, device=fake, inscribed=True)
