"""CPU tier of the measure stage's topology quantities (no kernel is launched): the restatements the GPU tests compare
with (tests/topology_ref.py) against each other, the identities between the window sums and the boundary counts, the
direction weights, the host arithmetic behind the columns, the C-ABI symbol and the command's flag."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from contacts_ref import ref_contacts
from topology_ref import (direction_weights, euler_by_cells, euler_by_label_2d, mask_window_sums, ref_topology_columns,
                          ref_topology_table, ref_window_sums)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT2, SQRT3 = math.sqrt(2.0), math.sqrt(3.0)


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))[f"{name}/labels"]


def _solids():
    """ball, shell and torus of the issue on a 31^3 grid, and the disc on 31^2"""
    zz, yy, xx = np.indices((31, 31, 31)) - 15
    d2 = zz ** 2 + yy ** 2 + xx ** 2
    y2, x2 = np.indices((31, 31)) - 15
    return {"ball": d2 <= 144, "shell": (d2 > 25) & (d2 <= 144),
            "torus": (np.sqrt(yy ** 2 + xx ** 2) - 9) ** 2 + zz ** 2 <= 3.2 ** 2, "disc": y2 ** 2 + x2 ** 2 <= 144}


def _pairs_by_offset(mask):
    """[n1, n2, n3]: neighbour pairs (set, not set) of a mask by the number of coordinates they differ in; the outside
    is not set"""
    nd = mask.ndim
    p = np.pad(mask, 1)
    out = [0, 0, 0]
    offsets = [o for o in np.ndindex((3,) * nd) if any(v != 1 for v in o)]
    for o in offsets:
        k = sum(v != 1 for v in o)
        shifted = p[tuple(slice(v, v + s) for v, s in zip(o, mask.shape))]       # the neighbour at offset o - 1
        out[k - 1] += int((mask & ~shifted).sum())
    return out


@pytest.mark.parametrize("shape", [(9, 11), (5, 6, 7)])
@pytest.mark.parametrize("density", [0.2, 0.5, 0.8])
def test_euler_restatements_agree_on_random_masks(shape, density):
    nd = len(shape)
    for seed in range(4):
        mask = np.random.default_rng(100 * seed + int(10 * density)).random(shape) < density
        sums = mask_window_sums(mask)
        hi, lo = euler_by_cells(mask)
        assert (sums[3], sums[4]) == (hi << nd, lo << nd)
        if nd == 2:
            assert euler_by_label_2d(mask) == (hi, lo)
        n = _pairs_by_offset(mask)
        assert sums[0] == n[0] << (nd - 1) and sums[1] == n[1] << (nd - 2) and sums[2] == n[2]
        assert ref_window_sums(mask.astype(np.int32), nd)[1].tolist() == sums       # the all-ids form, one id


@pytest.mark.parametrize("name", ["2d", "2d_edge", "3d"])
def test_restatements_on_the_fixture_maps(name):
    labels = _golden(name)
    nd = labels.ndim
    counts = ref_window_sums(labels, nd)
    keys, faces = ref_contacts(labels, nd)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids = np.unique(labels)
    assert len(counts) == ids.max() + 1
    for i in ids[ids > 0]:
        mask = labels == i
        assert counts[i].tolist() == mask_window_sums(mask)
        hi, lo = euler_by_cells(mask)
        assert (counts[i, 3], counts[i, 4]) == (hi << nd, lo << nd)
        if nd == 2:
            assert euler_by_label_2d(mask) == (hi, lo)
        assert counts[i, 0] == int(faces[(a == i) | (b == i)].sum()) << (nd - 1)     # T1 = 2^(nd-1) boundary_faces
        n = _pairs_by_offset(mask)
        assert counts[i, 1] == n[1] << (nd - 2) and counts[i, 2] == n[2]
    absent = np.setdiff1d(np.arange(len(counts)), ids[ids > 0])
    assert not counts[absent].any()


def test_nd3_on_a_flat_map_differs_from_nd2_as_defined():
    """Z == 1 under nd == 3: every 2-D window appears in two 3-D windows (the slice above and below are outside), and
    the pairs along z all differ"""
    labels = _golden("2d")
    c2, c3 = ref_window_sums(labels, 2), ref_window_sums(labels[None], 3)
    area = np.bincount(labels.ravel(), minlength=len(c2))
    for i in range(1, len(c2)):
        n = _pairs_by_offset(labels == i)
        n3 = _pairs_by_offset((labels == i)[None])
        assert c3[i, 0] == 2 * c2[i, 0] + 8 * area[i] == 4 * n3[0]
        assert (c3[i, 1], c3[i, 2]) == (2 * n3[1], n3[2]) and c2[i, 1] == n[1]
        assert (c3[i, 3], c3[i, 4]) == (2 * c2[i, 3], 2 * c2[i, 4])


def test_restatements_by_hand():
    assert mask_window_sums(np.ones((1, 1), bool)) == [8, 4, 0, 4, 4]
    assert mask_window_sums(np.ones((1, 1, 1), bool)) == [24, 24, 8, 8, 8]
    assert mask_window_sums(np.eye(2, dtype=bool)) == [16, 6, 0, 4, 8]
    ring = np.ones((3, 3), bool)
    ring[1, 1] = False
    assert euler_by_cells(ring) == (0, 0) and euler_by_label_2d(ring) == (0, 0)
    assert euler_by_cells(np.eye(3, dtype=bool)) == (1, 3)
    hollow = np.ones((3, 3, 3), bool)
    hollow[1, 1, 1] = False
    assert euler_by_cells(hollow) == (2, 2)
    two = np.array([[1, 1, 2], [0, 2, 2]], np.int32)
    assert ref_window_sums(two, 2)[1:].tolist() == [mask_window_sums(two == 1), mask_window_sums(two == 2)]
    assert ref_window_sums(np.array([[1, 5, -3], [9, 2, 2]]), 2, nid=3)[1:].tolist() == [[8, 4, 0, 4, 4], [12, 8, 0, 4, 4]]


def test_surface_weights_against_spherical_voronoi():
    from cellulus_amd.measure import SURFACE_WEIGHTS

    w = direction_weights()
    assert len(SURFACE_WEIGHTS) == 3
    for got, want in zip(SURFACE_WEIGHTS, w):
        assert abs(got - want) < 1e-12
    assert abs(3 * SURFACE_WEIGHTS[0] + 6 * SURFACE_WEIGHTS[1] + 4 * SURFACE_WEIGHTS[2] - 1.0) < 1e-12
    assert np.allclose(SURFACE_WEIGHTS, [0.0915557824, 0.0739612557, 0.0703912796], rtol=0, atol=1e-9)


def test_topology_columns_by_hand():
    """One pixel: its 4 windows each hold it alone, so each has 2 edge pairs and 1 diagonal pair that differ, and E = 1:
    T1 T2 T3 E_hi E_lo = 8 4 0 4 4, N1 = 4 faces, N2 = 4 diagonal neighbours.  One voxel: 8 windows, each with 3 + 3 + 1
    differing pairs: 24 24 8 8 8, N1 = 6, N2 = 12, N3 = 8.  The 2 x 2 checkerboard [[1, 0], [0, 1]]: 6 windows with one
    pixel and the middle one with the two diagonal pixels: E_hi = 6 - 2 = 4, E_lo = 6 + 2 = 8, T1 = 6 * 2 + 4 = 16,
    T2 = 6 (the middle window's diagonal pairs agree)."""
    from cellulus_amd.measure import SURFACE_WEIGHTS, topology_columns

    c = topology_columns([1, 2, 5], [[8, 4, 0, 4, 4], [16, 6, 0, 4, 8], [24, 14, 0, -4, 0]], 2)
    assert list(c) == ["euler_number", "euler_number_conn1", "perimeter_crofton"]
    assert c["euler_number"].tolist() == [1, 1, -1] and c["euler_number_conn1"].tolist() == [1, 2, 0]
    assert c["euler_number"].dtype == c["euler_number_conn1"].dtype == np.int64 and c["perimeter_crofton"].dtype == np.float64
    want = [math.pi / 8 * (4 + 4 / SQRT2), math.pi / 8 * (8 + 6 / SQRT2), math.pi / 8 * (12 + 14 / SQRT2)]
    assert np.allclose(c["perimeter_crofton"], want, rtol=1e-15, atol=0)
    w1, w2, w3 = SURFACE_WEIGHTS
    c = topology_columns([1, 7], [[24, 24, 8, 8, 8], [2 ** 42, 2 ** 41, 2 ** 40, -16, 2 ** 33]], 3)
    assert list(c) == ["euler_number", "euler_number_conn1", "surface_area", "sphericity"]
    assert c["euler_number"].tolist() == [1, -2] and c["euler_number_conn1"].tolist() == [1, 2 ** 30]
    surface = 4 * (w1 * 6 / 2 + w2 * 12 / (2 * SQRT2) + w3 * 8 / (2 * SQRT3))
    assert c["surface_area"][0] == pytest.approx(surface, rel=1e-15)
    assert c["sphericity"][0] == pytest.approx(math.pi ** (1 / 3) * 6 ** (2 / 3) / surface, rel=1e-15)
    big = 4 * (w1 * 2 ** 40 / 2 + w2 * 2 ** 40 / (2 * SQRT2) + w3 * 2 ** 40 / (2 * SQRT3))
    assert c["surface_area"][1] == pytest.approx(big, rel=1e-15)
    for nd, names in ((2, ["perimeter_crofton"]), (3, ["surface_area", "sphericity"])):
        e = topology_columns(np.zeros(0, np.int64), np.zeros((0, 5), np.int64), nd)
        assert list(e) == ["euler_number", "euler_number_conn1"] + names
        assert all(len(v) == 0 for v in e.values())
        assert e["euler_number"].dtype == e["euler_number_conn1"].dtype == np.int64
        assert all(e[k].dtype == np.float64 for k in names)
    # the restated columns give the same
    ref = ref_topology_columns([1, 2, 5], [[8, 4, 0, 4, 4], [16, 6, 0, 4, 8], [24, 14, 0, -4, 0]], 2)
    assert ref["euler_number"].tolist() == [1, 1, -1] and np.allclose(ref["perimeter_crofton"], want, rtol=1e-15, atol=0)


def test_ball_shell_torus_and_disc():
    from cellulus_amd.measure import topology_columns

    solids = _solids()
    r = 12.0
    for name, euler in (("ball", 1), ("shell", 2), ("torus", 0)):
        mask = solids[name]
        sums = mask_window_sums(mask)
        assert euler_by_cells(mask) == (euler, euler)
        c = topology_columns([int(mask.sum())], [sums], 3)
        assert c["euler_number"].tolist() == [euler] and c["euler_number_conn1"].tolist() == [euler]
        ref, _ = ref_topology_table(mask.astype(np.int32))
        assert ref["euler_number"].tolist() == [euler]
        assert c["surface_area"][0] == pytest.approx(ref["surface_area"][0], rel=1e-14)
        if name == "ball":
            faces = sums[0] // 4
            sphere = 4 * math.pi * r * r
            print("ball: surface_area", c["surface_area"][0], "boundary_faces", faces, "4 pi r^2", sphere, "sphericity", c["sphericity"][0])
            assert faces == 2646
            assert abs(c["surface_area"][0] - sphere) < abs(faces - sphere)
            assert c["surface_area"][0] == pytest.approx(1779.07, abs=0.01)
    disc = solids["disc"]
    sums = mask_window_sums(disc)
    c = topology_columns([int(disc.sum())], [sums], 2)
    faces = sums[0] // 2
    print("disc: perimeter_crofton", c["perimeter_crofton"][0], "boundary_faces", faces, "2 pi r", 2 * math.pi * r)
    assert faces == 100 and c["euler_number"].tolist() == [1] and c["euler_number_conn1"].tolist() == [1]
    assert abs(c["perimeter_crofton"][0] - 2 * math.pi * r) < abs(faces - 2 * math.pi * r)
    assert c["perimeter_crofton"][0] == pytest.approx(75.92, abs=0.01)


def test_symbol_declared_exported_prototyped():
    from cellulus_amd import _build, _clx

    _build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clx.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_clx.LIB_PATH)
    name = "clx_region_topology"
    assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} is not declared in include/clx.h"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in _clx.PROTOTYPES
    assert len(_clx.PROTOTYPES[name][1]) == 9


def test_cli_accepts_topology_flag():
    from click.testing import CliRunner

    from cellulus_amd import cli

    res = CliRunner().invoke(cli.measure, ["--help"])
    assert res.exit_code == 0 and "--topology" in res.output and "--contacts" in res.output
    res = CliRunner().invoke(cli.measure, ["--topology", "--contacts", "missing.toml"])
    assert res.exit_code != 0 and "does not exist" in res.output        # the flags parse; the file is what is wrong


def test_topology_has_no_cpu_path_and_checks_labels_first(monkeypatch):
    from cellulus_amd import _clx, measure
    from cellulus_amd._clx import ClxError

    labels = torch.ones(4, 5, dtype=torch.int32)
    with pytest.raises(ClxError, match="no CPU path"):
        measure.region_table(labels, device="cpu", topology=True)
    with pytest.raises(ClxError, match="no CPU path"):
        measure.region_table(labels.numpy(), device=torch.device("cpu"), boundary=True, topology=True)

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    monkeypatch.setattr(_clx, "require_device", no_call)
    fake = torch.device("cuda", 0)                                       # never used: every case fails on the host
    good = np.ones((4, 5), np.int32)
    for bad, error in ((good.astype(np.float32), TypeError), (good - 2, ValueError), (good.astype(np.int64) << 24, ValueError),
                       (np.ones(5, np.int32), ValueError)):
        with pytest.raises(error):
            measure.region_table(bad, device=fake, topology=True)
