"""clx_region_topology through the C ABI against the restatement of tests/topology_ref.py (shifted views of the
zero-padded map, np.bincount per id).  Everything is integer work: the five counts T1 T2 T3 E_hi E_lo from row 1 up must
be EQUAL for every id.  Outputs are prefilled with 0xAB bytes (or other garbage) and sit between guard words that must
stay untouched."""

import ctypes
import os

import numpy as np
import pytest
import torch

from test_gpu_measure import GUARD, Out, _blobs, _dev
from topology_ref import ref_window_sums

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))[f"{name}/labels"]


def call_topology(labels, nd, nid, device, offset=0, fill=0xAB):
    """-> (counts int64 (nid, 5), bad) as the entry point left them; the guard words are checked"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    Z, Y, X = (1,) * (3 - labels.ndim) + labels.shape
    lab = _dev(labels, device, offset)
    outs = dict(counts=Out((nid, 5), np.int64, device), bad=Out((1,), np.int32, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = _clx.load().clx_region_topology(_clx.ptr(lab), nd, Z, Y, X, nid, outs["counts"].ptr, outs["bad"].ptr,
                                             _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return outs["counts"].get(), int(outs["bad"].get()[0])


def assert_topology_equal(labels, nd, nid, device, **kw):
    counts, bad = call_topology(labels, nd, nid, device, **kw)
    want = ref_window_sums(labels, nd, nid)
    differ = np.flatnonzero((counts[1:] != want[1:]).any(axis=1)) + 1
    assert len(differ) == 0, (len(differ), [(int(i), counts[i].tolist(), want[i].tolist()) for i in differ[:4]])
    lab = np.asarray(labels)
    assert bad == int(((lab < 0) | (lab >= nid)).any())
    return counts


def _noise(shape, ids, seed):
    """every pixel its own draw of `ids` ids: windows of every kind at every position"""
    return np.random.default_rng(seed).integers(0, ids, size=shape).astype(np.int32)


def _solids(n=24):
    """a spherical shell (one cavity) and a torus (one tunnel) on an n^3 grid"""
    c = (n - 1) / 2.0
    zz, yy, xx = np.indices((n, n, n)) - c
    d2 = zz ** 2 + yy ** 2 + xx ** 2
    shell = (d2 > 16) & (d2 <= 100)
    torus = (np.sqrt(yy ** 2 + xx ** 2) - 7.5) ** 2 + zz ** 2 <= 2.6 ** 2
    return shell.astype(np.int32), torus.astype(np.int32)


def _cases():
    c = {}
    # row ends: a lane's 4 pixels straddle rows unless X is a multiple of 4
    for X in (1, 2, 3, 5):
        c[f"row_ends_9x{X}"] = (_noise((9, X), 4, X), 2, 4)
    c["row_ends_3x1027"] = (_noise((3, 1027), 3, 7), 2, 3)
    c["one_row_1x37"] = (_noise((1, 37), 4, 8), 2, 4)
    c["one_pixel"] = (np.ones((1, 1), np.int32), 2, 2)
    c["one_pixel_3d"] = (np.ones((1, 1, 1), np.int32), 3, 2)
    # 3-D: windows that hold several ids
    c["3d_2x5x7"] = (_noise((2, 5, 7), 4, 9), 3, 4)
    c["3d_5x6x10"] = (_noise((5, 6, 10), 5, 10), 3, 5)
    slabs = np.zeros((5, 6, 8), np.int32)
    slabs[1, 1:4, 2:6] = 1
    slabs[2, 1:4, 2:6] = 2                              # 1 and 2 touch only across a slice
    slabs[4, 0:2, 0:3] = 3
    c["3d_touch_across_z"] = (slabs, 3, 4)
    flat = _blobs((12, 19), 6, 11)
    c["flat_as_3d"] = (flat[None], 3, 7)                # Z == 1 under nd == 3: both slices next to it are outside
    c["flat_as_2d"] = (flat, 2, 7)
    c["3d_plane_above_a_tile_3x20x52"] = (_noise((3, 20, 52), 3, 14), 3, 3)     # Y * X = 1040 > 1024
    # seams: an object edge exactly on a multiple of 1024 pixels, along x and along y
    seam = np.ones((8, 512), np.int32)
    seam[2:] = 2                                        # pixel 1024 starts row 2
    seam[4:, 256:] = 3                                  # pixel 2048 + 256
    c["edge_on_tile_seam_8x512"] = (seam, 2, 4)
    rows = np.repeat(np.arange(1, 6, dtype=np.int32), 1024).reshape(5, 1024)
    c["one_id_per_tile_5x1024"] = (rows, 2, 6)
    # more tiles than the grid has blocks (MAX_GRID = 1024 tiles of 1024 pixels): blocks take two tiles
    c["second_trip_1100x1000"] = (_blobs((1100, 1000), 400, 12), 2, 401)
    c["blobs_3d_6x40x70"] = (_blobs((6, 40, 70), 20, 13), 3, 21)
    # labels
    c["all_background"] = (np.zeros((7, 19), np.int32), 2, 5)
    c["all_background_3d"] = (np.zeros((3, 7, 19), np.int32), 3, 5)
    c["one_object_fills_13x21"] = (np.full((13, 21), 3, np.int32), 2, 4)            # every contribution from edge windows
    c["one_object_fills_3x5x8"] = (np.full((3, 5, 8), 1, np.int32), 3, 2)
    yy, xx = np.indices((16, 16))
    c["checkerboard_one_id_16x16"] = (((yy + xx) % 2).astype(np.int32), 2, 2)
    c["checkerboard_two_ids_16x16"] = (((yy + xx) % 2 + 1).astype(np.int32), 2, 3)
    c["golden_2d"] = (_golden("2d"), 2, int(_golden("2d").max()) + 1)
    c["golden_2d_edge"] = (_golden("2d_edge"), 2, int(_golden("2d_edge").max()) + 1)
    c["golden_3d"] = (_golden("3d"), 3, int(_golden("3d").max()) + 1)
    shell, torus = _solids()
    c["shell_24"] = (shell, 3, 2)
    c["torus_24"] = (torus, 3, 2)
    # 4096 ids in 4 blocks of 256 LDS slots each: the overflow route straight to global memory
    c["distinct_64x64"] = (np.arange(1, 64 * 64 + 1, dtype=np.int32).reshape(64, 64), 2, 64 * 64 + 1)
    c["distinct_6x7x9"] = (np.arange(1, 6 * 7 * 9 + 1, dtype=np.int32).reshape(6, 7, 9), 3, 6 * 7 * 9 + 1)   # 8 ids a window
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_topology_equal_numpy(name, device):
    labels, nd, nid = CASES[name]
    assert_topology_equal(labels, nd, nid, device)


def test_topology_by_hand(device):
    counts, _ = call_topology(np.ones((1, 1), np.int32), 2, 2, device)
    assert counts[1].tolist() == [8, 4, 0, 4, 4]
    counts, _ = call_topology(np.ones((1, 1, 1), np.int32), 3, 2, device)
    assert counts[1].tolist() == [24, 24, 8, 8, 8]
    counts, _ = call_topology(np.zeros((7, 19), np.int32), 2, 5, device)
    assert not counts[1:].any()
    counts, _ = call_topology(np.full((13, 21), 3, np.int32), 2, 4, device)
    # a rectangle: 2 (13 + 21) faces, 4 diagonal neighbours at the corners and 2 along every unit of the edge
    assert counts[3].tolist() == [2 * 2 * (13 + 21), 4 + 2 * 2 * (12 + 20), 0, 4, 4] and not counts[1:3].any()
    counts, _ = call_topology(np.full((3, 5, 8), 1, np.int32), 3, 2, device)
    assert counts[1, 0] == 4 * 2 * (3 * 5 + 3 * 8 + 5 * 8) and counts[1, 3:].tolist() == [8, 8]
    counts, _ = call_topology(np.eye(2, dtype=np.int32), 2, 2, device)      # the 2 x 2 checkerboard: chi_hi 1, chi_lo 2
    assert counts[1].tolist() == [16, 6, 0, 4, 8]
    shell, torus = _solids()
    counts, _ = call_topology(shell, 3, 2, device)
    assert counts[1, 3:].tolist() == [16, 16]                               # one cavity: Euler number 2
    counts, _ = call_topology(torus, 3, 2, device)
    assert counts[1, 3:].tolist() == [0, 0]                                 # one tunnel: Euler number 0
    # Z == 1 under nd == 3 against the same map under nd == 2
    flat = CASES["flat_as_2d"][0]
    c2, _ = call_topology(flat, 2, 7, device)
    c3, _ = call_topology(flat[None], 3, 7, device)
    area = np.bincount(flat.ravel(), minlength=7)
    for i in range(1, 7):
        assert c3[i, 0] == 2 * c2[i, 0] + 8 * area[i]                      # the faces of both kinds, and 2 z faces a pixel
        assert c3[i, 3:].tolist() == (2 * c2[i, 3:]).tolist()              # the same Euler numbers
        assert area[i] == 0 or (c3[i, 2] > 0 and c2[i, 2] == 0)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", ["row_ends_9x5", "row_ends_3x1027", "3d_5x6x10", "edge_on_tile_seam_8x512", "golden_3d"])
def test_topology_unaligned_labels(name, offset, device):
    """a label map that does not start on a 16-byte boundary takes the 4-byte loads"""
    labels, nd, nid = CASES[name]
    assert_topology_equal(labels, nd, nid, device, offset=offset)


def test_topology_bad_labels(device):
    labels = _blobs((12, 70), 9, 5)
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[3, 7] = value
        lab[11, 69] = value
        lab[0, 0] = value
        counts = assert_topology_equal(lab, 2, 10, device)                  # bad == 1 and the guard words are checked there
        assert np.array_equal(counts[1:], ref_window_sums(np.where(lab == value, 0, lab), 2, 10)[1:])
        assert_topology_equal(np.stack([lab, labels]), 3, 10, device)


def test_topology_deterministic_and_stale_buffers(device):
    labels, nd, nid = CASES["second_trip_1100x1000"]
    first, _ = call_topology(labels, nd, nid, device)
    again, _ = call_topology(labels, nd, nid, device, fill=0x5C)
    zeros, _ = call_topology(labels, nd, nid, device, fill=0)
    assert np.array_equal(first[1:], again[1:]) and np.array_equal(first[1:], zeros[1:])
    noise = CASES["3d_5x6x10"]
    assert np.array_equal(call_topology(*noise, device)[0][1:], call_topology(*noise, device, fill=0xFF)[0][1:])


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(64, dtype=torch.int32, device=device)
    outs = {k: Out((1024,), np.uint64, device) for k in ("counts", "bad")}
    null = ctypes.c_void_p(0)

    def topology(nd=2, Z=1, Y=8, X=8, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(lab), counts=outs["counts"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_topology(p["labels"], nd, Z, Y, X, nid, p["counts"], p["bad"], st)

    refused = [lambda k=k: topology(**{k: null}) for k in ("labels", "counts", "bad")] + [
        lambda: topology(nd=1), lambda: topology(nd=4), lambda: topology(nd=0),
        lambda: topology(nd=2, Z=2, Y=4, X=8),                  # 2-D needs Z == 1
        lambda: topology(Z=0), lambda: topology(Y=0), lambda: topology(X=-1), lambda: topology(nd=3, Z=-2),
        lambda: topology(Y=65536, X=65536),                     # npix = 2^32
        lambda: topology(nd=3, Z=2, Y=46341, X=46341),          # just above 2^32
        lambda: topology(nid=0), lambda: topology(nid=-3), lambda: topology(nid=2 ** 24 + 1),
    ]
    for i, call in enumerate(refused):
        status = call()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert len(lib.clx_last_error()) > 0, f"case {i} left no message"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert topology() == 0 and topology(nd=3, Z=2, Y=4, X=8) == 0          # accepted with valid arguments
    torch.cuda.synchronize(device)
