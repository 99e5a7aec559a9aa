"""clx_region_hull through the C ABI against the restatement of tests/hull_ref.py (all corner points of every object, a
monotone chain in Python ints; none of the kernel's row spans).  Everything is integer work: the five integers A2 NV F2
C L2 must be EQUAL for every id from 1 up, and zero for absent ids.  The outputs and the workspace are prefilled with 0xAB
bytes (or other garbage) and sit between guard words that must stay untouched; bbox and row_base are formed here from
NumPy, so the kernel is tested alone.

nid = 2^24 is not run with real buffers: hull, bbox and row_base alone are 1.2 GB at that size, more than a test of this
suite allocates; the refused-argument test covers the bound itself."""

import ctypes
import os

import numpy as np
import pytest
import torch

from hull_ref import boxes_and_rows, ref_hull, rows_of, shapes
from test_gpu_measure import GUARD, Out, _blobs, _dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_LABEL, BAD_BOX = 1, 2


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))[f"{name}/labels"]


def call_hull(labels, nd, nid, device, offset=0, fill=0xAB, bbox=None, row_base=None, rows=None):
    """-> (hull int64 (nid, 5), bad) as the entry point left them; the guard words of the outputs and of the workspace
    are checked.  bbox / row_base / rows default to those of the map."""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    Z, Y, X = (1,) * (3 - labels.ndim) + labels.shape
    if bbox is None:
        bbox, row_base, rows = boxes_and_rows(labels, nid)
    lib = _clx.load()
    nbytes = lib.clx_region_hull_workspace(rows)
    assert nbytes >= 8 * rows and nbytes > 0
    lab = _dev(labels, device, offset)
    bbox_d, base_d = _dev(bbox.astype(np.int32), device), _dev(row_base.astype(np.int64), device)
    outs = dict(hull=Out((nid, 5), np.int64, device), bad=Out((1,), np.int32, device), work=Out((nbytes,), np.uint8, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = lib.clx_region_hull(_clx.ptr(lab), nd, Z, Y, X, nid, _clx.ptr(bbox_d), _clx.ptr(base_d), rows, outs["work"].ptr,
                                 nbytes, outs["hull"].ptr, outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    outs["work"].get()
    return outs["hull"].get(), int(outs["bad"].get()[0])


_WANT = {}


def want_hull(labels, nd, nid):
    """ref_hull, computed once per map and left unchanged"""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    key = (labels.shape, nd, nid, labels.tobytes())
    if key not in _WANT:
        _WANT[key] = ref_hull(labels, nd, nid)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def assert_hull_equal(labels, nd, nid, device, **kw):
    hull, bad = call_hull(labels, nd, nid, device, **kw)
    want = want_hull(labels, nd, nid)
    differ = np.flatnonzero((hull != want).any(axis=1))                # row 0 and absent ids: zero
    assert len(differ) == 0, (len(differ), [(int(i), hull[i].tolist(), want[i].tolist()) for i in differ[:4]])
    lab = np.asarray(labels)
    assert bad == (BAD_LABEL if ((lab < 0) | (lab >= nid)).any() else 0)
    return hull


def _noise(shape, ids, seed):
    """every pixel its own draw of `ids` ids: every object is scattered, the boxes overlap, rows inside a box are empty"""
    return np.random.default_rng(seed).integers(0, ids, size=shape).astype(np.int32)


def _small_blobs(shape, n, seed, size=40):
    """n discs and boxes of at most `size` pixels across, all over a 2-D map (the restatement walks every corner point
    in Python: the objects stay small where the map is large)"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.int32)
    for i in range(1, n + 1):
        cy, cx = (int(rng.integers(0, s)) for s in shape)
        ry, rx = (int(rng.integers(1, size // 2)) for _ in range(2))
        win = lab[max(0, cy - ry):cy + ry + 1, max(0, cx - rx):cx + rx + 1]        # a view: the object is drawn in place
        if i % 2:
            yy, xx = np.indices(win.shape)
            yy, xx = yy + max(0, cy - ry) - cy, xx + max(0, cx - rx) - cx
            win[yy * yy * rx * rx + xx * xx * ry * ry <= ry * ry * rx * rx] = i
        else:
            win[:] = i
    return lab


def _ball(n=24):
    c = (n - 1) / 2.0
    zz, yy, xx = np.indices((n, n, n)) - c
    return (zz ** 2 + yy ** 2 + xx ** 2 <= 100).astype(np.int32)


def _cases():
    c = {}
    # row ends: a lane's 4 pixels straddle rows unless X is a multiple of 4
    for X in (1, 2, 3, 5):
        c[f"row_ends_9x{X}"] = (_noise((9, X), 4, X), 2, 4)
    c["row_ends_3x1027"] = (_noise((3, 1027), 3, 7), 2, 3)
    c["one_row_1x37"] = (_noise((1, 37), 4, 8), 2, 4)
    sparse = _noise((40, 45), 60, 15)
    c["sparse_noise_40x45"] = (np.where(sparse < 5, sparse, 0).astype(np.int32), 2, 5)      # empty rows inside every box
    # seams: an object edge exactly on a multiple of 1024 pixels, along x and along y
    seam = np.ones((8, 512), np.int32)
    seam[2:] = 2                                        # pixel 1024 starts row 2
    seam[4:, 256:] = 3                                  # pixel 2048 + 256
    c["edge_on_tile_seam_8x512"] = (seam, 2, 4)
    rows = np.repeat(np.arange(1, 6, dtype=np.int32), 1024).reshape(5, 1024)
    c["one_id_per_tile_5x1024"] = (rows, 2, 6)
    # more tiles than MAX_GRID = 1024 tiles of 1024 pixels (where the sibling kernels start their second trip), and more
    # than the HULL_MAX_GRID = 4096 blocks of the span pass, whose blocks then take two tiles
    c["above_max_grid_1100x1000"] = (_small_blobs((1100, 1000), 60, 12), 2, 61)
    c["second_trip_2100x2000"] = (_small_blobs((2100, 2000), 80, 16), 2, 81)
    for name, (labels, nid) in shapes().items():
        c[name] = (labels, 2, nid)
    c["all_background"] = (np.zeros((7, 19), np.int32), 2, 5)
    c["all_background_3d"] = (np.zeros((3, 7, 19), np.int32), 3, 5)
    # 3-D
    c["3d_2x5x7"] = (_noise((2, 5, 7), 4, 9), 3, 4)
    c["3d_5x6x10"] = (_noise((5, 6, 10), 5, 10), 3, 5)
    slabs = np.zeros((5, 6, 8), np.int32)
    slabs[1, 1:4, 2:6] = 1
    slabs[2, 1:4, 2:6] = 2                              # 1 and 2 touch only across a slice
    slabs[4, 0:2, 0:3] = 3
    c["3d_touch_across_z"] = (slabs, 3, 4)
    pieces = np.zeros((6, 5, 9), np.int32)
    pieces[0, 1:3, 1:4] = 2
    pieces[4:, 3:, 6:] = 2                              # one id in two pieces: slices 1 .. 3 of its box are empty
    c["3d_empty_slices_in_a_box"] = (pieces, 3, 3)
    flat = _blobs((12, 19), 6, 11)
    c["flat_as_3d"] = (flat[None], 3, 7)
    c["flat_as_2d"] = (flat, 2, 7)
    c["ball_24"] = (_ball(), 3, 2)
    c["one_voxel"] = (np.ones((1, 1, 1), np.int32), 3, 2)
    c["blobs_3d_6x40x70"] = (_blobs((6, 40, 70), 20, 13), 3, 21)
    for name in ("2d", "2d_edge", "3d"):
        g = _golden(name)
        c[f"golden_{name}"] = (g, g.ndim, int(g.max()) + 1)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hull_equal_restatement(name, device):
    labels, nd, nid = CASES[name]
    assert_hull_equal(labels, nd, nid, device)


def test_hull_by_hand(device):
    hull, _ = call_hull(np.ones((1, 1), np.int32), 2, 2, device)
    assert hull[1].tolist() == [2, 4, 2, 1, 1]                                  # area 1, Feret max sqrt 2, min 1
    hull, _ = call_hull(np.ones((1, 1, 1), np.int32), 3, 2, device)
    assert hull[1].tolist() == [0, 0, 3, 0, 0]
    hull, _ = call_hull(CASES["bar_1x40"][0], 2, 2, device)
    assert hull[1].tolist() == [80, 4, 1601, 40, 1600]                          # the narrowest there is: width 40 / 40
    hull, _ = call_hull(CASES["trapezoid_tie"][0], 2, 2, device)
    assert hull[1].tolist() == [40, 6, 145, 8, 16]                              # the tie goes to the shorter edge
    hull, _ = call_hull(CASES["checkerboard_one_id_15x15"][0], 2, 2, device)
    assert hull[1].tolist() == [450, 4, 450, 225, 225]                          # the hull is the box
    hull, _ = call_hull(np.zeros((7, 19), np.int32), 2, 5, device)
    assert not hull.any()
    # Z == 1 under nd == 3 against the same map under nd == 2
    flat = CASES["flat_as_2d"][0]
    h2, _ = call_hull(flat, 2, 7, device)
    h3, _ = call_hull(flat[None], 3, 7, device)
    present = np.bincount(flat.ravel(), minlength=7) > 0
    present[0] = False
    assert present.any() and np.array_equal(h3[present, 2], h2[present, 2] + 1)
    assert not h3[:, [0, 1, 3, 4]].any() and not h3[~present].any() and not h2[~present].any()


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("name", ["row_ends_9x5", "row_ends_3x1027", "3d_5x6x10", "edge_on_tile_seam_8x512", "golden_3d"])
def test_hull_unaligned_labels(name, offset, device):
    """a label map that does not start on a 16-byte boundary takes the 4-byte loads"""
    labels, nd, nid = CASES[name]
    assert_hull_equal(labels, nd, nid, device, offset=offset)


def test_hull_bad_labels(device):
    labels = _blobs((12, 70), 9, 5)
    clean, bad = call_hull(labels, 2, 10, device)
    assert bad == 0
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[3, 7] = value
        lab[11, 69] = value
        lab[0, 0] = value
        # the boxes are those of the map without the bad pixels: they are background
        hull = assert_hull_equal(lab, 2, 10, device)                        # bad == 1 and the guard words are checked there
        assert np.array_equal(hull, ref_hull(np.where(lab == value, 0, lab), 2, 10))
        untouched = [i for i in range(1, 10) if not (labels == i)[[3, 11, 0], [7, 69, 0]].any()]
        assert untouched and np.array_equal(hull[untouched], clean[untouched])
        assert_hull_equal(np.stack([lab, labels]), 3, 10, device)


def test_hull_stale_box_sets_bit_1_and_spares_the_others(device):
    labels, nd, nid = CASES["golden_2d"]
    want = want_hull(labels, nd, nid)
    bbox, row_base, rows = boxes_and_rows(labels, nid)
    victim = int(np.argmax(bbox[:, 4] - bbox[:, 1]))                         # the tallest object
    for edit in ("ymax", "ymin", "xmax", "row_base_past_the_end", "rows_too_few", "box_outside_the_image"):
        b, base, n, hit = bbox.copy(), row_base.copy(), rows, victim
        if edit == "ymax":
            b[victim, 4] -= 1                                               # one row too small, row_base formed from it
            base, n = rows_of(b)
        elif edit == "ymin":
            b[victim, 1] += 1
            base, n = rows_of(b)
        elif edit == "xmax":
            b[victim, 5] -= 1
        elif edit == "row_base_past_the_end":
            base[victim] = rows - 1
        elif edit == "rows_too_few":                                        # the last object's rows end past the count
            hit = int(np.argmax(row_base))
            n = rows - 1
        else:
            b[victim, 4] = labels.shape[0]                                  # ymax == Y
        hull, bad = call_hull(labels, nd, nid, device, bbox=b, row_base=base, rows=n)       # the guards are checked there
        assert bad == BAD_BOX, (edit, bad)
        others = [i for i in range(1, nid) if i != hit]
        assert np.array_equal(hull[others], want[others]), edit
    # in 3-D: a box one slice too small
    labels, nd, nid = CASES["golden_3d"]
    want = want_hull(labels, nd, nid)
    bbox, _, _ = boxes_and_rows(labels, nid)
    victim = int(np.argmax(bbox[:, 3] - bbox[:, 0]))
    bbox[victim, 3] -= 1
    base, n = rows_of(bbox)
    hull, bad = call_hull(labels, nd, nid, device, bbox=bbox, row_base=base, rows=n)
    others = [i for i in range(1, nid) if i != victim]
    assert bad == BAD_BOX and np.array_equal(hull[others], want[others])
    # both at once
    lab = labels.copy()
    lab[0, 0, 0] = nid
    _, bad = call_hull(lab, nd, nid, device, bbox=bbox, row_base=base, rows=n)
    assert bad == BAD_LABEL | BAD_BOX


def test_hull_deterministic_and_stale_buffers(device):
    labels, nd, nid = CASES["second_trip_2100x2000"]
    first, _ = call_hull(labels, nd, nid, device)
    again, _ = call_hull(labels, nd, nid, device, fill=0x5C)
    zeros, _ = call_hull(labels, nd, nid, device, fill=0)
    assert np.array_equal(first, again) and np.array_equal(first, zeros)
    noise = CASES["3d_5x6x10"]
    assert np.array_equal(call_hull(*noise, device)[0], call_hull(*noise, device, fill=0xFF)[0])


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(64, dtype=torch.int32, device=device)
    bbox = torch.zeros((4, 6), dtype=torch.int32, device=device)
    base = torch.zeros(4, dtype=torch.int64, device=device)
    outs = {k: Out((1024,), np.uint64, device) for k in ("workspace", "hull", "bad")}
    null = ctypes.c_void_p(0)

    def hull(nd=2, Z=1, Y=8, X=8, nid=4, rows=24, nbytes=8192, **ptrs):
        p = dict(labels=_clx.ptr(lab), bbox=_clx.ptr(bbox), row_base=_clx.ptr(base), workspace=outs["workspace"].ptr,
                 hull=outs["hull"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_hull(p["labels"], nd, Z, Y, X, nid, p["bbox"], p["row_base"], rows, p["workspace"], nbytes,
                                   p["hull"], p["bad"], st)

    need = lib.clx_region_hull_workspace(24)
    assert 0 < need <= 8192
    odd = ctypes.c_void_p(outs["workspace"].ptr.value + 4)
    refused = [(lambda k=k: hull(**{k: null}), "null") for k in ("labels", "bbox", "row_base", "workspace", "hull", "bad")] + [
        (lambda: hull(nd=1), "nd"), (lambda: hull(nd=4), "nd"), (lambda: hull(nd=0), "nd"),
        (lambda: hull(nd=2, Z=2, Y=4, X=8), "Z == 1"),                      # 2-D needs Z == 1
        (lambda: hull(Z=0), "shape"), (lambda: hull(Y=0), "shape"), (lambda: hull(X=-1), "shape"), (lambda: hull(nd=3, Z=-2), "shape"),
        (lambda: hull(Y=65536, X=65536), "Z * Y * X"),                      # npix = 2^32
        (lambda: hull(nd=3, Z=2, Y=46341, X=46341), "Z * Y * X"),           # just above 2^32
        (lambda: hull(nid=0), "nid"), (lambda: hull(nid=-3), "nid"), (lambda: hull(nid=2 ** 24 + 1), "nid"),
        (lambda: hull(rows=-1), "rows"), (lambda: hull(rows=3 * 8 + 1, nbytes=8192), "rows"),      # more than (nid - 1) Z Y
        (lambda: hull(nbytes=need - 1), "workspace"), (lambda: hull(nbytes=0), "workspace"),
        (lambda: hull(workspace=odd), "workspace"),
        (lambda: hull(Y=46341, X=46340), "(Y + 1) * (X + 1)"),              # npix < 2^32 but (Y+1)(X+1) > 2^31
        (lambda: hull(Y=1, X=2 ** 30), "2^30"), (lambda: hull(Y=2 ** 30, X=1), "2^30"),
        (lambda: hull(nd=3, Z=2 ** 30, Y=1, X=1), "2^30"),
    ]
    for i, (call, word) in enumerate(refused):
        status = call()
        message = lib.clx_last_error().decode() if isinstance(lib.clx_last_error(), bytes) else str(lib.clx_last_error())
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message.startswith("clx_region_hull") and word in message, f"case {i}: {message!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert hull() == 0 and hull(nd=3, Z=2, Y=4, X=8) == 0 and hull(rows=0) == 0     # accepted with valid arguments
    torch.cuda.synchronize(device)
    assert int(outs["bad"].get()[:1].view(np.int32)[0]) == 0
