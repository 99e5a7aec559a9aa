"""clx_region_cooccurrence through the C ABI against the restatement of tests/texture_ref.py (shifted views of the whole map
and np.add.at).  The counts are integers: counts, seen and bad must be EQUAL, and zero for absent ids.  Outputs and the
workspace are prefilled with 0xAB bytes and sit between guard zones that must stay untouched (test_gpu_measure.py's harness).

Sizes: csrc/region_texture.hip cuts a box into slabs of SLAB_PIXELS = 8192 box pixels (whole box rows) and runs MAIN_GRID =
2048 blocks; the maps that are one object (300 x 300: 12 slabs of 27 rows; 8 x 40 x 40: 2 slabs of 204 box rows) lie above
the first, the map of 2500 two-pixel objects above the second.  Both constants are read from the source below."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_measure import F32, F64, I32, Out, _dev
from texture_ref import directions, ref_bbox, ref_cooccurrence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {F32: np.float32, F64: np.float64, I32: np.int32}


def _constant(name):
    text = open(os.path.join(ROOT, "cellulus_amd", "csrc", "region_texture.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


SLAB_PIXELS, MAIN_GRID = _constant("SLAB_PIXELS"), _constant("MAIN_GRID")


def run(labels, raw, raw_type, nid, ids, lo, hi, levels, distance, device, bbox=None, nd=None):
    """one clx_region_cooccurrence call -> dict(counts, seen, bad); the guards of every output and the workspace are checked"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    nd = nd or labels.ndim
    Z, Y, X = (1,) * (3 - labels.ndim) + labels.shape
    raw = np.asarray(raw).astype(DTYPES[raw_type])
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    nrows = len(ids)
    bbox = ref_bbox(labels, nid) if bbox is None else np.asarray(bbox, dtype=np.int32)
    lib = _clx.load()
    nbytes = lib.clx_region_cooccurrence_workspace(labels.size, nrows)
    assert nbytes > 0
    ndir = 4 if nd == 2 else 13
    lab_d, raw_d, box_d = _dev(labels, device), _dev(raw, device), _dev(bbox, device)
    ids_d = _dev(ids if nrows else np.zeros(1, np.int32), device)
    outs = dict(counts=Out((max(nrows, 1), ndir, levels, levels), np.int32, device), seen=Out((max(nrows, 1),), np.int64, device),
                bad=Out((1,), np.int32, device), work=Out((nbytes,), np.uint8, device))
    status = lib.clx_region_cooccurrence(_clx.ptr(lab_d), _clx.ptr(raw_d), raw_type, nd, Z, Y, X, nid, _clx.ptr(box_d), _clx.ptr(ids_d),
                                         nrows, lo, hi, levels, distance, outs["counts"].ptr, outs["seen"].ptr, outs["bad"].ptr,
                                         outs["work"].ptr, nbytes, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    got = {k: v.get() for k, v in outs.items()}
    if nrows == 0:                                           # nothing of the one spare row is written
        assert (got["counts"].view(np.uint8) == 0xAB).all() and (got["seen"].view(np.uint8) == 0xAB).all()
    return dict(counts=got["counts"][:nrows], seen=got["seen"][:nrows], bad=got["bad"])


def check(labels, raw, raw_type, nid, ids, lo, hi, levels, distance, device, bbox=None, want_bad=None):
    labels = np.asarray(labels)
    raw_t = np.asarray(raw).astype(DTYPES[raw_type])
    got = run(labels, raw_t, raw_type, nid, ids, lo, hi, levels, distance, device, bbox)
    want = ref_cooccurrence(labels, raw_t, nid, ids, lo, hi, levels, distance, bbox)
    assert got["bad"][0] == want["bad"][0], (got["bad"], want["bad"])
    if want_bad is not None:
        assert got["bad"][0] == want_bad
    assert np.array_equal(got["seen"], want["seen"]), (got["seen"][:8], want["seen"][:8])
    assert np.array_equal(got["counts"], want["counts"]), np.argwhere(got["counts"] != want["counts"])[:5]
    return got


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: (g[f"{name}/labels"], g[f"{name}/raw"]) for name in ("2d", "2d_edge", "3d")}


G = _fixture()


def _raw_as(raw, raw_type):
    if raw_type == I32:
        return raw.astype(np.int32)
    if raw_type == F32:
        return raw.astype(np.float32) * np.float32(0.3)
    return raw.astype(np.float64) * 0.7 - 1234.5


@pytest.mark.parametrize("raw_type", [F32, F64, I32])
@pytest.mark.parametrize("name", sorted(G))
def test_fixture_maps(name, raw_type, device):
    labels, raw = G[name]
    raw = _raw_as(raw, raw_type)
    nid = int(labels.max()) + 1
    ids = np.unique(labels[labels > 0])
    lo, hi = float(raw[labels > 0].min()), float(raw[labels > 0].max())
    total = 0
    for levels in (2, 8, 32):
        for distance in (1, 3):
            got = check(labels, raw, raw_type, nid, ids, lo, hi, levels, distance, device, want_bad=0)
            total += int(got["counts"].sum())
            assert np.array_equal(got["seen"], np.bincount(labels.reshape(-1), minlength=nid)[ids])
    assert total > 0


def _rng_raw(shape, seed, scale=100.0):
    return np.random.default_rng(seed).random(shape) * scale


def test_no_wrap_across_rows_and_slices(device):
    """objects touching the left and right edges in rows (and slices) where p +- distance, taken on the linear index, lands on a
    pixel of the same id in the neighbouring row (slice)"""
    edges = np.zeros((6, 9), np.int32)
    edges[:, :2] = 1
    edges[:, -2:] = 1
    edges[2:4, 3:6] = 2
    full2 = np.ones((5, 7), np.int32)
    slabs = np.zeros((4, 3, 5), np.int32)
    slabs[:, -1, :] = 1                                      # the last row of every slice ...
    slabs[:, 0, :] = 1                                       # ... and the first row of the next: neighbours in memory
    full3 = np.ones((3, 4, 5), np.int32)
    for k, labels in enumerate((edges, full2, slabs, full3)):
        nid = int(labels.max()) + 1
        raw = _rng_raw(labels.shape, 10 + k)
        for distance in (1, 2, 3):
            got = check(labels, raw, F64, nid, np.arange(1, nid), 0.0, 100.0, 8, distance, device, want_bad=0)
            # the number of pairs by coordinates, without any linear index
            for r, i in enumerate(range(1, nid)):
                pts = {tuple(p) for p in np.argwhere(labels == i)}
                for kd, d in enumerate(directions(labels.ndim)):
                    n = sum(tuple(a + distance * b for a, b in zip(p, d)) in pts for p in pts)
                    assert int(got["counts"][r, kd].sum()) == n, (k, distance, i, d)


def test_touching_objects_small_objects_and_long_distances(device):
    halves = np.ones((6, 8), np.int32)
    halves[:, 4:] = 2                                        # touch along a face: the partner carries another id
    check(halves, _rng_raw((6, 8), 1), F32, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=0)
    halves3 = np.ones((4, 5, 6), np.int32)
    halves3[2:] = 2
    check(halves3, _rng_raw((4, 5, 6), 2), F32, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=0)
    small = np.zeros((5, 6), np.int32)
    small[1:4, 1:4] = 1                                      # 3 x 3
    small[4, 5] = 2                                          # one pixel
    for distance in (2, 3, 4, 7, 64):                        # up to the object, above it, above the map's extents
        got = check(small, _rng_raw((5, 6), 3), F64, 3, [1, 2], 0.0, 100.0, 4, distance, device, want_bad=0)
        assert got["counts"][1].sum() == 0 and got["seen"].tolist() == [9, 1]
        assert (got["counts"][0].sum() == 0) == (distance >= 3)
    one = check(np.ones((1, 1), np.int32), [[5.0]], F64, 2, [1], 0.0, 10.0, 2, 1, device)
    assert one["counts"].sum() == 0 and one["seen"].tolist() == [1]
    one = check(np.ones((1, 1, 1), np.int32), [[[5]]], I32, 2, [1], 0.0, 10.0, 2, 64, device)
    assert one["counts"].sum() == 0 and one["seen"].tolist() == [1]


def test_ids_absent_subsets_repeats_and_out_of_range(device):
    labels, raw = G["2d"]
    raw = raw.astype(np.int32)
    present = np.unique(labels[labels > 0])
    nid = int(labels.max()) + 40                             # ids above the largest present one are absent
    lo, hi = float(raw.min()), float(raw.max())
    absent = [i for i in range(1, nid) if i not in set(present.tolist())][:5]
    ids = [int(present[-1]), absent[0], int(present[0]), int(present[3]), absent[-1]]          # a subset, not ascending
    got = check(labels, raw, I32, nid, ids, lo, hi, 8, 1, device, want_bad=0)
    assert got["counts"][1].sum() == 0 and got["counts"][4].sum() == 0 and got["seen"][[1, 4]].tolist() == [0, 0]
    assert got["counts"][0].sum() > 0
    # a repeated id gets two equal rows; ids outside [1, nid) get rows of zeros and nothing is indexed with them
    ids = [int(present[2]), 0, -5, nid, 2 ** 30, int(present[2]), -2 ** 31]
    got = check(labels, raw, I32, nid, ids, lo, hi, 8, 3, device, want_bad=0)
    assert np.array_equal(got["counts"][0], got["counts"][5]) and got["counts"][0].sum() > 0
    assert got["counts"][[1, 2, 3, 4, 6]].sum() == 0 and got["seen"][[1, 2, 3, 4, 6]].tolist() == [0] * 5
    # no ids at all: bad is still set from the map
    got = check(labels, raw, I32, nid, [], lo, hi, 8, 1, device, want_bad=0)
    assert got["counts"].shape[0] == 0
    # all of them, nrows == nid - 1
    check(labels, raw, I32, nid, np.arange(1, nid)[::-1], lo, hi, 2, 1, device, want_bad=0)


@pytest.mark.parametrize("shape", [(300, 300), (8, 40, 40)])
def test_one_object_filling_the_map_is_shared_by_many_blocks(shape, device):
    rows = int(np.prod(shape[:-1]))
    assert rows > max(1, SLAB_PIXELS // shape[-1]), "the box must be more than one slab"
    labels = np.ones(shape, np.int32)
    raw = _rng_raw(shape, 21)
    got = check(labels, raw, F32, 2, [1], 0.0, 100.0, 32, 1, device, want_bad=0)
    assert got["seen"].tolist() == [labels.size]
    check(labels, raw, F32, 3, [1, 1], 0.0, 100.0, 8, 2, device, want_bad=0)     # nid 3: two rows need nrows < nid
    # a second object inside, so that the big one's box holds pixels of another id
    labels[..., 100 % shape[-2]:, 7:19] = 2
    check(labels, raw, F64, 3, [2, 1], 0.0, 100.0, 8, 1, device, want_bad=0)


def test_more_objects_than_blocks(device):
    Y, X = 50, 100
    labels = (np.arange(Y * X).reshape(Y, X) // 2 + 1).astype(np.int32)         # 2500 objects of two pixels: one pair each
    nid = Y * X // 2 + 1
    assert nid - 1 > MAIN_GRID
    raw = np.random.default_rng(4).integers(0, 2, (Y, X)).astype(np.int32)
    got = check(labels, raw, I32, nid, np.arange(1, nid), 0.0, 1.0, 2, 1, device, want_bad=0)
    assert (got["counts"].sum(axis=(1, 2, 3)) == 1).all() and (got["counts"][:, 1:].sum() == 0)


def test_bin_edges_ranges_and_clamps(device):
    labels = np.ones((4, 33), np.int32)
    labels[3, 30:] = 0
    edges = np.tile(np.arange(33) / 32.0, (4, 1))            # every edge of 32 levels over [0, 1], exact in float32 too
    for raw_type in (F32, F64):
        got = check(labels, edges, raw_type, 2, [1], 0.0, 1.0, 32, 1, device, want_bad=0)
        # along (0,1) level a meets level a + 1, and 31 meets 31 (v == hi): 4 rows, the last without its three last pairs
        assert got["counts"][0, 0, 5, 6] == 4 and got["counts"][0, 0, 31, 31] == 3 and got["counts"][0, 0, 30, 31] == 3
    ints = np.tile(np.arange(33), (4, 1))
    check(labels, ints, I32, 2, [1], 0.0, 32.0, 32, 1, device, want_bad=0)
    check(labels, ints, I32, 2, [1], -7.0, 26.0, 11, 2, device, want_bad=0)                   # 33 / 11: edges at multiples of 3
    # hi == lo: every pixel at level 0
    got = check(labels, ints, I32, 2, [1], 5.0, 5.0, 8, 1, device, want_bad=0)
    assert got["counts"][0, :, 0, 0].sum() == got["counts"].sum() > 0
    # a range narrower than the data: both clamps are hit
    got = check(labels, ints, I32, 2, [1], 10.0, 20.0, 4, 1, device, want_bad=0)
    assert got["counts"][0, 0, 0, 0] > 20 and got["counts"][0, 0, 3, 3] > 20
    check(labels, edges * 1e300, F64, 2, [1], -1e300, 1e308, 32, 1, device, want_bad=0)        # huge but finite quotients


def test_non_finite_values_and_bad_labels(device):
    labels = np.zeros((6, 8), np.int32)
    labels[1:5, 1:6] = 1
    labels[0, 7] = 2
    raw = _rng_raw((6, 8), 8).astype(np.float32)
    outside = raw.copy()
    outside[5, 0], outside[0, 0], outside[5, 7] = np.nan, np.inf, -np.inf           # background: ignored
    clean = check(labels, raw, F32, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=0)
    got = check(labels, outside, F32, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=0)
    assert np.array_equal(got["counts"], clean["counts"])
    for value in (np.nan, np.inf, -np.inf):
        for raw_type in (F32, F64):
            inside = raw.copy()
            inside[2, 3] = value
            got = check(labels, inside, raw_type, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=2)
            # the 8 pairs of that pixel (4 as p, 4 as q) are absent, the pixel is still seen
            assert clean["counts"][0].sum() - got["counts"][0].sum() == 8 and got["seen"].tolist() == [20, 1]
    # labels outside [0, nid): bit 0, they match no id
    wild = labels.copy()
    wild[5, 5], wild[5, 6], wild[0, 0] = -3, 3, 2 ** 31 - 1
    got = check(wild, raw, F32, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=1)
    assert np.array_equal(got["counts"], clean["counts"])
    inside = raw.copy()
    inside[5, 5], inside[2, 2] = np.nan, np.nan              # under the label -3 (no object id: ignored) and inside object 1
    check(wild, inside, F32, 3, [1, 2], 0.0, 100.0, 8, 1, device, want_bad=3)


def test_stale_and_wrong_boxes(device):
    labels, raw = G["2d"]
    raw = raw.astype(np.int32)
    nid = int(labels.max()) + 1
    ids = np.unique(labels[labels > 0])
    lo, hi = float(raw.min()), float(raw.max())
    area = np.bincount(labels.reshape(-1), minlength=nid)
    good = ref_bbox(labels, nid)
    big = int(ids[np.argmax(area[ids])])
    stale = good.copy()
    stale[big, 4] -= 1                                       # one row short
    stale[big, 2] += 1                                       # one column short
    got = check(labels, raw, I32, nid, ids, lo, hi, 8, 1, device, bbox=stale, want_bad=0)
    r = int(np.searchsorted(ids, big))
    assert 0 < got["seen"][r] < area[big] and np.array_equal(np.delete(got["seen"], r), np.delete(area[ids], r))
    # a box larger than the object is not stale: the same counts
    wide = good.copy()
    wide[big, :3] = 0
    wide[big, 3:] = (0, labels.shape[0] - 1, labels.shape[1] - 1)
    assert np.array_equal(check(labels, raw, I32, nid, ids, lo, hi, 8, 1, device, bbox=wide)["seen"], area[ids])
    # boxes that reach outside the map, in every field: a row of zeros, nothing out of bounds is formed
    Y, X = labels.shape
    for field, value in ((0, -1), (0, 1), (3, 1), (1, -1), (4, Y), (2, -2 ** 31), (5, X), (5, 2 ** 31 - 1), (4, 2 ** 31 - 1), (1, 2 ** 31 - 1)):
        wrong = good.copy()
        wrong[big, field] = value
        got = check(labels, raw, I32, nid, ids, lo, hi, 8, 3, device, bbox=wrong, want_bad=0)
        assert got["seen"][r] == 0 and got["counts"][r].sum() == 0
    garbage = np.random.default_rng(9).integers(-2 ** 31, 2 ** 31, size=good.shape).astype(np.int32)
    check(labels, raw, I32, nid, ids, lo, hi, 8, 1, device, bbox=garbage, want_bad=0)
    labels3, raw3 = G["3d"]
    nid3 = int(labels3.max()) + 1
    wrong = ref_bbox(labels3, nid3)
    wrong[1, 3] = labels3.shape[0]
    wrong[2, 0] += 1
    check(labels3, raw3.astype(np.int32), I32, nid3, np.arange(1, nid3), lo, hi, 8, 1, device, bbox=wrong, want_bad=0)


def test_smooth_ramp_where_all_pairs_share_a_cell(device):
    """every pair of an object lands in one or two cells of a matrix: the LDS atomics of a wave all hit the same address"""
    yy, xx = np.indices((96, 200))
    labels = np.ones((96, 200), np.int32)
    labels[:, 150:] = 2
    labels[90:, :] = 0
    ramp = xx * 0.01 + yy * 0.001                            # 0 .. 2.1 over a range of 16: two levels in the whole map
    got = check(labels, ramp, F32, 3, [1, 2], 0.0, 16.0, 8, 1, device, want_bad=0)
    assert np.count_nonzero(got["counts"][0, 0]) <= 3 and got["counts"][0, 0, 0, 0] > 10000
    check(labels, np.zeros((96, 200)), F64, 3, [1, 2], 0.0, 16.0, 32, 2, device, want_bad=0)
    vol = np.ones((6, 40, 50), np.int32)
    check(vol, np.indices(vol.shape)[2] * 0.01, F32, 2, [1], 0.0, 16.0, 32, 1, device, want_bad=0)


def test_refused_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    null = ctypes.c_void_p(0)
    lab = _dev(np.zeros(64, np.int32), device)
    raw = _dev(np.zeros(64, np.float64), device)
    box = _dev(np.zeros((4, 6), np.int32), device)
    ids = _dev(np.ones(3, np.int32), device)
    need = lib.clx_region_cooccurrence_workspace(64, 3)
    outs = dict(counts=Out((3, 13, 32, 32), np.int32, device), seen=Out((3,), np.int64, device), bad=Out((1,), np.int32, device),
                workspace=Out((need,), np.uint8, device))

    def message():
        return lib.clx_last_error().decode()

    def call(raw_type=F64, nd=2, Z=1, Y=8, X=8, nid=4, nrows=3, lo=0.0, hi=1.0, levels=8, distance=1, nbytes=None, **ptrs):
        p = dict(labels=_clx.ptr(lab), raw=_clx.ptr(raw), bbox=_clx.ptr(box), ids=_clx.ptr(ids), counts=outs["counts"].ptr,
                 seen=outs["seen"].ptr, bad=outs["bad"].ptr, workspace=outs["workspace"].ptr)
        p.update(ptrs)
        return lib.clx_region_cooccurrence(p["labels"], p["raw"], raw_type, nd, Z, Y, X, nid, p["bbox"], p["ids"], nrows, lo, hi, levels,
                                           distance, p["counts"], p["seen"], p["bad"], p["workspace"], need if nbytes is None else nbytes, st)

    odd = ctypes.c_void_p(outs["workspace"].ptr.value + 4)
    inf, nan = float("inf"), float("nan")
    refused = [(lambda k=k: call(**{k: null}), "null") for k in ("labels", "raw", "bbox", "ids", "counts", "seen", "bad", "workspace")] + [
        (lambda: call(raw_type=3), "raw_type"), (lambda: call(raw_type=-1), "raw_type"),
        (lambda: call(nd=1), "nd must"), (lambda: call(nd=4), "nd must"), (lambda: call(nd=2, Z=2, Y=4), "Z == 1"),
        (lambda: call(Y=0), "extents"), (lambda: call(X=-8), "extents"), (lambda: call(nd=3, Z=0), "extents"),
        (lambda: call(Y=2 ** 16, X=2 ** 15), "2^31"), (lambda: call(nd=3, Z=2 ** 11, Y=2 ** 10, X=2 ** 10), "2^31"),
        (lambda: call(nd=3, Z=2 ** 30, Y=2 ** 30, X=2 ** 30), "2^31"),
        (lambda: call(nid=0, nrows=0), "nid"), (lambda: call(nid=2 ** 24 + 1), "nid"), (lambda: call(nid=-1), "nid"),
        (lambda: call(nrows=-1), "nrows"), (lambda: call(nrows=4), "nrows"),
        (lambda: call(levels=1), "levels"), (lambda: call(levels=33), "levels"), (lambda: call(levels=-8), "levels"),
        (lambda: call(distance=0), "distance"), (lambda: call(distance=65), "distance"),
        (lambda: call(lo=nan), "finite"), (lambda: call(hi=inf), "finite"), (lambda: call(lo=-inf), "finite"), (lambda: call(hi=nan), "finite"),
        (lambda: call(lo=1.0, hi=0.5), "below lo"),
        (lambda: call(nbytes=need - 1), "workspace_bytes"), (lambda: call(nbytes=0), "workspace_bytes"),
        (lambda: call(workspace=odd), "aligned"),
    ]
    for i, (c, word) in enumerate(refused):
        status = c()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message().startswith("clx_region_cooccurrence") and word in message(), f"case {i}: {message()!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    # accepted at the ends of every range: a background-only map
    assert call(levels=2, distance=64) == 0 and call(levels=32, lo=0.5, hi=0.5) == 0 and call(nrows=0) == 0, message()
    assert call(nd=3, Z=1, levels=32) == 0 and call(nd=3, Z=4, Y=4, X=4, raw_type=F32) == 0, message()
    torch.cuda.synchronize(device)
    assert outs["bad"].get()[0] == 0 and outs["seen"].get().tolist() == [0, 0, 0] and (outs["counts"].get()[:, :, :8, :8] == 0).all()
    outs["workspace"].get()
