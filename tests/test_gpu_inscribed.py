"""clx_label_distance_sq and clx_region_inscribed through the C ABI against the restatements of tests/inscribed_ref.py
(scipy's distance transform of every object's own mask on a crop; a sort for the per-object maximum).  Everything is integer
work: every element of the distance map and every output row must be EQUAL.  The outputs and the workspace are prefilled
with 0xAB bytes (or other garbage) and sit between guard words that must stay untouched.  clx_region_inscribed is also run
alone, on distance maps formed in NumPy."""

import ctypes

import numpy as np
import pytest
import torch

from inscribed_ref import DIST_INF, ref_distance_sq, ref_inscribed
from test_gpu_hull import _ball, _noise, _small_blobs
from test_gpu_measure import GUARD, Out, _blobs, _dev

pytestmark = pytest.mark.gpu

BAD_LABEL, BAD_DISTANCE = 1, 2


def call_distance(labels, nd, edge, device, offset=0, fill=0xAB):
    """-> dist_sq int32 in the shape of `labels` (ndim == nd) as the entry point left it; the guard words of the output and
    of the workspace are checked"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    assert labels.ndim == nd
    Z, Y, X = (1,) * (3 - nd) + labels.shape
    lib = _clx.load()
    nbytes = lib.clx_label_distance_workspace(labels.size)
    assert nbytes == 4 * labels.size
    lab = _dev(labels, device, offset)
    outs = dict(dist=Out(labels.shape, np.int32, device), work=Out((nbytes,), np.uint8, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    status = lib.clx_label_distance_sq(_clx.ptr(lab), nd, Z, Y, X, edge, outs["dist"].ptr, outs["work"].ptr, nbytes,
                                       _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    outs["work"].get()
    return outs["dist"].get()


def call_inscribed(labels, dist_sq, nid, device, offset=0, fill=0xAB):
    """-> (out int64 (nid, 3), bad) as the entry point left them; guard words checked"""
    from cellulus_amd import _clx

    lab = _dev(np.asarray(labels, dtype=np.int32), device, offset)
    dist = _dev(np.asarray(dist_sq, dtype=np.int32), device, offset)
    outs = dict(out=Out((nid, 3), np.int64, device), bad=Out((1,), np.int32, device))
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    lib = _clx.load()
    status = lib.clx_region_inscribed(_clx.ptr(lab), _clx.ptr(dist), lab.numel(), nid, outs["out"].ptr, outs["bad"].ptr,
                                      _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return outs["out"].get(), int(outs["bad"].get()[0])


_WANT = {}


def want_distance(labels, edge):
    """ref_distance_sq, computed once per map and left unchanged"""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    key = (labels.shape, edge, labels.tobytes())
    if key not in _WANT:
        _WANT[key] = ref_distance_sq(labels, edge)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def assert_distance_equal(labels, nd, edge, device, **kw):
    got = call_distance(labels, nd, edge, device, **kw)
    want = want_distance(labels, edge)
    differ = np.argwhere(got != want)
    assert len(differ) == 0, (len(differ), [(tuple(int(v) for v in p), int(got[tuple(p)]), int(want[tuple(p)])) for p in differ[:4]])
    return got


def _disc(shape, centre, radius):
    yy, xx = np.indices(shape)
    return ((yy - centre[0]) ** 2 + (xx - centre[1]) ** 2 <= radius * radius).astype(np.int32)


def _cases():
    c = {}
    # row ends: the outward search along x meets one or both ends of the row at once
    for X in (1, 2, 3, 5, 63, 65):
        c[f"row_ends_7x{X}"] = (_noise((7, X), 3, X), 2)
        c[f"blobs_7x{X}"] = (_blobs((7, X), 3, 20 + X), 2)
    c["one_row_1x37"] = (_noise((1, 37), 3, 8), 2)
    c["one_row_blobs_1x37"] = (_blobs((1, 37), 4, 9), 2)
    c["one_pixel"] = (np.ones((1, 1), np.int32), 2)
    c["one_background_pixel"] = (np.zeros((1, 1), np.int32), 2)
    c["all_background"] = (np.zeros((7, 19), np.int32), 2)
    # objects that touch with no background between them: a binary transform gives other numbers on these
    halves = np.ones((9, 14), np.int32)
    halves[:, 7:] = 2
    c["two_half_planes"] = (halves, 2)
    yy, xx = np.indices((24, 24))
    c["checkerboard_4_colours"] = (((yy // 6) % 2 * 2 + (xx // 6) % 2 + 1).astype(np.int32), 2)
    c["noise_no_background_17x19"] = (_noise((17, 19), 3, 31) + 1, 2)
    # the stop rule: the nearest candidate of a pixel near the centre lies on a diagonal, d^2 = a^2 + b^2 with both large
    c["disc_20_in_48"] = (_disc((48, 48), (24, 23), 20), 2)
    c["disc_20_cut_by_the_border"] = (_disc((48, 48), (8, 41), 20), 2)
    c["disc_in_a_sheet"] = (_disc((48, 48), (22, 25), 15) + 1, 2)                   # no background: disc 2 inside object 1
    # one value everywhere: no candidate without `edge`
    c["one_value_9x11"] = (np.full((9, 11), 5, np.int32), 2)
    c["one_value_3x4x5"] = (np.full((3, 4, 5), 2, np.int32), 3)
    c["one_value_1x4x5_z_counted"] = (np.full((1, 4, 5), 2, np.int32), 3)
    # 3-D
    c["3d_noise_5x7x9"] = (_noise((5, 7, 9), 3, 10) + 1, 3)
    c["3d_noise_background_5x7x9"] = (_noise((5, 7, 9), 3, 11), 3)
    c["3d_ball_24"] = (_ball(), 3)
    c["3d_flat_1x12x19"] = (_blobs((12, 19), 6, 11)[None], 3)
    slabs = np.zeros((6, 6, 8), np.int32)
    slabs[0:3, 1:5, 2:7] = 1
    slabs[3:5, 1:5, 2:7] = 2                            # 1 and 2 touch along z only
    c["3d_slabs_touch_along_z"] = (slabs, 3)
    c["3d_blobs_6x40x70"] = (_blobs((6, 40, 70), 20, 13), 3)
    # more pixels than one trip of the passes' capped grid takes (and than 1024 tiles of the reduction)
    c["above_the_launch_cap_1100x1024"] = (_small_blobs((1100, 1024), 300, 12), 2)
    # values are only compared: negative ones are objects of their own
    c["negative_values_11x13"] = (_noise((11, 13), 4, 14) - 2, 2)
    c["extreme_values_6x10"] = (np.array([-2 ** 31, 2 ** 31 - 1, 0, -1], np.int32)[_noise((6, 10), 4, 15)], 2)
    return c


CASES = _cases()


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_distance_equals_restatement(name, edge, device):
    labels, nd = CASES[name]
    got = assert_distance_equal(labels, nd, edge, device)
    assert ((got == 0) == (labels == 0)).all()
    if name.startswith("one_value") or name == "one_pixel":
        # without `edge` nothing to measure to; with it the padding (one step along z where Z == 1 is counted)
        assert (got == DIST_INF).all() if edge == 0 else (got.max() < DIST_INF and got.min() == 1)
    if name == "one_value_1x4x5_z_counted" and edge == 1:
        assert (got == 1).all()
    if name == "disc_20_cut_by_the_border":
        assert (call_distance(labels, nd, 0, device) != call_distance(labels, nd, 1, device)).any()


def test_distance_by_hand(device):
    square = np.zeros((7, 7), np.int32)
    square[1:6, 1:6] = 1
    for edge in (0, 1):
        d = call_distance(square, 2, edge, device)
        assert d[3, 3] == 9 and d[1, 1] == 1 and d[2, 2] == 4 and d[0, 0] == 0
    full = np.ones((5, 5), np.int32)
    assert call_distance(full, 2, 1, device).tolist() == [[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 4, 9, 4, 1], [1, 4, 4, 4, 1], [1, 1, 1, 1, 1]]
    halves = CASES["two_half_planes"][0]
    assert call_distance(halves, 2, 0, device)[4].tolist() == [49, 36, 25, 16, 9, 4, 1, 1, 4, 9, 16, 25, 36, 49]
    # the same map as a flat 3-D one: equal without `edge`, capped at one step with it
    flat = CASES["3d_flat_1x12x19"][0]
    assert np.array_equal(call_distance(flat, 3, 0, device)[0], call_distance(flat[0], 2, 0, device))
    assert np.array_equal(call_distance(flat, 3, 1, device)[0], np.minimum(call_distance(flat[0], 2, 1, device), 1))


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("name", ["row_ends_7x65", "3d_noise_5x7x9", "disc_20_cut_by_the_border"])
def test_distance_unaligned_labels(name, offset, device):
    labels, nd = CASES[name]
    for edge in (0, 1):
        assert_distance_equal(labels, nd, edge, device, offset=offset)


# ---------------------------------------------------------------------------------------------------------


def assert_inscribed_equal(labels, dist_sq, nid, device, **kw):
    out, bad = call_inscribed(labels, dist_sq, nid, device, **kw)
    want, want_bad = ref_inscribed(labels, dist_sq, nid)
    differ = np.flatnonzero((out != want).any(axis=1))
    assert len(differ) == 0, (len(differ), [(int(i), out[i].tolist(), want[i].tolist()) for i in differ[:4]])
    assert bad == want_bad
    return out


# clx_region_inscribed takes ids in [0, nid): the maps with negative values are left to test_inscribed_bad_labels_and_distances
@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][0].min() >= 0))
def test_inscribed_on_the_kernel_map_equals_restatement(name, edge, device):
    labels, nd = CASES[name]
    nid = int(labels.max()) + 2                                                     # the last id is absent
    dist = call_distance(labels, nd, edge, device)
    out = assert_inscribed_equal(labels, dist, nid, device)
    assert not out[0].any() and not out[nid - 1].any()
    present = np.unique(labels[labels > 0])
    assert (out[present, 0] >= 1).all() and (labels.reshape(-1)[out[present, 1]] == present).all()


def test_inscribed_ties_overflow_and_absent_ids(device):
    # a 2 x 6 bar: four pixels of the first row and four of the second attain the maximum; the smallest index is 1
    bar = np.ones((2, 6), np.int32)
    out, bad = call_inscribed(bar, np.array([[1, 4, 4, 4, 4, 1]] * 2), 4, device)
    assert out.tolist() == [[0, 0, 0], [4, 1, 36], [0, 0, 0], [0, 0, 0]] and bad == 0
    # a tie across lanes, waves and blocks: every pixel of a one-object map has the same distance
    flat = np.ones((40, 130), np.int32)
    for value in (0, 7, DIST_INF):
        out, bad = call_inscribed(flat, np.full(flat.shape, value), 2, device)
        assert out[1].tolist() == [value, 0, value * flat.size] and bad == 0
    # 2 000 ids in the pixels of a block against the 256 slots of its table: most go straight to global memory
    rng = np.random.default_rng(3)
    many = rng.integers(1, 2001, size=(40, 100)).astype(np.int32)
    dist = rng.integers(0, 50, size=many.shape).astype(np.int32)                     # few values: many ties
    dist[rng.random(many.shape) < 0.01] = DIST_INF
    assert_inscribed_equal(many, dist, 2001, device)
    assert_inscribed_equal(many, dist, 2001, device, offset=1)                       # the 4-byte loads
    out = assert_inscribed_equal(many, dist, 5000, device)
    assert not out[2001:].any()
    assert_inscribed_equal(_noise((16, 70), 3, 4), rng.integers(0, DIST_INF, size=(16, 70)), 3, device)


def test_inscribed_bad_labels_and_distances(device):
    labels = _blobs((12, 70), 9, 5)
    dist = ref_distance_sq(labels, 0)
    clean, bad = call_inscribed(labels, dist, 10, device)
    assert bad == 0
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[[3, 11, 0], [7, 69, 0]] = value
        out, bad = call_inscribed(lab, dist, 10, device)
        want, want_bad = ref_inscribed(np.where(lab == value, 0, lab), dist, 10)    # the pixel is skipped
        assert bad == BAD_LABEL and want_bad == 0 and np.array_equal(out, want)
    for value in (-1, -2 ** 31, DIST_INF + 1, 2 ** 31 - 1):
        d = dist.copy()
        ys, xs = np.nonzero(labels)
        d[ys[::17], xs[::17]] = value                                               # under objects
        d[labels == 0] = value                                                      # and on background, where nothing is read into a row
        out, bad = call_inscribed(labels, d, 10, device)
        skipped = np.zeros(labels.shape, bool)
        skipped[ys[::17], xs[::17]] = True
        want, _ = ref_inscribed(np.where(skipped, 0, labels), np.where(labels == 0, 0, d), 10)
        assert bad == BAD_DISTANCE and np.array_equal(out, want)
        assert_inscribed_equal(labels, d, 10, device)                               # the restatement's own flags agree
    lab = labels.copy()
    lab[0, 0] = 10
    d = dist.copy()
    d[tuple(np.argwhere(labels > 0)[0])] = -5
    _, bad = call_inscribed(lab, d, 10, device)
    assert bad == BAD_LABEL | BAD_DISTANCE
    _, bad = call_inscribed(labels, np.where(labels > 0, DIST_INF, 0), 10, device)  # INF itself is a value
    assert bad == 0


def test_deterministic_and_stale_buffers(device):
    labels, nd = CASES["above_the_launch_cap_1100x1024"]
    nid = int(labels.max()) + 1
    first = call_distance(labels, nd, 0, device)
    again = call_distance(labels, nd, 0, device, fill=0x5C)
    assert first.tobytes() == again.tobytes()
    a, _ = call_inscribed(labels, first, nid, device)
    b, _ = call_inscribed(labels, first, nid, device, fill=0xFF)
    z, _ = call_inscribed(labels, first, nid, device, fill=0)
    assert a.tobytes() == b.tobytes() == z.tobytes()
    noise = CASES["3d_noise_5x7x9"]
    assert call_distance(*noise, 1, device).tobytes() == call_distance(*noise, 1, device, fill=0).tobytes()


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(32768, dtype=torch.int32, device=device)
    outs = {k: Out((32768,), np.int32, device) for k in ("dist_sq", "workspace", "out", "bad")}
    null = ctypes.c_void_p(0)

    def message():
        m = lib.clx_last_error()
        return m.decode() if isinstance(m, bytes) else str(m)

    def distance(nd=2, Z=1, Y=8, X=8, edge=0, nbytes=4 * 32768, **ptrs):
        p = dict(labels=_clx.ptr(lab), dist_sq=outs["dist_sq"].ptr, workspace=outs["workspace"].ptr)
        p.update(ptrs)
        return lib.clx_label_distance_sq(p["labels"], nd, Z, Y, X, edge, p["dist_sq"], p["workspace"], nbytes, st)

    def inscribed(npix=64, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(lab), dist_sq=outs["dist_sq"].ptr, out=outs["out"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_inscribed(p["labels"], p["dist_sq"], npix, nid, p["out"], p["bad"], st)

    odd = ctypes.c_void_p(outs["workspace"].ptr.value + 2)
    refused = [(lambda k=k: distance(**{k: null}), "clx_label_distance_sq", "null") for k in ("labels", "dist_sq", "workspace")] + [
        (lambda: distance(nd=1), "clx_label_distance_sq", "nd"), (lambda: distance(nd=4), "clx_label_distance_sq", "nd"),
        (lambda: distance(nd=2, Z=2, Y=4, X=8), "clx_label_distance_sq", "Z == 1"),
        (lambda: distance(Z=0), "clx_label_distance_sq", "shape"), (lambda: distance(Y=0), "clx_label_distance_sq", "shape"),
        (lambda: distance(X=-1), "clx_label_distance_sq", "shape"), (lambda: distance(nd=3, Z=-2), "clx_label_distance_sq", "shape"),
        (lambda: distance(edge=2), "clx_label_distance_sq", "edge"), (lambda: distance(edge=-1), "clx_label_distance_sq", "edge"),
        (lambda: distance(Y=65536, X=65536), "clx_label_distance_sq", "Z * Y * X"),                 # npix = 2^32
        (lambda: distance(nd=3, Z=2, Y=46341, X=46341), "clx_label_distance_sq", "Z * Y * X"),
        (lambda: distance(Y=1, X=32769), "clx_label_distance_sq", "2^30"),                          # (X-1)^2 = 2^30
        (lambda: distance(Y=23172, X=23172), "clx_label_distance_sq", "2^30"),                      # 2 * 23171^2 > 2^30
        (lambda: distance(nd=3, Z=2, Y=23172, X=23172), "clx_label_distance_sq", "2^30"),
        (lambda: distance(nbytes=4 * 64 - 1), "clx_label_distance_sq", "workspace_bytes"),
        (lambda: distance(nbytes=0), "clx_label_distance_sq", "workspace_bytes"),
        (lambda: distance(workspace=odd), "clx_label_distance_sq", "aligned"),
    ] + [(lambda k=k: inscribed(**{k: null}), "clx_region_inscribed", "null") for k in ("labels", "dist_sq", "out", "bad")] + [
        (lambda: inscribed(nid=0), "clx_region_inscribed", "nid"), (lambda: inscribed(nid=-3), "clx_region_inscribed", "nid"),
        (lambda: inscribed(nid=2 ** 24 + 1), "clx_region_inscribed", "nid"),
        (lambda: inscribed(npix=0), "clx_region_inscribed", "npix"), (lambda: inscribed(npix=-1), "clx_region_inscribed", "npix"),
        (lambda: inscribed(npix=2 ** 32), "clx_region_inscribed", "npix"),
    ]
    for i, (call, who, word) in enumerate(refused):
        status = call()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message().startswith(who) and word in message(), f"case {i}: {message()!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    # accepted with valid arguments, the largest row the distance bound admits among them
    assert distance() == 0 and distance(nd=3, Z=2, Y=4, X=8, edge=1) == 0 and distance(Y=1, X=32768) == 0, message()
    assert distance(nbytes=4 * 64) == 0 and inscribed() == 0, message()
    torch.cuda.synchronize(device)
    assert int(outs["bad"].get()[0]) == 0 and not outs["dist_sq"].get()[:64].any()
