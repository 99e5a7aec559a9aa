"""clx_region_radial through the C ABI against the restatement of tests/radial_ref.py (the ring from the two inequalities in
int64, the wedge from eight masks, np.add.at).  Everything is integer work: count, isum and bad must be EQUAL.  The outputs
are prefilled with 0xAB bytes (or other garbage) and sit between guard words that must stay untouched."""

import ctypes

import numpy as np
import pytest
import torch

from radial_ref import BAD_LABEL, BAD_MAP, BAD_ROW, BAD_VALUE, DIST_INF, ref_distance_sq, ref_inscribed, ref_radial, rows_of_all
from test_gpu_hull import _noise
from test_gpu_measure import F32, F64, GUARD, I32, Out, _blobs, _dev, _raw, run_intensity, run_moments

pytestmark = pytest.mark.gpu

RAW_TYPE = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}


def call_radial(labels, dist_sq, raw, nid, inscribed, row, nrows, rings, width, wedges, shift, device, offset=0, fill=0xAB,
                with_isum=True):
    """one clx_region_radial call -> (count int64 (nrows, rings, wedges), isum int64 or None, bad); guard words checked"""
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    nd = labels.ndim
    Z, Y, X = (1,) * (3 - nd) + labels.shape
    lab = _dev(labels, device, offset)
    dist = _dev(np.array(dist_sq, dtype=np.int32), device, offset)
    raw_d, raw_type = None, 0
    if raw is not None:
        raw = np.ascontiguousarray(raw)
        raw_d, raw_type = _dev(raw, device, offset), RAW_TYPE[raw.dtype]
    ins = _dev(np.array(inscribed, dtype=np.int64).reshape(nid, 3), device)       # copies: maps_of's arrays are read-only
    row_d = _dev(np.array(row, dtype=np.int32).reshape(nid), device)
    outs = dict(count=Out((nrows, rings, wedges), np.int64, device), bad=Out((1,), np.int32, device))
    if with_isum:
        outs["isum"] = Out((nrows, rings, wedges), np.int64, device)
    for o in outs.values():
        o.buf[GUARD:GUARD + o.nbytes] = fill
    lib = _clx.load()
    status = lib.clx_region_radial(_clx.ptr(lab), _clx.ptr(dist), _clx.ptr(raw_d), raw_type, nd, Z, Y, X, nid, _clx.ptr(ins),
                                   _clx.ptr(row_d), nrows, rings, width, wedges, shift, outs["count"].ptr,
                                   outs["isum"].ptr if with_isum else ctypes.c_void_p(0), outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, lib.clx_last_error()
    torch.cuda.synchronize(device)
    return outs["count"].get(), outs["isum"].get() if with_isum else None, int(outs["bad"].get()[0])


def assert_radial_equal(labels, dist_sq, raw, nid, inscribed, row, nrows, rings, width, wedges, shift, device, want_bad=0, **kw):
    count, isum, bad = call_radial(labels, dist_sq, raw, nid, inscribed, row, nrows, rings, width, wedges, shift, device, **kw)
    want_count, want_isum, ref_bad = ref_radial(labels, dist_sq, raw, nid, inscribed, row, nrows, rings, width, wedges, shift)
    differ = np.argwhere(count != want_count)
    assert len(differ) == 0, (len(differ), [(p.tolist(), int(count[tuple(p)]), int(want_count[tuple(p)])) for p in differ[:4]])
    if isum is not None:
        differ = np.argwhere(isum != want_isum)
        assert len(differ) == 0, (len(differ), [(p.tolist(), int(isum[tuple(p)]), int(want_isum[tuple(p)])) for p in differ[:4]])
    assert bad == ref_bad == want_bad
    return count, isum


_MAPS = {}


def maps_of(labels, edge=0):
    """(dist_sq, nid, inscribed, row, nrows) of a label map from the restatements, computed once per map and left unchanged;
    the last id is absent and every id has a row"""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    key = (labels.shape, edge, labels.tobytes())
    if key not in _MAPS:
        nid = int(labels.max()) + 2
        dist = ref_distance_sq(labels, edge)
        ins, bad = ref_inscribed(labels, dist, nid)
        assert bad == 0
        row, nrows = rows_of_all(nid)
        for a in (dist, ins, row):
            a.setflags(write=False)
        _MAPS[key] = (dist, nid, ins, row, nrows)
    return _MAPS[key]


def check_map(labels, raw, rings, width, wedges, shift, device, edge=0, **kw):
    dist, nid, ins, row, nrows = maps_of(labels, edge)
    return assert_radial_equal(labels, dist, raw, nid, ins, row, nrows, rings, width, wedges, shift, device, **kw)


def _disc(shape, centre, radius, value=1):
    yy, xx = np.indices(shape)
    return np.where((yy - centre[0]) ** 2 + (xx - centre[1]) ** 2 <= radius * radius, value, 0).astype(np.int32)


def _values(shape, seed):
    """float32 values that quantise exactly at shift 4: multiples of 1/16 in (-2048, 2048)"""
    return (np.random.default_rng(seed).integers(-2 ** 15, 2 ** 15, size=shape) / 16.0).astype(np.float32)


SHAPES = [(5, 7), (9, 13), (33, 32), (3, 5, 7), (4, 9, 13), (1, 9, 13)]


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_ends_and_tails(shape, offset, device):
    """lanes whose 4 pixels straddle rows, the scalar tail past the last whole lane, the 4-byte loads of unaligned maps"""
    for labels in (_blobs(shape, 5, 3 + len(shape)), _noise(shape, 4, 11) + (1 if len(shape) == 2 else 0)):
        raw = _values(shape, 2)
        for edge in (0, 1):
            check_map(labels, raw, 4, 0, 1, 4, device, edge=edge, offset=offset)
        check_map(labels, raw, 3, 2, 1, 4, device, offset=offset)
        if len(shape) == 2:
            check_map(labels, raw, 4, 0, 8, 4, device, edge=1, offset=offset)
            check_map(labels, raw, 32, 1, 8, 4, device, offset=offset)


def test_ring_ties(device):
    square = np.zeros((12, 13), np.int32)
    square[2:10, 3:11] = 1
    for rings, width, want in ((4, 0, [28, 20, 12, 4]), (2, 0, [48, 16]), (1, 0, [64]), (4, 1, [28, 20, 12, 4]), (4, 2, [48, 16, 0, 0]),
                               (4, 3, [60, 4, 0, 0]), (3, 1, [28, 20, 16])):
        count, _ = check_map(square, None, rings, width, 1, 0, device)
        assert count[0, :, 0].tolist() == want
    for radius in (4, 5):
        disc = _disc((15, 17), (7, 8), radius)
        raw = _values(disc.shape, radius)
        for rings in (1, 2, 4, 5, 32):
            count, _ = check_map(disc, raw, rings, 0, 1, 4, device)
            assert count.sum() == disc.sum() and count[0, rings - 1, 0] >= 1           # the core holds the centre
            check_map(disc, raw, rings, 0, 8, 4, device)
        for width in (1, 2, 3, 32768):
            count, _ = check_map(disc, raw, 4, width, 1, 4, device)
            assert count.sum() == disc.sum()
        assert check_map(disc, raw, 4, 32768, 1, 4, device)[0][0, :, 0].tolist() == [int(disc.sum()), 0, 0, 0]


def test_wedges(device):
    # a disc whose centre pixel, axes and diagonals are all present: every ray of the table is met
    disc = _disc((21, 23), (10, 11), 8)
    count, _ = check_map(disc, _values(disc.shape, 1), 4, 0, 8, 4, device)
    assert (count[0].sum(axis=0) > 0).all() and count.sum() == disc.sum()
    # an L whose inscribed centre (in the thick foot) is far from its centroid
    ell = np.zeros((30, 34), np.int32)
    ell[2:28, 3:6] = 1
    ell[18:28, 3:30] = 1
    dist, nid, ins, _, _ = maps_of(ell)
    cy, cx = divmod(int(ins[1, 1]), ell.shape[1])
    my, mx = (float(v.mean()) for v in np.nonzero(ell))
    assert cy >= 18 and abs(cy - my) + abs(cx - mx) > 4
    check_map(ell, _values(ell.shape, 2), 4, 0, 8, 4, device)
    check_map(ell, _values(ell.shape, 2), 5, 2, 8, 4, device)
    # two objects side by side: the wedge centre is per object
    two = np.concatenate([_disc((17, 17), (8, 8), 6, 1), _disc((17, 17), (8, 8), 7, 2)], axis=1)
    count, _ = check_map(two, _values(two.shape, 3), 3, 0, 8, 4, device)
    assert (count[0].sum(axis=0) > 0).all() and (count[1].sum(axis=0) > 0).all()
    # touching objects with no background between them, every id of a noise map
    check_map(np.repeat(np.repeat(_noise((6, 9), 5, 4) + 1, 4, axis=0), 3, axis=1), None, 4, 0, 8, 0, device)


def test_64_bit_products(device):
    """d2 and D2 up to 2^30 with rings 32: d2 * 1024 and (k + 1)^2 * D2 reach 2^40; 32-bit products would wrap"""
    labels = np.ones((4, 8), np.int32)
    labels[2:] = 2
    labels[0, 0] = 0
    dist = np.array([5, 1, 2 ** 30 - 1, DIST_INF, 2 ** 20, 2 ** 29, 2 ** 29 + 1, 3] * 4, np.int32).reshape(4, 8)
    dist[3] = [1, 2 ** 10, 2 ** 20, 2 ** 22, 2 ** 24 + 1, 2 ** 28, 2 ** 30 - 1, DIST_INF]
    ins = np.array([[0, 0, 0], [DIST_INF, 3, 0], [DIST_INF, 31, 0]], np.int64)
    row, nrows = np.array([-1, 0, 1], np.int32), 2
    for rings in (32, 31, 4):
        count, _ = assert_radial_equal(labels, dist, None, 3, ins, row, nrows, rings, 0, 1, 0, device)
        assert count.sum() == 31 and count[0, rings - 1, 0] >= 2 and count[0, 0, 0] >= 2
        assert_radial_equal(labels, dist, None, 3, ins, row, nrows, rings, 0, 8, 0, device)
    for width in (1, 1024, 32767, 32768):
        assert_radial_equal(labels, dist, None, 3, ins, row, nrows, 32, width, 1, 0, device)
    # a D2 that is not the largest d2 of the object, below 2^30: the pixels above it are flagged, the others land
    ins2 = ins.copy()
    ins2[1, 0] = 2 ** 29
    assert_radial_equal(labels, dist, None, 3, ins2, row, nrows, 32, 0, 1, 0, device, want_bad=BAD_MAP)


@pytest.mark.parametrize("kind", ["f32", "f64", "i32"])
def test_raw_types(kind, device):
    from cellulus_amd.measure import intensity_shift

    labels = _blobs((12, 70), 9, 5)
    raw = _raw(kind, labels.shape, 11)                       # negative values among them
    shift = 0 if kind == "i32" else intensity_shift(float(np.abs(raw.astype(np.float64)).max()), labels.size)
    for wedges in (1, 8):
        _, isum = check_map(labels, raw, 4, 0, wedges, shift, device)
        assert (isum < 0).any() and (isum > 0).any()
        check_map(labels, raw, 4, 0, wedges, shift, device, offset=1)
    if kind != "i32":
        zeros = np.where(np.indices(labels.shape).sum(axis=0) % 2 == 0, 0.0, -0.0).astype(raw.dtype)
        _, isum = check_map(labels, zeros, 4, 0, 1, shift, device)
        assert not isum.any()
    # counts only: raw == NULL with and without an isum, whatever raw_type and shift say
    dist, nid, ins, row, nrows = maps_of(labels)
    count, isum, bad = call_radial(labels, dist, None, nid, ins, row, nrows, 4, 0, 1, 999, device)
    want = ref_radial(labels, dist, None, nid, ins, row, nrows, 4, 0, 1)[0]
    assert np.array_equal(count, want) and not isum.any() and bad == 0
    count, isum, bad = call_radial(labels, dist, None, nid, ins, row, nrows, 4, 0, 1, 0, device, with_isum=False)
    assert np.array_equal(count, want) and isum is None and bad == 0


def test_shift_at_both_clamps(device):
    """intensity_shift clamps to [-1022, 1023]: float64 values near the ends of the exponent range"""
    from cellulus_amd.measure import intensity_shift

    labels = _blobs((9, 40), 6, 8)
    rng = np.random.default_rng(6)
    tiny = rng.integers(-2 ** 20, 2 ** 20, size=labels.shape) * 2.0 ** -1040          # multiples of 2^-1040, subnormals among them
    assert intensity_shift(float(np.abs(tiny).max()), labels.size) == 1023
    _, isum = check_map(labels, tiny, 4, 0, 1, 1023, device)
    assert isum.any()
    huge = rng.integers(-2 ** 20, 2 ** 20, size=labels.shape) * 2.0 ** 1003
    _, isum = check_map(labels, huge, 4, 0, 1, -1022, device)
    assert isum.any() and np.abs(isum).max() < 2 ** 12


def test_sums_equal_intensity_and_moments(device):
    """for every taken id the sum over rings and wedges is clx_region_intensity's isum, bit for bit, and the area"""
    labels = _blobs((40, 70), 12, 21)
    nid = int(labels.max()) + 2
    area = run_moments(labels, nid, device)["area"].astype(np.int64)
    for kind, shift in (("f32", 9), ("f64", 20), ("i32", 0)):
        raw = _raw(kind, labels.shape, 4)
        whole = run_intensity(labels, raw, nid, shift, device)[0]
        assert whole["bad"][0] == 0
        for rings, width, wedges in ((4, 0, 1), (7, 0, 8), (5, 2, 8)):
            count, isum = check_map(labels, raw, rings, width, wedges, shift, device)
            assert np.array_equal(isum.sum(axis=(1, 2)), whole["isum"][1:]) and np.array_equal(count.sum(axis=(1, 2)), area[1:])


def test_lds_table(device):
    """far more cells than the 1024 slots of a block's table (most go straight to global memory), and one object over a whole
    map, every lane in the same few cells"""
    rng = np.random.default_rng(3)
    many = rng.integers(1, 2001, size=(40, 100)).astype(np.int32)
    dist = rng.integers(1, 50, size=many.shape).astype(np.int32)
    nid = 2001
    ins, _ = ref_inscribed(many, dist, nid)
    row, nrows = rows_of_all(nid)
    raw = _values(many.shape, 9)
    for rings, wedges in ((4, 8), (32, 8), (4, 1)):
        assert_radial_equal(many, dist, raw, nid, ins, row, nrows, rings, 0, wedges, 4, device)
    assert_radial_equal(many, dist, raw, nid, ins, row, nrows, 4, 0, 8, 4, device, offset=1)
    assert_radial_equal(many, dist, raw, nid, ins, row, nrows, 32, 3, 8, 4, device)
    one = np.ones((64, 64), np.int32)
    for rings, wedges in ((4, 1), (4, 8), (32, 8)):
        count, _ = check_map(one, _values(one.shape, 1), rings, 0, wedges, 4, device, edge=1)
        assert count.sum() == one.size
    # without `edge` the object has nothing to measure to: d2 = D2 = CLX_DIST_INF everywhere, all core
    count, _ = check_map(one, None, 4, 0, 1, 0, device)
    assert count[0, :, 0].tolist() == [0, 0, 0, one.size]


def test_grid_above_the_launch_cap(device):
    """more than 1024 tiles of 1024 pixels: every block takes a second tile; few objects keep the restatement cheap"""
    labels = np.zeros((1025, 1024), np.int32)
    labels[10:500, 20:600] = 1
    labels[500:1020, 20:300] = 2                             # touches 1 along a row
    labels |= _disc(labels.shape, (760, 680), 250, 4) * (labels == 0)
    labels[1021:, :] = 3                                     # the last rows, into the tail tile
    raw = _values(labels.shape, 5)
    count, isum = check_map(labels, raw, 4, 0, 8, 4, device)
    assert count.sum() == (labels > 0).sum()
    dist, nid, ins, row, nrows = maps_of(labels)
    again = call_radial(labels, dist, raw, nid, ins, row, nrows, 4, 0, 8, 4, device, fill=0x5C)           # the same bits in every run
    assert again[0].tobytes() == count.tobytes() and again[1].tobytes() == isum.tobytes()
    check_map(labels, raw, 32, 7, 1, 4, device)


def test_rows(device):
    labels = _blobs((30, 70), 12, 17)
    dist, nid, ins, row, nrows = maps_of(labels)
    raw = _values(labels.shape, 8)
    whole_count, whole_isum = assert_radial_equal(labels, dist, raw, nid, ins, row, nrows, 4, 0, 8, 4, device)
    present = np.unique(labels[labels > 0])
    # a subset of the ids, in reversed order
    take = present[::3][::-1]
    sub = np.full(nid, -1, np.int32)
    sub[take] = np.arange(len(take))
    count, isum = assert_radial_equal(labels, dist, raw, nid, ins, sub, len(take), 4, 0, 8, 4, device)
    assert np.array_equal(count, whole_count[take - 1]) and np.array_equal(isum, whole_isum[take - 1])
    # no id taken: nrows == 0, nothing is written but bad
    none = np.full(nid, -1, np.int32)
    count, isum = assert_radial_equal(labels, dist, raw, nid, ins, none, 0, 4, 0, 8, 4, device)
    assert count.shape == (0, 4, 8)
    # two chunks that together equal one call
    parts = []
    for chunk in (present[:5], present[5:]):
        r = np.full(nid, -1, np.int32)
        r[chunk] = np.arange(len(chunk))
        parts.append(assert_radial_equal(labels, dist, raw, nid, ins, r, len(chunk), 4, 0, 8, 4, device))
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole_count[present - 1])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole_isum[present - 1])


def test_every_bad_bit_alone(device):
    labels = _blobs((12, 70), 9, 5)
    dist, nid, ins, row, nrows = maps_of(labels)
    raw = _values(labels.shape, 8).astype(np.float64)
    args = (nid, ins, row, nrows, 4, 0, 8, 4, device)
    clean_count, clean_isum = assert_radial_equal(labels, dist, raw, *args)
    ys, xs = np.nonzero(labels)
    big = int(np.argmax(ins[:, 0]))                          # a present id
    # bit 0: labels outside [0, nid) count as background; every other pixel still lands
    for value in (nid, 2 ** 31 - 1, -1, -2 ** 31):
        lab = labels.copy()
        lab[ys[::29], xs[::29]] = value
        lab[0, 0] = value
        count, isum = assert_radial_equal(lab, dist, raw, *args, want_bad=BAD_LABEL)
        want = ref_radial(np.where(lab == value, 0, lab), dist, raw, nid, ins, row, nrows, 4, 0, 8, 4)
        assert want[2] == 0 and np.array_equal(count, want[0]) and np.array_equal(isum, want[1])
    # bit 1: a NaN, an Inf, a value above the per-pixel bound; on background they are ignored
    for poison in (np.nan, np.inf, -np.inf, 2.0 ** 60):
        r = raw.copy()
        r[labels == 0] = poison
        count, isum = assert_radial_equal(labels, dist, r, *args)
        assert np.array_equal(count, clean_count) and np.array_equal(isum, clean_isum)
        r = raw.copy()
        r[ys[7], xs[7]] = poison
        count, isum = assert_radial_equal(labels, dist, r, *args, want_bad=BAD_VALUE)
        assert count.sum() == clean_count.sum() - 1
        hit = labels[ys[7], xs[7]] - 1
        others = np.arange(nrows) != hit
        assert np.array_equal(count[others], clean_count[others]) and np.array_equal(isum[others], clean_isum[others])
    # ... and under an id that is not taken
    r = raw.copy()
    r[labels == big] = np.nan
    untaken = row.copy()
    untaken[big] = -1
    assert_radial_equal(labels, dist, r, nid, ins, untaken, nrows, 4, 0, 8, 4, device)
    # bit 2: a stale D2 below a pixel's d2; a d2 of 0 or below under an object; a d2 above CLX_DIST_INF; a centre past the map
    stale = ins.copy()
    stale[big, 0] = 1
    count, isum = assert_radial_equal(labels, dist, raw, nid, stale, row, nrows, 4, 0, 8, 4, device, want_bad=BAD_MAP)
    others = np.arange(nrows) != big - 1
    assert np.array_equal(count[others], clean_count[others]) and count[big - 1].sum() == ((labels == big) & (dist == 1)).sum()
    for value in (0, -1, -2 ** 31):
        d = dist.copy()
        d[ys[11], xs[11]] = value
        d[labels == 0] = value                              # on background nothing is read into a cell
        count, _ = assert_radial_equal(labels, d, raw, *args, want_bad=BAD_MAP)
        assert count.sum() == clean_count.sum() - 1
    d = dist.copy()
    d[ys[11], xs[11]] = DIST_INF + 1
    assert_radial_equal(labels, d, raw, nid, ins, row, nrows, 4, 5, 1, 4, device, want_bad=BAD_MAP)
    d[ys[11], xs[11]] = DIST_INF                            # the bound itself is a value in absolute mode
    assert_radial_equal(labels, d, raw, nid, ins, row, nrows, 4, 5, 1, 4, device)
    for centre in (labels.size, 2 ** 32, 2 ** 63 - 1, -1):
        off = ins.copy()
        off[big, 1] = centre
        count, isum = assert_radial_equal(labels, dist, raw, nid, off, row, nrows, 4, 0, 8, 4, device, want_bad=BAD_MAP)
        assert np.array_equal(count[others], clean_count[others]) and not count[big - 1].any() and not isum[big - 1].any()
        assert_radial_equal(labels, dist, raw, nid, off, row, nrows, 4, 0, 1, 4, device)        # no wedges: the centre is not read
    # garbage in every D2, far above any d2: all rim, no flag, nothing out of bounds
    wild = ins.copy()
    wild[1:, 0] = [2 ** 40 + i for i in range(nid - 2)] + [2 ** 63 - 1]                  # the last id is absent
    wild[big, 0] = 2 ** 45                                  # above the 2^41 at which the kernel cuts a D2
    count, _ = assert_radial_equal(labels, dist, raw, nid, wild, row, nrows, 32, 0, 8, 4, device)
    assert count[:, 1:].sum() == 0
    # bit 3: a row at or above nrows; the id is not taken
    for value in (nrows, 2 ** 31 - 1):
        r = row.copy()
        r[big] = value
        count, isum = assert_radial_equal(labels, dist, raw, nid, ins, r, nrows, 4, 0, 8, 4, device, want_bad=BAD_ROW)
        assert np.array_equal(count[others], clean_count[others]) and np.array_equal(isum[others], clean_isum[others])
        assert not count[big - 1].any() and not isum[big - 1].any()
    r = row.copy()
    r[nid - 1] = nrows                                      # an absent id: no pixel meets its row
    assert_radial_equal(labels, dist, raw, nid, ins, r, nrows, 4, 0, 8, 4, device)


def test_rejected_arguments_launch_nothing(device):
    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    zeros = torch.zeros(4096, dtype=torch.int64, device=device)
    outs = {k: Out((4096,), np.int64, device) for k in ("count", "isum", "bad")}
    null = ctypes.c_void_p(0)

    def message():
        m = lib.clx_last_error()
        return m.decode() if isinstance(m, bytes) else str(m)

    def radial(raw_type=F32, nd=2, Z=1, Y=8, X=8, nid=4, nrows=3, rings=4, width=0, wedges=1, shift=0, **ptrs):
        p = dict(labels=_clx.ptr(zeros), dist_sq=_clx.ptr(zeros), raw=_clx.ptr(zeros), inscribed=_clx.ptr(zeros), row=_clx.ptr(zeros),
                 count=outs["count"].ptr, isum=outs["isum"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_radial(p["labels"], p["dist_sq"], p["raw"], raw_type, nd, Z, Y, X, nid, p["inscribed"], p["row"], nrows,
                                     rings, width, wedges, shift, p["count"], p["isum"], p["bad"], st)

    refused = [(lambda k=k: radial(**{k: null}), "null") for k in ("labels", "dist_sq", "inscribed", "row", "count", "isum", "bad")] + [
        (lambda: radial(raw_type=3), "raw_type"), (lambda: radial(raw_type=-1), "raw_type"),
        (lambda: radial(nd=1), "nd"), (lambda: radial(nd=4), "nd"),
        (lambda: radial(nd=2, Z=2, Y=4), "Z == 1"),
        (lambda: radial(Z=0), "extents"), (lambda: radial(Y=0), "extents"), (lambda: radial(X=-1), "extents"),
        (lambda: radial(nd=3, Z=-2), "extents"),
        (lambda: radial(Y=65536, X=65536), "Z*Y*X"), (lambda: radial(nd=3, Z=2, Y=46341, X=46341), "Z*Y*X"),
        (lambda: radial(nid=0), "nid"), (lambda: radial(nid=-3), "nid"), (lambda: radial(nid=2 ** 24 + 1), "nid"),
        (lambda: radial(nrows=-1), "nrows"), (lambda: radial(nrows=4), "nrows"),
        (lambda: radial(rings=0), "rings"), (lambda: radial(rings=33), "rings"), (lambda: radial(rings=-4), "rings"),
        (lambda: radial(width=-1), "width"), (lambda: radial(width=32769), "width"),
        (lambda: radial(wedges=0), "wedges"), (lambda: radial(wedges=2), "wedges"), (lambda: radial(wedges=4), "wedges"),
        (lambda: radial(wedges=9), "wedges"),
        (lambda: radial(nd=3, Z=2, Y=4, wedges=8), "wedges == 8"), (lambda: radial(nd=3, wedges=8), "wedges == 8"),
        (lambda: radial(nid=2 ** 24, nrows=2 ** 23, rings=32, wedges=8), "2^31"),
    ]
    for i, (call, word) in enumerate(refused):
        status = call()
        assert status == -1, f"case {i} returned {status}, not CLX_ERR_ARG"
        assert message().startswith("clx_region_radial") and word in message(), f"case {i}: {message()!r} does not name {word!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    # accepted: the defaults, a flat 3-D map, the largest table the bound admits in name only (nrows == 0), counts only
    assert radial() == 0 and radial(nd=3, Z=1) == 0 and radial(nd=3, Z=2, Y=4) == 0 and radial(width=32768, rings=32, wedges=8) == 0, message()
    assert radial(nid=2 ** 12, nrows=0) == 0 and radial(raw=null, isum=null, raw_type=77) == 0 and radial(raw=null) == 0, message()
    torch.cuda.synchronize(device)
    assert int(outs["bad"].get().view(np.int32)[0]) == 0 and not outs["count"].get()[:12].any() and not outs["isum"].get()[:12].any()
