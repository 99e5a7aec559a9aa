"""The kernels of csrc/augment.hip through the C ABI (clx_elastic_crop with its own cp_shape, mats and records — not through
ZarrDataset) against augment_ref.py: float64 NumPy / SciPy on the entry's own inputs.

Constants mirrored from the source (augment_ref.plan): 256 threads, 4 consecutive x voxels per thread item, at most
max(2048 / B, 1) blocks per crop — beyond that a thread strides over several items —, one 16-byte store per item when
the last crop extent is a multiple of 4 and single stores (and a raw pointer that needs only 4-byte alignment) otherwise,
at most 60 000 bytes of LDS for the matrices and one record.

Every call writes raw, maxima and the workspace into 0xAB-filled buffers between guard zones that must come back
untouched; the data set lies between poison (NaN for float32, 0xFF otherwise), so that a read outside it — even with
weight 0 — shows in the result; and maxima[b] == raw[b].max() is checked for every crop of every call.

Exact cases (analytic, plain, maxima, batch against single calls) are compared with array_equal.  Cases against the
reference have the per-voxel bound augment_ref derives,
    |got - ref64| <= 2^-24 |ref64| + nd * 2 Vmax * 2 T 2^-52 R,
and print their worst err / bound.  Measured on an MI355X, the worst of each family: odd-width 0.995, control-points
0.996, mixed-room 0.983, reflect-wrap 0.990, types 0.998, lds 0.995, grid-cap 0.999, edges of the placement 0.000.  (A
figure just below 1 is the one rounding to float32 where the result sits at the bottom of a binade; float32(ref64) itself
gives the same figures, so the float64 sums of the kernels and of the reference round alike nearly everywhere.)

What no test of values can see: a grid-stride loop whose stride is too SHORT (256 instead of tiles * 256) makes blocks
redo items of later blocks with the same results — every output is the same.  A stride that is too long, or a loop that
stops after one trip, leaves the 0xAB filling in raw and fails every grid-cap case."""

import ctypes

import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                    # bytes in front of and behind every output (a multiple of 16)
POISON = 256                  # bytes in front of and behind the data set


class Out:
    """A device output of `nbytes`, 0xAB-filled, between two guard zones; `shift` bytes off a 16-byte boundary."""

    def __init__(self, nbytes, device, shift=0):
        self.nbytes, self.shift = int(nbytes), shift
        self.buf = torch.full((GUARD + shift + self.nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD + shift)

    def get(self, dtype, shape):
        host = self.buf.cpu().numpy()
        lo = GUARD + self.shift
        assert (host[:lo] == 0xAB).all() and (host[lo + self.nbytes:] == 0xAB).all(), "guard words overwritten"
        return host[lo:lo + self.nbytes].copy().view(dtype).reshape(shape)


def _upload(data, device):
    """The data set's bytes between two zones of poison -> (tensor that owns them, pointer to the data)."""
    raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    if data.dtype == np.float32:
        pad = np.full(POISON // 4, np.nan, dtype=np.float32).view(np.uint8)
    else:
        pad = np.full(POISON, 0xFF, dtype=np.uint8)
    t = torch.from_numpy(np.concatenate([pad, raw, pad])).to(device)
    return t, ctypes.c_void_p(t.data_ptr() + POISON)


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def crop_call(device, data, factor, crop, records, elastic, cp_shape=None, mats=None, shift=0, uploaded=None):
    """One clx_elastic_crop -> (raw (B, C, *crop) float32, maxima (B,) float32) as host arrays, the guards checked and
    maxima[b] == raw[b].max() asserted."""
    from cellulus_amd import _clx

    lib = _clx.load()
    data = np.ascontiguousarray(data)
    S, C, spatial, nd = data.shape[0], data.shape[1], data.shape[2:], len(crop)
    records = np.ascontiguousarray(records, dtype=np.float64)
    B = records.shape[0]
    assert records.shape[1] == (1 + nd * nd + nd + nd * int(np.prod(cp_shape)) if elastic else 1 + nd)
    assert records[:, 0].min() >= 0 and records[:, 0].max() < S
    keep, data_ptr = uploaded if uploaded is not None else _upload(data, device)
    rec_d = torch.from_numpy(records).to(device)
    nvox = int(np.prod(crop))
    raw = Out(B * C * nvox * 4, device, shift)
    maxima = Out(B * 4, device)
    cp_c = mats_d = work = None
    if elastic:
        assert all(m.shape == (c, p) and m.dtype == np.float64 for m, c, p in zip(mats, crop, cp_shape))
        assert R.lds_bytes(crop, cp_shape) <= R.AUG_MAX_LDS
        cp_c = _ints(cp_shape)
        mats_d = torch.from_numpy(np.concatenate([np.ascontiguousarray(m).ravel() for m in mats])).to(device)
        need = int(lib.clx_elastic_crop_workspace(nd, _ints(crop), B))
        assert need == B * R.plan(crop, C, B, True)["p1"] * 2 * nd * 8
        work = Out(need, device)
    _clx.call("clx_elastic_crop", data_ptr, R.AUG_DTYPES[data.dtype], S, C, nd, _ints(spatial), _ints(crop), cp_c,
              float(np.float32(factor)), int(bool(elastic)), B, _clx.ptr(rec_d), _clx.ptr(mats_d),
              work.ptr if work is not None else ctypes.c_void_p(0), raw.ptr, maxima.ptr, _clx.stream_ptr(device))
    torch.cuda.synchronize(device)
    if work is not None:
        work.get(np.float64, (-1,))
    got = raw.get(np.float32, (B, C) + tuple(crop))
    mx = maxima.get(np.float32, (B,))
    assert not np.isnan(got).any(), "NaN in the result: a read outside the data set"
    assert np.array_equal(mx, got.reshape(B, -1).max(axis=1)), "maxima[b] != raw[b].max()"
    del keep
    return got, mx


def against_reference(got, refs, what):
    """|got - ref64| <= bound per voxel for every crop; -> the worst err / bound (0 / 0 counts as 0)."""
    worst = 0.0
    for b, (ref, mode, _room, bound) in enumerate(refs):
        err = np.abs(got[b].astype(np.float64) - ref)
        ratio = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny), 0.0)
        worst = max(worst, float(ratio.max()))
        if not (err <= bound).all():
            i = np.unravel_index(int(ratio.argmax()), err.shape)
            raise AssertionError(f"{what} crop {b} ({mode}): |got - ref| = {err[i]:.3e} > bound {bound[i]:.3e} at {i}: "
                                 f"{got[b][i]!r} != {ref[i]!r}; {int((err > bound).sum())} of {err.size} voxels beyond the bound")
    return worst


def _slices(off, crop):
    return (slice(None),) + tuple(slice(int(o), int(o) + c) for o, c in zip(off, crop))


def _normalised32(data, factor):
    return data.astype(np.float32) * np.float32(factor)


# ------------------------------------------------------------------------------------------------------ a. analytic
ANALYTIC_DATA = {np.uint8: None, np.uint16: None, np.float32: 0.37}          # dtype -> factor (None: the type's default)


def _analytic_inputs(nd, dtype, spatial):
    data = R.random_data((3, 2) + tuple(spatial), dtype, seed=11, signed=True)
    factor = R.default_factor(dtype) if ANALYTIC_DATA[dtype] is None else ANALYTIC_DATA[dtype]
    return data, float(np.float32(factor))


@pytest.mark.parametrize("W", [50, 52], ids=["w50-single-stores", "w52-vector-stores"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("nd", [2, 3])
def test_identity_on_the_whole_source_is_the_source(device, nd, dtype, W):
    """A = I, no jitter, crop == source: room == 0 exactly on every axis, every coordinate is an integer, the upper
    neighbour of the last voxel is index n (weight 0, never read): raw == float32(data[s]) * factor, bit for bit, for
    any u."""
    crop = (20, W) if nd == 2 else (5, 6, W)
    data, factor = _analytic_inputs(nd, dtype, crop)
    cp = R.cp_shape_for(crop, 32)
    mats = R.make_mats(crop, cp)
    rng = np.random.default_rng(5)
    us = [0.5, 0.0, 1.0 - 2.0 ** -53, None]
    records = np.stack([R.make_record(cp, b % 3, rng, A=np.eye(nd), u=u) for b, u in enumerate(us)])
    got, _ = crop_call(device, data, factor, crop, records, True, cp, mats, shift=4 if W % 4 else 0)
    for b in range(len(us)):
        assert np.array_equal(got[b], _normalised32(data[b % 3], factor)), (b, us[b])
    for ref, mode, room, _bound in R.ref_crops(data, factor, crop, cp, mats, records, True):
        assert mode == "constant" and not room.any()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("spatial, crop", [((26, 58), (20, 50)), ((26, 60), (20, 52)), ((9, 8, 56), (5, 6, 50)),
                                           ((9, 8, 56), (5, 6, 52))], ids=["2d-w50", "2d-w52", "3d-w50", "3d-w52"])
def test_identity_with_an_even_margin_is_the_plain_crop(device, spatial, crop, dtype):
    """A = I, no jitter, the source larger by an even margin: with u = 1/2 the origin is the integer margin / 2 — the
    centred window, equal to slicing AND to aug_plain_kernel at that offset, bit for bit.  u = 0 and u = 1 - 2^-53 (the
    first and the last window) stay within the reference's bound and read nothing outside the source."""
    nd = len(crop)
    data, factor = _analytic_inputs(nd, dtype, spatial)
    cp = R.cp_shape_for(crop, 32)
    mats = R.make_mats(crop, cp)
    rng = np.random.default_rng(6)
    shift = 4 if crop[-1] % 4 else 0
    up = _upload(data, device)
    records = np.stack([R.make_record(cp, s, rng, A=np.eye(nd), u=u) for s, u in [(0, 0.5), (1, 0.0), (2, 1.0 - 2.0 ** -53)]])
    got, _ = crop_call(device, data, factor, crop, records, True, cp, mats, shift=shift, uploaded=up)
    off = [(n - c) // 2 for n, c in zip(spatial, crop)]
    want = _normalised32(data[0], factor)[_slices(off, crop)]
    assert np.array_equal(got[0], want)
    plain, _ = crop_call(device, data, factor, crop, [R.plain_record(0, off)], False, shift=shift, uploaded=up)
    assert np.array_equal(plain[0], want)
    refs = R.ref_crops(data, factor, crop, cp, mats, records, True)
    assert all(mode == "constant" and np.array_equal(room, np.subtract(spatial, crop)) for _r, mode, room, _b in refs)
    worst = against_reference(got, refs, "edges of the placement")
    print(f"placement u = 1/2, 0, 1 - 2^-53 ({np.dtype(dtype).name}, {crop} of {spatial}): worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("nd", [2, 3])
def test_quarter_turn_is_rot90_of_the_window(device, nd, dtype):
    """A = [[0, -1], [1, 0]] in the (y, x) plane (a leading 1 in 3-D), non-square source and crop, even margins, u = 1/2:
    every coordinate is an integer, so the crop is a rot90 of the centred window exactly.  WHICH rot90 is taken from
    augment_ref, and must be the same one for the kernel."""
    crop, spatial = ((6, 10), (16, 10)) if nd == 2 else ((3, 6, 10), (5, 16, 10))
    data, factor = _analytic_inputs(nd, dtype, spatial)
    cp = R.cp_shape_for(crop, 32)
    mats = R.make_mats(crop, cp)
    A = np.eye(nd)
    A[-2:, -2:] = [[0.0, -1.0], [1.0, 0.0]]
    rec = R.make_record(cp, 2, np.random.default_rng(0), A=A, u=0.5)
    (ref, mode, room, _), = R.ref_crops(data, factor, crop, cp, mats, [rec], True)
    turned = crop[:-2] + (crop[-1], crop[-2])                       # the window has the crop's last two extents swapped
    assert mode == "constant" and np.array_equal(room, np.subtract(spatial, turned))
    off = [(n - c) // 2 for n, c in zip(spatial, turned)]
    window = _normalised32(data[2], factor)[_slices(off, turned)]
    ks = [k for k in range(4) if np.rot90(window, k, axes=(-2, -1)).shape == ref.shape
          and np.array_equal(np.rot90(window, k, axes=(-2, -1)).astype(np.float64), ref)]
    assert len(ks) == 1, ks
    got, _ = crop_call(device, data, factor, crop, [rec], True, cp, mats)
    assert np.array_equal(got[0], np.rot90(window, ks[0], axes=(-2, -1)))


# ------------------------------------------------------------------------------- b. random parameters, c. grid caps
@pytest.mark.parametrize("name", R.RANDOMISED)
def test_random_parameters_against_the_reference(device, name):
    c = R.build_case(name)
    refs = R.case_reference(name)
    got, _ = crop_call(device, c["data"], c["factor"], c["crop"], c["records"], True, c["cp_shape"], c["mats"], shift=c["shift"])
    worst = against_reference(got, refs, name)
    print(f"{name} [{c['family']}]: modes {sorted({m for _r, m, _o, _b in refs})}, worst err / bound = {worst:.3f}")
    if c["family"] != "grid-cap":
        return
    # the batch against B = 1 calls of a handful of its crops (first, last, and where the draws and the samples wrap)
    B = c["B"]
    up = _upload(c["data"], device)
    for b in sorted({0, 1, 15, 16, 17, B // 2, B - 2, B - 1}):
        one, m = crop_call(device, c["data"], c["factor"], c["crop"], c["records"][b:b + 1], True, c["cp_shape"], c["mats"],
                           shift=c["shift"], uploaded=up)
        assert np.array_equal(one[0], got[b]), (name, b)


@pytest.mark.parametrize("name", ["cap-plain", "cap1-plain"])
def test_plain_batches_beyond_the_grid_cap_are_slicing(device, name):
    c = R.build_case(name)
    got, _ = crop_call(device, c["data"], c["factor"], c["crop"], c["records"], False, shift=c["shift"])
    norm = _normalised32(c["data"], c["factor"])
    for b, rec in enumerate(c["records"]):
        assert np.array_equal(got[b], norm[int(rec[0])][_slices(rec[1:], c["crop"])]), (name, b)
    for b, (ref, _mode, _room, _bound) in enumerate(R.case_reference(name)):
        assert np.array_equal(got[b].astype(np.float64), ref)
    up = _upload(c["data"], device)
    for b in (0, 1, c["B"] // 2, c["B"] - 1):
        one, _ = crop_call(device, c["data"], c["factor"], c["crop"], c["records"][b:b + 1], False, shift=c["shift"], uploaded=up)
        assert np.array_equal(one[0], got[b]), (name, b)


# ------------------------------------------------------------------------- d. the maximum across blocks, mixed signs
MAX_CROP, MAX_SPATIAL, MAX_OFF = (64, 64), (72, 80), (4, 8)


def _max_sources():
    """name -> data (2, 1, 72, 80) float32, two different samples; the window of the crop is spatial[4:68, 8:72]."""
    pl = R.plan(MAX_CROP, 1, 2, True)
    assert pl["tiles"] == 4 and pl["trips"] == 1 and R.plan(MAX_CROP, 1, 2, False)["tiles"] == 4
    tile = np.empty(MAX_CROP, dtype=np.int64)
    for y in range(MAX_CROP[0]):
        for x in range(MAX_CROP[1]):
            tile[y, x] = R.tile_of(pl, MAX_CROP, (y, x))
    assert [int((tile == t).sum()) for t in range(4)] == [1024] * 4
    base = -(R.random_data((2, 1) + MAX_SPATIAL, np.float32, seed=3) + np.float32(0.5))          # in [-1.5, -0.5]
    win = (slice(MAX_OFF[0], MAX_OFF[0] + 64), slice(MAX_OFF[1], MAX_OFF[1] + 64))
    out = {"all-negative": base.copy()}
    for t in range(4):
        one = base.copy()
        ys, xs = np.nonzero(tile == t)
        k = (7 * t + 3) % len(ys)
        one[0, 0][win][ys[k], xs[k]] = np.float32(0.75)               # sample 0: one positive voxel, in tile t only
        one[1, 0][win][ys[-1 - k], xs[-1 - k]] = np.float32(2.0 ** -100)  # sample 1: a tiny positive one
        out[f"one-positive-in-tile-{t}"] = one
        zeros = base.copy()
        zeros[0, 0][win][tile == t] = 0.0                            # zeros in tile t only
        zeros[1, 0][win][ys[k], xs[k]] = 0.0                         # a single zero
        out[f"zeros-in-tile-{t}"] = zeros
    return out


@pytest.mark.parametrize("elastic", [True, False], ids=["elastic", "plain"])
def test_maximum_across_blocks_with_mixed_signs(device, elastic):
    """float32, crop (64, 64), B = 2: four blocks per crop meet in one slot of maxima — an atomicMax on int bits from
    the blocks whose maximum is >= 0, an atomicMin on unsigned bits from those whose maximum is negative, in any order.
    The window is placed by integer offsets (A = I, u = 1/2, even margins), so raw is the window exactly and the
    maximum is known by value."""
    cp = R.cp_shape_for(MAX_CROP, 32)
    mats = R.make_mats(MAX_CROP, cp)
    rng = np.random.default_rng(0)
    if elastic:
        records = np.stack([R.make_record(cp, s, rng, A=np.eye(2), u=0.5) for s in (0, 1)])
    else:
        records = np.stack([R.plain_record(s, MAX_OFF) for s in (0, 1)])
    for name, data in _max_sources().items():
        got, mx = crop_call(device, data, 1.0, MAX_CROP, records, elastic, cp if elastic else None, mats if elastic else None)
        window = data[:, :, MAX_OFF[0]:MAX_OFF[0] + 64, MAX_OFF[1]:MAX_OFF[1] + 64]
        assert np.array_equal(got, window), name
        refs = R.ref_crops(data, 1.0, MAX_CROP, cp, mats, records, elastic)
        want = np.array([r[0].max() for r in refs])
        assert np.array_equal(mx.astype(np.float64), want), (name, mx, want)
        if name == "all-negative":
            assert (mx < 0).all()
