"""clx_region_moments / clx_region_intensity through the C ABI against a NumPy restatement (np.bincount, np.add.at,
np.minimum.at / np.maximum.at on 64-bit integers).  Everything is integer work: every output row from 1 up must be
EQUAL.  Outputs are prefilled with 0xAB bytes and sit between guard words that must stay untouched."""

import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                      # bytes before and after every output (keeps the outputs 16-byte aligned)
F32, F64, I32 = 0, 1, 2         # clx_raw_type


class Out:
    """A device output of `shape` / `dtype`, 0xAB-filled, between two guard zones."""

    def __init__(self, shape, dtype, device):
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=device)

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == 0xAB).all() and (host[GUARD + self.nbytes:] == 0xAB).all(), "guard words overwritten"
        return host[GUARD:GUARD + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def untouched(self):
        return bool((self.buf == 0xAB).all().item())


def _dev(a, device, offset=0):
    """numpy -> device tensor; offset > 0: the data starts `offset` elements into a 16-byte-aligned allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    if offset == 0:
        return t.to(device)
    big = torch.zeros(t.numel() + offset, dtype=t.dtype, device=device)
    big[offset:] = t.to(device)
    return big[offset:]


def run_moments(labels, nid, device, offset=0):
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32)
    Z, Y, X = (1,) * (3 - labels.ndim) + labels.shape
    lab = _dev(labels, device, offset)
    outs = dict(area=Out((nid,), np.uint64, device), bbox=Out((nid, 6), np.int32, device),
                sum1=Out((nid, 3), np.uint64, device), sum2=Out((nid, 6), np.uint64, device), bad=Out((1,), np.int32, device))
    status = _clx.load().clx_region_moments(_clx.ptr(lab), Z, Y, X, nid, outs["area"].ptr, outs["bbox"].ptr, outs["sum1"].ptr,
                                            outs["sum2"].ptr, outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return {k: v.get() for k, v in outs.items()}


def ref_moments(labels, nid):
    labels = np.asarray(labels, dtype=np.int64)
    shape = (1,) * (3 - labels.ndim) + labels.shape
    lab = labels.reshape(-1)
    coords = np.indices(shape).reshape(3, -1).astype(np.int64)
    ok = (lab > 0) & (lab < nid)
    ids = lab[ok]
    c = coords[:, ok].astype(np.uint64)
    area = np.bincount(ids, minlength=nid).astype(np.uint64)
    sum1 = np.zeros((nid, 3), dtype=np.uint64)
    sum2 = np.zeros((nid, 6), dtype=np.uint64)
    for k in range(3):
        np.add.at(sum1[:, k], ids, c[k])
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        np.add.at(sum2[:, k], ids, c[a] * c[b])
    bbox = np.empty((nid, 6), dtype=np.int32)
    bbox[:, :3] = 0x7FFFFFFF
    bbox[:, 3:] = -1
    for k in range(3):
        np.minimum.at(bbox[:, k], ids, coords[k, ok].astype(np.int32))
        np.maximum.at(bbox[:, 3 + k], ids, coords[k, ok].astype(np.int32))
    bad = int(((lab < 0) | (lab >= nid)).any())
    return dict(area=area, bbox=bbox, sum1=sum1, sum2=sum2, bad=np.array([bad], dtype=np.int32))


def assert_rows_equal(got, want):
    for k in want:
        if k == "bad":
            assert got[k][0] == want[k][0], f"bad: {got[k][0]} != {want[k][0]}"
        else:
            assert np.array_equal(got[k][1:], want[k][1:]), k


def _blobs(shape, n, seed):
    """seeded label map of n box-shaped objects separated by background"""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, dtype=np.int32)
    for i in range(1, n + 1):
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [min(s, a + int(rng.integers(1, max(2, s // 3)))) for s, a in zip(shape, lo)]
        lab[tuple(slice(a, b) for a, b in zip(lo, hi))] = i
    return lab


def _cases():
    c = {}
    c["one_pixel"] = (np.ones((1, 1), np.int32), 2)
    c["tail_lanes_5x67"] = (_blobs((5, 67), 6, 1), 7)
    # one run per image row over many waves and blocks; Σx and Σyx are wrong if a run continues into the next row
    c["one_label_3x1031"] = (np.full((3, 1031), 3, np.int32), 4)
    # no runs, and 1024 ids in the first block's pixels against its 256 table slots: the overflow route
    c["distinct_16x70"] = (np.arange(1, 1121, dtype=np.int32).reshape(16, 70), 1121)
    yy, xx = np.indices((16, 70))
    c["checkerboard_16x70"] = (((yy + xx) % 2 + 1).astype(np.int32), 3)
    sparse = np.zeros((9, 33), np.int32)
    sparse[2, 5:9] = 1
    sparse[7, 30:] = 65535
    sparse[8, 0] = 65535
    c["ids_1_and_65535"] = (sparse, 65536)
    c["all_background"] = (np.zeros((7, 19), np.int32), 5)
    c["separated_40x131"] = (_blobs((40, 131), 25, 2), 26)
    touching = np.zeros((5, 6, 7), np.int32)
    touching[:3] = 1
    touching[2:, 2:5, 1:6] = 2                      # labels meet across z, y and x
    c["3d_5x6x7"] = (touching, 3)
    c["3d_3x40x70"] = (_blobs((3, 40, 70), 12, 3), 13)
    # the grid is capped at 1024 blocks of 1024 pixels per trip (MAX_GRID, TILE in csrc/region_scan.h): 1030 x 1031 =
    # 1 061 930 pixels are 1038 tiles, so blocks take two tiles each
    c["second_trip_1030x1031"] = (_blobs((1030, 1031), 300, 4), 301)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_moments_equal_numpy(name, device):
    labels, nid = CASES[name]
    got = run_moments(labels, nid, device)
    want = ref_moments(labels, nid)
    assert_rows_equal(got, want)
    if name == "ids_1_and_65535":
        assert got["area"][2:65535].max() == 0 and got["bbox"][2:65535, 3:].max() < 0      # absent ids
        assert got["area"][1] == 4 and got["area"][65535] == 4
    if name == "all_background":
        assert got["area"][1:].max() == 0 and got["bbox"][1:, 3:].max() < 0 and got["bad"][0] == 0


@pytest.mark.parametrize("name", ["tail_lanes_5x67", "one_label_3x1031", "3d_3x40x70"])
def test_moments_unaligned_labels(name, device):
    """a label map that does not start on a 16-byte boundary takes the 4-byte loads"""
    labels, nid = CASES[name]
    assert_rows_equal(run_moments(labels, nid, device, offset=1), ref_moments(labels, nid))


def test_moments_bad_labels(device):
    labels = _blobs((12, 70), 9, 5)
    for value in (-1, -2 ** 31, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[3, 7] = value
        lab[11, 69] = value
        got = run_moments(lab, 10, device)               # run_moments checks the guard words
        want = ref_moments(lab, 10)
        assert want["bad"][0] == 1
        assert_rows_equal(got, want)


# ------------------------------------------------------------------------------------------------- intensity
def _keys(v):
    """clx_inst_stats' order-preserving keys of a float32 / float64 / int32 array, as uint64"""
    if v.dtype == np.int32:
        return (v.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    bits = v.view(np.uint32 if v.dtype == np.float32 else np.uint64)
    top = bits.dtype.type(1 << (bits.dtype.itemsize * 8 - 1))
    return np.where(bits & top, ~bits, bits | top).astype(np.uint64)


def run_intensity(labels, raw, nid, shift, device, offset=0):
    from cellulus_amd import _clx

    labels = np.asarray(labels, dtype=np.int32).reshape(-1)
    raw = np.ascontiguousarray(raw).reshape(-1)
    raw_type = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32}[raw.dtype]
    lab, rw = _dev(labels, device, offset), _dev(raw, device, offset)
    outs = dict(isum=Out((nid,), np.int64, device), vkey=Out((nid, 2), np.uint64, device), bad=Out((1,), np.int32, device))
    status = _clx.load().clx_region_intensity(_clx.ptr(lab), _clx.ptr(rw), raw_type, labels.size, nid, shift, outs["isum"].ptr,
                                              outs["vkey"].ptr, outs["bad"].ptr, _clx.stream_ptr(device))
    assert status == 0, _clx.load().clx_last_error()
    torch.cuda.synchronize(device)
    return {k: v.get() for k, v in outs.items()}, outs


def ref_intensity(labels, raw, nid, shift):
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    raw = np.ascontiguousarray(raw).reshape(-1)
    in_range = (lab >= 0) & (lab < nid)
    bad = 0 if in_range.all() else 1
    ok = in_range & (lab > 0)
    if raw.dtype == np.int32:
        q = raw.astype(np.int64)
    else:
        bound = float(2 ** 62 >> int(lab.size).bit_length())
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.rint(raw.astype(np.float64) * 2.0 ** shift)
            fits = np.abs(t) <= bound                       # False for NaN
        if (ok & ~fits).any():
            bad |= 2
        ok &= fits
        q = np.where(fits, t, 0.0).astype(np.int64)
    isum = np.zeros(nid, dtype=np.int64)
    np.add.at(isum, lab[ok], q[ok])
    vkey = np.empty((nid, 2), dtype=np.uint64)
    vkey[:, 0] = np.uint64(2 ** 64 - 1)
    vkey[:, 1] = 0
    k = _keys(raw)
    np.minimum.at(vkey[:, 0], lab[ok], k[ok])
    np.maximum.at(vkey[:, 1], lab[ok], k[ok])
    return dict(isum=isum, vkey=vkey, bad=np.array([bad], dtype=np.int32))


def _raw(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "i32":
        v = rng.integers(-2 ** 31 + 1, 2 ** 31, size=shape).astype(np.int32)
        v.reshape(-1)[::7] = 2 ** 31 - 1
        v.reshape(-1)[3::11] = -(2 ** 31 - 1)
        return v
    v = rng.normal(0, 100.0, size=shape) * np.exp(rng.normal(0, 3.0, size=shape))
    return v.astype(np.float32 if kind == "f32" else np.float64)


@pytest.mark.parametrize("kind", ["i32", "f32", "f64"])
@pytest.mark.parametrize("name", ["one_pixel", "tail_lanes_5x67", "one_label_3x1031", "distinct_16x70", "checkerboard_16x70",
                                  "ids_1_and_65535", "all_background", "3d_3x40x70", "second_trip_1030x1031"])
def test_intensity_equal_numpy(name, kind, device):
    from cellulus_amd.measure import intensity_shift

    labels, nid = CASES[name]
    raw = _raw(kind, labels.shape, 11)
    shift = 0 if kind == "i32" else intensity_shift(float(np.abs(raw).max()), labels.size)
    got, _ = run_intensity(labels, raw, nid, shift, device)
    want = ref_intensity(labels, raw, nid, shift)
    assert want["bad"][0] == 0
    assert_rows_equal(got, want)


@pytest.mark.parametrize("kind", ["i32", "f32", "f64"])
def test_intensity_unaligned(kind, device):
    from cellulus_amd.measure import intensity_shift

    labels, nid = CASES["separated_40x131"]
    raw = _raw(kind, labels.shape, 12)
    shift = 0 if kind == "i32" else intensity_shift(float(np.abs(raw).max()), labels.size)
    got, _ = run_intensity(labels, raw, nid, shift, device, offset=1)
    assert_rows_equal(got, ref_intensity(labels, raw, nid, shift))


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_intensity_sum_within_derived_bound_and_keys_decode(kind, device):
    """|Σq·2^-shift − Σv| <= area·2^-(shift+1): every q is within half a unit of v·2^shift.  The keys decode to
    numpy's min / max."""
    from cellulus_amd.measure import intensity_shift
    from cellulus_amd.segment import _decode_keys

    labels, nid = CASES["separated_40x131"]
    raw = _raw(kind, labels.shape, 13)
    shift = intensity_shift(float(np.abs(raw).max()), labels.size)
    got, _ = run_intensity(labels, raw, nid, shift, device)
    vals = _decode_keys(got["vkey"], F32 if kind == "f32" else F64)
    for i in range(1, nid):
        v = raw[labels == i]
        if v.size == 0:
            continue
        exact = sum(Fraction(float(x)) for x in v)
        assert abs(Fraction(int(got["isum"][i])) / Fraction(2) ** shift - exact) <= v.size * Fraction(1, 2 ** (shift + 1))
        assert abs(math.ldexp(int(got["isum"][i]), -shift) - math.fsum(v.tolist())) <= v.size * 2.0 ** -(shift + 1) * (1 + 2 ** -50)
        assert vals[i, 0] == v.min() and vals[i, 1] == v.max()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_intensity_signed_zeros_and_denormals(kind, device):
    from cellulus_amd.measure import intensity_shift
    from cellulus_amd.segment import _decode_keys

    dt = np.float32 if kind == "f32" else np.float64
    tiny = np.finfo(dt).smallest_subnormal if hasattr(np.finfo(dt), "smallest_subnormal") else np.nextafter(dt(0), dt(1))
    labels = np.zeros((4, 70), np.int32)
    labels[0] = 1
    labels[1] = 2
    labels[2, :35] = 3
    labels[3, 10:] = 4
    raw = np.ones((4, 70), dt)
    raw[0, ::2] = 0.0
    raw[0, 1::2] = -0.0                                   # object 1: only zeros of both signs
    raw[1] = tiny
    raw[1, ::3] = -tiny * 5                               # object 2: only denormals -> every q is 0
    raw[2, :35] = -0.0                                    # object 3: only -0.0
    shift = intensity_shift(1.0, labels.size)
    got, _ = run_intensity(labels, raw, 5, shift, device)
    want = ref_intensity(labels, raw, 5, shift)
    assert want["bad"][0] == 0
    assert_rows_equal(got, want)
    assert got["isum"][1] == 0 and got["isum"][2] == 0 and got["isum"][3] == 0 and got["isum"][4] == 60 << shift
    vals = _decode_keys(got["vkey"], F32 if kind == "f32" else F64)
    # clx_inst_stats' keys order -0.0 below +0.0
    assert vals[1, 0] == 0 and np.signbit(vals[1, 0]) and vals[1, 1] == 0 and not np.signbit(vals[1, 1])
    assert vals[2, 0] == -tiny * 5 and vals[2, 1] == tiny
    assert np.signbit(vals[3, 0]) and np.signbit(vals[3, 1])


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_intensity_non_finite_sets_bad(kind, poison, device):
    from cellulus_amd.measure import intensity_shift

    labels, nid = CASES["separated_40x131"]
    raw = _raw(kind, labels.shape, 14)
    shift = intensity_shift(float(np.abs(raw).max()), labels.size)
    y, x = np.argwhere(labels > 0)[17]
    raw[y, x] = poison
    raw[0, 0] = poison if labels[0, 0] == 0 else raw[0, 0]      # non-finite background is not an error
    got, _ = run_intensity(labels, raw, nid, shift, device)
    want = ref_intensity(labels, raw, nid, shift)                # skips that one pixel
    assert got["bad"][0] == 2 and want["bad"][0] == 2
    assert_rows_equal(got, want)


def test_intensity_shift_too_large_sets_bad(device):
    from cellulus_amd.measure import intensity_shift

    labels, nid = CASES["tail_lanes_5x67"]
    raw = _raw("f32", labels.shape, 15)
    shift = intensity_shift(float(np.abs(raw).max()), labels.size) + 3
    got, _ = run_intensity(labels, raw, nid, shift, device)
    want = ref_intensity(labels, raw, nid, shift)                # the pixels above the bound are skipped
    assert got["bad"][0] == 2 and want["bad"][0] == 2
    assert_rows_equal(got, want)
    got, _ = run_intensity(labels, raw, nid, 1023, device)       # far too large: q would not fit in 64 bits
    assert got["bad"][0] == 2
    assert_rows_equal(got, ref_intensity(labels, raw, nid, 1023))


def test_intensity_bad_labels(device):
    labels = _blobs((12, 70), 9, 5)
    raw = _raw("f32", labels.shape, 16)
    for value in (-1, 10, 2 ** 31 - 1):
        lab = labels.copy()
        lab[3, 7] = value
        lab[11, 69] = value
        got, _ = run_intensity(lab, raw, 10, 20, device)
        want = ref_intensity(lab, raw, 10, 20)
        assert got["bad"][0] == 1 and want["bad"][0] == 1
        assert_rows_equal(got, want)


def test_reproducible(device):
    from cellulus_amd.measure import intensity_shift

    labels, nid = CASES["checkerboard_16x70"]
    raw = _raw("f32", labels.shape, 17)
    shift = intensity_shift(float(np.abs(raw).max()), labels.size)
    runs = []
    for _ in range(2):
        _, outs = run_intensity(labels, raw, nid, shift, device)
        runs.append(outs)
    for k in runs[0]:
        skip = GUARD + (0 if k == "bad" else runs[0][k].nbytes // nid)         # row 0 is unspecified
        assert torch.equal(runs[0][k].buf[skip:], runs[1][k].buf[skip:]), k
    m = [run_moments(labels, nid, device) for _ in range(2)]
    for k in m[0]:
        assert np.array_equal(m[0][k][1:] if k != "bad" else m[0][k], m[1][k][1:] if k != "bad" else m[1][k]), k


# ------------------------------------------------------------------------------------------- rejected arguments
def test_rejected_arguments_launch_nothing(device):
    import ctypes

    from cellulus_amd import _clx

    lib = _clx.load()
    st = _clx.stream_ptr(device)
    lab = torch.zeros(64, dtype=torch.int32, device=device)
    raw = torch.zeros(64, dtype=torch.float32, device=device)
    names = ("area", "bbox", "sum1", "sum2", "bad")
    outs = {k: Out((64,), np.uint64, device) for k in names + ("isum", "vkey")}
    null = ctypes.c_void_p(0)

    def moments(Z=1, Y=8, X=8, nid=4, **ptrs):
        p = {k: outs[k].ptr for k in names}
        p["labels"] = _clx.ptr(lab)
        p.update(ptrs)
        return lib.clx_region_moments(p["labels"], Z, Y, X, nid, p["area"], p["bbox"], p["sum1"], p["sum2"], p["bad"], st)

    def intensity(raw_type=F32, npix=64, nid=4, **ptrs):
        p = dict(labels=_clx.ptr(lab), raw=_clx.ptr(raw), isum=outs["isum"].ptr, vkey=outs["vkey"].ptr, bad=outs["bad"].ptr)
        p.update(ptrs)
        return lib.clx_region_intensity(p["labels"], p["raw"], raw_type, npix, nid, 0, p["isum"], p["vkey"], p["bad"], st)

    refused = [
        lambda: moments(nid=0), lambda: moments(nid=-3), lambda: moments(nid=2 ** 24 + 1),
        lambda: moments(Y=65536, X=65536),                      # npix = 2^32
        lambda: moments(Z=2, Y=46341, X=46341),                 # npix just above 2^32
        lambda: moments(Y=1, X=3_000_000),                      # (X-1)^2 * npix = 2.7e19 >= 2^63 with npix < 2^32
        lambda: moments(Y=2, X=2 ** 31 - 1),
        lambda: moments(Z=0), lambda: moments(Y=-1),
    ] + [lambda k=k: moments(**{k: null}) for k in names + ("labels",)] + [
        lambda: intensity(nid=0), lambda: intensity(nid=2 ** 24 + 1), lambda: intensity(npix=2 ** 32), lambda: intensity(npix=0),
        lambda: intensity(raw_type=3), lambda: intensity(raw_type=-1),
    ] + [lambda k=k: intensity(**{k: null}) for k in ("labels", "raw", "isum", "vkey", "bad")]
    for i, call in enumerate(refused):
        status = call()
        assert status < 0, f"case {i} was accepted"
        assert len(lib.clx_last_error()) > 0, f"case {i} left no message"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    assert moments() == 0 and intensity() == 0                   # the same buffers are accepted with valid arguments
    torch.cuda.synchronize(device)
