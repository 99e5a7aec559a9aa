"""The kernels of csrc/meanshift.hip through the C ABI against the float64 NumPy restatements of meanshift_ref.py.

Constants mirrored from the source: a wave-tile is 1024 pixels (64 lanes x 16-byte groups: 8 x 2 doubles or 4 x 4
floats); the flags pass runs in at most 2048 blocks, each over a contiguous chunk of tiles that is a multiple of 4
(4 tiles per block up to 8192 tiles = 2^23 pixels, 8 from there); the scatter pass adds up the chunks in front of a
tile 256 at a time; BUCKET_BIG = 2048 points in a cell hand the ranking from a wavefront to a thread per point;
ms_assign_kernel stages CHUNK = 1024 centres at a time; the iteration takes 4 seeds per block and 64 points per trip;
GRID_MIN_POINTS = 2048 fit points switch mean_shift_on_device from the brute-force to the bucketed iteration.

Everything but the centres of the real-valued iteration must be EQUAL to the reference: the compaction and the
assignment do one IEEE operation at a time in a fixed order (the file is compiled with -ffp-contract=off), and on
lattice data (multiples of 1/4 below 1024) every sum of the iteration is exact in any order.  Outputs and workspaces
are 0xAB-filled and sit between guard zones that must stay untouched."""

import ctypes

import numpy as np
import pytest
import torch

from meanshift_ref import ref_assign, ref_bucket, ref_iterate, ref_margin, ref_prepare
from test_gpu_measure import GUARD, Out, _dev

pytestmark = pytest.mark.gpu

WAVE_TILE = 1024
BUCKET_BIG = 2048
CHUNK = 1024
MEMBER_MARGIN = 1e-6        # a seed counts only if every |d2 - bw^2| of its run is at least this ...
STOP_MARGIN = 1e-9          # ... and every |sqrt(shift2) - 1e-3 bw| at least this
ORDER_FACTOR = 16.0         # centre tolerance = 16 x the largest difference between three summation orders of the reference


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    if not np.array_equal(_bits(got), _bits(want)):
        bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at {bad[0]}: "
                             f"{got.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}")


def _lib():
    from cellulus_amd import _clx

    return _clx, _clx.load()


def _ok(status):
    _clx, lib = _lib()
    assert status == 0, lib.clx_last_error().decode()


def _cdoubles(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


# ----------------------------------------------------------------------------------------------------------- prepare
def prepare_patterns(npix, rng):
    """name -> (std as float64 — every value is exact in float32 —, threshold)"""
    tile = np.ones(npix)
    t0 = WAVE_TILE * min(1, (npix - 1) // WAVE_TILE)
    tile[t0:t0 + WAVE_TILE] = 0.25                      # exactly the pixels of one whole wave-tile (what the image has of it)
    special = np.resize(np.array([np.nan, np.inf, -np.inf, 0.25, 0.75, 0.5]), npix)
    zero = np.resize(np.array([-0.0, 0.0, -1.0, -0.0, 0.0, 0.0, -0.0]), npix)
    p = {
        "none": (np.ones(npix), 0.5), "all": (np.zeros(npix), 0.5),
        "first": (np.where(np.arange(npix) == 0, 0.25, 1.0), 0.5),
        "last": (np.where(np.arange(npix) == npix - 1, 0.25, 1.0), 0.5),
        "alternate": (np.where(np.arange(npix) % 2 == 0, 0.25, 1.0), 0.5),
        "one_tile": (tile, 0.5),
        "at_threshold": (np.where(rng.random(npix) < 0.3, 0.25, 0.5), 0.5),      # std == thr is background
        "nan_inf": (special, 0.5),                     # NaN, +inf, 0.75, 0.5: background; -inf, 0.25: foreground
        "neg_zero": (zero, 0.0),                       # -0.0 < 0.0 is false: only the -1.0 are foreground
    }
    for pct in (2, 50, 98):
        p[f"random_{pct}"] = (np.where(rng.random(npix) < pct / 100.0, 0.25, 1.0), 0.5)
    return p


def run_prepare(emb, std, thr, device, emb_off=0, std_off=0, with_index=True, ws_fill=0xAB):
    """One call of clx_ms_prepare (float64 inputs) or clx_ms_prepare_f32 (float32) -> dict of host arrays + the
    device buffers a following clx_ms_assign_dense needs."""
    _clx, lib = _lib()
    nd, spatial = emb.shape[0], emb.shape[1:]
    Z, Y, X = (1,) * (3 - nd) + tuple(spatial)
    npix = Z * Y * X
    f32 = emb.dtype == np.float32
    assert std.dtype == emb.dtype
    emb_d, std_d = _dev(emb, device, emb_off), _dev(std, device, std_off)
    pts = Out((npix, nd), np.float64, device)
    index = Out((npix,), np.int32, device)
    nfg = Out((1,), np.int32, device)
    ws = Out((int(lib.clx_ms_prepare_workspace(npix)),), np.uint8, device)
    ws.buf[GUARD:GUARD + ws.nbytes].fill_(ws_fill)
    fn = lib.clx_ms_prepare_f32 if f32 else lib.clx_ms_prepare
    _ok(fn(_clx.ptr(emb_d), _clx.ptr(std_d), float(thr), nd, Z, Y, X, pts.ptr, index.ptr if with_index else ctypes.c_void_p(0),
           nfg.ptr, ws.ptr, _clx.stream_ptr(device)))
    torch.cuda.synchronize(device)
    host_ws = ws.buf.cpu().numpy()
    assert (host_ws[:GUARD] == 0xAB).all() and (host_ws[GUARD + ws.nbytes:] == 0xAB).all(), "workspace guards overwritten"
    return dict(nfg=int(nfg.get()[0]), points=pts.get(), index=index.get(), emb=emb_d.cpu().numpy().reshape(emb.shape),
                pts_out=pts, ws_out=ws, f32=f32, dims=(Z, Y, X), nd=nd)


def run_dense_one_centre(r, device):
    """clx_ms_assign_dense with ONE centre in a 1 x 1 (x 1) grid on the workspace a prepare call left: label 1 on every
    foreground pixel, 0 elsewhere — the flag words and the points-in-front-of-every-tile the compaction keeps."""
    _clx, lib = _lib()
    nd = r["nd"]
    Z, Y, X = r["dims"]
    centre = _dev(np.zeros(nd), device)
    order = _dev(np.zeros(1, np.int32), device)
    start = _dev(np.array([0, 1], np.int32), device)
    labels = Out((Z * Y * X,), np.int32, device)
    _ok(lib.clx_ms_assign_dense(r["pts_out"].ptr, _clx.ptr(centre), 1, nd, _clx.ptr(order), _clx.ptr(start), _cdoubles([0.0] * nd),
                                1.0, 1, 1, 1, r["ws_out"].ptr, 1 if r["f32"] else 0, Z, Y, X, labels.ptr, _clx.stream_ptr(device)))
    torch.cuda.synchronize(device)
    return labels.get()


def check_prepare(emb, std, thr, device, emb_off=0, std_off=0, what=""):
    """Both forms of a prepare entry (with the raster index on a 0xAB workspace, without it on a 0x5C one) against
    ref_prepare, then the dense pass on the second call's workspace."""
    points, index, after = ref_prepare(emb, std, thr)
    nfg, npix = len(index), std.size
    filler = np.frombuffer(b"\xab" * 8, dtype=np.float64)[0]
    for with_index, fill in ((True, 0xAB), (False, 0x5C)):
        r = run_prepare(emb, std, thr, device, emb_off, std_off, with_index, fill)
        tag = f"{what} index={with_index}"
        assert r["nfg"] == nfg, f"{tag}: nfg {r['nfg']} != {nfg}"
        assert_same_bits(r["points"][:nfg], points, tag + " points")
        assert_same_bits(r["points"][nfg:], np.full((npix - nfg, emb.shape[0]), filler), tag + " rows behind nfg")
        if with_index:
            assert np.array_equal(r["index"][:nfg], index), tag + " raster index"
            assert (_bits(r["index"][nfg:]) == 0xABABABAB).all(), tag + " index behind nfg"
        else:
            assert (_bits(r["index"]) == 0xABABABAB).all(), tag + " index written although NULL was passed"
        if r["f32"]:
            assert_same_bits(r["emb"], emb, tag + " float32 embedding modified")
        else:
            assert_same_bits(r["emb"], after, tag + " coordinate-added embedding")
    with np.errstate(invalid="ignore"):
        want = (std.astype(np.float64).reshape(-1) < thr).astype(np.int32)
    assert np.array_equal(run_dense_one_centre(r, device), want), f"{what}: dense labels of one centre != (std < thr)"


def prepare_inputs(shape, dtype, rng):
    nd = len(shape)
    return rng.normal(0.0, 3.0, size=(nd,) + tuple(shape)).astype(dtype)


ROW_SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289]
IMAGES = [(19, 1), (7, 2), (5, 3), (9, 5), (61, 67), (64, 80), (3, 5, 7), (5, 1, 3), (2, 33, 65), (12, 20, 24)]
PREPARE_SHAPES = [(1, n) for n in ROW_SIZES] + IMAGES


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", PREPARE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prepare_equals_reference(shape, dtype, device):
    rng = np.random.default_rng(sum(shape))
    emb = prepare_inputs(shape, dtype, rng)
    npix = int(np.prod(shape))
    for name, (std, thr) in prepare_patterns(npix, rng).items():
        check_prepare(emb, std.astype(dtype).reshape(shape), thr, device, what=f"{shape} {name}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(1, 1024), (1, 4096), (64, 80), (12, 20, 24)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("which", ["emb", "std"])
def test_prepare_scalar_fallback_of_unaligned_planes(which, shape, dtype, device):
    """npix is a multiple of the 16-byte group, but one plane starts one element past a 16-byte boundary."""
    rng = np.random.default_rng(7 + sum(shape))
    emb = prepare_inputs(shape, dtype, rng)
    npix = int(np.prod(shape))
    assert npix % 4 == 0
    pats = prepare_patterns(npix, rng)
    for name in ("random_50", "all", "nan_inf", "one_tile"):
        std, thr = pats[name]
        check_prepare(emb, std.astype(dtype).reshape(shape), thr, device, emb_off=int(which == "emb"),
                      std_off=int(which == "std"), what=f"{shape} {name} {which}+1")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(1, 256 * 4096 + 5), (1027, 1025), (600, 2050)], ids=lambda s: "x".join(map(str, s)))
def test_prepare_more_than_256_chunks(shape, dtype, device):
    """4 tiles per block and more than 256 blocks in the flags pass: 257 chunks — the last tile has exactly 256 chunks
    in front of it, one full trip of the scatter pass's chunk sum —, 258 — the first second trip, one value — and 301."""
    npix = int(np.prod(shape))
    assert (npix + 4095) // 4096 > 256
    rng = np.random.default_rng(npix % 1000)
    emb = prepare_inputs(shape, dtype, rng)
    std = np.where(rng.random(npix) < 0.5, 0.25, 1.0)
    std[:3 * WAVE_TILE] = 1.0                            # (empty leading tiles, a full stretch in the far chunks)
    std[-40 * WAVE_TILE:-38 * WAVE_TILE] = 0.25
    check_prepare(emb, std.astype(dtype).reshape(shape), 0.5, device, what=f"{shape}")


def large_prepare_inputs():
    """(2049, 4100) float32: 8208 tiles -> 8 tiles per block, 1026 chunks (5 trips of the chunk sum), more than 2048
    tiles per quarter — the configuration of the 4096^2 workload."""
    shape = (2049, 4100)
    rng = np.random.default_rng(2049)
    npix = shape[0] * shape[1]
    emb = rng.integers(-64, 64, size=(2,) + shape).astype(np.float32)
    emb += np.float32(0.25)
    std = np.where(rng.random(npix) < 0.3, np.float32(0.25), np.float32(1.0)).astype(np.float32)
    std[:9 * WAVE_TILE] = 1.0
    std[npix // 2: npix // 2 + 17 * WAVE_TILE + 3] = 0.25
    return emb, std.reshape(shape)


def test_prepare_f32_at_eight_tiles_per_block(device):
    emb, std = large_prepare_inputs()
    npix = std.size
    nwt = (npix + 4095) // 4096 * 4
    assert nwt > 8192 and -(-nwt // 2048) > 4 and nwt // 4 > 2048
    points, index, _ = ref_prepare(emb, std, 0.5)
    nfg = len(index)
    r = run_prepare(emb, std, 0.5, device)
    assert r["nfg"] == nfg
    assert_same_bits(r["points"][:nfg], points, "points")
    assert np.array_equal(r["index"][:nfg], index)
    assert (_bits(r["points"][nfg:]) == 0xABABABABABABABAB).all() and (_bits(r["index"][nfg:]) == 0xABABABAB).all()
    assert_same_bits(r["emb"], emb, "float32 embedding modified")
    assert np.array_equal(run_dense_one_centre(r, device), (std.reshape(-1) < 0.5).astype(np.int32))


# ----------------------------------------------------------------------------------------------------------- iterate
def run_iterate(fit, seeds, nd, bw, max_iter, device, grid=False):
    """clx_ms_iterate, or clx_ms_iterate_grid on the buckets MS._bucket makes -> (centres, counts, iters) with the
    0xAB prefill where nothing was written."""
    from cellulus_amd.utils import mean_shift as MS

    _clx, lib = _lib()
    fit = np.ascontiguousarray(fit, dtype=np.float64).reshape(-1, nd)
    seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, nd)
    ns = len(seeds)
    fit_d = _dev(fit if len(fit) else np.zeros((1, nd)), device).view(-1, nd)
    seeds_d = _dev(seeds if ns else np.zeros((1, nd)), device)
    c, n, it = Out((max(ns, 1), nd), np.float64, device), Out((max(ns, 1),), np.int32, device), Out((max(ns, 1),), np.int32, device)
    st = _clx.stream_ptr(device)
    if grid:
        fs, cell_start, origin, cell, (nx, ny, nz) = MS._bucket(fit_d[:len(fit)], bw)
        _ok(lib.clx_ms_iterate_grid(_clx.ptr(fs), len(fit), _clx.ptr(cell_start), _cdoubles(origin), cell, nx, ny, nz,
                                    _clx.ptr(seeds_d), ns, nd, float(bw), max_iter, c.ptr, n.ptr, it.ptr, st))
    else:
        _ok(lib.clx_ms_iterate(_clx.ptr(fit_d), len(fit), _clx.ptr(seeds_d), ns, nd, float(bw), max_iter, c.ptr, n.ptr, it.ptr, st))
    torch.cuda.synchronize(device)
    return c.get(), n.get(), it.get()


def check_iterate_exact(fit, seeds, nd, bw, max_iter, device, forms=(False, True), what=""):
    want = ref_iterate(np.reshape(fit, (-1, nd)), np.reshape(seeds, (-1, nd)), bw, max_iter)
    for grid in forms:
        got = run_iterate(fit, seeds, nd, bw, max_iter, device, grid)
        tag = f"{what} {'grid' if grid else 'brute'}"
        ns = len(want[1])
        assert np.array_equal(got[1][:ns], want[1]), f"{tag}: counts {got[1][:ns]} != {want[1]}"
        assert np.array_equal(got[2][:ns], want[2]), f"{tag}: iterations {got[2][:ns]} != {want[2]}"
        assert_same_bits(got[0][:ns], want[0], tag + " centres")
    return want


def lattice_clusters(nd, nfit, nseeds, seed, bw=5.0):
    """Points and seeds on the lattice of quarters, |x| < 1024: clusters of a few bandwidths' width around integer
    centres (with duplicates), seeds next to fit points — some between clusters, so that they walk."""
    rng = np.random.default_rng(seed)
    k = max(1, min(6, nfit // 40))
    span = 900 if nd == 2 else 150                      # (the bucketed form makes a grid over the extent: 360^2 or 60^3 cells)
    cc = rng.integers(-span, span, size=(k, nd)).astype(np.float64)
    fit = cc[rng.integers(0, k, size=nfit)] + rng.integers(-24, 25, size=(nfit, nd)) / 4.0
    if nfit > 8:
        fit[nfit // 2] = fit[0]                                                  # duplicate points
        fit[nfit // 2 + 1] = fit[0]
    seeds = fit[rng.integers(0, nfit, size=nseeds)] + rng.integers(-8, 9, size=(nseeds, nd)) / 4.0
    assert np.abs(fit).max() < 1024 and (fit * 4 == np.round(fit * 4)).all() and (seeds * 4 == np.round(seeds * 4)).all()
    return fit, seeds, bw


NFITS = [1, 63, 64, 65, 257, 3000]
NSEEDS = [1, 3, 4, 5, 129]


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("nfit", NFITS)
def test_iterate_lattice_equals_reference(nfit, nd, device):
    for nseeds in NSEEDS:
        fit, seeds, bw = lattice_clusters(nd, nfit, nseeds, 100 * nfit + nseeds + nd)
        check_iterate_exact(fit, seeds, nd, bw, 300, device, what=f"nfit {nfit} nseeds {nseeds}")


def max_iter_case(nd):
    fit, seeds, bw = lattice_clusters(nd, 600, 37, 11 + nd)
    return fit, seeds, bw


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("max_iter", [0, 1, 2, 300])
def test_iterate_stops_at_max_iter(max_iter, nd, device):
    fit, seeds, bw = max_iter_case(nd)
    _, _, it = check_iterate_exact(fit, seeds, nd, bw, max_iter, device, what=f"max_iter {max_iter}")
    free = ref_iterate(fit, seeds, bw, 300)[2]
    assert it.max() <= max_iter
    if max_iter < 300:
        assert (free > max_iter).any() and (it[free > max_iter] == max_iter).all()      # seeds that max_iter really stopped


@pytest.mark.parametrize("nd", [2, 3])
def test_iterate_empty_sets_lonely_seeds_and_the_sphere(nd, device):
    _clx, lib = _lib()
    fit, seeds, bw = lattice_clusters(nd, 300, 9, 5)
    # no fit point: the centre is the seed, count 0, no iteration (brute force; a grid needs a point to have an origin)
    c, n, it = run_iterate(np.zeros((0, nd)), seeds, nd, bw, 300, device)
    assert_same_bits(c, seeds, "nfit 0 centres")
    assert (n == 0).all() and (it == 0).all()
    # no seed: nothing is written
    for grid in (False, True):
        c, n, it = run_iterate(fit, np.zeros((0, nd)), nd, bw, 300, device, grid)
        assert (_bits(c) == 0xABABABABABABABAB).all() and (_bits(n) == 0xABABABAB).all() and (_bits(it) == 0xABABABAB).all()
    # a seed without a member among seeds with members (inside the points' extent, so inside the grid as well)
    lonely = fit[:9].copy()                              # (each its own member at bandwidth 1/4)
    lonely[4] = fit.min(axis=0) + 0.5 * (fit.max(axis=0) - fit.min(axis=0))
    lonely[4] = np.round(lonely[4] * 4) / 4
    for r, forms in ((0.25, (False,)), (bw, (False, True))):       # (a grid of edge 1/4 over this extent would have 2^30 cells)
        want = check_iterate_exact(fit, lonely, nd, r, 300, device, forms, what=f"lonely, bandwidth {r}")
        assert np.array_equal(want[1] == 0, np.arange(9) == 4)
        assert_same_bits(want[0][4], lonely[4], "a seed without members stays where it is")
    # a point exactly ON the sphere is a member: d2 == bw^2
    far = [(0.0, 0.0), (3.0, 4.0)] if nd == 2 else [(0.0, 0.0, 0.0), (2.0, 3.0, 6.0)]
    r = 5.0 if nd == 2 else 7.0
    for max_iter in (0, 300):
        want = check_iterate_exact(np.array(far), np.array(far[:1]), nd, r, max_iter, device, what="sphere")
        if max_iter == 0:
            assert want[1][0] == 2 and want[2][0] == 0
            assert_same_bits(want[0][0], 0.5 * np.array(far[1]), "centre of the two")


def grid_box(nd):
    """All integer points of [0, 20]^ND, bandwidth 5: MS._bucket makes 4 cells of edge 5 (1 + 1e-9) per axis, the
    points at 20 sit just below the upper face of the last cell."""
    axes = [np.arange(21.0)] * nd
    fit = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, nd)
    return fit, 5.0


def outside_seeds(nd, off):
    """per axis and side, a seed `off` beyond the box in that axis, mid-range (10.25) in the others"""
    seeds = []
    for ax in range(nd):
        for v in (-off, 20.0 + off):
            s = [10.25] * nd
            s[ax] = v
            seeds.append(s)
    return np.array(seeds)


@pytest.mark.parametrize("nd", [2, 3])
def test_iterate_grid_seeds_outside_the_grid(nd, device):
    fit, bw = grid_box(nd)
    cell = bw * (1.0 + 1e-9)
    one = outside_seeds(nd, 0.25)                        # cell -1 and cell 4 of a 4-cell axis: their neighbours inside are within bw
    assert (np.floor(one / cell).min(axis=1) == -1).sum() == nd and (np.floor(one / cell).max(axis=1) == 4).sum() == nd
    want = check_iterate_exact(fit, one, nd, bw, 300, device, what="one cell outside")
    assert (want[1] > 0).all()
    two = outside_seeds(nd, 5.25)                        # two cells outside, and farther than bw from every point
    assert (np.floor(two / cell).min(axis=1) == -2).sum() == nd and (np.floor(two / cell).max(axis=1) == 5).sum() == nd
    want = check_iterate_exact(fit, two, nd, bw, 300, device, what="two cells outside")
    assert (want[1] == 0).all()
    # seeds whose cell coordinate does not fit an int, in every axis together and in one axis at a time (x inside the
    # grid and y at 1e300 once sent the kernel to row INT_MIN of cell_start)
    huge = np.concatenate([np.full((1, nd), 1e300), np.full((1, nd), -1e300), outside_seeds(nd, 1e300)])
    odd = np.full((5, nd), 10.25)                        # ... and seeds that are not finite: no member either
    odd[0], odd[1], odd[2], odd[3, 1], odd[4, nd - 1] = np.inf, -np.inf, np.nan, np.inf, np.nan
    huge = np.concatenate([huge, odd])
    want = check_iterate_exact(fit, huge, nd, bw, 300, device, what="1e300")
    assert (want[1] == 0).all() and (want[2] == 0).all()


@pytest.mark.parametrize("nd", [2, 3])
def test_iterate_grid_thin_grids_faces_and_empty_cells(nd, device):
    from cellulus_amd.utils import mean_shift as MS

    rng = np.random.default_rng(40 + nd)
    bw = 5.0
    # a grid of ONE cell: every point within less than a cell of the origin
    fit = rng.integers(0, 19, size=(200, nd)) / 4.0
    seeds = fit[::5] + 0.25
    assert MS._bucket(_dev(fit, device).view(-1, nd), bw)[4] == (1, 1, 1)
    check_iterate_exact(fit, seeds, nd, bw, 300, device, what="one cell")
    # one cell thick in each axis in turn, many cells in the others
    for thin in range(nd):
        fit = rng.integers(0, 400, size=(900, nd)) / 4.0
        fit[:, thin] = rng.integers(0, 16, size=900) / 4.0
        seeds = fit[::9] + 0.5
        dims = MS._bucket(_dev(fit, device).view(-1, nd), bw)[4]
        assert dims[thin] == 1 and all(d > 10 for a, d in enumerate(dims[:nd]) if a != thin)
        check_iterate_exact(fit, seeds, nd, bw, 300, device, what=f"thin axis {thin}")
    # points ON cell faces: origin + k * cell per axis for even k — two cells from one another, so a seed within half
    # a bandwidth of one has exactly that one member —, seeds around each of them
    fit, origin, cell = iterate_face_points(nd, bw)
    fs, cell_start, org, h, dims = MS._bucket(_dev(fit, device).view(-1, nd), bw)
    want_dims = tuple(int(d) for d in np.floor((fit.max(axis=0) - origin) / cell) + 1)
    assert h == cell and np.array_equal(org, origin) and dims[:nd] == want_dims and min(want_dims) >= 6
    assert_same_bits(fs.cpu().numpy(), ref_bucket(fit, origin, cell, want_dims)[0], "face points bucketed")
    seeds = np.concatenate([fit + o for o in FACE_SEED_OFFSETS[:, :nd]])
    want = check_iterate_exact(fit, seeds, nd, bw, 300, device, what="faces")
    assert (want[1] == 1).all()
    # clusters several cells apart: empty cells between occupied ones
    fit, seeds, _ = lattice_clusters(nd, 800, 61, 77)
    start = MS._bucket(_dev(fit, device).view(-1, nd), bw)[1].cpu().numpy()
    occupied = np.flatnonzero(np.diff(start) > 0)
    assert len(occupied) < occupied[-1] - occupied[0]
    check_iterate_exact(fit, seeds, nd, bw, 300, device, what="empty cells")


FACE_SEED_OFFSETS = np.array([[1.0, 0.5, -0.25], [-1.25, 0.0, 0.75], [0.0, -2.0, 1.5]])


def iterate_face_points(nd, bw):
    origin = np.array([-7.25, 3.5, 40.0][:nd])
    cell = bw * (1.0 + 1e-9)                              # the edge MS._bucket chooses
    ks = np.stack(np.meshgrid(*[2.0 * np.arange(4.0)] * nd, indexing="ij"), -1).reshape(-1, nd)
    return origin + ks * cell, origin, cell


def normal_clusters(nd):
    """Real-valued data, as test_mean_shift_kernels_match_oracle_numbers has it: three normal clusters of 300 points,
    sigma 2, bandwidth 6, every seventh point a seed (129 seeds)."""
    rng = np.random.default_rng(nd)
    cc = ((10, 10), (60, 20), (30, 70)) if nd == 2 else ((10, 10, 10), (60, 20, 35), (30, 70, 50))
    fit = np.concatenate([rng.normal(c, 2.0, size=(300, nd)) for c in cc])
    return fit, fit[::7].copy(), 6.0


_ORDER_CACHE = {}


def summation_orders(nd):
    """The reference on normal_clusters(nd) with the member sum taken forward, backward and pairwise -> (forward result,
    seeds the margin filter keeps, the largest centre difference between two orders among the kept seeds)."""
    if nd not in _ORDER_CACHE:
        fit, seeds, bw = normal_clusters(nd)
        res = {o: ref_iterate(fit, seeds, bw, 300, order=o) for o in ("forward", "backward", "pairwise")}
        m_member, m_stop = ref_margin(fit, seeds, bw, 300)
        keep = (m_member >= MEMBER_MARGIN) & (m_stop >= STOP_MARGIN)
        spread = 0.0
        for a in res.values():
            for b in res.values():
                spread = max(spread, float(np.abs(a[0][keep] - b[0][keep]).max()))
        _ORDER_CACHE[nd] = (res, keep, spread)
    return _ORDER_CACHE[nd]


@pytest.mark.parametrize("nd", [2, 3])
def test_iterate_real_valued_clusters(nd, device):
    """Counts and iterations equal the reference for the seeds whose decisions cannot flip with the summation order;
    centres within 16 x the spread of the reference's own three summation orders (the wavefront's tree is a fourth).
    Measured on the reference: spread 8.527e-14 in 2-D and 7.816e-14 in 3-D -> bounds 1.364e-12 and 1.251e-12 (centres
    are between 10 and 70: 6 to 12 ulp between two orders of a 300-term sum); the filter keeps all 129 seeds of both."""
    fit, seeds, bw = normal_clusters(nd)
    res, keep, spread = summation_orders(nd)
    want = res["forward"]
    bound = ORDER_FACTOR * spread
    assert spread > 0.0
    for grid in (False, True):
        c, n, it = run_iterate(fit, seeds, nd, bw, 300, device, grid)
        err = float(np.abs(c[keep] - want[0][keep]).max())
        print(f"nd {nd} grid {grid}: centre error {err:.3e}, bound {bound:.3e} (spread {spread:.3e}), kept {keep.sum()} of {len(keep)}")
        assert np.array_equal(n[keep], want[1][keep]) and np.array_equal(it[keep], want[2][keep])
        assert err <= bound


# ------------------------------------------------------------------------------------------------------------ bucket
def run_bucket(points, origin, cell, dims, device):
    _clx, lib = _lib()
    n, nd = points.shape
    ncells = int(np.prod(dims))
    nx, ny, nz = tuple(dims) + (1,) * (3 - nd)
    fit = _dev(points, device)
    out = Out((n, nd), np.float64, device)
    start = Out((ncells + 1,), np.int32, device)
    ws = Out((int(lib.clx_ms_bucket_workspace(n, ncells)),), np.uint8, device)
    _ok(lib.clx_ms_bucket(_clx.ptr(fit), n, nd, _cdoubles(origin), float(cell), nx, ny, nz, out.ptr, start.ptr, ws.ptr,
                          _clx.stream_ptr(device)))
    torch.cuda.synchronize(device)
    ws.get()
    return out.get(), start.get()


def check_bucket(points, origin, cell, dims, device, what=""):
    want = ref_bucket(points, origin, cell, dims)
    got = run_bucket(points, origin, cell, dims, device)
    assert np.array_equal(got[1], want[1]), f"{what}: cell offsets"
    assert_same_bits(got[0], want[0], f"{what}: sorted points")
    return want


def big_cell_case(nd, m, seed=0):
    """One cell of a 6^ND grid (edge 8) holding exactly m points among sparse ones, in shuffled order."""
    rng = np.random.default_rng(seed + m)
    dims = (6,) * nd
    heap = 16.0 + rng.integers(0, 32, size=(m, nd)) / 4.0                       # cell (2, 2[, 2])
    sparse = rng.integers(0, 192, size=(300, nd)) / 4.0
    sparse = sparse[~np.all(np.floor(sparse / 8.0) == 2, axis=1)]
    pts = np.concatenate([heap, sparse])[rng.permutation(m + len(sparse))]
    return pts, np.zeros(nd), 8.0, dims


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("m", [BUCKET_BIG - 1, BUCKET_BIG, BUCKET_BIG + 1])
def test_bucket_at_the_hand_over_to_thread_ranking(m, nd, device):
    pts, origin, cell, dims = big_cell_case(nd, m)
    _, start = check_bucket(pts, origin, cell, dims, device, what=f"{m} in one cell")
    assert np.diff(start).max() == m


def face_points(nd, cell, cells):
    """every lattice point origin + k * cell, k = 0 .. cells (the maximum of an extent of `cells` whole cells
    included), plus points a quarter to either side of every face"""
    origin = np.array([-49.0, 7.0, 3.0][:nd])
    ks = np.stack(np.meshgrid(*[np.arange(cells + 1.0)] * nd, indexing="ij"), -1).reshape(-1, nd)
    on = origin + ks * cell
    pts = np.concatenate([on, on + 0.25, on - 0.25, on])
    return pts[np.random.default_rng(int(cell)).permutation(len(pts))], origin


@pytest.mark.parametrize("nd", [2, 3])
def test_bucket_small_sets_faces_and_inexact_reciprocals(nd, device):
    rng = np.random.default_rng(nd)
    check_bucket(np.array([[3.0, 4.0, 5.0][:nd]]), np.zeros(nd), 8.0, (2,) * nd, device, what="n = 1")
    check_bucket(np.repeat(np.array([[9.0, 1.0, 17.0][:nd]]), 700, axis=0), np.zeros(nd), 8.0, (3,) * nd, device, what="identical")
    check_bucket(rng.integers(-40, 40, size=(500, nd)) / 4.0, np.full(nd, -10.0), 20.0, (1,) * nd, device, what="one cell")
    for cell in (3.0, 49.0, 8.0):
        cells = 20 if nd == 2 else 5
        pts, origin = face_points(nd, cell, cells)
        # k * cell / cell is exactly k: a point ON a face belongs to the cell above it, the maximum is clamped back
        want = check_bucket(pts, origin, cell, (cells,) * nd, device, what=f"faces, cell {cell}")
        assert np.diff(want[1]).min() >= 1


# ------------------------------------------------------------------------------------------------------------ assign
def points_as_image(points, dtype=np.float64):
    """A 1 x n (x 1 x n in 3-D) image whose compaction yields `points`: emb = points - coordinate (exact for the
    lattice values used here: checked), every pixel foreground."""
    n, nd = points.shape
    emb = np.ascontiguousarray(points.T).reshape((nd,) + (1,) * (nd - 1) + (n,)).astype(np.float64)
    emb[0] = emb[0] - np.arange(n, dtype=np.float64)
    emb = emb.astype(dtype)
    std = np.zeros((1,) * (nd - 1) + (n,), dtype)
    return emb, std


def run_assign_entries(emb, std, thr, centres, cell, device):
    """The four assignment entries on the foreground points of one image -> {entry: label map (npix,)}; the points the
    entries see are the ones clx_ms_prepare* made (checked against ref_prepare by the caller)."""
    from cellulus_amd.utils import mean_shift as MS

    _clx, lib = _lib()
    r = run_prepare(emb, std, thr, device)
    nd, nfg = r["nd"], r["nfg"]
    Z, Y, X = r["dims"]
    npix = Z * Y * X
    st = _clx.stream_ptr(device)
    K = len(centres)
    order, cstart, origin, (gx, gy, gz) = MS._center_grid(centres, cell)
    cc = _dev(centres, device)
    cs = _dev(centres[order], device)
    order_d, cstart_d = _dev(order, device), _dev(cstart, device)
    index = _dev(r["index"][:max(nfg, 1)], device)
    out = {}
    for name in ("assign", "grid", "cells", "dense"):
        labels = Out((npix,), np.int32, device)
        if name == "assign":
            _ok(lib.clx_ms_assign(r["pts_out"].ptr, _clx.ptr(index), nfg, _clx.ptr(cc), K, nd, labels.ptr, st))
        elif name == "grid":
            _ok(lib.clx_ms_assign_grid(r["pts_out"].ptr, _clx.ptr(index), nfg, _clx.ptr(cc), K, nd, _clx.ptr(order_d),
                                       _clx.ptr(cstart_d), _cdoubles(origin), float(cell), gx, gy, gz, labels.ptr, st))
        elif name == "cells":
            _ok(lib.clx_ms_assign_cells(r["pts_out"].ptr, _clx.ptr(index), nfg, _clx.ptr(cs), K, nd, _clx.ptr(order_d),
                                        _clx.ptr(cstart_d), _cdoubles(origin), float(cell), gx, gy, gz, labels.ptr, st))
        else:
            _ok(lib.clx_ms_assign_dense(r["pts_out"].ptr, _clx.ptr(cs), K, nd, _clx.ptr(order_d), _clx.ptr(cstart_d),
                                        _cdoubles(origin), float(cell), gx, gy, gz, r["ws_out"].ptr, 1 if r["f32"] else 0,
                                        Z, Y, X, labels.ptr, st))
        torch.cuda.synchronize(device)
        out[name] = labels.get()
    return r, out, (gx, gy, gz)


def check_assign(emb, std, thr, centres, cell, device, what=""):
    points, index, _ = ref_prepare(emb, std, thr)
    want_fg = ref_assign(points, centres)
    r, got, dims = run_assign_entries(emb, std, thr, centres, cell, device)
    assert r["nfg"] == len(index)
    assert_same_bits(r["points"][:len(index)], points, what + " points")
    for name, lab in got.items():
        # the three scattering entries write foreground pixels only (the prefill stays elsewhere), the dense one all
        want = np.full(std.size, 0 if name == "dense" else np.int32(-1414812757), np.int32)      # 0xABABABAB
        want[index] = want_fg
        bad = np.flatnonzero(lab != want)
        assert len(bad) == 0, (f"{what} clx_ms_assign{'' if name == 'assign' else '_' + name}: {len(bad)} labels differ, first at "
                               f"pixel {bad[0]}: {lab[bad[0]]} != {want[bad[0]]}")
    return points, want_fg, dims


def check_assign_points(points, centres, cell, device, what=""):
    emb, std = points_as_image(points)
    pts, _, _ = ref_prepare(emb, std, 0.5)
    assert_same_bits(pts, np.ascontiguousarray(points, dtype=np.float64), what + ": points - coordinate + coordinate is not exact")
    return check_assign(emb, std, 0.5, centres, cell, device, what)


def tie_case(nd, swap):
    """Integer centres 20 apart, shuffled; centres 6 and 7 moved to a place of their own, 6 apart in x (one cell at
    edge 9, two cells with one between at edge 3); points at their exact midpoint and on the quarter lattice around it."""
    rng = np.random.default_rng(60 + nd)
    centres = np.stack(np.meshgrid(*[20.0 * np.arange(4.0)] * nd, indexing="ij"), -1).reshape(-1, nd)
    centres = centres[rng.permutation(len(centres))]
    a = np.full(nd, 200.0)
    b = a.copy()
    b[0] += 6.0
    centres[6], centres[7] = (b, a) if swap else (a, b)
    mid = 0.5 * (a + b)
    ties = np.repeat(mid[None], 9, axis=0)
    ties[:, 1] += np.arange(-4, 5) * 0.25                 # still equidistant: the offset is perpendicular to the pair
    around = mid + rng.integers(-8, 9, size=(60, nd)) / 4.0
    return centres, np.concatenate([ties, around, centres + 0.25]), ties


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("cell", [9.0, 3.0])
@pytest.mark.parametrize("swap", [False, True])
def test_assign_exact_ties_go_to_the_smaller_id(swap, cell, nd, device):
    centres, points, ties = tie_case(nd, swap)
    d6 = ((ties - centres[6]) ** 2).sum(1)
    d7 = ((ties - centres[7]) ** 2).sum(1)
    others = np.delete(np.arange(len(centres)), [6, 7])
    assert np.array_equal(d6, d7) and (((ties[:, None] - centres[others][None]) ** 2).sum(-1) > d6[:, None]).all()
    pts, want, _ = check_assign_points(points, centres, cell, device, what=f"ties swap={swap} cell={cell}")
    assert (want[:len(ties)] == 7).all()                  # id 6, the smaller of the two, + 1


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("K", [1, 2, CHUNK - 1, CHUNK, CHUNK + 1])
def test_assign_centre_counts_around_the_lds_chunk(K, nd, device):
    """Integer centres and half-integer points: many exact ties, also between a centre of the first 1024 and one of
    the second staging chunk of ms_assign_kernel (the last centre mirrors the first about a point)."""
    rng = np.random.default_rng(K + nd)
    centres = rng.integers(0, 200, size=(K, nd)).astype(np.float64)
    points = rng.integers(0, 400, size=(3000, nd)) / 2.0
    if K > 1:
        centres[0] = 300.0
        centres[K - 1] = 300.0
        centres[K - 1, 0] = 310.0
        points[:5] = 300.0
        points[:5, 0] = 305.0
        points[:5, 1] += np.arange(5)
    _, want, _ = check_assign_points(points, centres, 10.0, device, what=f"K {K}")
    if K > 1:
        assert (want[:5] == 1).all()


@pytest.mark.parametrize("nd", [2, 3])
def test_assign_grid_edges(nd, device):
    rng = np.random.default_rng(90 + nd)
    # every centre in one cell
    centres = 50.0 + rng.integers(0, 30, size=(17, nd)) / 4.0
    points = 50.0 + rng.integers(-80, 120, size=(2000, nd)) / 4.0
    _, _, dims = check_assign_points(points, centres, 9.0, device, what="one cell")
    assert dims == (1, 1, 1)
    # sparse centres over a wide grid (most cells empty); points outside the grid on every side, whose border cell is
    # empty; points farther than `cell` from every centre (the ring search doubles until it covers the grid)
    centres = rng.integers(0, 40, size=(30, nd)) * 25.0
    centres = np.unique(centres, axis=0)[rng.permutation(len(np.unique(centres, axis=0)))]
    lo, hi = centres.min(axis=0), centres.max(axis=0)
    inside = lo + rng.integers(0, 4000, size=(3000, nd)) / 4.0 * (hi - lo) / 1000.0
    inside = np.round(inside * 4) / 4
    outside = []
    for ax in range(nd):
        for v in (lo[ax] - 30.25, lo[ax] - 400.0, hi[ax] + 30.25, hi[ax] + 400.0):
            p = lo + rng.integers(0, 1000, size=(40, nd)) / 1000.0 * (hi - lo)
            p = np.round(p * 4) / 4
            p[:, ax] = v
            outside.append(p)
    points = np.concatenate([inside] + outside)
    assert np.abs(points).max() < 2048
    pts, want, dims = check_assign_points(points, centres, 9.0, device, what="sparse grid")
    d2 = ((pts[:, None] - centres[None]) ** 2).sum(-1).min(1)
    assert (d2 > 4 * 81.0).sum() > 500 and np.prod(dims) > 20 * len(centres)
    # points exactly ON cell faces, the nearer centre in the cell beyond the face, cell edges with an inexact reciprocal
    for cell in (3.0, 49.0):
        origin = np.array([-49.0, 7.0, 3.0][:nd])
        ks = np.stack(np.meshgrid(*[np.arange(6.0)] * nd, indexing="ij"), -1).reshape(-1, nd)
        faces = origin + ks * cell                        # includes the origin: the grid's minimum corner
        centres = np.concatenate([faces + 0.25 * cell, faces[(ks >= 1).all(axis=1)][::3] - 0.5])      # just above a face ... and just below
        centres = np.concatenate([origin[None], centres])                          # (keeps the grid's origin at `origin`)
        points = np.concatenate([faces, faces + 0.25, faces - 0.25])
        check_assign_points(points, centres, cell, device, what=f"faces cell {cell}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(61, 67), (5, 301), (9, 20, 31)], ids=lambda s: "x".join(map(str, s)))
def test_assign_on_images(shape, dtype, device):
    """Real-valued embeddings on images with ragged tiles: the four entries against the first minimum over all centres."""
    nd = len(shape)
    rng = np.random.default_rng(sum(shape))
    emb = rng.normal(0.0, 3.0, size=(nd,) + shape).astype(dtype)
    std = rng.uniform(0, 1, size=shape).astype(dtype)
    centres = np.stack([rng.uniform(0, s, size=60) for s in shape[::-1]], axis=1)
    check_assign(emb, std, 0.5, centres, 4.0, device, what=f"{shape}")


# ---------------------------------------------------------------------------------------------------------- pipeline
PIPELINE_SEED_STRIDE = 17        # (every 16th foreground point would sit in two of the four block columns only)


def pipeline_case(nfit):
    """A 64 x 64 image of 16 blocks, integer embeddings that put every pixel within 1 of its block's centre, and a
    lattice foreground (every other pixel, less one for 2047) of exactly `nfit` points; every 17th point a seed."""
    rng = np.random.default_rng(nfit)
    yy, xx = np.indices((64, 64))
    cy, cx = (yy // 16) * 16 + 8, (xx // 16) * 16 + 8
    emb = np.stack([cx - xx + rng.integers(-1, 2, size=(64, 64)), cy - yy + rng.integers(-1, 2, size=(64, 64))]).astype(np.float64)
    std = np.where((yy * 64 + xx) % 2 == 0, 0.25, 1.0)
    if nfit == 2047:
        std[37, 20] = 1.0
    assert int((std < 0.5).sum()) == nfit
    return emb, std, 4.0


@pytest.mark.parametrize("nfit", [2047, 2048])
def test_pipeline_on_both_sides_of_the_grid_switch(nfit, device):
    from cellulus_amd.utils import mean_shift as MS

    assert MS.GRID_MIN_POINTS == 2048
    emb, std, bw = pipeline_case(nfit)
    points, index, after = ref_prepare(emb, std, 0.5)
    seeds = points[::PIPELINE_SEED_STRIDE].copy()
    c, n, _ = ref_iterate(points, seeds, bw, MS.MAX_ITER)
    centres = MS._dedup_centers_numpy(c, n, bw)
    want = np.zeros(std.size, np.int32)
    want[index] = ref_assign(points, centres)
    emb_d = torch.from_numpy(emb).to(device)
    labels, got_centres = MS.mean_shift_on_device(emb_d, torch.from_numpy(std).to(device), bw, 1.0, 0.5, seeds)
    assert_same_bits(got_centres, centres, "cluster centres")
    assert np.array_equal(labels.cpu().numpy().reshape(-1), want)
    assert_same_bits(emb_d.cpu().numpy(), after, "coordinate-added embedding")
    assert len(centres) == 16 and want.max() == 16


# ---------------------------------------------------------------------------------------------------------- refusals
def test_rejected_arguments_launch_nothing(device):
    """The nine clx_ms_* entry points that launch kernels: every refused call returns CLX_ERR_ARG, names its entry in
    clx_last_error() and leaves every output and workspace as it was."""
    _clx, lib = _lib()
    st = _clx.stream_ptr(device)
    null = None
    ins = {k: torch.zeros(4096, dtype=torch.float64, device=device) for k in ("emb", "std", "fit", "seeds", "pts", "centers")}
    ints = {k: torch.zeros(4096, dtype=torch.int32, device=device) for k in ("index", "order", "cell_start")}
    outs = {k: Out((4096,), np.float64, device) for k in ("Xout", "iout", "nfg", "ws", "centers_out", "counts", "iters", "labels",
                                                          "sorted", "start")}
    origin = _cdoubles([0.0, 0.0, 0.0])
    P = {k: _clx.ptr(v) for k, v in {**ins, **ints}.items()}
    P.update({k: o.ptr for k, o in outs.items()})
    P["origin"] = origin
    odd = lambda k: ctypes.c_void_p(P[k].value + 8)

    def prepare(fn):
        def call(ND=2, Z=1, Y=8, X=8, **p):
            q = {**P, **p}
            return fn(q["emb"], q["std"], 0.5, ND, Z, Y, X, q["Xout"], q["iout"], q["nfg"], q["ws"], st)
        return call

    def iterate(nfit=8, nseeds=4, ND=2, bw=2.0, max_iter=3, **p):
        q = {**P, **p}
        return lib.clx_ms_iterate(q["fit"], nfit, q["seeds"], nseeds, ND, bw, max_iter, q["centers_out"], q["counts"], q["iters"], st)

    def iterate_grid(nfit=8, nseeds=4, ND=2, bw=2.0, cell=2.5, nx=1, ny=1, nz=1, max_iter=3, **p):
        q = {**P, **p}
        return lib.clx_ms_iterate_grid(q["fit"], nfit, q["cell_start"], q["origin"], cell, nx, ny, nz, q["seeds"], nseeds, ND, bw,
                                       max_iter, q["centers_out"], q["counts"], q["iters"], st)

    def assign(nfg=8, K=1, ND=2, **p):
        q = {**P, **p}
        return lib.clx_ms_assign(q["pts"], q["index"], nfg, q["centers"], K, ND, q["labels"], st)

    def gridded(fn):
        def call(nfg=8, K=1, ND=2, cell=2.0, nx=1, ny=1, nz=1, **p):
            q = {**P, **p}
            return fn(q["pts"], q["index"], nfg, q["centers"], K, ND, q["order"], q["cell_start"], q["origin"], cell, nx, ny, nz,
                      q["labels"], st)
        return call

    def dense(K=1, ND=2, cell=2.0, nx=1, ny=1, nz=1, Z=1, Y=8, X=8, **p):
        q = {**P, **p}
        return lib.clx_ms_assign_dense(q["pts"], q["centers"], K, ND, q["order"], q["cell_start"], q["origin"], cell, nx, ny, nz,
                                       q["ws"], 0, Z, Y, X, q["labels"], st)

    def bucket(n=8, ND=2, cell=2.0, nx=1, ny=1, nz=1, **p):
        q = {**P, **p}
        return lib.clx_ms_bucket(q["fit"], n, ND, q["origin"], cell, nx, ny, nz, q["sorted"], q["start"], q["ws"], st)

    nd_bad = [dict(ND=1), dict(ND=4)]
    grid_bad = [dict(nx=0), dict(ny=-1), dict(nz=0), dict(nz=2), dict(ND=3, nz=-1), dict(cell=0.0), dict(cell=-1.0)]
    image_bad = [dict(Z=2), dict(Y=0), dict(X=-8), dict(ND=3, Z=0), dict(Y=65536, X=32768), dict(ND=3, Z=2, Y=32768, X=32768)]
    nulls = lambda *ks: [{k: null} for k in ks]
    table = {
        "clx_ms_prepare": (prepare(lib.clx_ms_prepare), nd_bad + image_bad + [dict(ws=odd("ws"))] + nulls("emb", "std", "Xout", "nfg", "ws")),
        "clx_ms_prepare_f32": (prepare(lib.clx_ms_prepare_f32),
                               nd_bad + image_bad + [dict(ws=odd("ws"))] + nulls("emb", "std", "Xout", "nfg", "ws")),
        "clx_ms_iterate": (iterate, nd_bad + [dict(nfit=-1), dict(nseeds=-1), dict(max_iter=-1), dict(bw=0.0), dict(bw=-2.0)]
                           + nulls("fit", "seeds", "centers_out", "counts", "iters")),
        "clx_ms_iterate_grid": (iterate_grid, nd_bad + [dict(nfit=-1), dict(nseeds=-1), dict(max_iter=-1), dict(bw=0.0), dict(bw=-2.0),
                                                        dict(cell=1.5), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nz=2), dict(ND=3, nz=-1)]
                                + nulls("fit", "cell_start", "origin", "seeds", "centers_out", "counts", "iters")),
        "clx_ms_assign": (assign, nd_bad + [dict(nfg=-1), dict(K=0), dict(K=-1)] + nulls("pts", "index", "centers", "labels")),
        "clx_ms_assign_grid": (gridded(lib.clx_ms_assign_grid), nd_bad + grid_bad + [dict(nfg=-1), dict(K=0)]
                               + nulls("pts", "index", "centers", "labels", "order", "cell_start", "origin")),
        "clx_ms_assign_cells": (gridded(lib.clx_ms_assign_cells), nd_bad + grid_bad + [dict(nfg=-1), dict(K=0), dict(pts=odd("pts")),
                                                                                     dict(centers=odd("centers"))]
                                + nulls("pts", "index", "centers", "labels", "order", "cell_start", "origin")),
        "clx_ms_assign_dense": (dense, nd_bad + grid_bad + image_bad + [dict(K=0), dict(ws=odd("ws")), dict(centers=odd("centers"))]
                                + nulls("pts", "centers", "labels", "order", "cell_start", "origin", "ws")),
        "clx_ms_bucket": (bucket, nd_bad + grid_bad + [dict(n=-1), dict(nx=32768, ny=32768)]
                          + nulls("fit", "origin", "sorted", "start", "ws")),
    }
    for name, (call, refused) in table.items():
        for kw in refused:
            assert call(**kw) == -1, f"{name} accepted {kw}"
            assert lib.clx_last_error().decode().startswith(name + ":"), f"{name} {kw}: {lib.clx_last_error().decode()!r}"
    torch.cuda.synchronize(device)
    for k, o in outs.items():
        assert o.untouched(), f"{k} was written by a refused call"
    for name, (call, _) in table.items():                  # the same buffers are accepted with valid arguments
        assert call() == 0, f"{name}: {lib.clx_last_error().decode()}"
    torch.cuda.synchronize(device)
