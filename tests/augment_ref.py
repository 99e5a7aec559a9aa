"""Plain float64 NumPy / SciPy restatement of clx_elastic_crop (csrc/augment.hip) — the reference side of
test_cpu_augment_ref.py and test_gpu_augment_abi.py.  Nothing here imports the product.

It takes what the C entry takes: the data set (S, C, *spatial) in its stored type, the normalisation factor, the crop,
the control-point extents, the per-axis (crop_d x cp_d) float64 up-sampling matrices and one float64 record per crop:
    elastic  [s, A row-major (nd*nd), u (nd), field_0 ... field_{nd-1} (each prod(cp), row-major)]
    plain    [s, offset_0 ... offset_{nd-1}]
and does what ZarrDataset._elastic_crop does with those numbers:
    rel_d  = sum_e A[d][e] (idx_e - (crop_e - 1) / 2) + (M_0 x ... x M_{nd-1}) field_d           (float64, einsum)
    room_d = spatial_d - 1 - (max rel_d - min rel_d);   constant if every room_d >= 0, else reflect
    origin_d = u_d max(room_d, 0) - min rel_d
    out = map_coordinates(float64(float32(data[s]) * float32(factor)), rel + origin, order=1, mode, cval=0)   (float64)

Also here, because the CPU test (conditions on the inputs) and the GPU test (the kernels) must speak of the same cases:
the case table `CASES` with `build_case`, and `plan`, the launch arithmetic of the entry point restated."""

import functools
import math

import numpy as np

AUG_THREADS = 256
AUG_VPT = 4
AUG_MAX_P1 = 64
AUG_MAX_BLOCKS = 2048
AUG_MAX_LDS = 60000
AUG_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}      # enum clx_aug_dtype


# ------------------------------------------------------------------------------------------------- launch arithmetic
def plan(crop, C, B, elastic):
    """items, p1 and tiles as clx_elastic_crop forms them, and what follows from them: `want` blocks per crop would give
    every thread one item, `cap` is what the grid limit leaves, `trips` is the longest grid-stride loop of a thread and
    `short_trips` says that some threads take fewer trips than others."""
    crop = tuple(int(c) for c in crop)
    xq = (crop[-1] + AUG_VPT - 1) // AUG_VPT
    rows = int(np.prod(crop[:-1], dtype=np.int64))
    items = rows * xq
    p1 = min(max((items + 2 * AUG_THREADS - 1) // (2 * AUG_THREADS), 1), AUG_MAX_P1)
    work = items if elastic else items * C
    cap = max(AUG_MAX_BLOCKS // B, 1)
    want = (work + AUG_THREADS - 1) // AUG_THREADS
    tiles = min(want, cap)
    per_trip = tiles * AUG_THREADS
    return dict(xq=xq, rows=rows, items=items, p1=p1, work=work, cap=cap, want=want, tiles=tiles,
                trips=(work + per_trip - 1) // per_trip, short_trips=work % per_trip != 0, vector_stores=crop[-1] % 4 == 0)


def item_of(crop, index):
    """The thread item that holds voxel `index` of a crop: rows of ceil(W / 4) items, 4 consecutive x each."""
    xq = (crop[-1] + AUG_VPT - 1) // AUG_VPT
    row = 0
    for c, i in zip(crop[:-1], index[:-1]):
        row = row * c + i
    return row * xq + index[-1] // AUG_VPT


def tile_of(pl, crop, index, channel=0, elastic=True):
    """The block (within its crop) that handles voxel `index` of `channel` under the plan `pl` (the channel counts only
    in the plain kernel, whose work runs over channels x items)."""
    it =item_of(crop, index) + (0 if elastic else channel * pl["items"])
    return (it // AUG_THREADS) % pl["tiles"]


def lds_bytes(crop, cp_shape):
    """Dynamic LDS of the elastic kernels: all matrices + one record without its sample index, in doubles."""
    nd = len(crop)
    nmat = sum(c * p for c, p in zip(crop, cp_shape))
    return (nmat + nd * nd + nd + nd * int(np.prod(cp_shape))) * 8


# ------------------------------------------------------------------------------------------------------ the inputs
def cp_shape_for(crop, spacing):
    return tuple(max(2, int(math.ceil(c / spacing)) + 1) for c in crop)


def make_mats(crop, cp_shape):
    """Cubic-spline up-sampling along one axis is linear: scipy's zoom on unit vectors gives its matrix (the expression
    of ZarrDataset._elastic_ops, restated).  One control point: the constant field, a column of ones."""
    from scipy.ndimage import zoom

    mats = []
    for c, p in zip(crop, cp_shape):
        if p == 1:
            mats.append(np.ones((c, 1)))
        else:
            mats.append(np.ascontiguousarray(zoom(np.eye(p), [c / p, 1.0], order=3, mode="nearest", grid_mode=False)[:c],
                                             dtype=np.float64))
        assert mats[-1].shape == (c, p), (mats[-1].shape, c, p)
    return mats


def rotation(nd, angle, scale=1.0):
    rot = np.eye(nd)
    c_, s_ = math.cos(angle), math.sin(angle)
    rot[-2:, -2:] = [[c_, -s_], [s_, c_]]              # in the (y, x) plane
    return rot * scale


def make_record(cp_shape, s, rng, angle=None, scale=1.0, A=None, sigma=0.0, u=None):
    """One elastic record.  A: an (nd, nd) matrix, or None for the rotation by `angle` (None: uniform in [0, pi/2]) times
    `scale` (a number, or a (low, high) pair to draw from); sigma: jitter of the control points, a number or one per
    displacement axis; u: the nd placement numbers (None: uniform in [0, 1))."""
    nd = len(cp_shape)
    if A is None:
        if angle is None:
            angle = rng.uniform(0.0, math.pi / 2)
        if isinstance(scale, tuple):
            scale = rng.uniform(*scale)
        A = rotation(nd, angle, scale)
    A = np.asarray(A, dtype=np.float64).reshape(nd, nd)
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (nd,))
    fields = [rng.normal(0.0, sig[d], size=cp_shape) if sig[d] > 0 else np.zeros(cp_shape) for d in range(nd)]
    u = rng.random(nd) if u is None else np.broadcast_to(np.asarray(u, dtype=np.float64), (nd,))
    return np.concatenate([[float(s)], A.ravel(), u, *[f.ravel() for f in fields]])


def plain_record(s, offsets):
    return np.asarray([float(s), *[float(o) for o in offsets]])


# --------------------------------------------------------------------------------------------------- the reference
def geometry(spatial, crop, cp_shape, mats, rec):
    """Everything of one elastic crop that does not touch image data -> dict(rel, lo, hi, room, mode, origin, coords)."""
    nd = len(crop)
    rec = np.asarray(rec, dtype=np.float64)
    A = rec[1:1 + nd * nd].reshape(nd, nd)
    u = rec[1 + nd * nd:1 + nd * nd + nd]
    fields = rec[1 + nd * nd + nd:].reshape((nd,) + tuple(cp_shape))
    axes = [np.arange(c, dtype=np.float64) - (np.float64(c) - 1.0) / 2.0 for c in crop]
    rel0 = np.stack(np.meshgrid(*axes, indexing="ij"))
    rel = np.tensordot(A, rel0, axes=1)
    spec = "yi,xj,ij->yx" if nd == 2 else "zi,yj,xk,ijk->zyx"
    for d in range(nd):
        rel[d] = rel[d] + np.einsum(spec, *mats, fields[d])
    lo, hi = rel.reshape(nd, -1).min(axis=1), rel.reshape(nd, -1).max(axis=1)
    room = np.asarray(spatial, dtype=np.float64) - 1.0 - (hi - lo)
    mode = "constant" if np.all(room >= 0) else "reflect"
    origin = u * np.maximum(room, 0.0) - lo
    coords = rel + origin.reshape((nd,) + (1,) * nd)
    return dict(rel=rel, lo=lo, hi=hi, room=room, mode=mode, origin=origin, coords=coords)


def normalised(data, factor):
    """The source as the kernels see it: normalised in float32, widened to float64."""
    return (np.asarray(data).astype(np.float32) * np.float32(factor)).astype(np.float64)


def ref_crops(data, factor, crop, cp_shape, mats, records, elastic):
    """-> one (ref64 (C, *crop), mode, room, bound (C, *crop)) per record.  Plain crops: mode "plain", room =
    spatial - crop, bound 0 (the result is exact).  Elastic:
        bound = 2^-24 |ref64| + nd * 2 Vmax * 2 T 2^-52 R
    — one rounding to float32, plus float64 sums of T = prod(cp) + nd + 2 terms of magnitude up to R (the largest of
    |rel|, |origin| and the source extents) taken in another order, through an interpolant of slope <= 2 Vmax per axis.
    Equal records are computed once."""
    from scipy.ndimage import map_coordinates

    data = np.asarray(data)
    spatial, nd = data.shape[2:], len(crop)
    records = np.asarray(records, dtype=np.float64)
    vmax = float(np.abs(normalised(data, factor)).max())
    geo, done, out = {}, {}, []
    for rec in records:
        key = rec.tobytes()
        if key not in done:
            s = int(rec[0])
            assert 0 <= s < data.shape[0]
            src = normalised(data[s], factor)
            if not elastic:
                off = [int(o) for o in rec[1:1 + nd]]
                assert all(0 <= o <= n - c for o, n, c in zip(off, spatial, crop))
                ref = src[(slice(None),) + tuple(slice(o, o + c) for o, c in zip(off, crop))].copy()
                done[key] = (ref, "plain", np.asarray(spatial, dtype=np.float64) - np.asarray(crop), np.zeros_like(ref))
            else:
                g = geo.get(rec[1:].tobytes())
                if g is None:
                    g = geo[rec[1:].tobytes()] = geometry(spatial, crop, cp_shape, mats, rec)
                ref = np.stack([map_coordinates(ch, g["coords"], order=1, mode=g["mode"], cval=0.0) for ch in src])
                T = int(np.prod(cp_shape)) + nd + 2
                R = max(float(np.abs(g["rel"]).max()), float(np.abs(g["origin"]).max()), float(max(spatial)))
                slack = nd * 2.0 * vmax * 2.0 * T * 2.0 ** -52 * R
                done[key] = (ref, g["mode"], g["room"], 2.0 ** -24 * np.abs(ref) + slack)
        out.append(done[key])
    return out


# ------------------------------------------------------------------------------------------------------- the cases
def random_data(shape, dtype, seed=1, signed=False):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        v = rng.random(shape).astype(dtype)
        return v - dtype.type(0.25) if signed else v
    return (rng.random(shape) * np.iinfo(dtype).max).astype(dtype)


def _c(name, family, dtype, S, C, spatial, crop, B, cp=None, spacing=32, elastic=True, factor=None, shift=0, seed=0,
       draws=None, signed=False, rec=None, expect=None):
    return dict(name=name, family=family, dtype=np.dtype(dtype), S=S, C=C, spatial=tuple(spatial), crop=tuple(crop), B=B,
                cp=cp, spacing=spacing, elastic=elastic, factor=factor, shift=shift, seed=seed, draws=draws, signed=signed,
                rec=rec or {}, expect=expect or {})


RANDOM = dict(scale=(0.9, 1.1), sigma=2.0)           # angle uniform in [0, pi/2]

# expect: entries of plan() that must hold as given, and
#   want_gt_tiles / trips / short_trips / cap   the grid cap is reached, threads take `trips` trips, some one fewer
#   room = per axis "+", "-" or "0": the sign of room in EVERY record;  mode: the mode of every record
#   wrap = True: every record has a coordinate >= 2 n on some axis (reflect over more than one period)
#   lds_at_least = bytes the kernels stage
CASES = [
    # b. random parameters ------------------------------------------------------------------------------------------
    _c("w67-2d-u8", "odd-width", np.uint8, 2, 1, (60, 90), (37, 67), 4, shift=4, expect=dict(vector_stores=False)),
    _c("w50-3d-u16", "odd-width", np.uint16, 2, 1, (12, 20, 70), (6, 11, 50), 3, shift=4, expect=dict(vector_stores=False)),
    _c("w1-2d-f32", "odd-width", np.float32, 2, 1, (20, 6), (13, 1), 3, shift=4, signed=True, expect=dict(vector_stores=False)),
    _c("w3-3d-u8", "odd-width", np.uint8, 2, 2, (9, 12, 8), (5, 7, 3), 3, shift=4, expect=dict(vector_stores=False)),
    _c("cp36-2d", "control-points", np.uint8, 2, 1, (50, 100), (24, 70), 3, spacing=16, shift=4, expect=dict(cp=(3, 6))),
    _c("cp345-3d", "control-points", np.uint8, 2, 1, (30, 48, 64), (20, 36, 50), 2, spacing=16, shift=4,
       expect=dict(cp=(3, 4, 5))),
    _c("cp1-2d", "control-points", np.uint16, 2, 1, (40, 60), (24, 40), 3, cp=(1, 4), expect=dict(cp=(1, 4))),
    _c("cp1-3d", "control-points", np.uint8, 1, 1, (20, 24, 30), (8, 12, 16), 2, cp=(3, 1, 2), expect=dict(cp=(3, 1, 2))),
    _c("mixed-2d", "mixed-room", np.uint8, 2, 1, (30, 200), (40, 44), 4, expect=dict(mode="reflect", room="-+")),
    _c("mixed-3d", "mixed-room", np.uint16, 2, 1, (8, 100, 100), (12, 16, 24), 3, expect=dict(mode="reflect", room="-++")),
    _c("wrap-2d", "reflect-wrap", np.uint8, 2, 1, (12, 15), (40, 44), 4, expect=dict(mode="reflect", room="--", wrap=True)),
    _c("wrap-3d", "reflect-wrap", np.float32, 2, 1, (5, 7, 6), (12, 20, 22), 3, signed=True,
       expect=dict(mode="reflect", room="---", wrap=True)),
    _c("wrap-scale3", "reflect-wrap", np.uint16, 2, 1, (40, 50), (40, 44), 3, rec=dict(scale=3.0, sigma=2.0),
       expect=dict(mode="reflect", room="--", wrap=True)),
    _c("u16-3d-s3c2", "types", np.uint16, 3, 2, (14, 20, 24), (8, 12, 16), 6),
    _c("f32-2d-neg", "types", np.float32, 2, 1, (50, 71), (24, 36), 4, factor=0.37, signed=True),
    _c("u8-2d-c3", "types", np.uint8, 2, 3, (40, 52), (20, 28), 4),
    _c("lds-56000", "lds", np.uint8, 1, 1, (420, 420), (256, 256), 1, spacing=22,
       expect=dict(cp=(13, 13), lds_at_least=56000, mode="constant")),
    # c. grid caps --------------------------------------------------------------------------------------------------
    _c("cap-2d", "grid-cap", np.uint8, 3, 1, (100, 180), (70, 150), 256, spacing=64, shift=4, draws=16,
       expect=dict(items=2660, want=11, tiles=8, trips=2, short_trips=True)),
    _c("cap-3d", "grid-cap", np.uint8, 3, 1, (16, 20, 64), (10, 14, 50), 300, spacing=64, shift=4, draws=16,
       expect=dict(items=1820, want=8, tiles=6, trips=2, short_trips=True)),
    _c("cap-plain", "grid-cap", np.uint16, 3, 2, (100, 180), (70, 150), 256, elastic=False, shift=4,
       expect=dict(items=2660, work=5320, want=21, tiles=8, trips=3, short_trips=True)),
    _c("cap1-elastic", "grid-cap", np.uint8, 3, 1, (12, 16), (5, 9), 2050, spacing=64, shift=4, draws=16,
       expect=dict(cap=1, tiles=1)),
    _c("cap1-plain", "grid-cap", np.float32, 3, 2, (12, 16), (5, 9), 2050, elastic=False, shift=4, signed=True,
       expect=dict(cap=1, tiles=1, trips=1)),
]
CASE_NAMES = [c["name"] for c in CASES]
RANDOMISED = [c["name"] for c in CASES if c["elastic"]]


def default_factor(dtype):
    dtype = np.dtype(dtype)
    return 1.0 if dtype.kind == "f" else 1.0 / np.iinfo(dtype).max


@functools.lru_cache(maxsize=None)
def build_case(name):
    """-> dict(case fields..., data, factor, cp_shape, mats, records): all inputs of the C entry, from the case's seed."""
    c = dict(next(k for k in CASES if k["name"] == name))
    nd = len(c["crop"])
    rng = np.random.default_rng(1000 + c["seed"])
    c["data"] = random_data((c["S"], c["C"]) + c["spatial"], c["dtype"], seed=7 + c["seed"], signed=c["signed"])
    c["factor"] = float(np.float32(default_factor(c["dtype"]) if c["factor"] is None else c["factor"]))
    B = c["B"]
    if c["elastic"]:
        c["cp_shape"] = tuple(c["cp"]) if c["cp"] else cp_shape_for(c["crop"], c["spacing"])
        c["mats"] = make_mats(c["crop"], c["cp_shape"])
        kw = dict(RANDOM, **c["rec"])
        draws = [make_record(c["cp_shape"], 0, rng, **kw) for _ in range(min(B, c["draws"] or B))]
        rows = []
        for b in range(B):                       # the draws tiled over the batch, the sample index running on its own
            r = draws[b % len(draws)].copy()
            r[0] = (b + b // len(draws)) % c["S"]
            rows.append(r)
    else:
        c["cp_shape"], c["mats"] = None, None
        rows = [plain_record(b % c["S"], [rng.integers(0, n - k + 1) for n, k in zip(c["spatial"], c["crop"])])
                for b in range(B)]
        for d in range(nd):                      # both ends of every axis are among the offsets
            rows[d][1 + d] = 0.0
            rows[nd + d][1 + d] = float(c["spatial"][d] - c["crop"][d])
    c["records"] = np.ascontiguousarray(np.stack(rows), dtype=np.float64)
    return c


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The reference of a whole case, computed once per process and shared (read-only) by the tests."""
    c = build_case(name)
    out = ref_crops(c["data"], c["factor"], c["crop"], c["cp_shape"], c["mats"], c["records"], c["elastic"])
    for ref, _mode, _room, bound in out:
        ref.setflags(write=False)
        bound.setflags(write=False)
    return out
