"""Host arithmetic of the measure stage: the columns of ``region_table`` from the exact integers the kernels give (the
``*_columns`` and ``*_table`` functions), the rank and threshold arithmetic that goes into a call (``intensity_shift``,
``quantile_ranks``, ``coloc_thresholds``) and the checks on the table's options that need no device.  Nothing here touches a
device or imports torch; ``measure.py`` has the device half, its docstring the definitions of the columns, and it re-exports
this module's names."""

import math
import numbers
from fractions import Fraction

import numpy as np

DIST_INF = 1 << 30                      # CLX_DIST_INF: a pixel of clx_label_distance_sq's map that has no candidate
MAX_QUANTILES = 16                      # two ranks each: clx_region_order_stats takes nq <= 32
MIN_LEVELS, MAX_LEVELS = 2, 32          # clx_region_cooccurrence: thirteen 32 x 32 int32 matrices are 52 KiB of LDS
MAX_TEXTURE_DISTANCE = 64
TEXTURE_FEATURES = ("asm", "contrast", "correlation", "variance", "idm", "sum_average", "sum_variance", "sum_entropy", "entropy",
                    "difference_variance", "difference_entropy", "info_correlation_1", "info_correlation_2")
_TEXTURE_INT64_MAX_T = 1 << 25          # texture_columns: numerators are below 2^12 T^2, so int64 holds them up to here
_TEXTURE_SLICE_CELLS = 1 << 22          # matrix cells texture_columns holds as float64 at a time
MAX_RINGS, MAX_RADIAL_WIDTH, RADIAL_WEDGES = 32, 32768, 8      # clx_region_radial: rings <= 32, width <= 2^15, 1 or 8 wedges
_SQRT2 = math.sqrt(2.0)
PERIMETER_WEIGHTS = (0.0, 1.0, _SQRT2, (1.0 + _SQRT2) / 2.0)   # of clx_region_perimeter's classes; [0] counts border pixels
_SHIFT_MIN, _SHIFT_MAX = -1022, 1023    # 2.0 ** shift stays a normal float64: scaling by it is exact
# Weights of the 13 line directions of the 26-neighbourhood in the Crofton surface estimate (``topology_columns``): the
# 26 unit vectors towards a voxel's neighbours cut the sphere into their Voronoi cells (a point belongs to the direction
# it is nearest to); a weight is the area of a direction's cell over 4 pi, the two antipodes of a line pooled, so that
# 3 w1 + 6 w2 + 4 w3 = 1 for the 3 axial, 6 face-diagonal and 4 space-diagonal lines.  The cells are spherical polygons
# (an octagon, a rectangle, a hexagon) whose corners are the points at equal distance from three neighbouring directions,
# the permutations of (0.28174743, 0.36718039, 0.88645189) with signs; their areas follow from the spherical excess.
# Computed that way in float64; tests/test_cpu_topology.py recomputes them with scipy.spatial.SphericalVoronoi.
SURFACE_WEIGHTS = (0.09155578240952184, 0.07396125575215028, 0.07039127956463334)
_SQRT3 = math.sqrt(3.0)


def intensity_shift(max_abs, npix):
    """Binary scale for ``clx_region_intensity``: with ``q = rint(v * 2**shift)``, every ``|v| <= max_abs`` gives
    ``|q| <= 2**(62 - L)``, ``L = npix.bit_length()``, so that a sum over up to ``npix`` pixels stays below ``2**62``.
    ``shift = 62 - L - E`` with ``E`` the smallest integer such that ``max_abs <= 2**E`` (the ``frexp`` exponent, one
    less for an exact power of two, whose ``q`` lands on the bound itself); the largest shift the kernel's per-pixel
    bound admits.  0 for ``max_abs == 0``; clamped to [-1022, 1023] so that ``ldexp`` stays finite and exact."""
    max_abs = float(max_abs)
    if not (max_abs >= 0.0 and math.isfinite(max_abs)):
        raise ValueError(f"intensity_shift: max_abs must be finite and >= 0, got {max_abs}")
    if int(npix) < 1:
        raise ValueError(f"intensity_shift: npix must be >= 1, got {npix}")
    if max_abs == 0.0:
        return 0
    mant, exp = math.frexp(max_abs)
    if mant == 0.5:
        exp -= 1
    return max(_SHIFT_MIN, min(_SHIFT_MAX, 62 - int(npix).bit_length() - exp))


_AXES = ("z", "y", "x")
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))        # order of sum2: zz yy xx zy zx yx


def _exact_div(num, den):
    """Element-wise ``num / den`` of Python-int object arrays as float64: one correctly rounded division each."""
    return np.array([n / d for n, d in zip(num, den)], dtype=np.float64)


def shape_columns(label, area, bbox, sum1, sum2, nd):
    """The geometric columns of ``region_table`` from integer moments.  label (n), area (n), bbox (n, 6) inclusive
    ``zmin ymin xmin zmax ymax xmax``, sum1 (n, 3) ``Σz Σy Σx``, sum2 (n, 6) ``Σzz Σyy Σxx Σzy Σzx Σyx``; nd 2 or 3
    (2-D: the z entries are ignored).  Covariance numerators ``area·Σab − Σa·Σb`` are exact Python integers."""
    assert nd in (2, 3)
    label = np.asarray(label)
    n = len(label)
    area_o = np.asarray(area).astype(object).reshape(n)
    bbox = np.asarray(bbox).reshape(n, 6)
    s1 = np.asarray(sum1).astype(object).reshape(n, 3)
    s2 = np.asarray(sum2).astype(object).reshape(n, 6)
    axes = range(3 - nd, 3)
    cols = {"label": label.astype(np.int64), "area": np.asarray(area).astype(np.int64).reshape(n)}
    for a in axes:
        cols[f"bbox_min_{_AXES[a]}"] = bbox[:, a].astype(np.int64)
    for a in axes:
        cols[f"bbox_max_{_AXES[a]}"] = bbox[:, 3 + a].astype(np.int64) + 1          # exclusive, as in skimage
    for a in axes:
        cols[f"centroid_{_AXES[a]}"] = _exact_div(s1[:, a], area_o)
    cov = np.zeros((n, 3, 3), dtype=np.float64)
    area_sq = area_o * area_o
    for k, (a, b) in enumerate(_PAIRS):
        if a < 3 - nd:
            continue
        c = _exact_div(area_o * s2[:, k] - s1[:, a] * s1[:, b], area_sq)
        cov[:, a, b] = cov[:, b, a] = c
        cols[f"cov_{_AXES[a]}{_AXES[b]}"] = c
    eig = np.linalg.eigvalsh(cov[:, 3 - nd:, 3 - nd:])[:, ::-1] if n else np.zeros((0, nd))
    for i in range(nd):
        cols[f"cov_eig_{i}"] = np.ascontiguousarray(eig[:, i])
    a = cols["area"].astype(np.float64)
    cols["equivalent_diameter"] = np.sqrt(4.0 * a / np.pi) if nd == 2 else np.cbrt(6.0 * a / np.pi)
    return cols


def perimeter_from_classes(classes):
    """``c1 + c2·√2 + c3·(1 + √2)/2`` per row of ``classes`` (n, 4) as float64: scikit-image's ``perimeter(mask,
    neighbourhood=4)`` from ``clx_region_perimeter``'s integer counts (column 0, the border pixels, has no weight)."""
    c = np.asarray(classes).reshape(-1, 4).astype(np.float64)
    return c[:, 1] * PERIMETER_WEIGHTS[1] + c[:, 2] * PERIMETER_WEIGHTS[2] + c[:, 3] * PERIMETER_WEIGHTS[3]


def boundary_columns(present, bbox, shape, a, b, faces, classes, nd):
    """The boundary columns of ``region_table`` from integer counts.  present (n) ids ascending, bbox (n, 6) inclusive
    ``zmin ymin xmin zmax ymax xmax``, shape the map's ``nd`` extents; a, b, faces: ``contact_pairs``' rows (a < b, a may
    be 0; every non-zero id is in ``present``); classes (n, 4) ``clx_region_perimeter``'s rows of the present ids, or
    None (3-D).  ``touches_border`` is host arithmetic on the bounding box."""
    assert nd in (2, 3) and len(shape) == nd
    present = np.asarray(present, dtype=np.int64)
    n = len(present)
    bbox = np.asarray(bbox).reshape(n, 6).astype(np.int64)
    a, b, faces = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (a, b, faces))
    row_a, row_b = np.searchsorted(present, a), np.searchsorted(present, b)       # a == 0 has no row
    between = a > 0
    boundary = np.zeros(n, dtype=np.int64)
    contact = np.zeros(n, dtype=np.int64)
    neighbours = np.zeros(n, dtype=np.int64)
    np.add.at(boundary, row_b, faces)
    np.add.at(boundary, row_a[between], faces[between])
    for rows in (row_a[between], row_b[between]):
        np.add.at(contact, rows, faces[between])
        np.add.at(neighbours, rows, 1)
    touches = np.zeros(n, dtype=bool)
    for k, extent in zip(range(3 - nd, 3), shape):
        touches |= (bbox[:, k] == 0) | (bbox[:, 3 + k] == int(extent) - 1)
    cols = {"boundary_faces": boundary, "contact_faces": contact, "num_neighbours": neighbours,
            "touches_border": touches.astype(np.int64)}
    if nd == 2:
        classes = np.asarray(classes).reshape(n, 4)
        cols["border_pixels"] = classes[:, 0].astype(np.int64)
        cols["perimeter"] = perimeter_from_classes(classes)
    return cols


def topology_columns(area, counts, nd):
    """The topology columns of ``region_table`` from integer counts.  area (n) pixel counts, counts (n, 5)
    ``clx_region_topology``'s rows ``T1 T2 T3 E_hi E_lo`` of the same objects; nd 2 or 3.  ``euler_number`` (8- / 26-
    connectivity, scikit-image's default) and ``euler_number_conn1`` (4- / 6-connectivity) are ``E / 2**nd``; with
    ``N1 = T1 / 2**(nd-1)``, ``N2 = T2 / 2**(nd-2)``, ``N3 = T3`` the boundary pairs along the axial, face-diagonal and
    space-diagonal directions, ``perimeter_crofton = (π/8)·(N1 + N2/√2)`` (2-D, four directions) and ``surface_area =
    4·(w1·N1/2 + w2·N2/(2√2) + w3·N3/(2√3))``, ``sphericity = π^(1/3)·(6·area)^(2/3) / surface_area`` (3-D).  The
    divisions by powers of two are exact integer divisions."""
    assert nd in (2, 3)
    area = [int(v) for v in np.asarray(area).reshape(-1)]
    rows = [[int(v) for v in r] for r in np.asarray(counts).reshape(-1, 5)]
    assert len(area) == len(rows)
    cell = 1 << nd
    for r in rows:
        assert r[0] % (cell // 2) == 0 and r[1] % (cell // 4) == 0 and r[3] % cell == 0 and r[4] % cell == 0, r
    cols = {"euler_number": np.array([r[3] // cell for r in rows], dtype=np.int64),
            "euler_number_conn1": np.array([r[4] // cell for r in rows], dtype=np.int64)}
    n1 = np.array([r[0] // (cell // 2) for r in rows], dtype=np.float64)
    n2 = np.array([r[1] // (cell // 4) for r in rows], dtype=np.float64)
    n3 = np.array([r[2] for r in rows], dtype=np.float64)
    if nd == 2:
        cols["perimeter_crofton"] = (math.pi / 8.0) * (n1 + n2 / _SQRT2)
    else:
        w1, w2, w3 = SURFACE_WEIGHTS
        surface = 4.0 * (w1 * n1 / 2.0 + w2 * n2 / (2.0 * _SQRT2) + w3 * n3 / (2.0 * _SQRT3))
        cols["surface_area"] = surface
        cols["sphericity"] = math.pi ** (1.0 / 3.0) * (6.0 * np.array(area, dtype=np.float64)) ** (2.0 / 3.0) / surface
    return cols


def _sqrt_ratio(num, den):
    """``sqrt(num / den)`` of Python ints (``num >= 0``, ``den > 0``) as a float64, correctly rounded: the integer square
    root of the ratio scaled to more than 60 bits, a sticky bit for what it drops, one int -> float conversion"""
    num, den = int(num), int(den)
    assert num >= 0 and den > 0
    if num == 0:
        return 0.0
    k = max(0, (124 + den.bit_length() - num.bit_length()) // 2)
    scaled = num << (2 * k)
    q = scaled // den
    s = math.isqrt(q)
    sticky = int(s * s != q or q * den != scaled)
    return math.ldexp(float(2 * s + sticky), -(k + 1))


def hull_columns(area, hull, nd):
    """The convex hull columns of ``region_table`` from integers.  area (n) pixel counts, hull (n, 5)
    ``clx_region_hull``'s rows ``A2 NV F2 C L2`` of the same objects; nd 2 or 3.  The object is the union of its pixels as
    closed unit squares (cubes), its hull that of the pixels' corner points: NOT scikit-image's definitions, which count
    the pixels of the rasterised ``convex_hull_image`` and take the Feret diameter from a contour.  2-D: ``area_convex =
    A2 / 2``, ``solidity = area / area_convex`` (at most 1), ``feret_diameter_max = sqrt(F2)``, ``feret_diameter_min =
    C / sqrt(L2)`` (the minimum caliper width, ImageJ's MinFeret) and ``hull_vertices = NV`` (int64); a one-pixel object
    has 1, 1.0, sqrt 2, 1.0, 4.  3-D: ``feret_diameter_max`` only; convex volume and solidity in 3-D are not computed.
    Every float is one correctly rounded operation on exact integers."""
    assert nd in (2, 3)
    area = [int(v) for v in np.asarray(area).reshape(-1)]
    rows = [[int(v) for v in r] for r in np.asarray(hull).reshape(-1, 5)]
    assert len(area) == len(rows)
    feret_max = np.array([_sqrt_ratio(r[2], 1) for r in rows], dtype=np.float64)
    if nd == 3:
        return {"feret_diameter_max": feret_max}
    return {"area_convex": np.array([r[0] / 2 for r in rows], dtype=np.float64),
            "solidity": np.array([2 * a / r[0] for a, r in zip(area, rows)], dtype=np.float64),
            "feret_diameter_max": feret_max,
            "feret_diameter_min": np.array([_sqrt_ratio(r[3] * r[3], r[4]) for r in rows], dtype=np.float64),
            "hull_vertices": np.array([r[1] for r in rows], dtype=np.int64)}


def inscribed_columns(area, rows, shape, nd):
    """The inscribed circle / ball columns of ``region_table`` from integers.  area (n) pixel counts, rows (n, 3)
    ``clx_region_inscribed``'s rows ``D2, index, Σd²`` of the same objects, shape the map's ``nd`` extents; nd 2 or 3.
    ``inscribed_radius = sqrt(D2)``: the largest distance from a pixel centre of the object to the nearest pixel centre
    that is not the object's (scipy's ``distance_transform_edt(labels == i).max()``; a one-pixel object with anything
    beside it has 1.0), ``inscribed_centre_z/_y/_x`` (2-D: y and x; int64) the first pixel in raster order that attains
    it, ``distance_sq_mean = Σd² / area``.  Radius and mean are ``inf`` where ``D2 == DIST_INF``: the object fills a
    map that has no edge to measure to.  Every float is one correctly rounded operation on exact integers."""
    assert nd in (2, 3) and len(shape) == nd
    area = [int(v) for v in np.asarray(area).reshape(-1)]
    rows = [[int(v) for v in r] for r in np.asarray(rows).reshape(-1, 3)]
    assert len(area) == len(rows)
    inf = [r[0] >= DIST_INF for r in rows]
    cols = {"inscribed_radius": np.array([math.inf if i else _sqrt_ratio(r[0], 1) for r, i in zip(rows, inf)], dtype=np.float64)}
    index = np.array([r[1] for r in rows], dtype=np.int64)
    centre = np.unravel_index(index, tuple(int(v) for v in shape)) if len(rows) else (np.zeros(0, dtype=np.int64),) * nd
    for axis, c in zip(_AXES[3 - nd:], centre):
        cols[f"inscribed_centre_{axis}"] = np.asarray(c, dtype=np.int64)
    cols["distance_sq_mean"] = np.array([math.inf if i else r[2] / a for r, a, i in zip(rows, area, inf)], dtype=np.float64)
    return cols


def quantile_ranks(area, q):
    """Where the ``q``-quantile of ``area`` sorted values lies, by NumPy's default ("linear") definition with the index
    computed without rounding: ``h = Fraction(q) * (area - 1)`` with ``q`` taken as the float64 it is, ``lo = floor(h)``,
    ``hi = ceil(h)``, ``t = h - lo``.  area (n) counts >= 1.  Returns ``(lo, hi, t)``: int64 arrays (n) of 0-based ranks and a
    list of n ``Fraction`` in [0, 1)."""
    q = float(q)
    if not 0.0 <= q <= 1.0:                                  # a NaN fails both comparisons
        raise ValueError(f"quantile_ranks: q must lie in [0, 1], got {q}")
    fq = Fraction(q)
    area = [int(a) for a in np.asarray(area).reshape(-1)]
    if any(a < 1 for a in area):
        raise ValueError("quantile_ranks: every area must be >= 1")
    h = [fq * (a - 1) for a in area]
    lo = [v.numerator // v.denominator for v in h]
    hi = [-((-v.numerator) // v.denominator) for v in h]
    return np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64), [v - f for v, f in zip(h, lo)]


def quantile_columns(low, high, t):
    """``float(Fraction(a) + (Fraction(b) - Fraction(a)) * t)`` per object as float64: the quantile from the order statistics
    ``a = x_(lo)`` (low) and ``b = x_(hi)`` (high), finite numbers of any one dtype, and ``quantile_ranks``' ``t``.  The sum
    is exact; the only rounding is the last step, as in ``_exact_div``.  Where ``t == 0`` the column is ``a`` itself."""
    low, high = np.asarray(low).reshape(-1), np.asarray(high).reshape(-1)
    assert len(low) == len(high) == len(t)
    integral = low.dtype.kind in "ui"
    out = np.empty(len(low), dtype=np.float64)
    for i, (a, b, w) in enumerate(zip(low, high, t)):
        if w == 0 or a == b:
            out[i] = float(a)
        else:
            fa, fb = (Fraction(int(a)), Fraction(int(b))) if integral else (Fraction(float(a)), Fraction(float(b)))
            out[i] = float(fa + (fb - fa) * w)
    return out


def _check_quantiles(quantiles, mad, raw, who="region_table"):
    """-> tuple of float64 quantiles (empty for None) after the checks the table's new arguments share"""
    qs = () if quantiles is None else tuple(float(q) + 0.0 for q in quantiles)       # -0.0 is 0.0, in the column's name too
    if len(qs) > MAX_QUANTILES:
        raise ValueError(f"{who}: at most {MAX_QUANTILES} quantiles, got {len(qs)}")
    for q in qs:
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"{who}: a quantile must lie in [0, 1], got {q}")
    if len(set(qs)) != len(qs):
        raise ValueError(f"{who}: quantiles must be distinct, got {list(qs)}")
    if (qs or mad) and raw is None:
        raise ValueError(f"{who}: quantiles and mad need raw")
    return qs


def _check_texture(levels, distance, value_range, who="region_table"):
    """-> (levels, distance, (lo, hi) or None) after the checks the texture arguments share"""
    levels, distance = int(levels), int(distance)
    if not MIN_LEVELS <= levels <= MAX_LEVELS:
        raise ValueError(f"{who}: texture levels must lie in [{MIN_LEVELS}, {MAX_LEVELS}], got {levels}")
    if not 1 <= distance <= MAX_TEXTURE_DISTANCE:
        raise ValueError(f"{who}: texture distance must lie in [1, {MAX_TEXTURE_DISTANCE}], got {distance}")
    if value_range is not None:
        lo, hi = (float(v) for v in value_range)
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"{who}: texture range must be finite with lo <= hi, got {(lo, hi)}")
        value_range = (lo, hi)
    return levels, distance, value_range


def texture_directions(nd):
    """The offsets of {-1, 0, 1}^nd that are lexicographically greater than zero, ascending: 4 in 2-D, ``(dy, dx)`` =
    (0,1), (1,-1), (1,0), (1,1); 13 in 3-D.  The order of ``cooccurrence``'s direction axis."""
    assert nd in (2, 3)
    codes = range(14, 18) if nd == 2 else range(14, 27)      # (dz+1)*9 + (dy+1)*3 + (dx+1), from (0, 0, 1) on
    return [tuple(v - 1 for v in (c // 9, c // 3 % 3, c % 3))[3 - nd:] for c in codes]


def _neg_xlog2x(p, axis):
    """``-Σ p log2 p`` along ``axis`` (a tuple or an int), a zero ``p`` contributing 0"""
    positive = p > 0
    return -(p * np.log2(np.where(positive, p, 1.0))).sum(axis=axis)


def _texture_slice(counts):
    """texture_columns for a slice of objects -> (pairs (n), features (13, n))"""
    n, ndir, L, _ = counts.shape
    C = counts.astype(np.int64)
    N = C.sum(axis=(2, 3))                                   # (n, ndir) pairs per direction
    present = N > 0
    T64 = 2 * N
    dt = np.int64 if int(T64.max(initial=0)) <= _TEXTURE_INT64_MAX_T else object
    S = (C + C.transpose(0, 1, 3, 2)).astype(dt).reshape(n, ndir, L * L)
    T = T64.astype(dt)
    i = np.arange(L).astype(dt)
    ii, jj = (v.reshape(-1) for v in np.meshgrid(i, i, indexing="ij"))
    # exact integer numerators over T or T^2; with levels <= 32 the weights are at most 62^2 = 3844 < 2^12, so every one
    # of them is below 2^12 T^2 in magnitude and fits int64 for T <= 2^25; above that they are Python ints
    A = (S * S).sum(axis=2)                                  # Σ S^2                <= T^2
    M1 = (S * ii).sum(axis=2)                                # Σ i S = T μ          <= 31 T
    M2 = (S * (ii * ii)).sum(axis=2)                         # Σ i^2 S              <= 961 T
    MIJ = (S * (ii * jj)).sum(axis=2)                        # Σ i j S              <= 961 T
    DA = (S * abs(ii - jj)).sum(axis=2)                      # Σ k D_k              <= 31 T
    DQ = (S * ((ii - jj) * (ii - jj))).sum(axis=2)           # Σ k^2 D_k            <= 961 T
    SA = (S * (ii + jj)).sum(axis=2)                         # Σ k P_k              <= 62 T
    SQ = (S * ((ii + jj) * (ii + jj))).sum(axis=2)           # Σ k^2 P_k            <= 3844 T
    V = T * M2 - M1 * M1                                     # T^2 σ^2              <= 961 T^2
    Tf = np.where(present, T64, 1).astype(np.float64)        # exact: T < 2^33

    def ratio(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return num.astype(np.float64) / den.astype(np.float64)

    TT = T * T
    f = {}
    f["asm"] = ratio(A, TT)
    f["contrast"] = ratio(DQ, T)
    f["correlation"] = np.where(V == 0, 1.0, ratio(T * MIJ - M1 * M1, V))
    f["variance"] = ratio(V, TT)
    f["sum_average"] = ratio(SA, T)
    f["sum_variance"] = ratio(T * SQ - SA * SA, TT)
    f["difference_variance"] = ratio(T * DQ - DA * DA, TT)
    # the others in float64: S, its row sums and its diagonal sums are integers below 2^53, so every probability is ONE
    # rounding of an exact ratio
    Sf = (C + C.transpose(0, 1, 3, 2)).astype(np.float64)
    flat = Sf.reshape(n * ndir, L * L)
    ki, kj = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    diff_of = (abs(ki - kj).reshape(-1)[:, None] == np.arange(L)[None, :]).astype(np.float64)              # (L^2, L)
    sum_of = ((ki + kj).reshape(-1)[:, None] == np.arange(2 * L - 1)[None, :]).astype(np.float64)          # (L^2, 2L-1)
    p = Sf / Tf[:, :, None, None]
    px = Sf.sum(axis=3) / Tf[:, :, None]
    p_diff = (flat @ diff_of).reshape(n, ndir, L) / Tf[:, :, None]          # sums of integers in float64: exact
    p_sum = (flat @ sum_of).reshape(n, ndir, 2 * L - 1) / Tf[:, :, None]
    k = np.arange(L, dtype=np.float64)
    f["idm"] = (p_diff / (1.0 + k * k)).sum(axis=2)
    f["sum_entropy"] = _neg_xlog2x(p_sum, 2)
    f["entropy"] = hxy = _neg_xlog2x(p, (2, 3))
    f["difference_entropy"] = _neg_xlog2x(p_diff, 2)
    hx = _neg_xlog2x(px, 2)
    lx = np.log2(np.where(px > 0, px, 1.0))
    lxy = lx[:, :, :, None] + lx[:, :, None, :]              # log2(px(i) px(j)) where both are positive
    hxy1 = -(p * lxy).sum(axis=(2, 3))
    hxy2 = -(px[:, :, :, None] * px[:, :, None, :] * lxy).sum(axis=(2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        f["info_correlation_1"] = np.where(hx == 0.0, 0.0, (hxy - hxy1) / hx)
    f["info_correlation_2"] = np.sqrt(np.maximum(0.0, 1.0 - np.exp2(-2.0 * (hxy2 - hxy))))
    ndirs = present.sum(axis=1)
    out = np.empty((len(TEXTURE_FEATURES), n), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for row, name in enumerate(TEXTURE_FEATURES):
            out[row] = np.where(present, f[name], 0.0).sum(axis=1) / ndirs          # 0 / 0: no direction has a pair
    return N.sum(axis=1), out


def texture_columns(counts, nd):
    """Haralick's texture features from ``cooccurrence``'s integer counts.  counts (n, ndir, levels, levels), ndir 4 for
    nd == 2 and 13 for nd == 3.  Returns a dict of ``pairs`` (int64: the ordered same-object pixel pairs, summed over the
    directions) and thirteen float64 columns.  Per direction with ``N = Σ C > 0``: ``S = C + Cᵀ``, ``p = S / (2N)``, ``i, j``
    0-based levels, ``px(i) = Σ_j p(i, j)``, ``μ = Σ i px(i)``, ``σ² = Σ (i − μ)² px(i)``, ``p₊(k) = Σ_{i+j=k} p``,
    ``p₋(k) = Σ_{|i−j|=k} p``, entropies in bits, a zero probability contributing 0:
    ``asm`` Σ p²; ``contrast`` Σ k² p₋(k); ``correlation`` (Σ i j p − μ²) / σ², 1.0 where σ² = 0; ``variance`` σ²; ``idm``
    Σ p / (1 + (i−j)²); ``sum_average`` Σ k p₊(k); ``sum_variance`` Σ (k − sum_average)² p₊(k); ``sum_entropy`` −Σ p₊ log2 p₊;
    ``entropy`` HXY = −Σ p log2 p; ``difference_variance`` the variance of p₋; ``difference_entropy`` −Σ p₋ log2 p₋;
    ``info_correlation_1`` (HXY − HXY1) / HX with HXY1 = −Σ p log2(px(i) px(j)) and HX the entropy of px, 0.0 where HX = 0;
    ``info_correlation_2`` sqrt(max(0, 1 − 2^(−2 (HXY2 − HXY)))) with HXY2 = −Σ px(i) px(j) log2(px(i) px(j)).
    A column is the mean over the directions that have a pair, NaN where none has (a one-pixel object, a distance larger
    than the object).  These are the project's own stated conventions (Haralick's 1973 features with 0-based levels, base-2
    logarithms and his 14th left out); no fixture compares them with mahotas, scikit-image or CellProfiler, whose
    conventions differ from each other in the level numbering, the logarithm and the normalisation.
    The seven rational features (asm, contrast, correlation, variance, sum_average, sum_variance, difference_variance) are
    exact integer numerators and denominators (vectorised int64 while ``2N <= 2**25``, which bounds every numerator by
    ``2**12 (2N)**2 < 2**63``; Python ints above that), each converted to float64 and divided once; the others are float64
    sums of probabilities that are each one rounding of an exact ratio.  Vectorised over the objects."""
    assert nd in (2, 3)
    counts = np.asarray(counts)
    ndir = 4 if nd == 2 else 13
    if counts.ndim != 4 or counts.shape[1] != ndir or counts.shape[2] != counts.shape[3]:
        raise ValueError(f"texture_columns: counts must have shape (n, {ndir}, levels, levels), got {counts.shape}")
    if counts.dtype.kind not in "ui":
        raise TypeError(f"texture_columns: counts must be integers, got {counts.dtype}")
    n = counts.shape[0]
    step = max(1, _TEXTURE_SLICE_CELLS // (ndir * counts.shape[2] * counts.shape[3]))
    parts = [_texture_slice(counts[a:a + step]) for a in range(0, n, step)]
    cols = {"pairs": np.concatenate([p[0] for p in parts]).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)}
    values = np.concatenate([p[1] for p in parts], axis=1) if parts else np.zeros((len(TEXTURE_FEATURES), 0))
    for row, name in enumerate(TEXTURE_FEATURES):
        cols[name] = np.ascontiguousarray(values[row])
    return cols


def _check_radial(rings, width, wedges, nd, who="region_table"):
    """-> (rings, width or 0, 1 or 8 wedges) after the checks the radial arguments share; ``nd`` None: not known yet"""
    if isinstance(rings, bool) or rings != int(rings) or not 1 <= int(rings) <= MAX_RINGS:
        raise ValueError(f"{who}: radial rings must be an integer in [1, {MAX_RINGS}], got {rings!r}")
    if width is not None and (isinstance(width, bool) or width != int(width) or not 1 <= int(width) <= MAX_RADIAL_WIDTH):
        raise ValueError(f"{who}: radial width must be None or an integer in [1, {MAX_RADIAL_WIDTH}], got {width!r}")
    if wedges and nd == 3:
        raise ValueError(f"{who}: radial wedges need a 2-D map")
    return int(rings), 0 if width is None else int(width), RADIAL_WEDGES if wedges else 1


def radial_columns(area, count, isum=None, shift=0, nd=2, k=None):
    """The radial columns of ``region_table`` from ``radial_distribution``'s integers, in Python integers.  area (n) pixel
    counts, count (n, rings, W) pixels per ring and wedge (W 1 or 8; 8 needs nd == 2), and either
    ``isum=None``: the columns that belong to no channel, ``radial_area_r{j}`` (int64): the pixels of ring j, ring 0 the rim;
    or ``isum`` (n, rings, W) the sums of channel ``k`` quantised with ``shift``: per ring j, with S_j and N_j the ring's sum and
    count, S the object's sum and A its area,
    ``radial_mean_r{j}_c{k}`` = S_j / N_j, one division, then ``ldexp(-shift)``; NaN for an empty ring;
    ``radial_frac_r{j}_c{k}`` = S_j / S, the share of the object's intensity in the ring (CellProfiler's FracAtD); NaN where S = 0;
    ``radial_meanfrac_r{j}_c{k}`` = (S_j A) / (S N_j), the ring's mean over the object's mean (MeanFrac), one rounding of the
    exact rational; NaN for an empty ring or S = 0;
    and with W == 8 ``radial_cv_r{j}_c{k}``: with m_o = S_jo / N_jo the means of the occupied wedges (one division each) and
    w their number, in float64 ``mu = sum(m) / w``, ``sqrt(sum((m - mu)^2) / w) / mu``: the population standard deviation over
    the mean of the wedge means (RadialCV, which no scaling of the channel changes); NaN with no occupied wedge or mu = 0.
    An object thinner than ``rings * width`` leaves inner rings empty in absolute mode, and a small one may leave some empty in
    relative mode (its squared distances take few values); the core ring of relative mode always holds the centre."""
    assert nd in (2, 3)
    count = np.asarray(count)
    if count.ndim != 3 or count.shape[2] not in (1, RADIAL_WEDGES) or (count.shape[2] == RADIAL_WEDGES and nd != 2):
        raise ValueError(f"radial_columns: count must have shape (n, rings, 1) or, in 2-D, (n, rings, {RADIAL_WEDGES}), got {count.shape}")
    n, rings, W = count.shape
    area = [int(v) for v in np.asarray(area).reshape(-1)]
    assert len(area) == n
    N = [[[int(v) for v in ring] for ring in obj] for obj in count.tolist()]
    ring_n = [[sum(ring) for ring in obj] for obj in N]
    for a, r in zip(area, ring_n):
        assert sum(r) == a, "radial_columns: the rings of an object do not add up to its area"
    if isum is None:
        return {f"radial_area_r{j}": np.array([r[j] for r in ring_n], dtype=np.int64) for j in range(rings)}
    isum = np.asarray(isum)
    assert isum.shape == count.shape and isum.dtype.kind in "iu" and k is not None
    S = [[[int(v) for v in ring] for ring in obj] for obj in isum.tolist()]
    ring_s = [[sum(ring) for ring in obj] for obj in S]
    total = [sum(r) for r in ring_s]
    nan = math.nan
    cols = {}
    for j in range(rings):
        mean = np.array([r[j] / c[j] if c[j] else nan for r, c in zip(ring_s, ring_n)], dtype=np.float64)
        cols[f"radial_mean_r{j}_c{k}"] = np.ldexp(mean, -shift) if shift else mean
        cols[f"radial_frac_r{j}_c{k}"] = np.array([r[j] / t if t else nan for r, t in zip(ring_s, total)], dtype=np.float64)
        cols[f"radial_meanfrac_r{j}_c{k}"] = np.array([(r[j] * a) / (t * c[j]) if t and c[j] else nan
                                                       for r, c, t, a in zip(ring_s, ring_n, total, area)], dtype=np.float64)
        if W == RADIAL_WEDGES:
            cv = np.full(n, nan, dtype=np.float64)
            for i in range(n):
                m = np.array([s / c for s, c in zip(S[i][j], N[i][j]) if c], dtype=np.float64)
                if len(m):
                    mu = m.sum() / len(m)
                    if mu != 0.0:
                        d = m - mu
                        cv[i] = math.sqrt((d * d).sum() / len(m)) / mu
            cols[f"radial_cv_r{j}_c{k}"] = cv
    return cols


def _check_products(std, colocalization, coloc_threshold, labels, raw, who="region_table"):
    """-> coloc_threshold as a float after the checks the std / colocalization arguments share (no device is touched)"""
    f = float(coloc_threshold)
    if not 0.0 <= f <= 1.0:                                  # a NaN fails both comparisons
        raise ValueError(f"{who}: coloc_threshold must lie in [0, 1], got {coloc_threshold!r}")
    if (std or colocalization) and raw is None:
        raise ValueError(f"{who}: std and colocalization need raw")
    if colocalization and (raw.ndim == getattr(labels, "ndim", raw.ndim - 1) or raw.shape[0] < 2):
        raise ValueError(f"{who}: colocalization needs at least 2 raw channels")
    return f + 0.0


def quantised(values, shift):
    """``q`` of ``clx_region_intensity`` for values of one raw dtype as Python ints: integers are themselves, floats
    ``rint(ldexp(float64(v), shift))``"""
    values = np.asarray(values).reshape(-1)
    if values.dtype.kind in "ui":
        return [int(v) for v in values]
    return [int(v) for v in np.rint(np.ldexp(values.astype(np.float64), int(shift)))]


def coloc_thresholds(qmax, f):
    """``ceil(f * qmax)`` per object in exact rational arithmetic, ``f`` in [0, 1] taken as the float64 it is and ``qmax`` the
    object's quantised maximum (Python ints): a pixel is "above" where ``q >= threshold``, so a pixel exactly at ``f * qmax`` is.
    ``f = 0`` puts every non-negative pixel above, ``f = 1`` the pixels at the maximum only.  The project's own convention, in
    the manner of CellProfiler's "15 % of the object's maximum".  Returns an int64 array."""
    f = float(f)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"coloc_thresholds: f must lie in [0, 1], got {f}")
    fq = Fraction(f)
    out = np.empty(len(qmax), dtype=np.int64)
    for i, q in enumerate(qmax):
        t = fq * int(q)
        out[i] = -((-t.numerator) // t.denominator)
    return out


PRODUCT_WORDS = 20                      # clx_region_products: words per id
_PRODUCT_SUMS = ("n", "sum_a", "sum_b", "n_both", "sum_a_above", "sum_b_above", "sum_a_both", "sum_b_both")
_PRODUCT_SQUARES = ("sum_aa", "sum_bb", "sum_ab", "sum_aa_both", "sum_bb_both", "sum_ab_both")


def _signed128(lo, hi):
    """Python ints of (lo, hi) uint64 word columns: signed 128-bit, two's complement"""
    out = np.empty(len(lo), dtype=object)
    out[:] = [l + (h << 64) - ((h >> 63) << 128) for l, h in zip(lo.tolist(), hi.tolist())]
    return out


def product_table(words):
    """``clx_region_products``' rows (n, 20) of uint64 words as a dict: int64 arrays ``n, sum_a, sum_b, n_both, sum_a_above,
    sum_b_above, sum_a_both, sum_b_both`` and object arrays of Python ints ``sum_aa, sum_bb, sum_ab, sum_aa_both, sum_bb_both,
    sum_ab_both`` (a (lo, hi) pair is one signed 128-bit integer, two's complement)"""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, PRODUCT_WORDS)
    table = {name: np.ascontiguousarray(words[:, i]).view(np.int64) for i, name in enumerate(_PRODUCT_SUMS)}
    for i, name in enumerate(_PRODUCT_SQUARES):
        table[name] = _signed128(words[:, 8 + 2 * i], words[:, 9 + 2 * i])
    return table


def _signed_root(num, den):
    """``sign(num) * sqrt(num**2 / den)`` of Python ints, NaN where ``den == 0``: one correctly rounded operation"""
    if den == 0:
        return math.nan
    r = _sqrt_ratio(num * num, den)
    return -r if num < 0 else r


def _ratio(num, den):
    return num / den if den else math.nan


def _scaled_column(values, n, exponent):
    c = np.array(values, dtype=np.float64).reshape(n)
    with np.errstate(over="ignore", under="ignore"):           # shifts at both clamps can leave float64's range
        return np.ldexp(c, exponent) if exponent else c


def products_columns(table, shift_a=0, shift_b=0, j=0, k=1, std=False, colocalization=True):
    """The columns of ``region_table`` that need second moments, from ``product_table``'s exact integers (channel ``j`` is a,
    quantised with ``shift_a``; channel ``k`` is b with ``shift_b``), in Python integers.  With ``A = Σa``, ``B = Σb``,
    ``Va = n Σaa − A²``, ``Vb = n Σbb − B²``, ``C = n Σab − A B`` and the subscript T for the sums over the pixels above both
    thresholds:
    ``std=True``: ``intensity_std_c{j}`` = sqrt(Va / n²) · 2^−shift_a, the POPULATION standard deviation (regionprops'
    ``intensity_std``, CellProfiler's StdIntensity), and, where ``k != j``, ``intensity_std_c{k}`` likewise;
    ``colocalization=True``:
    ``coloc_pearson_c{j}_c{k}`` = sign(C) sqrt(C² / (Va Vb)); ``coloc_slope_c{j}_c{k}`` = C / Va · 2^(shift_a − shift_b), the
    regression of channel k on channel j; ``coloc_overlap_c{j}_c{k}`` = sign(Σab_T) sqrt(Σab_T² / (Σaa_T Σbb_T));
    ``coloc_k1_c{j}_c{k}`` = Σab_T / Σaa_T · 2^(shift_a − shift_b); ``coloc_k2_c{j}_c{k}`` = Σab_T / Σbb_T · 2^(shift_b − shift_a);
    ``coloc_manders1_c{j}_c{k}`` = Σa_T / Σa|above a; ``coloc_manders2_c{j}_c{k}`` = Σb_T / Σb|above b.
    Every column is ONE correctly rounded operation on exact integers and an exact scaling by a power of two; NaN where its
    denominator is 0 (a constant channel has no correlation, an object with no pixel above both thresholds no overlap)."""
    n = [int(v) for v in table["n"]]
    A, B = [int(v) for v in table["sum_a"]], [int(v) for v in table["sum_b"]]
    aa, bb, ab = (list(table[name]) for name in ("sum_aa", "sum_bb", "sum_ab"))
    Va = [m * s - a * a for m, s, a in zip(n, aa, A)]
    Vb = [m * s - b * b for m, s, b in zip(n, bb, B)]
    assert all(v >= 0 for v in Va) and all(v >= 0 for v in Vb), "products_columns: a negative variance: the sums do not belong together"
    scale = int(shift_a) - int(shift_b)
    cols = {}

    def column(values, exponent=0):
        return _scaled_column(values, len(n), exponent)

    if std:
        cols[f"intensity_std_c{j}"] = column([_sqrt_ratio(v, m * m) if m else math.nan for v, m in zip(Va, n)], -int(shift_a))
        if k != j:
            cols[f"intensity_std_c{k}"] = column([_sqrt_ratio(v, m * m) if m else math.nan for v, m in zip(Vb, n)], -int(shift_b))
    if colocalization:
        C = [m * s - a * b for m, s, a, b in zip(n, ab, A, B)]
        aT, bT, abT = (list(table[name]) for name in ("sum_aa_both", "sum_bb_both", "sum_ab_both"))
        pair = f"c{j}_c{k}"
        cols[f"coloc_pearson_{pair}"] = column([_signed_root(c, va * vb) for c, va, vb in zip(C, Va, Vb)])
        cols[f"coloc_slope_{pair}"] = column([_ratio(c, va) for c, va in zip(C, Va)], scale)
        cols[f"coloc_overlap_{pair}"] = column([_signed_root(s, x * y) for s, x, y in zip(abT, aT, bT)])
        cols[f"coloc_k1_{pair}"] = column([_ratio(s, x) for s, x in zip(abT, aT)], scale)
        cols[f"coloc_k2_{pair}"] = column([_ratio(s, y) for s, y in zip(abT, bT)], -scale)
        cols[f"coloc_manders1_{pair}"] = column([_ratio(int(s), int(d)) for s, d in zip(table["sum_a_both"], table["sum_a_above"])])
        cols[f"coloc_manders2_{pair}"] = column([_ratio(int(s), int(d)) for s, d in zip(table["sum_b_both"], table["sum_b_above"])])
    return cols


WEIGHTED_WORDS = 21                     # clx_region_weighted: words per id
BORDER_WORDS = 7                        # clx_region_border_intensity: words per id
NO_PEAK = (1 << 64) - 1                 # clx_region_weighted's word 2 where no pixel carries the key
_WEIGHTED_MOMENTS = ("sum_qz", "sum_qy", "sum_qx", "sum_qzz", "sum_qyy", "sum_qxx", "sum_qzy", "sum_qzx", "sum_qyx")


def weighted_table(words):
    """``clx_region_weighted``'s rows (n, 21) of uint64 words as a dict: int64 arrays ``n`` (the counted pixels) and ``sum_q``,
    an object array ``peak`` (the flat index of the first pixel that attains the maximum, ``NO_PEAK`` where there is none) and
    object arrays of Python ints ``sum_qz, sum_qy, sum_qx, sum_qzz, sum_qyy, sum_qxx, sum_qzy, sum_qzx, sum_qyx`` (a (lo, hi) pair
    is one signed 128-bit integer, two's complement)"""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, WEIGHTED_WORDS)
    table = {"n": np.ascontiguousarray(words[:, 0]).view(np.int64), "sum_q": np.ascontiguousarray(words[:, 1]).view(np.int64)}
    table["peak"] = np.empty(len(words), dtype=object)
    table["peak"][:] = words[:, 2].tolist()
    for i, name in enumerate(_WEIGHTED_MOMENTS):
        table[name] = _signed128(words[:, 3 + 2 * i], words[:, 4 + 2 * i])
    return table


def border_table(words):
    """``clx_region_border_intensity``'s rows (n, 7) of uint64 words as a dict: int64 arrays ``pixels`` (the border pixels),
    ``n`` (those whose value was counted) and ``sum_q``, uint64 arrays ``key_min`` and ``key_max`` (order keys) and an object array
    of Python ints ``sum_qq``"""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, BORDER_WORDS)
    table = {name: np.ascontiguousarray(words[:, i]).view(np.int64) for i, name in enumerate(("pixels", "n", "sum_q"))}
    table["key_min"], table["key_max"] = words[:, 3].copy(), words[:, 4].copy()
    table["sum_qq"] = _signed128(words[:, 5], words[:, 6])
    return table


def weighted_columns(area, sum1, table, shift, nd, k, shape):
    """The intensity-weighted columns of channel ``k`` of ``region_table`` from exact integers.  area (n) pixel counts and sum1
    (n, 3) ``clx_region_moments``' ``Σz Σy Σx`` of the same objects (for the plain centroid), table ``weighted_table``'s dict
    of them, its sums those of ``q = rint(v * 2**shift)``; nd 2 or 3 (2-D: the z entries are ignored); shape the map's ``nd``
    extents, which place the peak.  With ``Q = Σq``:
    ``intensity_sum_c{k}`` = Q · 2^−shift (CellProfiler's IntegratedIntensity);
    ``centroid_weighted_{a}_c{k}`` = Σq·a / Q (regionprops' ``centroid_weighted``, CellProfiler's Location_CenterMassIntensity);
    ``cov_weighted_{ab}_c{k}`` = (Q · Σq·a·b − Σq·a · Σq·b) / Q², in ``shape_columns``' pair order (the order-2 central weighted
    moments over Q);
    ``mass_displacement_c{k}`` = the distance between ``centroid_*`` and ``centroid_weighted_*`` (MassDisplacement), the square
    root of the exact fraction;
    ``intensity_peak_{a}_c{k}`` (int64) = the coordinates of the first pixel in raster order that attains the object's maximum
    (Location_MaxIntensity; ties go to the first pixel: the project's own convention).
    Every float is ONE correctly rounded operation on exact integers (and an exact scaling by a power of two); NaN where
    Q = 0.  Negative weights are taken as they are.  A peak of ``NO_PEAK`` raises: the object has pixels, one of them is its
    maximum."""
    assert nd in (2, 3) and len(shape) == nd
    n = len(table["n"])
    area = [int(v) for v in np.asarray(area).reshape(-1)]
    s1 = [[int(v) for v in r] for r in np.asarray(sum1).reshape(-1, 3).tolist()]
    assert len(area) == len(s1) == n
    Q = [int(v) for v in table["sum_q"]]
    m1 = [list(table[name]) for name in _WEIGHTED_MOMENTS[:3]]
    m2 = [list(table[name]) for name in _WEIGHTED_MOMENTS[3:]]
    axes = range(3 - nd, 3)
    nan = math.nan
    cols = {f"intensity_sum_c{k}": _scaled_column([float(q) for q in Q], n, -int(shift))}
    for a in axes:
        cols[f"centroid_weighted_{_AXES[a]}_c{k}"] = np.array([m / q if q else nan for m, q in zip(m1[a], Q)], dtype=np.float64).reshape(n)
    for p, (a, b) in enumerate(_PAIRS):
        if a >= 3 - nd:
            cols[f"cov_weighted_{_AXES[a]}{_AXES[b]}_c{k}"] = np.array(
                [(q * s - x * y) / (q * q) if q else nan for q, s, x, y in zip(Q, m2[p], m1[a], m1[b])], dtype=np.float64).reshape(n)
    disp = []
    for i, (A, q) in enumerate(zip(area, Q)):
        disp.append(_sqrt_ratio(sum((s1[i][a] * q - m1[a][i] * A) ** 2 for a in axes), (A * q) ** 2) if q and A else nan)
    cols[f"mass_displacement_c{k}"] = np.array(disp, dtype=np.float64).reshape(n)
    peak = [int(v) for v in table["peak"]]
    if any(v == NO_PEAK for v in peak):
        raise RuntimeError("weighted_columns: internal error: an object without a peak pixel")
    where = np.unravel_index(np.array(peak, dtype=np.int64), tuple(int(v) for v in shape)) if n else (np.zeros(0, dtype=np.int64),) * nd
    for axis, c in zip(_AXES[3 - nd:], where):
        cols[f"intensity_peak_{axis}_c{k}"] = np.asarray(c, dtype=np.int64)
    return cols


def border_intensity_columns(table, shift=0, raw_type=None, k=None):
    """The border columns of ``region_table`` from ``border_table``'s exact integers.  ``k=None``: the column that belongs to no
    channel, ``intensity_border_pixels`` (int64): the object's pixels with a face neighbour (4 in 2-D, 6 in 3-D) that is not the
    object's, the outside of the image among them; in 2-D it equals ``border_pixels``.  Else the columns of channel ``k``, whose
    sums are those of ``q = rint(v * 2**shift)`` and whose keys decode to ``raw_type`` (0 float32, 1 float64, 2 int32), over the
    border pixels (CellProfiler's *IntensityEdge): ``intensity_border_sum_c{k}`` = Σq · 2^−shift, ``intensity_border_mean_c{k}``
    = Σq / n · 2^−shift, ``intensity_border_std_c{k}`` = sqrt((n Σq² − (Σq)²) / n²) · 2^−shift, the POPULATION standard
    deviation, ``intensity_border_min_c{k}`` and ``intensity_border_max_c{k}`` in the raw dtype.  Every float is ONE correctly
    rounded operation on exact integers and an exact scaling by a power of two; NaN where n = 0."""
    if k is None:
        return {"intensity_border_pixels": np.asarray(table["pixels"]).astype(np.int64).reshape(-1)}
    from .segment import _decode_keys

    n = [int(v) for v in table["n"]]
    S = [int(v) for v in table["sum_q"]]
    SS = list(table["sum_qq"])
    var = [m * ss - s * s for m, s, ss in zip(n, S, SS)]
    assert all(v >= 0 for v in var), "border_intensity_columns: a negative variance: the sums do not belong together"
    nan = math.nan
    values = _decode_keys(np.stack([np.asarray(table["key_min"], dtype=np.uint64), np.asarray(table["key_max"], dtype=np.uint64)],
                                   axis=1).reshape(-1, 2), raw_type)
    return {f"intensity_border_sum_c{k}": _scaled_column([float(s) for s in S], len(n), -int(shift)),
            f"intensity_border_mean_c{k}": _scaled_column([s / m if m else nan for s, m in zip(S, n)], len(n), -int(shift)),
            f"intensity_border_std_c{k}": _scaled_column([_sqrt_ratio(v, m * m) if m else nan for v, m in zip(var, n)], len(n), -int(shift)),
            f"intensity_border_min_c{k}": values[:, 0].copy(), f"intensity_border_max_c{k}": values[:, 1].copy()}


def _check_weighted(weighted, border_intensity, raw, who="region_table"):
    if (weighted or border_intensity) and raw is None:
        raise ValueError(f"{who}: weighted and border_intensity need raw")


def _extents(shape, who):
    """-> the number of extents of a map's ``shape``, which must be 2 or 3"""
    if len(shape) not in (2, 3):
        raise ValueError(f"{who}: shape must have 2 or 3 extents, got {len(shape)}")
    return len(shape)


def _raster_columns(prefix, index, shape, who, mask=None):
    """the pixels of the raster indices ``index`` (checked to lie inside the map) in a map of ``shape``, as the int64 columns
    ``<prefix>_z/_y/_x`` (2-D: y and x); -1 where ``mask`` is given and false"""
    nd = _extents(shape, who)
    where = np.unravel_index(index, tuple(int(v) for v in shape)) if len(index) else (np.zeros(0, dtype=np.int64),) * nd
    where = [np.asarray(c, dtype=np.int64) for c in where]
    return {f"{prefix}_{axis}": c if mask is None else np.where(mask, c, -1) for axis, c in zip(_AXES[3 - nd:], where)}


def _real_fraction(value, who, name, none=False):
    """a real number >= 0 as an exact Fraction; None stays None where ``none`` allows it"""
    if value is None and none:
        return None
    if isinstance(value, bool) or not isinstance(value, (numbers.Real, np.integer, np.floating)):
        raise TypeError(f"{who}: {name} must be a real number{' or None' if none else ''}, got {type(value).__name__}")
    if isinstance(value, (float, np.floating)) and not math.isfinite(value):
        raise ValueError(f"{who}: {name} must be finite, got {value!r}")
    exact = Fraction(float(value)) if isinstance(value, np.floating) else Fraction(value)
    if exact < 0:
        raise ValueError(f"{who}: {name} must be >= 0, got {value!r}")
    return exact


def _format(value):
    """a column's value in a CSV line: floats as ``%.17g``"""
    return "%.17g" % value if isinstance(value, (float, np.floating)) else "%d" % value
