"""Measure stage: the per-object table users take from ``skimage.measure.regionprops`` on the host —
area, bounding box, centroid, covariance, equivalent diameter and mean / min / max intensity per raw
channel — from integer sums gathered in one pass over the label map on the device
(``csrc/measure.hip``: ``clx_region_moments``, ``clx_region_intensity``).  The sums are exact integers, so
the only rounding in a column is its final division.  On request also what an object's BOUNDARY gives: the faces it
shares with every other object (``contact_pairs``: the region adjacency graph), with the background and the image edge,
and in 2-D its border pixels and perimeter (``clx_region_contacts``, ``clx_region_perimeter``), all integer counts too.
Also on request its TOPOLOGY and smooth boundary measure: the Euler numbers (holes, cavities, tunnels, pieces), the Crofton
perimeter in 2-D, surface area and sphericity in 3-D, from integer sums over the 2 x 2 (x 2) windows of the map
(``clx_region_topology``).  And its CONVEX HULL: convex area, solidity and the maximum / minimum Feret diameter from the hull
of the pixels' corner points, exact integers again (``clx_region_hull``; the definitions are the project's own, not
scikit-image's rasterised ones: ``hull_columns``).  And its THICKNESS: the largest inscribed circle / ball and where it sits,
from the label-aware distance map (``label_distance_sq``: for every object pixel the squared distance to the nearest pixel
of another value; ``clx_label_distance_sq``, ``clx_region_inscribed``, ``inscribed_columns``).  And the ORDER STATISTICS of
its intensity: quantiles (the median among them) and the median absolute deviation per raw channel, which a one-pass sum
cannot give: the pixels' order-preserving keys are bucketed by object and selected by rank on the device
(``csrc/region_order.hip``: ``clx_region_order_stats``).  A selected key is one of the values, so it is exact; the
interpolation between two of them is rational arithmetic with one rounding (``quantile_ranks``, ``quantile_columns``).
And its TEXTURE, the one family of columns that changes when an object's pixels are shuffled: the grey-level co-occurrence
matrices of every object per raw channel (``cooccurrence``; ``csrc/region_texture.hip``: ``clx_region_cooccurrence``), integer
counts again, and Haralick's thirteen features of them (``texture_columns``).  The grey levels divide the range between the
smallest and the largest value under the objects of ONE image: levels are relative to each image's objects, so texture
columns of two images are comparable only where their ranges are (or where ``region_table`` is given a ``texture_range``).
And its RADIAL DISTRIBUTION, where inside the object the signal sits: every pixel is sorted into a ring by its distance to the
object's boundary (and in 2-D into one of eight wedges around the inscribed centre) and counted and summed per ring
(``radial_distribution``; ``csrc/region_radial.hip``: ``clx_region_radial``), integers again; ``radial_columns`` forms the
mean, the fraction of the object's sum and the normalised mean of every ring and the variation around it (CellProfiler's
FracAtD, MeanFrac, RadialCV).
And its SECOND MOMENTS, the columns that compare a channel with itself or with another: the intensity standard deviation and,
for every pair of raw channels, Pearson's correlation, the regression slope, the overlap coefficient, K1 / K2 and the Manders
coefficients inside every object (CellProfiler's MeasureColocalization).  They need Σ q_a q_b, which 64 bits do not hold for
values quantised to 62 - L bits: the products are summed exactly in 128 bits on the device (``channel_products``;
``csrc/region_coloc.hip``: ``clx_region_products``) and ``products_columns`` rounds once.
And WHERE the signal sits, in coordinates, and what it is on the object's RIM: the intensity-weighted centroid and covariance, the
distance between the plain and the weighted centroid, the integrated intensity and the position of the brightest pixel
(regionprops' ``centroid_weighted``, CellProfiler's Location_CenterMassIntensity, MassDisplacement, Location_MaxIntensity,
IntegratedIntensity), from Σ q·a and Σ q·a·b over an object's pixels, 128-bit sums again, and an arg-max whose ties go to the first
pixel in raster order (``weighted_moments``; ``csrc/region_weighted.hip``: ``clx_region_weighted``; ``weighted_columns``); and the
sum, mean, standard deviation, minimum and maximum over the pixels that have a face neighbour outside the object (CellProfiler's
*IntensityEdge; ``border_intensity``; ``csrc/region_border.hip``: ``clx_region_border_intensity``, a stencil fused with the value
reduction; ``border_intensity_columns``).  With these the stage covers CellProfiler's MeasureObjectIntensity.

    python -m cellulus_amd.measure experiment.toml [--contacts] [--topology] [--hull] [--inscribed]
                                                   [--quantiles 0.25,0.5,0.75] [--mad]
                                                   [--texture] [--texture-levels 8] [--texture-distance 1]
                                                   [--radial] [--radial-rings 4] [--radial-width W] [--radial-wedges]
                                                   [--std] [--colocalization] [--coloc-threshold 0.15]
                                                   [--weighted] [--border-intensity]

writes ``measurements_bandwidth-<b>.csv`` next to ``evaluate``'s ``results_bandwidth-<b>.txt`` and, with ``--contacts``,
the boundary columns in it and ``contacts_bandwidth-<b>.csv`` beside it; ``--topology`` adds the topology columns,
``--hull`` the convex hull columns, ``--inscribed`` the inscribed circle / ball columns, ``--quantiles`` one
``intensity_q<q>_c<k>`` column per quantile and channel, ``--mad`` ``intensity_mad_c<k>``, ``--texture``
``texture_pairs_c<k>`` and the thirteen ``texture_<feature>_c<k>`` per channel (the range is per sample and channel),
``--radial`` ``radial_area_r<j>`` and per channel ``radial_mean_r<j>_c<k>``, ``radial_frac_r<j>_c<k>`` and
``radial_meanfrac_r<j>_c<k>`` for ``--radial-rings`` rings (relative to every object's inscribed radius, or ``--radial-width``
pixels wide from the boundary), ``--radial-wedges`` ``radial_cv_r<j>_c<k>`` too (2-D), ``--std`` ``intensity_std_c<k>`` per
channel and ``--colocalization`` the seven ``coloc_<quantity>_c<j>_c<k>`` per pair of channels, with ``--coloc-threshold`` the
fraction of an object's maximum from which a pixel counts for overlap, K1 / K2 and Manders, ``--weighted`` per channel
``intensity_sum_c<k>``, ``centroid_weighted_<a>_c<k>``, ``cov_weighted_<ab>_c<k>``, ``mass_displacement_c<k>`` and
``intensity_peak_<a>_c<k>``, and ``--border-intensity`` ``intensity_border_pixels`` and per channel
``intensity_border_{sum,mean,std,min,max}_c<k>``.
"""

import math
from fractions import Fraction

import numpy as np

from . import _clx

MAX_IDS = 1 << 24                       # clx_region_moments / clx_region_intensity: nid <= 2^24
MIN_CAPACITY, MAX_CAPACITY = 1 << 10, 1 << 28       # clx_region_contacts: slots of the pair table
_INFO_BAD_LABEL, _INFO_FULL = 1, 4      # bits of clx_region_contacts' info[0]
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
DIST_INF = 1 << 30                      # CLX_DIST_INF: a pixel of clx_label_distance_sq's map that has no candidate
_BAD_LABEL, _BAD_DISTANCE = 1, 2        # bits of clx_region_inscribed's bad[0]
MAX_QUANTILES = 16                      # two ranks each: clx_region_order_stats takes nq <= 32
_ORDER_BAD_LABEL, _ORDER_BAD_VALUE, _ORDER_BAD_AREA, _ORDER_BAD_RANK = 1, 2, 4, 8   # bits of clx_region_order_stats' bad[0]
MIN_LEVELS, MAX_LEVELS = 2, 32          # clx_region_cooccurrence: thirteen 32 x 32 int32 matrices are 52 KiB of LDS
MAX_TEXTURE_DISTANCE = 64
TEXTURE_TABLE_BYTES = 1 << 28           # the counts table of one clx_region_cooccurrence call stays below this
_TEXTURE_BAD_LABEL, _TEXTURE_BAD_VALUE = 1, 2       # bits of clx_region_cooccurrence's bad[0]
TEXTURE_FEATURES = ("asm", "contrast", "correlation", "variance", "idm", "sum_average", "sum_variance", "sum_entropy", "entropy",
                    "difference_variance", "difference_entropy", "info_correlation_1", "info_correlation_2")
_TEXTURE_INT64_MAX_T = 1 << 25          # texture_columns: numerators are below 2^12 T^2, so int64 holds them up to here
_TEXTURE_SLICE_CELLS = 1 << 22          # matrix cells texture_columns holds as float64 at a time
MAX_RINGS, MAX_RADIAL_WIDTH, RADIAL_WEDGES = 32, 32768, 8      # clx_region_radial: rings <= 32, width <= 2^15, 1 or 8 wedges
RADIAL_TABLE_BYTES = 1 << 28            # the count and isum tables of one clx_region_radial call stay below this together
_RADIAL_BAD_LABEL, _RADIAL_BAD_VALUE, _RADIAL_BAD_MAP, _RADIAL_BAD_ROW = 1, 2, 4, 8     # bits of clx_region_radial's bad[0]


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
_PRODUCTS_BAD_LABEL, _PRODUCTS_BAD_VALUE = 1, 2     # bits of clx_region_products' bad[0]


def product_table(words):
    """``clx_region_products``' rows (n, 20) of uint64 words as a dict: int64 arrays ``n, sum_a, sum_b, n_both, sum_a_above,
    sum_b_above, sum_a_both, sum_b_both`` and object arrays of Python ints ``sum_aa, sum_bb, sum_ab, sum_aa_both, sum_bb_both,
    sum_ab_both`` (a (lo, hi) pair is one signed 128-bit integer, two's complement)"""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, PRODUCT_WORDS)
    table = {name: np.ascontiguousarray(words[:, i]).view(np.int64) for i, name in enumerate(_PRODUCT_SUMS)}
    for i, name in enumerate(_PRODUCT_SQUARES):
        lo, hi = words[:, 8 + 2 * i].tolist(), words[:, 9 + 2 * i].tolist()
        table[name] = np.empty(len(lo), dtype=object)
        table[name][:] = [l + (h << 64) - ((h >> 63) << 128) for l, h in zip(lo, hi)]
    return table


def _signed_root(num, den):
    """``sign(num) * sqrt(num**2 / den)`` of Python ints, NaN where ``den == 0``: one correctly rounded operation"""
    if den == 0:
        return math.nan
    r = _sqrt_ratio(num * num, den)
    return -r if num < 0 else r


def _ratio(num, den):
    return num / den if den else math.nan


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
        c = np.array(values, dtype=np.float64).reshape(len(n))
        with np.errstate(over="ignore", under="ignore"):       # shifts at both clamps can leave float64's range
            return np.ldexp(c, exponent) if exponent else c

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
_WEIGHTED_BAD_LABEL, _WEIGHTED_BAD_VALUE = 1, 2     # bits of bad[0] of clx_region_weighted and clx_region_border_intensity


def _signed128(lo, hi):
    """Python ints of (lo, hi) uint64 word columns: signed 128-bit, two's complement"""
    out = np.empty(len(lo), dtype=object)
    out[:] = [l + (h << 64) - ((h >> 63) << 128) for l, h in zip(lo.tolist(), hi.tolist())]
    return out


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


def _scaled_column(values, n, exponent):
    c = np.array(values, dtype=np.float64).reshape(n)
    with np.errstate(over="ignore", under="ignore"):           # shifts at both clamps can leave float64's range
        return np.ldexp(c, exponent) if exponent else c


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


def _resolve_device(labels, device):
    import torch

    if torch.is_tensor(labels) and labels.is_cuda:
        device = labels.device
    elif device is None:
        if not torch.cuda.is_available():
            raise _clx.ClxError("measure needs a HIP device; cellulus_amd has no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _clx.ClxError(f"measure needs a HIP device, got {device}; cellulus_amd has no CPU path")
    return device


def _to_device_labels(labels, device, who="region_table"):
    import torch

    if torch.is_tensor(labels):
        if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dtype.is_complex:
            raise TypeError(f"{who}: labels must be integers, got {labels.dtype}")
        lab = labels.to(device)
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= MAX_IDS):
            raise ValueError(f"{who}: label ids must lie in [0, {MAX_IDS})")
        return lab.to(torch.int32).contiguous()
    labels = np.ascontiguousarray(labels)
    if labels.dtype.kind not in "ui":
        raise TypeError(f"{who}: labels must be integers, got {labels.dtype}")
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= MAX_IDS):
        raise ValueError(f"{who}: label ids must lie in [0, {MAX_IDS})")
    return torch.from_numpy(labels.astype(np.int32)).to(device)


def _to_device_raw(channel, device):
    import torch

    from .segment import _RAW_F32, _RAW_F64, _RAW_I32, _raw_to_device

    if not torch.is_tensor(channel):
        return _raw_to_device(channel, device)
    if channel.dtype == torch.float32:
        return channel.to(device).contiguous(), _RAW_F32
    if channel.dtype == torch.float64:
        return channel.to(device).contiguous(), _RAW_F64
    if channel.dtype.is_floating_point or channel.dtype.is_complex or channel.dtype == torch.bool:
        raise TypeError(f"region_table: unsupported raw dtype {channel.dtype}")
    c = channel.to(device)
    if c.numel() and (int(c.min()) < -2 ** 31 or int(c.max()) >= 2 ** 31):
        raise ValueError("region_table: integer raw values must fit in int32")
    return c.to(torch.int32).contiguous(), _RAW_I32


def _intensity(lab, raw_d, raw_type, nid, shift):
    """One clx_region_intensity call -> (isum int64 (nid), keys uint64 (nid, 2), bad)."""
    import torch

    dev = lab.device
    isum = torch.empty(nid, dtype=torch.int64, device=dev)
    vkey = torch.empty((nid, 2), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    _clx.call("clx_region_intensity", _clx.ptr(lab), _clx.ptr(raw_d), raw_type, lab.numel(), nid, int(shift),
              _clx.ptr(isum), _clx.ptr(vkey), _clx.ptr(bad), _clx.stream_ptr(dev))
    return isum.cpu().numpy(), vkey.cpu().numpy().view(np.uint64), int(bad.item())


def _channel_columns(lab, raw_d, raw_type, nid, present, area, k):
    """-> (the intensity columns of channel k, the shift its sums were quantised with)"""
    return _channel_columns_keys(lab, raw_d, raw_type, nid, present, area, k)[:2]


def _channel_columns_keys(lab, raw_d, raw_type, nid, present, area, k):
    """-> (the intensity columns of channel k, the shift its sums were quantised with, the largest order key of every id
    (uint64 (nid)): clx_region_weighted's peak_keys)"""
    from .segment import _RAW_I32, _decode_keys
    from .utils.otsu import minmax_on_device

    npix = lab.numel()
    shift = 0
    if raw_type != _RAW_I32:
        lo, hi = minmax_on_device(raw_d.reshape(-1))
        max_abs = max(abs(lo), abs(hi))
        if not math.isfinite(max_abs):
            # something outside the objects is not finite: take the maximum under the objects from the keys of a first
            # call whose scale lets every finite value pass
            _, keys, bad = _intensity(lab, raw_d, raw_type, nid, _SHIFT_MIN)
            if bad & 2:
                raise ValueError(f"region_table: raw channel {k} has non-finite values inside objects")
            vals = _decode_keys(keys[present], raw_type).astype(np.float64)
            max_abs = float(np.abs(vals).max()) if vals.size else 0.0
        shift = intensity_shift(max_abs, npix)
    isum, keys, bad = _intensity(lab, raw_d, raw_type, nid, shift)
    if bad & 2:
        raise ValueError(f"region_table: raw channel {k} has non-finite values inside objects")
    if bad & 1:
        raise ValueError("region_table: label ids changed under the measurement")
    vals = _decode_keys(keys[present], raw_type)
    mean = _exact_div(isum[present].astype(object), area[present].astype(object))
    if shift:
        mean = np.ldexp(mean, -shift)
    return ({f"intensity_mean_c{k}": mean, f"intensity_min_c{k}": vals[:, 0].copy(), f"intensity_max_c{k}": vals[:, 1].copy()}, shift,
            np.ascontiguousarray(keys[:, 1]))


def _labels_on_device(labels, device, who):
    """-> (int32 device tensor, device, nd, spatial, nid) after the type and range checks every entry point shares;
    `who` names the caller in their messages"""
    device = _resolve_device(labels, device)
    nd = labels.ndim
    if nd not in (2, 3):
        raise ValueError(f"{who}: labels must be 2-D or 3-D, got {nd} dimensions")
    spatial = tuple(int(v) for v in labels.shape)
    lab = _to_device_labels(labels, device, who)
    _clx.require_device(lab, "labels")
    nid = int(lab.max().item()) + 1 if lab.numel() else 1
    return lab, device, nd, spatial, nid


def _moments(lab, Z, Y, X, nid, who):
    """one clx_region_moments call -> (area, bbox, sum1, sum2) left on the device"""
    import torch

    device = lab.device
    area_d = torch.empty(nid, dtype=torch.int64, device=device)
    bbox_d = torch.empty((nid, 6), dtype=torch.int32, device=device)
    sum1_d = torch.empty((nid, 3), dtype=torch.int64, device=device)
    sum2_d = torch.empty((nid, 6), dtype=torch.int64, device=device)
    bad_d = torch.empty(1, dtype=torch.int32, device=device)
    _clx.call("clx_region_moments", _clx.ptr(lab), Z, Y, X, nid, _clx.ptr(area_d), _clx.ptr(bbox_d),
              _clx.ptr(sum1_d), _clx.ptr(sum2_d), _clx.ptr(bad_d), _clx.stream_ptr(device))
    if int(bad_d.item()):
        raise ValueError(f"{who}: label ids must lie in [0, {MAX_IDS})")
    return area_d, bbox_d, sum1_d, sum2_d


def _pair_capacity(objects):
    """power of two, at least 8 x the object count (an object of a tissue has about six neighbours, so about four
    pairs with the background's: the table stays below half full) and at least MIN_CAPACITY"""
    return max(MIN_CAPACITY, 1 << max(0, 8 * int(objects) - 1).bit_length())


def _contacts(lab, nd, spatial, nid, objects, who):
    """clx_region_contacts, repeated with twice the table while it reports a pair it could not place
    -> (a, b, faces) int64, sorted by (a, b).  `objects`: the object count or a bound on it, which sizes the first table"""
    import torch

    device = lab.device
    Z, Y, X = (1,) * (3 - nd) + tuple(spatial)
    capacity = _pair_capacity(objects)
    while True:
        if capacity > MAX_CAPACITY:
            raise ValueError(f"{who}: more id pairs than a table of {MAX_CAPACITY} slots holds")
        keys = torch.empty(capacity, dtype=torch.int64, device=device)
        counts = torch.empty(capacity, dtype=torch.int64, device=device)
        info = torch.empty(2, dtype=torch.int32, device=device)
        _clx.call("clx_region_contacts", _clx.ptr(lab), nd, Z, Y, X, nid, capacity, _clx.ptr(keys), _clx.ptr(counts),
                  _clx.ptr(info), _clx.stream_ptr(device))
        flags, used = info.tolist()
        if flags & _INFO_BAD_LABEL:
            raise ValueError(f"{who}: label ids must lie in [0, {MAX_IDS})")
        if not flags & _INFO_FULL:
            break
        capacity *= 2
    slot = torch.nonzero(keys).reshape(-1)
    assert slot.numel() == used
    k = keys[slot].cpu().numpy()
    order = np.argsort(k, kind="stable")                     # keys are (a << 32) | b with a < 2^24: the (a, b) order
    k = k[order]
    return k >> 32, k & 0xFFFFFFFF, counts[slot].cpu().numpy()[order]


def contact_pairs(labels, device=None):
    """The faces between pixels of different ids of ``labels`` (2-D or 3-D integers, array or device tensor; the same
    types and range as ``region_table``), connectivity 1, the outside of the image counting as id 0: ``(a, b, faces)``
    int64 arrays, one row per pair with ``a < b``, sorted by ``(a, b)``.  Rows with ``a == 0`` are an object's faces to
    the background and the image edge; the others are the region adjacency graph with the size of every contact.
    Runs on a HIP device; there is no CPU path."""
    lab, device, nd, spatial, nid = _labels_on_device(labels, device, "contact_pairs")
    if nid == 1:                                             # no pixel, or background only: no object, no pair
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    # the first table is sized without another pass over the map: neither the largest id nor the pixel count is below
    # the object count
    return _contacts(lab, nd, spatial, nid, min(nid - 1, lab.numel()), "contact_pairs")


def _perimeter_classes(lab, Y, X, nid):
    import torch

    classes = torch.empty((nid, 4), dtype=torch.int64, device=lab.device)
    bad = torch.empty(1, dtype=torch.int32, device=lab.device)
    _clx.call("clx_region_perimeter", _clx.ptr(lab), Y, X, nid, _clx.ptr(classes), _clx.ptr(bad), _clx.stream_ptr(lab.device))
    if int(bad.item()):
        raise ValueError(f"region_table: label ids must lie in [0, {MAX_IDS})")
    return classes.cpu().numpy()


def _topology_counts(lab, nd, Z, Y, X, nid):
    import torch

    counts = torch.empty((nid, 5), dtype=torch.int64, device=lab.device)
    bad = torch.empty(1, dtype=torch.int32, device=lab.device)
    _clx.call("clx_region_topology", _clx.ptr(lab), nd, Z, Y, X, nid, _clx.ptr(counts), _clx.ptr(bad), _clx.stream_ptr(lab.device))
    if int(bad.item()):
        raise ValueError(f"region_table: label ids must lie in [0, {MAX_IDS})")
    return counts.cpu().numpy()


def _hull_rows(lab, nd, Z, Y, X, nid, bbox_d, bbox, present):
    """one clx_region_hull call on clx_region_moments' bounding boxes (bbox_d on the device, bbox: its host copy)
    -> hull int64 (nid, 5)"""
    import torch

    device = lab.device
    box = bbox[present].astype(np.int64)
    nrows = np.zeros(nid, dtype=np.int64)
    nrows[present] = (box[:, 3] - box[:, 0] + 1) * (box[:, 4] - box[:, 1] + 1)
    row_base = np.cumsum(nrows) - nrows                      # exclusive; absent ids have no rows
    rows = int(nrows.sum())
    nbytes = int(_clx.load().clx_region_hull_workspace(rows))
    if nbytes == 0:
        raise ValueError("region_table: too many bounding-box rows for clx_region_hull")
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
    row_base_d = torch.from_numpy(row_base).to(device)
    hull = torch.empty((nid, 5), dtype=torch.int64, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    _clx.call("clx_region_hull", _clx.ptr(lab), nd, Z, Y, X, nid, _clx.ptr(bbox_d), _clx.ptr(row_base_d), rows,
              _clx.ptr(workspace), nbytes, _clx.ptr(hull), _clx.ptr(bad), _clx.stream_ptr(device))
    flags = int(bad.item())
    if flags & 1:
        raise ValueError(f"region_table: label ids must lie in [0, {MAX_IDS})")
    if flags & 2:
        raise ValueError("region_table: label ids changed under the measurement")
    return hull.cpu().numpy()


def _distance_map(lab, nd, Z, Y, X, edge):
    """one clx_label_distance_sq call -> int32 device tensor, flat"""
    import torch

    device = lab.device
    npix = lab.numel()
    nbytes = int(_clx.load().clx_label_distance_workspace(npix))
    if nbytes == 0:
        raise ValueError("label_distance_sq: the map must have fewer than 2^32 pixels")
    dist = torch.empty(npix, dtype=torch.int32, device=device)
    workspace = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
    _clx.call("clx_label_distance_sq", _clx.ptr(lab), nd, Z, Y, X, int(bool(edge)), _clx.ptr(dist), _clx.ptr(workspace), nbytes,
              _clx.stream_ptr(device))
    return dist


def label_distance_sq(labels, edge=False, device=None):
    """For every pixel of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as
    ``region_table``) that belongs to an object the squared Euclidean distance, an exact integer, to the nearest pixel that
    carries ANOTHER value, another object or the background alike; 0 on background.  Inside object ``i`` this is
    ``scipy.ndimage.distance_transform_edt(labels == i) ** 2``, for every ``i`` at once: the input of a seeded watershed,
    of skeletons, of an erosion that does not merge neighbours.  ``edge=False``: only pixels of the map count (scipy's
    convention; a map that is one object everywhere has no candidate and gives ``DIST_INF``).  ``edge=True``: the map
    counts as padded with one layer of background.  Returns the int32 DEVICE tensor in the shape of ``labels``.
    Runs on a HIP device; there is no CPU path."""
    import torch

    lab, device, nd, spatial, _ = _labels_on_device(labels, device, "label_distance_sq")
    if lab.numel() == 0:
        return torch.empty(spatial, dtype=torch.int32, device=device)
    Z, Y, X = (1,) * (3 - nd) + spatial
    return _distance_map(lab, nd, Z, Y, X, edge).reshape(spatial)


def _inscribed_rows(lab, nd, Z, Y, X, nid, edge):
    """clx_label_distance_sq, then clx_region_inscribed on its map -> (the map, flat int32; the rows, int64 (nid, 3)), both
    left on the device"""
    import torch

    device = lab.device
    dist = _distance_map(lab, nd, Z, Y, X, edge)
    out = torch.empty((nid, 3), dtype=torch.int64, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    _clx.call("clx_region_inscribed", _clx.ptr(lab), _clx.ptr(dist), lab.numel(), nid, _clx.ptr(out), _clx.ptr(bad),
              _clx.stream_ptr(device))
    flags = int(bad.item())
    if flags & _BAD_LABEL:
        raise ValueError(f"region_table: label ids must lie in [0, {MAX_IDS})")
    if flags & _BAD_DISTANCE:
        raise ValueError("region_table: the distance map changed under the measurement")
    return dist, out


def _order_keys(lab, raw_d, raw_type, nid, area_d, seg_base_d, total, centre_d, rank_d, workspace, nbytes, k):
    """one clx_region_order_stats call -> uint64 keys (nid, nq) on the host"""
    import torch

    device = lab.device
    nq = rank_d.shape[1]
    out = torch.empty((nid, nq), dtype=torch.int64, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    _clx.call("clx_region_order_stats", _clx.ptr(lab), _clx.ptr(raw_d), raw_type, lab.numel(), nid, _clx.ptr(area_d),
              _clx.ptr(seg_base_d), total, _clx.ptr(centre_d), _clx.ptr(rank_d), nq, _clx.ptr(out), _clx.ptr(workspace), nbytes,
              _clx.ptr(bad), _clx.stream_ptr(device))
    flags = int(bad.item())
    if flags & _ORDER_BAD_VALUE:
        raise ValueError(f"region_table: raw channel {k} has non-finite values inside objects")
    if flags & (_ORDER_BAD_LABEL | _ORDER_BAD_AREA):
        raise ValueError("region_table: label ids changed under the measurement")
    if flags & _ORDER_BAD_RANK:
        raise RuntimeError("region_table: internal error: a rank at or above its object's area reached clx_region_order_stats")
    return out.cpu().numpy().view(np.uint64)


def _order_columns(lab, channels, nid, present, area, area_d, quantiles, mad):
    """the quantile and MAD columns of every channel: one clx_region_order_stats call per channel for all quantiles (two
    ranks each, and the median's where ``mad`` needs them; a second call where that makes more than 32 ranks), and one with
    the medians as ``centre`` for the MAD.
    channels: [(raw_d, raw_type)]; area: the host copy of area_d with area[0] = 0"""
    import torch

    from .segment import _RAW_F64, _decode_keys

    device = lab.device
    names = [f"intensity_q{float(q)!r}" for q in quantiles]
    cols = {}
    if not len(present):
        for k in range(len(channels)):
            cols.update({f"{n}_c{k}": np.zeros(0) for n in names})
            if mad:
                cols[f"intensity_mad_c{k}"] = np.zeros(0)
        return cols
    needed = list(quantiles) + ([0.5] if mad and 0.5 not in quantiles else [])
    nq = 2 * len(needed)
    rank = np.zeros((nid, nq), dtype=np.int64)
    weights = []
    for j, q in enumerate(needed):
        lo, hi, t = quantile_ranks(area[present], q)
        rank[present, 2 * j], rank[present, 2 * j + 1] = lo, hi
        weights.append(t)
    seg_base = np.cumsum(area) - area                        # exclusive; absent ids (and row 0) take no pixels
    total = int(area.sum())
    nbytes = int(_clx.load().clx_region_order_workspace(total, nid))
    if nbytes == 0:
        raise ValueError("region_table: too many object pixels for clx_region_order_stats")
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)         # reused by every call
    seg_base_d = torch.from_numpy(seg_base.astype(np.int64)).to(device)
    rank_d = torch.from_numpy(rank).to(device)
    if mad:
        m = needed.index(0.5)
        mad_rank_d = rank_d[:, 2 * m:2 * m + 2].contiguous()
    # 16 quantiles without 0.5 and the MAD's median are 17 pairs of ranks: more than one call takes
    pairs = 2 * MAX_QUANTILES
    rank_calls = [rank_d[:, c:c + pairs].contiguous() for c in range(0, nq, pairs)]
    for k, (raw_d, raw_type) in enumerate(channels):
        keys = np.concatenate([_order_keys(lab, raw_d, raw_type, nid, area_d, seg_base_d, total, None, r, workspace, nbytes, k)
                               for r in rank_calls], axis=1)
        vals = _decode_keys(keys[present], raw_type)
        columns = [quantile_columns(vals[:, 2 * j], vals[:, 2 * j + 1], weights[j]) for j in range(len(needed))]
        for n, c in zip(names, columns):
            cols[f"{n}_c{k}"] = c
        if mad:
            centre = np.zeros(nid, dtype=np.float64)
            centre[present] = columns[m]
            keys = _order_keys(lab, raw_d, raw_type, nid, area_d, seg_base_d, total, torch.from_numpy(centre).to(device),
                               mad_rank_d, workspace, nbytes, k)
            dev = _decode_keys(keys[present], _RAW_F64)
            cols[f"intensity_mad_c{k}"] = quantile_columns(dev[:, 0], dev[:, 1], weights[m])
    return cols


def _cooccurrence_counts(lab, raw_d, raw_type, nd, Z, Y, X, nid, bbox_d, ids, area, lo, hi, levels, distance, k, who):
    """clx_region_cooccurrence for the objects ``ids`` (host int64, any order), in chunks of them whose counts table stays
    below TEXTURE_TABLE_BYTES -> counts int64 (len(ids), ndir, levels, levels).  area: the host areas by id, against which
    the pixels every call saw are checked"""
    import torch

    device = lab.device
    ndir = 4 if nd == 2 else 13
    row_bytes = ndir * levels * levels * 4
    step = max(1, TEXTURE_TABLE_BYTES // row_bytes)
    out = np.empty((len(ids), ndir, levels, levels), dtype=np.int64)
    workspace, have = None, 0
    for a in range(0, len(ids), step):
        chunk = np.asarray(ids[a:a + step], dtype=np.int64)
        nrows = len(chunk)
        nbytes = int(_clx.load().clx_region_cooccurrence_workspace(lab.numel(), nrows))
        if nbytes == 0:
            raise ValueError(f"{who}: the map must have fewer than 2^31 pixels for the texture columns")
        if nbytes > have:
            workspace, have = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device), nbytes
        ids_d = torch.from_numpy(chunk.astype(np.int32)).to(device)
        counts = torch.empty((nrows, ndir, levels, levels), dtype=torch.int32, device=device)
        seen = torch.empty(nrows, dtype=torch.int64, device=device)
        bad = torch.empty(1, dtype=torch.int32, device=device)
        _clx.call("clx_region_cooccurrence", _clx.ptr(lab), _clx.ptr(raw_d), raw_type, nd, Z, Y, X, nid, _clx.ptr(bbox_d),
                  _clx.ptr(ids_d), nrows, float(lo), float(hi), levels, distance, _clx.ptr(counts), _clx.ptr(seen), _clx.ptr(bad),
                  _clx.ptr(workspace), nbytes, _clx.stream_ptr(device))
        flags = int(bad.item())
        if flags & _TEXTURE_BAD_VALUE:
            raise ValueError(f"{who}: raw channel {k} has non-finite values inside objects")
        if flags & _TEXTURE_BAD_LABEL or not np.array_equal(seen.cpu().numpy(), area[chunk]):
            raise ValueError(f"{who}: label ids changed under the measurement")
        out[a:a + nrows] = counts.cpu().numpy()
    return out


def _texture_columns_of(lab, channels, nd, Z, Y, X, nid, bbox_d, present, area, cols, levels, distance, value_range):
    """the texture columns of every channel; channels: [(raw_d, raw_type)]; cols: the table so far, whose
    intensity_min / _max columns give the range where none is given"""
    out = {}
    for k, (raw_d, raw_type) in enumerate(channels):
        if len(present):
            lo, hi = value_range or (float(cols[f"intensity_min_c{k}"].min()), float(cols[f"intensity_max_c{k}"].max()))
            counts = _cooccurrence_counts(lab, raw_d, raw_type, nd, Z, Y, X, nid, bbox_d, present, area, lo, hi, levels, distance, k,
                                          "region_table")
        else:
            counts = np.zeros((0, 4 if nd == 2 else 13, levels, levels), dtype=np.int64)
        t = texture_columns(counts, nd)
        out[f"texture_pairs_c{k}"] = t.pop("pairs")
        out.update({f"texture_{name}_c{k}": column for name, column in t.items()})
    return out


def cooccurrence(labels, raw, levels=8, distance=1, value_range=None, device=None):
    """The grey-level co-occurrence matrices of every object of ``labels`` (2-D or 3-D integers, array or device tensor; the
    same types and range as ``region_table``) in ONE raw channel ``raw`` (the shape of ``labels``; float32, float64 or
    integers that fit int32): ``(ids, counts)``, ``ids`` int64 (n) the objects present, ascending, ``counts`` int64
    (n, ndir, levels, levels).  ``counts[r, k, a, b]`` is the number of pixels ``p`` of ``ids[r]`` at level ``a`` whose
    partner ``p + distance * texture_directions(nd)[k]`` lies inside the map, carries the same id and is at level ``b``:
    ordered pairs, not symmetrised, no wrap across the map's ends (``texture_columns`` forms ``C + Cᵀ``).
    ``level(v) = min(levels - 1, max(0, floor((float64(v) - lo) / (hi - lo) * levels)))`` with ``2 <= levels <= 32``; ``hi ==
    lo`` puts every pixel at level 0.  ``value_range=(lo, hi)``; ``None`` takes the smallest and the largest value under
    the objects of this map, so the levels are relative to this image's objects.  ``1 <= distance <= 64``.
    This is the door to the matrices for per-direction features; ``region_table(texture=True)`` has their means.
    Runs on a HIP device; there is no CPU path."""
    who = "cooccurrence"
    levels, distance, value_range = _check_texture(levels, distance, value_range, who)
    lab, device, nd, spatial, nid = _labels_on_device(labels, device, who)
    ndir = 4 if nd == 2 else 13
    if tuple(raw.shape) != spatial:
        raise ValueError(f"{who}: raw has shape {tuple(raw.shape)}, labels {spatial}: one channel in the shape of labels")
    empty = np.zeros(0, dtype=np.int64), np.zeros((0, ndir, levels, levels), dtype=np.int64)
    if lab.numel() == 0 or nid == 1:
        return empty
    Z, Y, X = (1,) * (3 - nd) + spatial
    area_d, bbox_d, _, _ = _moments(lab, Z, Y, X, nid, who)
    area = area_d.cpu().numpy()
    area[0] = 0
    present = np.flatnonzero(area > 0)
    if not len(present):
        return empty
    raw_d, raw_type = _to_device_raw(raw, device)
    raw_d = raw_d.reshape(-1)
    if value_range is None:
        c, _ = _channel_columns(lab.reshape(-1), raw_d, raw_type, nid, present, area, 0)
        value_range = float(c["intensity_min_c0"].min()), float(c["intensity_max_c0"].max())
    counts = _cooccurrence_counts(lab, raw_d, raw_type, nd, Z, Y, X, nid, bbox_d, present, area, *value_range, levels, distance, 0, who)
    return present.astype(np.int64), counts


def _radial_tables(lab, dist, inscribed_d, channels, nd, Z, Y, X, nid, ids, area, rings, width, wedges, who):
    """clx_region_radial for the objects ``ids`` (host int64, any order) on the distance map ``dist`` and
    clx_region_inscribed's rows ``inscribed_d`` (both on the device), in chunks of objects whose two tables stay below
    RADIAL_TABLE_BYTES together; one call per chunk and channel, one without a channel where there is none
    -> (count int64 (len(ids), rings, wedges), [isum int64 of the same shape per channel]).
    channels: [(raw_d, raw_type, shift)]; width 0: relative rings; area: the host areas by id, against which the pixels
    every call counted are checked"""
    import torch

    device = lab.device
    n = len(ids)
    step = max(1, RADIAL_TABLE_BYTES // (rings * wedges * 16))
    count = np.empty((n, rings, wedges), dtype=np.int64)
    isums = [np.empty((n, rings, wedges), dtype=np.int64) for _ in channels]
    for a in range(0, n, step):
        chunk = np.asarray(ids[a:a + step], dtype=np.int64)
        nrows = len(chunk)
        row = np.full(nid, -1, dtype=np.int32)
        row[chunk] = np.arange(nrows, dtype=np.int32)
        row_d = torch.from_numpy(row).to(device)
        count_d = torch.empty((nrows, rings, wedges), dtype=torch.int64, device=device)
        isum_d = torch.empty((nrows, rings, wedges), dtype=torch.int64, device=device) if channels else None
        bad = torch.empty(1, dtype=torch.int32, device=device)
        for k, (raw_d, raw_type, shift) in enumerate(channels or [(None, 0, 0)]):
            _clx.call("clx_region_radial", _clx.ptr(lab), _clx.ptr(dist), _clx.ptr(raw_d), raw_type, nd, Z, Y, X, nid,
                      _clx.ptr(inscribed_d), _clx.ptr(row_d), nrows, rings, width, wedges, int(shift), _clx.ptr(count_d),
                      _clx.ptr(isum_d), _clx.ptr(bad), _clx.stream_ptr(device))
            flags = int(bad.item())
            if flags & _RADIAL_BAD_VALUE:
                raise ValueError(f"{who}: raw channel {k} has non-finite values inside objects")
            if flags & _RADIAL_BAD_MAP:
                raise ValueError(f"{who}: the distance map changed under the measurement")
            got = count_d.cpu().numpy()
            if flags & (_RADIAL_BAD_LABEL | _RADIAL_BAD_ROW) or not np.array_equal(got.sum(axis=(1, 2)), area[chunk]):
                raise ValueError(f"{who}: label ids changed under the measurement")
            count[a:a + nrows] = got
            if raw_d is not None:
                isums[k][a:a + nrows] = isum_d.cpu().numpy()
    return count, isums


def _raw_channels(raw, spatial, who):
    """``raw`` as (C, *spatial): one channel in the shape of the labels gets its leading axis"""
    if tuple(raw.shape) == spatial:
        raw = raw[None]
    if tuple(raw.shape[1:]) != spatial:
        raise ValueError(f"{who}: raw has shape {tuple(raw.shape)}, labels {spatial}")
    return raw


def radial_distribution(labels, raw=None, rings=4, width=None, wedges=False, edge=False, device=None):
    """The radial distribution of every object of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and
    range as ``region_table``) as integer tables: ``(ids, count, isum, shift)``.  ``ids`` int64 (n): the objects present,
    ascending.  ``count`` int64 (n, rings, W): the pixels of ``ids[r]`` in ring j and wedge o.  ``isum``: per channel of ``raw``
    (``None``, ``(*spatial)`` or ``(C, *spatial)``; float32, float64 or integers that fit int32) an int64 (n, rings, W) with the
    sums of ``q = rint(v * 2**shift[k])`` over those pixels; ``shift``: per channel the scale ``region_table`` uses for its
    ``intensity_mean`` (``intensity_shift``; 0 for integers).  Both lists are empty without ``raw``.
    Ring: with ``d2`` the pixel's ``label_distance_sq`` (``edge`` is that function's) and ``D2`` its object's largest,
    ``width=None`` takes the smallest j with ``d2 * rings**2 <= (j + 1)**2 * D2``: rings of equal width in units of the
    object's inscribed radius, ring 0 the rim and ring ``rings - 1`` the core; ``width`` in 1 .. 32768 the smallest j with
    ``d2 <= ((j + 1) * width)**2``, at most ``rings - 1``: bands of ``width`` pixels from the boundary.  ``1 <= rings <= 32``.
    Wedge: ``wedges=False``: W = 1.  ``wedges=True`` (2-D): W = 8 sectors of 45 degrees around the object's inscribed centre
    (the first pixel in raster order that attains D2), wedge o holding ``o * 45 <= atan2(dy, dx) < (o + 1) * 45`` degrees.
    Every number is an exact integer and the same in every run; the tables do not depend on RADIAL_TABLE_BYTES, which only
    bounds what one call holds.  ``radial_columns`` forms ``region_table``'s columns of them.
    Runs on a HIP device; there is no CPU path."""
    who = "radial_distribution"
    rings, width, W = _check_radial(rings, width, wedges, getattr(labels, "ndim", None), who)
    lab, device, nd, spatial, nid = _labels_on_device(labels, device, who)
    if raw is not None:
        raw = _raw_channels(raw, spatial, who)
    nch = 0 if raw is None else raw.shape[0]
    empty = (np.zeros(0, dtype=np.int64), np.zeros((0, rings, W), dtype=np.int64),
             [np.zeros((0, rings, W), dtype=np.int64) for _ in range(nch)], [0] * nch)
    if lab.numel() == 0 or nid == 1:
        return empty
    Z, Y, X = (1,) * (3 - nd) + spatial
    area_d, _, _, _ = _moments(lab, Z, Y, X, nid, who)
    area = area_d.cpu().numpy()
    area[0] = 0
    present = np.flatnonzero(area > 0)
    if not len(present):
        return empty
    flat = lab.reshape(-1)
    channels = []
    for k in range(nch):
        raw_d, raw_type = _to_device_raw(raw[k], device)
        _, shift = _channel_columns(flat, raw_d.reshape(-1), raw_type, nid, present, area, k)
        channels.append((raw_d.reshape(-1), raw_type, shift))
    dist, inscribed_d = _inscribed_rows(flat, nd, Z, Y, X, nid, edge)
    count, isums = _radial_tables(flat, dist, inscribed_d, channels, nd, Z, Y, X, nid, present, area, rings, width, W, who)
    return present.astype(np.int64), count, isums, [c[2] for c in channels]


def _products_rows(lab, chan_a, chan_b, nid, shift_a, shift_b, thr_a, thr_b, area, present, who, j, k):
    """one clx_region_products call -> product_table of the present ids.  chan_*: (raw_d, raw_type); thr_*: int64 host arrays
    (nid) or None, both or neither; area: the host areas by id, against which the pixels the call counted are checked"""
    import torch

    device = lab.device
    if chan_a[1] != chan_b[1]:
        raise ValueError(f"{who}: raw channels {j} and {k} differ in type")
    out = torch.empty((nid, PRODUCT_WORDS), dtype=torch.int64, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    thr_a_d = None if thr_a is None else torch.from_numpy(np.ascontiguousarray(thr_a, dtype=np.int64)).to(device)
    thr_b_d = None if thr_b is None else torch.from_numpy(np.ascontiguousarray(thr_b, dtype=np.int64)).to(device)
    _clx.call("clx_region_products", _clx.ptr(lab), _clx.ptr(chan_a[0]), _clx.ptr(chan_b[0]), chan_a[1], lab.numel(), nid,
              int(shift_a), int(shift_b), _clx.ptr(thr_a_d), _clx.ptr(thr_b_d), _clx.ptr(out), _clx.ptr(bad), _clx.stream_ptr(device))
    flags = int(bad.item())
    if flags & _PRODUCTS_BAD_VALUE:
        raise ValueError(f"{who}: raw channel {j} or {k} has non-finite values inside objects")
    words = out.cpu().numpy().view(np.uint64)
    if flags & _PRODUCTS_BAD_LABEL or not np.array_equal(words[present, 0].view(np.int64), area[present]):
        raise ValueError(f"{who}: label ids changed under the measurement")
    return product_table(words[present])


def _channel_thresholds(qmax, f, nid, present):
    thr = np.zeros(nid, dtype=np.int64)
    thr[present] = coloc_thresholds(qmax, f)
    return thr


def _products_columns_of(lab, channels, shifts, nid, present, area, cols, std, colocalization, f):
    """the std and colocalization columns; channels: [(raw_d, raw_type)]; cols: the table so far, whose intensity_max columns
    give the thresholds.  One clx_region_products call per pair j < k; a channel that no pair covers (no colocalization) takes
    one with a == b and no thresholds for its std"""
    nch = len(channels)
    pairs = [(j, k) for j in range(nch) for k in range(j + 1, nch)] if colocalization else []
    out_std, out_coloc = {}, {}
    if not len(present):
        empty = product_table(np.zeros((0, PRODUCT_WORDS), dtype=np.uint64))
        for k in range(nch if std else 0):
            out_std.update(products_columns(empty, j=k, k=k, std=True, colocalization=False))
        for j, k in pairs:
            out_coloc.update(products_columns(empty, j=j, k=k))
        return {**out_std, **out_coloc}
    thr = {}
    for j, k in pairs:
        for c in (j, k):
            if c not in thr:
                thr[c] = _channel_thresholds(quantised(cols[f"intensity_max_c{c}"], shifts[c]), f, nid, present)
        table = _products_rows(lab, channels[j], channels[k], nid, shifts[j], shifts[k], thr[j], thr[k], area, present, "region_table", j, k)
        got = products_columns(table, shifts[j], shifts[k], j, k, std=std, colocalization=True)
        for name in [n for n in got if n.startswith("intensity_std_")]:
            out_std.setdefault(name, got.pop(name))
        out_coloc.update(got)
    for k in range(nch if std and not pairs else 0):
        table = _products_rows(lab, channels[k], channels[k], nid, shifts[k], shifts[k], None, None, area, present, "region_table", k, k)
        out_std.update(products_columns(table, shifts[k], shifts[k], k, k, std=True, colocalization=False))
    return {**{f"intensity_std_c{k}": out_std[f"intensity_std_c{k}"] for k in range(nch if std else 0)}, **out_coloc}


def channel_products(labels, raw, j=0, k=1, threshold=None, device=None):
    """The sums of products of channels ``j`` and ``k`` of ``raw`` (``(*spatial)`` or ``(C, *spatial)``; float32, float64 or
    integers that fit int32) inside every object of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and
    range as ``region_table``): ``(ids, table, shift_j, shift_k)``.  ``ids`` int64 (n): the objects present, ascending.
    ``table``: ``product_table``'s dict of ``clx_region_products``' twenty words per object, exact integers of
    ``q = rint(v * 2**shift)`` with the scales ``region_table`` uses for its ``intensity_mean`` (``intensity_shift``; 0 for
    integers): int64 arrays ``n, sum_a, sum_b, n_both, sum_a_above, sum_b_above, sum_a_both, sum_b_both`` and object arrays of
    Python ints ``sum_aa, sum_bb, sum_ab, sum_aa_both, sum_bb_both, sum_ab_both`` (a is channel j, b channel k; ``j == k`` is
    allowed).  ``threshold=None``: every pixel counts as above, the conditioned sums equal the others; a float ``f`` in [0, 1]:
    a pixel of object i is above in a channel where ``q >= ceil(f * qmax_i)``, ``qmax_i`` the object's quantised maximum in that
    channel (``coloc_thresholds``).  ``products_columns`` forms ``region_table``'s columns of the table.
    Runs on a HIP device; there is no CPU path."""
    who = "channel_products"
    f = None if threshold is None else _check_products(False, False, threshold, labels, raw, who)
    if raw is None:
        raise ValueError(f"{who}: raw is needed")
    raw = _raw_channels(raw, tuple(int(v) for v in labels.shape), who)
    j, k = int(j), int(k)
    if not (0 <= j < raw.shape[0] and 0 <= k < raw.shape[0]):
        raise ValueError(f"{who}: channels j = {j} and k = {k} must lie in [0, {raw.shape[0]})")
    lab, device, nd, spatial, nid = _labels_on_device(labels, device, who)
    empty = np.zeros(0, dtype=np.int64), product_table(np.zeros((0, PRODUCT_WORDS), dtype=np.uint64)), 0, 0
    if lab.numel() == 0 or nid == 1:
        return empty
    Z, Y, X = (1,) * (3 - nd) + spatial
    area_d, _, _, _ = _moments(lab, Z, Y, X, nid, who)
    area = area_d.cpu().numpy()
    area[0] = 0
    present = np.flatnonzero(area > 0)
    if not len(present):
        return empty
    flat = lab.reshape(-1)
    chans, shifts, thr = {}, {}, {}
    for c in sorted({j, k}):
        raw_d, raw_type = _to_device_raw(raw[c], device)
        chans[c] = (raw_d.reshape(-1), raw_type)
        columns, shifts[c] = _channel_columns(flat, chans[c][0], raw_type, nid, present, area, c)
        thr[c] = None if f is None else _channel_thresholds(quantised(columns[f"intensity_max_c{c}"], shifts[c]), f, nid, present)
    table = _products_rows(flat, chans[j], chans[k], nid, shifts[j], shifts[k], thr[j], thr[k], area, present, who, j, k)
    return present.astype(np.int64), table, shifts[j], shifts[k]


def _weighted_rows(lab, raw_d, raw_type, Z, Y, X, nid, shift, peak_keys, area, present, who, k):
    """one clx_region_weighted call -> weighted_table of the present ids.  peak_keys: uint64 host array (nid), clx_region_intensity's
    largest keys; area: the host areas by id, against which the pixels the call counted are checked"""
    import torch

    device = lab.device
    out = torch.empty((nid, WEIGHTED_WORDS), dtype=torch.int64, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    keys_d = torch.from_numpy(np.ascontiguousarray(peak_keys, dtype=np.uint64).view(np.int64)).to(device)
    _clx.call("clx_region_weighted", _clx.ptr(lab), _clx.ptr(raw_d), raw_type, Z, Y, X, nid, int(shift), _clx.ptr(keys_d),
              _clx.ptr(out), _clx.ptr(bad), _clx.stream_ptr(device))
    flags = int(bad.item())
    if flags & _WEIGHTED_BAD_VALUE:
        raise ValueError(f"{who}: raw channel {k} has non-finite values inside objects")
    words = out.cpu().numpy().view(np.uint64)
    if flags & _WEIGHTED_BAD_LABEL or not np.array_equal(words[present, 0].view(np.int64), area[present]):
        raise ValueError(f"{who}: label ids changed under the measurement")
    return weighted_table(words[present])


def _border_rows(lab, raw_d, raw_type, nd, Z, Y, X, nid, shift, area, present, who, k):
    """one clx_region_border_intensity call -> border_table of the present ids; area: the host areas by id, which bound the
    border pixels of every object from above (and 1 bounds them from below)"""
    import torch

    device = lab.device
    out = torch.empty((nid, BORDER_WORDS), dtype=torch.int64, device=device)
    bad = torch.empty(1, dtype=torch.int32, device=device)
    _clx.call("clx_region_border_intensity", _clx.ptr(lab), _clx.ptr(raw_d), raw_type, nd, Z, Y, X, nid, int(shift), _clx.ptr(out),
              _clx.ptr(bad), _clx.stream_ptr(device))
    flags = int(bad.item())
    if flags & _WEIGHTED_BAD_VALUE:
        raise ValueError(f"{who}: raw channel {k} has non-finite values inside objects")
    words = out.cpu().numpy().view(np.uint64)
    pixels = words[present, 0].view(np.int64)
    if flags & _WEIGHTED_BAD_LABEL or (pixels < 1).any() or (pixels > area[present]).any():
        raise ValueError(f"{who}: label ids changed under the measurement")
    return border_table(words[present])


def _weighted_columns_of(lab, channels, shifts, peak_keys, nd, Z, Y, X, spatial, nid, present, area, sum1, weighted, border):
    """the weighted and the border columns: weighted's of every channel, then the border pixels and border's of every channel;
    one clx_region_weighted and one clx_region_border_intensity call per channel.  channels: [(raw_d, raw_type)]; peak_keys: per
    channel clx_region_intensity's largest keys (uint64 (nid)); sum1: clx_region_moments' rows of the present ids"""
    out = {}
    for k, (raw_d, raw_type) in enumerate(channels if weighted else []):
        if len(present):
            table = _weighted_rows(lab, raw_d, raw_type, Z, Y, X, nid, shifts[k], peak_keys[k], area, present, "region_table", k)
        else:
            table = weighted_table(np.zeros((0, WEIGHTED_WORDS), dtype=np.uint64))
        out.update(weighted_columns(area[present], sum1, table, shifts[k], nd, k, spatial))
    for k, (raw_d, raw_type) in enumerate(channels if border else []):
        if len(present):
            table = _border_rows(lab, raw_d, raw_type, nd, Z, Y, X, nid, shifts[k], area, present, "region_table", k)
        else:
            table = border_table(np.zeros((0, BORDER_WORDS), dtype=np.uint64))
        if k == 0:
            out.update(border_intensity_columns(table))
        out.update(border_intensity_columns(table, shifts[k], raw_type, k))
    return out


def _one_channel(labels, raw, k, device, who):
    """the front weighted_moments and border_intensity share -> None for a map without objects, else (lab flat, nd, spatial,
    (Z, Y, X), nid, area, present, raw_d flat, raw_type, shift, largest keys)"""
    if raw is None:
        raise ValueError(f"{who}: raw is needed")
    raw = _raw_channels(raw, tuple(int(v) for v in labels.shape), who)
    k = int(k)
    if not 0 <= k < raw.shape[0]:
        raise ValueError(f"{who}: channel k = {k} must lie in [0, {raw.shape[0]})")
    lab, device, nd, spatial, nid = _labels_on_device(labels, device, who)
    if lab.numel() == 0 or nid == 1:
        return None
    Z, Y, X = (1,) * (3 - nd) + spatial
    area_d, _, _, _ = _moments(lab, Z, Y, X, nid, who)
    area = area_d.cpu().numpy()
    area[0] = 0
    present = np.flatnonzero(area > 0)
    if not len(present):
        return None
    flat = lab.reshape(-1)
    raw_d, raw_type = _to_device_raw(raw[k], device)
    raw_d = raw_d.reshape(-1)
    _, shift, keys = _channel_columns_keys(flat, raw_d, raw_type, nid, present, area, k)
    return flat, nd, spatial, (Z, Y, X), nid, area, present, raw_d, raw_type, shift, keys


def weighted_moments(labels, raw, k=0, device=None):
    """The intensity-weighted sums of channel ``k`` of ``raw`` (``(*spatial)`` or ``(C, *spatial)``; float32, float64 or integers
    that fit int32) inside every object of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as
    ``region_table``): ``(ids, table, shift)``.  ``ids`` int64 (n): the objects present, ascending.  ``table``:
    ``weighted_table``'s dict of ``clx_region_weighted``'s 21 words per object, exact integers of ``q = rint(v * 2**shift)`` with
    the scale ``region_table`` uses for its ``intensity_mean`` (``intensity_shift``; 0 for integers): int64 arrays ``n`` and
    ``sum_q``, and Python ints ``peak`` (the flat index of the first pixel in raster order that attains the object's maximum)
    and ``sum_qz, sum_qy, sum_qx, sum_qzz, sum_qyy, sum_qxx, sum_qzy, sum_qzx, sum_qyx`` (a 2-D map has z = 0).
    ``weighted_columns`` forms ``region_table``'s columns of the table.  Runs on a HIP device; there is no CPU path."""
    who = "weighted_moments"
    got = _one_channel(labels, raw, k, device, who)
    if got is None:
        return np.zeros(0, dtype=np.int64), weighted_table(np.zeros((0, WEIGHTED_WORDS), dtype=np.uint64)), 0
    flat, _, _, (Z, Y, X), nid, area, present, raw_d, raw_type, shift, keys = got
    return present.astype(np.int64), _weighted_rows(flat, raw_d, raw_type, Z, Y, X, nid, shift, keys, area, present, who, int(k)), shift


def border_intensity(labels, raw, k=0, device=None):
    """The sums of channel ``k`` of ``raw`` over the BORDER pixels of every object of ``labels`` (the arguments of
    ``weighted_moments``): ``(ids, table, shift)``.  A border pixel of object i has a face neighbour (4 in 2-D, 6 in 3-D) that is
    not i: another object, background or the outside of the image.  ``table``: ``border_table``'s dict of
    ``clx_region_border_intensity``'s seven words per object: int64 arrays ``pixels`` (the border pixels), ``n`` (those counted)
    and ``sum_q``, uint64 order keys ``key_min`` and ``key_max`` and Python ints ``sum_qq``, of ``q = rint(v * 2**shift)``.
    ``border_intensity_columns`` forms ``region_table``'s columns of the table.  Runs on a HIP device; there is no CPU path."""
    who = "border_intensity"
    got = _one_channel(labels, raw, k, device, who)
    if got is None:
        return np.zeros(0, dtype=np.int64), border_table(np.zeros((0, BORDER_WORDS), dtype=np.uint64)), 0
    flat, nd, _, (Z, Y, X), nid, area, present, raw_d, raw_type, shift, _ = got
    return present.astype(np.int64), _border_rows(flat, raw_d, raw_type, nd, Z, Y, X, nid, shift, area, present, who, int(k)), shift


def region_table(labels, raw=None, device=None, boundary=False, topology=False, hull=False, inscribed=False, edge=False,
                 quantiles=None, mad=False, texture=False, texture_levels=8, texture_distance=1, texture_range=None,
                 radial=False, radial_rings=4, radial_width=None, radial_wedges=False, std=False, colocalization=False,
                 coloc_threshold=0.15, weighted=False, border_intensity=False):
    """One row per object id present in ``labels`` (2-D or 3-D integers, array or device tensor), ascending; columns
    ``label, area, bbox_min_*, bbox_max_*`` (max exclusive), ``centroid_*, cov_*, cov_eig_0..nd-1`` (descending),
    ``equivalent_diameter`` and, per channel k of ``raw`` (``None``, ``(*spatial)`` or ``(C, *spatial)``; float32,
    float64 or integers that fit int32), ``intensity_mean_c{k}, intensity_min_c{k}, intensity_max_c{k}``.
    ``boundary=True`` appends ``boundary_faces`` (faces to anything that is not the object), ``contact_faces`` (to
    other objects), ``num_neighbours`` (objects touched), ``touches_border`` (0 / 1: the bounding box reaches the image
    edge) and in 2-D ``border_pixels`` and ``perimeter`` (scikit-image's 4-neighbourhood formula, restated).
    ``topology=True`` appends, after those, ``euler_number`` (8- / 26-connectivity, as scikit-image's), ``euler_number_conn1``
    (4- / 6-connectivity) and in 2-D ``perimeter_crofton`` (four directions), in 3-D ``surface_area`` (Crofton, 13
    directions) and ``sphericity`` (``topology_columns``).
    ``hull=True`` appends, after those, in 2-D ``area_convex``, ``solidity``, ``feret_diameter_max``, ``feret_diameter_min``
    and ``hull_vertices``, in 3-D ``feret_diameter_max``: the hull of the pixels' corner points, which is not
    scikit-image's rasterised definition (``hull_columns``).
    ``inscribed=True`` appends, after those, ``inscribed_radius`` (the radius of the largest circle / ball inside the
    object: the maximum of ``label_distance_sq`` over its pixels, square-rooted), ``inscribed_centre_*`` (where it sits) and
    ``distance_sq_mean`` (``inscribed_columns``); ``edge`` is ``label_distance_sq``'s: whether the image edge counts as
    background.
    ``quantiles`` (at most 16 distinct floats in [0, 1], ``-0.0`` counting as ``0.0``; needs ``raw``) appends, after all of those, per channel k the float64
    columns ``intensity_q{repr(float(q))}_c{k}`` in the order given (``intensity_q0.25_c0``, ``intensity_q0.5_c0`` ...): NumPy's
    default ("linear") quantile of the object's raw values, with the index and the interpolation in exact rational
    arithmetic and one rounding (``quantile_ranks``, ``quantile_columns``).  ``mad=True`` appends ``intensity_mad_c{k}`` behind
    them: the median, by the same rule, of ``|v - median|`` in float64, unscaled (CellProfiler's MADIntensity).  The columns
    of channel 0 come first, then those of channel 1.
    ``texture=True`` (needs ``raw``) appends, after all of those, per channel k ``texture_pairs_c{k}`` (int64: the ordered
    same-object pixel pairs over all directions) and the thirteen float64 columns ``texture_<feature>_c{k}``, features in
    ``TEXTURE_FEATURES``' order: Haralick's features of the object's grey-level co-occurrence matrices at ``texture_levels``
    levels (2 .. 32) and pixel distance ``texture_distance`` (1 .. 64), the mean over the 4 (2-D) or 13 (3-D) directions that
    have a pair, NaN where none has (``cooccurrence``, ``texture_columns``: the project's own stated conventions).
    ``texture_range=(lo, hi)`` is the range the levels divide, for every channel; ``None`` takes per channel the smallest
    and the largest value under the objects of this map: levels are then relative to this image's objects.  All of
    channel 0's texture columns come before channel 1's.
    ``radial=True`` appends, after all of those, ``radial_area_r{j}`` (int64) for the ``radial_rings`` rings j (1 .. 32; ring 0
    is the rim, the last ring the core) and, with ``raw``, per channel k and ring j the float64 columns
    ``radial_mean_r{j}_c{k}``, ``radial_frac_r{j}_c{k}`` and ``radial_meanfrac_r{j}_c{k}``, with ``radial_wedges=True`` (2-D only)
    ``radial_cv_r{j}_c{k}`` behind them: the ring's mean, its share of the object's sum, its mean over the object's mean and
    the variation of the means of its eight 45-degree wedges (``radial_distribution``, ``radial_columns``: the quantities of
    CellProfiler's MeasureObjectIntensityDistribution on the project's own ring and wedge definitions, exact integers).  ``radial_width=None``: the rings divide every object's
    inscribed radius; an integer in 1 .. 32768: bands of that many pixels from the boundary, the last ring taking what lies
    deeper.  ``edge`` is the one of ``inscribed``; the distance map is formed once for both.  All of channel 0's radial
    columns come before channel 1's.
    ``std=True`` (needs ``raw``) appends, after all of those, ``intensity_std_c{k}`` per channel: the population standard
    deviation of the object's raw values (regionprops' ``intensity_std``, CellProfiler's StdIntensity), from the exact 128-bit
    sum of the squared quantised values.  ``colocalization=True`` (needs at least 2 channels) appends, after those, for every
    pair of channels j < k in lexicographic order ``coloc_pearson_c{j}_c{k}``, ``coloc_slope_c{j}_c{k}``,
    ``coloc_overlap_c{j}_c{k}``, ``coloc_k1_c{j}_c{k}``, ``coloc_k2_c{j}_c{k}``, ``coloc_manders1_c{j}_c{k}`` and
    ``coloc_manders2_c{j}_c{k}``: the quantities of CellProfiler's MeasureColocalization per object (``channel_products``,
    ``products_columns``).  Pearson and slope take all of the object's pixels; the other five the pixels at or above
    ``coloc_threshold`` (a float in [0, 1]) times the object's quantised maximum in each channel (``coloc_thresholds``: the
    project's own convention).  A column is NaN where its denominator is 0.
    ``weighted=True`` (needs ``raw``) appends, after all of those, per channel k ``intensity_sum_c{k}`` (the integrated
    intensity), ``centroid_weighted_*_c{k}``, ``cov_weighted_*_c{k}`` (the pairs of ``cov_*``), ``mass_displacement_c{k}`` (the
    distance between ``centroid_*`` and ``centroid_weighted_*``) and ``intensity_peak_*_c{k}`` (int64: where the object's
    brightest pixel sits, the first in raster order among equals): regionprops' ``centroid_weighted`` and order-2
    ``moments_weighted_central`` over the sum, CellProfiler's Location_CenterMassIntensity, MassDisplacement and
    Location_MaxIntensity, from exact 128-bit sums of value times coordinates (``weighted_moments``, ``weighted_columns``);
    float columns are NaN where the object's values sum to 0.  ``border_intensity=True`` (needs ``raw``) appends, after those,
    ``intensity_border_pixels`` (int64, once: the object's pixels with a face neighbour that is not the object's; in 2-D it
    equals ``border_pixels``) and per channel k ``intensity_border_sum_c{k}``, ``intensity_border_mean_c{k}``,
    ``intensity_border_std_c{k}`` (population) and, in the raw dtype, ``intensity_border_min_c{k}`` and
    ``intensity_border_max_c{k}`` over those pixels (CellProfiler's *IntensityEdge; ``border_intensity``,
    ``border_intensity_columns``).  It has nothing to do with ``edge``, which says whether the image edge counts as background
    for the distance map.  All of channel 0's weighted columns come before channel 1's, and so do the border columns.
    Returns ``dict[str, np.ndarray]``.  Runs on a HIP device; there is no CPU path."""
    return _region_table(labels, raw, device, boundary, topology, hull, inscribed, edge, quantiles, mad, texture, texture_levels,
                         texture_distance, texture_range, radial, radial_rings, radial_width, radial_wedges, std, colocalization,
                         coloc_threshold, weighted, border_intensity)[0]


def _region_table(labels, raw, device, boundary, topology=False, hull=False, inscribed=False, edge=False, quantiles=None,
                  mad=False, texture=False, texture_levels=8, texture_distance=1, texture_range=None, radial=False,
                  radial_rings=4, radial_width=None, radial_wedges=False, std=False, colocalization=False, coloc_threshold=0.15,
                  weighted=False, border_intensity=False):
    """region_table's columns and, with ``boundary``, contact_pairs' rows (else None)"""
    quantiles = _check_quantiles(quantiles, mad, raw)
    coloc_threshold = _check_products(std, colocalization, coloc_threshold, labels, raw)
    _check_weighted(weighted, border_intensity, raw)
    if radial:
        radial_rings, radial_width, radial_W = _check_radial(radial_rings, radial_width, radial_wedges, getattr(labels, "ndim", None))
    if texture:
        if raw is None:
            raise ValueError("region_table: texture needs raw")
        texture_levels, texture_distance, texture_range = _check_texture(texture_levels, texture_distance, texture_range)
    lab, device, nd, spatial, nid = _labels_on_device(labels, device, "region_table")
    Z, Y, X = (1,) * (3 - nd) + spatial
    if lab.numel() == 0 or nid == 1:
        area = np.zeros(1, dtype=np.int64)
        cols = shape_columns(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 6), np.int32),
                             np.zeros((0, 3), np.uint64), np.zeros((0, 6), np.uint64), nd)
        present = np.zeros(0, dtype=np.int64)
        bbox = np.zeros((0, 6), dtype=np.int32)
        sum1 = np.zeros((0, 3), dtype=np.uint64)
        bbox_d = bbox_all = area_d = None
    else:
        area_d, bbox_d, sum1_d, sum2_d = _moments(lab, Z, Y, X, nid, "region_table")
        area = area_d.cpu().numpy()
        area[0] = 0
        present = np.flatnonzero(area > 0)
        bbox_all = bbox_d.cpu().numpy()
        bbox = bbox_all[present]
        sum1 = sum1_d.cpu().numpy().view(np.uint64)[present]
        cols = shape_columns(present, area[present], bbox, sum1, sum2_d.cpu().numpy().view(np.uint64)[present], nd)
    channels, shifts, peak_keys = [], [], []                 # kept on the device for the order statistics, texture, radial ...
    if raw is not None:
        raw = _raw_channels(raw, spatial, "region_table")
        for k in range(raw.shape[0]):
            raw_d, raw_type = _to_device_raw(raw[k], device)
            if quantiles or mad or texture or radial or std or colocalization or weighted or border_intensity:
                channels.append((raw_d.reshape(-1), raw_type))
            shifts.append(0)
            peak_keys.append(None)
            if len(present):
                intensity, shifts[k], peak_keys[k] = _channel_columns_keys(lab.reshape(-1), raw_d.reshape(-1), raw_type, nid, present, area, k)
                cols.update(intensity)
            else:
                dt = raw_d.cpu().numpy().dtype
                cols.update({f"intensity_mean_c{k}": np.zeros(0), f"intensity_min_c{k}": np.zeros(0, dt),
                             f"intensity_max_c{k}": np.zeros(0, dt)})
    pairs = None
    if boundary:
        if len(present):
            pairs = _contacts(lab, nd, spatial, nid, len(present), "region_table")
        else:
            pairs = tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
        classes = None
        if nd == 2:
            classes = _perimeter_classes(lab, Y, X, nid)[present] if len(present) else np.zeros((0, 4), dtype=np.int64)
        cols.update(boundary_columns(present, bbox, spatial, *pairs, classes, nd))
    if topology:
        counts = _topology_counts(lab, nd, Z, Y, X, nid)[present] if len(present) else np.zeros((0, 5), dtype=np.int64)
        cols.update(topology_columns(area[present], counts, nd))
    if hull:
        ints = _hull_rows(lab, nd, Z, Y, X, nid, bbox_d, bbox_all, present)[present] if len(present) else np.zeros((0, 5), dtype=np.int64)
        cols.update(hull_columns(area[present], ints, nd))
    if (inscribed or radial) and len(present):               # one distance map and one reduction for both
        dist_d, inscribed_d = _inscribed_rows(lab.reshape(-1), nd, Z, Y, X, nid, edge)
    if inscribed:
        ints = inscribed_d.cpu().numpy()[present] if len(present) else np.zeros((0, 3), dtype=np.int64)
        cols.update(inscribed_columns(area[present], ints, spatial, nd))
    if quantiles or mad:
        cols.update(_order_columns(lab.reshape(-1), channels, nid, present, area, area_d, quantiles, mad))
    if texture:
        cols.update(_texture_columns_of(lab, channels, nd, Z, Y, X, nid, bbox_d, present, area, cols, texture_levels, texture_distance,
                                        texture_range))
    if radial:
        if len(present):
            count, isums = _radial_tables(lab.reshape(-1), dist_d, inscribed_d, [c + (s,) for c, s in zip(channels, shifts)], nd, Z, Y,
                                          X, nid, present, area, radial_rings, radial_width, radial_W, "region_table")
        else:
            count = np.zeros((0, radial_rings, radial_W), dtype=np.int64)
            isums = [count] * len(channels)
        cols.update(radial_columns(area[present], count, nd=nd))
        for k, isum in enumerate(isums):
            cols.update(radial_columns(area[present], count, isum, shifts[k], nd, k))
    if std or colocalization:
        cols.update(_products_columns_of(lab.reshape(-1), channels, shifts, nid, present, area, cols, std, colocalization, coloc_threshold))
    if weighted or border_intensity:
        cols.update(_weighted_columns_of(lab.reshape(-1), channels, shifts, peak_keys, nd, Z, Y, X, spatial, nid, present, area, sum1,
                                         weighted, border_intensity))
    return cols, pairs


def _format(value):
    return "%.17g" % value if isinstance(value, (float, np.floating)) else "%d" % value


def measure(inference_config, contacts=False, topology=False, hull=False, inscribed=False, quantiles=None, mad=False, texture=False,
            texture_levels=8, texture_distance=1, radial=False, radial_rings=4, radial_width=None, radial_wedges=False, std=False,
            colocalization=False, coloc_threshold=0.15, weighted=False, border_intensity=False) -> None:
    """For every bandwidth: the tables of all samples' label maps (``segmentation_dataset_config.dataset_name``) with
    every channel of the raw dataset, as ``measurements_bandwidth-<b>.csv`` in the working directory — a header line,
    then ``sample`` and ``region_table``'s columns, floats as ``%.17g``.  ``contacts=True`` adds the boundary columns
    and writes ``contacts_bandwidth-<b>.csv`` beside it: ``sample,label_a,label_b,faces``, one line per pair of
    objects that touch.  ``topology=True`` adds the topology columns, ``hull=True`` the convex hull columns,
    ``inscribed=True`` the inscribed circle / ball columns (``edge=False``: distances to pixels of the map only),
    ``quantiles`` and ``mad`` the intensity quantile and median-absolute-deviation columns of every channel
    (``region_table``'s arguments), ``texture=True`` the texture columns of every channel at ``texture_levels`` grey levels and
    pixel distance ``texture_distance``; their range is per sample and channel, the smallest and the largest value under that
    sample's objects, so the levels are relative to each image's objects; ``radial=True`` the radial distribution columns at
    ``radial_rings`` rings, relative or ``radial_width`` pixels wide, with ``radial_wedges`` the wedge variation too
    (``region_table``'s arguments, ``edge=False``); ``std=True`` the intensity standard deviation of every channel,
    ``colocalization=True`` the colocalization columns of every pair of channels with ``coloc_threshold`` (``region_table``'s
    arguments); ``weighted=True`` the intensity-weighted centroid, covariance, mass displacement, integrated intensity and peak
    position of every channel, ``border_intensity=True`` the intensity columns over every object's border pixels
    (``region_table``'s arguments, ``edge=False``).  Rank 0 works alone under torch.distributed."""
    import torch

    from . import parallel
    from .datasets.meta_data import DatasetMetaData
    from .train import _require_hip_device
    from .utils import zarr_io

    if parallel.rank() != 0:
        return
    dataset_config = inference_config.dataset_config
    meta = DatasetMetaData.from_dataset_config(dataset_config)
    device = _require_hip_device(inference_config.device)
    if parallel.world_size() > 1:
        device = torch.device("cuda", torch.cuda.current_device())
    seg_config = inference_config.segmentation_dataset_config
    ds_seg = zarr_io.open(seg_config.container_path, "r")[seg_config.dataset_name]
    ds_raw = zarr_io.open(dataset_config.container_path, "r")[dataset_config.dataset_name]
    for bandwidth in range(inference_config.num_bandwidths):
        header, lines, pair_lines = None, [], []
        for sample in range(meta.num_samples):
            labels = ds_seg[sample, bandwidth].astype(np.int32)
            table, pairs = _region_table(labels, ds_raw[sample], device, contacts, topology, hull, inscribed, False, quantiles, mad,
                                         texture, texture_levels, texture_distance, None, radial, radial_rings, radial_width,
                                         radial_wedges, std, colocalization, coloc_threshold, weighted, border_intensity)
            if contacts:
                pair_lines += [f"{sample},{a},{b},{n}" for a, b, n in zip(*pairs) if a > 0]
            header = header or ["sample"] + list(table)
            columns = list(table.values())
            for i in range(len(table["label"])):
                lines.append(",".join([str(sample)] + [_format(c[i]) for c in columns]))
        with open(f"measurements_bandwidth-{bandwidth}.csv", "w") as out:
            out.write(",".join(header or ["sample"]) + "\n")
            for line in lines:
                out.write(line + "\n")
        if contacts:
            with open(f"contacts_bandwidth-{bandwidth}.csv", "w") as out:
                out.write("sample,label_a,label_b,faces\n")
                for line in pair_lines:
                    out.write(line + "\n")


if __name__ == "__main__":
    from .cli import measure as _command

    _command()
