"""``relate`` stage: what connects TWO label maps of the same image -- the nuclei and the cells the pipeline segments, a
prediction and a reference -- where the measure stage describes each map on its own.  CellProfiler's RelateObjects,
IdentifyTertiaryObjects and MeasureObjectOverlap, which users do on the host with one mask pass per object.

The device gives integers (``csrc/label_overlap.hip``): ``clx_label_overlaps``, the sparse joint histogram of the two maps as a
set of ``(a, b, pixels)`` rows, a few per object whatever the number of objects (``label_overlaps``), and, on request,
``clx_region_clearance``: over every child's pixels inside its parent the smallest value of the parent map's label-aware
distance map (``clx_label_distance_sq``), where it is attained, and the map's sum.  Areas and centroids are
``clx_region_moments``'.  The host forms the tables from them (``assign_parents``, ``relate_columns``); every float is one
correctly rounded operation on exact integers.

Definitions.  The PARENT of a child ``i`` is the object ``j > 0`` of the other map that shares the most pixels with it, the
smallest ``j`` among equals; 0 if ``i`` lies over background only.  ``overlap`` is that number of pixels, ``fraction_inside =
overlap / area``, ``outside`` the child's pixels over the parents' background, ``num_parents`` the distinct ``j > 0`` it
touches, ``parent_centroid_distance`` the distance between the two centroids.  ``clearance`` is the smallest distance from a
pixel of the child inside its parent to the nearest pixel that is not the parent's (1.0: the child touches the parent's
boundary), ``clearance_<axis>`` the first pixel in raster order that attains it, ``depth_sq_mean`` the mean squared distance
over those pixels.  A parent's ``num_children`` counts the children assigned to it, ``children_area`` its pixels under ANY
child, ``tertiary_area = area - children_area`` what ``tertiary_labels`` leaves of it: the cytoplasm, cell minus nucleus.

    python -m cellulus_amd.relate experiment.toml --children NAME --parents NAME [--clearance] [--tertiary NAME]

writes ``relate_children_bandwidth-<b>.csv`` and ``relate_parents_bandwidth-<b>.csv`` next to the measure stage's files and,
with ``--tertiary``, the tertiary label maps into the segmentation container.
"""

import math

import numpy as np
import torch

from . import _clx, _stage
from .measure import (DISTANCE_CHANGED, FLAGS, LABELS_OUT_OF_RANGE, _call, _check_map, _distance_map, _pair_capacity, _pair_table,
                      _resolve_device, _Scene, _to_device_labels)
from .measure_columns import DIST_INF, _exact_div, _extents, _raster_columns, _sqrt_ratio

NO_PIXEL = (1 << 64) - 1                # clx_region_clearance's out[i][1] of an id without a counted pixel


def _check_maps(a, b, who, names=("children", "parents")):
    """the checks on a pair of label maps that need no device: integers, 2-D or 3-D, of one shape -> (nd, spatial)"""
    for name, m in zip(names, (a, b)):
        _check_map(m, who, name)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{who}: {names[0]} has shape {tuple(a.shape)}, {names[1]} {tuple(b.shape)}")
    return a.ndim, tuple(int(v) for v in a.shape)


def _scenes(a, b, device, who, names=("children", "parents")):
    """-> the measure stage's scenes of the two maps after the host checks, their moments not taken yet"""
    nd, spatial = _check_maps(a, b, who, names)
    on_device = [m for m in (a, b) if torch.is_tensor(m) and m.is_cuda]
    device = _resolve_device(on_device[0] if on_device else a, device)
    la, lb = _to_device_labels(a, device, who), _to_device_labels(b, device, who)
    _clx.require_device(la, names[0])
    _clx.require_device(lb, names[1])
    return tuple(_Scene(who, m, device, nd, spatial, int(m.max().item()) + 1 if m.numel() else 1) for m in (la, lb))


def _overlaps(sa, sb):
    """clx_label_overlaps of two scenes -> (a, b, pixels) int64, sorted by (a, b)"""
    npix = sa.lab.numel()
    if npix == 0 or (sa.nid == 1 and sb.nid == 1):           # no pixel, or background only in both maps: no pair
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    # an object overlaps one or two of the other map and the background: a few pairs per object, never more than pixels
    capacity = _pair_capacity(min(sa.nid - 1 + sb.nid - 1, npix))
    return _pair_table(sa.device, sa.who, "clx_label_overlaps", {1 | 2: LABELS_OUT_OF_RANGE}, capacity, sa.lab, sb.lab, npix, sa.nid,
                       sb.nid)


def label_overlaps(a, b, device=None):
    """The sparse joint histogram of two label maps ``a`` and ``b`` (2-D or 3-D integers of one shape, arrays or device
    tensors; the same types and range as ``region_table``): ``(ids_a, ids_b, pixels)`` int64 arrays, one row per pair
    ``(a[p], b[p]) != (0, 0)`` that occurs, sorted by ``(a, b)``.  Rows with ``ids_b == 0`` are an object's pixels over the
    other map's background; an object's pixel count is the sum of its rows.  Runs on a HIP device; there is no CPU path."""
    return _overlaps(*_scenes(a, b, device, "label_overlaps", ("a", "b")))


def _rows(ids_a, ids_b, pixels, who):
    rows = [np.asarray(v).astype(np.int64).reshape(-1) for v in (ids_a, ids_b, pixels)]
    if not len(rows[0]) == len(rows[1]) == len(rows[2]):
        raise ValueError(f"{who}: ids_a, ids_b and pixels must have one length, got {[len(r) for r in rows]}")
    if len(rows[0]) and (rows[0].min() < 0 or rows[1].min() < 0 or rows[2].min() < 1):
        raise ValueError(f"{who}: ids must be >= 0 and pixels >= 1")
    return rows


def assign_parents(ids_a, ids_b, pixels):
    """From ``label_overlaps``' rows: for every id of ``a`` (every ``ids_a > 0`` that occurs) the id ``b > 0`` it shares the
    most pixels with, the smallest such id among equals, or 0 if it lies over background only.  Returns ``(label, parent,
    overlap)`` int64 arrays sorted by label; ``overlap`` is the number of shared pixels (0 without a parent).  Host only."""
    a, b, n = _rows(ids_a, ids_b, pixels, "assign_parents")
    label = np.unique(a[a > 0])
    parent = np.zeros(len(label), dtype=np.int64)
    overlap = np.zeros(len(label), dtype=np.int64)
    both = (a > 0) & (b > 0)
    a, b, n = a[both], b[both], n[both]
    order = np.lexsort((b, -n, a))                           # per a: most pixels first, the smaller b among equals
    a, b, n = a[order], b[order], n[order]
    first = np.flatnonzero(np.r_[True, a[1:] != a[:-1]]) if len(a) else np.zeros(0, dtype=np.int64)
    at = np.searchsorted(label, a[first])
    parent[at] = b[first]
    overlap[at] = n[first]
    return label, parent, overlap


def _moments_arg(m, who, name):
    label, area, sum1 = m
    label = np.asarray(label).astype(np.int64).reshape(-1)
    area = np.asarray(area).astype(np.int64).reshape(-1)
    sum1 = np.asarray(sum1).reshape(-1, 3)
    if not len(label) == len(area) == len(sum1):
        raise ValueError(f"{who}: {name} must be (label (n), area (n), sum1 (n, 3)) of one n")
    if len(label) and (np.any(np.diff(label) <= 0) or label[0] < 1 or area.min() < 1):
        raise ValueError(f"{who}: {name} needs increasing labels >= 1 with areas >= 1")
    return label, area, [[int(v) for v in r] for r in sum1]


def relate_columns(ids_a, ids_b, pixels, child_moments, parent_moments, shape, clearance=None):
    """The two tables of ``relate`` from integers.  ``ids_a, ids_b, pixels``: ``label_overlaps``' rows of (children, parents);
    ``child_moments`` / ``parent_moments``: ``(label (n), area (n), sum1 (n, 3) = Σz Σy Σx)`` of the objects present in either
    map, as ``clx_region_moments`` gives them; ``shape`` the maps' 2 or 3 extents; ``clearance``: ``clx_region_clearance``'s
    rows ``(n, 3)`` of the children, or None.  Returns ``(child_table, parent_table)``, dicts of columns:

    child: ``label``, ``area``, ``parent`` (0: none), ``overlap``, ``fraction_inside``, ``outside``, ``num_parents``,
    ``parent_centroid_distance`` (NaN without a parent) and, with ``clearance``, ``clearance`` (NaN without a pixel inside a
    parent, inf where the parent fills a map without an edge to measure to), ``clearance_z/_y/_x`` (2-D: y and x; int64, -1
    without such a pixel) and ``depth_sq_mean``.
    parent: ``label``, ``area``, ``num_children``, ``children_area``, ``children_fraction``, ``tertiary_area``.
    Host only; the module's docstring has the definitions."""
    who = "relate_columns"
    nd = _extents(shape, who)
    a, b, n = _rows(ids_a, ids_b, pixels, who)
    clabel, carea, csum = _moments_arg(child_moments, who, "child_moments")
    plabel, parea, psum = _moments_arg(parent_moments, who, "parent_moments")
    nc, npar = len(clabel), len(plabel)
    # the pixel counts are the row and column sums of the table: the rows must belong to these moments
    rows_a, rows_b = a[a > 0], b[b > 0]
    if (not np.array_equal(np.unique(rows_a), clabel) or not np.array_equal(np.unique(rows_b), plabel)
            or not np.array_equal(np.bincount(np.searchsorted(clabel, rows_a), n[a > 0], nc).astype(np.int64), carea)
            or not np.array_equal(np.bincount(np.searchsorted(plabel, rows_b), n[b > 0], npar).astype(np.int64), parea)):
        raise ValueError(f"{who}: the overlap rows and the moments describe different maps")
    label, parent, overlap = assign_parents(a, b, n)
    at = np.searchsorted(clabel, a[a > 0])
    outside = np.bincount(at[b[a > 0] == 0], n[(a > 0) & (b == 0)], nc).astype(np.int64)
    num_parents = np.bincount(at[b[a > 0] > 0], minlength=nc).astype(np.int64)
    distance = np.full(nc, math.nan)
    where = np.searchsorted(plabel, parent)
    for i in np.flatnonzero(parent > 0):
        na, nb = int(carea[i]), int(parea[where[i]])
        num = sum((sa * nb - sb * na) ** 2 for sa, sb in zip(csum[i][3 - nd:], psum[where[i]][3 - nd:]))
        distance[i] = _sqrt_ratio(num, (na * nb) ** 2)
    child = {"label": clabel, "area": carea, "parent": parent, "overlap": overlap,
             "fraction_inside": _exact_div(overlap.astype(object), carea.astype(object)), "outside": outside,
             "num_parents": num_parents, "parent_centroid_distance": distance}
    if clearance is not None:
        rows = np.asarray(clearance).reshape(-1, 3)
        if len(rows) != nc:
            raise ValueError(f"{who}: clearance has {len(rows)} rows for {nc} children")
        rows = [[int(v) & NO_PIXEL for v in r] for r in rows]                 # int64 views of the device words included
        some = [r[0] > 0 for r in rows]
        if any(s != (r[1] != NO_PIXEL) for s, r in zip(some, rows)) or any(r[0] != o for r, o in zip(rows, overlap)):
            raise ValueError(f"{who}: the clearance rows and the overlap rows describe different maps")
        d2 = [r[1] >> 32 for r in rows]
        inf = [s and d >= DIST_INF for s, d in zip(some, d2)]
        child["clearance"] = np.array([math.nan if not s else math.inf if i else _sqrt_ratio(d, 1) for s, d, i in zip(some, d2, inf)],
                                      dtype=np.float64)
        index = np.array([r[1] & 0xFFFFFFFF if s else 0 for r, s in zip(rows, some)], dtype=np.int64)
        if len(index) and index.max() >= int(np.prod(shape)):
            raise ValueError(f"{who}: a clearance row points outside a map of shape {tuple(shape)}")
        child.update(_raster_columns("clearance", index, shape, who, mask=some))
        child["depth_sq_mean"] = np.array([math.nan if not s else math.inf if i else r[2] / r[0] for r, s, i in zip(rows, some, inf)],
                                          dtype=np.float64)
    inside = (a > 0) & (b > 0)
    children_area = np.bincount(np.searchsorted(plabel, b[inside]), n[inside], npar).astype(np.int64)
    table = {"label": plabel, "area": parea,
             "num_children": np.bincount(where[parent > 0], minlength=npar).astype(np.int64), "children_area": children_area,
             "children_fraction": _exact_div(children_area.astype(object), parea.astype(object)),
             "tertiary_area": parea - children_area}
    return child, table


def _present_moments(scene):
    """(label, area, sum1) of the objects present in the scene's map, from one clx_region_moments call"""
    scene.measured()
    return scene.present.astype(np.int64), scene.area[scene.present], scene.sum1


def _clearance_rows(sa, sb, label, parent, edge):
    """clx_label_distance_sq of the parents' map, then clx_region_clearance -> int64 (n, 3) rows of the children `label`"""
    dist = _distance_map(sb, edge)
    table = np.zeros(sa.nid, dtype=np.int32)
    table[label] = parent
    out = sa.ids(3)
    _call(sa.device, sa.who, "clx_region_clearance", {1: LABELS_OUT_OF_RANGE, 2: DISTANCE_CHANGED}, sa.lab, sb.lab, dist,
          torch.from_numpy(table).to(sa.device), sa.lab.numel(), sa.nid, out, FLAGS)
    return out.cpu().numpy()[label]


def relate(children, parents, device=None, clearance=False, edge=False):
    """``(child_table, parent_table)`` of two label maps of one image (2-D or 3-D integers of one shape, arrays or device
    tensors; the same types and range as ``region_table``): which parent every child lies in and how much of it, how many
    children every parent holds and what they leave of it; ``relate_columns`` lists the columns, the module's docstring has
    the definitions.  ``clearance=True`` adds how near every child comes to its parent's boundary, from the label-aware
    distance map of ``parents``; ``edge`` has ``label_distance_sq``'s meaning there (True: the image edge counts as boundary).
    Runs on a HIP device; there is no CPU path."""
    sa, sb = _scenes(children, parents, device, "relate")
    a, b, n = _overlaps(sa, sb)
    child_moments, parent_moments = _present_moments(sa), _present_moments(sb)
    rows = None
    if clearance:
        label, parent, _ = assign_parents(a, b, n)
        rows = _clearance_rows(sa, sb, label, parent, edge) if len(label) else np.zeros((0, 3), dtype=np.int64)
    return relate_columns(a, b, n, child_moments, parent_moments, sa.spatial, rows)


def tertiary_labels(children, parents):
    """The parents' map with every pixel under a child set to 0: the cytoplasm when the parents are cells and the children their
    nuclei.  Arrays or tensors, 2-D or 3-D integers of one shape; the result has the type, dtype and device of ``parents``.
    ``region_table`` of it measures the tertiary objects with everything the measure stage has."""
    _check_maps(children, parents, "tertiary_labels")
    if torch.is_tensor(parents):
        under = torch.as_tensor(children, device=parents.device) > 0
        return torch.where(under, torch.zeros_like(parents), parents)
    return np.where(children > 0, np.zeros((), parents.dtype), parents)


def relate_stage(inference_config, children, parents, clearance=False, tertiary=None) -> None:
    """For every bandwidth: ``relate``'s tables of all samples, with ``children`` and ``parents`` the names of two label
    datasets ``[sample, bandwidth, ...]`` in ``segmentation_dataset_config.container_path`` (``segment()``'s output under the
    two ``post_processing`` settings, say), as ``relate_children_bandwidth-<b>.csv`` and ``relate_parents_bandwidth-<b>.csv`` in
    the working directory -- a header line, then ``sample`` and the table's columns, floats as ``%.17g``.  ``clearance=True``
    adds the clearance columns (``edge=False``).  ``tertiary=NAME`` writes ``tertiary_labels`` of every sample and bandwidth
    into a new uint16 dataset NAME of that container.  Rank 0 works alone under torch.distributed."""
    for name, value in (("children", children), ("parents", parents)):
        if not isinstance(value, str) or not value:
            raise ValueError(f"relate_stage: {name} must be the name of a dataset, got {value!r}")
    if children == parents:
        raise ValueError(f"relate_stage: children and parents are the same dataset {children!r}")
    if tertiary is not None and (not isinstance(tertiary, str) or not tertiary or tertiary in (children, parents)):
        raise ValueError(f"relate_stage: tertiary must name a new dataset other than children and parents, got {tertiary!r}")
    stage = _stage.begin("relate_stage", inference_config)
    if stage is None:
        return
    stage.open("a" if tertiary else "r", children, parents)
    ds_children, ds_parents = stage.f[children], stage.f[parents]
    ds_tertiary = stage.create(tertiary) if tertiary else None      # one that exists: the container's ContainsArrayError

    def per_sample(sample, bandwidth):
        a = ds_children[sample, bandwidth].astype(np.int32)
        b = ds_parents[sample, bandwidth].astype(np.int32)
        tables = relate(a, b, stage.device, clearance=clearance)
        if ds_tertiary is not None:
            ds_tertiary[sample, bandwidth] = tertiary_labels(a, b).astype(np.uint16)
        return tables

    stage.run(per_sample, ("relate_children", "relate_parents"))


if __name__ == "__main__":
    from .cli import relate as _command

    _command()
