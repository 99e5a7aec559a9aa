"""``expand`` stage: what MAKES the second label map of a nucleus-based workflow from the first -- every nucleus grown by N
pixels without letting neighbours merge (CellProfiler's IdentifySecondaryObjects "Distance-N" and ExpandOrShrinkObjects,
scikit-image's ``expand_labels``) -- and the neighbour graph of objects that do not touch, from the Voronoi zones of the objects
(MeasureObjectNeighbors' "expand until adjacent"), which users take from ``scipy.ndimage.distance_transform_edt(...,
return_indices=True)`` on the host, where the choice among equidistant objects is an accident of the scan order.

The device gives integers (``csrc/label_nearest.hip``): ``clx_label_nearest``, the exact Euclidean feature transform of a label
map -- for every pixel the squared distance to the nearest object pixel and that object's id (``nearest_object``).  The zones'
areas are ``clx_region_moments`` of the nearest-object map, their reach ``clx_region_inscribed`` of that map and the distances,
their adjacency ``clx_region_contacts`` of it.  The host forms the table from them (``zone_columns``); every float is one
correctly rounded operation on exact integers.

Definitions.  An object pixel is a pixel with a label > 0.  ``dist_sq[p]`` is the smallest ``|p - q|²`` over the object pixels
``q``, ``nearest[p]`` the SMALLEST label among the object pixels at that distance: the result is a function of the map alone,
whatever the axis order.  With a ``limit`` a pixel farther than it from every object has ``nearest 0`` and ``dist_sq DIST_INF``.
The ZONE of an object is the set of pixels whose nearest object it is, its own included.  ``zone_fraction = area / zone_area``
is the local density, ``zone_reach`` the largest distance inside the zone and ``zone_reach_<axis>`` the first pixel in raster
order that attains it, ``zone_dist_sq_mean`` the mean of ``dist_sq`` over the zone, ``num_neighbours`` the zones that share a
face with it, ``zone_border`` those faces and ``zone_border_open`` its faces towards pixels of no zone (beyond the limit).

    python -m cellulus_amd.expand experiment.toml --source NAME [--distance D --output NAME] [--neighbours [--limit D]]

writes, with ``--output``, ``expand_labels`` of every sample and bandwidth of ``NAME`` into a new dataset of the segmentation
container and, with ``--neighbours``, ``zones_bandwidth-<b>.csv`` and ``zone_pairs_bandwidth-<b>.csv`` next to the measure
stage's files.
"""

import math

import numpy as np
import torch

from . import _stage
from .measure import FLAGS, LABELS_OUT_OF_RANGE, _check_map, _contacts, _in_type_of, _inscribed_of, _result_scene, _scene, _workspace
from .measure_columns import DIST_INF, _exact_div, _extents, _raster_columns, _real_fraction, _sqrt_ratio


def _limit_sq(limit, who, name="limit"):
    """``floor(limit²)``, formed exactly, of a real distance >= 0; -1 (no limit) for None"""
    exact = _real_fraction(limit, who, name, none=True)
    if exact is None:
        return -1
    limit_sq = math.floor(exact ** 2)
    if limit_sq >= DIST_INF:
        raise ValueError(f"{who}: the square of {name} must be below 2^30, got {limit!r}")
    return limit_sq


def _nearest_maps(scene, limit_sq):
    """one clx_label_nearest call -> (nearest, dist_sq), flat int32 device tensors"""
    npix = scene.lab.numel()
    workspace, nbytes = _workspace(scene, "clx_label_nearest_workspace", npix)
    nearest = torch.empty(npix, dtype=torch.int32, device=scene.device)
    dist = torch.empty(npix, dtype=torch.int32, device=scene.device)
    scene.call("clx_label_nearest", {1: LABELS_OUT_OF_RANGE}, scene.lab, scene.nd, scene.Z, scene.Y, scene.X, scene.nid, limit_sq,
               nearest, dist, FLAGS, workspace, nbytes)
    return nearest, dist


def _nearest(labels, limit, device, who, name="limit"):
    """the host checks, then the scene of ``labels`` and ``_nearest_maps`` of it (None for a map without a pixel)"""
    limit_sq = _limit_sq(limit, who, name)
    _check_map(labels, who)
    scene = _scene(labels, device, who)
    return scene, (_nearest_maps(scene, limit_sq) if scene.lab.numel() else None)


def nearest_object(labels, limit=None, device=None):
    """For every pixel of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as
    ``region_table``) the nearest object and the squared Euclidean distance to it, exact integers: ``(nearest, dist_sq)``,
    int32 DEVICE tensors in the shape of ``labels``.  ``dist_sq`` is ``scipy.ndimage.distance_transform_edt(labels == 0) ** 2``,
    ``nearest`` the label at its ``return_indices`` wherever one object is nearest, and the SMALLEST label among the nearest
    where several are: the same for a map and its transpose.  A pixel of an object has its own label and 0.  ``limit`` (a real
    distance >= 0 whose square is below 2^30, or None): a pixel farther than ``limit`` from every object has ``nearest 0`` and
    ``dist_sq DIST_INF``, as every pixel of a map without objects has; the comparison is ``dist_sq <= floor(limit²)``, formed
    exactly.  The search along y and z costs O(distance to the nearest object) per pixel, at most ``limit``: a map with one
    small object and no limit is the slow case.  Runs on a HIP device; there is no CPU path."""
    scene, maps = _nearest(labels, limit, device, "nearest_object")
    if maps is None:
        return tuple(torch.empty(scene.spatial, dtype=torch.int32, device=scene.device) for _ in range(2))
    return maps[0].reshape(scene.spatial), maps[1].reshape(scene.spatial)


def expand_labels(labels, distance, device=None):
    """``skimage.segmentation.expand_labels``: every background pixel within ``distance`` (inclusive; a real number >= 0) of an
    object takes the label of the nearest object, the smallest label among equally near ones; objects keep their pixels and
    never merge.  Arrays or tensors, 2-D or 3-D integers (the same range as ``region_table``); the result has the type, dtype
    and device of ``labels``.  ``distance = 0`` returns an equal map.  The grown objects are the "cells" of nuclei: ``relate``
    assigns the nuclei to them, ``tertiary_labels`` leaves the cytoplasm.  Runs on a HIP device; there is no CPU path."""
    if distance is None:
        raise TypeError("expand_labels: distance must be a real number, got None")
    scene, maps = _nearest(labels, distance, device, "expand_labels", "distance")
    return _in_type_of(labels, scene, None if maps is None else maps[0])


def zone_columns(label, area, zone_area, rows, a, b, faces, edge_faces, shape):
    """The two tables of ``zone_table`` from integers.  ``label`` (n): the objects present, ascending; ``area`` (n) their
    pixels, ``zone_area`` (n) the pixels of their zones (``clx_region_moments`` of the map and of its nearest-object map);
    ``rows`` (n, 3): ``clx_region_inscribed``'s rows ``D2, index, Σd²`` of the nearest-object map and the distances; ``a, b,
    faces``: ``contact_pairs``' rows of the nearest-object map (a < b; a == 0: faces to pixels of no zone and to the outside of
    the image); ``edge_faces`` (n): the zones' faces to the outside of the image; ``shape`` the map's 2 or 3 extents.  Returns
    ``(object_table, pair_table)``, dicts of columns:

    object: ``label``, ``area``, ``zone_area``, ``zone_fraction``, ``zone_reach``, ``zone_reach_z/_y/_x`` (2-D: y and x; int64),
    ``zone_dist_sq_mean``, ``num_neighbours``, ``zone_border``, ``zone_border_open``.
    pair: ``label_a``, ``label_b``, ``faces``: the rows given, sorted by (a, b).
    Host only; the module's docstring has the definitions."""
    who = "zone_columns"
    _extents(shape, who)
    label, area, zone_area, edge_faces = (np.asarray(v).astype(np.int64).reshape(-1) for v in (label, area, zone_area, edge_faces))
    a, b, faces = (np.asarray(v).astype(np.int64).reshape(-1) for v in (a, b, faces))
    n = len(label)
    rows = [[int(v) for v in r] for r in np.asarray(rows).reshape(-1, 3)]
    if not len(area) == len(zone_area) == len(edge_faces) == len(rows) == n:
        raise ValueError(f"{who}: area, zone_area, rows and edge_faces must have one row per label")
    if not len(a) == len(b) == len(faces):
        raise ValueError(f"{who}: a, b and faces must have one length")
    if n and (np.any(np.diff(label) <= 0) or label[0] < 1 or area.min() < 1 or np.any(zone_area < area)):
        raise ValueError(f"{who}: needs increasing labels >= 1 with 1 <= area <= zone_area")
    if len(a) and (np.any(a >= b) or a.min() < 0 or faces.min() < 1 or not np.isin(b, label).all() or not np.isin(a[a > 0], label).all()):
        raise ValueError(f"{who}: the pairs need 0 <= a < b, faces >= 1 and ids among the labels")
    if any(r[0] >= DIST_INF or r[1] >= int(np.prod(shape)) for r in rows):
        raise ValueError(f"{who}: a row of the reach lies outside a map of shape {tuple(shape)}")
    order = np.lexsort((b, a))
    a, b, faces = a[order], b[order], faces[order]
    between = a > 0
    row_a, row_b = np.searchsorted(label, a[between]), np.searchsorted(label, b[between])
    neighbours, border = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for at in (row_a, row_b):
        np.add.at(neighbours, at, 1)
        np.add.at(border, at, faces[between])
    towards_none = np.zeros(n, dtype=np.int64)
    np.add.at(towards_none, np.searchsorted(label, b[~between]), faces[~between])
    if np.any(towards_none < edge_faces):
        raise ValueError(f"{who}: the pairs and edge_faces describe different maps")
    table = {"label": label, "area": area, "zone_area": zone_area,
             "zone_fraction": _exact_div(area.astype(object), zone_area.astype(object)),
             "zone_reach": np.array([_sqrt_ratio(r[0], 1) for r in rows], dtype=np.float64)}
    table.update(_raster_columns("zone_reach", np.array([r[1] for r in rows], dtype=np.int64), shape, who))
    table["zone_dist_sq_mean"] = _exact_div([r[2] for r in rows], zone_area.astype(object))
    table.update({"num_neighbours": neighbours, "zone_border": border, "zone_border_open": towards_none - edge_faces})
    return table, {"label_a": a, "label_b": b, "faces": faces}


def _edge_faces(zones, scene):
    """the faces of every id of the map ``zones`` to the outside of the image, int64 (nid): a pixel in the first or the last
    position of a counted axis has one there (an axis of extent 1: both).  The border slices are counted on the host"""
    grid = zones.reshape(scene.spatial)
    edge = [grid.select(axis, at).reshape(-1) for axis in range(scene.nd) for at in (0, -1)]
    return np.bincount(torch.cat(edge).cpu().numpy(), minlength=scene.nid).astype(np.int64)


def zone_table(labels, limit=None, device=None):
    """``(object_table, pair_table)`` of the zones of a label map (2-D or 3-D integers, array or device tensor; the same types
    and range as ``region_table``): the Voronoi tessellation of the image by its objects, every pixel belonging to the nearest
    object (``nearest_object``; ``limit`` is that function's: zones reach no farther).  The object table has one row per object:
    its area and its zone's, how far and where the zone reaches, how many zones it borders and with how many faces; the pair
    table is ``contact_pairs`` of the zone map: the neighbour graph of objects that need not touch.  ``zone_columns`` lists the
    columns, the module's docstring has the definitions.  A map without objects gives empty tables with these columns.
    Runs on a HIP device; there is no CPU path."""
    scene, maps = _nearest(labels, limit, device, "zone_table")
    scene.measured()
    if scene.empty:
        none = np.zeros(0, dtype=np.int64)
        return zone_columns(none, none, none, np.zeros((0, 3), dtype=np.int64), none, none, none, none, scene.spatial)
    nearest, dist = maps
    present = scene.present
    zones = _result_scene(scene, nearest)
    rows = _inscribed_of(zones, dist)
    pairs = _contacts(zones, len(present))
    return zone_columns(present, scene.area[present], zones.area[present], rows.cpu().numpy()[present], *pairs,
                        _edge_faces(nearest, scene)[present], scene.spatial)


def expand_stage(inference_config, source, output=None, distance=None, neighbours=False, limit=None) -> None:
    """For every sample and bandwidth of ``source``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (``segment()``'s nuclei, say): with ``output=NAME`` and ``distance=D``
    ``expand_labels(labels, D)`` into a new uint16 dataset NAME of that container (the cells); with ``neighbours=True``
    ``zone_table``'s two tables of all samples (``limit``: how far a zone reaches at most; None: no limit) as
    ``zones_bandwidth-<b>.csv`` and ``zone_pairs_bandwidth-<b>.csv`` in the working directory -- a header line, then ``sample``
    and the table's columns, floats as ``%.17g``; the pair file has the pairs of two zones (``label_a > 0``).  At least one of
    the two is asked for.  Rank 0 works alone under torch.distributed."""
    who = "expand_stage"
    if not isinstance(source, str) or not source:
        raise ValueError(f"{who}: source must be the name of a dataset, got {source!r}")
    if output is None and not neighbours:
        raise ValueError(f"{who}: nothing to do: give output and distance, neighbours or both")
    if output is not None and (not isinstance(output, str) or not output or output == source):
        raise ValueError(f"{who}: output must name a new dataset other than source, got {output!r}")
    if (output is None) != (distance is None):
        raise ValueError(f"{who}: output and distance go together, got output {output!r} and distance {distance!r}")
    if limit is not None and not neighbours:
        raise ValueError(f"{who}: limit belongs to neighbours")
    _limit_sq(distance, who, "distance")
    _limit_sq(limit, who)
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    stage.open("a" if output else "r", source)
    if output is not None:
        stage.refuse_existing(output)
    ds_source = stage.f[source]
    ds_output = stage.create(output) if output else None

    def per_sample(sample, bandwidth):
        labels = ds_source[sample, bandwidth].astype(np.int32)
        if ds_output is not None:
            ds_output[sample, bandwidth] = expand_labels(labels, distance, stage.device).astype(np.uint16)
        return zone_table(labels, limit, stage.device) if neighbours else ()

    stage.run(per_sample, ("zones", "zone_pairs") if neighbours else (), keep={"zone_pairs": lambda pairs: pairs["label_a"] > 0})


if __name__ == "__main__":
    from .cli import expand as _command

    _command()
