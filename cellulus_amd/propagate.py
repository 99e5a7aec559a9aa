"""``propagate`` stage: what gives every nucleus its TERRITORY inside a foreground -- seeds grown only through allowed pixels,
the border between two seeds following the image, so that a bright membrane or a dark gap stops the growth early and nothing
leaks across background (CellProfiler's IdentifySecondaryObjects "Propagation", its default; ``skimage.segmentation.watershed(
image, markers, mask=...)``).  Those are serial priority-queue floods on the host whose result depends on the queue's order
among equal costs.  Here the result is a function of the inputs alone, from exact integers, for all objects in one sequence of
calls on the device (``csrc/label_propagate.hip``: ``clx_label_propagate``).  ``expand_labels`` grows by Euclidean distance,
straight through background; the two compose through the mask.

Definitions.  The inputs are three maps of one 2-D or 3-D shape.  ``seeds``: int32 labels; a pixel with ``0 < seeds[p] < nid`` is
a SEED pixel.  ``mask``: uint8, or absent (all allowed); a non-seed pixel is ALLOWED iff ``mask[p] != 0``; seed pixels are always
sources and keep their label, in or out of the mask.  ``weight``: int32 in ``[0, 65535]``, or absent (flat): the image in grey
levels.  NEIGHBOURS are the 8 (2-D) or 26 (3-D) pixels around ``p`` inside the map; rows and slices never wrap.  A STEP goes
from ``p`` to a neighbour ``q`` that is an allowed non-seed pixel and costs ``reg * a(p, q) + |weight[p] - weight[q]|``, ``a`` = 3
for a face neighbour, 4 for an edge neighbour, 5 for a corner neighbour (the <3, 4, 5> chamfer), ``reg`` an integer in
``[0, 65535]``.  A PATH starts at a seed pixel and makes steps; its cost is their sum.  Every pixel holds the KEY ``(cost, id)``
of its best path: the smaller cost wins, among equal costs the smaller seed id; ``cost[p]`` and ``owner[p]`` are that key.  A
seed pixel has cost 0 and its own label.  Paths costlier than ``limit`` (in ``[0, 2^30)``; None: ``2^30 - 1``) do not exist; a
pixel that no path reaches has ``owner 0`` and ``cost COST_INF = 2^30``.  Zero-cost steps are legal (``reg = 0``, flat image) and
the definition still has one answer: a key only grows along a path, so the minimum over paths is the unique least fixed point
of ``key[q] = min(key[q], key[p] + step(p, q))``.  It follows that the transposed inputs give the transposed result, that the
result with limit L is the unlimited one with every pixel of ``cost > L`` cleared, and that a monotone renumbering of the ids
renumbers the owners.

    python -m cellulus_amd.propagate infer.toml --seeds NAME --output NAME [--mask NAME] [--channel K [--levels 256]]
                                                [--regularisation 1] [--limit COST]

writes ``propagate_labels`` of every sample and bandwidth of the seeds into a new dataset of the segmentation container and
``propagate_bandwidth-<b>.csv``, one row per seed label, next to the measure stage's files.
"""

import numbers

import numpy as np
import torch

from . import _clx, _stage
from .measure import (LABELS_OUT_OF_RANGE, ROUNDS_PER_CALL, _check_map, _device_mask, _in_type_of, _inscribed_of, _result_scene, _scene,
                      _settle, _workspace)
from .measure_columns import DIST_INF, _exact_div, _extents, _raster_columns

COST_INF = DIST_INF                     # CLX_COST_INF: the cost of a pixel that no path reaches
MAX_WEIGHT = 65535                      # clx_label_propagate: weight and reg lie in [0, 65535]
_WEIGHT_OUT_OF_RANGE = f"{{who}}: weight must lie in [0, {MAX_WEIGHT}]"


def _integer(value, who, name, top, none=None):
    """an integer in [0, top] (``none`` for None where that is given)"""
    if value is None and none is not None:
        return none
    if isinstance(value, bool) or not isinstance(value, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: {name} must be an integer{'' if none is None else ' or None'}, got {type(value).__name__}")
    if not 0 <= int(value) <= top:
        raise ValueError(f"{who}: {name} must lie in [0, {top}], got {value!r}")
    return int(value)


def image_levels(image, levels=256, value_range=None, where=None):
    """``image`` (an array or a tensor of real numbers) in grey levels, an int32 array of its shape:
    ``min(levels - 1, floor((v - lo) * levels / (hi - lo)))`` in float64, ``lo`` and ``hi`` the smallest and the largest value
    under ``where`` (anything ``!= 0`` makes boolean; default: everywhere) or ``value_range = (lo, hi)``; values outside the range
    go to the nearest level.  ``lo == hi`` gives all zeros.  ``levels`` lies in [2, 65536].  Non-finite values under ``where``
    raise ValueError; elsewhere they become level 0.  An integer image with ``value_range=(0, levels)`` comes back unchanged.
    Host only."""
    who = "image_levels"
    if isinstance(levels, bool) or not isinstance(levels, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: levels must be an integer, got {type(levels).__name__}")
    if not 2 <= levels <= MAX_WEIGHT + 1:
        raise ValueError(f"{who}: levels must lie in [2, {MAX_WEIGHT + 1}], got {levels!r}")
    values = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if values.dtype.kind not in "uif":
        raise TypeError(f"{who}: image must be real numbers, got {values.dtype}")
    values = values.astype(np.float64)
    inside = np.ones(values.shape, bool) if where is None else (where.detach().cpu().numpy() if torch.is_tensor(where) else np.asarray(where)) != 0
    if inside.shape != values.shape:
        raise ValueError(f"{who}: where has shape {inside.shape}, image {values.shape}")
    if not np.isfinite(values[inside]).all():
        raise ValueError(f"{who}: image has non-finite values under where")
    if value_range is not None:
        lo, hi = (float(v) for v in value_range)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"{who}: value_range must be finite with lo <= hi, got {value_range!r}")
    elif inside.any():
        lo, hi = float(values[inside].min()), float(values[inside].max())
    else:
        lo = hi = 0.0
    if lo == hi:
        return np.zeros(values.shape, dtype=np.int32)
    finite = np.where(np.isfinite(values), values, lo)
    level = np.floor((finite - lo) * levels / (hi - lo))
    return np.clip(level, 0, levels - 1).astype(np.int32)


def _same_shape(other, seeds, who, name):
    if not torch.is_tensor(other) and not isinstance(other, np.ndarray):
        raise TypeError(f"{who}: {name} must be an array or a tensor, got {type(other).__name__}")
    if tuple(other.shape) != tuple(seeds.shape):
        raise ValueError(f"{who}: {name} has shape {tuple(other.shape)}, seeds {tuple(seeds.shape)}")


def _check_inputs(seeds, mask, weight, regularisation, limit, who):
    """the checks that need no device -> (reg, limit as the library takes it)"""
    reg = _integer(regularisation, who, "regularisation", MAX_WEIGHT)
    limit = _integer(limit, who, "limit", COST_INF - 1, none=-1)
    _check_map(seeds, who)
    if mask is not None:
        _same_shape(mask, seeds, who, "mask")
    if weight is not None:
        _same_shape(weight, seeds, who, "weight")
        if ((weight.dtype.is_floating_point or weight.dtype.is_complex or weight.dtype == torch.bool) if torch.is_tensor(weight)
                else weight.dtype.kind not in "ui"):
            raise TypeError(f"{who}: weight must be integers, got {weight.dtype}")
        if not torch.is_tensor(weight) and weight.size and (int(weight.min()) < 0 or int(weight.max()) > MAX_WEIGHT):
            raise ValueError(_WEIGHT_OUT_OF_RANGE.format(who=who))
    return reg, limit


def _device_weight(weight, device, who):
    if weight is None:
        return None
    if torch.is_tensor(weight):
        w = weight.to(device)
        if w.numel() and (int(w.min()) < 0 or int(w.max()) > MAX_WEIGHT):
            raise ValueError(_WEIGHT_OUT_OF_RANGE.format(who=who))
        return w.to(torch.int32).contiguous().reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(weight).astype(np.int32)).to(device).reshape(-1)


def _propagate(scene, mask_d, weight_d, reg, limit):
    """the clx_label_propagate calls of one map (``_settle``) -> (owner, cost), flat int32 device tensors"""
    npix = scene.lab.numel()
    workspace, nbytes = _workspace(scene, "clx_label_propagate_workspace", scene.nd, scene.Z, scene.Y, scene.X)
    owner = torch.empty(npix, dtype=torch.int32, device=scene.device)
    cost = torch.empty(npix, dtype=torch.int32, device=scene.device)
    _settle(scene, lambda resume, info: _clx.call(
        "clx_label_propagate", _clx.ptr(scene.lab), _clx.ptr(mask_d), _clx.ptr(weight_d), scene.nd, scene.Z, scene.Y, scene.X,
        scene.nid, reg, limit, ROUNDS_PER_CALL, resume, _clx.ptr(owner), _clx.ptr(cost), _clx.ptr(info), _clx.ptr(workspace), nbytes,
        _clx.stream_ptr(scene.device)),
        {1: LABELS_OUT_OF_RANGE.format(who=scene.who), 2: _WEIGHT_OUT_OF_RANGE.format(who=scene.who)}, "relaxation")
    return owner, cost


def _front(seeds, mask, weight, regularisation, limit, device, who):
    """the host checks, the scene of the seeds and the maps of one propagation (None for a map without pixels or seeds)
    -> (scene, (owner, cost) or None, the mask on the device or None)"""
    reg, limit = _check_inputs(seeds, mask, weight, regularisation, limit, who)
    scene = _scene(seeds, device, who)
    if scene.lab.numel() == 0 or scene.nid == 1:
        return scene, None, None
    mask_d = _device_mask(mask, scene.device)
    return scene, _propagate(scene, mask_d, _device_weight(weight, scene.device, who), reg, limit), mask_d


def geodesic_owner(seeds, mask=None, weight=None, regularisation=1, limit=None, device=None):
    """For every pixel the seed that reaches it on the cheapest path inside ``mask`` and that path's cost: ``(owner, cost)``,
    int32 DEVICE tensors in the shape of ``seeds``.  ``seeds``: 2-D or 3-D integers, array or device tensor (the same types and
    range as ``region_table``); ``mask``: anything of that shape that ``!= 0`` makes boolean, or None (all allowed); ``weight``:
    integers in [0, 65535] of that shape (``image_levels`` makes them), or None (flat); ``regularisation``: the integer ``reg``
    in [0, 65535], the price of distance against the price of a grey level; ``limit``: an integer cost in [0, 2^30) beyond which
    no path exists, or None.  The module's docstring has the definitions.  A pixel that no path reaches has ``owner 0`` and
    ``cost COST_INF``; a map without seeds has them everywhere.  A function of the inputs alone: the same bits in every run,
    and the transposed inputs give the transposed result.  Runs on a HIP device; there is no CPU path."""
    scene, maps, _ = _front(seeds, mask, weight, regularisation, limit, device, "geodesic_owner")
    if maps is None:
        return (torch.zeros(scene.spatial, dtype=torch.int32, device=scene.device),
                torch.full(scene.spatial, COST_INF, dtype=torch.int32, device=scene.device))
    return maps[0].reshape(scene.spatial), maps[1].reshape(scene.spatial)


def _weight_of(seeds, mask, image, levels, value_range, who):
    """``image`` in grey levels over the mask united with the seed pixels (None stays None)"""
    if image is None:
        return None
    _check_map(seeds, who)
    _same_shape(image, seeds, who, "image")
    host = (lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
    where = host(seeds) > 0
    if mask is not None:
        _same_shape(mask, seeds, who, "mask")
        where = where | (host(mask) != 0)
    else:
        where = np.ones(where.shape, bool)
    return image_levels(image, levels, value_range, where)


def propagate_labels(seeds, mask=None, image=None, levels=256, value_range=None, regularisation=1, limit=None, device=None):
    """``seeds`` grown inside ``mask`` along the cheapest paths of ``image``: every allowed pixel a path reaches takes the label
    of the seed with the smallest ``(cost, id)``; seeds keep their pixels; the rest is 0.  ``image`` (real numbers in the shape of
    ``seeds``, or None: a flat image, the growth is the <3, 4, 5> chamfer distance inside the mask) goes through
    ``image_levels(image, levels, value_range, where=the mask united with the seed pixels)``; the other arguments are
    ``geodesic_owner``'s.  The result has the type, dtype and device of ``seeds``.  With ``mask = cells > 0`` the territories are
    the cells of the nuclei: ``relate`` assigns the nuclei to them.  Runs on a HIP device; there is no CPU path."""
    who = "propagate_labels"
    weight = _weight_of(seeds, mask, image, levels, value_range, who)
    scene, maps, _ = _front(seeds, mask, weight, regularisation, limit, device, who)
    return _in_type_of(seeds, scene, None if maps is None else maps[0])


def propagate_columns(label, seed_area, area, rows, unreached, shape):
    """The table of ``propagate_table`` from integers.  ``label`` (n): the seed labels present, ascending; ``seed_area`` (n) the
    pixels of the seeds, ``area`` (n) those of their territories (``clx_region_moments`` of the seeds and of the owner map);
    ``rows`` (n, 3): ``clx_region_inscribed``'s rows ``largest cost, index, Σcost`` of the owner map and the costs;
    ``unreached``: the allowed pixels that no seed reached; ``shape`` the map's 2 or 3 extents.  Columns: ``label``,
    ``seed_area``, ``area``, ``reach_cost`` (the largest cost inside the territory), ``reach_z/_y/_x`` (2-D: y and x; the first
    pixel in raster order that attains it), ``cost_mean`` (one correctly rounded division of exact integers) and ``unreached``
    (the same number in every row); int64 but ``cost_mean``.  Host only."""
    who = "propagate_columns"
    _extents(shape, who)
    label, seed_area, area = (np.asarray(v).astype(np.int64).reshape(-1) for v in (label, seed_area, area))
    n = len(label)
    rows = [[int(v) for v in r] for r in np.asarray(rows).reshape(-1, 3)]
    if not len(seed_area) == len(area) == len(rows) == n:
        raise ValueError(f"{who}: seed_area, area and rows must have one row per label")
    if n and (np.any(np.diff(label) <= 0) or label[0] < 1 or seed_area.min() < 1 or np.any(area < seed_area)):
        raise ValueError(f"{who}: needs increasing labels >= 1 with 1 <= seed_area <= area")
    if any(r[0] >= COST_INF or r[1] >= int(np.prod(shape)) for r in rows):
        raise ValueError(f"{who}: a row of the reach lies outside a map of shape {tuple(shape)}")
    unreached = int(unreached)
    if unreached < 0:
        raise ValueError(f"{who}: unreached must be >= 0, got {unreached}")
    table = {"label": label, "seed_area": seed_area, "area": area, "reach_cost": np.array([r[0] for r in rows], dtype=np.int64)}
    table.update(_raster_columns("reach", np.array([r[1] for r in rows], dtype=np.int64), shape, who))
    table["cost_mean"] = _exact_div([r[2] for r in rows], area.astype(object))
    table["unreached"] = np.full(n, unreached, dtype=np.int64)
    return table


def _table(scene, maps, mask_d):
    """``propagate_columns`` of a propagation (``_front``'s results)"""
    scene.measured()
    if maps is None or scene.empty:
        none = np.zeros(0, dtype=np.int64)
        return propagate_columns(none, none, none, np.zeros((0, 3), dtype=np.int64), 0, scene.spatial)
    owner, cost = maps
    present = scene.present
    grown = _result_scene(scene, owner)
    rows = _inscribed_of(grown, cost)
    nobody = owner == 0
    unreached = int((nobody if mask_d is None else nobody & (mask_d != 0)).sum().item())
    return propagate_columns(present, scene.area[present], grown.area[present], rows.cpu().numpy()[present], unreached, scene.spatial)


def propagate_table(seeds, mask=None, image=None, levels=256, value_range=None, regularisation=1, limit=None, device=None):
    """The table of the territories ``propagate_labels`` gives the seeds (its arguments), one row per seed label present:
    ``propagate_columns`` lists the columns.  A map without seeds gives an empty table with these columns.  Runs on a HIP
    device; there is no CPU path."""
    who = "propagate_table"
    weight = _weight_of(seeds, mask, image, levels, value_range, who)
    return _table(*_front(seeds, mask, weight, regularisation, limit, device, who))


def propagate_stage(inference_config, seeds, output, mask=None, channel=None, levels=256, regularisation=1, limit=None) -> None:
    """For every sample and bandwidth of ``seeds``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (the nuclei): ``propagate_labels`` of it into a new uint16 dataset ``output`` of
    that container and ``propagate_table``'s rows of all samples as ``propagate_bandwidth-<b>.csv`` in the working directory -- a
    header line, then ``sample`` and the table's columns, floats as ``%.17g``.  ``mask``: the name of a dataset of that shape in
    the container whose non-zero pixels are allowed (``segment()``'s label map, say), or None; ``channel``: the channel of the
    raw dataset that is the image, in ``levels`` grey levels between its smallest and largest value under the mask and the
    seeds, or None (flat).  Rank 0 works alone under torch.distributed."""
    from .utils import zarr_io

    who = "propagate_stage"
    if not isinstance(seeds, str) or not seeds:
        raise ValueError(f"{who}: seeds must be the name of a dataset, got {seeds!r}")
    if not isinstance(output, str) or not output or output == seeds or output == mask:
        raise ValueError(f"{who}: output must name a new dataset other than seeds, got {output!r}")
    if mask is not None and (not isinstance(mask, str) or not mask):
        raise ValueError(f"{who}: mask must be the name of a dataset or None, got {mask!r}")
    if channel is not None and (isinstance(channel, bool) or not isinstance(channel, (numbers.Integral, np.integer)) or channel < 0):
        raise ValueError(f"{who}: channel must be an integer >= 0 or None, got {channel!r}")
    _integer(levels, who, "levels", MAX_WEIGHT + 1)
    if levels < 2:
        raise ValueError(f"{who}: levels must lie in [2, {MAX_WEIGHT + 1}], got {levels!r}")
    _integer(regularisation, who, "regularisation", MAX_WEIGHT)
    _integer(limit, who, "limit", COST_INF - 1, none=-1)
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    stage.open("a", seeds, mask)
    stage.refuse_existing(output)
    ds_raw = None
    if channel is not None:
        dataset_config = inference_config.dataset_config
        ds_raw = zarr_io.open(dataset_config.container_path, "r")[dataset_config.dataset_name]
        if channel >= ds_raw.shape[1]:
            raise ValueError(f"{who}: no channel {channel} in a raw dataset of {ds_raw.shape[1]} channels")
    ds_seeds, ds_mask = stage.f[seeds], stage.f[mask] if mask is not None else None
    ds_output = stage.create(output)

    def per_sample(sample, bandwidth):
        labels = ds_seeds[sample, bandwidth].astype(np.int32)
        allowed = None if ds_mask is None else np.asarray(ds_mask[sample, bandwidth]) != 0
        image = None if ds_raw is None else np.asarray(ds_raw[sample][channel])
        weight = _weight_of(labels, allowed, image, levels, None, who)
        scene, maps, mask_d = _front(labels, allowed, weight, regularisation, limit, stage.device, who)
        ds_output[sample, bandwidth] = _in_type_of(labels, scene, None if maps is None else maps[0]).astype(np.uint16)
        return (_table(scene, maps, mask_d),)

    stage.run(per_sample, ("propagate",))


if __name__ == "__main__":
    from .cli import propagate as _command

    _command()
