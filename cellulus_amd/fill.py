"""``fill`` stage: what REPAIRS the holes of the label map a segmentation handed over -- mean-shift drops every pixel whose
embedding is uncertain, so ``segment()``'s objects come out with pinholes, which ``region_table(topology=True)`` counts,
``label_distance_sq`` sees as boundary (``inscribed_radius``, the radial rings, ``--clearance``) and ``split_labels`` cuts false
necks around.  CellProfiler's FillObjects and "fill holes" of IdentifyPrimaryObjects (centrosome's ``fill_labeled_holes``) and
``scipy.ndimage.binary_fill_holes`` per object are floods on the host; here all objects are repaired in one call on the device
(``csrc/label_holes.hip``: ``clx_label_holes``), which also lists the holes.  ``fill -> split -> measure`` is a chain.

Definitions.  The input is one map, 2-D or 3-D.  Every non-zero value is an OBJECT pixel; value 0 is BACKGROUND.  Background
pixels are FACE neighbours (4 in 2-D, 6 in 3-D): the complement of the 8 / 26-connectivity the objects have; rows and slices
never wrap.  A COMPONENT is a maximal face-connected set of background pixels.  With ``planewise`` (3-D only) z neighbours do
not exist and every slice is a 2-D map of its own: CellProfiler's planewise fill, the useful mode for stacks whose cavities are
open along z.  A component REACHES THE BORDER iff one of its pixels has ``x in {0, X-1}`` or ``y in {0, Y-1}``; in 3-D without
planewise, ``z in {0, Z-1}`` counts as well.  A component is a HOLE of label L iff it does not reach the border and every object
pixel that is a face neighbour of one of its pixels carries the same value L; edge and corner neighbours do not count
("surrounded by a single object").  A gap that touches two labels is not a hole and stays background; so does a ring between an
object and a different object nested inside it.  A hole's FIRST pixel is its smallest raster index, its AREA its pixel count.
The repaired map has L on the pixels of every hole of L with ``area <= max_size`` (None: no cap) and is equal to the input
elsewhere; ``max_size = 0`` changes nothing and makes the call a census.  The pixels filled are always a subset of the union
over L of ``binary_fill_holes(labels == L) & (labels == 0)``, and equal to it on every map in which no enclosed background
component touches a second label.

    python -m cellulus_amd.fill infer.toml --source NAME --output NAME [--max-size N] [--planewise]

writes ``fill_holes`` of every sample and bandwidth of ``NAME`` into a new dataset of the segmentation container and
``fill_bandwidth-<b>.csv``, one row per label, and ``holes_bandwidth-<b>.csv``, one row per hole, next to the measure stage's
files.
"""

import numbers

import numpy as np
import torch

from . import _clx, _stage
from .measure import _check_map, _in_type_of, _result_scene, _scene, _workspace
from .measure_columns import _extents, _raster_columns

MAX_HOLES = (1 << 31) - 1               # clx_label_holes: capacity is an int


def _max_size(max_size, who):
    """``max_size`` as the library takes it: an integer >= 0, -1 for None"""
    if max_size is None:
        return -1
    if isinstance(max_size, bool) or not isinstance(max_size, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: max_size must be an integer or None, got {type(max_size).__name__}")
    if not 0 <= int(max_size) < 1 << 63:
        raise ValueError(f"{who}: max_size must lie in [0, 2^63), got {max_size!r}")
    return int(max_size)


def _planewise(planewise, nd, who):
    if not isinstance(planewise, (bool, np.bool_)):
        raise TypeError(f"{who}: planewise must be a bool, got {type(planewise).__name__}")
    if planewise and nd == 2:
        raise ValueError(f"{who}: planewise needs a 3-D map")
    return int(bool(planewise))


def hole_columns(first, owner, area, kept, shape):
    """The table of ``hole_table`` from ``clx_label_holes``' rows, one row per hole in the order given: ``owner`` (the label
    around the hole), ``first_z/_y/_x`` (2-D: y and x; the hole's first pixel in raster order), ``area`` and ``filled`` (0: the
    hole exceeded ``max_size`` and was left open); int64.  ``shape`` is the map's 2 or 3 extents.  Host only."""
    who = "hole_columns"
    _extents(shape, who)
    first, owner, area, kept = (np.asarray(v).astype(np.int64).reshape(-1) for v in (first, owner, area, kept))
    n = len(first)
    if not len(owner) == len(area) == len(kept) == n:
        raise ValueError(f"{who}: first, owner, area and kept must have one row per hole")
    if n and (first.min() < 0 or first.max() >= int(np.prod(shape)) or area.min() < 1 or np.any(owner == 0) or np.any((kept != 0) & (kept != 1))):
        raise ValueError(f"{who}: needs first pixels inside a map of shape {tuple(shape)}, owners != 0, area >= 1 and kept in {{0, 1}}")
    return {"owner": owner, **_raster_columns("first", first, shape, who), "area": area, "filled": 1 - kept}


def fill_columns(label, area_before, owner, hole_area, kept):
    """The table of ``fill_table`` from integers.  ``label`` (n): the labels present, ascending; ``area_before`` (n): their
    pixels in the input; ``owner``, ``hole_area`` and ``kept`` (m): ``clx_label_holes``' rows, in any order.  Columns: ``label``,
    ``area_before``, ``area = area_before + filled_area``, ``holes_filled``, ``filled_area`` (the pixels of the holes filled),
    ``largest_hole`` (the largest area among the label's holes, filled or kept; 0: it has none) and ``holes_kept`` (the holes
    larger than ``max_size``, left open); int64.  Host only."""
    who = "fill_columns"
    label, area_before = (np.asarray(v).astype(np.int64).reshape(-1) for v in (label, area_before))
    owner, hole_area, kept = (np.asarray(v).astype(np.int64).reshape(-1) for v in (owner, hole_area, kept))
    n = len(label)
    if len(area_before) != n:
        raise ValueError(f"{who}: label and area_before must have one row per label")
    if not len(owner) == len(hole_area) == len(kept):
        raise ValueError(f"{who}: owner, hole_area and kept must have one row per hole")
    if n and (np.any(np.diff(label) <= 0) or np.any(label == 0) or area_before.min() < 1):
        raise ValueError(f"{who}: needs increasing labels != 0 with area_before >= 1")
    row = np.searchsorted(label, owner)
    if len(owner) and (n == 0 or row.max() >= n or np.any(label[row] != owner) or hole_area.min() < 1 or np.any((kept != 0) & (kept != 1))):
        raise ValueError(f"{who}: a hole needs an owner among the labels, area >= 1 and kept in {{0, 1}}")
    filled = kept == 0
    holes_filled = np.bincount(row[filled], minlength=n).astype(np.int64)
    filled_area = np.zeros(n, dtype=np.int64)
    np.add.at(filled_area, row[filled], hole_area[filled])
    largest = np.zeros(n, dtype=np.int64)
    np.maximum.at(largest, row, hole_area)
    return {"label": label, "area_before": area_before, "area": area_before + filled_area, "holes_filled": holes_filled,
            "filled_area": filled_area, "largest_hole": largest, "holes_kept": np.bincount(row[~filled], minlength=n).astype(np.int64)}


def _holes(scene, max_size, planewise):
    """one clx_label_holes call (a second one, with exactly the capacity the first asked for, where the first list was too
    short) -> (the repaired map, flat int32 on the device; the rows (first, owner, area, kept), int64 (n, 4) sorted by first, on
    the host; info as a list)"""
    npix = scene.lab.numel()
    workspace, nbytes = _workspace(scene, "clx_label_holes_workspace", scene.nd, scene.Z, scene.Y, scene.X, below="2^31")
    out = torch.empty(npix, dtype=torch.int32, device=scene.device)
    info = torch.empty(4, dtype=torch.int32, device=scene.device)
    capacity = min(npix, max(1024, npix // 64))
    while True:
        rows = torch.empty((capacity, 4), dtype=torch.int32, device=scene.device)
        _clx.call("clx_label_holes", _clx.ptr(scene.lab), scene.nd, scene.Z, scene.Y, scene.X, planewise, max_size, capacity, _clx.ptr(out),
                  _clx.ptr(rows), _clx.ptr(info), _clx.ptr(workspace), nbytes, _clx.stream_ptr(scene.device))
        found = info.tolist()
        if found[0] <= capacity:
            break
        capacity = found[0]                                   # the count is exact: the second list fits
    rows = rows[:found[0]].cpu().numpy().astype(np.int64)
    return out, rows[np.argsort(rows[:, 0], kind="stable")], found


def _fill(labels, max_size, planewise, device, who, tables=False):
    """-> (scene, the repaired map as a flat int32 device tensor or None for a map the library was not called for, and with
    ``tables`` (hole_columns, fill_columns) of it; ``tables="holes"``: without the second, which takes the moments)"""
    max_size = _max_size(max_size, who)
    _check_map(labels, who)
    planewise = _planewise(planewise, labels.ndim, who)
    scene = _scene(labels, device, who)
    none = np.zeros(0, dtype=np.int64)
    out, rows = None, np.zeros((0, 4), dtype=np.int64)
    if scene.lab.numel() and not bool((scene.lab != 0).all()):
        out, rows, _ = _holes(scene, max_size, planewise)
    if not tables:
        return scene, out, None
    hole_table_ = hole_columns(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], scene.spatial)
    if tables == "holes":
        return scene, out, (hole_table_, None)
    scene.measured()
    if scene.empty:
        return scene, out, (hole_table_, fill_columns(none, none, none, none, none))
    present = scene.present
    table = fill_columns(present, scene.area[present], rows[:, 1], rows[:, 2], rows[:, 3])
    after = scene if out is None else _result_scene(scene, out)
    assert np.array_equal(after.area[present], table["area"]), f"{who}: area != area_before + filled_area"
    return scene, out, (hole_table_, table)


def fill_holes(labels, max_size=None, planewise=False, device=None):
    """``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as ``region_table``) with the holes of
    its objects closed: every face-connected component of background that does not reach the border and has one label L
    among its face neighbours becomes L, if it has at most ``max_size`` pixels (an integer >= 0, or None: no cap; 0 changes
    nothing).  ``planewise`` (3-D only): every slice is filled as a 2-D map of its own.  A gap between two labels and the ring
    around a nested object of another label stay open.  The result has the type, dtype and device of ``labels``.  The module's
    docstring has the definitions.  A function of the map alone: the same bits in every run.  Runs on a HIP device; there is
    no CPU path."""
    scene, out, _ = _fill(labels, max_size, planewise, device, "fill_holes")
    return _in_type_of(labels, scene, out)


def hole_table(labels, max_size=None, planewise=False, device=None):
    """The holes of ``labels`` (``fill_holes``' arguments), one row per hole sorted by its first pixel in raster order, filled or
    not: ``hole_columns`` lists the columns.  ``max_size = 0`` is a census that would fill nothing.  A first list that proves too
    short is followed by one second call with exactly the capacity needed.  Runs on a HIP device; there is no CPU path."""
    return _fill(labels, max_size, planewise, device, "hole_table", tables="holes")[2][0]


def fill_table(labels, max_size=None, planewise=False, device=None):
    """What ``fill_holes`` (its arguments) does to every object, one row per label present: ``fill_columns`` lists the columns.
    ``area_before`` and ``area`` are ``clx_region_moments`` of the map and of the repaired map; ``area == area_before +
    filled_area`` is asserted.  A map without objects gives an empty table with these columns.  Runs on a HIP device; there is
    no CPU path."""
    return _fill(labels, max_size, planewise, device, "fill_table", tables=True)[2][1]


def fill_stage(inference_config, source, output, max_size=None, planewise=False) -> None:
    """For every sample and bandwidth of ``source``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (``segment()``'s, say): ``fill_holes(labels, max_size, planewise)`` into a new
    uint16 dataset ``output`` of that container, ``fill_table``'s rows of all samples as ``fill_bandwidth-<b>.csv`` and
    ``hole_table``'s as ``holes_bandwidth-<b>.csv`` in the working directory -- a header line, then ``sample`` and the table's
    columns, floats as ``%.17g``.  Rank 0 works alone under torch.distributed."""
    who = "fill_stage"
    if not isinstance(source, str) or not source:
        raise ValueError(f"{who}: source must be the name of a dataset, got {source!r}")
    if not isinstance(output, str) or not output or output == source:
        raise ValueError(f"{who}: output must name a new dataset other than source, got {output!r}")
    _max_size(max_size, who)
    if not isinstance(planewise, (bool, np.bool_)):
        raise TypeError(f"{who}: planewise must be a bool, got {type(planewise).__name__}")
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    _planewise(planewise, stage.nd, who)
    stage.open("a", source)
    stage.refuse_existing(output)
    ds_source, ds_output = stage.f[source], stage.create(output)

    def per_sample(sample, bandwidth):
        labels = ds_source[sample, bandwidth].astype(np.int32)
        scene, out, tables = _fill(labels, max_size, planewise, stage.device, who, tables=True)
        ds_output[sample, bandwidth] = _in_type_of(labels, scene, out).astype(np.uint16)
        return tables

    stage.run(per_sample, ("holes", "fill"))


if __name__ == "__main__":
    from .cli import fill as _command

    _command()
