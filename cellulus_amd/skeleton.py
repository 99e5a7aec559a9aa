"""``skeleton`` stage: what THINS the objects of a label map to their centre lines and measures the lines -- how long an
elongated or branching object (a neurite, a filament, a hypha, a clump with necks) is along itself, how often it branches, how
many free ends it has and how wide it is along its axis.  CellProfiler's MorphologicalSkeleton / MeasureObjectSkeleton, MATLAB's
``bwmorph('thin')`` and ``skimage.morphology.thin`` work on one mask on the host; here all objects are thinned in one pass on
the device (``csrc/label_thin.hip``: ``clx_label_thin``, ``clx_skeleton_census``), label-aware.  ``fill -> skeleton`` is a
chain: a pinhole becomes a loop of the skeleton.

Definitions.  The input is one map.  Every non-zero value is an OBJECT pixel.  A 3-D map is thinned slice by slice
(``planewise=True``; 3-D curve skeletons are not done); rows and slices never wrap.  The NEIGHBOURS of a pixel p are
``P2 .. P9`` = N, NE, E, SE, S, SW, W, NW, N at ``y - 1``; ``Pk = 1`` iff that pixel lies inside the slice, is still alive and
carries p's label, so touching objects thin independently.  With

    C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
    N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),   N = min(N1, N2)

a SUB-ITERATION deletes every alive pixel with ``C == 1``, ``2 <= N <= 3`` and ``m == 0``, all at once from the state before
it; odd sub-iterations have ``m = (P2 | P3 | !P5) & P4``, even ones ``m = (P6 | P7 | !P9) & P8`` (Guo & Hall 1989, algorithm
A1).  An ITERATION is an odd, then an even sub-iteration; the SKELETON is the state after the first iteration that deletes
nothing, or after ``max_iter`` iterations.  Thinning keeps every object's 8-connected components and holes.

On the thinned map, per label: a FACE LINK is a pair of face neighbours, a DIAGONAL LINK a pair of diagonal neighbours neither
of whose two common face neighbours carries the label, a BLOCK a 2 x 2 window full of the label; the DEGREE of a pixel is the
number of its links, an END has degree 1, a BRANCH POINT (junction pixel) degree >= 3, an ISOLATED pixel degree 0.
``pixels - face_links - diag_links + blocks`` is the label's Euler number with 8-connectivity.

    python -m cellulus_amd.skeleton infer.toml --source NAME --output NAME [--max-iter N] [--planewise] [--radius]

writes ``thin_labels`` of every sample and bandwidth of ``NAME`` into a new dataset of the segmentation container and
``skeleton_bandwidth-<b>.csv``, one row per label, next to the measure stage's files.
"""

import numbers

import numpy as np
import torch

from . import _clx, _stage
from .measure import FLAGS, LABELS_OUT_OF_RANGE, _check_map, _distance_map, _in_type_of, _scene, _Scene, _workspace

CALL_ITERATIONS = 64                    # clx_label_thin: the iterations a call queues at most
CENSUS_WORDS = 10                       # clx_skeleton_census: words per label
REFUSE_3D = "{who}: 3-D thinning is not implemented; planewise=True thins every slice on its own"


def _max_iter(max_iter, who):
    if max_iter is None:
        return None
    if isinstance(max_iter, bool) or not isinstance(max_iter, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: max_iter must be an integer or None, got {type(max_iter).__name__}")
    if not 0 <= int(max_iter) < 1 << 31:
        raise ValueError(f"{who}: max_iter must lie in [0, 2^31), got {max_iter!r}")
    return int(max_iter)


def _flag(value, name, who):
    if not isinstance(value, (bool, np.bool_)):
        raise TypeError(f"{who}: {name} must be a bool, got {type(value).__name__}")
    return bool(value)


def _planewise(planewise, nd, who):
    planewise = _flag(planewise, "planewise", who)
    if planewise and nd == 2:
        raise ValueError(f"{who}: planewise needs a 3-D map")
    if nd == 3 and not planewise:
        raise ValueError(REFUSE_3D.format(who=who))
    return planewise


def skeleton_columns(label, area, words, radius=False):
    """The table of ``skeleton_table`` from integers.  ``label`` (n): the labels present, ascending; ``area`` (n): their pixels
    in the input map; ``words`` (n, 10): their rows of ``clx_skeleton_census`` on the thinned map -- pixels, face_links,
    diag_links, blocks, ends, junctions, isolated, d2_sum, d2_min, d2_max.  Columns: ``label``, ``area``, ``skeleton_pixels``,
    ``skeleton_length = face_links + sqrt(2) * diag_links`` (float64), ``skeleton_end_points``, ``skeleton_branch_points``,
    ``skeleton_isolated``, ``skeleton_euler_number = pixels - face_links - diag_links + blocks``, and with ``radius``
    ``skeleton_radius_min`` and ``skeleton_radius_max`` (the square roots of d2_min and d2_max) and ``skeleton_dist_sq_mean``
    (d2_sum / pixels), float64; a label none of whose skeleton pixels has a finite distance (``d2_max < 0``: the map is one
    object everywhere) has ``inf`` in the three.  Integers are int64.  Host only."""
    who = "skeleton_columns"
    label, area = (np.asarray(v).astype(np.int64).reshape(-1) for v in (label, area))
    words = np.asarray(words).astype(np.int64).reshape(-1, CENSUS_WORDS)
    n = len(label)
    if len(area) != n or len(words) != n:
        raise ValueError(f"{who}: label, area and words must have one row per label")
    if n and (np.any(np.diff(label) <= 0) or np.any(label == 0) or area.min() < 1 or words[:, :7].min() < 0 or np.any(words[:, 0] > area)):
        raise ValueError(f"{who}: needs increasing labels != 0 with area >= 1 and 0 <= pixels <= area")
    pixels, face, diag, blocks = words[:, 0], words[:, 1], words[:, 2], words[:, 3]
    table = {"label": label, "area": area, "skeleton_pixels": pixels,
             "skeleton_length": face.astype(np.float64) + np.sqrt(2.0) * diag.astype(np.float64),
             "skeleton_end_points": words[:, 4], "skeleton_branch_points": words[:, 5], "skeleton_isolated": words[:, 6],
             "skeleton_euler_number": pixels - face - diag + blocks}
    if _flag(radius, "radius", who):
        finite = words[:, 9] >= 0
        inf = np.full(n, np.inf)
        table["skeleton_radius_min"] = np.where(finite, np.sqrt(np.where(finite, words[:, 8], 0).astype(np.float64)), inf)
        table["skeleton_radius_max"] = np.where(finite, np.sqrt(np.where(finite, words[:, 9], 0).astype(np.float64)), inf)
        table["skeleton_dist_sq_mean"] = np.where(finite, words[:, 7].astype(np.float64) / np.maximum(pixels, 1), inf)
    return table


def _thin_map(scene, max_iter):
    """clx_label_thin calls, the first with resume = 0, until an iteration deletes nothing or ``max_iter`` iterations have run
    -> the thinned map, flat int32 on the device; None for a map the library was not called for"""
    npix = scene.lab.numel()
    if npix == 0 or max_iter == 0:
        return None
    workspace, nbytes = _workspace(scene, "clx_label_thin_workspace", scene.nd, scene.Z, scene.Y, scene.X, below="2^31")
    out = torch.empty(npix, dtype=torch.int32, device=scene.device)
    info = torch.empty(3, dtype=torch.int32, device=scene.device)
    done = 0
    while True:
        iterations = CALL_ITERATIONS if max_iter is None else min(CALL_ITERATIONS, max_iter - done)
        _clx.call("clx_label_thin", _clx.ptr(scene.lab), scene.nd, scene.Z, scene.Y, scene.X, iterations, int(done > 0), _clx.ptr(out),
                  _clx.ptr(info), _clx.ptr(workspace), nbytes, _clx.stream_ptr(scene.device))
        done += iterations
        if info.tolist()[1] == 0 or (max_iter is not None and done >= max_iter):
            return out


def _distance_slices(scene):
    """``label_distance_sq`` of the scene's map with the default edge convention, every slice on its own -> flat int32 on the
    device"""
    if scene.nd == 2:
        return _distance_map(scene, False)
    plane = scene.Y * scene.X
    return torch.cat([_distance_map(_Scene(scene.who, scene.lab[z * plane:(z + 1) * plane], scene.device, 2, scene.spatial[1:], scene.nid),
                                    False) for z in range(scene.Z)])


def _skeleton(labels, max_iter, planewise, radius, device, who, table=False):
    """-> (scene, the thinned map as a flat int32 device tensor or None for a map the library was not called for, and with
    ``table`` the ``skeleton_columns`` of it)"""
    max_iter = _max_iter(max_iter, who)
    _check_map(labels, who)
    _planewise(planewise, labels.ndim, who)
    radius = _flag(radius, "radius", who)
    scene = _scene(labels, device, who)
    out = _thin_map(scene, max_iter)
    if not table:
        return scene, out, None
    scene.measured()
    if scene.empty:
        none = np.zeros(0, dtype=np.int64)
        return scene, out, skeleton_columns(none, none, np.zeros((0, CENSUS_WORDS), dtype=np.int64), radius)
    words = scene.ids(CENSUS_WORDS)
    # (bit 1, a pixel without a finite distance, is no error: skeleton_columns reports inf)
    scene.call("clx_skeleton_census", {1: LABELS_OUT_OF_RANGE}, scene.lab if out is None else out, _distance_slices(scene) if radius else None,
               scene.nd, scene.Z, scene.Y, scene.X, scene.nid, words, FLAGS)
    present = scene.present
    return scene, out, skeleton_columns(present, scene.area[present], words.cpu().numpy()[present], radius)


def thin_labels(labels, max_iter=None, planewise=False, device=None):
    """``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as ``region_table``) with every object
    thinned to its centre lines: the state after the first iteration that deletes nothing, or after ``max_iter`` iterations (an
    integer >= 0, or None: to the end; 0 changes nothing).  A 3-D map needs ``planewise=True``: every slice is thinned as a 2-D
    map of its own.  Objects that touch thin independently.  The result has the type, dtype and device of ``labels``.  The
    module's docstring has the definitions.  A function of the map alone: the same bits in every run.  Runs on a HIP device;
    there is no CPU path."""
    scene, out, _ = _skeleton(labels, max_iter, planewise, False, device, "thin_labels")
    return _in_type_of(labels, scene, out)


def skeleton_table(labels, max_iter=None, planewise=False, radius=False, device=None):
    """The skeleton of every object of ``labels`` (``thin_labels``' arguments) measured, one row per label present:
    ``skeleton_columns`` lists the columns.  ``area`` is ``clx_region_moments`` of the input map.  With ``radius`` the distance
    map is ``label_distance_sq`` of the INPUT map (of every slice on its own when planewise) with the edge convention
    ``region_table(inscribed=True)`` has by default.  A map without objects gives an empty table with these columns.  Runs on a
    HIP device; there is no CPU path."""
    return _skeleton(labels, max_iter, planewise, radius, device, "skeleton_table", table=True)[2]


def skeleton_stage(inference_config, source, output, max_iter=None, planewise=False, radius=False) -> None:
    """For every sample and bandwidth of ``source``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (``segment()``'s, say): ``thin_labels(labels, max_iter, planewise)`` into a
    new uint16 dataset ``output`` of that container and ``skeleton_table``'s rows of all samples as
    ``skeleton_bandwidth-<b>.csv`` in the working directory -- a header line, then ``sample`` and the table's columns, floats
    as ``%.17g``.  Rank 0 works alone under torch.distributed."""
    who = "skeleton_stage"
    if not isinstance(source, str) or not source:
        raise ValueError(f"{who}: source must be the name of a dataset, got {source!r}")
    if not isinstance(output, str) or not output or output == source:
        raise ValueError(f"{who}: output must name a new dataset other than source, got {output!r}")
    _max_iter(max_iter, who)
    _flag(planewise, "planewise", who)
    _flag(radius, "radius", who)
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    _planewise(planewise, stage.nd, who)
    stage.open("a", source)
    stage.refuse_existing(output)
    ds_source, ds_output = stage.f[source], stage.create(output)

    def per_sample(sample, bandwidth):
        labels = ds_source[sample, bandwidth].astype(np.int32)
        scene, out, table = _skeleton(labels, max_iter, planewise, radius, stage.device, who, table=True)
        ds_output[sample, bandwidth] = _in_type_of(labels, scene, out).astype(np.uint16)
        return (table,)

    stage.run(per_sample, ("skeleton",))


if __name__ == "__main__":
    from .cli import skeleton as _command

    _command()
