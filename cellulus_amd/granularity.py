"""``granularity`` stage: the SIZE SPECTRUM of the bright structure inside every object -- speckles, granules, nucleoli --
CellProfiler's MeasureGranularity, and the grey-scale morphology it stands on: erosion, dilation, opening, top-hat and
reconstruction by dilation of an image in grey levels (``skimage.morphology.erosion`` / ``dilation`` / ``reconstruction``, which
are serial on the host; reconstruction is a queue flood there).  Here reconstruction is the least fixed point of a monotone
integer update, so a function of the inputs alone, reached in rounds on the device (``csrc/grey_morph.hip``: ``clx_grey_morph``,
``clx_grey_reconstruct``); the sums per object are ``clx_region_intensity``'s exact integers.

Definitions.  All maps have one 2-D or 3-D shape and hold grey levels, integers in ``[0, 65535]`` (``propagate.image_levels``
makes them).  ``mask``: anything that ``!= 0`` makes boolean, or None; a pixel with ``mask[p] == 0`` is OUTSIDE, and so is
everything beyond the map; rows and slices never wrap.  NEIGHBOURS are the 4 (2-D) or 6 (3-D) face neighbours, CellProfiler's
footprint, the disc of radius 1.  One STEP of erosion (dilation) gives every inside pixel the min (max) over itself and its
inside neighbours; k steps are the step k times: the min (max) over the inside pixels within k face steps through inside pixels,
without a mask the L1 ball (a diamond) of radius k.  Outside pixels get 0.  OPENING is k steps of erosion, then k of dilation;
the white TOP-HAT is the image minus its opening, never negative.  The RECONSTRUCTION by dilation of ``marker`` under ``image``
is, with ``m = min(marker, image)``, the least map ``r >= m`` with ``r[p] = min(image[p], max(r[p], r[neighbours of p]))``:
``r[p]`` is the maximum over the face paths of inside pixels from some ``q`` to ``p`` of ``min(m[q], the smallest image value on
the path)``.  Hence ``m <= r <= image``, reconstructing ``r`` again changes nothing, ``r`` is monotone in ``marker``, and the
transposed inputs give the transposed result.

The GRANULAR SPECTRUM of a channel with ``scales = n`` and ``background = R``: ``g`` is the channel in grey levels; with ``R > 0``
``g`` becomes its top-hat of radius ``R``; ``e_0 = r_0 = g``, ``e_i`` is one step of erosion of ``e_(i-1)`` and ``r_i`` the
reconstruction of ``e_i`` under ``g``; ``S_i[id]`` is the sum of ``r_i`` over the object's pixels, an exact integer.  The
columns are ``granularity_<i>_c<k> = 100 (S_(i-1) - S_i) / S_0`` for ``i = 1 .. n``, all ``>= 0``, and
``granularity_residual_c<k> = 100 S_n / S_0``: a row sums to 100 up to rounding; NaN where ``S_0 == 0``.  This is CellProfiler's
loop -- erode, reconstruct, take the mean -- on the stored image: scale ``i`` is a diamond of radius ``i`` pixels.  Its
subsampling of image and background is not done, and its background is removed with a disc where this one uses the diamond.

    python -m cellulus_amd.granularity infer.toml --source NAME [--channel K] [--scales 16] [--levels 256] [--background R]

writes ``granularity_bandwidth-<b>.csv``, one row per label of every sample and bandwidth of ``NAME``, next to the measure stage's
files.
"""

import numbers

import numpy as np
import torch

from . import _clx, _stage
from .measure import (FLAGS, LABELS_CHANGED, ROUNDS_PER_CALL, _check_map, _device_mask, _in_type_of, _resolve_device, _scene, _Scene,
                      _settle, _workspace)
from .measure_columns import _exact_div
from .propagate import image_levels

MAX_LEVEL = 65535                       # clx_grey_morph / clx_grey_reconstruct: values lie in [0, 65535]
MORPH_STEPS = {2: 16, 3: 4}             # clx_grey_morph: the steps of one call, by the map's dimensions
MAX_SCALES, MAX_BACKGROUND = 64, 64
_RAW_I32 = 2                            # CLX_RAW_I32: clx_region_intensity sums the values as they are
_OUT_OF_RANGE = f"{{who}}: {{name}} must lie in [0, {MAX_LEVEL}]"


def _int_in(value, who, name, low, top):
    if isinstance(value, bool) or not isinstance(value, (numbers.Integral, np.integer)):
        raise TypeError(f"{who}: {name} must be an integer, got {type(value).__name__}")
    if not low <= int(value) <= top:
        raise ValueError(f"{who}: {name} must lie in [{low}, {top}], got {value!r}")
    return int(value)


def _steps(value, who, name="steps"):
    return _int_in(value, who, name, 1, (1 << 31) - 1)


def _check_levels(image, who, name="image", like=None):
    """the checks on a map of grey levels that need no device: integers, 2-D or 3-D, in range where it lies on the host, and
    the shape of ``like``"""
    _check_map(image, who, name)
    if like is not None and tuple(image.shape) != tuple(like.shape):
        raise ValueError(f"{who}: {name} has shape {tuple(image.shape)}, expected {tuple(like.shape)}")
    if not torch.is_tensor(image) and image.size and (int(image.min()) < 0 or int(image.max()) > MAX_LEVEL):
        raise ValueError(_OUT_OF_RANGE.format(who=who, name=name))


def _check_mask(mask, like, who):
    if mask is None:
        return
    if not torch.is_tensor(mask) and not isinstance(mask, np.ndarray):
        raise TypeError(f"{who}: mask must be an array or a tensor, got {type(mask).__name__}")
    if tuple(mask.shape) != tuple(like.shape):
        raise ValueError(f"{who}: mask has shape {tuple(mask.shape)}, expected {tuple(like.shape)}")


def _device_levels(image, device, who, name="image"):
    """a checked map of grey levels -> flat int32 on the device"""
    if torch.is_tensor(image):
        t = image.to(device)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > MAX_LEVEL):
            raise ValueError(_OUT_OF_RANGE.format(who=who, name=name))
        return t.to(torch.int32).contiguous().reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(image).astype(np.int32)).to(device).reshape(-1)


def _grey_scene(image, device, who):
    """the ``_Scene`` of a checked map of grey levels: ``lab`` holds the levels, and there are no ids"""
    device = _resolve_device(image, device)
    levels = _device_levels(image, device, who)
    _clx.require_device(levels, "image")
    return _Scene(who, levels, device, image.ndim, tuple(int(v) for v in image.shape), 1)


def _morph(scene, values, mask_d, op, steps, name="image"):
    """``steps`` steps of erosion (``op`` 0) or dilation (1) of ``values`` (flat int32 on the scene's device) in clx_grey_morph
    calls of at most MORPH_STEPS steps each -> a new flat int32 device tensor"""
    per_call = MORPH_STEPS[scene.nd]
    while steps > 0:
        k = min(per_call, steps)
        out = torch.empty_like(values)
        scene.call("clx_grey_morph", {1: _OUT_OF_RANGE.format(who="{who}", name=name)}, values, mask_d, scene.nd, scene.Z, scene.Y, scene.X,
                   op, k, out, FLAGS)
        values, steps = out, steps - k
    return values


def _reconstruct(scene, marker, image, mask_d):
    """the clx_grey_reconstruct calls of one reconstruction (``_settle``) -> (the result, flat int32 on the device; the rounds
    in which a tile changed)"""
    workspace, nbytes = _workspace(scene, "clx_grey_reconstruct_workspace", scene.nd, scene.Z, scene.Y, scene.X)
    out = torch.empty(image.numel(), dtype=torch.int32, device=scene.device)
    total = _settle(scene, lambda resume, info: _clx.call(
        "clx_grey_reconstruct", _clx.ptr(marker), _clx.ptr(image), _clx.ptr(mask_d), scene.nd, scene.Z, scene.Y, scene.X,
        ROUNDS_PER_CALL, resume, _clx.ptr(out), _clx.ptr(info), _clx.ptr(workspace), nbytes, _clx.stream_ptr(scene.device)),
        {1: _OUT_OF_RANGE.format(who=scene.who, name="marker"), 2: _OUT_OF_RANGE.format(who=scene.who, name="image")}, "reconstruction")
    return out, total


def _morphology(image, steps, mask, device, who, ops):
    """``ops`` (0 erode, 1 dilate; each ``steps`` steps) applied in turn to ``image`` -> (scene, the result flat on the device or
    None for a map without pixels, the mask on the device)"""
    steps = _steps(steps, who, "radius" if who == "grey_tophat" else "steps")
    _check_levels(image, who)
    _check_mask(mask, image, who)
    scene = _grey_scene(image, device, who)
    if scene.lab.numel() == 0:
        return scene, None, None
    mask_d = _device_mask(mask, scene.device)
    values = scene.lab
    for op in ops:
        values = _morph(scene, values, mask_d, op, steps)
    return scene, values, mask_d


def grey_erode(image, steps=1, mask=None, device=None):
    """``image`` (2-D or 3-D integers in [0, 65535], array or device tensor) eroded ``steps`` (>= 1) times: every inside pixel
    gets the minimum over the inside pixels within ``steps`` face steps through inside pixels, outside pixels get 0.  ``mask``:
    anything of that shape that ``!= 0`` makes boolean, or None (all inside).  The result has the type, dtype and device of
    ``image``.  The module's docstring has the definitions.  Runs on a HIP device; there is no CPU path."""
    scene, out, _ = _morphology(image, steps, mask, device, "grey_erode", (0,))
    return _in_type_of(image, scene, out)


def grey_dilate(image, steps=1, mask=None, device=None):
    """``grey_erode`` with the maximum."""
    scene, out, _ = _morphology(image, steps, mask, device, "grey_dilate", (1,))
    return _in_type_of(image, scene, out)


def grey_open(image, steps=1, mask=None, device=None):
    """``steps`` steps of erosion, then ``steps`` steps of dilation (``grey_erode``'s arguments): the opening by the diamond of
    radius ``steps``, which removes the bright structure that is narrower."""
    scene, out, _ = _morphology(image, steps, mask, device, "grey_open", (0, 1))
    return _in_type_of(image, scene, out)


def grey_tophat(image, radius, mask=None, device=None):
    """The white top-hat: ``image - grey_open(image, radius)`` on inside pixels, 0 outside; never negative (``grey_erode``'s
    arguments)."""
    scene, opened, mask_d = _morphology(image, radius, mask, device, "grey_tophat", (0, 1))
    if opened is None:
        return _in_type_of(image, scene, None)
    hat = scene.lab - opened
    return _in_type_of(image, scene, hat if mask_d is None else hat * (mask_d != 0))


def grey_reconstruct(marker, image, mask=None, device=None):
    """The reconstruction by dilation of ``marker`` under ``image`` (both 2-D or 3-D integers in [0, 65535] of one shape, arrays
    or device tensors; ``mask`` as in ``grey_erode``): the least map ``r >= min(marker, image)`` with ``r[p] = min(image[p],
    max(r[p], r[face neighbours of p]))``; outside pixels get 0 and conduct nothing.  The result has the type, dtype and device
    of ``image``.  A function of the inputs alone: the same bits in every run, and the transposed inputs give the transposed
    result.  Runs on a HIP device; there is no CPU path."""
    who = "grey_reconstruct"
    _check_levels(image, who)
    _check_levels(marker, who, "marker", like=image)
    _check_mask(mask, image, who)
    scene = _grey_scene(image, device, who)
    if scene.lab.numel() == 0:
        return _in_type_of(image, scene, None)
    out, _ = _reconstruct(scene, _device_levels(marker, scene.device, who, "marker"), scene.lab, _device_mask(mask, scene.device))
    return _in_type_of(image, scene, out)


def _check_spectrum(scales, background, who):
    return _int_in(scales, who, "scales", 1, MAX_SCALES), _int_in(background, who, "background", 0, MAX_BACKGROUND)


def _sums(scene, values):
    """clx_region_intensity of the scene's labels and a map of grey levels -> the exact sums by id, int64 on the host"""
    isum, vkey = scene.ids(), scene.ids(2)
    scene.call("clx_region_intensity", {1: LABELS_CHANGED}, scene.lab, values, _RAW_I32, scene.lab.numel(), scene.nid, 0, isum, vkey, FLAGS)
    return isum.cpu().numpy()


def _spectrum(scene, levels, scales, background, rounds=None):
    """the sums ``S[n + 1][objects]`` (int64) of a measured scene that has objects and a flat int32 device map of grey levels;
    ``rounds`` (a list) takes the changing rounds of every scale's reconstruction"""
    grey = _Scene(scene.who, levels, scene.device, scene.nd, scene.spatial, 1)
    g = levels
    if background:
        g = g - _morph(grey, _morph(grey, g, None, 0, background), None, 1, background)
    sums, e = [_sums(scene, g)], g
    for _ in range(scales):
        e = _morph(grey, e, None, 0, 1)
        r, busy = _reconstruct(grey, e, g, None)
        sums.append(_sums(scene, r))
        if rounds is not None:
            rounds.append(busy)
    return np.stack(sums)[:, scene.present]


def granular_spectrum(labels, levels_image, scales=16, background=0, device=None):
    """The sums behind the granular spectrum: ``(ids, S)`` with ``ids`` the labels present in ``labels`` (2-D or 3-D integers, the
    same types and range as ``region_table``), ascending, and ``S`` an int64 array ``(scales + 1, len(ids))``, ``S[i]`` the sum of
    ``r_i`` over each object's pixels: exact integers.  ``levels_image``: integers in [0, 65535] in the shape of ``labels``;
    ``scales`` in [1, 64]; ``background`` in [0, 64], the radius of the top-hat taken first (0: none).  The module's docstring
    has the definitions.  Runs on a HIP device; there is no CPU path."""
    who = "granular_spectrum"
    scales, background = _check_spectrum(scales, background, who)
    _check_map(labels, who)
    _check_levels(levels_image, who, "levels_image", like=labels)
    scene = _scene(labels, device, who).measured()
    if scene.empty:
        return np.zeros(0, dtype=np.int64), np.zeros((scales + 1, 0), dtype=np.int64)
    return scene.present.astype(np.int64), _spectrum(scene, _device_levels(levels_image, scene.device, who, "levels_image"), scales, background)


def granularity_columns(sums, k=0):
    """The columns of one channel from the sums ``S`` (``granular_spectrum``'s: ``(n + 1, objects)`` integers, non-increasing
    down every column and >= 0): ``granularity_<i>_c<k> = 100 (S[i - 1] - S[i]) / S[0]`` for ``i = 1 .. n`` and
    ``granularity_residual_c<k> = 100 S[n] / S[0]``, float64, each one correctly rounded division of exact integers; NaN where
    ``S[0] == 0``.  Host only."""
    who = "granularity_columns"
    k = _int_in(k, who, "k", 0, (1 << 31) - 1)
    sums = np.asarray(sums)
    if sums.ndim != 2 or sums.shape[0] < 2 or (sums.dtype.kind not in "ui" and sums.dtype != object):
        raise ValueError(f"{who}: sums must be integers of shape (scales + 1, objects) with scales >= 1")
    rows = [[int(v) for v in row] for row in sums]
    if any(v < 0 for v in rows[-1]) or any(a < b for upper, lower in zip(rows, rows[1:]) for a, b in zip(upper, lower)):
        raise ValueError(f"{who}: sums must be >= 0 and must not increase from one scale to the next")
    nobj, nan = sums.shape[1], float("nan")
    den = [s0 if s0 else 1 for s0 in rows[0]]
    zero = np.array([s0 == 0 for s0 in rows[0]], dtype=bool).reshape(nobj)

    def column(num):
        return np.where(zero, nan, _exact_div([100 * v for v in num], den)) if nobj else np.zeros(0)

    table = {f"granularity_{i}_c{k}": column([a - b for a, b in zip(rows[i - 1], rows[i])]) for i in range(1, len(rows))}
    table[f"granularity_residual_c{k}"] = column(rows[-1])
    return table


def _check_table(scales, levels, background, who):
    scales, background = _check_spectrum(scales, background, who)
    return scales, _int_in(levels, who, "levels", 2, MAX_LEVEL + 1), background


def _channels(image, labels, who):
    """``image`` as (C, *spatial): real numbers; one channel in the shape of the labels gets its leading axis"""
    if not torch.is_tensor(image) and not isinstance(image, np.ndarray):
        raise TypeError(f"{who}: image must be an array or a tensor, got {type(image).__name__}")
    spatial = tuple(labels.shape)
    if tuple(image.shape) == spatial:
        image = image[None]
    if tuple(image.shape[1:]) != spatial:
        raise ValueError(f"{who}: image has shape {tuple(image.shape)}, labels {spatial}")
    return image


def _columns_of(scene, image, scales, levels, value_range, background, who, channels=None):
    """the granularity columns of the channels of ``image`` (checked, (C, *spatial)) for a measured scene"""
    table = {}
    for k in range(image.shape[0]) if channels is None else channels:
        grey = image_levels(image[k], levels, value_range)
        if scene.empty:
            sums = np.zeros((scales + 1, 0), dtype=np.int64)
        else:
            sums = _spectrum(scene, torch.from_numpy(grey).to(scene.device).reshape(-1), scales, background)
        table.update(granularity_columns(sums, k))
    return table


def granularity_table(labels, image, scales=16, levels=256, value_range=None, background=0, device=None):
    """The granular spectrum of every object of ``labels``, one row per label present: ``label``, ``area`` and per channel k of
    ``image`` (real numbers, ``(*spatial)`` or ``(C, *spatial)``) ``granularity_columns``' columns.  A channel goes through
    ``image_levels(channel, levels, value_range)`` over the WHOLE map -- the morphology reads the pixels around the objects
    too.  ``scales`` in [1, 64], ``levels`` in [2, 65536], ``background`` in [0, 64].  A map without objects gives an empty
    table with these columns.  Runs on a HIP device; there is no CPU path."""
    who = "granularity_table"
    scales, levels, background = _check_table(scales, levels, background, who)
    _check_map(labels, who)
    image = _channels(image, labels, who)
    scene = _scene(labels, device, who).measured()
    table = {"label": scene.present.astype(np.int64), "area": scene.area[scene.present].astype(np.int64)}
    table.update(_columns_of(scene, image, scales, levels, value_range, background, who))
    return table


def granularity_stage(inference_config, source, channel=None, scales=16, levels=256, background=0) -> None:
    """For every sample and bandwidth of ``source``, the name of a label dataset ``[sample, bandwidth, ...]`` in
    ``segmentation_dataset_config.container_path`` (``segment()``'s, say): ``granularity_table``'s rows of all samples as
    ``granularity_bandwidth-<b>.csv`` in the working directory -- a header line, then ``sample`` and the table's columns, floats
    as ``%.17g``.  ``channel``: the channel of the raw dataset to measure, or None: all of them.  The grey levels divide the
    range of each sample's raw channel over the whole image.  No dataset is written.  Rank 0 works alone under
    torch.distributed."""
    from .utils import zarr_io

    who = "granularity_stage"
    if not isinstance(source, str) or not source:
        raise ValueError(f"{who}: source must be the name of a dataset, got {source!r}")
    if channel is not None and (isinstance(channel, bool) or not isinstance(channel, (numbers.Integral, np.integer)) or channel < 0):
        raise ValueError(f"{who}: channel must be an integer >= 0 or None, got {channel!r}")
    scales, levels, background = _check_table(scales, levels, background, who)
    stage = _stage.begin(who, inference_config)
    if stage is None:
        return
    stage.open("r", source)
    dataset_config = inference_config.dataset_config
    ds_raw = zarr_io.open(dataset_config.container_path, "r")[dataset_config.dataset_name]
    if channel is not None and channel >= ds_raw.shape[1]:
        raise ValueError(f"{who}: no channel {channel} in a raw dataset of {ds_raw.shape[1]} channels")
    ds_source = stage.f[source]

    def per_sample(sample, bandwidth):
        labels = ds_source[sample, bandwidth].astype(np.int32)
        scene = _scene(labels, stage.device, who).measured()
        table = {"label": scene.present.astype(np.int64), "area": scene.area[scene.present].astype(np.int64)}
        table.update(_columns_of(scene, np.asarray(ds_raw[sample]), scales, levels, None, background, who,
                                 channels=None if channel is None else (int(channel),)))
        return (table,)

    stage.run(per_sample, ("granularity",))


if __name__ == "__main__":
    from .cli import granularity as _command

    _command()
