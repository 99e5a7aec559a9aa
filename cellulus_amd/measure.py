"""Measure stage: the per-object table users take from ``skimage.measure.regionprops`` on the host —
area, bounding box, centroid, covariance, equivalent diameter and mean / min / max intensity per raw
channel — from integer sums gathered in one pass over the label map on the device
(``csrc/region_moments.hip``: ``clx_region_moments``, ``clx_region_intensity``).  The sums are exact integers, so
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
from collections import namedtuple

import numpy as np

from . import _clx, _stage
# every name of the host half stays importable from here (its two patchable constants aside: a copy would not be read)
from .measure_columns import (BORDER_WORDS, DIST_INF, MAX_LEVELS, MAX_QUANTILES, MAX_RADIAL_WIDTH, MAX_RINGS,  # noqa: F401
                              MAX_TEXTURE_DISTANCE, MIN_LEVELS, NO_PEAK, PERIMETER_WEIGHTS, PRODUCT_WORDS, RADIAL_WEDGES,
                              SURFACE_WEIGHTS, TEXTURE_FEATURES, WEIGHTED_WORDS, _AXES, _PAIRS, _PRODUCT_SQUARES, _PRODUCT_SUMS,
                              _SHIFT_MAX, _SHIFT_MIN, _SQRT2, _SQRT3, _WEIGHTED_MOMENTS, _check_products, _check_quantiles,
                              _check_radial, _check_texture, _check_weighted, _exact_div, _format, _neg_xlog2x, _ratio,
                              _scaled_column, _signed128, _signed_root, _sqrt_ratio, _texture_slice, border_intensity_columns,
                              border_table, boundary_columns, coloc_thresholds, hull_columns, inscribed_columns, intensity_shift,
                              perimeter_from_classes, product_table, products_columns, quantile_columns, quantile_ranks,
                              quantised, radial_columns, shape_columns, texture_columns, texture_directions, topology_columns,
                              weighted_columns, weighted_table)

MAX_IDS = 1 << 24                       # clx_region_moments / clx_region_intensity: nid <= 2^24
MIN_CAPACITY, MAX_CAPACITY = 1 << 10, 1 << 28       # clx_region_contacts: slots of the pair table
TEXTURE_TABLE_BYTES = 1 << 28           # the counts table of one clx_region_cooccurrence call stays below this
RADIAL_TABLE_BYTES = 1 << 28            # the count and isum tables of one clx_region_radial call stay below this together
_PAIRS_FULL = 4                         # bit of info[0] of clx_region_contacts and clx_label_overlaps: a pair found no slot
_CONTACTS_HEADER = ("sample", "label_a", "label_b", "faces")         # of contacts_bandwidth-<b>.csv, with or without rows

# What a call's flag bits say.  Which bit says what is the kernel's and differs per entry point: every call has its own
# {bit: message} table beside it, in the order its bits are looked at.
LABELS_OUT_OF_RANGE = f"{{who}}: label ids must lie in [0, {MAX_IDS})"
LABELS_CHANGED = "{who}: label ids changed under the measurement"
VALUES_NOT_FINITE = "{who}: raw channel {k} has non-finite values inside objects"
DISTANCE_CHANGED = "{who}: the distance map changed under the measurement"
FLAGS = object()                         # stands in a call's arguments where its flags go


def _call(device, who, name, messages, *args, k=None, words=1):
    """One library call on ``device``'s current stream: tensors (and None) go as their addresses, a fresh int32 tensor of
    ``words`` words where ``FLAGS`` stands, the stream last.  Raises the first message of ``messages`` ({bit of word 0: text, or
    (exception type, text)}, ValueError where no type is given) whose bit is set, formatted with ``who`` and ``k``; else
    -> the words as a list"""
    import torch

    bad = torch.empty(words, dtype=torch.int32, device=device)
    _clx.call(name, *[_clx.ptr(bad) if a is FLAGS else _clx.ptr(a) if a is None or torch.is_tensor(a) else a for a in args],
              _clx.stream_ptr(device))
    flags = bad.tolist()
    for bit, message in messages.items():
        if flags[0] & bit:
            kind, text = message if isinstance(message, tuple) else (ValueError, message)
            raise kind(text.format(who=who, k=k))
    return flags


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
            raise ValueError(LABELS_OUT_OF_RANGE.format(who=who))
        return lab.to(torch.int32).contiguous()
    labels = np.ascontiguousarray(labels)
    if labels.dtype.kind not in "ui":
        raise TypeError(f"{who}: labels must be integers, got {labels.dtype}")
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= MAX_IDS):
        raise ValueError(LABELS_OUT_OF_RANGE.format(who=who))
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


def _raw_channels(raw, spatial, who):
    """``raw`` as (C, *spatial): one channel in the shape of the labels gets its leading axis"""
    if tuple(raw.shape) == spatial:
        raw = raw[None]
    if tuple(raw.shape[1:]) != spatial:
        raise ValueError(f"{who}: raw has shape {tuple(raw.shape)}, labels {spatial}")
    return raw


_Channel = namedtuple("_Channel", "raw_d raw_type shift peak_keys columns")


class _Scene:
    """One label map on the device and what the stage's blocks share of it: ``lab`` the flat int32 map, ``device``, ``nd``,
    ``spatial``, ``Z, Y, X`` and ``nid``; after ``measured()`` ``area_d`` and ``bbox_d`` on the device and on the host ``area``
    and ``bbox`` by id (``area[0] = 0``), ``present`` the ids of the objects, ascending, and ``sum1`` and ``sum2`` their rows,
    all of ONE clx_region_moments call; per channel of ``raw`` (set by the entry point once it has checked it) the
    ``_Channel`` of ``channel(k)``; the distance map and clx_region_inscribed's rows of ``inscribed(edge)``.  A map without
    objects makes no library call and has no ``present`` id.  ``who`` names the entry point in the messages."""

    def __init__(self, who, lab, device, nd, spatial, nid):
        self.who, self.lab, self.device, self.nd, self.spatial, self.nid = who, lab.reshape(-1), device, nd, spatial, nid
        self.Z, self.Y, self.X = (1,) * (3 - nd) + spatial
        self.area, self.bbox = np.zeros(1, dtype=np.int64), np.zeros((1, 6), dtype=np.int32)
        self.present = np.zeros(0, dtype=np.int64)
        self.sum1, self.sum2 = np.zeros((0, 3), dtype=np.uint64), np.zeros((0, 6), dtype=np.uint64)
        self.area_d = self.bbox_d = self.raw = self._inscribed = None
        self.channels, self._device_raw = {}, {}

    @property
    def empty(self):
        return not len(self.present)

    def ids(self, *width, dtype=None):
        """an uninitialised device tensor of one row per id: what a reduction over the map fills"""
        import torch

        return torch.empty((self.nid,) + width, dtype=dtype or torch.int64, device=self.device)

    def call(self, name, messages, *args, who=None, k=None):
        return _call(self.device, who or self.who, name, messages, *args, k=k)

    def measured(self):
        """takes the moments: the one clx_region_moments call of a map that has objects -> the scene"""
        if self.lab.numel() and self.nid > 1:
            import torch

            self.area_d, self.bbox_d, sum1_d, sum2_d = self.ids(), self.ids(6, dtype=torch.int32), self.ids(3), self.ids(6)
            self.call("clx_region_moments", {1: LABELS_OUT_OF_RANGE}, self.lab, self.Z, self.Y, self.X, self.nid, self.area_d,
                      self.bbox_d, sum1_d, sum2_d, FLAGS)
            area = self.area_d.cpu().numpy()
            area[0] = 0
            self.area, self.bbox, self.present = area, self.bbox_d.cpu().numpy(), np.flatnonzero(area > 0)
            self.sum1, self.sum2 = (s.cpu().numpy().view(np.uint64)[self.present] for s in (sum1_d, sum2_d))
        return self

    def device_raw(self, k):
        """-> (channel k of ``raw`` on the device, flat; its clx_raw_type), copied when first asked for"""
        if k not in self._device_raw:
            raw_d, raw_type = _to_device_raw(self.raw[k], self.device)
            self._device_raw[k] = raw_d.reshape(-1), raw_type
        return self._device_raw[k]

    def channel(self, k):
        """``device_raw(k)`` with the shift the channel's sums are quantised with, the largest order key of every id (uint64
        (nid): clx_region_weighted's peak_keys) and the channel's intensity columns, formed when first asked for"""
        if k not in self.channels:
            self.channels[k] = _Channel(*self.device_raw(k), *_intensity_columns(self, *self.device_raw(k), k))
        return self.channels[k]

    def inscribed(self, edge):
        """-> (the label-aware distance map, flat int32; clx_region_inscribed's rows, int64 (nid, 3)), both on the device and
        formed once; None for a map without objects"""
        if self._inscribed is None and not self.empty:
            dist = _distance_map(self, edge)
            self._inscribed = dist, _inscribed_of(self, dist, who="region_table")
        return self._inscribed


def _inscribed_of(scene, values, who=None):
    """clx_region_inscribed of the scene's map and a map of ``values`` (flat int32 on the device): per id the largest value,
    the first pixel that attains it and the sum -> int64 (nid, 3) on the device"""
    rows = scene.ids(3)
    scene.call("clx_region_inscribed", {1: LABELS_OUT_OF_RANGE, 2: DISTANCE_CHANGED}, scene.lab, values, scene.lab.numel(), scene.nid,
               rows, FLAGS, who=who)
    return rows


def _check_map(labels, who, name="labels"):
    """the checks on a label map that need no device: an array or a tensor of integers, 2-D or 3-D"""
    import torch

    if not torch.is_tensor(labels) and not isinstance(labels, np.ndarray):
        raise TypeError(f"{who}: {name} must be an array or a tensor, got {type(labels).__name__}")
    if ((labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool) if torch.is_tensor(labels)
            else labels.dtype.kind not in "ui"):
        raise TypeError(f"{who}: {name} must be integers, got {labels.dtype}")
    if labels.ndim not in (2, 3):
        raise ValueError(f"{who}: {name} must be 2-D or 3-D, got {labels.ndim} dimensions")


def _in_type_of(labels, scene, out):
    """a result map ``out`` of ``scene`` (flat on the device; None: the map came through unchanged) in the type, dtype and
    device of ``labels``, the map the scene was made of"""
    import torch

    if torch.is_tensor(labels):
        return labels.clone() if out is None else out.reshape(scene.spatial).to(device=labels.device, dtype=labels.dtype)
    return labels.copy() if out is None else out.reshape(scene.spatial).cpu().numpy().astype(labels.dtype)


def _workspace(scene, entry, *args, below="2^32"):
    """the scratch an entry point asks for through its ``clx_*_workspace`` function ``entry(*args)`` -> (an int32 device
    tensor of at least that many bytes, the bytes); 0 bytes say that the map has ``below`` pixels or more"""
    import torch

    nbytes = int(getattr(_clx.load(), entry)(*args))
    if nbytes == 0:
        raise ValueError(f"{scene.who}: the map must have fewer than {below} pixels")
    return torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=scene.device), nbytes


ROUNDS_PER_CALL = 8                     # rounds a call of a round-driven entry point queues between two looks at info[1]


def _settle(scene, call, errors, what):
    """the library calls of one fixed point reached in rounds (clx_label_propagate, clx_grey_reconstruct), ROUNDS_PER_CALL
    rounds each, until no tile changes.  ``call(resume, info)`` makes one call through ``_clx.call``; ``errors``: {bit of
    info[0]: message}, raised as ValueError in that order; ``what`` names the iteration where it does not end -> the rounds
    in which a tile changed"""
    import torch

    npix = scene.lab.numel()
    info = torch.empty(3, dtype=torch.int32, device=scene.device)
    total, resume = 0, 0
    while True:
        call(resume, info)
        flags, changed, busy = info.tolist()
        for bit, message in errors.items():
            if flags & bit:
                raise ValueError(message)
        total, resume = total + busy, 1
        if changed == 0:
            return total
        if total > npix + 1:                                  # every changing round settles one more pixel of some best path
            raise RuntimeError(f"{scene.who}: {total} rounds changed a map of {npix} pixels: the {what} does not come to rest")


def _device_mask(mask, device):
    """anything that ``!= 0`` makes boolean -> flat uint8 on the device (None stays None)"""
    import torch

    if mask is None:
        return None
    m = mask.to(device) != 0 if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)).to(device)
    return m.to(torch.uint8).contiguous().reshape(-1)


def _result_scene(scene, lab):
    """a map ``lab`` made of the scene's (flat int32 on the device, the same ids) as a measured scene of its own, which must
    hold the objects the scene holds"""
    result = _Scene(scene.who, lab, scene.device, scene.nd, scene.spatial, scene.nid).measured()
    if not np.array_equal(result.present, scene.present):
        raise ValueError(LABELS_CHANGED.format(who=scene.who))
    return result


def _scene(labels, device, who):
    """the ``_Scene`` of ``labels`` after the type and range checks every entry point shares, its moments not taken yet; `who`
    names the caller in their messages"""
    device = _resolve_device(labels, device)
    nd = labels.ndim
    if nd not in (2, 3):
        raise ValueError(f"{who}: labels must be 2-D or 3-D, got {nd} dimensions")
    spatial = tuple(int(v) for v in labels.shape)
    lab = _to_device_labels(labels, device, who)
    _clx.require_device(lab, "labels")
    return _Scene(who, lab, device, nd, spatial, int(lab.max().item()) + 1 if lab.numel() else 1)


def _intensity(scene, raw_d, raw_type, shift, k, messages):
    """One clx_region_intensity call -> (isum int64 (nid), keys uint64 (nid, 2))."""
    isum, vkey = scene.ids(), scene.ids(2)
    scene.call("clx_region_intensity", messages, scene.lab, raw_d, raw_type, scene.lab.numel(), scene.nid, int(shift), isum, vkey, FLAGS,
               who="region_table", k=k)
    return isum.cpu().numpy(), vkey.cpu().numpy().view(np.uint64)


def _intensity_columns(scene, raw_d, raw_type, k):
    """-> (the shift the sums of channel k are quantised with, the largest order key of every id, the intensity columns)"""
    from .segment import _RAW_I32, _decode_keys
    from .utils.otsu import minmax_on_device

    if scene.empty:
        dt = raw_d.cpu().numpy().dtype
        return 0, None, {f"intensity_mean_c{k}": np.zeros(0), f"intensity_min_c{k}": np.zeros(0, dt),
                         f"intensity_max_c{k}": np.zeros(0, dt)}
    present = scene.present
    shift = 0
    if raw_type != _RAW_I32:
        lo, hi = minmax_on_device(raw_d)
        max_abs = max(abs(lo), abs(hi))
        if not math.isfinite(max_abs):
            # something outside the objects is not finite: take the maximum under the objects from the keys of a first
            # call whose scale lets every finite value pass
            _, keys = _intensity(scene, raw_d, raw_type, _SHIFT_MIN, k, {2: VALUES_NOT_FINITE})
            vals = _decode_keys(keys[present], raw_type).astype(np.float64)
            max_abs = float(np.abs(vals).max()) if vals.size else 0.0
        shift = intensity_shift(max_abs, scene.lab.numel())
    isum, keys = _intensity(scene, raw_d, raw_type, shift, k, {2: VALUES_NOT_FINITE, 1: LABELS_CHANGED})
    vals = _decode_keys(keys[present], raw_type)
    mean = _exact_div(isum[present].astype(object), scene.area[present].astype(object))
    if shift:
        mean = np.ldexp(mean, -shift)
    return shift, np.ascontiguousarray(keys[:, 1]), {f"intensity_mean_c{k}": mean, f"intensity_min_c{k}": vals[:, 0].copy(),
                                                     f"intensity_max_c{k}": vals[:, 1].copy()}


def _pair_capacity(objects):
    """power of two, at least 8 x the object count (an object of a tissue has about six neighbours, so about four
    pairs with the background's: the table stays below half full) and at least MIN_CAPACITY"""
    return max(MIN_CAPACITY, 1 << max(0, 8 * int(objects) - 1).bit_length())


def _pair_slots(device, who, name, messages, capacity, *args):
    """A library call that fills a table of 64-bit pairs (``args``, then the slots, keys, values and info), repeated with twice the
    table while it reports a pair it could not place -> (keys uint64, values int64) of the occupied slots, in slot order.
    `capacity`: the slots of the first table, ``_pair_capacity`` of the object count or of a bound on it"""
    import torch

    while True:
        if capacity > MAX_CAPACITY:
            raise ValueError(f"{who}: more id pairs than a table of {MAX_CAPACITY} slots holds")
        keys = torch.empty(capacity, dtype=torch.int64, device=device)
        counts = torch.empty(capacity, dtype=torch.int64, device=device)
        flags, used = _call(device, who, name, messages, *args, capacity, keys, counts, FLAGS, words=2)
        if not flags & _PAIRS_FULL:
            break
        capacity *= 2
    slot = torch.nonzero(keys).reshape(-1)
    assert slot.numel() == used
    return keys[slot].cpu().numpy().view(np.uint64), counts[slot].cpu().numpy()


def _pair_table(device, who, name, messages, capacity, *args):
    """``_pair_slots`` of a table of id pairs -> (a, b, count) int64, sorted by (a, b)"""
    k, counts = _pair_slots(device, who, name, messages, capacity, *args)
    k = k.view(np.int64)
    order = np.argsort(k, kind="stable")                     # keys are (a << 32) | b with a < 2^24: the (a, b) order
    k = k[order]
    return k >> 32, k & 0xFFFFFFFF, counts[order]


def _contacts(scene, objects):
    """clx_region_contacts -> (a, b, faces) int64, sorted by (a, b); no row and no call for a map without objects.  `objects`:
    the object count or a bound on it, which sizes the first table"""
    if scene.nid == 1:                                       # no pixel, or background only: no object, no pair
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    return _pair_table(scene.device, scene.who, "clx_region_contacts", {1: LABELS_OUT_OF_RANGE}, _pair_capacity(objects), scene.lab,
                       scene.nd, scene.Z, scene.Y, scene.X, scene.nid)


def contact_pairs(labels, device=None):
    """The faces between pixels of different ids of ``labels`` (2-D or 3-D integers, array or device tensor; the same
    types and range as ``region_table``), connectivity 1, the outside of the image counting as id 0: ``(a, b, faces)``
    int64 arrays, one row per pair with ``a < b``, sorted by ``(a, b)``.  Rows with ``a == 0`` are an object's faces to
    the background and the image edge; the others are the region adjacency graph with the size of every contact.
    Runs on a HIP device; there is no CPU path."""
    scene = _scene(labels, device, "contact_pairs")
    # the first table is sized without another pass over the map: neither the largest id nor the pixel count is below
    # the object count
    return _contacts(scene, min(scene.nid - 1, scene.lab.numel()))


def _perimeter_classes(scene):
    """clx_region_perimeter's rows of the present ids, int64 (n, 4)"""
    if scene.empty:
        return np.zeros((0, 4), dtype=np.int64)
    classes = scene.ids(4)
    scene.call("clx_region_perimeter", {1: LABELS_OUT_OF_RANGE}, scene.lab, scene.Y, scene.X, scene.nid, classes, FLAGS)
    return classes.cpu().numpy()[scene.present]


def _topology_counts(scene):
    """clx_region_topology's rows of the present ids, int64 (n, 5)"""
    if scene.empty:
        return np.zeros((0, 5), dtype=np.int64)
    counts = scene.ids(5)
    scene.call("clx_region_topology", {1: LABELS_OUT_OF_RANGE}, scene.lab, scene.nd, scene.Z, scene.Y, scene.X, scene.nid, counts,
               FLAGS)
    return counts.cpu().numpy()[scene.present]


def _hull_rows(scene):
    """one clx_region_hull call on clx_region_moments' bounding boxes -> its rows of the present ids, int64 (n, 5)"""
    import torch

    if scene.empty:
        return np.zeros((0, 5), dtype=np.int64)
    box = scene.bbox[scene.present].astype(np.int64)
    nrows = np.zeros(scene.nid, dtype=np.int64)
    nrows[scene.present] = (box[:, 3] - box[:, 0] + 1) * (box[:, 4] - box[:, 1] + 1)
    row_base = np.cumsum(nrows) - nrows                      # exclusive; absent ids have no rows
    rows = int(nrows.sum())
    nbytes = int(_clx.load().clx_region_hull_workspace(rows))
    if nbytes == 0:
        raise ValueError("region_table: too many bounding-box rows for clx_region_hull")
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=scene.device)
    hull = scene.ids(5)
    scene.call("clx_region_hull", {1: LABELS_OUT_OF_RANGE, 2: LABELS_CHANGED}, scene.lab, scene.nd, scene.Z, scene.Y, scene.X,
               scene.nid, scene.bbox_d, torch.from_numpy(row_base).to(scene.device), rows, workspace, nbytes, hull, FLAGS)
    return hull.cpu().numpy()[scene.present]


def _distance_map(scene, edge):
    """one clx_label_distance_sq call -> int32 device tensor, flat"""
    import torch

    npix = scene.lab.numel()
    nbytes = int(_clx.load().clx_label_distance_workspace(npix))
    if nbytes == 0:
        raise ValueError("label_distance_sq: the map must have fewer than 2^32 pixels")
    dist = torch.empty(npix, dtype=torch.int32, device=scene.device)
    workspace = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=scene.device)
    _clx.call("clx_label_distance_sq", _clx.ptr(scene.lab), scene.nd, scene.Z, scene.Y, scene.X, int(bool(edge)), _clx.ptr(dist),
              _clx.ptr(workspace), nbytes, _clx.stream_ptr(scene.device))
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

    scene = _scene(labels, device, "label_distance_sq")
    if scene.lab.numel() == 0:
        return torch.empty(scene.spatial, dtype=torch.int32, device=scene.device)
    return _distance_map(scene, edge).reshape(scene.spatial)


def _inscribed_rows(scene, edge):
    """clx_region_inscribed's rows of the present ids on the host, int64 (n, 3)"""
    if scene.empty:
        return np.zeros((0, 3), dtype=np.int64)
    return scene.inscribed(edge)[1].cpu().numpy()[scene.present]


def _order_columns(scene, quantiles, mad):
    """the quantile and MAD columns of every channel: one clx_region_order_stats call per channel for all quantiles (two
    ranks each, and the median's where ``mad`` needs them; a second call where that makes more than 32 ranks), and one with
    the medians as ``centre`` for the MAD"""
    import torch

    from .segment import _RAW_F64, _decode_keys

    device, nid, present, area = scene.device, scene.nid, scene.present, scene.area
    nch = scene.raw.shape[0]
    names = [f"intensity_q{float(q)!r}" for q in quantiles]
    if scene.empty:
        return {f"{n}_c{k}": np.zeros(0) for k in range(nch) for n in names + ["intensity_mad"] * bool(mad)}
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

    def order_keys(ch, k, centre_d, rank_d):
        """one clx_region_order_stats call -> uint64 keys (nid, nq) on the host"""
        out = scene.ids(rank_d.shape[1])
        scene.call("clx_region_order_stats", {
            2: VALUES_NOT_FINITE, 1 | 4: LABELS_CHANGED,
            8: (RuntimeError, "{who}: internal error: a rank at or above its object's area reached clx_region_order_stats")},
            scene.lab, ch.raw_d, ch.raw_type, scene.lab.numel(), nid, scene.area_d, seg_base_d, total, centre_d, rank_d, rank_d.shape[1],
            out, workspace, nbytes, FLAGS, k=k)
        return out.cpu().numpy().view(np.uint64)

    if mad:
        m = needed.index(0.5)
        mad_rank_d = rank_d[:, 2 * m:2 * m + 2].contiguous()
    # 16 quantiles without 0.5 and the MAD's median are 17 pairs of ranks: more than one call takes
    pairs = 2 * MAX_QUANTILES
    rank_calls = [rank_d[:, c:c + pairs].contiguous() for c in range(0, nq, pairs)]
    cols = {}
    for k in range(nch):
        ch = scene.channel(k)
        keys = np.concatenate([order_keys(ch, k, None, r) for r in rank_calls], axis=1)
        vals = _decode_keys(keys[present], ch.raw_type)
        columns = [quantile_columns(vals[:, 2 * j], vals[:, 2 * j + 1], weights[j]) for j in range(len(needed))]
        for n, c in zip(names, columns):
            cols[f"{n}_c{k}"] = c
        if mad:
            centre = np.zeros(nid, dtype=np.float64)
            centre[present] = columns[m]
            dev = _decode_keys(order_keys(ch, k, torch.from_numpy(centre).to(device), mad_rank_d)[present], _RAW_F64)
            cols[f"intensity_mad_c{k}"] = quantile_columns(dev[:, 0], dev[:, 1], weights[m])
    return cols


def _cooccurrence_counts(scene, k, value_range, levels, distance):
    """clx_region_cooccurrence of channel k for the objects of the scene, in chunks of them whose counts table stays below
    TEXTURE_TABLE_BYTES -> counts int64 (n, ndir, levels, levels); the pixels every call saw are checked against the areas.
    value_range None: the smallest and the largest value under the objects"""
    import torch

    ndir = 4 if scene.nd == 2 else 13
    ids = scene.present
    out = np.empty((len(ids), ndir, levels, levels), dtype=np.int64)
    if scene.empty:
        return out
    raw_d, raw_type = scene.device_raw(k)
    if value_range is None:
        columns = scene.channel(k).columns
        value_range = float(columns[f"intensity_min_c{k}"].min()), float(columns[f"intensity_max_c{k}"].max())
    lo, hi = value_range
    step = max(1, TEXTURE_TABLE_BYTES // (ndir * levels * levels * 4))
    workspace, have = None, 0
    for a in range(0, len(ids), step):
        chunk = np.asarray(ids[a:a + step], dtype=np.int64)
        nrows = len(chunk)
        nbytes = int(_clx.load().clx_region_cooccurrence_workspace(scene.lab.numel(), nrows))
        if nbytes == 0:
            raise ValueError(f"{scene.who}: the map must have fewer than 2^31 pixels for the texture columns")
        if nbytes > have:
            workspace, have = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=scene.device), nbytes
        counts = torch.empty((nrows, ndir, levels, levels), dtype=torch.int32, device=scene.device)
        seen = torch.empty(nrows, dtype=torch.int64, device=scene.device)
        scene.call("clx_region_cooccurrence", {2: VALUES_NOT_FINITE, 1: LABELS_CHANGED}, scene.lab, raw_d, raw_type, scene.nd, scene.Z,
                   scene.Y, scene.X, scene.nid, scene.bbox_d, torch.from_numpy(chunk.astype(np.int32)).to(scene.device), nrows,
                   float(lo), float(hi), levels, distance, counts, seen, FLAGS, workspace, nbytes, k=k)
        if not np.array_equal(seen.cpu().numpy(), scene.area[chunk]):
            raise ValueError(LABELS_CHANGED.format(who=scene.who))
        out[a:a + nrows] = counts.cpu().numpy()
    return out


def _texture_columns_of(scene, levels, distance, value_range):
    """the texture columns of every channel"""
    out = {}
    for k in range(scene.raw.shape[0]):
        t = texture_columns(_cooccurrence_counts(scene, k, value_range, levels, distance), scene.nd)
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
    scene = _scene(labels, device, who)
    if tuple(raw.shape) != scene.spatial:
        raise ValueError(f"{who}: raw has shape {tuple(raw.shape)}, labels {scene.spatial}: one channel in the shape of labels")
    scene.raw = raw[None]
    scene.measured()
    return scene.present.astype(np.int64), _cooccurrence_counts(scene, 0, value_range, levels, distance)


def _radial_tables(scene, edge, rings, width, wedges):
    """clx_region_radial for the objects of the scene on its distance map and clx_region_inscribed's rows, in chunks of objects
    whose two tables stay below RADIAL_TABLE_BYTES together; one call per chunk and channel of ``scene.raw``, one without a
    channel where there is none -> (count int64 (n, rings, wedges), [isum int64 of the same shape per channel]).
    width 0: relative rings; the pixels every call counted are checked against the areas"""
    import torch

    ids, nid = scene.present, scene.nid
    n = len(ids)
    nch = 0 if scene.raw is None else scene.raw.shape[0]
    count = np.empty((n, rings, wedges), dtype=np.int64)
    isums = [np.empty((n, rings, wedges), dtype=np.int64) for _ in range(nch)]
    if scene.empty:
        return count, isums
    channels = [scene.channel(k) for k in range(nch)]
    dist, inscribed_d = scene.inscribed(edge)
    step = max(1, RADIAL_TABLE_BYTES // (rings * wedges * 16))
    for a in range(0, n, step):
        chunk = np.asarray(ids[a:a + step], dtype=np.int64)
        nrows = len(chunk)
        row = np.full(nid, -1, dtype=np.int32)
        row[chunk] = np.arange(nrows, dtype=np.int32)
        row_d = torch.from_numpy(row).to(scene.device)
        count_d = torch.empty((nrows, rings, wedges), dtype=torch.int64, device=scene.device)
        isum_d = torch.empty((nrows, rings, wedges), dtype=torch.int64, device=scene.device) if channels else None
        for k, ch in enumerate(channels or [_Channel(None, 0, 0, None, None)]):
            scene.call("clx_region_radial", {2: VALUES_NOT_FINITE, 4: DISTANCE_CHANGED, 1 | 8: LABELS_CHANGED}, scene.lab, dist,
                       ch.raw_d, ch.raw_type, scene.nd, scene.Z, scene.Y, scene.X, nid, inscribed_d, row_d, nrows, rings, width, wedges,
                       int(ch.shift), count_d, isum_d, FLAGS, k=k)
            got = count_d.cpu().numpy()
            if not np.array_equal(got.sum(axis=(1, 2)), scene.area[chunk]):
                raise ValueError(LABELS_CHANGED.format(who=scene.who))
            count[a:a + nrows] = got
            if ch.raw_d is not None:
                isums[k][a:a + nrows] = isum_d.cpu().numpy()
    return count, isums


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
    scene = _scene(labels, device, who)
    if raw is not None:
        scene.raw = _raw_channels(raw, scene.spatial, who)
    scene.measured()
    count, isums = _radial_tables(scene, edge, rings, width, W)
    return scene.present.astype(np.int64), count, isums, [0 if scene.empty else scene.channel(k).shift for k in range(len(isums))]


def _counted(scene, words, low=None):
    """the uint64 rows of the present ids of a reduction's (nid, W) int64 words, after checking word 0, the pixels the call
    counted, against the areas (``low``: the areas only bound it from above, ``low`` from below)"""
    words = words.cpu().numpy().view(np.uint64)[scene.present]
    pixels, area = words[:, 0].view(np.int64), scene.area[scene.present]
    ok = np.array_equal(pixels, area) if low is None else (pixels >= low).all() and (pixels <= area).all()
    if not ok:
        raise ValueError(LABELS_CHANGED.format(who=scene.who))
    return words


def _products_rows(scene, j, k, thr_a=None, thr_b=None):
    """one clx_region_products call on channels j and k -> product_table of the present ids.  thr_*: int64 host arrays (nid) or
    None, both or neither"""
    import torch

    if scene.empty:
        return product_table(np.zeros((0, PRODUCT_WORDS), dtype=np.uint64))
    a, b = scene.channel(j), scene.channel(k)
    if a.raw_type != b.raw_type:
        raise ValueError(f"{scene.who}: raw channels {j} and {k} differ in type")
    out = scene.ids(PRODUCT_WORDS)
    thr_a_d, thr_b_d = (None if t is None else torch.from_numpy(np.ascontiguousarray(t, dtype=np.int64)).to(scene.device)
                        for t in (thr_a, thr_b))
    scene.call("clx_region_products", {2: VALUES_NOT_FINITE, 1: LABELS_CHANGED}, scene.lab, a.raw_d, b.raw_d, a.raw_type,
               scene.lab.numel(), scene.nid, int(a.shift), int(b.shift), thr_a_d, thr_b_d, out, FLAGS, k=f"{j} or {k}")
    return product_table(_counted(scene, out))


def _channel_threshold(scene, k, f):
    """coloc_thresholds of channel k's quantised maxima by id, int64 (nid); None for ``f`` None"""
    if f is None or scene.empty:
        return None
    ch = scene.channel(k)
    thr = np.zeros(scene.nid, dtype=np.int64)
    thr[scene.present] = coloc_thresholds(quantised(ch.columns[f"intensity_max_c{k}"], ch.shift), f)
    return thr


def _products_columns_of(scene, std, colocalization, f):
    """the std and colocalization columns.  One clx_region_products call per pair j < k, with the thresholds of the channels'
    intensity_max columns; a channel that no pair covers (no colocalization) takes one with a == b and no thresholds for its std"""
    nch = scene.raw.shape[0]
    pairs = [(j, k) for j in range(nch) for k in range(j + 1, nch)] if colocalization else []
    shift = [scene.channel(k).shift for k in range(nch)]
    out_std, out_coloc, thr = {}, {}, {}
    for j, k in pairs:
        for c in (j, k):
            if c not in thr:
                thr[c] = _channel_threshold(scene, c, f)
        got = products_columns(_products_rows(scene, j, k, thr[j], thr[k]), shift[j], shift[k], j, k, std=std, colocalization=True)
        for name in [n for n in got if n.startswith("intensity_std_")]:
            out_std.setdefault(name, got.pop(name))
        out_coloc.update(got)
    for k in range(nch if std and not pairs else 0):
        out_std.update(products_columns(_products_rows(scene, k, k), shift[k], shift[k], k, k, std=True, colocalization=False))
    return {**{f"intensity_std_c{k}": out_std[f"intensity_std_c{k}"] for k in range(nch if std else 0)}, **out_coloc}


def _channel_scene(labels, raw, channels, device, who):
    """the front of the entry points that take some ``channels`` (names and numbers) of ``raw``: the scene with ``raw`` set"""
    if raw is None:
        raise ValueError(f"{who}: raw is needed")
    raw = _raw_channels(raw, tuple(int(v) for v in labels.shape), who)
    if not all(0 <= k < raw.shape[0] for k in channels.values()):
        names = " and ".join(f"{name} = {k}" for name, k in channels.items())
        raise ValueError(f"{who}: channel{'s' * (len(channels) > 1)} {names} must lie in [0, {raw.shape[0]})")
    scene = _scene(labels, device, who).measured()
    scene.raw = raw
    return scene


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
    j, k = int(j), int(k)
    scene = _channel_scene(labels, raw, {"j": j, "k": k}, device, who)
    thr = {c: _channel_threshold(scene, c, f) for c in sorted({j, k})}
    table = _products_rows(scene, j, k, thr[j], thr[k])
    return (scene.present.astype(np.int64), table) + ((0, 0) if scene.empty else (scene.channel(j).shift, scene.channel(k).shift))


def _weighted_rows(scene, k):
    """one clx_region_weighted call on channel k -> weighted_table of the present ids"""
    import torch

    if scene.empty:
        return weighted_table(np.zeros((0, WEIGHTED_WORDS), dtype=np.uint64))
    ch = scene.channel(k)
    out = scene.ids(WEIGHTED_WORDS)
    keys_d = torch.from_numpy(np.ascontiguousarray(ch.peak_keys, dtype=np.uint64).view(np.int64)).to(scene.device)
    scene.call("clx_region_weighted", {2: VALUES_NOT_FINITE, 1: LABELS_CHANGED}, scene.lab, ch.raw_d, ch.raw_type, scene.Z, scene.Y,
               scene.X, scene.nid, int(ch.shift), keys_d, out, FLAGS, k=k)
    return weighted_table(_counted(scene, out))


def _border_rows(scene, k):
    """one clx_region_border_intensity call on channel k -> border_table of the present ids; an object has at least one border
    pixel and at most its area"""
    if scene.empty:
        return border_table(np.zeros((0, BORDER_WORDS), dtype=np.uint64))
    ch = scene.channel(k)
    out = scene.ids(BORDER_WORDS)
    scene.call("clx_region_border_intensity", {2: VALUES_NOT_FINITE, 1: LABELS_CHANGED}, scene.lab, ch.raw_d, ch.raw_type, scene.nd,
               scene.Z, scene.Y, scene.X, scene.nid, int(ch.shift), out, FLAGS, k=k)
    return border_table(_counted(scene, out, low=1))


def _weighted_columns_of(scene, weighted, border):
    """the weighted and the border columns: weighted's of every channel, then the border pixels and border's of every channel;
    one clx_region_weighted and one clx_region_border_intensity call per channel"""
    nch = scene.raw.shape[0]
    shift = [scene.channel(k).shift for k in range(nch)]
    out = {}
    for k in range(nch if weighted else 0):
        out.update(weighted_columns(scene.area[scene.present], scene.sum1, _weighted_rows(scene, k), shift[k], scene.nd, k,
                                    scene.spatial))
    for k in range(nch if border else 0):
        table = _border_rows(scene, k)
        if k == 0:
            out.update(border_intensity_columns(table))
        out.update(border_intensity_columns(table, shift[k], scene.channel(k).raw_type, k))
    return out


def weighted_moments(labels, raw, k=0, device=None):
    """The intensity-weighted sums of channel ``k`` of ``raw`` (``(*spatial)`` or ``(C, *spatial)``; float32, float64 or integers
    that fit int32) inside every object of ``labels`` (2-D or 3-D integers, array or device tensor; the same types and range as
    ``region_table``): ``(ids, table, shift)``.  ``ids`` int64 (n): the objects present, ascending.  ``table``:
    ``weighted_table``'s dict of ``clx_region_weighted``'s 21 words per object, exact integers of ``q = rint(v * 2**shift)`` with
    the scale ``region_table`` uses for its ``intensity_mean`` (``intensity_shift``; 0 for integers): int64 arrays ``n`` and
    ``sum_q``, and Python ints ``peak`` (the flat index of the first pixel in raster order that attains the object's maximum)
    and ``sum_qz, sum_qy, sum_qx, sum_qzz, sum_qyy, sum_qxx, sum_qzy, sum_qzx, sum_qyx`` (a 2-D map has z = 0).
    ``weighted_columns`` forms ``region_table``'s columns of the table.  Runs on a HIP device; there is no CPU path."""
    scene = _channel_scene(labels, raw, {"k": int(k)}, device, "weighted_moments")
    return scene.present.astype(np.int64), _weighted_rows(scene, int(k)), 0 if scene.empty else scene.channel(int(k)).shift


def border_intensity(labels, raw, k=0, device=None):
    """The sums of channel ``k`` of ``raw`` over the BORDER pixels of every object of ``labels`` (the arguments of
    ``weighted_moments``): ``(ids, table, shift)``.  A border pixel of object i has a face neighbour (4 in 2-D, 6 in 3-D) that is
    not i: another object, background or the outside of the image.  ``table``: ``border_table``'s dict of
    ``clx_region_border_intensity``'s seven words per object: int64 arrays ``pixels`` (the border pixels), ``n`` (those counted)
    and ``sum_q``, uint64 order keys ``key_min`` and ``key_max`` and Python ints ``sum_qq``, of ``q = rint(v * 2**shift)``.
    ``border_intensity_columns`` forms ``region_table``'s columns of the table.  Runs on a HIP device; there is no CPU path."""
    scene = _channel_scene(labels, raw, {"k": int(k)}, device, "border_intensity")
    return scene.present.astype(np.int64), _border_rows(scene, int(k)), 0 if scene.empty else scene.channel(int(k)).shift


def region_table(labels, raw=None, device=None, boundary=False, topology=False, hull=False, inscribed=False, edge=False,
                 quantiles=None, mad=False, texture=False, texture_levels=8, texture_distance=1, texture_range=None,
                 radial=False, radial_rings=4, radial_width=None, radial_wedges=False, std=False, colocalization=False,
                 coloc_threshold=0.15, granularity=None, granularity_background=0, granularity_levels=256, weighted=False,
                 border_intensity=False):
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
    ``granularity=n`` (an integer in 1 .. 64; needs ``raw``) appends, after all of those, per channel k ``granularity_1_c{k}`` ..
    ``granularity_{n}_c{k}`` and ``granularity_residual_c{k}``: the granular spectrum of the object in that channel, CellProfiler's
    MeasureGranularity without its subsampling (``cellulus_amd.granularity``: ``granularity_table``, ``granularity_columns``), at
    ``granularity_levels`` grey levels (2 .. 65536) over the whole image's range, after a top-hat of radius
    ``granularity_background`` (0 .. 64; 0: none).
    Returns ``dict[str, np.ndarray]``.  Runs on a HIP device; there is no CPU path."""
    return _region_table(labels, raw, device, boundary, topology=topology, hull=hull, inscribed=inscribed, edge=edge, quantiles=quantiles,
                         mad=mad, texture=texture, texture_levels=texture_levels, texture_distance=texture_distance,
                         texture_range=texture_range, radial=radial, radial_rings=radial_rings, radial_width=radial_width,
                         radial_wedges=radial_wedges, std=std, colocalization=colocalization, coloc_threshold=coloc_threshold,
                         weighted=weighted, border_intensity=border_intensity, granularity=granularity,
                         granularity_background=granularity_background, granularity_levels=granularity_levels)[0]


def _region_table(labels, raw, device, boundary, topology=False, hull=False, inscribed=False, edge=False, quantiles=None,
                  mad=False, texture=False, texture_levels=8, texture_distance=1, texture_range=None, radial=False,
                  radial_rings=4, radial_width=None, radial_wedges=False, std=False, colocalization=False, coloc_threshold=0.15,
                  granularity=None, granularity_background=0, granularity_levels=256, weighted=False, border_intensity=False):
    """region_table's columns and, with ``boundary``, contact_pairs' rows (else None)"""
    if granularity is not None:
        from . import granularity as _granularity

        if raw is None:
            raise ValueError("region_table: granularity needs raw")
        granularity, granularity_levels, granularity_background = _granularity._check_table(granularity, granularity_levels,
                                                                                              granularity_background, "region_table")
    quantiles = _check_quantiles(quantiles, mad, raw)
    coloc_threshold = _check_products(std, colocalization, coloc_threshold, labels, raw)
    _check_weighted(weighted, border_intensity, raw)
    if radial:
        radial_rings, radial_width, radial_W = _check_radial(radial_rings, radial_width, radial_wedges, getattr(labels, "ndim", None))
    if texture:
        if raw is None:
            raise ValueError("region_table: texture needs raw")
        texture_levels, texture_distance, texture_range = _check_texture(texture_levels, texture_distance, texture_range)
    scene = _scene(labels, device, "region_table").measured()
    nd, present, area = scene.nd, scene.present, scene.area[scene.present]
    cols = shape_columns(present, area, scene.bbox[present], scene.sum1, scene.sum2, nd)
    if raw is not None:
        scene.raw = _raw_channels(raw, scene.spatial, "region_table")
        for k in range(scene.raw.shape[0]):
            cols.update(scene.channel(k).columns)
    pairs = None
    if boundary:
        pairs = _contacts(scene, len(present))
        classes = _perimeter_classes(scene) if nd == 2 else None
        cols.update(boundary_columns(present, scene.bbox[present], scene.spatial, *pairs, classes, nd))
    if topology:
        cols.update(topology_columns(area, _topology_counts(scene), nd))
    if hull:
        cols.update(hull_columns(area, _hull_rows(scene), nd))
    if inscribed or radial:
        scene.inscribed(edge)                                # one distance map and one reduction for both, formed here
    if inscribed:
        cols.update(inscribed_columns(area, _inscribed_rows(scene, edge), scene.spatial, nd))
    if quantiles or mad:
        cols.update(_order_columns(scene, quantiles, mad))
    if texture:
        cols.update(_texture_columns_of(scene, texture_levels, texture_distance, texture_range))
    if radial:
        count, isums = _radial_tables(scene, edge, radial_rings, radial_width, radial_W)
        cols.update(radial_columns(area, count, nd=nd))
        for k, isum in enumerate(isums):
            cols.update(radial_columns(area, count, isum, scene.channel(k).shift, nd, k))
    if std or colocalization:
        cols.update(_products_columns_of(scene, std, colocalization, coloc_threshold))
    if weighted or border_intensity:
        cols.update(_weighted_columns_of(scene, weighted, border_intensity))
    if granularity is not None:
        cols.update(_granularity._columns_of(scene, scene.raw, granularity, granularity_levels, None, granularity_background, "region_table"))
    return cols, pairs


def measure(inference_config, contacts=False, topology=False, hull=False, inscribed=False, quantiles=None, mad=False, texture=False,
            texture_levels=8, texture_distance=1, radial=False, radial_rings=4, radial_width=None, radial_wedges=False, std=False,
            colocalization=False, coloc_threshold=0.15, granularity=None, granularity_background=0, granularity_levels=256,
            weighted=False, border_intensity=False) -> None:
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
    (``region_table``'s arguments, ``edge=False``); ``granularity=n`` the granular spectrum of every channel at ``n`` scales, with
    ``granularity_background`` and ``granularity_levels`` (``region_table``'s arguments; the levels divide the range of each
    sample's raw channel over the whole image).  Rank 0 works alone under torch.distributed."""
    from .utils import zarr_io

    stage = _stage.begin("measure", inference_config)
    if stage is None:
        return
    stage.open("r")
    dataset_config = inference_config.dataset_config
    ds_seg = stage.f[inference_config.segmentation_dataset_config.dataset_name]
    ds_raw = zarr_io.open(dataset_config.container_path, "r")[dataset_config.dataset_name]

    def per_sample(sample, bandwidth):
        labels = ds_seg[sample, bandwidth].astype(np.int32)
        table, pairs = _region_table(labels, ds_raw[sample], stage.device, contacts, topology=topology, hull=hull, inscribed=inscribed,
                                     quantiles=quantiles, mad=mad, texture=texture, texture_levels=texture_levels,
                                     texture_distance=texture_distance, radial=radial, radial_rings=radial_rings,
                                     radial_width=radial_width, radial_wedges=radial_wedges, std=std,
                                     colocalization=colocalization, coloc_threshold=coloc_threshold, weighted=weighted,
                                     border_intensity=border_intensity, granularity=granularity,
                                     granularity_background=granularity_background, granularity_levels=granularity_levels)
        return (table, dict(zip(_CONTACTS_HEADER[1:], pairs))) if contacts else (table,)

    stage.run(per_sample, ("measurements", "contacts") if contacts else ("measurements",), keep={"contacts": lambda t: t["label_a"] > 0},
              headers={"contacts": list(_CONTACTS_HEADER)})


if __name__ == "__main__":
    from .cli import measure as _command

    _command()
