"""`ZarrDataset` — random crops + pair coordinates, the producer side of
``train_iteration`` (cellulus/datasets/zarr_dataset.py:12-251).

The reference builds a gunpowder pipeline (ZarrSource -> RandomLocation ->
Normalize [-> ElasticAugment]); gunpowder and zarr are absent here, so the
pipeline is restated on numpy/scipy: uniform random sample + spatial offset,
``float32(data) * factor`` normalisation, optional elastic deformation
(jittered control-point grid + rotation in [0, pi/2] + scale in [0.9, 1.1],
linear interpolation), rejection of all-zero crops (zarr_dataset.py:139-158).
The pair sampler (`sample_coordinates`, `sample_offsets_within_radius`) follows
zarr_dataset.py:177-251 call for call on the global numpy RNG, so seeding
``np.random`` reproduces the reference's coordinates.

Opt-in (``CLX_DEVICE_AUGMENT=1``): `DeviceCropSource` makes the same crops on the device
from the same kind of draws (``ZarrDataset.elastic_params`` + ``clx_elastic_crop``).
"""

import math
import os
import random
from typing import Tuple

import numpy as np
from torch.utils.data import IterableDataset

from ..configs import DatasetConfig
from ..utils import zarr_io
from .meta_data import DatasetMetaData


def default_normalization_factor(dtype):
    """gunpowder.Normalize(factor=None): scale integer types to [0, 1]."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return 1.0 / 255
    if dtype == np.uint16:
        return 1.0 / 65535
    if dtype.kind == "f":
        return 1.0
    raise RuntimeError(f"automatic normalization is not implemented for dtype {dtype}; "
                       "set normalization_factor")


_BLAS_LIMIT = None


def _single_threaded_blas():
    """Inside a loader process: numpy's BLAS on ONE thread.  The augmentation's small matrix products (a 2 x 2 rotation
    over 65 536 grid points, the spline matrices over the jitter grids) are enough for OpenBLAS to wake its whole
    pool — one thread per host core, per loader process — and eight such pools spinning beside each other made the
    crops' times jitter: `train()` lost 4 % against the step rate on some hosts and nothing on others (round 5)."""
    global _BLAS_LIMIT
    if _BLAS_LIMIT is None:
        try:
            from threadpoolctl import threadpool_limits

            _BLAS_LIMIT = threadpool_limits(limits=1)
        except Exception:            # (threadpoolctl absent: nothing to limit with)
            _BLAS_LIMIT = False


class ZarrDataset(IterableDataset):  # type: ignore
    def __init__(
        self,
        dataset_config: DatasetConfig,
        crop_size: Tuple[int, ...],
        elastic_deform: bool,
        control_point_spacing: int,
        control_point_jitter: float,
        density: float,
        kappa: float,
        normalization_factor: float,
    ):
        self.dataset_config = dataset_config
        self.crop_size = tuple(crop_size)
        self.elastic_deform = elastic_deform
        self.control_point_spacing = control_point_spacing
        self.control_point_jitter = control_point_jitter
        self.normalization_factor = normalization_factor
        self.__read_meta_data()
        assert len(crop_size) == self.num_spatial_dims, (
            f'"crop_size" must have the same dimension as the spatial(temporal) dimensions of the '
            f'"{self.dataset_config.dataset_name}" dataset which is {self.num_spatial_dims}, '
            f"but it is {crop_size}")
        self.density = density
        self.kappa = kappa
        self.output_shape = tuple(int(_ - 16) for _ in self.crop_size)
        self.unbiased_shape = tuple(int(_ - (2 * self.kappa)) for _ in self.output_shape)
        self._array = None
        # opt-in (CLX_DEVICE_PAIRS=1, set by train()): the crops come without coordinates and the pairs
        # are drawn on the device (DevicePairSampler) — same distribution, not the reference's stream
        self.skip_pairs = False

    def __iter__(self):
        import torch.utils.data

        if torch.utils.data.get_worker_info() is not None:
            _single_threaded_blas()
        return iter(self.__yield_sample())

    # ------------------------------------------------------------------ source
    def _open(self):
        if self._array is None:
            container = zarr_io.open(self.dataset_config.container_path, "r")
            self._array = container[self.dataset_config.dataset_name]
            for size, crop in zip(self._array.shape[2:], self.crop_size):
                if size < crop:
                    raise RuntimeError(f"crop_size {self.crop_size} exceeds the dataset's spatial "
                                       f"extent {self._array.shape[2:]}")
        return self._array

    def _random_crop(self):
        arr = self._open()
        s = random.randint(0, arr.shape[0] - 1)
        factor = self.normalization_factor
        if factor is None:
            factor = default_normalization_factor(arr.dtype)
        spatial = arr.shape[2:]
        if not self.elastic_deform:
            off = [random.randint(0, n - c) for n, c in zip(spatial, self.crop_size)]
            sl = (s, slice(None)) + tuple(slice(o, o + c) for o, c in zip(off, self.crop_size))
            return arr[sl].astype(np.float32) * np.float32(factor)
        return self._elastic_crop(arr, s, factor)

    def _elastic_ops(self):
        """What the elastic augmentation needs per crop and never changes: the crop's pixel grid relative to its centre,
        and — cubic-spline up-sampling being linear and separable — one (crop extent x control points) matrix per axis
        that maps a control-point grid to its up-sampled field, obtained from scipy's ``zoom`` itself on unit vectors
        (the same numbers as zooming every crop's jitter grid, which cost 8 ms per axis and crop)."""
        ops = getattr(self, "_elastic_cache", None)
        if ops is None:
            from scipy.ndimage import zoom

            nd = self.num_spatial_dims
            grid = np.stack(np.meshgrid(*[np.arange(c, dtype=np.float64) for c in self.crop_size], indexing="ij"))
            centre = (np.asarray(self.crop_size, dtype=np.float64) - 1) / 2
            rel0 = grid - centre.reshape((nd,) + (1,) * nd)
            cp_shape = [max(2, int(math.ceil(c / self.control_point_spacing)) + 1) for c in self.crop_size]
            mats = [zoom(np.eye(p), [c / p, 1.0], order=3, mode="nearest", grid_mode=False)[:c]
                    for c, p in zip(self.crop_size, cp_shape)]
            ops = self._elastic_cache = (rel0, cp_shape, mats)
        return ops

    def _elastic_crop(self, arr, s, factor):
        from scipy.ndimage import map_coordinates

        nd = self.num_spatial_dims
        rel0, cp_shape, mats = self._elastic_ops()
        spatial = np.asarray(arr.shape[2:], dtype=np.float64)
        angle = random.uniform(0, math.pi / 2)
        scale = random.uniform(0.9, 1.1)
        rot = np.eye(nd)
        c_, s_ = math.cos(angle), math.sin(angle)
        rot[-2:, -2:] = [[c_, -s_], [s_, c_]]          # rotate in the (y, x) plane
        rel = np.tensordot(rot, rel0, axes=1) * scale
        for d in range(nd):
            field = np.random.normal(0.0, self.control_point_jitter, size=cp_shape)
            for axis, m in enumerate(mats):            # up-sample axis by axis: field <- m applied along `axis`
                field = np.moveaxis(np.tensordot(m, field, axes=(1, axis)), 0, axis)
            rel[d] += field
        lo, hi = rel.reshape(nd, -1).min(axis=1), rel.reshape(nd, -1).max(axis=1)
        room = spatial - 1 - (hi - lo)
        mode = "constant" if np.all(room >= 0) else "reflect"
        origin = np.array([random.uniform(0, max(r, 0)) for r in room]) - lo
        coords = rel + origin.reshape((nd,) + (1,) * nd)
        data = arr[s].astype(np.float32) * np.float32(factor)
        out = np.stack([map_coordinates(ch, coords, order=1, mode=mode, cval=0.0) for ch in data])
        return out.astype(np.float32)

    def elastic_params(self, array_shape, py_rng=random, np_rng=np.random):
        """The random numbers of one crop, without touching image data: exactly the draws ``_random_crop`` (+
        ``_elastic_crop``) consume from ``random`` / ``np.random``, in their order, so that the two generators end in the
        same state as after a host crop.  ``array_shape``: the data set's ``(S, C, *spatial)``.

        Elastic: ``dict(s, angle, scale, grids, u)`` — ``grids`` the ``nd`` jittered control-point grids, ``u`` the
        ``nd`` uniform numbers behind the placement: ``_elastic_crop`` calls ``random.uniform(0, max(room_d, 0))``, which
        is ``max(room_d, 0) * random()`` — the draw does not depend on ``room``, so it is taken here and the origin is
        formed later as ``u_d * max(room_d, 0) - lo_d`` (``clx_elastic_crop`` does, on the device).
        Plain crop: ``dict(s, offsets)``."""
        s = py_rng.randint(0, array_shape[0] - 1)
        if not self.elastic_deform:
            off = [py_rng.randint(0, n - c) for n, c in zip(array_shape[2:], self.crop_size)]
            return dict(s=s, offsets=off)
        _rel0, cp_shape, _mats = self._elastic_ops()
        angle = py_rng.uniform(0, math.pi / 2)
        scale = py_rng.uniform(0.9, 1.1)
        grids = [np_rng.normal(0.0, self.control_point_jitter, size=cp_shape) for _ in range(self.num_spatial_dims)]
        u = [py_rng.random() for _ in range(self.num_spatial_dims)]
        return dict(s=s, angle=angle, scale=scale, grids=grids, u=u)

    def pack_params(self, params):
        """``elastic_params`` results -> the float64 records ``clx_elastic_crop`` reads (include/clx.h), one row per crop."""
        nd = self.num_spatial_dims
        rows = []
        for q in params:
            if not self.elastic_deform:
                rows.append(np.asarray([q["s"], *q["offsets"]], dtype=np.float64))
                continue
            rot = np.eye(nd)
            c_, s_ = math.cos(q["angle"]), math.sin(q["angle"])
            rot[-2:, -2:] = [[c_, -s_], [s_, c_]]          # rotate in the (y, x) plane, as _elastic_crop
            rows.append(np.concatenate([[float(q["s"])], (rot * q["scale"]).ravel(), np.asarray(q["u"], dtype=np.float64),
                                        *[np.asarray(g, dtype=np.float64).ravel() for g in q["grids"]]]))
        return np.ascontiguousarray(np.stack(rows), dtype=np.float64)

    def __yield_sample(self):
        """An infinite generator of crops."""
        while True:
            array_is_zero = True
            while array_is_zero:   # reject empty crops (zarr_dataset.py:139-158)
                sample_data = self._random_crop()
                if np.max(sample_data) <= 0.0:
                    continue
                array_is_zero = False
                if self.skip_pairs:
                    anchor_samples = reference_samples = np.zeros((0, self.num_spatial_dims), dtype=np.int64)
                else:
                    anchor_samples, reference_samples = self.sample_coordinates()
            yield sample_data, anchor_samples, reference_samples

    def __read_meta_data(self):
        meta_data = DatasetMetaData.from_dataset_config(self.dataset_config)
        self.num_dims = meta_data.num_dims
        self.num_spatial_dims = meta_data.num_spatial_dims
        self.num_channels = meta_data.num_channels
        self.num_samples = meta_data.num_samples
        self.sample_dim = meta_data.sample_dim
        self.channel_dim = meta_data.channel_dim
        self.time_dim = meta_data.time_dim

    def get_num_channels(self):
        return self.num_channels

    def get_num_spatial_dims(self):
        return self.num_spatial_dims

    # ------------------------------------------------------------ pair sampler
    def sample_offsets_within_radius(self, radius, number_offsets):
        """zarr_dataset.py:185-198.  Same offsets and the same state of numpy's global generator afterwards as the
        reference's code; drawn by libclx's host function (MT19937 + numpy's masked rejection restated in C: 20 -> 4 ms
        for a 256^2 crop's 196 850 pairs) when that generator is the legacy MT19937 and the radius an integer, by numpy
        (`_sample_offsets_numpy`) otherwise."""
        nd = self.num_spatial_dims
        if os.environ.get("CLX_NATIVE_PAIR_SAMPLER", "1") != "0" and float(radius).is_integer() and 1 <= radius < 16384:
            state = np.random.get_state(legacy=True)
            if state[0] == "MT19937":
                import ctypes

                from .. import _clx

                key = np.ascontiguousarray(state[1], dtype=np.uint32).copy()
                pos = ctypes.c_int(int(state[2]))
                offsets = np.empty((number_offsets, nd), dtype=np.int64)
                _clx.call("clx_sample_offsets_mt19937", key.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pos),
                          int(radius), nd, int(number_offsets), offsets.ctypes.data_as(ctypes.c_void_p), None)
                np.random.set_state(("MT19937", key, pos.value, state[3], state[4]))
                return offsets
        return self._sample_offsets_numpy(radius, number_offsets)

    def _sample_offsets_numpy(self, radius, number_offsets):
        # (the reference stacks the draws, filters twice with temporaries of the full size and slices: 19 of the 31 ms
        #  a 256^2 crop's pairs cost; the same draws in the same order, one combined mask, the survivors gathered once)
        nd = self.num_spatial_dims
        draws = [np.random.randint(-radius, radius + 1, size=nd * number_offsets) for _ in range(nd)]
        sq = draws[0] * draws[0]
        for d in draws[1:]:
            sq += d * d
        keep = np.flatnonzero((sq < radius ** 2) & (sq > 0))     # (integers: |o|_1 > 0 <=> |o|^2 > 0)
        if len(keep) < number_offsets:
            return self._sample_offsets_numpy(radius, number_offsets)
        keep = keep[:number_offsets]
        offsets = np.empty((number_offsets, nd), dtype=draws[0].dtype)
        for d in range(nd):
            offsets[:, d] = draws[d][keep]
        return offsets

    def sample_coordinates(self):
        num_anchors = self.get_num_anchors()
        num_references = self.get_num_references()
        columns = [np.random.randint(self.kappa, self.output_shape[d] - self.kappa + 1, size=num_anchors)
                   for d in range(self.num_spatial_dims)]
        anchor_coordinates = np.stack(columns, axis=1)
        anchor_samples = np.repeat(anchor_coordinates, num_references, axis=0)
        offset_in_pos_radius = self.sample_offsets_within_radius(self.kappa, len(anchor_samples))
        reference_samples = anchor_samples + offset_in_pos_radius
        return anchor_samples, reference_samples

    def get_num_anchors(self):
        return int(self.density * self.unbiased_shape[0] * self.unbiased_shape[1])

    def get_num_references(self):
        return int(self.density * self.kappa ** 2 * np.pi)

    def get_num_samples(self):
        return self.get_num_anchors() * self.get_num_references()


class DevicePairSampler:
    """Pairs with the distribution of ``ZarrDataset.sample_coordinates`` drawn by ``clx_sample_pairs``
    on the device: anchor column d uniform on the integers [kappa, output_shape[d] - kappa], every
    anchor repeated ``get_num_references()`` times, reference = anchor + an offset uniform over
    {o integer: |o|^2 < kappa^2, o != 0} (what the rejection loop of ``sample_offsets_within_radius``
    converges to).  Counter-based generator: (seed, step) reproduces a batch.  Opt-in: the numbers
    are NOT the reference's ``np.random`` stream."""

    def __init__(self, dataset, device, seed):
        import ctypes
        import itertools

        import torch

        self.device = device
        self.nd = dataset.num_spatial_dims
        kappa = float(dataset.kappa)
        self.lo = int(math.ceil(kappa))
        self.hi = [int(math.floor(s - kappa)) for s in dataset.output_shape]
        if any(h < self.lo for h in self.hi):
            raise ValueError(f"kappa={kappa} leaves no anchor position in an output of extent {dataset.output_shape}")
        r = range(int(math.ceil(-kappa)), int(math.floor(kappa)) + 1)
        table = [o for o in itertools.product(r, repeat=self.nd)
                 if sum(v * v for v in o) < kappa * kappa and sum(abs(v) for v in o) > 0]
        if not table:
            raise ValueError(f"kappa={kappa} admits no offset")
        self.offsets = torch.tensor(table, dtype=torch.int32, device=device).contiguous()
        self.num_anchors = dataset.get_num_anchors()
        self.num_refs = dataset.get_num_references()
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._hi_c = (ctypes.c_int * self.nd)(*self.hi)

    def sample(self, batch_size, step):
        import torch

        from .. import _clx

        P = self.num_anchors * self.num_refs
        anchor = torch.empty((batch_size, P, self.nd), dtype=torch.int64, device=self.device)
        reference = torch.empty_like(anchor)
        _clx.call("clx_sample_pairs", _clx.ptr(anchor), _clx.ptr(reference), _clx.ptr(self.offsets),
                  self.offsets.shape[0], batch_size, self.num_anchors, self.num_refs, self.nd, self.lo, self._hi_c,
                  self.seed, int(step) & 0xFFFFFFFFFFFFFFFF, _clx.stream_ptr(self.device))
        return anchor, reference


_AUG_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}     # enum clx_aug_dtype


def elastic_crop_on_device(dataset, data, shape, stored_dtype, factor, records, device, out=None, maxima=None):
    """``clx_elastic_crop`` for ``records`` (``ZarrDataset.pack_params``: a float64 numpy array, or a device tensor of
    it) on the current stream of ``device``.  ``data``: the device-resident data set of ``shape = (S, C, *spatial)``
    as a tensor of its bytes, element type ``stored_dtype`` (uint8, uint16 or float32); ``dataset`` supplies the crop
    size and the augmentation's settings.  Returns ``(raw, maxima)``: ``(B, C, *crop)`` float32 and ``max(raw[b])``."""
    import ctypes

    import torch

    from .. import _clx

    nd = dataset.num_spatial_dims
    shape = tuple(int(n) for n in shape)
    B = int(records.shape[0])
    if not torch.is_tensor(records):
        records = np.ascontiguousarray(records, dtype=np.float64)
        s = records[:, 0]
        if s.min() < 0 or s.max() >= shape[0]:
            raise IndexError(f"sample index outside [0, {shape[0]})")
        records = torch.from_numpy(records).pin_memory().to(device, non_blocking=True)
    _clx.require_device(records, "records")
    crop = (ctypes.c_int * nd)(*dataset.crop_size)
    spatial = (ctypes.c_int * nd)(*shape[2:])
    if out is None:
        out = torch.empty((B, shape[1]) + tuple(dataset.crop_size), dtype=torch.float32, device=device)
    if maxima is None:
        maxima = torch.empty(B, dtype=torch.float32, device=device)
    cp_c = mats = work = None
    if dataset.elastic_deform:
        cache = getattr(dataset, "_device_elastic_cache", None)
        if cache is None or cache[0] != device:
            _rel0, cp_shape, m = dataset._elastic_ops()
            flat = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in m])
            cache = dataset._device_elastic_cache = (device, list(cp_shape), torch.from_numpy(flat).to(device))
        cp_c = (ctypes.c_int * nd)(*cache[1])
        mats = cache[2]
        need = int(_clx.load().clx_elastic_crop_workspace(nd, crop, B))
        work = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    _clx.call("clx_elastic_crop", _clx.ptr(data), _AUG_DTYPES[np.dtype(stored_dtype)], shape[0], shape[1], nd, spatial,
              crop, cp_c, float(np.float32(factor)), int(bool(dataset.elastic_deform)), B, _clx.ptr(records),
              _clx.ptr(mats), _clx.ptr(work), _clx.ptr(out), _clx.ptr(maxima), _clx.stream_ptr(device))
    return out, maxima


class DeviceCropSource:
    """The crops of ``ZarrDataset`` made on the device (opt-in: ``CLX_DEVICE_AUGMENT=1``): the data set is uploaded once,
    the random numbers of every crop are drawn on the host (``ZarrDataset.elastic_params``, from private generators), and
    ``clx_elastic_crop`` builds the deformation field, resamples and takes the maximum of every crop of a batch in one
    call.  An iterable of ``(raw,)`` batches that are already device tensors: it stands where the DataLoader stands, in
    front of ``train._DevicePrefetcher``, starts no process, and its kernels run on the stream it is given
    (``use_stream``: the prefetcher's side stream).

    One batch is kept in flight: a call launches the batch after the one it returns, so the maxima it reads back
    (one small D2H copy) were written a training step earlier and the host does not wait for the device.

    Empty-crop rule (``np.max(crop) <= 0`` -> draw again, zarr_dataset.py:139-158): the rejected crops of a batch, and
    only they, get new parameters and are made again until none is left — the host path's distribution.  The host path
    redraws crop ``b`` before it draws crop ``b + 1``; here a batch is drawn first and its rejects afterwards, so the
    host's stream ORDER is reproduced only while no crop is rejected.

    ``DeviceCropSource.decide`` tells, without a device, whether a data set can be served (budget
    ``CLX_DEVICE_AUGMENT_MB``, default 8192; crop within the data set) and why not."""

    SEED_OFFSET = 104729

    @staticmethod
    def decide(dataset, budget_mb=None):
        """(True, summary) or (False, reason): never raises what the host loader would not raise."""
        if budget_mb is None:
            budget_mb = float(os.environ.get("CLX_DEVICE_AUGMENT_MB", "8192"))
        container = zarr_io.open(dataset.dataset_config.container_path, "r")
        arr = container[dataset.dataset_config.dataset_name]
        shape, dtype = tuple(arr.shape), np.dtype(arr.dtype)
        if any(n < c for n, c in zip(shape[2:], dataset.crop_size)):
            return False, (f"crop_size {dataset.crop_size} exceeds the data set's spatial extent {shape[2:]}: "
                           "the host loader reports it")
        if dataset.normalization_factor is None and dtype not in _AUG_DTYPES and dtype.kind != "f":
            return False, f"no automatic normalization for dtype {dtype}: the host loader reports it"
        itemsize = dtype.itemsize if dtype in _AUG_DTYPES else 4
        mb = float(np.prod(shape, dtype=np.float64)) * itemsize / 2 ** 20
        if mb > budget_mb:
            return False, (f"the data set takes {mb:.0f} MB on the device, over the budget of {budget_mb:.0f} MB "
                           "(CLX_DEVICE_AUGMENT_MB)")
        if dataset.elastic_deform:
            _rel0, cp_shape, _m = dataset._elastic_ops()
            lds = 8 * (sum(c * p for c, p in zip(dataset.crop_size, cp_shape))
                       + dataset.num_spatial_dims * (dataset.num_spatial_dims + 1 + int(np.prod(cp_shape))))
            if lds > 60000:
                return False, (f"control_point_spacing {dataset.control_point_spacing} gives {cp_shape} control points: "
                               f"{lds} bytes of LDS per block, over clx_elastic_crop's 60000")
        return True, f"{mb:.1f} MB {dtype} {shape} resident on the device"

    def __init__(self, dataset, device, batch_size, seed):
        import torch

        self.dataset = dataset
        self.device = device
        self.batch_size = int(batch_size)
        container = zarr_io.open(dataset.dataset_config.container_path, "r")
        arr = container[dataset.dataset_config.dataset_name]
        host = np.ascontiguousarray(arr[...])
        self.factor = dataset.normalization_factor
        if self.factor is None:
            self.factor = default_normalization_factor(host.dtype)
        if host.dtype not in _AUG_DTYPES:
            host = host.astype(np.float32)               # what the host path makes of it before it multiplies
        self.stored_dtype = host.dtype
        self.shape = tuple(host.shape)
        self.data = torch.from_numpy(host.view(np.uint8).reshape(-1)).to(device)
        seed = int(seed) + self.SEED_OFFSET
        self.py_rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed % 2 ** 32)
        self.stream = None
        self.rejected = 0                                # crops drawn again under the empty-crop rule
        self._flying = None

    def use_stream(self, stream):
        self.stream = stream

    def _launch(self, count, out=None, maxima=None):
        params = [self.dataset.elastic_params(self.shape, self.py_rng, self.np_rng) for _ in range(count)]
        return elastic_crop_on_device(self.dataset, self.data, self.shape, self.stored_dtype, self.factor,
                                      self.dataset.pack_params(params), self.device, out, maxima)

    def _start(self):
        """Launch one batch and the copy of its maxima: (raw, maxima, pinned host maxima, event behind the copy)."""
        import torch

        raw, maxima = self._launch(self.batch_size)
        host = torch.empty(self.batch_size, dtype=torch.float32).pin_memory()
        host.copy_(maxima, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        return raw, maxima, host, done

    def _finish(self, flying):
        """Wait for a launched batch and make its empty crops again until none is left."""
        import torch

        raw, maxima, host, done = flying
        done.synchronize()
        while True:
            empty = np.flatnonzero(host.numpy() <= 0.0)
            if len(empty) == 0:
                return raw
            self.rejected += len(empty)
            for b in empty:
                self._launch(1, raw[b:b + 1], maxima[b:b + 1])
            host.copy_(maxima, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()

    def __iter__(self):
        return self

    def __next__(self):
        import torch

        if self.stream is None:
            self.stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self.stream):
            if self._flying is None:
                self._flying = self._start()
            raw = self._finish(self._flying)
            self._flying = self._start()
        raw.record_stream(torch.cuda.current_stream(self.device))      # made on self.stream, read by the caller's
        return (raw,)
