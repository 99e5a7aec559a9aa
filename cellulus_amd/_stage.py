"""What the label stages (``measure``, ``relate``, ``expand``, ``split``, ``propagate``, ``fill``, ``skeleton``, ``granularity``) share on the
host around their device work: rank 0 reads label datasets ``[sample, bandwidth, ...]`` of the segmentation container, writes a new one
and one or two CSV files per bandwidth.  A stage checks its own arguments on every rank, then

    stage = _stage.begin(who, inference_config)          # None on every rank but 0; the metadata is read
    if stage is None:
        return
    stage.open(mode, *names)                             # the device, the container, "no dataset ..."
    stage.refuse_existing(output)                        # "a dataset ... exists ... already"
    ds = stage.create(output)                            # uint16 [sample, bandwidth, *spatial]
    stage.run(per_sample, stems)                         # the loops and the CSV files

with checks of its own between any two steps.  Host only; it imports none of the stage modules."""

import numpy as np

from .measure_columns import _format


def _create(f, name, shape, dtype, nd):
    ds = f.create_dataset(name, shape=shape, dtype=dtype)
    ds.attrs["axis_names"] = ["s", "c"] + ["t", "z", "y", "x"][-nd:]
    ds.attrs["resolution"] = (1,) * nd
    ds.attrs["offset"] = (0,) * nd
    return ds


def _write_csv(path, header, lines):
    with open(path, "w") as out:
        out.write(",".join(header or ["sample"]) + "\n")
        for line in lines:
            out.write(line + "\n")


def begin(who, inference_config):
    """-> the ``_Stage`` of rank 0 with the dataset's metadata read; None on every other rank, before any file is opened"""
    from . import parallel
    from .datasets.meta_data import DatasetMetaData

    if parallel.rank() != 0:
        return None
    return _Stage(who, inference_config, DatasetMetaData.from_dataset_config(inference_config.dataset_config))


class _Stage:
    """One run of a stage on rank 0: ``who`` names it in the messages, ``config`` is the inference config, ``meta`` the
    dataset's metadata, ``nd`` its spatial dimensions, ``path`` the segmentation container; after ``open()`` ``device`` and
    ``f``, the container."""

    def __init__(self, who, config, meta):
        self.who, self.config, self.meta, self.nd = who, config, meta, meta.num_spatial_dims
        self.path = config.segmentation_dataset_config.container_path
        self.device = self.f = None

    def open(self, mode, *names):
        """requires the HIP device, opens the container (``mode`` "r" or "a") and refuses a name (None: not asked for) that
        is no dataset of it"""
        import torch

        from . import parallel
        from .train import _require_hip_device
        from .utils import zarr_io

        self.device = _require_hip_device(self.config.device)
        if parallel.world_size() > 1:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.f = zarr_io.open(self.path, mode)
        for name in names:
            if name is not None and name not in self.f:
                raise ValueError(f"{self.who}: no dataset {name!r} in {self.path}")

    def refuse_existing(self, output):
        if output in self.f:
            raise ValueError(f"{self.who}: a dataset {output!r} exists in {self.path} already")

    def create(self, name):
        """-> a new uint16 dataset ``[sample, bandwidth, *spatial]`` of the container"""
        return _create(self.f, name, (self.meta.num_samples, self.config.num_bandwidths, *self.meta.spatial_array), np.uint16, self.nd)

    def run(self, per_sample, stems, keep=None, headers=None):
        """For every bandwidth, for every sample: ``per_sample(sample, bandwidth)`` -> one table (a dict of columns of one
        length) per entry of ``stems``; their rows, ``sample`` first, go to ``<stem>_bandwidth-<b>.csv`` in the working
        directory.  A file's header is ``headers[stem]`` where that is given, else ``sample`` and the columns of the first
        table seen (``sample`` alone where there was none); of a table with ``keep[stem]`` the rows where that function of the
        table is true are written."""
        keep, headers = keep or {}, headers or {}
        for bandwidth in range(self.config.num_bandwidths):
            header, lines = [headers.get(stem) for stem in stems], [[] for _ in stems]
            for sample in range(self.meta.num_samples):
                for k, table in enumerate(per_sample(sample, bandwidth)):
                    header[k] = header[k] or ["sample"] + list(table)
                    columns = list(table.values())
                    rows = np.flatnonzero(keep[stems[k]](table)) if stems[k] in keep else range(len(columns[0]))
                    lines[k] += [",".join([str(sample)] + [_format(c[i]) for c in columns]) for i in rows]
            for k, stem in enumerate(stems):
                _write_csv(f"{stem}_bandwidth-{bandwidth}.csv", header[k], lines[k])
