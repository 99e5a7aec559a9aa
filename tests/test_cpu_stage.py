"""The plumbing the label stages share (cellulus_amd/_stage.py) without a device: the CSV files byte for byte from tables
written by hand, the dataset it creates in 2-D and 3-D, its two refusals and what they leave behind, rank 0 working alone and
the read-only mode."""

import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from cellulus_amd import _stage, parallel
from cellulus_amd.utils import zarr_io

SHAPES = {2: (5, 6), 3: (3, 4, 5)}
AXES = {2: ["s", "c", "y", "x"], 3: ["s", "c", "z", "y", "x"]}
DEVICE = "the device the stage was given"


@pytest.fixture
def config(tmp_path, monkeypatch, request):
    """an inference config over a container of 2 samples and 2 bandwidths (2-D unless the test asks for ``nd = 3``), in an
    empty working directory, with the device requirement answered by a stub"""
    nd = getattr(request, "param", 2)
    container = str(tmp_path / "data.zarr")
    f = zarr_io.open(container)
    f["raw"] = np.zeros((2, 1) + SHAPES[nd], np.uint16)
    f["cells"] = np.arange(4 * math.prod(SHAPES[nd])).reshape((2, 2) + SHAPES[nd]).astype(np.uint16)
    for name in ("raw", "cells"):
        f[name].attrs["axis_names"] = AXES[nd]
    os.mkdir(tmp_path / "work")
    monkeypatch.chdir(tmp_path / "work")
    monkeypatch.setattr("cellulus_amd.train._require_hip_device", lambda device: DEVICE)
    return SimpleNamespace(device="cuda:0", num_bandwidths=2, dataset_config=SimpleNamespace(container_path=container, dataset_name="raw"),
                           segmentation_dataset_config=SimpleNamespace(container_path=container))


def tree(config):
    """every file of the container with its size"""
    root = config.segmentation_dataset_config.container_path
    return sorted((os.path.relpath(os.path.join(d, name), root), os.path.getsize(os.path.join(d, name)))
                  for d, _, names in os.walk(root) for name in names)


def a_stage(config, source, output, per_sample, stems, **files):
    """a stage as the five are written: the shared steps in their order, ``output=None`` for one that only reads"""
    stage = _stage.begin("a_stage", config)
    if stage is None:
        return None
    stage.open("a" if output else "r", source)
    if output:
        stage.refuse_existing(output)
        ds = stage.create(output)
        ds[0, 0] = stage.f[source][1, 1]
    stage.run(per_sample, stems, **files)
    return stage


def objects(sample, bandwidth):
    """sample 0 has three rows, sample 1 none"""
    n = 0 if sample else 3
    return {"label": np.array([3, 5, 1 << 40][:n], dtype=np.int64) + bandwidth, "value": np.array([0.1, math.nan, -math.inf][:n]),
            "count": np.array([7, 0, -2][:n], dtype=np.int32)}


def pairs(sample, bandwidth):
    return {"label_a": np.array([0, 0, 1, 2], dtype=np.int64), "label_b": np.array([1, 2, 2, 3 + sample], dtype=np.int64),
            "faces": np.array([9, 8, 0.5, 2.0]) * (1 + bandwidth)}


def test_csv_files_byte_for_byte(config):
    calls = []

    def per_sample(sample, bandwidth):
        calls.append((sample, bandwidth))
        return objects(sample, bandwidth), pairs(sample, bandwidth)

    stage = a_stage(config, "cells", None, per_sample, ("objects", "pairs"), keep={"pairs": lambda table: table["label_a"] > 0})
    assert stage.device == DEVICE and stage.nd == 2
    assert calls == [(0, 0), (1, 0), (0, 1), (1, 1)]                     # for every bandwidth, for every sample
    assert sorted(os.listdir(".")) == [f"{stem}_bandwidth-{b}.csv" for stem in ("objects", "pairs") for b in (0, 1)]
    assert open("objects_bandwidth-0.csv", "rb").read() == (b"sample,label,value,count\n" b"0,3,0.10000000000000001,7\n" b"0,5,nan,0\n"
                                                            b"0,1099511627776,-inf,-2\n")
    assert open("objects_bandwidth-1.csv", "rb").read() == (b"sample,label,value,count\n" b"0,4,0.10000000000000001,7\n" b"0,6,nan,0\n"
                                                            b"0,1099511627777,-inf,-2\n")
    # the rows with label_a == 0 are dropped, the others stay in sample order
    assert open("pairs_bandwidth-0.csv", "rb").read() == b"sample,label_a,label_b,faces\n" b"0,1,2,0.5\n" b"0,2,3,2\n" b"1,1,2,0.5\n" b"1,2,4,2\n"
    assert open("pairs_bandwidth-1.csv", "rb").read() == b"sample,label_a,label_b,faces\n" b"0,1,2,1\n" b"0,2,3,4\n" b"1,1,2,1\n" b"1,2,4,4\n"
    # without the filter every row is written
    a_stage(config, "cells", None, lambda s, b: (pairs(s, b),), ("all_pairs",))
    assert open("all_pairs_bandwidth-0.csv", "rb").read().startswith(b"sample,label_a,label_b,faces\n" b"0,0,1,9\n" b"0,0,2,8\n" b"0,1,2,0.5\n")
    assert len(open("all_pairs_bandwidth-0.csv", "rb").read().splitlines()) == 1 + 2 * 4


def test_header_of_a_run_without_rows(config):
    a_stage(config, "cells", None, lambda s, b: (), ("none",))           # no table at all: the header is the sample column
    assert open("none_bandwidth-0.csv", "rb").read() == open("none_bandwidth-1.csv", "rb").read() == b"sample\n"
    a_stage(config, "cells", None, lambda s, b: (objects(1, b),), ("empty",))       # tables without rows still name their columns
    assert open("empty_bandwidth-1.csv", "rb").read() == b"sample,label,value,count\n"
    a_stage(config, "cells", None, lambda s, b: (pairs(s, b),), ("filtered",), keep={"filtered": lambda table: table["label_a"] > 2})
    assert open("filtered_bandwidth-0.csv", "rb").read() == b"sample,label_a,label_b,faces\n"
    a_stage(config, "cells", None, lambda s, b: (), ("fixed",), headers={"fixed": ["sample", "label_a", "label_b", "faces"]})
    assert open("fixed_bandwidth-0.csv", "rb").read() == b"sample,label_a,label_b,faces\n"
    a_stage(config, "cells", None, lambda s, b: (), ())                  # no file asked for: none written
    assert len(os.listdir(".")) == 2 * 4


@pytest.mark.parametrize("config", [2, 3], indirect=True, ids=["2d", "3d"])
def test_created_dataset(config):
    stage = a_stage(config, "cells", "copy", lambda s, b: (), ())
    nd = stage.nd
    ds = zarr_io.open(config.segmentation_dataset_config.container_path, "r")["copy"]
    assert ds.shape == (2, 2) + SHAPES[nd] and ds.dtype == np.uint16
    assert ds.attrs["axis_names"] == AXES[nd] and list(ds.attrs["resolution"]) == [1] * nd and list(ds.attrs["offset"]) == [0] * nd
    assert sorted(ds.attrs.keys()) == ["axis_names", "offset", "resolution"]
    cells = zarr_io.open(config.segmentation_dataset_config.container_path, "r")["cells"]
    assert np.array_equal(ds[0, 0], cells[1, 1]) and not ds[1].any()
    # detect's datasets are made by the same function, with a shape and a dtype of their own
    other = _stage._create(stage.f, "embeddings", (2, nd + 1) + SHAPES[nd], float, nd)
    assert other.dtype == np.float64 and other.shape == (2, nd + 1) + SHAPES[nd] and other.attrs["axis_names"] == AXES[nd]


def test_refusals_change_nothing(config):
    path = config.segmentation_dataset_config.container_path
    before = tree(config)

    def never(sample, bandwidth):
        raise AssertionError("a refused stage has nothing to measure")

    with pytest.raises(ValueError) as refusal:
        a_stage(config, "cell", "copy", never, ("objects",))
    assert str(refusal.value) == f"a_stage: no dataset 'cell' in {path}"
    with pytest.raises(ValueError) as refusal:
        a_stage(config, "cells", "raw", never, ("objects",))
    assert str(refusal.value) == f"a_stage: a dataset 'raw' exists in {path} already"
    with pytest.raises(ValueError, match="^a_stage: no dataset 'cell' in "):
        a_stage(config, "cell", None, never, ("objects",))
    stage = _stage.begin("a_stage", config)
    stage.open("a", "cells", None, "raw")                                # a name that is None was not asked for
    with pytest.raises(ValueError, match="^a_stage: no dataset 'mask' in "):
        stage.open("a", "cells", None, "mask")
    assert tree(config) == before and os.listdir(".") == []


def test_rank_0_works_alone(config, monkeypatch):
    before = tree(config)
    calls = []

    def forbidden(*args, **kwargs):
        raise AssertionError("another rank than 0 touched a file or the device")

    with monkeypatch.context() as patch:
        patch.setattr(parallel, "rank", lambda: 1)
        patch.setattr(zarr_io, "open", forbidden)
        patch.setattr("cellulus_amd.train._require_hip_device", forbidden)
        assert _stage.begin("a_stage", config) is None
        assert a_stage(config, "cells", "copy", lambda s, b: calls.append((s, b)), ("objects",)) is None
        assert a_stage(None, "cells", "copy", lambda s, b: calls.append((s, b)), ("objects",)) is None   # not even the config is read
    assert calls == [] and tree(config) == before and os.listdir(".") == []


def test_more_ranks_than_one_use_the_current_device(config, monkeypatch):
    import torch

    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    stage = _stage.begin("a_stage", config)
    stage.open("r")
    assert stage.device == torch.device("cuda", 3)


def test_read_only_mode_creates_nothing(config, tmp_path):
    before = tree(config)
    a_stage(config, "cells", None, lambda s, b: (objects(s, b),), ("objects",))
    assert tree(config) == before and len(os.listdir(".")) == 2
    config.segmentation_dataset_config.container_path = str(tmp_path / "missing.zarr")
    with pytest.raises(zarr_io.ZarrError, match="does not exist"):
        a_stage(config, "cells", None, lambda s, b: (), ())
    assert not os.path.exists(tmp_path / "missing.zarr")
