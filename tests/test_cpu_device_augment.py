"""CPU tier of the device crop source (CLX_DEVICE_AUGMENT=1): the parameters of a crop are drawn from the generators
exactly as the host path draws them, the C ABI of clx_elastic_crop refuses bad arguments before any launch, and the
decisions of DeviceCropSource that need no device."""

import ctypes
import math
import random

import numpy as np
import pytest

from cellulus_amd import _build, _clx


def _dataset(tmp_path, shape, crop, elastic, dtype=np.uint8, name="d.zarr"):
    from cellulus_amd.configs import DatasetConfig
    from cellulus_amd.datasets import get_dataset
    from cellulus_amd.utils import zarr_io

    rng = np.random.default_rng(5)
    f = zarr_io.open(tmp_path / name)
    top = 1.0 if np.dtype(dtype).kind == "f" else np.iinfo(dtype).max
    f["train/raw"] = (rng.random(shape) * top).astype(dtype)
    f["train/raw"].attrs["axis_names"] = ["s", "c"] + ["z", "y", "x"][-len(crop):]
    return get_dataset(DatasetConfig(container_path=tmp_path / name, dataset_name="train/raw"), crop_size=crop,
                       elastic_deform=elastic, control_point_spacing=16, control_point_jitter=2.0, density=0.1, kappa=4.0,
                       normalization_factor=None)


@pytest.mark.parametrize("shape, crop", [((3, 2, 60, 70), (40, 48)), ((3, 1, 30, 36, 40), (20, 24, 28))])
@pytest.mark.parametrize("elastic", [True, False])
def test_elastic_params_consumes_the_host_paths_draws(tmp_path, shape, crop, elastic):
    ds = _dataset(tmp_path, shape, crop, elastic)
    nd = len(crop)
    for seed in (0, 1, 2):
        random.seed(seed)
        np.random.seed(seed)
        ds._random_crop()
        want = (random.getstate(), np.random.get_state())
        random.seed(seed)
        np.random.seed(seed)
        q = ds.elastic_params(shape)
        got = (random.getstate(), np.random.get_state())
        assert got[0] == want[0]
        assert got[1][0] == want[1][0] and np.array_equal(got[1][1], want[1][1]) and got[1][2:] == want[1][2:]
        # the values themselves: the host path's draws, taken by hand in its order
        random.seed(seed)
        np.random.seed(seed)
        assert q["s"] == random.randint(0, shape[0] - 1)
        if not elastic:
            assert q["offsets"] == [random.randint(0, n - c) for n, c in zip(shape[2:], crop)]
            assert set(q) == {"s", "offsets"}
            continue
        assert q["angle"] == random.uniform(0, math.pi / 2)
        assert q["scale"] == random.uniform(0.9, 1.1)
        cp_shape = ds._elastic_ops()[1]
        assert len(q["grids"]) == nd
        for g in q["grids"]:
            assert np.array_equal(g, np.random.normal(0.0, 2.0, size=cp_shape))
        assert q["u"] == [random.random() for _ in range(nd)]
        # ... and the record clx_elastic_crop reads
        rec = ds.pack_params([q])
        rot = np.eye(nd)
        rot[-2:, -2:] = [[math.cos(q["angle"]), -math.sin(q["angle"])], [math.sin(q["angle"]), math.cos(q["angle"])]]
        assert rec.shape == (1, 1 + nd * nd + nd + nd * int(np.prod(cp_shape))) and rec.dtype == np.float64
        assert rec[0, 0] == q["s"] and np.array_equal(rec[0, 1:1 + nd * nd], (rot * q["scale"]).ravel())
        assert np.array_equal(rec[0, 1 + nd * nd:1 + nd * nd + nd], q["u"])
        assert np.array_equal(rec[0, 1 + nd * nd + nd:], np.concatenate([g.ravel() for g in q["grids"]]))


def test_elastic_params_private_generators_leave_the_global_ones_alone(tmp_path):
    ds = _dataset(tmp_path, (3, 1, 60, 70), (40, 48), True)
    random.seed(3)
    np.random.seed(3)
    before = (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2])
    a = ds.elastic_params((3, 1, 60, 70), random.Random(9), np.random.RandomState(9))
    b = ds.elastic_params((3, 1, 60, 70), random.Random(9), np.random.RandomState(9))
    assert random.getstate() == before[0]
    assert np.array_equal(np.random.get_state()[1], before[1]) and np.random.get_state()[2] == before[2]
    assert a["angle"] == b["angle"] and a["u"] == b["u"] and all(np.array_equal(x, y) for x, y in zip(a["grids"], b["grids"]))


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _clx.load()


def test_elastic_crop_is_exported_and_declared(lib):
    raw = ctypes.CDLL(_clx.LIB_PATH)
    assert hasattr(raw, "clx_elastic_crop") and hasattr(raw, "clx_elastic_crop_workspace")
    assert "clx_elastic_crop" in _clx.PROTOTYPES and "clx_elastic_crop_workspace" in _clx.PROTOTYPES
    assert lib.clx_abi_version() == 13
    crop = (ctypes.c_int * 2)(256, 256)
    # one (lo, hi) pair of doubles per axis, block of the extent pass and crop
    need = lib.clx_elastic_crop_workspace(2, crop, 8)
    assert need > 0 and need % (8 * 2 * 2 * 8) == 0
    assert lib.clx_elastic_crop_workspace(4, crop, 8) == 0


P = ctypes.c_void_p(4096)          # aligned, never dereferenced: every call below is refused before a launch
NULL = ctypes.c_void_p(0)
INTS = (ctypes.c_int * 3)(64, 64, 64)
CP = (ctypes.c_int * 3)(2, 2, 2)
NOINTS = ctypes.POINTER(ctypes.c_int)()
# data, dtype, S, C, nd, spatial, crop, cp_shape, factor, elastic, B, params, mats, workspace, raw, maxima, stream
GOOD = [P, 0, 2, 1, 3, INTS, INTS, CP, 1.0, 1, 4, P, P, P, P, P, NULL]


@pytest.mark.parametrize("change, message", [
    ({0: NULL}, "null pointer"),
    ({5: NOINTS}, "null pointer"),
    ({6: NOINTS}, "null pointer"),
    ({11: NULL}, "null pointer"),
    ({14: NULL}, "null pointer"),
    ({15: NULL}, "null pointer"),
    ({7: NOINTS}, "null pointer"),                # the elastic crop needs the control-point extents ...
    ({12: NULL}, "null pointer"),                 # ... the up-sampling matrices ...
    ({13: NULL}, "null pointer"),                 # ... and the workspace
    ({4: 4}, "2 or 3 spatial dimensions"),
    ({4: 1}, "2 or 3 spatial dimensions"),
    ({1: 3}, "element type 3"),
    ({1: -1}, "element type -1"),
    ({10: 0}, "1 <= B"),
    ({10: -2}, "1 <= B"),
    ({2: 0}, "S >= 1"),
    ({3: 0}, "C >= 1"),
    ({6: (ctypes.c_int * 3)(64, 0, 64)}, "extents must be in"),
    ({7: (ctypes.c_int * 3)(2, 0, 2)}, "control-point extents"),
    ({7: (ctypes.c_int * 3)(40, 40, 40)}, "bytes of LDS"),
    ({9: 0, 6: (ctypes.c_int * 3)(64, 65, 64)}, "plain crop must fit"),
    ({14: ctypes.c_void_p(4100)}, "aligned"),
    ({11: ctypes.c_void_p(4100)}, "aligned"),
])
def test_elastic_crop_refuses_bad_arguments(lib, change, message):
    args = list(GOOD)
    for i, v in change.items():
        args[i] = v
    assert lib.clx_elastic_crop(*args) == -1
    assert message in lib.clx_last_error().decode()
    with pytest.raises(_clx.ClxError, match="clx_elastic_crop"):
        _clx.call("clx_elastic_crop", *args)


def test_device_crop_source_decisions_without_a_device(tmp_path, monkeypatch):
    from cellulus_amd.datasets.zarr_dataset import DeviceCropSource

    ds = _dataset(tmp_path, (4, 1, 512, 512), (64, 64), True, dtype=np.uint16)        # 2 MB as stored
    ok, why = DeviceCropSource.decide(ds, budget_mb=8)
    assert ok and "2.0 MB" in why and "uint16" in why
    ok, why = DeviceCropSource.decide(ds, budget_mb=1)
    assert not ok and "over the budget of 1 MB" in why and "CLX_DEVICE_AUGMENT_MB" in why
    monkeypatch.setenv("CLX_DEVICE_AUGMENT_MB", "1.5")
    assert not DeviceCropSource.decide(ds)[0]
    monkeypatch.delenv("CLX_DEVICE_AUGMENT_MB")
    assert DeviceCropSource.decide(ds)[0]                                             # default budget: 8192 MB
    # float64 is uploaded as the float32 the host path makes of it: 4 bytes per element
    ds64 = _dataset(tmp_path, (2, 1, 256, 256), (64, 64), True, dtype=np.float64, name="e.zarr")
    ok, why = DeviceCropSource.decide(ds64, budget_mb=0.75)
    assert ok and "0.5 MB" in why
    # a crop larger than the data set: the host path raises there, so the host loader is kept and nothing raises here
    big = _dataset(tmp_path, (2, 1, 48, 80), (64, 64), True, name="f.zarr")
    ok, why = DeviceCropSource.decide(big)
    assert not ok and "exceeds" in why
    with pytest.raises(RuntimeError, match="exceeds"):
        big._random_crop()


def test_loader_policy_with_and_without_the_switch(monkeypatch):
    from cellulus_amd.train import loader_policy

    monkeypatch.delenv("CLX_DEVICE_AUGMENT", raising=False)
    monkeypatch.delenv("CLX_DEVICE_PAIRS", raising=False)
    base = loader_policy(1, 8)
    assert base["loader_procs"] == 8 and not base["device_pairs"] and "device_augment" not in base
    monkeypatch.setenv("CLX_DEVICE_AUGMENT", "0")
    assert loader_policy(1, 8) == base
    monkeypatch.setenv("CLX_DEVICE_AUGMENT", "1")
    for world in (1, 8):
        on = loader_policy(world, 8)
        assert on["loader_procs"] == 0 and on["device_pairs"] and on["device_augment"]
        assert "num_workers 8 ignored" in on["why"]
    assert loader_policy(1, 8, device_augment=False) == base                          # train()'s fallback
