"""No GPU: augment_ref.py is right, and every case of test_gpu_augment_abi.py reaches the code it is meant for.

1. The reference against the host path it restates: ZarrDataset._elastic_crop (float32 out of scipy) under the seeds of
   test_gpu_device_augment._host_and_params, augment_ref fed with pack_params(elastic_params(...)) from the same seeds.
2. The plain crop is slicing.
3. Conditions on the inputs of every named case, from the reference alone: the launch plan (which loop, which store
   path, how much LDS), the boundary mode, the sign of room per axis, |room| > 1e-6 for random parameters (the mode
   decision is discontinuous at 0), a coordinate beyond one reflect period where the case is about that."""

import math
import random

import numpy as np
import pytest

import augment_ref as R


def _dataset(tmp_path, data, crop, elastic):
    from cellulus_amd.configs import DatasetConfig
    from cellulus_amd.datasets import get_dataset
    from cellulus_amd.utils import zarr_io

    f = zarr_io.open(tmp_path / "d.zarr")
    f["train/raw"] = data
    f["train/raw"].attrs["axis_names"] = ["s", "c"] + ["z", "y", "x"][-len(crop):]
    return get_dataset(DatasetConfig(container_path=tmp_path / "d.zarr", dataset_name="train/raw"), crop_size=crop,
                       elastic_deform=elastic, control_point_spacing=64, control_point_jitter=2.0, density=0.1, kappa=4.0,
                       normalization_factor=None)


def _host_and_params(ds, shape, seeds):
    import scipy.ndimage

    modes = []
    real = scipy.ndimage.map_coordinates

    def spy(*a, **k):
        modes.append(k["mode"])
        return real(*a, **k)

    host, params = [], []
    scipy.ndimage.map_coordinates = spy
    try:
        for seed in seeds:
            random.seed(seed)
            np.random.seed(seed)
            host.append(ds._random_crop())
            random.seed(seed)
            np.random.seed(seed)
            params.append(ds.elastic_params(shape))
    finally:
        scipy.ndimage.map_coordinates = real
    return np.stack(host), params, modes


HOST = [
    ("2d-u8-constant", (3, 2, 120, 120), (64, 64), np.uint8, "constant"),
    ("2d-u16-reflect", (3, 1, 66, 66), (64, 64), np.uint16, "reflect"),
    ("3d-f32-constant", (2, 1, 56, 70, 70), (24, 32, 32), np.float32, "constant"),
]


@pytest.mark.parametrize("name, shape, crop, dtype, mode", HOST, ids=[c[0] for c in HOST])
def test_reference_against_the_host_path(tmp_path, name, shape, crop, dtype, mode):
    data = R.random_data(shape, dtype)
    ds = _dataset(tmp_path, data, crop, True)
    seeds = list(range(6))
    host, params, modes = _host_and_params(ds, shape, seeds)
    assert set(modes) == {mode}
    _rel0, cp_shape, mats = ds._elastic_ops()
    assert tuple(cp_shape) == R.cp_shape_for(crop, 64)
    for mine, theirs in zip(R.make_mats(crop, cp_shape), mats):
        assert np.array_equal(mine, theirs)
    records = ds.pack_params(params)
    factor = R.default_factor(dtype)
    worst = 0.0
    for b, (ref, ref_mode, room, bound) in enumerate(R.ref_crops(data, factor, crop, tuple(cp_shape), mats, records, True)):
        assert ref.dtype == np.float64 and ref.shape == host[b].shape
        assert ref_mode == mode and ref_mode == modes[b * shape[1]]
        err = np.abs(host[b].astype(np.float64) - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (name, seeds[b], float((err / bound).max()))
    print(f"{name}: worst |host - ref64| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("shape, crop", [((3, 2, 30, 41), (16, 22)), ((2, 2, 10, 14, 17), (6, 8, 9))], ids=["2d", "3d"])
def test_plain_reference_is_slicing(shape, crop, dtype):
    data = R.random_data(shape, dtype, signed=True)
    rng = np.random.default_rng(3)
    factor = 0.37
    for _ in range(4):
        s = int(rng.integers(shape[0]))
        off = [int(rng.integers(0, n - c + 1)) for n, c in zip(shape[2:], crop)]
        (ref, mode, room, bound), = R.ref_crops(data, factor, crop, None, None, [R.plain_record(s, off)], False)
        want = data[(s, slice(None)) + tuple(slice(o, o + c) for o, c in zip(off, crop))].astype(np.float32) * np.float32(factor)
        assert mode == "plain" and not bound.any() and np.array_equal(room, np.subtract(shape[2:], crop))
        assert np.array_equal(ref.astype(np.float32), want) and np.array_equal(ref, want.astype(np.float64))


def test_identity_and_quarter_turn_of_the_reference():
    """What test_gpu_augment_abi.py's analytic cases rely on: A = I without jitter and crop == source is the source
    (room == 0 exactly, constant); with an even margin and u = 1/2 it is the centred window; the quarter turn is a rot90
    of the centred window — exactly, in float64."""
    rng = np.random.default_rng(0)
    for spatial, crop in [((20, 50), (20, 50)), ((26, 58), (20, 50)), ((5, 6, 52), (5, 6, 52)), ((9, 8, 56), (5, 6, 52))]:
        nd = len(crop)
        data = R.random_data((2, 2) + spatial, np.float32, signed=True)
        cp = R.cp_shape_for(crop, 32)
        mats = R.make_mats(crop, cp)
        rec = R.make_record(cp, 1, rng, A=np.eye(nd), u=0.5)
        (ref, mode, room, _), = R.ref_crops(data, 0.37, crop, cp, mats, [rec], True)
        off = [(n - c) // 2 for n, c in zip(spatial, crop)]
        assert mode == "constant" and np.array_equal(room, np.subtract(spatial, crop))
        assert np.array_equal(ref, R.normalised(data[1], 0.37)[(slice(None),) + tuple(slice(o, o + c) for o, c in zip(off, crop))])
    turn = np.array([[0.0, -1.0], [1.0, 0.0]])
    spatial, crop = (16, 10), (6, 10)
    data = R.random_data((1, 1) + spatial, np.float32)
    cp = R.cp_shape_for(crop, 32)
    (ref, mode, room, _), = R.ref_crops(data, 1.0, crop, cp, R.make_mats(crop, cp), [R.make_record(cp, 0, rng, A=turn, u=0.5)], True)
    assert mode == "constant" and np.array_equal(room, [6.0, 4.0])
    window = R.normalised(data[0, 0], 1.0)[3:13, 2:8]
    assert [k for k in range(4) if np.rot90(window, k).shape == crop and np.array_equal(np.rot90(window, k), ref[0])] == [3]


def test_plan_restates_the_entry_point():
    # hand-worked: crop (70, 150) -> 38 items per row; B = 256 leaves 2048 / 256 = 8 blocks per crop
    p = R.plan((70, 150), 1, 256, True)
    assert (p["xq"], p["items"], p["p1"], p["want"], p["cap"], p["tiles"], p["trips"]) == (38, 2660, 6, 11, 8, 8, 2)
    p = R.plan((70, 150), 2, 256, False)
    assert (p["work"], p["want"], p["tiles"], p["trips"]) == (5320, 21, 8, 3)
    assert R.plan((64, 64), 1, 2, True)["tiles"] == 4 and R.plan((256, 256), 1, 1, True)["p1"] == 32
    assert R.plan((5, 9), 1, 2050, True)["cap"] == 1 and R.plan((512, 512, 512), 1, 1, True)["p1"] == 64
    assert R.lds_bytes((256, 256), (13, 13)) == 56000
    pl = R.plan((64, 64), 1, 2, True)
    assert [R.tile_of(pl, (64, 64), (y, 0)) for y in (0, 15, 16, 32, 63)] == [0, 0, 1, 2, 3]


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_reaches_what_it_is_for(name):
    c = R.build_case(name)
    nd, e = len(c["crop"]), dict(c["expect"])
    pl = R.plan(c["crop"], c["C"], c["B"], c["elastic"])
    assert c["records"].shape[0] == c["B"] and set(c["records"][:, 0]) == set(range(c["S"])), "every sample index is used"
    if c["shift"]:
        assert c["crop"][-1] % 4 != 0, "a raw pointer off the 16-byte boundary is admitted only with W % 4 != 0"
    if c["family"] == "grid-cap":
        assert pl["want"] > pl["tiles"] or pl["cap"] == 1
    if c["elastic"]:
        assert R.lds_bytes(c["crop"], c["cp_shape"]) <= R.AUG_MAX_LDS
        assert R.lds_bytes(c["crop"], c["cp_shape"]) >= e.pop("lds_at_least", 0)
        assert tuple(c["cp_shape"]) == tuple(e.pop("cp", c["cp_shape"]))
    mode, signs, wrap = e.pop("mode", None), e.pop("room", None), e.pop("wrap", False)
    for key, value in e.items():
        assert pl[key] == value, (name, key, pl[key], value)
    if c["family"] == "grid-cap" and c["name"] == "cap-plain":
        # the channel boundary falls inside one thread's stride: some thread's consecutive trips are in different channels
        stride = pl["tiles"] * R.AUG_THREADS
        assert any(it // pl["items"] != (it + stride) // pl["items"] for it in range(pl["work"] - stride))
    if not c["elastic"]:
        return
    modes = set()
    for rec in {r[1:].tobytes(): r for r in c["records"]}.values():
        g = R.geometry(c["spatial"], c["crop"], c["cp_shape"], c["mats"], rec)
        modes.add(g["mode"])
        assert (np.abs(g["room"]) > 1e-6).all(), (name, g["room"])
        if mode:
            assert g["mode"] == mode
        if signs:
            assert "".join("+" if r > 0 else "-" for r in g["room"]) == signs, (name, g["room"])
        if wrap:
            n = np.asarray(c["spatial"], dtype=np.float64).reshape((nd,) + (1,) * nd)
            assert (g["coords"] >= 2 * n).any(), name
    print(f"{name}: plan {pl}, modes {sorted(modes)}")


def test_cases_cover_the_families():
    fam = {c["family"] for c in R.CASES}
    assert fam == {"odd-width", "control-points", "mixed-room", "reflect-wrap", "types", "lds", "grid-cap"}
    assert {c["crop"][-1] for c in R.CASES if c["family"] == "odd-width"} == {1, 3, 50, 67}
    assert math.prod(R.build_case("lds-56000")["cp_shape"]) == 169
