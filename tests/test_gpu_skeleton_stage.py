"""The skeleton stage above the kernels: thin_labels() and skeleton_table() against the restatement (tests/skeleton_ref.py) on
arrays, tensors and the label dtypes, max_iter, the Euler number of region_table(topology=True) of the input and of the skeleton
against the census, the radius columns against region_table(inscribed=True), the chain from fill_holes(), and skeleton_stage() /
the command end to end on a small container.  Integers must be EQUAL; the float columns are formed by the same host code from
equal integers."""

import os

import numpy as np
import pytest
import torch

from skeleton_ref import census, disc, noise_map, skeleton, thin
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _toml

pytestmark = pytest.mark.gpu

MAPS = {"noise_2d": noise_map((70, 110), 1, block=16, labels=6), "noise_3d": noise_map((3, 40, 50), 2, block=12, labels=4),
        "wide": noise_map((100, 420), 3, block=30, sigma=3.0, labels=3)}
_WANT = {}


def ref_distance(labels):
    """label_distance_sq with the default edge convention, slice by slice: inside object i it is
    scipy.ndimage.distance_transform_edt(labels == i) ** 2, an integer"""
    from scipy import ndimage

    lab = labels.reshape((-1,) + labels.shape[-2:])
    out = np.zeros(lab.shape, np.int64)
    for z, s in enumerate(lab):
        for label in np.unique(s[s != 0]):
            mask = s == label
            out[z][mask] = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)[mask]
    return out.reshape(labels.shape)


def ref_table(labels, max_iter=None, radius=False):
    from cellulus_amd.skeleton import skeleton_columns

    skel = thin(labels, max_iter)[0]
    words = census(skel, ref_distance(labels) if radius else None)[0]
    present = np.unique(labels[labels != 0]).astype(np.int64)
    area = np.bincount(labels.reshape(-1), minlength=len(words))
    return skel, skeleton_columns(present, area[present], words[present], radius)


def want(name, max_iter=None, radius=False):
    """the restatement's map and table, computed once per key and left unchanged"""
    key = name, max_iter, radius
    if key not in _WANT:
        _WANT[key] = ref_table(MAPS[name], max_iter, radius)
    return _WANT[key]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_entry_points_equal_restatement(name, device):
    from cellulus_amd.skeleton import skeleton_table, thin_labels

    labels = MAPS[name]
    planewise = labels.ndim == 3
    for max_iter in (None, 0, 1, 3):
        want_map, want_table = want(name, max_iter)
        for g in (labels, torch.from_numpy(labels).to(device)):
            new = thin_labels(g, max_iter, planewise, device=device)
            assert type(new) is type(g) and new.dtype == g.dtype and tuple(new.shape) == labels.shape
            assert np.array_equal(new.cpu().numpy() if torch.is_tensor(new) else new, want_map)
        assert_same_tables((skeleton_table(labels, max_iter, planewise, device=device),), (want_table,))
    assert np.array_equal(want(name, 0)[0], labels) and not np.array_equal(want(name, 1)[0], want(name)[0])
    assert_same_tables((skeleton_table(labels, None, planewise, radius=True, device=device),), (want(name, None, True)[1],))
    assert len(want(name)[1]["label"]) >= 3 and np.array_equal(thin_labels(labels, planewise=planewise, device=device), want(name)[0])


def test_label_dtypes_and_tensors(device):
    from cellulus_amd.skeleton import thin_labels

    labels = MAPS["noise_2d"]
    want_map = want("noise_2d")[0]
    given = [labels.astype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int64, np.uint64)]
    given += [torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(labels.astype(np.int16)), torch.from_numpy(labels.astype(np.uint8))]
    for g in given:
        new = thin_labels(g, device=device)
        assert type(new) is type(g) and new.dtype == g.dtype
        if torch.is_tensor(g):
            assert new.device == g.device
            new = new.cpu().numpy()
        assert np.array_equal(new, want_map)
    with pytest.raises(ValueError, match="^thin_labels: label ids must lie in"):
        thin_labels(np.full((4, 4), 2 ** 24, np.int64), device=device)
    with pytest.raises(ValueError, match="^thin_labels: 3-D thinning is not implemented; planewise=True thins every slice on its own$"):
        thin_labels(MAPS["noise_3d"], device=device)


def test_calls_resume_until_nothing_is_deleted(device, monkeypatch):
    from cellulus_amd import _clx, skeleton as module
    from cellulus_amd.skeleton import thin_labels

    labels = disc(40)
    want_map, deleted = thin(labels)
    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append(args[5:7]) if name == "clx_label_thin" else None, real(name, *args))[1])
    monkeypatch.setattr(module, "CALL_ITERATIONS", 16)
    assert np.array_equal(thin_labels(labels, device=device), want_map)
    assert calls == [(16, 0)] + [(16, 1)] * (-(-len(deleted) // 16) - 1) and len(calls) == 3
    del calls[:]
    assert np.array_equal(thin_labels(labels, 21, device=device), thin(labels, 21)[0]) and calls == [(16, 0), (5, 1)]
    del calls[:]
    for same in (np.zeros((0, 5), np.int32), torch.zeros((3, 0, 5), dtype=torch.int64)):
        new = thin_labels(same, planewise=same.ndim == 3, device=device)
        assert type(new) is type(same) and new.dtype == same.dtype and tuple(new.shape) == tuple(same.shape)
    assert np.array_equal(thin_labels(labels, 0, device=device), labels) and calls == []


def test_euler_number_of_input_and_skeleton(device):
    from cellulus_amd.measure import region_table
    from cellulus_amd.skeleton import skeleton_table, thin_labels

    seen = set()
    for labels in (MAPS["noise_2d"], MAPS["wide"], ring_map()):
        table = skeleton_table(labels, device=device)
        skel = thin_labels(labels, device=device)
        before, after = region_table(labels, topology=True, device=device), region_table(skel, topology=True, device=device)
        assert np.array_equal(table["label"], before["label"]) and np.array_equal(table["label"], after["label"])
        assert np.array_equal(table["skeleton_euler_number"], before["euler_number"])
        assert np.array_equal(table["skeleton_euler_number"], after["euler_number"])
        assert np.array_equal(table["area"], before["area"]) and np.array_equal(table["skeleton_pixels"], after["area"])
        seen |= set(table["skeleton_euler_number"].tolist())
    assert -1 in seen and max(seen) > 1                                    # loops, and labels of several pieces


def test_radius_against_the_inscribed_ball(device):
    from cellulus_amd.measure import region_table
    from cellulus_amd.skeleton import skeleton_table

    for name in ("noise_2d", "wide"):
        table = skeleton_table(MAPS[name], radius=True, device=device)
        ball = region_table(MAPS[name], inscribed=True, device=device)
        assert np.array_equal(table["label"], ball["label"])
        assert (table["skeleton_radius_max"] <= ball["inscribed_radius"]).all() and (table["skeleton_radius_min"] >= 1).all()
        assert (table["skeleton_radius_min"] <= table["skeleton_radius_max"]).all()
        assert (table["skeleton_dist_sq_mean"] <= table["skeleton_radius_max"] ** 2 + 1e-9).all()
    yy, xx = np.indices((45, 120))                                        # a thick bar: its centre line is its widest place
    bar = ((yy >= 15) & (yy < 30) & (xx >= 10) & (xx < 110)).astype(np.int32)
    table, ball = skeleton_table(bar, radius=True, device=device), region_table(bar, inscribed=True, device=device)
    assert table["skeleton_radius_max"][0] == ball["inscribed_radius"][0] == 8.0 and table["skeleton_end_points"][0] == 2
    whole = skeleton_table(np.ones((9, 9), np.int32), radius=True, device=device)       # no pixel of another value: infinite
    assert whole["skeleton_radius_max"][0] == np.inf and whole["skeleton_pixels"][0] == 1


def ring_map():
    """one object: a ring -- a loop that is its shape -- joined to a block with a pinhole -- a loop that is damage"""
    yy, xx = np.indices((70, 140))
    r2 = (yy - 35) ** 2 + (xx - 35) ** 2
    labels = ((r2 <= 30 ** 2) & (r2 >= 18 ** 2)).astype(np.int32)
    labels[25:45, 80:130], labels[20:50, 100:110], labels[30:40, 60:85] = 1, 1, 1
    labels[35, 105] = 0
    return labels


def test_fill_then_thin(device):
    from cellulus_amd.fill import fill_holes
    from cellulus_amd.skeleton import skeleton_table

    labels = ring_map()
    holed = skeleton_table(labels, device=device)
    mended = skeleton_table(fill_holes(labels, max_size=4, device=device), device=device)
    assert holed["skeleton_euler_number"].tolist() == [-1] and mended["skeleton_euler_number"].tolist() == [0]
    assert mended["area"][0] == holed["area"][0] + 1


def test_skeleton_stage_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import skeleton as skeleton_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.skeleton import skeleton_stage
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    raw = np.random.default_rng(91).integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    cells = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    cells[0, 0], cells[0, 1] = noise_map((40, 50), 21, block=10), noise_map((40, 50), 22, block=14, sigma=3.0)
    cells[1, 1] = noise_map((40, 50), 23, block=8)                         # sample 1: nothing at bandwidth 0
    f = zarr_io.open(container)
    for name, data in (("test/raw", raw), ("cells", cells)):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    header_want = ["sample", "label", "area", "skeleton_pixels", "skeleton_length", "skeleton_end_points", "skeleton_branch_points",
                   "skeleton_isolated", "skeleton_euler_number"]
    radius_want = ["skeleton_radius_min", "skeleton_radius_max", "skeleton_dist_sq_mean"]

    def check(name, max_iter, radius):
        ds = zarr_io.open(container, "r")[name]
        assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16
        assert ds.attrs["axis_names"] == ["s", "c", "y", "x"] and list(ds.attrs["resolution"]) == [1, 1] and list(ds.attrs["offset"]) == [0, 0]
        total = 0
        for b in range(2):
            lines = open(f"skeleton_bandwidth-{b}.csv").read().splitlines()
            header, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
            assert header == header_want + (radius_want if radius else [])
            row = 0
            for s in range(2):
                labels = cells[s, b].astype(np.int32)
                skel, table = ref_table(labels, max_iter, radius)
                assert np.array_equal(ds[s, b], skel)
                for i in range(len(table["label"])):
                    assert rows[row] == [str(s)] + [("%.17g" if c.dtype == np.float64 else "%d") % c[i] for c in table.values()], (b, s, i)
                    row += 1
            assert row == len(rows)
            total += row
        return total

    skeleton_stage(config.inference_config, "cells", "lines")
    assert check("lines", None, False) > 10
    before = {n: open(n).read() for n in os.listdir(tmp_path) if n.endswith(".csv")}
    with pytest.raises(ValueError, match="^skeleton_stage: a dataset 'lines' exists"):
        skeleton_stage(config.inference_config, "cells", "lines", max_iter=2)
    with pytest.raises(ValueError, match="^skeleton_stage: no dataset 'cell'"):
        skeleton_stage(config.inference_config, "cell", "lines2")
    with pytest.raises(ValueError, match="^skeleton_stage: output must name a new dataset"):
        skeleton_stage(config.inference_config, "cells", "cells")
    with pytest.raises(ValueError, match="^skeleton_stage: planewise needs a 3-D map"):
        skeleton_stage(config.inference_config, "cells", "lines2", planewise=True)
    with pytest.raises(TypeError, match="^skeleton_stage: max_iter must be an integer or None"):
        skeleton_stage(config.inference_config, "cells", "lines2", max_iter=1.5)
    assert {n: open(n).read() for n in os.listdir(tmp_path) if n.endswith(".csv")} == before      # the refusals changed nothing
    check("lines", None, False)
    assert "lines2" not in zarr_io.open(container, "r")
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "lines2", "--max-iter", "2", "--radius"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("lines2", 2, True)
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "lines3"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("lines3", None, False)
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "cells"])
    assert res.exit_code == 1 and isinstance(res.exception, ValueError) and "output must name" in str(res.exception)
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "lines4", "--planewise"])
    assert res.exit_code == 1 and "planewise needs a 3-D map" in str(res.exception)
    assert "lines4" not in zarr_io.open(container, "r") and os.path.exists("skeleton_bandwidth-0.csv")
