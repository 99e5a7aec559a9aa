"""The fill stage above the kernel: fill_holes(), hole_table() and fill_table() against the restatement (tests/fill_ref.py) on
arrays and tensors and the label dtypes, the transposed map, the Euler number of region_table(topology=True) against the
census, the inscribed columns of a repaired disc, the chain into split_labels(), and fill_stage() / the command end to end on
a small container.  Everything is integers and must be EQUAL."""

import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from fill_ref import discs_map, random_map, ref_fill_table, ref_hole_table, ref_holes
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _toml

pytestmark = pytest.mark.gpu

MAPS = {"random_2d": random_map((37, 70), 1), "random_3d": random_map((5, 19, 23), 2, block=3), "discs": discs_map((48, 56), 4),
        "balls": discs_map((9, 40, 44), 5)}
_WANT = {}


def want(name, max_size=None, planewise=False):
    """the restatement's map and tables, computed once per key and left unchanged"""
    key = name, max_size, planewise
    if key not in _WANT:
        _WANT[key] = (ref_holes(MAPS[name], max_size, planewise)[0], ref_hole_table(MAPS[name], max_size, planewise),
                      ref_fill_table(MAPS[name], max_size, planewise))
    return _WANT[key]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_entry_points_equal_restatement(name, device):
    from cellulus_amd.fill import fill_holes, fill_table, hole_table

    labels = MAPS[name]
    for max_size, planewise in ((None, False), (2, False), (0, False)) + (((None, True), (1, True)) if labels.ndim == 3 else ()):
        want_map, want_holes, want_table = want(name, max_size, planewise)
        for g in (labels, torch.from_numpy(labels).to(device)):
            new = fill_holes(g, max_size, planewise, device=device)
            assert type(new) is type(g) and new.dtype == g.dtype and tuple(new.shape) == labels.shape
            assert np.array_equal(new.cpu().numpy() if torch.is_tensor(new) else new, want_map)
        assert_same_tables((hole_table(labels, max_size, planewise, device=device), fill_table(labels, max_size, planewise, device=device)),
                           (want_holes, want_table))
    assert len(want(name)[1]["owner"]) > 3 and np.array_equal(fill_holes(labels, device=device), want(name)[0])       # the defaults


def test_label_dtypes_and_tensors(device):
    from cellulus_amd.fill import fill_holes

    labels = MAPS["random_2d"]
    want_map = want("random_2d")[0]
    given = [labels.astype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int64, np.uint64)]
    given += [torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(labels.astype(np.int16)), torch.from_numpy(labels.astype(np.uint8))]
    for g in given:
        new = fill_holes(g, device=device)
        assert type(new) is type(g) and new.dtype == g.dtype
        if torch.is_tensor(g):
            assert new.device == g.device
            new = new.cpu().numpy()
        assert np.array_equal(new, want_map)


def test_second_call_with_the_exact_capacity(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.fill import hole_table

    labels = np.ones((70, 70), np.int32)
    labels[1:69:2, 1:69:2] = 0                                           # 34 x 34 = 1156 pinholes: more than the first list of 1024 holds
    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append(args[7] if name == "clx_label_holes" else None), real(name, *args))[1])
    table = hole_table(labels, device=device)
    assert [c for c in calls if c is not None] == [1024, 1156]          # the default capacity, then exactly the count
    assert_same_tables((table,), (ref_hole_table(labels),))


def test_transposed_map(device):
    from cellulus_amd.fill import fill_holes, fill_table, hole_table

    for name, axes in (("random_2d", (1, 0)), ("random_3d", (2, 1, 0)), ("discs", (1, 0))):
        labels = MAPS[name]
        turned = np.ascontiguousarray(labels.transpose(axes))
        assert np.array_equal(fill_holes(turned, device=device).transpose(axes), want(name)[0])
        assert_same_tables((fill_table(turned, device=device),), (want(name)[2],))
        holes = hole_table(turned, device=device)                         # only `first` differs: it is recomputed for the turned map
        assert_same_tables((holes,), (ref_hole_table(turned),))
        assert sorted(zip(holes["owner"].tolist(), holes["area"].tolist())) == sorted(zip(want(name)[1]["owner"].tolist(), want(name)[1]["area"].tolist()))


def connected_discs(seed):
    """discs_map with every disc cut down to its largest 8-connected piece: non-touching CONNECTED objects"""
    labels = discs_map((48, 56), seed, knock=0.25)
    for i in range(1, 5):
        pieces, n = ndimage.label(labels == i, np.ones((3, 3)))
        sizes = ndimage.sum(labels == i, pieces, range(1, n + 1))
        labels[(labels == i) & (pieces != 1 + int(np.argmax(sizes)))] = 0
    return labels


def test_census_equals_one_minus_euler_number(device):
    """an exact kernel of the measure stage against the new one: a connected object has 1 - euler_number holes"""
    from cellulus_amd.fill import fill_table
    from cellulus_amd.measure import region_table

    total = 0
    for seed in (1, 2):
        labels = connected_discs(seed)
        euler = region_table(labels, topology=True, device=device)
        for max_size in (None, 1):
            table = fill_table(labels, max_size, device=device)
            assert np.array_equal(table["label"], euler["label"])
            assert np.array_equal(table["holes_filled"] + table["holes_kept"], 1 - euler["euler_number"])
        total += int(table["holes_kept"].sum())
        assert (table["holes_filled"] > 5).all()
    assert total > 0


def test_inscribed_columns_of_a_repaired_disc(device):
    from cellulus_amd.fill import fill_holes
    from cellulus_amd.measure import region_table

    yy, xx = np.indices((41, 45))
    solid = np.where((yy - 20) ** 2 + (xx - 22) ** 2 <= 15 ** 2, 3, 0).astype(np.int32)
    holed = solid.copy()
    holed[20, 22], holed[14, 25], holed[25:27, 15:17] = 0, 0, 0          # pinholes at and near the centre
    assert np.array_equal(fill_holes(holed, device=device), solid)
    columns = ("inscribed_radius", "inscribed_centre_y", "inscribed_centre_x", "distance_sq_mean")
    broken, whole, mended = (region_table(m, inscribed=True, device=device) for m in (holed, solid, fill_holes(holed, device=device)))
    assert all(np.array_equal(mended[c], whole[c]) for c in columns) and whole["inscribed_radius"][0] >= 15
    assert broken["inscribed_radius"][0] < whole["inscribed_radius"][0]


def test_fill_then_split(device):
    from cellulus_amd.fill import fill_holes
    from cellulus_amd.split import split_labels

    yy, xx = np.indices((40, 70))
    clump = (((yy - 20) ** 2 + (xx - 22) ** 2 <= 14 ** 2) | ((yy - 20) ** 2 + (xx - 46) ** 2 <= 14 ** 2)).astype(np.int32)
    holed = clump.copy()
    holed[20, 22], holed[18, 48] = 0, 0
    assert np.array_equal(fill_holes(holed, device=device), clump)
    pieces = split_labels(fill_holes(holed, device=device), 1, device=device)
    assert np.array_equal(pieces, split_labels(clump, 1, device=device)) and pieces.max() >= 2 and np.array_equal(pieces > 0, clump > 0)


def test_maps_that_make_no_library_call(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.fill import fill_holes, fill_table, hole_table

    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    for same in (np.full((6, 7), 4, np.int32), np.zeros((0, 5), np.int32), torch.full((3, 4, 5), 2, dtype=torch.int64)):
        new = fill_holes(same, device=device)
        assert type(new) is type(same) and new.dtype == same.dtype and tuple(new.shape) == tuple(same.shape)
        assert np.array_equal(np.asarray(new), np.asarray(same)) and len(hole_table(same, device=device)["owner"]) == 0
        assert fill_table(same, device=device)["holes_filled"].tolist() == [0] * min(1, int(np.prod(same.shape)))
    assert "clx_label_holes" not in calls
    zeros = np.zeros((6, 7), np.int32)                                   # background only: the census finds one component and no hole
    assert not fill_holes(zeros, device=device).any() and len(fill_table(zeros, device=device)["label"]) == 0
    with pytest.raises(ValueError, match="^fill_holes: label ids must lie in"):
        fill_holes(np.full((4, 4), 2 ** 24, np.int64), device=device)


def test_fill_stage_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import fill as fill_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.fill import fill_stage
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    raw = np.random.default_rng(91).integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    cells = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    cells[0, 0], cells[0, 1] = random_map((40, 50), 21), discs_map((40, 50), 22)
    cells[1, 1] = random_map((40, 50), 23, block=6, knock=0.1)            # sample 1: nothing at bandwidth 0
    f = zarr_io.open(container)
    for name, data in (("test/raw", raw), ("cells", cells)):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))

    def check(name, max_size):
        ds = zarr_io.open(container, "r")[name]
        assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16
        assert ds.attrs["axis_names"] == ["s", "c", "y", "x"] and list(ds.attrs["resolution"]) == [1, 1] and list(ds.attrs["offset"]) == [0, 0]
        for b in range(2):
            for stem, ref, header_want in (("fill", ref_fill_table, ["sample", "label", "area_before", "area", "holes_filled", "filled_area",
                                                                    "largest_hole", "holes_kept"]),
                                           ("holes", ref_hole_table, ["sample", "owner", "first_y", "first_x", "area", "filled"])):
                lines = open(f"{stem}_bandwidth-{b}.csv").read().splitlines()
                header, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
                assert header == header_want
                row = 0
                for s in range(2):
                    labels = cells[s, b].astype(np.int32)
                    assert np.array_equal(ds[s, b], ref_holes(labels, max_size)[0])
                    table = ref(labels, max_size)
                    for i in range(len(table[header_want[1]])):
                        assert rows[row] == [str(s)] + ["%d" % c[i] for c in table.values()], (stem, b, s, i)
                        row += 1
                assert row == len(rows)
        return len(open("holes_bandwidth-1.csv").readlines())

    fill_stage(config.inference_config, "cells", "solid")
    assert check("solid", None) > 20
    with pytest.raises(ValueError, match="^fill_stage: a dataset 'solid' exists"):
        fill_stage(config.inference_config, "cells", "solid", max_size=2)
    with pytest.raises(ValueError, match="^fill_stage: no dataset 'cell'"):
        fill_stage(config.inference_config, "cell", "solid2")
    with pytest.raises(ValueError, match="^fill_stage: output must name a new dataset"):
        fill_stage(config.inference_config, "cells", "cells")
    with pytest.raises(ValueError, match="^fill_stage: planewise needs a 3-D map"):
        fill_stage(config.inference_config, "cells", "solid2", planewise=True)
    check("solid", None)                                                 # the refusals changed nothing
    assert "solid2" not in zarr_io.open(container, "r")
    res = CliRunner().invoke(fill_cli, ["experiment.toml", "--source", "cells", "--output", "solid2", "--max-size", "1"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("solid2", 1)
    res = CliRunner().invoke(fill_cli, ["experiment.toml", "--source", "cells", "--output", "solid3"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("solid3", None)
    res = CliRunner().invoke(fill_cli, ["experiment.toml", "--source", "cells", "--output", "cells"])
    assert res.exit_code == 1 and isinstance(res.exception, ValueError) and "output must name" in str(res.exception)
    res = CliRunner().invoke(fill_cli, ["experiment.toml", "--source", "cells", "--output", "solid4", "--planewise"])
    assert res.exit_code == 1 and "planewise needs a 3-D map" in str(res.exception)
    assert os.path.exists("fill_bandwidth-0.csv")
