"""The propagate stage above the kernel: geodesic_owner(), propagate_labels() and propagate_table() against the restatement
(tests/propagate_ref.py) on arrays and device tensors, the seed dtypes, the transpose, the chain nuclei -> territories ->
relate(), and propagate_stage() / the command end to end on a small container.

The device maps and the integer columns must be EQUAL to the restatement's; the one float column is a correctly rounded
division of exact integers and is compared with == too."""

import os

import numpy as np
import pytest
import torch

from propagate_ref import COST_INF, dots_map, ref_propagate, ref_propagate_sweeps, ref_propagate_table
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _toml

pytestmark = pytest.mark.gpu


def blobs(shape, seed, level=0.55):
    """a seeded foreground of smooth blobs"""
    rng = np.random.default_rng(seed)
    field = rng.random(shape)
    for axis in range(len(shape)):
        for _ in range(3):
            field = (np.roll(field, 1, axis) + field + np.roll(field, -1, axis)) / 3
    return (field > np.quantile(field, level)).astype(np.uint8)


def case(shape, seed):
    """-> (seeds, mask, image as float32, its grey levels over the mask and the seeds at 16 levels)"""
    seeds = dots_map(shape, 7, seed)
    mask = blobs(shape, seed)
    image = np.random.default_rng(seed + 1).random(shape).astype(np.float32) * 3 - 1
    where = (mask != 0) | (seeds > 0)
    lo, hi = float(image[where].min()), float(image[where].max())
    level = np.minimum(15, np.floor((image.astype(np.float64) - lo) * 16 / (hi - lo)))
    return seeds, mask, image, np.clip(level, 0, 15).astype(np.int32)


CASES = {"2d": case((40, 70), 3), "3d": case((9, 12, 20), 4)}
_WANT = {}


def want(name, reg=1, limit=None, masked=True, weighted=True):
    """the restatement's maps, computed once per key and left unchanged"""
    key = (name, reg, limit, masked, weighted)
    if key not in _WANT:
        seeds, mask, _, weight = CASES[name]
        _WANT[key] = ref_propagate(seeds, mask if masked else None, weight if weighted else None, reg=reg, limit=limit)[:2]
    return _WANT[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_geodesic_owner_and_labels_equal_restatement(name, device):
    from cellulus_amd.propagate import geodesic_owner, propagate_labels

    seeds, mask, image, weight = CASES[name]
    on = lambda a: torch.from_numpy(a).to(device)                   # noqa: E731
    for reg, limit in ((1, None), (0, None), (3, 40)):
        want_owner, want_cost = want(name, reg, limit)
        for s, m, w, i in ((seeds, mask, weight, image), (on(seeds), on(mask), on(weight), on(image)), (seeds, mask != 0, weight.astype(np.uint16), image)):
            owner, cost = geodesic_owner(s, m, w, reg, limit, device=device)
            assert owner.is_cuda and cost.is_cuda and owner.dtype == cost.dtype == torch.int32 and tuple(owner.shape) == seeds.shape
            assert np.array_equal(owner.cpu().numpy(), want_owner) and np.array_equal(cost.cpu().numpy(), want_cost)
            new = propagate_labels(s, m, i, levels=16, regularisation=reg, limit=limit, device=device)
            assert type(new) is type(s) and new.dtype == s.dtype and tuple(new.shape) == seeds.shape
            assert np.array_equal(new.cpu().numpy() if torch.is_tensor(new) else new, want_owner)
    owner, cost = geodesic_owner(seeds, device=device)              # the defaults: no mask, flat, reg 1, no limit
    flat = want(name, masked=False, weighted=False)
    assert np.array_equal(owner.cpu().numpy(), flat[0]) and np.array_equal(cost.cpu().numpy(), flat[1]) and (flat[0] > 0).all()


def test_seed_dtypes_and_tensors(device):
    from cellulus_amd.propagate import propagate_labels

    seeds, mask, image, _ = CASES["2d"]
    want_owner = want("2d")[0]
    given = [seeds.astype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int64, np.uint64)]
    given += [torch.from_numpy(seeds.astype(np.int64)).to(device), torch.from_numpy(seeds.astype(np.int16)), torch.from_numpy(seeds.astype(np.uint8))]
    for g in given:
        new = propagate_labels(g, mask, image, levels=16, device=device)
        assert type(new) is type(g) and new.dtype == g.dtype
        if torch.is_tensor(g):
            assert new.device == g.device
            new = new.cpu().numpy()
        assert np.array_equal(new, want_owner)


@pytest.mark.parametrize("name", sorted(CASES))
def test_transposed_inputs_give_the_transposed_result(name, device):
    from cellulus_amd.propagate import geodesic_owner

    seeds, mask, _, weight = CASES[name]
    axes = tuple(reversed(range(seeds.ndim)))
    turn = lambda a: np.ascontiguousarray(a.transpose(axes))        # noqa: E731
    for reg in (0, 1):
        owner, cost = geodesic_owner(turn(seeds), turn(mask), turn(weight), reg, device=device)
        want_owner, want_cost = want(name, reg)
        assert np.array_equal(owner.cpu().numpy().transpose(axes), want_owner) and np.array_equal(cost.cpu().numpy().transpose(axes), want_cost)


def test_without_mask_or_image_covers_what_the_limit_allows(device):
    from cellulus_amd.propagate import propagate_labels

    seeds = dots_map((50, 90), 12, 8)
    _, cost, _ = ref_propagate_sweeps(seeds)
    for limit in (0, 9, 10, 31):
        new = propagate_labels(seeds, limit=limit, device=device)
        assert np.array_equal(new > 0, cost <= limit) and np.array_equal(new[seeds > 0], seeds[seeds > 0])
        assert np.array_equal(new, ref_propagate_sweeps(seeds, limit=limit)[0])
    assert (propagate_labels(seeds, device=device) > 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_equals_columns_of_the_restatement(name, device):
    from cellulus_amd.propagate import propagate_table

    seeds, mask, image, _ = CASES[name]
    for reg, limit in ((1, None), (3, 40)):
        table = propagate_table(seeds, mask, image, levels=16, regularisation=reg, limit=limit, device=device)
        assert_same_tables((table,), (ref_propagate_table(seeds, *want(name, reg, limit), mask),))
    assert len(table["label"]) == len(np.unique(seeds)) - 1 and table["unreached"][0] > 0 and (table["area"] >= table["seed_area"]).all()
    open_table = propagate_table(seeds, device=device)
    assert not open_table["unreached"].any() and open_table["area"].sum() == seeds.size


def test_empty_maps_make_no_call(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.propagate import geodesic_owner, propagate_labels, propagate_table

    def no_call(*args, **kwargs):
        raise AssertionError("an entry point was called")

    monkeypatch.setattr(_clx, "call", no_call)
    for zeros in (np.zeros((6, 7), np.int32), np.zeros((3, 6, 7), np.uint16), np.zeros((0, 5), np.int32), torch.zeros(4, 5, dtype=torch.int64)):
        new = propagate_labels(zeros, device=device)
        assert type(new) is type(zeros) and new.dtype == zeros.dtype and tuple(new.shape) == tuple(zeros.shape) and not new.any()
        owner, cost = geodesic_owner(zeros, device=device)
        assert tuple(owner.shape) == tuple(zeros.shape) and not owner.any() and (cost == COST_INF).all()
        table = propagate_table(zeros, device=device)
        assert len(table) == 6 + zeros.ndim and all(len(c) == 0 for c in table.values())
    monkeypatch.undo()
    with pytest.raises(ValueError, match="^propagate_labels: label ids must lie in"):
        propagate_labels(np.full((4, 4), 2 ** 24, np.int64), device=device)
    with pytest.raises(ValueError, match="^geodesic_owner: weight must lie in"):
        geodesic_owner(np.ones((4, 4), np.int32), weight=torch.full((4, 4), 65536, device=device), device=device)


def test_nuclei_territories_relate(device):
    from cellulus_amd.propagate import propagate_labels
    from cellulus_amd.relate import relate

    shape = (60, 90)
    cells = blobs(shape, 12, 0.4)
    rng = np.random.default_rng(13)
    nuclei = np.zeros(shape, np.int32)
    inside = np.argwhere(cells[:-2, :-2] > 0)
    for i, at in enumerate(inside[rng.choice(len(inside), 14, replace=False)], 1):
        nuclei[at[0]:at[0] + 2, at[1]:at[1] + 2] = i
    territory = propagate_labels(nuclei, mask=cells > 0, device=device)
    assert not territory[(cells == 0) & (nuclei == 0)].any()            # no territory pixel outside the mask but seed pixels
    assert np.array_equal(territory[nuclei > 0], nuclei[nuclei > 0]) and (territory > 0).sum() > 5 * (nuclei > 0).sum()
    child = relate(nuclei, territory, device=device)[0]
    assert np.array_equal(child["label"], child["parent"]) and (child["overlap"] == child["area"]).all()       # wholly inside its own


def test_propagate_stage_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import propagate as propagate_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.propagate import propagate_stage
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    raw = np.random.default_rng(91).integers(0, 65536, size=(2, 2, 40, 50)).astype(np.uint16)
    nuclei, fg = np.zeros((2, 2, 40, 50), dtype=np.uint16), np.zeros((2, 2, 40, 50), dtype=np.uint16)
    nuclei[0, 0], nuclei[0, 1], nuclei[1, 1] = dots_map((40, 50), 6, 21), dots_map((40, 50), 9, 22), dots_map((40, 50), 3, 23)
    fg[0, 0], fg[0, 1], fg[1, 0], fg[1, 1] = blobs((40, 50), 31) * 5, blobs((40, 50), 32), blobs((40, 50), 33), blobs((40, 50), 34).astype(np.uint16) * 300
    f = zarr_io.open(container)                                          # sample 1 has no nuclei at bandwidth 0
    for name, data in (("test/raw", raw), ("nuclei", nuclei), ("fg", fg)):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))

    def check(name, mask, channel, levels, reg, limit):
        ds = zarr_io.open(container, "r")[name]
        assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16
        assert ds.attrs["axis_names"] == ["s", "c", "y", "x"] and list(ds.attrs["resolution"]) == [1, 1] and list(ds.attrs["offset"]) == [0, 0]
        for b in range(2):
            lines = open(f"propagate_bandwidth-{b}.csv").read().splitlines()
            header, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
            assert header == ["sample", "label", "seed_area", "area", "reach_cost", "reach_y", "reach_x", "cost_mean", "unreached"]
            row = 0
            for s in range(2):
                seeds = nuclei[s, b].astype(np.int32)
                allowed = fg[s, b] != 0 if mask else None
                weight = None
                if channel is not None:
                    where = (allowed | (seeds > 0)) if mask else np.ones(seeds.shape, bool)
                    image = raw[s, channel].astype(np.float64)
                    lo, hi = image[where].min(), image[where].max()
                    weight = np.minimum(levels - 1, np.floor((image - lo) * levels / (hi - lo))).clip(0).astype(np.int32)
                owner, cost, _ = ref_propagate(seeds, allowed, weight, nid=int(seeds.max()) + 1, reg=reg, limit=limit)
                assert np.array_equal(ds[s, b], owner)
                table = ref_propagate_table(seeds, owner, cost, allowed)
                for i in range(len(table["label"])):
                    text = ["%.17g" % c[i] if c.dtype == np.float64 else "%d" % c[i] for c in table.values()]
                    assert rows[row] == [str(s)] + text, (b, s, i)
                    row += 1
            assert row == len(rows)
        return len(open("propagate_bandwidth-1.csv").readlines())

    propagate_stage(config.inference_config, "nuclei", "cells", mask="fg", channel=1, levels=32)
    assert check("cells", True, 1, 32, 1, None) == 1 + len(np.unique(nuclei[0, 1])) - 1 + len(np.unique(nuclei[1, 1])) - 1 > 8
    with pytest.raises(ValueError, match="^propagate_stage: a dataset 'cells' exists"):
        propagate_stage(config.inference_config, "nuclei", "cells")
    with pytest.raises(ValueError, match="^propagate_stage: no dataset 'nucleus'"):
        propagate_stage(config.inference_config, "nucleus", "cells2")
    with pytest.raises(ValueError, match="^propagate_stage: no dataset 'bg'"):
        propagate_stage(config.inference_config, "nuclei", "cells2", mask="bg")
    with pytest.raises(ValueError, match="^propagate_stage: no channel 2"):
        propagate_stage(config.inference_config, "nuclei", "cells2", channel=2)
    with pytest.raises(ValueError, match="^propagate_stage: output must name a new dataset"):
        propagate_stage(config.inference_config, "nuclei", "nuclei")
    check("cells", True, 1, 32, 1, None)                                # the refusals changed nothing
    assert "cells2" not in zarr_io.open(container, "r")
    res = CliRunner().invoke(propagate_cli, ["experiment.toml", "--seeds", "nuclei", "--output", "cells2", "--mask", "fg", "--channel", "0", "--levels",
                                             "8", "--regularisation", "2", "--limit", "60"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("cells2", True, 0, 8, 2, 60)
    res = CliRunner().invoke(propagate_cli, ["experiment.toml", "--seeds", "nuclei", "--output", "cells3"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("cells3", False, None, 256, 1, None)
    res = CliRunner().invoke(propagate_cli, ["experiment.toml", "--seeds", "nuclei", "--output", "nuclei"])
    assert res.exit_code == 1 and isinstance(res.exception, ValueError) and "output must name" in str(res.exception)
    assert os.path.exists("propagate_bandwidth-0.csv")
