"""The granularity stage above the kernels: grey_erode() / grey_dilate() / grey_open() / grey_tophat() / grey_reconstruct()
against the restatement (tests/granularity_ref.py) on arrays, tensors and the integer dtypes, steps beyond one call,
granular_spectrum() and granularity_table() on a 96 x 96 map of four objects holding blobs of two sizes, S_0 against
region_table's integrated intensity, region_table(granularity=...), and measure(granularity=...), granularity_stage() and both
commands end to end on a small container.  Integers must be EQUAL; the float columns are formed by the same host code from equal
integers."""

import os

import numpy as np
import pytest
import torch

from granularity_ref import quadrant_scene, random_levels, ref_columns, ref_morph, ref_reconstruct, ref_spectrum
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _blob_map, _toml

pytestmark = pytest.mark.gpu

SCALES = 8
_WANT = {}


def blobs():
    """the 96 x 96 scene and its grey levels, made once"""
    from cellulus_amd.propagate import image_levels

    if "scene" not in _WANT:
        labels, image = quadrant_scene(96)
        _WANT["scene"] = labels, image, image_levels(image, 256)
    return _WANT["scene"]


def want_spectrum(background=0):
    """the restatement's sums, computed once per background and left unchanged"""
    if background not in _WANT:
        labels, _, levels = blobs()
        _WANT[background] = ref_spectrum(labels, levels, SCALES, background)
    return _WANT[background]


def ref_open(image, mask, steps):
    return ref_morph(ref_morph(image, mask, 0, steps)[0], mask, 1, steps)[0]


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def test_morphology_on_arrays_tensors_and_dtypes(device):
    from cellulus_amd.granularity import grey_dilate, grey_erode, grey_open, grey_reconstruct, grey_tophat

    rng = np.random.default_rng(41)
    image = random_levels(rng, (45, 130), 200)
    mask = rng.random(image.shape) < 0.85
    marker = np.maximum(image - 40, 0)
    want = {"erode": ref_morph(image, mask, 0, 3)[0], "dilate": ref_morph(image, None, 1, 2)[0], "open": ref_open(image, mask, 2),
            "recon": ref_reconstruct(marker, image, mask)[0]}
    given = [image.astype(t) for t in (np.uint8, np.uint16, np.int16, np.int32, np.uint32, np.int64, np.uint64)]
    given += [torch.from_numpy(image.astype(np.int64)).to(device), torch.from_numpy(image.astype(np.int16)), torch.from_numpy(image.astype(np.uint8))]
    for g in given:
        masks = (mask, torch.from_numpy(mask).to(device), mask.astype(np.float32))
        for k, (name, new) in enumerate((("erode", grey_erode(g, 3, mask=masks[0], device=device)), ("dilate", grey_dilate(g, 2, device=device)),
                                         ("open", grey_open(g, 2, mask=masks[1], device=device)),
                                         ("recon", grey_reconstruct(marker, g, mask=masks[2], device=device)))):
            assert type(new) is type(g) and new.dtype == g.dtype and tuple(new.shape) == image.shape, name
            if torch.is_tensor(g):
                assert new.device == g.device
            assert np.array_equal(_host(new), want[name]), name
    hat = grey_tophat(image, 2, mask=mask, device=device)
    assert np.array_equal(hat, np.where(mask, image - want["open"], 0)) and hat.min() >= 0 and hat.max() > 0
    assert np.array_equal(grey_tophat(image, 3, device=device), image - ref_open(image, None, 3))
    volume = random_levels(rng, (6, 20, 40), 300)
    assert np.array_equal(grey_erode(volume, 2, device=device), ref_morph(volume, None, 0, 2)[0])
    assert np.array_equal(grey_reconstruct(np.maximum(volume - 50, 0), volume, device=device), ref_reconstruct(np.maximum(volume - 50, 0), volume)[0])
    for same in (np.zeros((0, 5), np.int32), torch.zeros((3, 0, 5), dtype=torch.int64)):
        for new in (grey_erode(same, device=device), grey_tophat(same, 2, device=device), grey_reconstruct(same, same, device=device)):
            assert type(new) is type(same) and new.dtype == same.dtype and tuple(new.shape) == tuple(same.shape)
    with pytest.raises(ValueError, match="^grey_erode: image must lie in \\[0, 65535\\]$"):
        grey_erode(torch.full((4, 4), 65536, dtype=torch.int64, device=device))
    with pytest.raises(ValueError, match="^grey_reconstruct: marker must lie in \\[0, 65535\\]$"):
        grey_reconstruct(torch.full((4, 4), -1, dtype=torch.int64, device=device), np.ones((4, 4), np.int32), device=device)


def test_steps_beyond_one_call_are_chained(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.granularity import grey_dilate, grey_erode, grey_open

    rng = np.random.default_rng(43)
    image = random_levels(rng, (70, 150), 60000)
    mask = rng.random(image.shape) < 0.9
    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append(args[6:8]) if name == "clx_grey_morph" else None, real(name, *args))[1])
    assert np.array_equal(grey_erode(image, 37, mask=mask, device=device), ref_morph(image, mask, 0, 37)[0])
    assert calls == [(0, 16), (0, 16), (0, 5)]
    del calls[:]
    assert np.array_equal(grey_dilate(image, 17, device=device), ref_morph(image, None, 1, 17)[0]) and calls == [(1, 16), (1, 1)]
    del calls[:]
    assert np.array_equal(grey_open(image, 20, device=device), ref_open(image, None, 20)) and calls == [(0, 16), (0, 4), (1, 16), (1, 4)]
    del calls[:]
    volume = random_levels(rng, (9, 20, 40), 60000)
    assert np.array_equal(grey_erode(volume, 6, device=device), ref_morph(volume, None, 0, 6)[0]) and calls == [(0, 4), (0, 2)]


def test_spectrum_equals_restatement_and_peaks_differ(device):
    from cellulus_amd.granularity import granular_spectrum, granularity_columns, granularity_table

    labels, image, levels = blobs()
    for background in (0, 3):
        ids, sums = want_spectrum(background)
        for given in ((labels, levels), (torch.from_numpy(labels).to(device), torch.from_numpy(levels).to(device)), (labels.astype(np.uint8), levels.astype(np.int64))):
            got_ids, got = granular_spectrum(*given, scales=SCALES, background=background, device=device)
            assert got_ids.dtype == np.int64 and got.dtype == np.int64 and got.shape == (SCALES + 1, 4)
            assert np.array_equal(got_ids, ids) and got.tolist() == sums
    ids, sums = want_spectrum()
    want = ref_columns(sums)
    table = granularity_table(labels, image, scales=SCALES, device=device)
    assert list(table) == ["label", "area"] + list(want) and table["label"].tolist() == [1, 2, 3, 4]
    assert np.array_equal(table["area"], np.bincount(labels.reshape(-1))[1:])
    assert_same_tables(({k: table[k] for k in want},), (want,))
    assert_same_tables((granularity_columns(np.array(sums)),), (want,))
    spectrum = np.stack([table[f"granularity_{i}_c0"] for i in range(1, SCALES + 1)])
    peaks = spectrum.argmax(axis=0)
    assert (spectrum >= 0).all() and peaks[0] == peaks[1] < peaks[2] == peaks[3]            # the two blob sizes peak at different scales
    total = spectrum.sum(axis=0) + table["granularity_residual_c0"]
    assert np.allclose(total, 100.0, rtol=0, atol=1e-11)
    hat = granularity_table(labels, np.stack([image, image.max() - image]), scales=3, levels=64, background=3, device=device)
    assert list(hat) == ["label", "area"] + [f"granularity_{i}_c{k}" for k in (0, 1) for i in ("1", "2", "3", "residual")]
    from cellulus_amd.propagate import image_levels

    for k, channel in enumerate((image, image.max() - image)):
        want_k = ref_columns(ref_spectrum(labels, image_levels(channel, 64), 3, 3)[1], k)
        assert_same_tables(({name: hat[name] for name in want_k},), (want_k,))
    none = granularity_table(np.zeros((20, 30), np.int32), np.zeros((20, 30)), scales=2, device=device)
    assert list(none) == ["label", "area", "granularity_1_c0", "granularity_2_c0", "granularity_residual_c0"] and all(len(c) == 0 for c in none.values())
    dark = granularity_table(labels, np.where(labels == 1, 0.0, image), scales=2, background=2, device=device)
    assert (dark["granularity_1_c0"][1:] >= 0).all()                     # object 1 is flat: S_0 may be 0 after the top-hat
    got_ids, got = granular_spectrum(labels, np.where(labels == 1, 0, levels).astype(np.int32), scales=2, device=device)
    assert got[:, 0].tolist() == [0, 0, 0]
    flat = granularity_table(labels, np.where(labels == 1, 0.0, image), scales=2, value_range=(0.0, float(image.max())), device=device)
    assert np.isnan(flat["granularity_1_c0"][0]) and np.isnan(flat["granularity_residual_c0"][0]) and not np.isnan(flat["granularity_1_c0"][1:]).any()


def test_first_sum_is_the_integrated_intensity(device):
    from cellulus_amd.granularity import granular_spectrum
    from cellulus_amd.measure import region_table

    labels, _, levels = blobs()
    ids, sums = granular_spectrum(labels, levels, scales=1, device=device)
    table = region_table(labels, levels, device=device, weighted=True)
    assert np.array_equal(table["label"], ids) and table["intensity_sum_c0"].tolist() == [float(v) for v in sums[0]]


def test_region_table_granularity_alone_and_after_the_other_columns(device):
    from cellulus_amd.granularity import granularity_table
    from cellulus_amd.measure import region_table

    labels, image, _ = blobs()
    raw = np.stack([image, np.sqrt(image)]).astype(np.float32)
    want = granularity_table(labels, raw, scales=4, levels=128, background=2, device=device)
    names = [n for n in want if n.startswith("granularity_")]
    assert len(names) == 10
    plain = region_table(labels, raw, device=device)
    alone = region_table(labels, raw, device=device, granularity=4, granularity_levels=128, granularity_background=2)
    assert list(alone) == list(plain) + names
    assert_same_tables(({n: alone[n] for n in names},), ({n: want[n] for n in names},))
    assert_same_tables(({n: alone[n] for n in plain},), (plain,))
    options = dict(boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.5,), mad=True, texture=True, radial=True, std=True,
                   colocalization=True, weighted=True, border_intensity=True)
    others = region_table(labels, raw, device=device, **options)
    every = region_table(labels, raw, device=device, granularity=4, granularity_levels=128, granularity_background=2, **options)
    assert list(every) == list(others) + names
    assert_same_tables(({n: every[n] for n in names},), ({n: want[n] for n in names},))
    assert_same_tables(({n: every[n] for n in others},), (others,))
    on_device = region_table(torch.from_numpy(labels).to(device), torch.from_numpy(raw).to(device), granularity=4, granularity_levels=128,
                             granularity_background=2)
    assert_same_tables(({n: on_device[n] for n in names},), ({n: want[n] for n in names},))


def test_stage_measure_and_commands_end_to_end(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import granularity as granularity_cli, measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.granularity import granularity_stage, granularity_table
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(51)
    raw = rng.integers(0, 65536, size=(2, 2, 40, 50)).astype(np.uint16)
    raw[:, 0, 10:14, 10:14], raw[:, 1, 20:30, 20:30] = 65535, 60000
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0], seg[0, 1] = _blob_map((40, 50), 7, 32), _blob_map((40, 50), 5, 33)
    seg[1, 1] = _blob_map((40, 50), 3, 34)                              # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    for name, data in (("test/raw", raw), ("segmentation", seg), ("cells", seg[:, ::-1].copy())):
        f[name] = data
        f[name].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    before = sorted(os.listdir(container))

    def check(stem, tables):
        """the CSV files of `stem` hold the rows of tables(sample, bandwidth) -> how many"""
        total = 0
        for b in range(2):
            lines = open(f"{stem}_bandwidth-{b}.csv").read().splitlines()
            rows, row = [line.split(",") for line in lines[1:]], 0
            for s in range(2):
                table = tables(s, b)
                assert lines[0].split(",") == ["sample"] + list(table)
                for i in range(len(table["label"])):
                    assert rows[row] == [str(s)] + [("%.17g" if c.dtype.kind == "f" else "%d") % c[i] for c in table.values()], (b, s, i)
                    row += 1
            assert row == len(rows)
            total += row
            os.remove(f"{stem}_bandwidth-{b}.csv")
        return total

    cells = seg[:, ::-1]
    granularity_stage(config.inference_config, "cells")
    assert check("granularity", lambda s, b: granularity_table(cells[s, b].astype(np.int32), raw[s], device=device)) > 8
    granularity_stage(config.inference_config, "cells", channel=1, scales=3, levels=16, background=2)
    check("granularity", lambda s, b: {k: v for k, v in granularity_table(cells[s, b].astype(np.int32), raw[s], scales=3, levels=16, background=2,
                                                                           device=device).items() if not k.endswith("_c0")})
    with pytest.raises(ValueError, match="^granularity_stage: no dataset 'cell'"):
        granularity_stage(config.inference_config, "cell")
    with pytest.raises(ValueError, match="^granularity_stage: no channel 2 in a raw dataset of 2 channels$"):
        granularity_stage(config.inference_config, "cells", channel=2)
    assert not [n for n in os.listdir(tmp_path) if n.endswith(".csv")]       # the refusals wrote nothing
    res = CliRunner().invoke(granularity_cli, ["experiment.toml", "--source", "segmentation", "--channel", "0", "--scales", "2", "--levels", "32", "--background", "1"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("granularity", lambda s, b: {k: v for k, v in granularity_table(seg[s, b].astype(np.int32), raw[s], scales=2, levels=32, background=1,
                                                                           device=device).items() if not k.endswith("_c1")})
    res = CliRunner().invoke(granularity_cli, ["experiment.toml", "--source", "cells", "--scales", "65"])
    assert res.exit_code == 2
    res = CliRunner().invoke(granularity_cli, ["experiment.toml", "--source", "nothing"])
    assert res.exit_code == 1 and isinstance(res.exception, ValueError) and "no dataset 'nothing'" in str(res.exception)
    assert sorted(os.listdir(container)) == before and "granularity" not in zarr_io.open(container, "r")          # no dataset was created

    def measured(s, b):
        return region_table(seg[s, b].astype(np.int32), raw[s], device, std=True, granularity=3, granularity_background=1, granularity_levels=64)

    measure(config.inference_config, std=True, granularity=3, granularity_background=1, granularity_levels=64)
    assert check("measurements", measured) > 8
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--std", "--granularity", "3", "--granularity-background", "1", "--granularity-levels", "64"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("measurements", measured)
    assert "granularity_residual_c1" in measured(0, 0) and "granularity_3_c0" in measured(0, 0)
