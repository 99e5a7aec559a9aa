"""The texture columns above the kernel: cooccurrence() and region_table(texture=True) against the restatement
(tests/texture_ref.py: counts from shifted views of the whole map), and measure(texture=True) / the command's --texture
options end to end.

The device counts are integers and must be EQUAL to the restatement's; the columns are then texture_columns of equal counts,
so they are compared with == too (tests/test_cpu_texture.py holds texture_columns against the Fraction restatement)."""

import os

import numpy as np
import pytest
import torch

from test_gpu_contacts_stage import BOUNDARY, KEYS_2D, KEYS_3D
from test_gpu_measure_stage import _blob_map, _toml
from texture_ref import FEATURES, ref_cooccurrence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["texture_pairs"] + [f"texture_{f}" for f in FEATURES]


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: (g[f"{name}/labels"], g[f"{name}/raw"]) for name in ("2d", "2d_edge", "3d")}


G = _fixture()


def _raws(name):
    raw = G[name][1]
    return {"uint16": raw, "float32": raw.astype(np.float32) * np.float32(0.3), "two_channels": np.stack([raw, 65535 - raw])}


_WANT = {}


def want_counts(labels, channel, levels, distance, value_range=None, key=None):
    """(ids, counts int64) of the restatement over the range of the object pixels, computed once per key"""
    if key is None or key not in _WANT:
        nid = int(labels.max()) + 1
        ids = np.unique(labels[labels > 0])
        lo, hi = value_range or (float(channel[labels > 0].min()), float(channel[labels > 0].max()))
        counts = ref_cooccurrence(labels, channel, nid, ids, lo, hi, levels, distance)["counts"].astype(np.int64)
        counts.setflags(write=False)
        if key is None:
            return ids, counts
        _WANT[key] = (ids, counts)
    return _WANT[key]


def want_columns(labels, raw, levels, distance, value_range=None, key=None):
    from cellulus_amd.measure import texture_columns

    channels = raw if raw.ndim == labels.ndim + 1 else raw[None]
    cols = {}
    for k, channel in enumerate(channels):
        t = texture_columns(want_counts(labels, channel, levels, distance, value_range, key and key + (k,))[1], labels.ndim)
        cols[f"texture_pairs_c{k}"] = t.pop("pairs")
        cols.update({f"texture_{f}_c{k}": v for f, v in t.items()})
    return cols


@pytest.mark.parametrize("kind", ["uint16", "float32", "two_channels"])
@pytest.mark.parametrize("name", sorted(G))
def test_counts_and_columns_equal_restatement(name, kind, device):
    from cellulus_amd.measure import cooccurrence, region_table

    labels, raw = G[name][0], _raws(name)[kind]
    nchan = 2 if kind == "two_channels" else 1
    names = [f"{n}_c{k}" for k in range(nchan) for n in NEW]                 # all of channel 0's columns before channel 1's
    plain = region_table(labels, raw, device)
    given_raw = raw.astype(np.int32) if raw.dtype == np.uint16 else raw     # torch has no uint16 arithmetic
    for levels, distance in ((8, 1), (32, 3)):
        want = want_columns(labels, raw, levels, distance, key=(name, kind, levels, distance))
        assert list(want) == names
        for lab, r in ((labels, raw), (torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(given_raw).to(device))):
            table = region_table(lab, r, device, texture=True, texture_levels=levels, texture_distance=distance)
            assert list(table) == list(plain) + names                        # appended; every old column where it was
            for k in plain:
                assert np.array_equal(plain[k], table[k]), k
            for k in names:
                assert table[k].dtype == (np.int64 if "pairs" in k else np.float64) and table[k].shape == plain["label"].shape
                assert np.array_equal(table[k], want[k], equal_nan=True), (k, table[k][:4], want[k][:4])
        for k, channel in enumerate(raw if nchan == 2 else raw[None]):
            ids, counts = cooccurrence(labels, channel, levels, distance, device=device)
            wi, wc = want_counts(labels, channel, levels, distance, key=(name, kind, levels, distance, k))
            assert ids.dtype == np.int64 and counts.dtype == np.int64 and counts.shape == wc.shape
            assert np.array_equal(ids, wi) and np.array_equal(counts, wc)
    # defaults: 8 levels at distance 1
    assert all(np.array_equal(region_table(labels, raw, device, texture=True)[k], want_columns(labels, raw, 8, 1)[k], equal_nan=True)
               for k in names)


def test_given_range_other_flags_and_bad_arguments(device):
    from cellulus_amd.measure import cooccurrence, region_table

    labels, raw = G["2d"]
    names = [f"{n}_c0" for n in NEW]
    assert list(region_table(labels, raw, device)) == KEYS_2D
    assert list(region_table(labels, raw, device, texture=False, texture_levels=99)) == KEYS_2D       # unused, unchecked
    assert list(region_table(G["3d"][0], G["3d"][1], device, texture=True))[len(KEYS_3D) + 3:] == names
    # a range narrower than the data, for the table and for the matrices
    rng = (20000.0, 30000.0)
    table = region_table(labels, raw, device, texture=True, texture_levels=16, texture_distance=2, texture_range=rng)
    want = want_columns(labels, raw, 16, 2, rng)
    assert all(np.array_equal(table[k], want[k], equal_nan=True) for k in names)
    ids, counts = cooccurrence(labels, raw.astype(np.float64), 16, 2, rng, device)
    assert np.array_equal(counts, want_counts(labels, raw, 16, 2, rng)[1]) and np.array_equal(ids, table["label"])
    # with the other flags the texture columns come last, after the quantiles
    rest = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.5,), mad=True)
    assert list(rest)[:len(KEYS_2D) + len(BOUNDARY)] == KEYS_2D + BOUNDARY and list(rest)[-2:] == ["intensity_q0.5_c0", "intensity_mad_c0"]
    full = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.5,), mad=True, texture=True)
    assert list(full) == list(rest) + names
    want = want_columns(labels, raw, 8, 1)
    assert all(np.array_equal(full[k], rest[k]) for k in rest) and all(np.array_equal(full[k], want[k], equal_nan=True) for k in names)
    with pytest.raises(ValueError, match="^region_table: texture needs raw"):
        region_table(labels, None, device, texture=True)
    for kw in (dict(texture_levels=1), dict(texture_levels=33), dict(texture_distance=0), dict(texture_distance=65),
               dict(texture_range=(2.0, 1.0)), dict(texture_range=(0.0, float("nan")))):
        with pytest.raises(ValueError, match="^region_table: texture"):
            region_table(labels, raw, device, texture=True, **kw)
    with pytest.raises(ValueError, match="^cooccurrence: texture levels"):
        cooccurrence(labels, raw, 64, device=device)
    with pytest.raises(ValueError, match="^cooccurrence: raw has shape"):
        cooccurrence(labels, np.stack([raw, raw]), device=device)
    bad = raw.astype(np.float32)
    bad[tuple(np.argwhere(labels > 0)[0])] = np.nan
    with pytest.raises(ValueError, match="non-finite values inside objects"):
        region_table(labels, bad, device, texture=True)
    with pytest.raises(ValueError, match="non-finite values inside objects"):
        cooccurrence(labels, bad, value_range=(0.0, 1.0), device=device)       # no intensity pass: the kernel's own bit


def test_chunks_do_not_change_the_table(monkeypatch, device):
    from cellulus_amd import measure

    for name in ("2d", "3d"):
        labels, raw = G[name][0], _raws(name)["two_channels"]
        whole = measure.region_table(labels, raw, device, texture=True, texture_levels=32)
        ids, counts = measure.cooccurrence(labels, raw[1], 32, device=device)
        calls = []
        real = measure._clx.call
        monkeypatch.setattr(measure._clx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        monkeypatch.setattr(measure, "TEXTURE_TABLE_BYTES", 1)               # every object is its own chunk
        parts = measure.region_table(labels, raw, device, texture=True, texture_levels=32)
        assert calls.count("clx_region_cooccurrence") == 2 * len(whole["label"]) > 2
        assert list(parts) == list(whole) and all(np.array_equal(parts[k], whole[k], equal_nan=True) for k in whole)
        ids2, counts2 = measure.cooccurrence(labels, raw[1], 32, device=device)
        assert np.array_equal(ids, ids2) and np.array_equal(counts, counts2)
        monkeypatch.undo()


def test_maps_without_objects_and_single_pixels(device):
    from cellulus_amd.measure import cooccurrence, region_table

    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zeros = np.zeros(shape, np.int32)
        empty = region_table(zeros, np.zeros((2,) + shape, np.float32), device, quantiles=(0.5,), texture=True, texture_levels=4)
        names = [f"{n}_c{k}" for k in range(2) for n in NEW]
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert all(empty[k].dtype == (np.int64 if "pairs" in k else np.float64) for k in names)
        ids, counts = cooccurrence(zeros, np.zeros(shape, np.float32), 4, device=device)
        assert ids.shape == (0,) and counts.shape == (0, 4 if len(shape) == 2 else 13, 4, 4) and counts.dtype == np.int64
    lab = np.array([[0, 3, 0], [1, 1, 0]], np.int32)
    raw = np.array([[9.0, 4.0, 9.0], [2.0, 5.0, 9.0]], np.float32)
    t = region_table(lab, raw, device, texture=True)
    assert t["label"].tolist() == [1, 3] and t["texture_pairs_c0"].tolist() == [1, 0]
    # object 1: values 2 and 5 over the range [2, 5] of the object pixels: levels 0 and 7; object 3 is one pixel: NaN
    assert t["texture_contrast_c0"][0] == 49.0 and t["texture_asm_c0"][0] == 0.5
    assert all(np.isnan(t[f"texture_{f}_c0"][1]) for f in FEATURES)


def test_measure_texture_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(81)
    raw = rng.integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 9, 82)
    seg[0, 1] = _blob_map((40, 50), 6, 83)
    seg[1, 1] = _blob_map((40, 50), 5, 84)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    old_header = ["sample"] + KEYS_2D
    names = [f"{n}_c0" for n in NEW]
    paths = [f"measurements_bandwidth-{b}.csv" for b in range(2)]

    def check(header_want, **flags):
        for b, path in enumerate(paths):
            header = open(path).readline().strip().split(",")
            assert header == header_want
            data = np.genfromtxt(path, delimiter=",", skip_header=1, dtype=np.float64).reshape(-1, len(header))
            row = 0
            for s in range(2):
                table = region_table(seg[s, b], raw[s], device, **flags)
                assert header == ["sample"] + list(table)
                n = len(table["label"])
                for name, column in table.items():                    # %.17g round-trips a float64, nan reads back as nan
                    assert np.array_equal(data[row:row + n, header.index(name)], column.astype(np.float64), equal_nan=True), (b, s, name)
                row += n
            assert row == len(data)
        return [open(path, "rb").read() for path in paths]

    measure(config.inference_config)
    plain = check(old_header)
    measure(config.inference_config, texture=True)
    check(old_header + names, texture=True)
    # the range is per sample: the restatement over the object pixels of sample 0 alone
    labels0 = seg[0, 0].astype(np.int32)
    want = want_columns(labels0, raw[0, 0], 8, 1)
    lines = open(paths[0]).read().splitlines()
    header = lines[0].split(",")
    rows = [line.split(",") for line in lines[1:] if line.split(",")[0] == "0"]
    for n in names:
        assert np.array_equal([float(r[header.index(n)]) for r in rows], want[n], equal_nan=True), n
    measure(config.inference_config, texture=True, texture_levels=16, texture_distance=2)
    check(old_header + names, texture=True, texture_levels=16, texture_distance=2)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--texture", "--texture-levels", "16", "--texture-distance", "2"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + names, texture=True, texture_levels=16, texture_distance=2)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--texture", "--quantiles", "0.5", "--hull"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(list(["sample"] + list(region_table(seg[0, 0], raw[0], device, hull=True, quantiles=(0.5,), texture=True))), hull=True,
          quantiles=(0.5,), texture=True)
    for bad in (["--texture-levels", "1"], ["--texture-distance", "65"]):
        assert CliRunner().invoke(measure_cli, ["experiment.toml", "--texture"] + bad).exit_code != 0
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check(old_header) == plain                                 # without the options: the same bytes as before
