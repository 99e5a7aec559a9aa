"""The radial columns above the kernel: radial_distribution() and region_table(radial=True) against the restatement
(tests/radial_ref.py on the maps of tests/inscribed_ref.py), and measure(radial=True) / the command's --radial options end to
end.

The device tables are integers and must be EQUAL to the restatement's; the columns are then radial_columns of equal
integers, so they are compared with == too (tests/test_cpu_radial.py holds radial_columns against the Fraction restatement)."""

import os

import numpy as np
import pytest
import torch

from radial_ref import ref_distance_sq, ref_inscribed, ref_radial
from test_gpu_contacts_stage import KEYS_2D
from test_gpu_measure_stage import _blob_map, _toml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: (g[f"{name}/labels"], g[f"{name}/raw"]) for name in ("2d", "2d_edge", "3d")}


G = _fixture()


def _raws(name):
    raw = G[name][1]
    return {"none": None, "uint16": raw, "float32": raw.astype(np.float32) * np.float32(0.3) - np.float32(5000.0),
            "two_channels": np.stack([raw.astype(np.float64) / 7.0, 65535.0 - raw])}


_MAPS = {}


def want_tables(labels, raw, rings, width, wedges, edge):
    """(ids, count, [isum], [shift]) of the restatement; the maps are computed once per label map and edge"""
    from cellulus_amd.measure import intensity_shift

    labels = np.ascontiguousarray(labels).astype(np.int32)
    key = (labels.shape, bool(edge), labels.tobytes())
    if key not in _MAPS:
        nid = int(labels.max()) + 1
        dist = ref_distance_sq(labels, int(bool(edge)))
        _MAPS[key] = (nid, dist, ref_inscribed(labels, dist, nid)[0])
    nid, dist, ins = _MAPS[key]
    ids = np.unique(labels[labels > 0]).astype(np.int64)
    row = np.full(nid, -1, np.int32)
    row[ids] = np.arange(len(ids))
    W = 8 if wedges else 1
    channels = [] if raw is None else (raw if raw.ndim == labels.ndim + 1 else raw[None])
    count = ref_radial(labels, dist, None, nid, ins, row, len(ids), rings, width or 0, W)[0]
    isums, shifts = [], []
    for channel in channels:
        if channel.dtype.kind in "iu":
            channel, shift = channel.astype(np.int32), 0
        else:
            shift = intensity_shift(float(np.abs(channel.astype(np.float64)).max()), labels.size)
        c, s, bad = ref_radial(labels, dist, channel, nid, ins, row, len(ids), rings, width or 0, W, shift)
        assert bad == 0 and np.array_equal(c, count)
        isums.append(s)
        shifts.append(shift)
    return ids, count, isums, shifts


def want_columns(labels, raw, rings=4, width=None, wedges=False, edge=False):
    from cellulus_amd.measure import radial_columns

    ids, count, isums, shifts = want_tables(labels, raw, rings, width, wedges, edge)
    area = count.sum(axis=(1, 2))
    cols = radial_columns(area, count, nd=labels.ndim)
    for k, (isum, shift) in enumerate(zip(isums, shifts)):
        cols.update(radial_columns(area, count, isum, shift, labels.ndim, k))
    return cols


def _names(rings, nchan, wedges):
    per = ("mean", "frac", "meanfrac") + (("cv",) if wedges else ())
    return [f"radial_area_r{j}" for j in range(rings)] + [f"radial_{q}_r{j}_c{k}" for k in range(nchan) for j in range(rings) for q in per]


@pytest.mark.parametrize("kind", ["none", "uint16", "float32", "two_channels"])
@pytest.mark.parametrize("name", sorted(G))
def test_tables_and_columns_equal_restatement(name, kind, device):
    from cellulus_amd.measure import radial_distribution, region_table

    labels, raw = G[name][0], _raws(name)[kind]
    nd = labels.ndim
    nchan = 0 if raw is None else 2 if kind == "two_channels" else 1
    plain = region_table(labels, raw, device)
    given_raw = raw.astype(np.int32) if kind == "uint16" else raw               # torch has no uint16 arithmetic
    settings = [(4, None, False, False), (3, 2, False, True)] + ([(5, None, True, False), (2, 3, True, True)] if nd == 2 else [])
    for rings, width, wedges, edge in settings:
        names = _names(rings, nchan, wedges)
        want = want_columns(labels, raw, rings, width, wedges, edge)
        assert list(want) == names
        given = [(labels, raw)]
        if kind != "none":
            given.append((torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(given_raw).to(device)))
        for lab, r in given:
            table = region_table(lab, r, device, edge=edge, radial=True, radial_rings=rings, radial_width=width, radial_wedges=wedges)
            assert list(table) == list(plain) + names                           # appended; every old column where it was
            for k in plain:
                assert np.array_equal(plain[k], table[k]), k
            for k in names:
                assert table[k].dtype == (np.int64 if "area" in k else np.float64) and table[k].shape == plain["label"].shape
                assert np.array_equal(table[k], want[k], equal_nan=True), (k, table[k][:4], want[k][:4])
        ids, count, isum, shift = radial_distribution(labels, raw, rings, width, wedges, edge, device)
        wi, wc, ws, wshift = want_tables(labels, raw, rings, width, wedges, edge)
        assert ids.dtype == np.int64 and count.dtype == np.int64 and count.shape == (len(wi), rings, 8 if wedges else 1)
        assert np.array_equal(ids, wi) and np.array_equal(count, wc) and list(shift) == wshift and len(isum) == nchan
        assert all(a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(isum, ws))
    # defaults: 4 relative rings, no wedges
    want = want_columns(labels, raw)
    table = region_table(labels, raw, device, radial=True)
    assert all(np.array_equal(table[k], want[k], equal_nan=True) for k in _names(4, nchan, False))
    area = sum(table[f"radial_area_r{j}"] for j in range(4))
    assert np.array_equal(area, table["area"])
    if nchan:
        frac = sum(table[f"radial_frac_r{j}_c0"] for j in range(4))
        assert np.allclose(frac, 1.0, rtol=0, atol=16 * 2.0 ** -53 * sum(np.abs(table[f"radial_frac_r{j}_c0"]) for j in range(4)).max())


def test_inscribed_shares_the_maps_other_flags_and_bad_arguments(monkeypatch, device):
    from cellulus_amd import measure
    from cellulus_amd.measure import radial_distribution, region_table

    labels, raw = G["2d_edge"]
    names = _names(4, 1, True)
    for edge in (False, True):
        alone = region_table(labels, raw, device, edge=edge, inscribed=True)
        radial = region_table(labels, raw, device, edge=edge, radial=True, radial_wedges=True)
        calls = []
        real = measure._clx.call
        monkeypatch.setattr(measure._clx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        both = region_table(labels, raw, device, edge=edge, inscribed=True, radial=True, radial_wedges=True)
        monkeypatch.undo()
        assert calls.count("clx_label_distance_sq") == 1 and calls.count("clx_region_inscribed") == 1 and calls.count("clx_region_radial") == 1
        assert list(both) == list(alone) + names and list(radial) == KEYS_2D + names
        assert all(np.array_equal(both[k], alone[k]) for k in alone) and all(np.array_equal(both[k], radial[k], equal_nan=True) for k in names)
        want = want_columns(labels, raw, wedges=True, edge=edge)
        assert all(np.array_equal(both[k], want[k], equal_nan=True) for k in names)
    # with every other flag the radial columns come last, after the texture
    rest = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.5,), mad=True, texture=True)
    full = region_table(labels, raw, device, boundary=True, topology=True, hull=True, inscribed=True, quantiles=(0.5,), mad=True, texture=True,
                        radial=True, radial_rings=2, radial_width=3)
    assert list(full) == list(rest) + _names(2, 1, False) and all(np.array_equal(full[k], rest[k], equal_nan=True) for k in rest)
    want = want_columns(labels, raw, 2, 3)
    assert all(np.array_equal(full[k], want[k], equal_nan=True) for k in want)
    assert list(region_table(labels, raw, device, radial=False, radial_rings=99, radial_wedges=True)) == KEYS_2D      # unused, unchecked
    # argument errors, before any device work
    calls = []
    monkeypatch.setattr(measure._clx, "call", lambda name, *a: calls.append(name))
    for kw in (dict(radial_rings=0), dict(radial_rings=33), dict(radial_rings=2.5), dict(radial_width=0), dict(radial_width=32769),
               dict(radial_width=1.5)):
        with pytest.raises(ValueError, match="^region_table: radial"):
            region_table(labels, raw, device, radial=True, **kw)
    with pytest.raises(ValueError, match="^region_table: radial wedges need a 2-D map"):
        region_table(G["3d"][0], G["3d"][1], device, radial=True, radial_wedges=True)
    with pytest.raises(ValueError, match="^radial_distribution: radial rings"):
        radial_distribution(labels, raw, 40, device=device)
    with pytest.raises(ValueError, match="^radial_distribution: radial wedges"):
        radial_distribution(G["3d"][0], None, wedges=True, device=device)
    assert calls == []
    monkeypatch.undo()
    with pytest.raises(ValueError, match="^radial_distribution: raw has shape"):
        radial_distribution(labels, raw[:, :-1], device=device)
    bad = raw.astype(np.float32)
    bad[tuple(np.argwhere(labels > 0)[0])] = np.nan
    with pytest.raises(ValueError, match="non-finite values inside objects"):
        region_table(labels, bad, device, radial=True)
    with pytest.raises(ValueError, match="non-finite values inside objects"):
        radial_distribution(labels, bad, device=device)


def test_chunks_do_not_change_the_tables(monkeypatch, device):
    from cellulus_amd import measure

    labels = _blob_map((60, 80), 20, 7).astype(np.int32)
    objects = len(np.unique(labels[labels > 0]))
    assert objects >= 15
    raw = np.stack([np.random.default_rng(c).normal(100.0, 30.0, size=labels.shape).astype(np.float32) for c in range(2)])
    whole = measure.region_table(labels, raw, device, radial=True, radial_rings=3, radial_wedges=True)
    tables = measure.radial_distribution(labels, raw, 3, None, True, device=device)
    want = want_tables(labels, raw, 3, None, True, False)
    assert np.array_equal(tables[1], want[1]) and all(np.array_equal(a, b) for a, b in zip(tables[2], want[2])) and tables[3] == want[3]
    for bound, calls_want in ((1, 2 * objects), (3 * 8 * 16 * 7, 2 * -(-objects // 7))):
        calls = []
        real = measure._clx.call
        monkeypatch.setattr(measure._clx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        monkeypatch.setattr(measure, "RADIAL_TABLE_BYTES", bound)
        parts = measure.region_table(labels, raw, device, radial=True, radial_rings=3, radial_wedges=True)
        assert calls.count("clx_region_radial") == calls_want > 4
        again = measure.radial_distribution(labels, raw, 3, None, True, device=device)
        monkeypatch.undo()
        assert list(parts) == list(whole) and all(np.array_equal(parts[k], whole[k], equal_nan=True) for k in whole)
        assert np.array_equal(again[0], tables[0]) and np.array_equal(again[1], tables[1])
        assert all(np.array_equal(a, b) for a, b in zip(again[2], tables[2])) and again[3] == tables[3]


def test_maps_without_objects_and_tiny_objects(device):
    from cellulus_amd.measure import radial_distribution, region_table

    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zeros = np.zeros(shape, np.int32)
        wedges = len(shape) == 2
        empty = region_table(zeros, np.zeros((2,) + shape, np.float32), device, texture=True, radial=True, radial_rings=3, radial_wedges=wedges)
        names = _names(3, 2, wedges)
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert all(empty[k].dtype == (np.int64 if "area" in k else np.float64) for k in names)
        assert list(region_table(zeros, None, device, radial=True))[-4:] == _names(4, 0, False)
        ids, count, isum, shift = radial_distribution(zeros, np.zeros(shape, np.float32), 3, wedges=wedges, device=device)
        assert ids.shape == (0,) and count.shape == (0, 3, 8 if wedges else 1) and count.dtype == np.int64
        assert len(isum) == 1 and isum[0].shape == count.shape and shift == [0]
        assert radial_distribution(zeros, None, device=device)[2:] == ([], [])
    lab = np.array([[0, 3, 0, 0], [1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]], np.int32)
    raw = np.array([[9, 4, 9, 9], [2, 2, 2, 9], [2, 10, 2, 9], [2, 2, 2, 9]], np.float32)
    t = region_table(lab, raw, device, edge=True, radial=True, radial_rings=2)
    # object 1 is a 3 x 3 square: 8 pixels at distance 1 (d2 * 4 <= 4: the rim), the middle one at 2 (the core); object 3 is
    # one pixel at D2 = 1: the inequality 1 * 4 <= (k + 1)^2 * 1 puts it in the core, its rim is empty
    assert t["label"].tolist() == [1, 3] and t["radial_area_r0"].tolist() == [8, 0] and t["radial_area_r1"].tolist() == [1, 1]
    assert t["radial_mean_r0_c0"][0] == 2.0 and t["radial_mean_r1_c0"].tolist() == [10.0, 4.0] and np.isnan(t["radial_mean_r0_c0"][1])
    assert t["radial_frac_r1_c0"].tolist() == [10.0 / 26.0, 1.0] and t["radial_meanfrac_r1_c0"][0] == 90.0 / 26.0
    assert t["radial_frac_r0_c0"][1] == 0.0 and np.isnan(t["radial_meanfrac_r0_c0"][1])
    thin = region_table(lab, raw, device, edge=True, radial=True, radial_rings=3, radial_width=1)
    assert thin["radial_area_r2"].tolist() == [0, 0] and np.isnan(thin["radial_mean_r2_c0"]).all()       # thinner than three rings


def test_measure_radial_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(91)
    raw = rng.integers(0, 65536, size=(2, 1, 40, 50)).astype(np.uint16)
    seg = np.zeros((2, 2, 40, 50), dtype=np.uint16)
    seg[0, 0] = _blob_map((40, 50), 9, 92)
    seg[0, 1] = _blob_map((40, 50), 6, 93)
    seg[1, 1] = _blob_map((40, 50), 5, 94)                            # sample 1 has no objects at bandwidth 0
    f = zarr_io.open(container)
    f["test/raw"] = raw
    f["test/raw"].attrs["axis_names"] = ["s", "c", "y", "x"]
    f["segmentation"] = seg
    f["segmentation"].attrs["axis_names"] = ["s", "c", "y", "x"]
    open("experiment.toml", "w").write(_toml(container))
    config = ExperimentConfig(**tomli.loads(_toml(container)))
    old_header = ["sample"] + KEYS_2D
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
    measure(config.inference_config, radial=True)
    check(old_header + _names(4, 1, False), radial=True)
    want = want_columns(seg[0, 0].astype(np.int32), raw[0, 0])
    lines = open(paths[0]).read().splitlines()
    header = lines[0].split(",")
    rows = [line.split(",") for line in lines[1:] if line.split(",")[0] == "0"]
    for n in _names(4, 1, False):
        assert np.array_equal([float(r[header.index(n)]) for r in rows], want[n].astype(np.float64), equal_nan=True), n
    measure(config.inference_config, radial=True, radial_rings=3, radial_width=2, radial_wedges=True)
    check(old_header + _names(3, 1, True), radial=True, radial_rings=3, radial_width=2, radial_wedges=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--radial", "--radial-rings", "3", "--radial-width", "2", "--radial-wedges"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(old_header + _names(3, 1, True), radial=True, radial_rings=3, radial_width=2, radial_wedges=True)
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--radial", "--inscribed", "--texture", "--quantiles", "0.5"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(["sample"] + list(region_table(seg[0, 0], raw[0], device, inscribed=True, quantiles=(0.5,), texture=True, radial=True)),
          inscribed=True, quantiles=(0.5,), texture=True, radial=True)
    for bad in (["--radial-rings", "0"], ["--radial-width", "40000"]):
        assert CliRunner().invoke(measure_cli, ["experiment.toml", "--radial"] + bad).exit_code != 0
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check(old_header) == plain                                 # without the options: the same bytes as before
