"""The std and colocalization columns above the kernel: channel_products() and region_table(std=True, colocalization=True)
against the restatement (tests/coloc_ref.py), and measure(std=True, colocalization=True) / the command's options end to end.

The device tables are integers and must be EQUAL to the restatement's; the columns are then compared with the restatement's
Fractions rounded once, with == too."""

import itertools
import os

import numpy as np
import pytest
import torch

from coloc_ref import SQUARES, SUMS, ref_columns, ref_products, ref_q, ref_thresholds, same_floats
from test_gpu_contacts_stage import KEYS_2D
from test_gpu_measure_stage import _blob_map, _toml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTITIES = ("pearson", "slope", "overlap", "k1", "k2", "manders1", "manders2")


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_regionprops.npz"))
    return {name: (g[f"{name}/labels"], g[f"{name}/raw"]) for name in ("2d", "2d_edge", "3d")}


G = _fixture()


def _case(name):
    labels, raw = G[name]
    if name == "3d":                                         # three float32 channels
        f = raw.astype(np.float32)
        noise = np.random.default_rng(3).normal(0.0, 2000.0, size=raw.shape).astype(np.float32)
        return labels, np.stack([f * np.float32(0.3) - np.float32(5000.0), np.float32(40000.0) - f / np.float32(7.0) + noise, noise])
    other = np.random.default_rng(2).integers(0, 65536, size=raw.shape).astype(np.uint16)
    return labels, np.stack([raw, (raw // 2 + other // 2).astype(np.uint16)])             # two uint16 channels


def _shift(channel, npix):
    from cellulus_amd.measure import intensity_shift

    return 0 if channel.dtype.kind in "iu" else intensity_shift(float(np.abs(channel.astype(np.float64)).max()), npix)


def want_rows(labels, raw, j, k, f):
    """(ids, rows of 14 Python ints of the present ids, shift_j, shift_k) of the restatement; f None: no thresholds"""
    labels = np.ascontiguousarray(labels).astype(np.int32)
    nid = int(labels.max()) + 1
    ids = np.unique(labels[labels > 0]).astype(np.int64)
    chan = [c.astype(np.int32) if c.dtype.kind in "iu" else c for c in (raw[j], raw[k])]
    shifts = [_shift(c, labels.size) for c in chan]
    thr = [None, None]
    if f is not None:
        for i, (c, s) in enumerate(zip(chan, shifts)):
            q, fits = ref_q(c, s, labels.size)
            assert fits.all()
            qmax = np.full(nid, -2 ** 62, dtype=np.int64)
            np.maximum.at(qmax, labels.reshape(-1), q)
            thr[i] = np.zeros(nid, dtype=np.int64)
            thr[i][ids] = ref_thresholds(qmax[ids], f)
    rows, bad = ref_products(labels, chan[0], chan[1], nid, shifts[0], shifts[1], thr[0], thr[1])
    assert bad == 0
    return ids, [rows[i] for i in ids], shifts[0], shifts[1]


def want_columns(labels, raw, std, coloc, f=0.15):
    nch = raw.shape[0]
    cols = {}
    pairs = list(itertools.combinations(range(nch), 2))
    if std:
        for c in range(nch):
            _, rows, s, _ = want_rows(labels, raw, c, c, None)
            cols[f"intensity_std_c{c}"] = np.array(ref_columns(rows, s, s, c, c)[f"intensity_std_c{c}"], dtype=np.float64)
    for j, k in pairs if coloc else []:
        _, rows, sj, sk = want_rows(labels, raw, j, k, f)
        got = ref_columns(rows, sj, sk, j, k)
        cols.update({f"coloc_{q}_c{j}_c{k}": np.array(got[f"coloc_{q}_c{j}_c{k}"], dtype=np.float64) for q in QUANTITIES})
    return cols


def _names(nch, std, coloc):
    return ([f"intensity_std_c{c}" for c in range(nch)] if std else []) + (
        [f"coloc_{q}_c{j}_c{k}" for j, k in itertools.combinations(range(nch), 2) for q in QUANTITIES] if coloc else [])


@pytest.mark.parametrize("name", ["2d", "3d"])
def test_tables_and_columns_equal_restatement(name, device):
    from cellulus_amd.measure import channel_products, region_table

    labels, raw = _case(name)
    nch = raw.shape[0]
    plain = region_table(labels, raw, device)
    assert not any(k.startswith(("intensity_std", "coloc_")) for k in plain)
    for j, k, f in [(0, 1, None), (0, 1, 0.15), (1, 0, 0.5), (nch - 1, nch - 1, None), (0, 0, 0.25)]:
        ids, table, sj, sk = channel_products(labels, raw, j, k, f, device)
        wi, rows, wj, wk = want_rows(labels, raw, j, k, f)
        assert ids.dtype == np.int64 and np.array_equal(ids, wi) and (sj, sk) == (wj, wk) and list(table) == list(SUMS + SQUARES)
        for w, key in enumerate(SUMS + SQUARES):
            assert table[key].dtype == (np.int64 if key in SUMS else object) and [int(v) for v in table[key]] == [r[w] for r in rows], key
    given = [(labels, raw)]
    if name == "3d":
        given.append((torch.from_numpy(labels.astype(np.int64)).to(device), torch.from_numpy(raw).to(device)))
    for std, coloc, f in ((True, True, 0.15), (True, False, 0.15), (False, True, 0.4), (True, True, 0.0), (True, True, 1.0)):
        names = _names(nch, std, coloc)
        want = want_columns(labels, raw, std, coloc, f)
        assert list(want) == names
        for lab, r in given:
            table = region_table(lab, r, device, std=std, colocalization=coloc, coloc_threshold=f)
            assert list(table) == list(plain) + names            # appended; every old column where it was
            assert all(np.array_equal(plain[k], table[k]) for k in plain)
            for k in names:
                assert table[k].dtype == np.float64 and table[k].shape == plain["label"].shape
                assert same_floats(table[k], want[k]), (k, table[k][:4], want[k][:4])
    # against NumPy on the pixels themselves, loosely: these are the quantities they claim to be
    table = region_table(labels, raw, device, std=True, colocalization=True)
    for row, i in enumerate(plain["label"][:5]):
        a, b = (raw[c][labels == i].astype(np.float64) for c in (0, 1))
        assert np.isclose(table["intensity_std_c0"][row], a.std(), rtol=1e-5)       # float32 channels are scaled to integers first
        if len(a) > 2 and a.std() > 0 and b.std() > 0:
            assert np.isclose(table["coloc_pearson_c0_c1"][row], np.corrcoef(a, b)[0, 1], atol=1e-5)


def test_order_among_the_other_flags_and_call_counts(monkeypatch, device):
    from cellulus_amd import measure
    from cellulus_amd.measure import region_table

    labels, raw = _case("2d")
    names = _names(2, True, True)
    want = want_columns(labels, raw, True, True)
    rest = region_table(labels, raw, device, quantiles=(0.25, 0.5), mad=True, radial=True, radial_rings=2)
    calls = []
    real = measure._clx.call
    monkeypatch.setattr(measure._clx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    full = region_table(labels, raw, device, quantiles=(0.25, 0.5), mad=True, radial=True, radial_rings=2, std=True, colocalization=True)
    monkeypatch.undo()
    assert calls.count("clx_region_products") == 1           # the pair covers both channels' std
    assert list(full) == list(rest) + names and all(np.array_equal(full[k], rest[k], equal_nan=True) for k in rest)
    assert all(same_floats(full[k], want[k]) for k in names)
    calls = []
    monkeypatch.setattr(measure._clx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    only_std = region_table(labels, raw, device, std=True)
    one = region_table(labels, raw[0], device, std=True)
    monkeypatch.undo()
    assert calls.count("clx_region_products") == 3           # a == b, one call per channel
    assert list(one) == KEYS_2D + ["intensity_std_c0"] and same_floats(one["intensity_std_c0"], want["intensity_std_c0"])
    assert all(same_floats(only_std[f"intensity_std_c{c}"], want[f"intensity_std_c{c}"]) for c in (0, 1))
    # without the flags the table keeps exactly its present keys, whatever the unused threshold says
    assert list(region_table(labels, raw[0], device)) == KEYS_2D
    assert list(region_table(labels, raw[0], device, std=False, colocalization=False, coloc_threshold=0.9)) == KEYS_2D


def test_errors_and_the_empty_map(monkeypatch, device):
    from cellulus_amd import measure
    from cellulus_amd.measure import channel_products, region_table

    labels, raw = _case("2d")
    calls = []
    monkeypatch.setattr(measure._clx, "call", lambda name, *a: calls.append(name))
    with pytest.raises(ValueError, match="^region_table: std and colocalization need raw"):
        region_table(labels, None, device, std=True)
    with pytest.raises(ValueError, match="^region_table: colocalization needs at least 2 raw channels"):
        region_table(labels, raw[0], device, colocalization=True)
    for f in (-0.5, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="^region_table: coloc_threshold"):
            region_table(labels, raw, device, colocalization=True, coloc_threshold=f)
    with pytest.raises(ValueError, match="^channel_products: channels"):
        channel_products(labels, raw, 0, 2, device=device)
    assert calls == []
    monkeypatch.undo()
    bad = raw.astype(np.float32)
    bad[1][tuple(np.argwhere(labels > 0)[0])] = np.nan
    with pytest.raises(ValueError, match="non-finite values inside objects"):
        region_table(labels, bad, device, colocalization=True)
    for shape in ((6, 7), (3, 6, 7), (0, 5)):
        zeros = np.zeros(shape, np.int32)
        empty = region_table(zeros, np.zeros((3,) + shape, np.float32), device, std=True, colocalization=True)
        names = _names(3, True, True)
        assert list(empty)[-len(names):] == names and all(len(v) == 0 for v in empty.values())
        assert all(empty[k].dtype == np.float64 for k in names)
        ids, table, sj, sk = channel_products(zeros, np.zeros((2,) + shape, np.float32), device=device)
        assert ids.shape == (0,) and (sj, sk) == (0, 0) and all(len(v) == 0 for v in table.values()) and list(table) == list(SUMS + SQUARES)
    # a tiny map by hand: object 1 has a = 1 2 3 4 and b = 2 1 4 3 (tests/test_cpu_coloc.py works it out), object 2 one pixel
    lab = np.array([[1, 1, 0], [1, 1, 2]], np.int32)
    two = np.array([[[1, 2, 9], [3, 4, 5]], [[2, 1, 9], [4, 3, 7]]], np.float32)
    t = region_table(lab, two, device, std=True, colocalization=True, coloc_threshold=0.5)       # thresholds ceil(0.5 * 4) = 2
    assert t["intensity_std_c0"].tolist() == [np.sqrt(1.25), 0.0] and t["coloc_pearson_c0_c1"][0] == 0.6 and np.isnan(t["coloc_pearson_c0_c1"][1])
    assert t["coloc_overlap_c0_c1"].tolist() == [0.96, 1.0] and t["coloc_manders1_c0_c1"].tolist() == [7 / 9, 1.0]
    assert t["coloc_k1_c0_c1"].tolist() == [0.96, 1.4] and t["coloc_k2_c0_c1"].tolist() == [0.96, 5 / 7]


def test_measure_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import measure as measure_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.measure import measure, region_table
    from cellulus_amd.utils import zarr_io

    monkeypatch.chdir(tmp_path)
    container = str(tmp_path / "data.zarr")
    rng = np.random.default_rng(91)
    raw = rng.integers(0, 65536, size=(2, 2, 40, 50)).astype(np.uint16)
    raw[:, 1] = raw[:, 0] // 3 + raw[:, 1] // 2                      # two channels that co-vary
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
    paths = [f"measurements_bandwidth-{b}.csv" for b in range(2)]

    def check(**flags):
        for b, path in enumerate(paths):
            header = open(path).readline().strip().split(",")
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
    plain = check()
    measure(config.inference_config, std=True, colocalization=True)
    check(std=True, colocalization=True)
    header = open(paths[0]).readline().strip().split(",")
    assert header[-9:] == _names(2, True, True)
    want = want_columns(seg[0, 0].astype(np.int32), raw[0], True, True)
    lines = open(paths[0]).read().splitlines()
    rows = [line.split(",") for line in lines[1:] if line.split(",")[0] == "0"]
    for n in _names(2, True, True):
        assert same_floats([float(r[header.index(n)]) for r in rows], want[n]), n
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--std", "--colocalization", "--coloc-threshold", "0.25"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(std=True, colocalization=True, coloc_threshold=0.25)
    want = want_columns(seg[0, 0].astype(np.int32), raw[0], True, True, 0.25)
    lines = open(paths[0]).read().splitlines()
    rows = [line.split(",") for line in lines[1:] if line.split(",")[0] == "0"]
    for n in _names(2, True, True):
        assert same_floats([float(r[header.index(n)]) for r in rows], want[n]), n
    res = CliRunner().invoke(measure_cli, ["experiment.toml", "--std", "--quantiles", "0.5", "--radial"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check(std=True, quantiles=(0.5,), radial=True)
    assert CliRunner().invoke(measure_cli, ["experiment.toml", "--colocalization", "--coloc-threshold", "1.5"]).exit_code != 0
    res = CliRunner().invoke(measure_cli, ["experiment.toml"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert check() == plain                                           # without the options: the same bytes as before
