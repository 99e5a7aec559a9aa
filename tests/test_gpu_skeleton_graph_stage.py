"""The branch graph above the kernels: branch_graph() and prune_spurs() against the restatement (tests/skeleton_graph_ref.py)
on arrays, tensors and the label dtypes, the capacity retry, skeleton_table(graph=True, prune=...) against the restatement and
against the census columns of skeleton_table() through the conservation identities, skeleton_components against
scipy.ndimage.label, and skeleton_stage(graph=True, prune=...) / the command end to end on a small container.  Integers must
be EQUAL; the float columns are formed by the same host code from equal integers."""

import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from skeleton_graph_ref import CYCLE, SPUR, graph, prune_q10, summary
from skeleton_ref import noise_map, skeleton
from test_cpu_relate import assert_same_tables
from test_gpu_measure_stage import _toml
from test_gpu_skeleton_stage import ref_distance

pytestmark = pytest.mark.gpu

MAPS = {"noise_2d": noise_map((70, 110), 1, block=16, labels=6), "noise_3d": noise_map((3, 40, 50), 2, block=12, labels=4)}
_WANT = {}


def want(name, limit=0, rounds=0):
    """the restatement of map ``name`` thinned, then pruned ``rounds`` times with ``limit`` -> (the map, graph() of it),
    computed once per key and left unchanged"""
    key = name, limit, rounds
    if key not in _WANT:
        skel = skeleton(MAPS[name]) if rounds == 0 else want(name, limit, rounds - 1)[1]["out"]
        _WANT[key] = skel, graph(skel, None, limit)
    return _WANT[key]


def tables_of(result, shape, radius=False):
    from cellulus_amd.skeleton import branch_columns, node_columns

    return branch_columns(result["branches"], shape, radius), node_columns(result["nodes"], shape)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_branch_graph_equals_restatement(name, device):
    from cellulus_amd.skeleton import branch_graph

    skel, ref = want(name)
    planewise = skel.ndim == 3
    for g in (skel, torch.from_numpy(skel).to(device), skel.astype(np.uint8), torch.from_numpy(skel.astype(np.int64))):
        got = branch_graph(g, planewise, device=device)
        assert list(got) == ["branches", "nodes", "branch_map"]
        assert_same_tables((got["branches"], got["nodes"]), tables_of(ref, skel.shape))
        m = got["branch_map"]
        assert type(m) is (torch.Tensor if torch.is_tensor(g) else np.ndarray) and tuple(m.shape) == skel.shape
        if torch.is_tensor(g):
            assert m.device == g.device and m.dtype == torch.int32
            m = m.cpu().numpy()
        assert m.dtype == np.int32 and np.array_equal(m, ref["branch_map"])
    assert len(got["branches"]["first"]) > 30 and np.isnan(got["branches"]["tortuosity"]).sum() < len(got["branches"]["first"])
    # with radius the distance map is the given map's, slice by slice
    labels = MAPS[name]
    wide = branch_graph(labels, planewise, radius=True, device=device)
    assert_same_tables((wide["branches"],), (tables_of(graph(labels, ref_distance(labels)), labels.shape, True)[0],))
    assert np.isfinite(wide["branches"]["radius_max"]).any()


def test_empty_maps_and_refusals(device):
    from cellulus_amd.skeleton import branch_graph, prune_spurs

    for same in (np.zeros((0, 5), np.int32), torch.zeros((3, 0, 5), dtype=torch.int64), np.zeros((4, 6), np.uint16)):
        got = branch_graph(same, planewise=same.ndim == 3, device=device)
        assert all(len(c) == 0 for table in (got["branches"], got["nodes"]) for c in table.values()) and "length" in got["branches"]
        assert tuple(got["branch_map"].shape) == tuple(same.shape) and not np.asarray(got["branch_map"].cpu() if torch.is_tensor(same) else got["branch_map"]).any()
        new = prune_spurs(same, 3.0, planewise=same.ndim == 3, device=device)
        assert type(new) is type(same) and new.dtype == same.dtype and tuple(new.shape) == tuple(same.shape)
    with pytest.raises(ValueError, match="^branch_graph: label ids must lie in"):
        branch_graph(np.full((4, 4), 2 ** 24, np.int64), device=device)
    with pytest.raises(ValueError, match="^prune_spurs: 3-D curve skeletons are not implemented"):
        prune_spurs(MAPS["noise_3d"], 2.0, device=device)


def test_capacity_retry(device, monkeypatch):
    from cellulus_amd import _clx, skeleton as module

    skel, ref = want("noise_2d")
    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append(args[7:9]) if name == "clx_skeleton_graph" else None, real(name, *args))[1])
    full = module.branch_graph(skel, device=device)
    assert calls == [(module.GRAPH_CAPACITY, module.GRAPH_CAPACITY)]
    del calls[:]
    monkeypatch.setattr(module, "GRAPH_CAPACITY", 7)
    small = module.branch_graph(skel, device=device)
    assert calls == [(7, 7), tuple(ref["info"][:2])] and ref["info"][0] > 7
    assert_same_tables((small["branches"], small["nodes"]), (full["branches"], full["nodes"]))
    assert_same_tables((small["branches"], small["nodes"]), tables_of(ref, skel.shape))
    del calls[:]
    monkeypatch.setattr(module, "GRAPH_CAPACITY", ref["info"][0])                 # the branches fit, the nodes do not
    assert ref["info"][1] > ref["info"][0]
    assert_same_tables((module.branch_graph(skel, device=device)["nodes"],), (full["nodes"],))
    assert calls == [(ref["info"][0],) * 2, tuple(ref["info"][:2])]


def twig_map():
    """a line with an arm of three links that forks into two twigs of one diagonal link: the twigs go in the first round, the arm,
    a spur from then on, in the second"""
    m = np.zeros((14, 50), np.int32)
    m[10, 5:46], m[7:10, 20], m[6, 19], m[6, 21] = 3, 3, 3, 3
    return m


def test_prune_spurs_rounds_dtypes_and_tensors(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.skeleton import prune_spurs

    labels, limit = twig_map(), prune_q10(3.3)
    first = graph(labels, None, limit)
    second = graph(first["out"], None, limit)
    one, two = first["out"], second["out"]
    assert first["info"][2:4] == [2, 2] and second["info"][2:4] == [3, 1] and graph(two, None, limit)["info"][3] == 0
    for g in (labels, torch.from_numpy(labels).to(device), labels.astype(np.uint8), labels.astype(np.int64), torch.from_numpy(labels.astype(np.int16))):
        for rounds, want_map in ((1, one), (2, two), (3, two)):
            new = prune_spurs(g, 3.3, rounds, device=device)
            assert type(new) is type(g) and new.dtype == g.dtype
            if torch.is_tensor(g):
                assert new.device == g.device
                new = new.cpu().numpy()
            assert np.array_equal(new, want_map)
    assert np.array_equal(prune_spurs(labels, 0, device=device), labels) and np.array_equal(prune_spurs(labels, 1.0, device=device), labels)
    # min_length is rounded UP to a multiple of 1 / 1024: 1.4142 < sqrt(2) becomes 1449 / 1024 > sqrt(2), 1448 / 1024 stays
    assert np.array_equal(prune_spurs(labels, 1.4142, device=device), one) and np.array_equal(prune_spurs(labels, 1448 / 1024, device=device), labels)
    for name in sorted(MAPS):
        skel = want(name)[0]
        assert np.array_equal(prune_spurs(skel, 3.3, planewise=skel.ndim == 3, device=device), want(name, limit, 1)[0])
        assert int((want(name, limit, 1)[0] != skel).sum()) == want(name, limit)[1]["info"][2] > 10
    # the rounds stop when one prunes nothing
    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append((args[6],) + args[7:9]) if name == "clx_skeleton_graph" else None, real(name, *args))[1])
    assert np.array_equal(prune_spurs(labels, 3.3, 50, device=device), two) and calls == [(limit, 0, 0)] * 3
    del calls[:]
    stack, wide = want("noise_3d")[0], prune_q10(9.5)
    assert np.array_equal(prune_spurs(stack, 9.5, 50, planewise=True, device=device), want("noise_3d", wide, 2)[0]) and calls == [(wide, 0, 0)] * 3
    assert want("noise_3d", wide, 1)[1]["info"][3] > 0 and want("noise_3d", wide, 2)[1]["info"][3] == 0
    del calls[:]
    assert np.array_equal(prune_spurs(labels, 0.0, 5, device=device), labels) and calls == []


@pytest.mark.parametrize("name", sorted(MAPS))
def test_skeleton_table_graph_and_prune(name, device):
    from cellulus_amd.skeleton import graph_columns, skeleton_table

    labels = MAPS[name]
    planewise = labels.ndim == 3
    plain = skeleton_table(labels, None, planewise, device=device)
    table = skeleton_table(labels, None, planewise, device=device, graph=True)
    assert list(table)[:len(plain)] == list(plain) and all(np.array_equal(table[c], plain[c]) for c in plain)
    skel, ref = want(name)
    extra = graph_columns(plain["label"], ref["branches"], ref["nodes"])
    assert list(table)[len(plain):] == list(extra)
    assert_same_tables(({c: table[c] for c in extra},), (extra,))
    brute = summary(ref["branches"], ref["nodes"])
    assert table["skeleton_longest_path"].tolist() == pytest.approx([brute[int(v)]["skeleton_longest_path"] for v in plain["label"]], rel=1e-12, abs=0)
    # the conservation identities against the census columns of the plain table
    b, v = ref["branches"], ref["nodes"]
    for row, label in enumerate(plain["label"]):
        bl, vl = b[b[:, 1] == label], v[v[:, 1] == label]
        assert bl[:, 3].sum() + vl[:, 3].sum() == plain["skeleton_pixels"][row]
        assert (vl[:, 2] == 1).sum() == plain["skeleton_end_points"][row] and (vl[:, 2] == 0).sum() == plain["skeleton_isolated"][row]
        assert vl[vl[:, 2] == 3, 3].sum() == plain["skeleton_branch_points"][row]
        assert plain["skeleton_length"][row] == pytest.approx((bl[:, 4].sum() + vl[:, 5].sum()) + np.sqrt(2.0) * (bl[:, 5].sum() + vl[:, 6].sum()), rel=1e-12)
        assert table["skeleton_branches"][row] == len(bl) and table["skeleton_spurs"][row] == (bl[:, 2] == SPUR).sum()
        assert table["skeleton_cycles"][row] == (bl[:, 2] == CYCLE).sum()
        pieces = sum(ndimage.label(s == label, np.ones((3, 3), int))[1] for s in skel.reshape((-1,) + skel.shape[-2:]))
        assert table["skeleton_components"][row] == pieces
    # pruned before it is measured: fewer ends, the same Euler number
    pruned = skeleton_table(labels, None, planewise, device=device, graph=True, prune=3.3, radius=True)
    assert list(pruned)[:len(plain)] == list(plain) and np.array_equal(pruned["label"], plain["label"]) and np.array_equal(pruned["area"], plain["area"])
    assert (pruned["skeleton_end_points"] <= plain["skeleton_end_points"]).all() and pruned["skeleton_end_points"].sum() < plain["skeleton_end_points"].sum()
    assert np.array_equal(pruned["skeleton_euler_number"], plain["skeleton_euler_number"])
    assert np.array_equal(pruned["skeleton_components"], table["skeleton_components"])
    cut = want(name, prune_q10(3.3), 1)[0]
    after = graph(cut)
    assert_same_tables(({c: pruned[c] for c in extra},), (graph_columns(plain["label"], after["branches"], after["nodes"]),))
    assert pruned["skeleton_pixels"].sum() == int((cut != 0).sum()) == plain["skeleton_pixels"].sum() - want(name, prune_q10(3.3), 0)[1]["info"][2]


def test_the_default_path_makes_the_same_calls(device, monkeypatch):
    from cellulus_amd import _clx
    from cellulus_amd.skeleton import skeleton_table, thin_labels

    calls = []
    real = _clx.call
    monkeypatch.setattr(_clx, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    labels = MAPS["noise_2d"]
    skeleton_table(labels, device=device)
    default = list(calls)
    assert default == ["clx_label_thin", "clx_region_moments", "clx_skeleton_census"]
    del calls[:]
    skeleton_table(labels, radius=True, device=device)
    assert calls == ["clx_label_thin", "clx_region_moments", "clx_label_distance_sq", "clx_skeleton_census"]
    del calls[:]
    thin_labels(labels, device=device)
    assert calls == ["clx_label_thin"]
    del calls[:]
    skeleton_table(labels, device=device, graph=True)
    assert calls == default + ["clx_skeleton_graph"]
    del calls[:]
    skeleton_table(labels, device=device, prune=2.5)
    assert calls == ["clx_label_thin", "clx_skeleton_graph", "clx_region_moments", "clx_skeleton_census"]


def test_skeleton_stage_graph_end_to_end_and_cli(tmp_path, monkeypatch, device):
    import tomli
    from click.testing import CliRunner

    from cellulus_amd.cli import skeleton as skeleton_cli
    from cellulus_amd.configs import ExperimentConfig
    from cellulus_amd.skeleton import branch_columns, graph_columns, skeleton_stage, skeleton_table
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

    def fmt(c, i):
        return ("%.17g" if c.dtype == np.float64 else "%d") % c[i]

    def check(name, prune, radius):
        ds = zarr_io.open(container, "r")[name]
        assert ds.shape == (2, 2, 40, 50) and ds.dtype == np.uint16
        total = 0
        for b in range(2):
            tables, branch_tables = [], []
            for s in range(2):
                labels = cells[s, b].astype(np.int32)
                skel = skeleton(labels)
                if prune is not None:
                    skel = graph(skel, None, prune_q10(prune))["out"]
                assert np.array_equal(ds[s, b], skel)
                r = graph(skel, ref_distance(labels) if radius else None)
                table = skeleton_table(labels, radius=radius, prune=prune, device=device)          # the census columns: tested above
                table.update(graph_columns(table["label"], r["branches"], r["nodes"]))
                tables.append(table)
                branch_tables.append(branch_columns(r["branches"], labels.shape, radius))
            for stem, per_sample in (("skeleton", tables), ("skeleton_branches", branch_tables)):
                lines = open(f"{stem}_bandwidth-{b}.csv").read().splitlines()
                assert lines[0].split(",") == ["sample"] + list(per_sample[0])
                want_lines = [",".join([str(s)] + [fmt(c, i) for c in t.values()]) for s, t in enumerate(per_sample) for i in range(len(next(iter(t.values()))))]
                assert lines[1:] == want_lines, (stem, b)
                total += len(want_lines)
        return total

    skeleton_stage(config.inference_config, "cells", "lines", graph=True)
    assert check("lines", None, False) > 60
    header = open("skeleton_branches_bandwidth-0.csv").readline().strip().split(",")
    assert header[:4] == ["sample", "first", "label", "kind"] and header[-3:] == ["length", "euclidean", "tortuosity"]
    skeleton_stage(config.inference_config, "cells", "lines_pruned", graph=True, prune=2.5, radius=True)
    check("lines_pruned", 2.5, True)
    assert open("skeleton_branches_bandwidth-1.csv").readline().strip().split(",")[-3:] == ["radius_min", "radius_max", "dist_sq_mean"]
    with pytest.raises(ValueError, match="^skeleton_stage: prune must lie in"):
        skeleton_stage(config.inference_config, "cells", "lines2", prune=-1.0)
    assert "lines2" not in zarr_io.open(container, "r")
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "lines2", "--graph", "--prune", "2.5", "--radius"])
    assert res.exit_code == 0, res.output + str(res.exception)
    check("lines2", 2.5, True)
    # the default command writes what it wrote before: one file per bandwidth, and the same bytes as the graph-less call
    for n in os.listdir(tmp_path):
        if n.endswith(".csv"):
            os.remove(n)
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "lines3"])
    assert res.exit_code == 0, res.output + str(res.exception)
    assert sorted(n for n in os.listdir(tmp_path) if n.endswith(".csv")) == ["skeleton_bandwidth-0.csv", "skeleton_bandwidth-1.csv"]
    by_command = {n: open(n).read() for n in os.listdir(tmp_path) if n.endswith(".csv")}
    skeleton_stage(config.inference_config, "cells", "lines4")
    assert {n: open(n).read() for n in os.listdir(tmp_path) if n.endswith(".csv")} == by_command
    assert np.array_equal(zarr_io.open(container, "r")["lines3"][:], zarr_io.open(container, "r")["lines"][:])
    res = CliRunner().invoke(skeleton_cli, ["experiment.toml", "--source", "cells", "--output", "lines5", "--prune", "-1"])
    assert res.exit_code == 2 and "lines5" not in zarr_io.open(container, "r")
