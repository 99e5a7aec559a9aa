"""How the launch plan is put together (no device is used): the topology module stands without the library and the
switches, a plan decides before it allocates and decides the same without memory, and models/plan.py still hands out
every name it used to define."""

import importlib
import os
import sys

import pytest
import torch

import plan_trace
from cellulus_amd import _clx
from cellulus_amd.models import descriptors, dual, plan, subpixel, topology

CPU = torch.device("cpu")


def test_topology_needs_neither_the_library_nor_a_switch(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the topology module loaded libclx")

    real_get = os.environ.get

    def no_switch(key, default=None):
        assert not str(key).startswith("CLX_"), "the topology module read %s" % key
        return real_get(key, default)

    monkeypatch.setattr(_clx, "load", no_library)
    monkeypatch.setattr(os.environ, "get", no_switch)
    monkeypatch.delitem(sys.modules, "cellulus_amd.models.topology")        # (put back on exit: a fresh import below)
    fresh = importlib.import_module("cellulus_amd.models.topology")
    assert fresh is not topology and fresh.build_topology is not topology.build_topology
    assert not {"_clx", "os", "torch"} & set(vars(fresh))
    for net in ("bench_2d", "bench_3d"):
        c = plan_trace.NETWORKS[net]
        topo = fresh.build_topology(spatial=c["spatial"], **c["cfg"])
        assert topo.convs and topo.nd == c["cfg"]["num_spatial_dims"]
        flops = fresh.forward_flops(topo, c["batch"])
        assert flops > 0
        assert flops == plan.forward_flops(plan.build_topology(spatial=c["spatial"], **c["cfg"]), c["batch"])


def _decisions(p, backward):
    """what a plan has decided, as plain values"""
    d = dict(algo=p.algo, sp_pass=p.sp_pass, chains=sorted(p.chains), fused_pool=sorted(p.fused_pool), ws_bytes=p.ws_bytes,
             halves={name: [(h.wino, h.wino_dgrad, h.fused) for h in sp.halves] for name, sp in p.subpixel.items()})
    if backward:
        d.update(adjoint=sorted(p.adjoint), gate=sorted(p.gate_shape), vcache=sorted(p.vcache_bytes),
                 xplanes=sorted(p.xplanes_bytes))
    return d


@pytest.mark.parametrize("net", sorted(plan_trace.NETWORKS))
def test_deciding_allocates_nothing_and_depends_on_no_memory(net, monkeypatch):
    def no_memory(*a, **k):
        raise AssertionError("memory was allocated while the plan decided")

    for name in [k for k in os.environ if k.startswith("CLX_")]:
        monkeypatch.delenv(name)
    c = plan_trace.NETWORKS[net]
    topo = plan.build_topology(spatial=c["spatial"], **c["cfg"])
    for setting in ("default", "f32", "g64", "deterministic", "plain"):
        for keep in (False, True):
            with monkeypatch.context() as m:
                for k, v in plan_trace.ENVS[setting].items():
                    m.setenv(k, v)
                with m.context() as mm:
                    for mod, fn in ((torch, "empty"), (torch, "zeros"), (_clx, "zeros")):
                        mm.setattr(mod, fn, no_memory)
                    decided = plan.UNetPlan(topo, c["batch"], CPU, keep, allocate=False)
                    if keep:
                        decided._decide_backward()
                    assert not decided.buf and decided.workspace is None and not decided._wplanes
                    got = _decisions(decided, keep)
                m.setattr(_clx, "zeros", lambda shape, dtype, device: torch.empty(shape, dtype=dtype, device=device))
                full = plan.UNetPlan(topo, c["batch"], CPU, keep)
                if keep:
                    full._alloc_backward()
                assert got == _decisions(full, keep), (setting, keep)
                # ... and the memory the full plan took is what was decided
                if got["ws_bytes"]:
                    assert full.workspace.numel() == got["ws_bytes"] // 4 + 4
                else:
                    assert full.workspace is None
                if keep:
                    assert got["adjoint"] == sorted(full.adjoint) and got["gate"] == sorted(full.gate)
                    assert got["vcache"] == sorted(full.vcache) and got["xplanes"] == sorted(full.xplanes)
                    assert {n: tuple(g.shape) for n, g in full.gate.items()} == decided.gate_shape


OWNERS = {topology: ("pad4", "Source", "ConvLayer", "PoolOp", "Topology", "build_topology", "tensor_consumers",
                     "find_chain_pairs", "forward_flops"),
          descriptors: ("conv_src", "conv_desc", "WINO_PACK_FWD", "WINO_PACK_DGRAD", "WINO_TILE", "wino_taps", "packed_taps",
                        "pack_job_elements", "winograd_code", "winograd_enabled", "FUSED_MAX_CHANNELS", "fused_pays",
                        "fused_wanted", "DEFAULT_PRECISION",
                        "PRECISION_CODES", "precision_name", "precision_code"),
          subpixel: ("SubpixelHalf", "Subpixel"),
          dual: ("DualPlan", "dual_stream_wanted")}


@pytest.mark.parametrize("owner", list(OWNERS), ids=lambda m: m.__name__.rsplit(".", 1)[1])
def test_plan_module_hands_out_the_names_of_the_modules_split_from_it(owner):
    for name in OWNERS[owner]:
        assert getattr(plan, name) is getattr(owner, name), name
    assert plan.UNetPlan.__module__ == plan.__name__


def test_winograd_thresholds_are_read_where_tests_lower_them(monkeypatch):
    """tests/test_gpu_unet.py lowers plan.WINO_MIN_CHANNELS[_3D] with setattr: the plan must read them in that module"""
    for name in [k for k in os.environ if k.startswith("CLX_")]:
        monkeypatch.delenv(name)
    monkeypatch.setattr(_clx, "zeros", lambda shape, dtype, device: torch.empty(shape, dtype=dtype, device=device))
    for net, kernel in (("2d_small", (1, 3, 3)), ("3d_small", (3, 3, 3))):
        c = plan_trace.NETWORKS[net]
        topo = plan.build_topology(spatial=c["spatial"], **c["cfg"])
        assert not any(a["fwd"] for a in plan.UNetPlan(topo, c["batch"], CPU, True, allocate=False).algo.values())
        with monkeypatch.context() as m:
            m.setattr(plan, "WINO_MIN_CHANNELS", 4)
            m.setattr(plan, "WINO_MIN_CHANNELS_3D", 4)
            assert plan.wino_min_channels(kernel) == 4
            lowered = plan.UNetPlan(topo, c["batch"], CPU, True, allocate=False)
            assert any(a["fwd"] and a["wgrad"] and a["dgrad"] for a in lowered.algo.values())
