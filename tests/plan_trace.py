"""Launch traces of UNetPlan, made on the CPU: with _clx.call / stream_ptr / zero_many stubbed a plan packs, runs forward
and backward on host tensors, and every call it would launch is written down as text (tests/test_cpu_plan_trace.py
compares the sha256 of each trace with tests/plan_traces.json).

One line per call: the entry point, then its arguments.  A descriptor is written as its non-zero fields.  An address is
written as s<k>[<bytes of the storage>]+<byte offset>, k numbering the storages in order of first appearance; the
storages are those of every tensor reachable from the plans and the run's tensors WHEN the call is made (so a
temporary's address is never taken for a buffer that reuses it later).  16 (geometry-only queries) is `fake`, NULL is
`0`, an address in no known storage is ?<k>, k counting such addresses within the line.

    python tests/plan_trace.py --dump DIR     one text file per trace
    python tests/plan_trace.py --write        rewrite tests/plan_traces.json (only from a tree whose plan is trusted)
"""

import bisect
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), HERE) if p not in sys.path]

from cellulus_amd import _clx                                                   # noqa: E402
from cellulus_amd._clx import ClxConvDesc, ClxPackJob, ClxSrc                   # noqa: E402
from cellulus_amd.models.plan import UNetPlan, build_topology                   # noqa: E402
from test_gpu_unet import CONFIGS                                               # noqa: E402

HASHES = os.path.join(HERE, "plan_traces.json")


def _bench(nd, num_fmaps, spatial):
    return dict(cfg=dict(in_channels=1, out_channels=nd, num_fmaps=num_fmaps, fmap_inc_factor=3, features_in_last_layer=64,
                         downsampling_factors=[[2] * nd], num_spatial_dims=nd), spatial=spatial, batch=2)


NETWORKS = dict(CONFIGS, bench_2d=_bench(2, 256, (44, 52)), bench_3d=_bench(3, 64, (20, 20, 24)))
ENVS = {"default": {}, "f32": {"CLX_PRECISION": "f32"}, "g64": {"CLX_PRECISION": "f32x3bf16g64"},
        "deterministic": {"CLX_DETERMINISTIC": "1"}, "pack_single": {"CLX_PACK_BATCH": "0"},
        "plain": {"CLX_SUBPIXEL": "0", "CLX_WINOGRAD": "0"},
        "f32_fused_train": {"CLX_PRECISION": "f32", "CLX_WINO_FUSED_TRAIN": "1"}}
TRAIN_ENVS = {k + "=" + v: {k: v} for k, v in [
    ("CLX_WINOGRAD_TILE", "2"), ("CLX_FUSED_POOL", "0"), ("CLX_CHAIN64", "0"), ("CLX_GATE_BITS", "0"),
    ("CLX_WINO_ADJOINT", "0"), ("CLX_DY_DUAL", "0"), ("CLX_WINOGRAD_VCACHE", "0"), ("CLX_SP_EPILOGUE_PLANES", "0"),
    ("CLX_FIRST_DGRAD", "0")]}


class Recorder:
    def __init__(self, roots):
        self.roots, self.lines, self.held, self.starts, self.label = roots, [], {}, [], {}

    def _walk(self, o, seen):
        if id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            s = o.untyped_storage()
            self.held.setdefault(s.data_ptr(), (s.nbytes(), o))         # (held: a known storage is never freed and reused)
        elif isinstance(o, (dict, list, tuple, set)):
            for v in (o.values() if isinstance(o, dict) else o):
                self._walk(v, seen)
        elif type(o).__module__.startswith("cellulus_amd") and hasattr(o, "__dict__"):
            self._walk(vars(o), seen)

    def _find(self, a):
        i = bisect.bisect_right(self.starts, a) - 1
        if i >= 0 and a < self.starts[i] + max(self.held[self.starts[i]][0], 1):
            return self.starts[i]
        return None

    def addr(self, a, unknown):
        if not a:
            return "0"
        if a == 16:
            return "fake"
        start = self._find(a)
        if start is None:
            self._walk(self.roots, set())
            self.starts = sorted(self.held)
            start = self._find(a)
        if start is None:
            return "?%d" % unknown.setdefault(a, len(unknown))
        k = self.label.setdefault(start, len(self.label))
        return "s%d[%d]+%d" % (k, self.held[start][0], a - start)

    def struct(self, s, unknown, prefix=""):
        out = []
        for name, ctype in s._fields_:
            v = getattr(s, name)
            if ctype is ctypes.c_void_p:
                if v:
                    out.append("%s%s=%s" % (prefix, name, self.addr(v, unknown)))
            elif isinstance(v, ctypes.Array):
                for i, e in enumerate(v):
                    out += self.struct(e, unknown, "%s%s[%d]." % (prefix, name, i))
            elif v:
                out.append("%s%s=%d" % (prefix, name, v))
        return out

    def call(self, name, *args):
        unknown, words = {}, [name]
        for a in args:
            if isinstance(a, ctypes.c_void_p):
                words.append(self.addr(a.value, unknown))
            elif isinstance(getattr(a, "_obj", None), (ClxConvDesc, ClxSrc)):
                words.append("{" + " ".join(self.struct(a._obj, unknown)) + "}")
            else:
                words.append(repr(a))
        if name == "clx_pack_weights_batch":
            for job in (ClxPackJob * args[1]).from_address(args[0].value):
                words.append("[" + " ".join(self.struct(job, unknown)) + "]")
        self.lines.append(" ".join(words))

    def zero_many(self, *tensors):
        ts = [t for t in tensors if t is not None and t.numel() > 0]
        self.call("clx_zero_many", *[x for t in ts for x in (_clx.ptr(t), t.numel() * t.element_size())])

    def text(self, plan):
        head = [plan.algo, plan.sp_pass] + [sorted(getattr(plan, n, ())) for n in       # (adjoint, gate: training plans)
                                            ("chains", "fused_pool", "adjoint", "gate", "vcache", "xplanes")]
        return "\n".join([repr(h) for h in head] + ["arena_bytes %d" % plan.arena_bytes()] + self.lines) + "\n"


def network_traces(mp, net, envname, runs):
    """{trace id: text} of the runs `runs` (of infer, train, shared, sparse, share_forward) of one network"""
    c = NETWORKS[net]
    cfg, B, cpu = c["cfg"], c["batch"], torch.device("cpu")
    topo = build_topology(spatial=c["spatial"], **cfg)
    nd = topo.nd
    params = []
    for layer in topo.convs:
        params += [torch.empty((layer.cout, layer.cin) + tuple(layer.kernel[3 - nd:])), torch.empty(layer.cout)]
    flat = torch.empty(sum(p.numel() for p in params))
    grads, at = [], 0
    for p in params:
        grads.append(flat[at:at + p.numel()].view(p.shape))
        at += p.numel()
    raw = torch.empty((B, cfg["in_channels"]) + tuple(c["spatial"]))
    out = torch.empty((B, cfg["out_channels"]) + tuple(topo.out_shape[3 - nd:]))
    dout, dx = torch.empty_like(out), torch.empty_like(raw)
    roots, result = [params, flat, raw, out, dout, dx], {}
    mp.setattr(_clx, "stream_ptr", lambda device=None: ctypes.c_void_p(0))
    mp.setattr(_clx, "zeros", lambda shape, dtype, device: torch.empty(shape, dtype=dtype, device=device))  # (nothing computes)

    def record(run, plan, body):
        rec = Recorder(roots)
        mp.setattr(_clx, "call", rec.call)
        mp.setattr(_clx, "zero_many", rec.zero_many)
        body()
        result["%s/%s/%s" % (net, run, envname)] = rec.text(plan)

    def step(plan, version):
        plan.pack_weights(params, version, True)
        plan.forward(raw, params, out=out)
        plan.backward(dout, params, grads, flat_grad=flat, dx=dx)

    if "train" in runs:
        first = UNetPlan(topo, B, cpu, True)
        roots.append(first)
        record("train", first, lambda: (step(first, 1), step(first, 2)))
        if "shared" in runs:                # the second half of a DualPlan (DualPlan.pack_weights)
            second = UNetPlan(topo, B, cpu, True)
            roots.append(second)

            def shared():
                second._alloc_backward()
                second.share_from(first)
                second._packed_version = first._packed_version
                step(second, 2)
            record("shared", second, shared)
    if "infer" in runs:
        plan = UNetPlan(topo, B, cpu, False)
        roots.append(plan)
        record("infer", plan, lambda: (plan.pack_weights(params, 1, False), plan.forward(raw, params, out=out)))
        if "share_forward" in runs:
            other = UNetPlan(topo, B, cpu, False)
            roots.append(other)
            record("share_forward", other, lambda: (other.share_forward_from(plan), other.pack_weights(params, 1, False),
                                                    other.forward(raw, params, out=out)))
        if "sparse" in runs and plan.pointwise_prefix() is not None:
            # noisy copies of one image (UNetModel._sparse_prepare): the clean image's prefix on a one-image plan that reads
            # the chunk plan's weights, then the chunk plan on a few changed rows (and tiles)
            tail, tiled = plan.pointwise_prefix()[1], plan.tiled_layer_behind_prefix()
            one = UNetPlan(topo, 1, cpu, False)
            one.wpack_fwd, one._wplanes = plan.wpack_fwd, plan._wplanes
            sparse = dict(rows=torch.tensor([0, 5, 9], dtype=torch.int32), n=3)
            roots.extend([one, sparse])

            def body():
                rows = one.forward_prefix(raw[:1], params, len(tail) + (1 if tiled else 0))
                sparse["clean_rows"] = rows
                if tiled:
                    pool = one.fused_pool.get(tiled[0].name)
                    sparse.update(clean_rows=one.buf[tail[-1].out], clean_tile_rows=rows, tile_op=tiled[0], ntiles=2,
                                  tiles=torch.tensor([1, 3], dtype=torch.int32),
                                  clean_pool_rows=one.buf[pool.out] if pool is not None else None)
                plan.forward(raw, params, out=out, sparse=sparse)
            record("sparse", plan, body)
    return result


def all_traces(mp):
    """mp: a pytest.MonkeyPatch, which the caller undoes.  Every CLX_* switch of the caller's environment is dropped."""
    for name in [k for k in os.environ if k.startswith("CLX_")]:
        mp.delenv(name)
    result = {}
    for net in NETWORKS:
        for group, runs in ((ENVS, ("infer", "train", "shared", "sparse")), (TRAIN_ENVS, ("train",))):
            for envname, env in group.items():
                with mp.context() as m:
                    for k, v in env.items():
                        m.setenv(k, v)
                    result.update(network_traces(m, net, envname, runs + (("share_forward",) if not env else ())))
    return result


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


if __name__ == "__main__":
    with pytest.MonkeyPatch.context() as mp_:
        traces = all_traces(mp_)
    if sys.argv[1:2] == ["--dump"]:
        os.makedirs(sys.argv[2], exist_ok=True)
        for key, text_ in traces.items():
            with open(os.path.join(sys.argv[2], key.replace("/", "__") + ".txt"), "w") as f:
                f.write(text_)
    elif sys.argv[1:] == ["--write"]:
        with open(HASHES, "w") as f:
            json.dump({k: digest(v) for k, v in sorted(traces.items())}, f, indent=0)
            f.write("\n")
    else:
        sys.exit(__doc__)
