"""Launch plan of the U-Net + head on libclx (forward, backward, inference): UNetPlan executes a Topology
(topology.py) for a fixed batch size on one HIP device.

Everything device-side is channels-last f32 with channel counts padded to a
multiple of 4; the padded channels stay zero for the life of a buffer.

A plan is built in two phases: _decide chooses every layer's algorithm and every size from the topology, the switches
and the library's geometry-only queries, then _alloc takes the device memory those decisions ask for.  The backward
half does the same on the first training step (_decide_backward, _alloc_backward).
"""

import ctypes
import os

import torch

from .. import _clx
# (every name this module defined before topology.py, descriptors.py, subpixel.py and dual.py were split from it can
#  still be imported from here)
from .descriptors import (DEFAULT_PRECISION, FUSED_MAX_CHANNELS, PRECISION_CODES, QUERY_PTR, WINO_PACK_DGRAD,  # noqa: F401
                          WINO_PACK_FWD, WINO_TILE, conv_desc, conv_src, fused_pays, fused_wanted, pack_job_elements,
                          packed_taps, precision_code, precision_name, wino_taps, winograd_code, winograd_enabled)
from .subpixel import Subpixel, SubpixelHalf, fold_phase_grads, phase_weights, subpixel_geometry  # noqa: F401
from .topology import (ConvLayer, PoolOp, Source, Topology, build_topology, find_chain_pairs, forward_flops, pad4,  # noqa: F401
                       tensor_consumers)

# Winograd is used for 3x3 layers whose channel counts (both sides) reach this value: below it the
# extra HBM traffic of the transformed tensors and the short contraction (K = C per batched GEMM)
# outweigh the fewer MFMA FLOPs (measured at the benchmark config: 64 beats 128 by 2 %).
# CLX_WINOGRAD=0 forces the direct implicit-GEMM kernels everywhere; CLX_WINOGRAD_TILE selects
# F(2x2, 3x3) (2.25x fewer multiplications, error ~7e-7 of the output range on a 768-channel
# layer) or F(4x4, 3x3) (4x fewer, ~5e-6; the direct kernel: ~4e-7).
# (these two stay in this module, where the plan reads them: tests lower them here)
WINO_MIN_CHANNELS = int(os.environ.get("CLX_WINOGRAD_MIN_CHANNELS", "64"))
# 3-D layers (F(4x4) in (y, x) per z plane, the z taps inside the batched GEMMs): K = 3 * C per GEMM, so
# it pays from fewer channels than in 2-D
WINO_MIN_CHANNELS_3D = int(os.environ.get("CLX_WINOGRAD_MIN_CHANNELS_3D", "64"))


def wino_min_channels(kernel):
    return WINO_MIN_CHANNELS_3D if kernel[0] > 1 else WINO_MIN_CHANNELS


class UNetPlan:
    """Executes a Topology for a fixed batch size on one HIP device."""

    def __init__(self, topo: Topology, batch: int, device: torch.device, keep_activations: bool, allocate=True):
        """allocate=False: the decisions only — the plan owns no device memory and cannot run"""
        self.topo = topo
        self.B = int(batch)
        self.device = device
        self.keep = keep_activations
        self.precision = precision_code()
        # (the one-launch Winograd kernels multiply in float32: a layer whose products can run in the split precision takes
        #  the three-launch form — _fused_ok —, the narrow layers keep the one-launch form)
        self.fused = fused_wanted(keep_activations)
        # opt-in: run-to-run reproducible training (CLX_DETERMINISTIC=1; the reference's CPU autograd is
        # deterministic, cellulus/train.py:177-179).  Weight-gradient slices add in a fixed order, bias
        # gradients come from ordered column sums, the first layer takes the generic kernel and the fused
        # 1x1 pairs are off (their block sums meet in float atomics); train._fused_step switches the loss.
        self.deterministic = os.environ.get("CLX_DETERMINISTIC", "0") == "1"
        self._wplanes = {}          # data_ptr of a packed-weight tensor -> (tensor, its P3 planes, rows, K)
        self.aplanes = None         # scratch for the planes of a 1x1 layer's input (inference) ...
        self.xplanes = {}           # ... or one buffer per layer (training: the weight gradient reuses them)
        self._xplanes_fresh = set()
        self.dyplanes = None        # planes of the dY a 1x1 layer's weight gradient has split, reused by its data gradient
        self.dyplanes2 = None
        self._pointwise_reader = {}
        self.dx_bufs = {}           # the generic route of the input-image gradient (first_dgrad): scratch, made on first use
        self.buf = {}
        self.workspace = None
        self.vcache = {}
        self._vcache_fresh = set()
        self._packed_version = None
        self._bwd_ready = False
        # tensor -> the convolution / the pooling that produces it (backward_steps routes gradients by them)
        self._conv_by_out = {layer.out: layer for layer in topo.convs}
        self._pool_by_out = {p.out: p for p in topo.pools}
        self._decide()
        if allocate:
            self._alloc()

    def _fused_ok(self, cin_pad, cout):
        """the one-launch (float32) Winograd form for a 2-D layer cin_pad -> cout?  Where it pays (fused_pays) — in the
        float32-MFMA precision only: its 36 x 32 x 64 accumulators are ONE chain over the contraction (no room for the
        second set of the two-level summation), and with it on the 64-channel layers the default precision's inference
        plan sat at 8.26e-5 from float64 at a trained network's output scale where the three-launch forms give 7.20e-5
        and float32 MFMA 8.16e-5 (profiles/r06_parity_trained_scale_2d*.txt) — the promotion rule of DESIGN.md 4 asks
        for <=, so the default precision runs every Winograd layer in three launches (-4 % on an inference tile)."""
        return bool(self.fused and not self.precision and fused_pays(cin_pad, cout))

    # --------------------------------------------------------------- decisions
    def _addr(self, name, query):
        """the address of buffer `name` in a descriptor — of a geometry-only query, asked before the buffers exist: QUERY_PTR"""
        return QUERY_PTR if query else self.buf[name].data_ptr()

    def _takes(self, code, *passes):
        """Can every pass of `passes` — (descriptor, which: 0 clx_conv_fwd, 1 clx_conv_wgrad) — run with algorithm `code`?
        The library's answer is the workspace each needs (0: not applicable); taken, the plan's workspace covers them."""
        lib = _clx.load()
        need = []
        for d, which in passes:
            d.algo = code
            need.append(int(lib.clx_conv_workspace_bytes(ctypes.byref(d), which)))
        if not all(need):
            return False
        self.ws_bytes = max([self.ws_bytes] + need)
        return True

    def _fused_takes(self, d, cin_pad, cout):
        """the one-launch form for the F(4x4) forward call `d`?  (_fused_ok, and the library's word on the geometry)"""
        return bool(self._fused_ok(cin_pad, cout) and int(_clx.load().clx_conv_fused_applicable(ctypes.byref(d))))

    def _decide(self):
        """Phase one of construction: per layer the algorithm (direct implicit GEMM / Winograd) of forward, data gradient
        and weight gradient, the sub-pixel records, the split-precision passes, the fused pairs and poolings, and the size
        of the workspace — from the topology, the switches and the library's geometry-only queries.  Allocates nothing."""
        t = self.topo
        lib = _clx.load()
        code = winograd_code() if winograd_enabled() else 0
        self.algo = {}
        self.ws_bytes = 0
        for layer in t.convs:
            a = dict(fwd=0, dgrad=0, wgrad=0)
            if (code and min(layer.cin_pad, layer.cout) >= wino_min_channels(layer.kernel)
                    and (layer.kernel[0] == 1 or code == 2)):
                d = self._desc(layer, layer.cout, query=True)
                if self._takes(code, (d, 0)):
                    a["fwd"] = code
                    if code == 2 and layer.cout == pad4(layer.cout) and self._fused_takes(d, layer.cin_pad, layer.cout):
                        a["fwd"] = 3
                        self.ws_bytes = max(self.ws_bytes, int(lib.clx_conv_fused_workspace_bytes(ctypes.byref(d))))
                d.N = pad4(layer.cout)
                if self.keep and self._takes(code, (d, 1)):
                    a["wgrad"] = code
                if self.keep and layer.param_index > 0 and self._takes(code, (self._dgrad_desc(layer, None), 0)):
                    a["dgrad"] = code
            self.algo[layer.name] = a
        # sub-pixel form of the convolutions that read a nearest-upsampled tensor
        self.subpixel = {}
        for info in t.r_info:
            conv0 = info["conv0"]
            sp = subpixel_geometry(t, conv0)
            if sp is None:
                continue
            self.subpixel[conv0.name] = sp
            skip, low = sp.halves
            # the 2x2 convolution over the low-res tensor as Winograd F(4x4, 2x2)
            if (code == 2 and low.kernel in ((1, 2, 2), (2, 2, 2))
                    and min(low.Cp, low.rows) >= wino_min_channels(low.kernel)):
                dz = self._sp_descs(conv0, sp, query=True)[0]
                backward = [(dz, 1), (self._sp_low_dgrad_desc(conv0, sp, None), 0)] if self.keep else []
                if self._takes(2, (dz, 0), *backward):
                    low.wino = low.wino_dgrad = 2
                    low.fused = self._fused_takes(dz, low.Cp, low.rows)
                    if low.fused:
                        self.ws_bytes = max(self.ws_bytes, int(lib.clx_conv_fused_workspace_bytes(ctypes.byref(dz))))
            # ... and the 3x3 convolution over the skip tensor as F(4x4, 3x3), forward and weight
            # gradient only: its data gradient has K = N (64 at the benchmark config), too short
            # a contraction for the batched GEMMs to pay
            if (code == 2 and skip.kernel in ((1, 3, 3), (3, 3, 3)) and skip.Cp >= wino_min_channels(skip.kernel)
                    and sp.N >= wino_min_channels(skip.kernel) // 2):
                ds, dsw = (self._sp_descs(conv0, sp, query=True)[1] for _ in range(2))
                dsw.N = sp.N
                if self._takes(2, (ds, 0), *([(dsw, 1)] if self.keep else [])):
                    skip.wino = 2
                    skip.fused = conv0.cout == sp.N and self._fused_takes(ds, skip.Cp, conv0.cout)
            # its data gradient contracts over z taps x output channels: long enough only in 3-D
            if skip.wino and self.keep and sp.N * skip.kernel[0] >= WINO_MIN_CHANNELS:
                dd = self._dgrad_desc(conv0, None)
                dd.N = skip.Cp
                if self._takes(2, (dd, 0)):
                    skip.wino_dgrad = 2
            low.planes_fwd = bool(low.wino and self._sp_covers(self._sp_descs(conv0, sp, query=True)[0], 0,
                                                               3 if low.fused else low.wino))
        self._decide_sp()
        # scratch for the planes of a 1x1 layer's input (a training plan keeps one buffer per layer instead)
        rows_k = [(self.B * layer.in_shape[0] * layer.in_shape[1] * layer.in_shape[2], layer.cin_pad)
                  for layer in t.convs if self.sp_pass[layer.name][0] and not self.algo[layer.name]["fwd"]]
        self.aplanes_bytes = max((int(lib.clx_planes_bytes(r, k)) for r, k in rows_k), default=0)
        self._find_chains()
        # 2 x 2 max-pooling written by the Winograd output transform of the layer that produces the pooled tensor (2-D:
        # a pooling window lies inside one output tile; clx_conv_desc.pool_out).  CLX_FUSED_POOL=0: the separate pass
        self.fused_pool = {}
        if os.environ.get("CLX_FUSED_POOL", "1") != "0":
            by_out = {layer.out: layer for layer in t.convs}
            for pool in t.pools:
                layer = by_out.get(pool.src)
                if (layer is not None and self.algo[layer.name]["fwd"] and layer.kernel[0] == 1 and layer.in_shape[0] == 1
                        and tuple(pool.factor) == (1, 2, 2) and layer.cout % 4 == 0 and layer.name not in self.subpixel
                        and layer.out_shape[1] % 2 == 0 and layer.out_shape[2] % 2 == 0):
                    self.fused_pool[layer.name] = pool

    # ------------------------------------------------------------------ memory
    def _alloc(self):
        """Phase two: the device memory of the forward pass, as _decide sized it."""
        t = self.topo
        for name, (shape, c) in t.shapes.items():
            n = self.B * shape[0] * shape[1] * shape[2]
            self.buf[name] = _clx.zeros((n, pad4(c)), torch.float32, self.device)
        for sp in self.subpixel.values():
            n = self.B * sp.zshape[0] * sp.zshape[1] * sp.zshape[2]
            self.buf[sp.zname] = _clx.zeros((n, sp.low.rows), torch.float32, self.device)
            for h in sp.halves:
                h.w = torch.empty(h.rows * h.C * h.taps, dtype=torch.float32, device=self.device)
                h.wp_fwd = torch.empty(h.rows_pad * packed_taps(h.wino, h.kernel) * h.Cp, dtype=torch.float32,
                                       device=self.device)
        if self.ws_bytes:
            self.workspace = self._float_scratch(self.ws_bytes)
        # packed weights (with their P3 planes where the split-precision products read them)
        self.wpack_fwd = {}
        self.wpack_dgrad = {}
        for layer in t.convs:
            self.wpack_fwd[layer.name] = torch.empty(
                pad4(layer.cout) * packed_taps(self.algo[layer.name]["fwd"], layer.kernel) * layer.cin_pad,
                dtype=torch.float32, device=self.device)
            if self.sp_pass[layer.name][0]:
                self._register_wplanes(self.wpack_fwd[layer.name], layer.cin_pad)
        for sp in self.subpixel.values():
            if sp.low.planes_fwd:
                self._register_wplanes(sp.low.wp_fwd, sp.low.Cp)
        if self.aplanes_bytes:
            self.aplanes = torch.empty(self.aplanes_bytes, dtype=torch.uint8, device=self.device)

    def share_from(self, other):
        """Use `other`'s packed weights and gradient accumulators (same topology, batch size and switches): this
        plan then never packs, and its weight-gradient kernels add into the accumulators `other` unpacks."""
        assert other._bwd_ready and self._bwd_ready and other.B == self.B and other.algo == self.algo
        assert other.dw_off == self.dw_off and other.dwpack.numel() == self.dwpack.numel()
        self.wpack_fwd, self.wpack_dgrad, self.dwpack = other.wpack_fwd, other.wpack_dgrad, other.dwpack
        self._wplanes = other._wplanes
        for name, sp in self.subpixel.items():
            for h, o in zip(sp.halves, other.subpixel[name].halves):
                h.w, h.wp_fwd, h.wp_dgrad, h.dw = o.w, o.wp_fwd, o.wp_dgrad, o.dw

    def share_forward_from(self, other):
        """Forward-only version of share_from: this plan reads `other`'s packed weights and never packs."""
        assert other.B == self.B and other.algo == self.algo and other.keep == self.keep
        self.wpack_fwd = other.wpack_fwd
        self._wplanes = other._wplanes
        for name, sp in self.subpixel.items():
            for h, o in zip(sp.halves, other.subpixel[name].halves):
                h.w, h.wp_fwd = o.w, o.wp_fwd
        self._packed_version = other._packed_version

    def _find_chains(self):
        """Pairs of consecutive 64-channel 1x1 layers (conv_pass.2 -> conv_pass.4 of a level, head.0 ->
        head.2) that run as ONE launch each way (csrc/chain64.hip: the intermediate tensor is written once
        and never read back, its gradient never exists in HBM).  CLX_CHAIN64=0 keeps the layer-by-layer path."""
        self.chains, self.chain_second = {}, {}
        if os.environ.get("CLX_CHAIN64", "1") == "0" or self.deterministic:
            return
        for a, b in find_chain_pairs(self.topo, {n: v["fwd"] for n, v in self.algo.items()}, self.B):
            self.chains[a.name] = (a, b)
            self.chain_second[b.name] = (a, b)

    def _subpixel_layers(self):
        """(layer, its record) of every convolution that runs in the sub-pixel form"""
        return [(info["conv0"], self.subpixel[info["conv0"].name]) for info in self.topo.r_info
                if info["conv0"].name in self.subpixel]

    def _decide_backward(self):
        """Phase one of the backward half, taken with its allocation on the first training step (its switches are read
        then): which tensors get ReLU gate bits, the adjoint data gradients, which transformed tensors and operand planes
        are kept, and the size of each.  Allocates nothing."""
        t = self.topo
        lib = _clx.load()
        keep_v = os.environ.get("CLX_WINOGRAD_VCACHE", "1") != "0"
        for layer, sp in self._subpixel_layers():
            dz, ds = self._sp_descs(layer, sp, query=True)
            for h, d in ((sp.skip, ds), (sp.low, dz)):
                h.vcache_bytes = self._vcache_bytes(d, h.wino, 0) if h.wino and not h.fused and keep_v else None
            sp.low.planes_dgrad = bool(sp.low.wino
                                       and self._sp_covers(self._sp_low_dgrad_desc(layer, sp, None), 0, sp.low.wino))
        # ReLU gates as bits: written by the epilogue that produces a layer's output, read by the data
        # gradient that passes through that ReLU — 1/32 of the float tensor it would otherwise read (the
        # 64-channel 1x1 layers of the 3-D network are HBM-bound).  Whole words per pixel (channels %
        # 32 == 0) and a producer that knows the bits (not the first-layer kernels); CLX_GATE_BITS=0 = off
        self.gate_shape = {}
        # (the fused 1x1 pairs gate by the float tensors they read anyway: no bits for their input and middle)
        chain_gated = {a.out for a, _b in self.chains.values()} | {a.sources[0].tensor for a, _b in self.chains.values()}
        if os.environ.get("CLX_GATE_BITS", "1") != "0":
            for layer in t.convs:
                if layer.out in chain_gated:
                    continue
                if layer.relu and layer.param_index > 0 and pad4(layer.cout) % 32 == 0:
                    n = self.B * layer.out_shape[0] * layer.out_shape[1] * layer.out_shape[2]
                    self.gate_shape[layer.out] = (n, pad4(layer.cout) // 32)
        # F(4x4, 3x3[x3]) layers whose weight AND data gradient are Winograd: the data gradient in its ADJOINT form,
        # dX = sum over tiles of B [U^T (A dY A^T)] B^T — its operand A dY A^T is what the weight gradient has just left
        # in the workspace, so dY is transformed once and the (K-1)-padded input transform of dY is never written
        # (clx_conv_desc.adjoint; CLX_WINO_ADJOINT=0 = the two-transform form)
        self.adjoint = set()
        if os.environ.get("CLX_WINO_ADJOINT", "1") != "0":
            for layer in t.convs:
                a = self.algo[layer.name]
                if (a["wgrad"] == 2 and a["dgrad"] == 2 and tuple(layer.kernel) in ((1, 3, 3), (3, 3, 3)) and layer.param_index > 0
                        and layer.name not in self.subpixel and len(layer.sources) == 1):
                    self.adjoint.add(layer.name)
        # a Winograd layer's weight gradient and data gradient both transform dY: one pass produces both
        # (clx_conv_desc.dy_vcache); the buffer is shared by all layers (written and consumed back to back)
        self.dycache_bytes = 0
        if os.environ.get("CLX_DY_DUAL", "1") != "0":
            for layer in t.convs:
                a = self.algo[layer.name]
                if a["wgrad"] and a["wgrad"] == a["dgrad"] and layer.name not in self.subpixel and layer.name not in self.adjoint:
                    d = self._desc(layer, pad4(layer.cout), query=True)
                    self.dycache_bytes = max(self.dycache_bytes, self._vcache_bytes(d, a["wgrad"], 1))
            for layer, sp in self._subpixel_layers():
                if sp.low.wino:
                    dz = self._sp_descs(layer, sp, query=True)[0]
                    self.dycache_bytes = max(self.dycache_bytes, self._vcache_bytes(dz, sp.low.wino, 1))
        # forward and weight gradient of a Winograd layer transform the same input: keep V
        self.vcache_bytes = {}
        for layer in t.convs:
            a = self.algo[layer.name]
            if a["fwd"] and a["fwd"] == a["wgrad"] and keep_v:
                self.vcache_bytes[layer.name] = self._vcache_bytes(self._desc(layer, layer.cout, query=True), a["fwd"], 0)
        # the packed weight gradients: one accumulator, a slice per layer
        total = 0
        self.dw_off = {}
        for layer in t.convs:
            self.dw_off[layer.name] = total
            total += packed_taps(self.algo[layer.name]["wgrad"], layer.kernel) * pad4(layer.cout) * layer.cin_pad
        # training: the planes of a split 1x1 layer's input stay for its weight gradient; one scratch for the planes of dY
        self.xplanes_bytes = {}
        self.dyplanes_bytes = 0
        for layer in t.convs:
            if layer.name in self.chains or layer.name in self.chain_second:
                continue
            a = self.algo[layer.name]
            fwd_sp, dgrad_sp, wgrad_sp = (on and not a[k] for on, k in zip(self.sp_pass[layer.name], ("fwd", "dgrad", "wgrad")))
            rows = self.B * layer.in_shape[0] * layer.in_shape[1] * layer.in_shape[2]
            if fwd_sp or wgrad_sp:
                self.xplanes_bytes[layer.name] = int(lib.clx_planes_bytes(rows, layer.cin_pad))
            if dgrad_sp or wgrad_sp:
                self.dyplanes_bytes = max(self.dyplanes_bytes, int(lib.clx_planes_bytes(rows, pad4(layer.cout))))
        # tensor -> the 1x1 layer that reads it as its one plain source and keeps planes of it
        for layer in t.convs:
            if layer.name in self.xplanes_bytes and pad4(t.shapes[layer.sources[0].tensor][1]) == layer.cin_pad:
                self._pointwise_reader[layer.sources[0].tensor] = layer
        # the sub-pixel layers' weight-gradient accumulators live behind the others: one fill zeroes all
        self.sp_dw_slices = []
        for sp in self.subpixel.values():
            for h in sp.halves:
                n = packed_taps(h.wino, h.kernel) * h.rows_pad * h.Cp
                self.sp_dw_slices.append((h, total, n))
                total += n
        self.dwpack_numel = total

    def _alloc_backward(self):
        """Phase two of the backward half: its device memory, as _decide_backward sized it."""
        self._decide_backward()
        t = self.topo
        self.gbuf = {}
        for name, (shape, c) in t.shapes.items():
            if name == "raw":
                continue
            n = self.B * shape[0] * shape[1] * shape[2]
            self.gbuf[name] = _clx.zeros((n, pad4(c)), torch.float32, self.device)
        for info in t.r_info:
            layer = info["conv0"]
            n = self.B * layer.in_shape[0] * layer.in_shape[1] * layer.in_shape[2]
            sp = self.subpixel.get(layer.name)
            if sp is None:
                self.gbuf["cat%d" % info["level"]] = _clx.zeros((n, layer.cin_pad), torch.float32, self.device)
                continue
            self.gbuf["dskip%d" % info["level"]] = _clx.zeros((n, sp.skip.Cp), torch.float32, self.device)
            self.gbuf[sp.zname] = _clx.zeros(tuple(self.buf[sp.zname].shape), torch.float32, self.device)
            for h in sp.halves:
                h.wp_dgrad = torch.empty(h.Cp * packed_taps(h.wino_dgrad, h.kernel) * h.rows_pad, dtype=torch.float32,
                                         device=self.device)
                h.g = torch.empty(h.rows * h.C * h.taps, dtype=torch.float32, device=self.device)
                if h.vcache_bytes is not None:
                    h.vcache = self._float_scratch(h.vcache_bytes)
            if sp.low.planes_dgrad:
                self._register_wplanes(sp.low.wp_dgrad, sp.low.rows, dgrad=True)
        self.gate = {name: _clx.zeros(shape, torch.int32, self.device) for name, shape in self.gate_shape.items()}
        self.dycache = self._float_scratch(self.dycache_bytes) if self.dycache_bytes else None
        self.vcache = {name: self._float_scratch(n) for name, n in self.vcache_bytes.items()}
        for layer in t.convs:
            if layer.param_index > 0:  # first layer needs no data gradient
                self.wpack_dgrad[layer.name] = torch.empty(
                    layer.cin_pad * packed_taps(self.algo[layer.name]["dgrad"], layer.kernel) * pad4(layer.cout),
                    dtype=torch.float32, device=self.device)
                if self.sp_pass[layer.name][1]:
                    self._register_wplanes(self.wpack_dgrad[layer.name], pad4(layer.cout), dgrad=True)
        for name, n in self.xplanes_bytes.items():
            self.xplanes[name] = torch.empty(n, dtype=torch.uint8, device=self.device)
        if self.dyplanes_bytes:
            # two of them: a data gradient reads the planes of its dY out of one while its epilogue writes the planes
            # of the next layer's dY into the other
            self.dyplanes = torch.empty(self.dyplanes_bytes, dtype=torch.uint8, device=self.device)
            self.dyplanes2 = torch.empty(self.dyplanes_bytes, dtype=torch.uint8, device=self.device)
        self.dwpack = _clx.zeros(self.dwpack_numel, torch.float32, self.device)
        if self.deterministic:
            width = max(pad4(layer.cout) for layer in t.convs)
            self._det_turns = _clx.zeros(1 << 20, torch.int32, self.device)     # 4 MB of turn counters
            self._det_colsum = torch.empty(int(_clx.load().clx_colsum_scratch_bytes(width)) // 4, dtype=torch.float32,
                                           device=self.device)
        for h, off, n in self.sp_dw_slices:
            h.dw = self.dwpack[off:off + n]
        self._bwd_ready = True

    # --------------------------------------------------------------- sub-pixel
    def _phase_weights(self, layer, sp, w_up):
        return phase_weights(layer, sp, w_up)

    def _fold_phase_grads(self, layer, sp, dweff):
        return fold_phase_grads(layer, sp, dweff)

    def _sp_descs(self, layer, sp, query=False):
        """(Z-convolution descriptor over the low-res tensor, skip-convolution descriptor with the forward pass's N =
        cout: its weight gradient has N = pad4(cout)).  query: for a geometry-only query (_addr)."""
        t = self.topo
        skip_s, up_s = layer.sources
        low_shape, low_c = t.shapes[up_s.tensor]
        sshape, sc = t.shapes[skip_s.tensor]
        dz = conv_desc([conv_src(self._addr(up_s.tensor, query), sp.low.Cp, pad4(low_c), low_shape)], self.B, low_shape,
                       sp.low.kernel, (0, 0, 0), sp.low.rows, self.precision)
        ds = conv_desc([conv_src(self._addr(skip_s.tensor, query), sp.skip.Cp, pad4(sc), sshape, crop=skip_s.crop)],
                       self.B, layer.in_shape, layer.kernel, (0, 0, 0), layer.cout, self.precision)
        return dz, ds

    def _sp_split(self, layer, sp, w, st):
        """one launch: the skip half's weights and the phase-summed weights of the upsampled half
        (_phase_weights is the same algebra in torch ops, kept as the CPU-testable statement)"""
        wv = w.detach()
        if not wv.is_contiguous():
            wv = wv.contiguous()
        _clx.call("clx_subpixel_split_weights", _clx.ptr(wv), _clx.ptr(sp.skip.w), _clx.ptr(sp.low.w), layer.cout,
                  layer.cin, sp.skip.C, sp.N, *layer.kernel, *sp.fac, st)

    def _sp_half_forward(self, h, d):
        """what the forward launches of both halves share: packed weights, algorithm, the transformed input kept"""
        self._set_wpack(d, h.wp_fwd)
        h.v_fresh = False
        if h.fused:
            self._use_workspace(d, 3)
        elif h.wino:
            self._use_workspace(d, h.wino)
            if self.keep and h.vcache is not None:
                d.vcache = h.vcache.data_ptr()
                h.v_fresh = True

    def _sp_forward(self, layer, sp, bias, st):
        dz, ds = self._sp_descs(layer, sp)
        zbuf = self.buf[sp.zname]
        dz.out = zbuf.data_ptr()
        dz.ld_out = sp.low.rows
        self._sp_half_forward(sp.low, dz)
        _clx.call("clx_conv_fwd", ctypes.byref(dz), st)
        out = self.buf[layer.out]
        zs = sp.zshape
        _clx.call("clx_depth_to_space", _clx.ptr(zbuf), sp.low.rows, _clx.ptr(out), sp.N, self.B,
                  zs[0], zs[1], zs[2], sp.N, *sp.fac, st)
        ds.bias = bias.data_ptr() if bias is not None else None
        ds.relu = 1 if layer.relu else 0
        ds.accumulate = 1
        ds.out = out.data_ptr()
        ds.ld_out = sp.N
        if layer.relu and self.keep:
            self._set_gate_out(ds, layer.out)
        self._sp_half_forward(sp.skip, ds)
        _clx.call("clx_conv_fwd", ctypes.byref(ds), st)

    def _sp_wgrad(self, layer, sp, dy, gw, gb, st):
        """weight/bias gradient of a sub-pixel layer (added into the layer's slices of self.dwpack); returns
        unpack(stream), which unpacks both halves and folds them into `gw`."""
        dz, ds = self._sp_descs(layer, sp)
        skip, low = sp.halves
        zs = sp.zshape
        # dZ = space_to_depth(dY)
        dzbuf = self.gbuf[sp.zname]
        _clx.call("clx_space_to_depth", _clx.ptr(dy), sp.N, _clx.ptr(dzbuf), low.rows, self.B,
                  zs[0], zs[1], zs[2], sp.N, *sp.fac, st)
        # weight gradients (the halves' dw are slices of self.dwpack: zeroed with it)
        ds.N = sp.N
        if low.wino and self.dycache is not None:
            dz.dy_vcache = self.dycache.data_ptr()
        for h, d, dyh, ld_dy, gbh, nbias in ((skip, ds, dy, sp.N, gb, layer.cout), (low, dz, dzbuf, low.rows, None, 0)):
            if h.wino:
                self._use_workspace(d, h.wino)
                if h.v_fresh:
                    d.vcache = h.vcache.data_ptr()
                    d.vcache_valid = 1
            self._wgrad(d, dyh, ld_dy, h.dw, gbh, nbias, st)

        def unpack(st):
            for h in sp.halves:
                if h.wino:
                    _clx.call("clx_unpack_wgrad_wino", _clx.ptr(h.dw), _clx.ptr(h.g), h.rows, h.C, h.rows_pad, h.Cp,
                              WINO_TILE[h.wino], h.kernel[1], h.kernel[0], st)
                else:
                    _clx.call("clx_unpack_wgrad", _clx.ptr(h.dw), _clx.ptr(h.g), h.rows, h.C, h.taps, h.rows_pad, h.Cp, st)
            # adjoint of the weight split (one launch; _fold_phase_grads states the same in torch ops)
            _clx.call("clx_subpixel_fold_grads", _clx.ptr(skip.g), _clx.ptr(low.g), _clx.ptr(gw), layer.cout, layer.cin,
                      skip.C, sp.N, *layer.kernel, *sp.fac, st)
        return unpack

    def _sp_dgrad(self, layer, sp, dy, st):
        """both data gradients of a sub-pixel layer (after _sp_wgrad: it reads the transformed dZ that call left
        in self.dycache); returns the skip gradient buffer (pre-gate, full skip-crop grid)."""
        skip, low = sp.halves
        dzbuf = self.gbuf[sp.zname]
        # data gradient of the skip branch (gated later, together with the max-pool gradient)
        dskip = self.gbuf["dskip%d" % sp.level]
        dd = self._dgrad_desc(layer, dy)
        dd.N = skip.Cp
        self._set_wpack(dd, skip.wp_dgrad)
        dd.out = dskip.data_ptr()
        dd.ld_out = skip.Cp
        if skip.wino_dgrad:
            self._use_workspace(dd, skip.wino_dgrad)
        _clx.call("clx_conv_fwd", ctypes.byref(dd), st)
        # data gradient of the low-res tensor straight from dZ (replaces upsample backward)
        dl = self._sp_low_dgrad_desc(layer, sp, dzbuf)
        self._set_wpack(dl, low.wp_dgrad)
        if low.wino:
            self._use_workspace(dl, low.wino)
            if self.dycache is not None:       # written by the weight-gradient call on dZ above
                dl.vcache = self.dycache.data_ptr()
                dl.vcache_valid = 1
        _clx.call("clx_conv_fwd", ctypes.byref(dl), st)
        return dskip

    def _sp_low_dgrad_desc(self, layer, sp, dzbuf):
        """dL/d(low-res tensor) as the transposed 2x2(x2) convolution of dZ, ReLU gate fused."""
        low = sp.low
        up_s = layer.sources[1]
        low_shape, low_c = self.topo.shapes[up_s.tensor]
        # (geometry-only queries never dereference)
        dl = conv_desc([conv_src(dzbuf.data_ptr() if dzbuf is not None else QUERY_PTR, low.rows, low.rows, sp.zshape)], self.B,
                       sp.zshape, low.kernel, tuple(k - 1 for k in low.kernel), low.Cp, self.precision)
        dl.ld_out = pad4(low_c)
        if dzbuf is not None:
            self._set_mask(dl, up_s.tensor)                 # ReLU gate of the low-res tensor
            dl.out = self.gbuf[up_s.tensor].data_ptr()
        else:                                               # geometry-only query
            dl.mask = QUERY_PTR
            dl.ld_mask = pad4(low_c)
        return dl

    # ------------------------------------------------------------- descriptors
    def _desc(self, layer: ConvLayer, N, query=False):
        """forward / weight-gradient descriptor of a plain layer with N output channels (cout / pad4(cout)); query: for a
        geometry-only query (_addr)"""
        t = self.topo
        srcs = [conv_src(self._addr(s.tensor, query), pad4(s.channels), pad4(t.shapes[s.tensor][1]), t.shapes[s.tensor][0],
                         s.crop, s.factor) for s in layer.sources]
        # a raw image with 1-3 channels is stored padded to 4: tell the first-layer kernels
        return conv_desc(srcs, self.B, layer.in_shape, layer.kernel, (0, 0, 0), N, self.precision,
                         c_real=layer.sources[0].channels if len(layer.sources) == 1 else 0)

    def _set_gate_out(self, d, name):
        """forward epilogue of the layer producing buffer `name`: also emit the ReLU gates as bits"""
        g = getattr(self, "gate", {}).get(name) if self._bwd_ready else None
        if g is not None:
            d.gate_out = g.data_ptr()
            d.ld_gate = g.shape[1]

    def _set_mask(self, d, name, relu=True):
        """data-gradient epilogue: gate by the ReLU of the layer that produced buffer `name`"""
        g = self.gate.get(name)
        if not relu:
            return
        if g is not None:
            d.mask_bits = g.data_ptr()
            d.ld_mask_bits = g.shape[1]
        else:
            d.mask = self.buf[name].data_ptr()
            d.ld_mask = self.buf[name].shape[1]

    def _use_workspace(self, d, code):
        d.algo = code
        if self.workspace is None:      # (only one-launch fused layers: nothing needs scratch)
            return
        d.workspace = self.workspace.data_ptr()
        d.workspace_bytes = self.workspace.numel() * 4

    # ------------------------------------------------- split precision (CLX_PRECISION=f32x3bf16 / f32x3bf16g64; csrc/gemm_sp.hip)
    def arena_bytes(self):
        """device bytes of this plan's own activations and scratch (not the packed weights and their planes, which plans of one
        model share): what a second plan of the same shape on another stream takes"""
        ts = list(self.buf.values()) + [self.workspace, self.aplanes, self.dyplanes, getattr(self, "dyplanes2", None)]
        ts += list(self.xplanes.values()) + list(self.vcache.values())
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def _sp_covers(self, d, pass_, algo):
        """clx_conv_sp_covers: does the call of pass `pass_` (0: clx_conv_fwd, data-gradient form included; 1:
        clx_conv_wgrad) with descriptor `d` and algorithm `algo` run its products in the split precision?"""
        d.algo = algo
        return bool(_clx.load().clx_conv_sp_covers(ctypes.byref(d), pass_))

    def _decide_sp(self):
        """sp_pass[layer name] = (forward, data gradient, weight gradient) in the split precision: the library's answer
        for the descriptors the layer launches with.  (A sub-pixel layer launches descriptors of its own: _sp_descs.)"""
        self.sp_pass = {}
        for layer in self.topo.convs:
            if layer.name in self.subpixel:
                self.sp_pass[layer.name] = (False, False, False)
                continue
            a = self.algo[layer.name]
            d = self._desc(layer, layer.cout, query=True)
            fwd = self._sp_covers(d, 0, a["fwd"])
            d.N = pad4(layer.cout)
            wgrad = self._sp_covers(d, 1, a["wgrad"])
            dgrad = layer.param_index > 0 and self._sp_covers(self._dgrad_desc(layer, None), 0, a["dgrad"])
            self.sp_pass[layer.name] = (fwd, dgrad, wgrad)

    def _register_wplanes(self, wp, k, dgrad=False):
        """planes for the packed weights `wp` seen as [rows][k] (the B operand of the split-precision products that read
        them); `dgrad`: data-gradient weights, split only after a packing that includes them"""
        if wp.data_ptr() not in self._wplanes:
            rows = wp.numel() // k
            nbytes = int(_clx.load().clx_planes_bytes(rows, k))
            self._wplanes[wp.data_ptr()] = (wp, torch.empty(nbytes, dtype=torch.uint8, device=self.device), rows, k, dgrad)

    def _set_wpack(self, d, wp):
        d.wpack = wp.data_ptr()
        e = self._wplanes.get(wp.data_ptr())
        d.wplanes = e[1].data_ptr() if e is not None else None

    def _split_wplanes(self, need_dgrad, st):
        """the planes of every registered packed-weight tensor the last packing wrote"""
        for wp, planes, rows, k, dgrad in self._wplanes.values():
            if need_dgrad or not dgrad:
                _clx.call("clx_split_planes", _clx.ptr(wp), k, rows, k, _clx.ptr(planes), st)

    def _vcache_bytes(self, d, algo, which):
        """clx_conv_vcache_bytes of the Winograd call `d` with algorithm `algo` (float32, or P3 planes where it runs in the
        split precision)"""
        d.algo = algo
        return int(_clx.load().clx_conv_vcache_bytes(ctypes.byref(d), which))

    def _float_scratch(self, nbytes):
        return torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=self.device)

    def _dgrad_desc(self, layer: ConvLayer, dy):
        """Data gradient as a convolution of dy (zero padding k-1, flipped transposed weights)."""
        n = pad4(layer.cout)
        # (geometry-only queries never dereference)
        return conv_desc([conv_src(dy.data_ptr() if dy is not None else QUERY_PTR, n, n, layer.out_shape)], self.B, layer.out_shape,
                         layer.kernel, tuple(k - 1 for k in layer.kernel), layer.cin_pad, self.precision)

    def _expand_cin(self, layer, w):
        """torch weight (cout, cin, taps) -> (cout, cin_gapped, taps) when a concat source is padded."""
        if len(layer.sources) == 1 or all(s.channels % 4 == 0 for s in layer.sources[:-1]):
            return w, layer.cin
        parts, c0 = [], 0
        for s in layer.sources:
            blk = w[:, c0:c0 + s.channels]
            padw = pad4(s.channels) - s.channels
            if padw:
                blk = torch.cat([blk, blk.new_zeros(blk.shape[0], padw, blk.shape[2])], dim=1)
            parts.append(blk)
            c0 += s.channels
        g = torch.cat(parts, dim=1).contiguous()
        return g, g.shape[1]

    def _compress_cin(self, layer, g):
        """inverse of _expand_cin for gradients: (cout, cin_gapped, taps) -> (cout, cin, taps)."""
        parts, c0 = [], 0
        for s in layer.sources:
            parts.append(g[:, c0:c0 + s.channels])
            c0 += pad4(s.channels)
        return torch.cat(parts, dim=1)

    def _wgrad(self, d, dy, ld_dy, dwp, gb, nbias, st):
        """clx_conv_wgrad; in reproducible mode with ordered slices and the bias gradient from ordered column
        sums of dy (rows = output pixels of the layer, `nbias` real channels)."""
        if not self.deterministic:
            _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy), ld_dy, _clx.ptr(dwp),
                      _clx.ptr(gb) if gb is not None else None, st)
            return
        need = int(_clx.load().clx_conv_wgrad_turns_bytes(ctypes.byref(d)))
        if need > self._det_turns.numel() * 4:
            self._det_turns = _clx.zeros(need // 4 + 1, torch.int32, self.device)
        d.det_turns = self._det_turns.data_ptr()
        _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy), ld_dy, _clx.ptr(dwp), None, st)
        if gb is not None:
            _clx.call("clx_colsum_ordered", _clx.ptr(dy), ld_dy, dy.shape[0], nbias, _clx.ptr(gb),
                      _clx.ptr(self._det_colsum), st)

    def _unpack_step(self, layer, dwp, gw, wino_w):
        """unpack(stream) for one layer: packed weight gradient `dwp` -> torch-layout gradient `gw`."""
        def unpack(st):
            if wino_w:
                _clx.call("clx_unpack_wgrad_wino", _clx.ptr(dwp), _clx.ptr(gw), layer.cout, layer.cin,
                          pad4(layer.cout), layer.cin_pad, WINO_TILE[wino_w], 3, layer.kernel[0], st)
            elif len(layer.sources) == 1 or all(s.channels % 4 == 0 for s in layer.sources[:-1]):
                _clx.call("clx_unpack_wgrad", _clx.ptr(dwp), _clx.ptr(gw), layer.cout, layer.cin,
                          layer.taps, pad4(layer.cout), layer.cin_pad, st)
            else:       # (torch ops: they run on torch's current stream, which is the caller's `st`)
                tmp = torch.empty((layer.cout, layer.cin_pad, layer.taps), dtype=torch.float32,
                                  device=self.device)
                _clx.call("clx_unpack_wgrad", _clx.ptr(dwp), _clx.ptr(tmp), layer.cout, layer.cin_pad,
                          layer.taps, pad4(layer.cout), layer.cin_pad, st)
                gw.copy_(self._compress_cin(layer, tmp).reshape(gw.shape))
        return unpack

    def _chain_forward(self, a, b, params, st):
        """y1 = relu(x w1^T + b1), y2 = act(y1 w2^T + b2) in one launch (clx_chain64_fwd)."""
        M = self.B * a.in_shape[0] * a.in_shape[1] * a.in_shape[2]
        x = self.buf[a.sources[0].tensor]
        y1, y2 = self.buf[a.out], self.buf[b.out]
        g1 = g2 = None
        if self.keep and self._bwd_ready:
            g1 = self.gate.get(a.out)
            g2 = self.gate.get(b.out) if b.relu else None
        b1, b2 = params[2 * a.param_index + 1], params[2 * b.param_index + 1]
        _clx.call("clx_chain64_fwd", _clx.ptr(x), x.shape[1], M, _clx.ptr(self.wpack_fwd[a.name]), _clx.ptr(b1),
                  _clx.ptr(y1) if self.keep else None, y1.shape[1], _clx.ptr(g1), g1.shape[1] if g1 is not None else 0,
                  _clx.ptr(self.wpack_fwd[b.name]), _clx.ptr(b2), b.cout, 1 if b.relu else 0, _clx.ptr(y2),
                  y2.shape[1], _clx.ptr(g2), g2.shape[1] if g2 is not None else 0, st)

    def _chain_backward(self, a, b, prev, grads, st):
        """Both data gradients, both weight gradients and both bias gradients of the pair in one launch
        (clx_chain64_bwd); the gradient w.r.t. the middle tensor is never written.  Returns unpack(stream)."""
        M = self.B * a.in_shape[0] * a.in_shape[1] * a.in_shape[2]
        dp2 = self.gbuf[b.out]
        x, y1 = self.buf[a.sources[0].tensor], self.buf[a.out]
        dp0 = self.gbuf[prev.out]
        n2p = pad4(b.cout)
        dw2 = self.dwpack[self.dw_off[b.name]:self.dw_off[b.name] + n2p * 64]
        dw1 = self.dwpack[self.dw_off[a.name]:self.dw_off[a.name] + 64 * 64]
        _clx.call("clx_chain64_bwd", _clx.ptr(dp2), dp2.shape[1], b.cout, _clx.ptr(y1), y1.shape[1], _clx.ptr(x),
                  x.shape[1], 1 if prev.relu else 0, M, _clx.ptr(self.wpack_dgrad[b.name]),
                  _clx.ptr(self.wpack_dgrad[a.name]), _clx.ptr(dp0), dp0.shape[1], _clx.ptr(dw2),
                  _clx.ptr(grads[2 * b.param_index + 1]), _clx.ptr(dw1), _clx.ptr(grads[2 * a.param_index + 1]), st)

        def unpack(st):
            for layer, dwp in ((b, dw2), (a, dw1)):
                _clx.call("clx_unpack_wgrad", _clx.ptr(dwp), _clx.ptr(grads[2 * layer.param_index]), layer.cout,
                          layer.cin, 1, pad4(layer.cout), layer.cin_pad, st)
        return unpack

    def _pack_jobs(self, params, need_dgrad):
        """The packings of a step, layer by layer in launch order: yields (layer, copy, jobs), jobs = the argument lists
        (source, destination, cout, cin, taps, cin_pad, cout_pad, clx_pack_mode) of the layer's clx_pack_weights calls.
        A sub-pixel layer packs its halves' weights (_sp_split writes them first).  copy: the parameter cannot be read
        as it is — not contiguous, or a concatenation of odd channel counts — and _pack_one reads a copy instead."""
        for layer in self.topo.convs:
            w = params[2 * layer.param_index]
            sp = self.subpixel.get(layer.name)
            if sp is not None:
                jobs = [(h.w, h.wp_fwd, h.rows, h.C, h.taps, h.Cp, h.rows_pad, 7 if h.fused else 4 if h.wino else 0)
                        for h in sp.halves]
                if need_dgrad:
                    jobs += [(h.w, h.wp_dgrad, h.rows, h.C, h.taps, h.Cp, h.rows_pad, 5 if h.wino_dgrad else 1)
                             for h in sp.halves]
                yield layer, False, jobs
                continue
            algo = self.algo[layer.name]
            dsts = [(self.wpack_fwd[layer.name], WINO_PACK_FWD.get(algo["fwd"], 0))]
            if need_dgrad and layer.name in self.wpack_dgrad:
                dsts.append((self.wpack_dgrad[layer.name],
                             6 if layer.name in self.adjoint else WINO_PACK_DGRAD.get(algo["dgrad"], 1)))
            gapped = len(layer.sources) > 1 and not all(s.channels % 4 == 0 for s in layer.sources[:-1])
            yield layer, gapped or not w.is_contiguous(), [
                (w, dst, layer.cout, layer.cin, layer.taps, layer.cin_pad, pad4(layer.cout), mode) for dst, mode in dsts]

    def _pack_one(self, layer, copy, jobs, params, st):
        """one layer's packings, a launch each"""
        if copy:
            wv = params[2 * layer.param_index].detach().reshape(layer.cout, layer.cin, layer.taps)
            if not wv.is_contiguous():
                wv = wv.contiguous()
            wv, cin_eff = self._expand_cin(layer, wv)
            jobs = [(wv, dst, cout, cin_eff) + tuple(rest) for _w, dst, cout, _cin, *rest in jobs]
        for src, dst, *rest in jobs:
            _clx.call("clx_pack_weights", _clx.ptr(src), _clx.ptr(dst), *rest, st)

    def _pack_batched(self, params, need_dgrad, st):
        """Every packing of the step in ONE launch (clx_pack_weights_batch): the job table — the arguments of
        the ~40 clx_pack_weights calls — is built once per plan and lives on the device; it is rebuilt when a
        parameter's storage moves.  The sub-pixel layers' weight split runs first (its outputs are sources of
        jobs); layers whose weights need a copy (_pack_jobs) keep their calls."""
        from .._clx import ClxPackJob

        sig = (bool(need_dgrad),) + tuple(params[2 * layer.param_index].data_ptr() for layer in self.topo.convs)
        cache = getattr(self, "_pack_table", None)
        if cache is None or cache["sig"] != sig:
            table_jobs, singles, biggest = [], [], 1
            for layer, copy, jobs in self._pack_jobs(params, need_dgrad):
                if copy:
                    singles.append((layer, copy, jobs))
                    continue
                for src, dst, *rest in jobs:
                    table_jobs.append(ClxPackJob(src.data_ptr(), dst.data_ptr(), *rest))
                    biggest = max(biggest, pack_job_elements(*rest))
            table = None
            if table_jobs:
                arr = (ClxPackJob * len(table_jobs))(*table_jobs)
                host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
                table = host.to(self.device)
            cache = self._pack_table = dict(sig=sig, table=table, njobs=len(table_jobs), biggest=int(biggest),
                                            singles=singles)
        for layer in self.topo.convs:
            if layer.name in self.subpixel:
                self._sp_split(layer, self.subpixel[layer.name], params[2 * layer.param_index], st)
        if cache["table"] is not None:
            _clx.call("clx_pack_weights_batch", _clx.ptr(cache["table"]), cache["njobs"], cache["biggest"], st)
        for layer, copy, jobs in cache["singles"]:
            self._pack_one(layer, copy, jobs, params, st)

    def pack_weights(self, params, version, need_dgrad):
        """(Re)pack weights when the parameters changed (version = tuple of tensor versions)."""
        if need_dgrad and not self._bwd_ready:
            self._alloc_backward()
        if self._packed_version is not None and self._packed_version[0] == version and \
                (self._packed_version[1] or not need_dgrad):
            return
        st = _clx.stream_ptr(self.device)
        if os.environ.get("CLX_PACK_BATCH", "1") != "0":
            self._pack_batched(params, need_dgrad, st)
        else:
            for layer, copy, jobs in self._pack_jobs(params, need_dgrad):
                if layer.name in self.subpixel:
                    self._sp_split(layer, self.subpixel[layer.name], params[2 * layer.param_index], st)
                self._pack_one(layer, copy, jobs, params, st)
        self._split_wplanes(need_dgrad, st)
        self._packed_version = (version, need_dgrad)

    # ----------------------------------------------------------------- forward
    # ------------------------------------------------- changed rows of noisy copies (csrc/sparse_rows.hip)
    def pointwise_prefix(self):
        """(first convolution, [the 1x1 layers straight behind it]) if the forward order starts that way with plain
        launches — conv_pass.0 (k x k on the image), conv_pass.2, conv_pass.4 (1 x 1) of the first level — else None.
        These are the layers a noisy copy of an image shares with the clean image outside the window-dilated set of
        its noise pixels (UNetModel._forward_chunks)."""
        ops = self.topo.fwd_order
        if not ops or not isinstance(ops[0], ConvLayer):
            return None
        special = lambda op: op.name in self.chains or op.name in self.chain_second or op.name in self.subpixel
        first = ops[0]
        if special(first) or len(first.sources) != 1 or first.sources[0].tensor != "raw":
            return None
        # On the changed-rows path the copies' tensors between `first` and the LAST layer of the tail are never written
        # (only the last one is rebuilt by broadcast + scatter): every tensor in between must have the next layer of the
        # prefix as its ONLY reader — a topology in which one of them is also a skip connection or pooled would read
        # stale rows (today's build_topology never makes one; find_chain_pairs guards its pairs the same way)
        readers = tensor_consumers(self.topo)
        tail, src = [], first.out
        for op in ops[1:]:
            if not isinstance(op, ConvLayer) or op.taps != 1 or special(op) or self.algo[op.name]["fwd"]:
                break
            s = op.sources[0]
            if len(op.sources) != 1 or s.tensor != src or tuple(s.crop) != (0, 0, 0) or tuple(s.factor) != (1, 1, 1):
                break
            if readers.get(src, 0) != 1:
                break
            tail.append(op)
            src = op.out
        return (first, tail) if tail else None

    def first_layer_on_rows(self):
        """True if the first layer of pointwise_prefix can be computed for a list of output pixels by clx_grey_rows: a
        one-channel image under a 3 x 3 (x 3) kernel — the layers clx_conv_fwd gives to conv_grey_fwd_kernel."""
        prefix = self.pointwise_prefix()
        if prefix is None or os.environ.get("CLX_SPARSE_FIRST", "1") == "0":
            return False
        first = prefix[0]
        return (self.topo.in_channels == 1 and tuple(first.kernel) in ((1, 3, 3), (3, 3, 3)) and first.cout % 4 == 0
                and first.in_shape[0] >= first.kernel[0])

    def tiled_layer_behind_prefix(self):
        """The 2-D Winograd layer that reads the last 1x1 layer of pointwise_prefix (conv_pass.6 of the first level), or
        None: its output tiles can be computed for a list of tiles only (clx_conv_desc.tile_list)."""
        prefix = self.pointwise_prefix()
        if prefix is None:
            return None
        first, tail = prefix
        ops = self.topo.fwd_order
        k = 1 + len(tail)
        if k >= len(ops) or not isinstance(ops[k], ConvLayer):
            return None
        op = ops[k]
        code = self.algo[op.name]["fwd"]
        if (not code or op.kernel[0] != 1 or op.in_shape[0] != 1 or op.name in self.subpixel or op.name in self.chains
                or op.name in self.chain_second or len(op.sources) != 1):
            return None
        s = op.sources[0]
        if s.tensor != tail[-1].out or tuple(s.crop) != (0, 0, 0) or tuple(s.factor) != (1, 1, 1):
            return None
        return op, WINO_TILE[code]

    def _compact(self, slot, rows, width):
        """grow-only scratch for `rows` compact rows of `width` floats, ZEROED when made: the 1x1 layers write their real
        channels only, and the pad lanes are read by the next layer (times zero weights) and copied into the dense tensor
        by the scatter — left as the allocator's memory, a NaN there becomes NaN * 0 = NaN, which a ReLU turns into 0"""
        bufs = self.__dict__.setdefault("_compact_bufs", {})
        b = bufs.get(slot)
        if b is None or b.shape[0] < rows or b.shape[1] != width:
            b = bufs[slot] = _clx.zeros((max(rows, 1), width), torch.float32, self.device)
        return b

    def forward_prefix(self, raw, params, nlayers):
        """the first convolution and the `nlayers` layers behind it on `raw` -> the last one's output rows
        (B * pixels, padded channels), in this plan's buffer (a Winograd layer with a fused pooling also leaves the
        pooled tensor in its buffer)"""
        t = self.topo
        st = _clx.stream_ptr(self.device)
        npix_in = t.in_shape[0] * t.in_shape[1] * t.in_shape[2]
        raw = raw.contiguous()
        _clx.call("clx_planar_to_pixel", _clx.ptr(raw), _clx.ptr(self.buf["raw"]), self.B,
                  t.in_channels, npix_in, pad4(t.in_channels), st)
        for op in t.fwd_order[:1 + nlayers]:
            self._conv_forward(op, params, st)
        return self.buf[t.fwd_order[nlayers].out]

    def _conv_forward(self, op, params, st, tiles=None):
        """one plain convolution layer of the forward pass (tiles = (int32 tensor, count): a Winograd layer computes the
        listed output tiles only)"""
        d = self._desc(op, op.cout)
        self._set_wpack(d, self.wpack_fwd[op.name])
        b = params[2 * op.param_index + 1]
        d.bias = b.data_ptr() if b is not None else None
        d.relu = 1 if op.relu else 0
        d.out = self.buf[op.out].data_ptr()
        d.ld_out = pad4(op.cout)
        if op.relu and self.keep:
            self._set_gate_out(d, op.out)
        if self.sp_pass[op.name][0] and not self.algo[op.name]["fwd"]:
            xp = self.xplanes.get(op.name) if self.keep and self._bwd_ready and tiles is None else None
            d.aplanes = (xp if xp is not None else self.aplanes).data_ptr()
            if xp is not None:
                # (planes the layer before this one has already written in its epilogue: no split pass)
                d.aplanes_valid = 1 if op.name in self._xplanes_fresh else 0
                self._xplanes_fresh.add(op.name)
                # ... and this layer's epilogue writes the planes of the 1x1 layer that reads its output
                nxt = self._pointwise_reader.get(op.out)
                if nxt is not None and os.environ.get("CLX_SP_EPILOGUE_PLANES", "1") != "0":
                    d.out_planes = self.xplanes[nxt.name].data_ptr()
                    self._xplanes_fresh.add(nxt.name)
        if self.algo[op.name]["fwd"]:
            self._use_workspace(d, self.algo[op.name]["fwd"])
            if self.keep and self._bwd_ready and op.name in self.vcache:
                d.vcache = self.vcache[op.name].data_ptr()
                self._vcache_fresh.add(op.name)
            pool = self.fused_pool.get(op.name)
            if pool is not None:
                d.pool_out = self.buf[pool.out].data_ptr()
                d.ld_pool = pad4(pool.channels)
        if tiles is not None:
            d.tile_list = tiles[0].data_ptr()
            d.tile_count = int(tiles[1])
        _clx.call("clx_conv_fwd", ctypes.byref(d), st)

    def _tiles_forward(self, op, params, sparse, st):
        """The Winograd layer behind the 1x1 layers for a chunk of noisy copies: the clean image's output (and pooled
        output) under every copy, then the CHANGED tiles of each copy — those whose input window holds a changed row —
        through the transforms and the batched products (clx_conv_desc.tile_list).  A tile's output depends on its own
        input window alone: the dense computation's bits."""
        dense = self.buf[op.out]
        clean = sparse["clean_tile_rows"]
        assert clean.shape[1] == dense.shape[1] and clean.shape[0] * self.B == dense.shape[0]
        _clx.call("clx_broadcast_rows", _clx.ptr(clean), clean.numel(), _clx.ptr(dense), self.B, st)
        pool = self.fused_pool.get(op.name)
        if pool is not None:
            pooled, clean_pooled = self.buf[pool.out], sparse["clean_pool_rows"]
            assert clean_pooled.shape[0] * self.B == pooled.shape[0]
            _clx.call("clx_broadcast_rows", _clx.ptr(clean_pooled), clean_pooled.numel(), _clx.ptr(pooled), self.B, st)
        if int(sparse["ntiles"]) > 0:
            self._conv_forward(op, params, st, tiles=(sparse["tiles"], sparse["ntiles"]))

    def _pointwise_on_rows(self, tail, params, sparse, st):
        """The 1x1 layers `tail` for a chunk of noisy copies: once on the clean image (done by the caller: sparse
        ["clean_rows"]) and here on the copies' CHANGED rows — gathered from the first convolution's dense output, run
        through the layers as a (1, 1, n) image, scattered over the broadcast clean rows.  A row of a 1x1 layer depends on
        its own input row alone, so the tensor is the dense computation's, bit for bit."""
        n, rows = int(sparse["n"]), sparse["rows"]
        src = self.buf[tail[0].sources[0].tensor]
        width = src.shape[1]
        cur = None
        if n > 0:
            cur = self._compact(0, n, width)
            if sparse.get("noisy") is not None:
                # one-channel image: the first layer itself on the changed rows (clx_grey_rows: the dense kernel's
                # arithmetic) — the dense first-layer tensor of the copies is never written
                first = self.topo.fwd_order[0]
                b = params[2 * first.param_index + 1]
                _clx.call("clx_grey_rows", _clx.ptr(sparse["noisy"]), self.B, *first.in_shape, first.kernel[0],
                          _clx.ptr(rows), n, _clx.ptr(self.wpack_fwd[first.name]), _clx.ptr(b) if b is not None else None,
                          1 if first.relu else 0, first.cout, _clx.ptr(cur), width, st)
            else:
                _clx.call("clx_gather_rows", _clx.ptr(src), width, _clx.ptr(rows), n, width, _clx.ptr(cur), width, st)
            for k, op in enumerate(tail):
                y = self._compact(1 + k % 2, n, pad4(op.cout))
                d = conv_desc([conv_src(cur.data_ptr(), cur.shape[1], cur.shape[1], (1, 1, n))], 1, (1, 1, n), (1, 1, 1),
                              (0, 0, 0), op.cout, self.precision)
                self._set_wpack(d, self.wpack_fwd[op.name])
                if self.precision and self.aplanes is not None:       # (n <= the dense tensor's rows: the scratch fits)
                    d.aplanes = self.aplanes.data_ptr()
                b = params[2 * op.param_index + 1]
                d.bias = b.data_ptr() if b is not None else None
                d.relu = 1 if op.relu else 0
                d.out = y.data_ptr()
                d.ld_out = y.shape[1]
                _clx.call("clx_conv_fwd", ctypes.byref(d), st)
                cur = y
        dense = self.buf[tail[-1].out]
        clean = sparse["clean_rows"]
        assert clean.shape[1] == dense.shape[1] and clean.shape[0] * self.B == dense.shape[0]
        _clx.call("clx_broadcast_rows", _clx.ptr(clean), clean.numel(), _clx.ptr(dense), self.B, st)
        if n > 0:
            _clx.call("clx_scatter_rows", _clx.ptr(cur), cur.shape[1], _clx.ptr(rows), n, dense.shape[1],
                      _clx.ptr(dense), dense.shape[1], st)

    def forward(self, raw, params, out=None, on_op=None, sparse=None):
        """raw: (B, C, *spatial) f32 on device -> offsets (B, out_channels, *out_spatial), written into `out`
        (contiguous, that shape) when given.  on_op(i): called after the launches of the i-th operation of the forward
        order are enqueued (a second stream can be started behind a chosen point of this one).
        sparse: {"clean_rows", "rows", "n"} — the batch is noisy copies of ONE image whose pointwise prefix
        (pointwise_prefix) was computed on the clean image: the 1x1 layers run on the changed rows only."""
        t = self.topo
        st = _clx.stream_ptr(self.device)
        sparse_tail = self.pointwise_prefix()[1] if sparse is not None else None
        self._vcache_fresh = set()      # Winograd layers whose V this forward left in self.vcache
        self._xplanes_fresh = set()     # 1x1 layers whose input planes this forward left in self.xplanes
        npix_in = t.in_shape[0] * t.in_shape[1] * t.in_shape[2]
        raw = raw.contiguous()
        rows_only_first = sparse is not None and self.first_layer_on_rows()
        if rows_only_first:
            sparse = dict(sparse, noisy=raw)                # the first layer runs on the changed rows only
        else:
            _clx.call("clx_planar_to_pixel", _clx.ptr(raw), _clx.ptr(self.buf["raw"]), self.B,
                      t.in_channels, npix_in, pad4(t.in_channels), st)
        for op_index, op in enumerate(t.fwd_order):
            if on_op is not None and op_index > 0:
                on_op(op_index - 1)
            if op_index == 0 and rows_only_first:
                continue
            if isinstance(op, ConvLayer) and op.name in self.chain_second:
                continue                                    # computed with its predecessor
            if isinstance(op, ConvLayer) and op.name in self.chains:
                self._chain_forward(*self.chains[op.name], params, st)
            elif isinstance(op, ConvLayer) and op.name in self.subpixel:
                self._sp_forward(op, self.subpixel[op.name], params[2 * op.param_index + 1], st)
            elif isinstance(op, ConvLayer) and sparse_tail and op is sparse_tail[0]:
                self._pointwise_on_rows(sparse_tail, params, sparse, st)
            elif isinstance(op, ConvLayer) and sparse_tail and any(op is q for q in sparse_tail):
                continue                                    # computed with the first 1x1 layer of the prefix
            elif isinstance(op, ConvLayer) and sparse is not None and sparse.get("tiles") is not None \
                    and op is sparse["tile_op"]:
                self._tiles_forward(op, params, sparse, st)
            elif isinstance(op, ConvLayer):
                self._conv_forward(op, params, st)
            elif any(p is op for p in self.fused_pool.values()):
                continue                                    # written by the producing layer's output transform
            else:
                D, H, W = op.in_shape
                _clx.call("clx_maxpool_fwd", _clx.ptr(self.buf[op.src]), _clx.ptr(self.buf[op.out]),
                          self.B, D, H, W, pad4(op.channels), *op.factor, st)
        npix_out = t.out_shape[0] * t.out_shape[1] * t.out_shape[2]
        spatial = t.out_shape[3 - t.nd:]
        if out is None:
            out = torch.empty((self.B, t.out_channels) + tuple(spatial), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and tuple(out.shape) == (self.B, t.out_channels) + tuple(spatial)
        _clx.call("clx_pixel_to_planar", _clx.ptr(self.buf["h1"]), _clx.ptr(out), self.B,
                  t.out_channels, npix_out, pad4(t.out_channels), st)
        return out

    # ---------------------------------------------------------------- backward
    def backward(self, dout, params, grads, on_layer_done=None, flat_grad=None, dx=None):
        """dout: (B, out_channels, *out_spatial) gradient of the loss w.r.t. forward()'s result.
        grads: list aligned with params; every entry is OVERWRITTEN with the gradient.
        flat_grad: the flat buffer the entries of `grads` are views of, if there is one.
        on_layer_done(param_index): called once the kernels that write a layer's weight and bias
        gradient are enqueued (layers finish in reverse forward order: the data-parallel step
        starts reducing the tail of the flat gradient while the rest is still being computed).
        dx: contiguous float32 tensor shaped like raw, OVERWRITTEN with the gradient w.r.t. raw (first_dgrad); None: none."""
        st = _clx.stream_ptr(self.device)
        self.zero_gradients(grads, flat_grad)
        for done, unpack in self.backward_steps(dout, params, grads, dx=dx):
            unpack(st)
            if on_layer_done is not None:
                for i in done:
                    on_layer_done(i)

    def train_pass(self, raw, params, grads, flat_grad, loss_fn, after_loss=None, on_layer_done=None):
        """forward -> loss_fn(offsets, lo, hi) (enqueues the loss of crops lo..hi-1 on the current stream, returns the
        gradient w.r.t. those offsets) -> after_loss() -> backward.  Returns the offsets."""
        out = self.forward(raw, params)
        dout = loss_fn(out, 0, self.B)
        if after_loss is not None:
            after_loss()
        self.backward(dout, params, grads, on_layer_done=on_layer_done, flat_grad=flat_grad)
        return out

    def zero_gradients(self, grads, flat_grad=None):
        """The accumulators the backward kernels add into: packed weight gradients and bias gradients."""
        if flat_grad is not None:          # `grads` tile this buffer: ONE launch for both accumulators
            _clx.zero_many(self.dwpack, flat_grad)
        else:
            _clx.zero_many(self.dwpack)
            for g in grads[1::2]:
                if g is not None:
                    g.zero_()

    def first_dgrad(self, layer, dy, w, dx, st):
        """dx (planar, raw's shape) = the data gradient of the first convolution, from `dy` = gbuf[layer.out] (its
        pre-activation gradient, the ReLU gate applied by the consumer).  1-4 channels: clx_conv_first_dgrad straight from
        the torch weight; otherwise (or CLX_FIRST_DGRAD=0) the generic route every other layer takes — the data-gradient
        convolution (clx_conv_fwd with _dgrad_desc) into pixel-major scratch, then clx_pixel_to_planar.  That route's
        weight pack and scratch are made here, on first use, and packed on every call."""
        assert dx.is_contiguous() and dx.dtype == torch.float32 and dx.shape[0] == self.B
        wv = w.detach()
        if not wv.is_contiguous():
            wv = wv.contiguous()
        OD, OH, OW = layer.out_shape
        if _first_dgrad_kernel_wanted(layer):
            _clx.call("clx_conv_first_dgrad", _clx.ptr(dy), dy.shape[1], _clx.ptr(wv), layer.cout, layer.cin, self.B,
                      OD, OH, OW, layer.kernel[0], _clx.ptr(dx), st)
            return
        if not self.dx_bufs:
            n = self.B * layer.in_shape[0] * layer.in_shape[1] * layer.in_shape[2]
            self.dx_bufs["wpack"] = torch.empty(layer.cin_pad * layer.taps * pad4(layer.cout), dtype=torch.float32,
                                                device=self.device)
            self.dx_bufs["pixels"] = torch.empty((n, layer.cin_pad), dtype=torch.float32, device=self.device)
        wp, px = self.dx_bufs["wpack"], self.dx_bufs["pixels"]
        _clx.call("clx_pack_weights", _clx.ptr(wv), _clx.ptr(wp), layer.cout, layer.cin, layer.taps, layer.cin_pad,
                  pad4(layer.cout), 1, st)
        dd = self._dgrad_desc(layer, dy)
        dd.wpack = wp.data_ptr()
        dd.out = px.data_ptr()
        dd.ld_out = layer.cin_pad
        _clx.call("clx_conv_fwd", ctypes.byref(dd), st)
        _clx.call("clx_pixel_to_planar", _clx.ptr(px), _clx.ptr(dx), self.B, layer.cin,
                  layer.in_shape[0] * layer.in_shape[1] * layer.in_shape[2], layer.cin_pad, st)

    def backward_steps(self, dout, params, grads, dx=None):
        """The backward pass as a generator, one step per layer (or fused pair) in reverse order.  Each step
        enqueues the layer's weight/bias-gradient kernels — they ADD into self.dwpack and the bias gradients, which
        the caller has zeroed (zero_gradients) — and yields (param_indices, unpack): unpack(stream) enqueues the
        launches that turn the packed weight gradient of those layers into `grads`; the layer's data gradient is
        enqueued when the generator is resumed.  DualPlan drives two of these on two streams over one accumulator.
        dx: see backward; the first layer's data gradient is enqueued after its weight gradient."""
        t = self.topo
        st = _clx.stream_ptr(self.device)
        assert self._bwd_ready, "pack_weights(need_dgrad=True) must run before backward"
        npix_out = t.out_shape[0] * t.out_shape[1] * t.out_shape[2]
        dout = dout.contiguous()
        _clx.call("clx_planar_to_pixel", _clx.ptr(dout), _clx.ptr(self.gbuf["h1"]), self.B,
                  t.out_channels, npix_out, pad4(t.out_channels), st)

        pending_skip = {}   # skip tensor name -> (gradient buffer of its consumer's input, its row length, that layer)
        dy_planes_of = {}   # tensor name -> buffer that holds the P3 planes of its gradient (split precision)

        # reverse execution order; gbuf[x] holds dL/d(pre-activation of x)
        for op in reversed(t.fwd_order):
            if isinstance(op, PoolOp):
                continue  # handled when its consumer's data gradient is produced
            layer = op
            dy = self.gbuf[layer.out]
            if layer.name in self.chains:
                continue                                    # done with its successor
            if layer.name in self.chain_second:
                a, b = self.chain_second[layer.name]
                yield (b.param_index, a.param_index), self._chain_backward(a, b, self._conv_by_out[a.sources[0].tensor],
                                                                           grads, st)
            elif layer.name in self.subpixel:
                sp = self.subpixel[layer.name]
                yield (layer.param_index,), self._sp_wgrad(layer, sp, dy, grads[2 * layer.param_index],
                                                           grads[2 * layer.param_index + 1], st)
                dskip = self._sp_dgrad(layer, sp, dy, st)
                pending_skip[layer.sources[0].tensor] = (dskip, sp.skip.Cp, layer)
            else:
                unpack, dy_planes, dy_ready = self._layer_wgrad(layer, dy, grads, dy_planes_of, st)
                yield (layer.param_index,), unpack
                if layer.param_index > 0:
                    self._layer_dgrad(layer, dy, grads, dy_planes, dy_ready, dy_planes_of, pending_skip, st)
                elif dx is not None:
                    self.first_dgrad(layer, dy, params[0], dx, st)
        assert not pending_skip

    def _dy_dual(self, layer):
        """weight and data gradient of a Winograd layer from ONE transform of dY, kept in self.dycache?"""
        a = self.algo[layer.name]
        return bool(self.dycache is not None and a["wgrad"] and layer.param_index > 0 and a["dgrad"] == a["wgrad"]
                    and layer.name not in self.adjoint)

    def _layer_wgrad(self, layer, dy, grads, dy_planes_of, st):
        """weight + bias gradient of a plain layer -> (unpack(stream), dy_planes, dy_ready): the buffer for the P3 planes
        of dy (split precision) and whether it holds them now, for the layer's data gradient"""
        d = self._desc(layer, pad4(layer.cout))
        gb = grads[2 * layer.param_index + 1]
        off = self.dw_off[layer.name]
        wino_w = self.algo[layer.name]["wgrad"]
        dwp = self.dwpack[off:off + packed_taps(wino_w, layer.kernel) * pad4(layer.cout) * layer.cin_pad]
        if wino_w:
            self._use_workspace(d, wino_w)
            if layer.name in self.vcache and layer.name in self._vcache_fresh:
                d.vcache = self.vcache[layer.name].data_ptr()
                d.vcache_valid = 1
            if self._dy_dual(layer):
                d.dy_vcache = self.dycache.data_ptr()
        # split precision, 1x1 layers: the planes of this layer's dY — written by the epilogue of the data gradient that
        # produced dY (dy_planes_of, with the bias gradient as that epilogue's column sums), or split by the weight
        # gradient below — serve the weight gradient and the data gradient
        dy_planes = dy_planes_of.pop(layer.out, None)
        dy_ready = dy_planes is not None
        if dy_planes is None and self.dyplanes is not None:
            dy_planes = self.dyplanes
        if self.sp_pass[layer.name][2] and not wino_w:
            d.aplanes = self.xplanes[layer.name].data_ptr()
            d.aplanes_valid = 1 if layer.name in self._xplanes_fresh else 0
            d.dyplanes = dy_planes.data_ptr()
            d.dyplanes_valid = 1 if dy_ready else 0
            if dy_ready:
                gb = None                       # (the bias gradient is in already)
            dy_ready = True
        elif dy_ready:
            raise AssertionError("planes of dY were written for a layer whose weight gradient does not read them")
        self._wgrad(d, dy, pad4(layer.cout), dwp, gb, layer.cout, st)
        return self._unpack_step(layer, dwp, grads[2 * layer.param_index], wino_w), dy_planes, dy_ready

    def _layer_dgrad(self, layer, dy, grads, dy_planes, dy_ready, dy_planes_of, pending_skip, st):
        """data gradient of a plain layer (after _layer_wgrad, which leaves it the transformed dY or its planes), routed
        to what produced the layer's input: a concatenation, a pooling, or a convolution"""
        t = self.topo
        dd = self._dgrad_desc(layer, dy)
        self._set_wpack(dd, self.wpack_dgrad[layer.name])
        code = self.algo[layer.name]["dgrad"]
        dgrad_sp = self.sp_pass[layer.name][1] and not code
        if dgrad_sp:
            dd.aplanes = dy_planes.data_ptr()
            dd.aplanes_valid = 1 if dy_ready else 0          # (left by the weight gradient, or by the layer behind)
        if code:
            self._use_workspace(dd, code)
            if layer.name in self.adjoint:      # A dY A^T was left in the workspace by the weight-gradient call
                dd.adjoint = 1
            elif self._dy_dual(layer):          # V of dY was written by the weight-gradient call
                dd.vcache = self.dycache.data_ptr()
                dd.vcache_valid = 1
        s = layer.sources[0]
        pool = self._pool_by_out.get(s.tensor)
        if len(layer.sources) == 2:
            level = [i["level"] for i in t.r_info if i["conv0"] is layer][0]
            out, ld_out = self.gbuf["cat%d" % level], layer.cin_pad
        elif pool is not None:
            # input is a pooled tensor: dgrad -> gradient of the pool output (no gate),
            # then route through the max-pool, add the skip gradient, gate by ReLU.
            out, ld_out = self.gbuf[pool.out], pad4(pool.channels)
        else:
            prev = self._conv_by_out[s.tensor]
            out, ld_out = self.gbuf[prev.out], pad4(prev.cout)
            self._set_mask(dd, prev.out, relu=prev.relu)
            if (dgrad_sp and prev.name in self.xplanes and self.sp_pass[prev.name][2]
                    and os.environ.get("CLX_SP_EPILOGUE_PLANES", "1") != "0"):
                # the epilogue writes the planes of prev's dY and adds prev's bias gradient (its column sums): prev
                # is a split 1x1 layer (xplanes: not one of a fused pair) whose weight gradient reads those planes
                other = self.dyplanes2 if dy_planes is self.dyplanes else self.dyplanes
                dd.out_planes = other.data_ptr()
                gbp = grads[2 * prev.param_index + 1]
                dd.out_colsum = gbp.data_ptr() if gbp is not None else None
                dy_planes_of[prev.out] = other
        dd.out = out.data_ptr()
        dd.ld_out = ld_out
        _clx.call("clx_conv_fwd", ctypes.byref(dd), st)
        if len(layer.sources) == 2:
            skip_s, up_s = layer.sources
            # upsampled branch -> pre-activation gradient of the low-res tensor
            ushape, uc = t.shapes[up_s.tensor]
            LD, LH, LW = layer.in_shape
            _clx.call("clx_upsample_bwd", _clx.ptr(out), layer.cin_pad, pad4(skip_s.channels),
                      LD, LH, LW, *up_s.crop, _clx.ptr(self.buf[up_s.tensor]),
                      _clx.ptr(self.gbuf[up_s.tensor]), self.B, ushape[0], ushape[1], ushape[2],
                      pad4(uc), *up_s.factor, st)
            pending_skip[skip_s.tensor] = (out, layer.cin_pad, layer)
        elif pool is not None:
            cat, ld_cat, rl = pending_skip.pop(pool.src)
            skip_s = rl.sources[0]
            D, H, W = pool.in_shape
            SD, SH, SW = rl.in_shape
            _clx.call("clx_maxpool_bwd", _clx.ptr(self.buf[pool.src]), _clx.ptr(self.buf[pool.out]),
                      _clx.ptr(out), _clx.ptr(cat), ld_cat, SD, SH, SW,
                      *skip_s.crop, _clx.ptr(self.gbuf[pool.src]), self.B, D, H, W,
                      pad4(pool.channels), *pool.factor, st)


def _first_dgrad_kernel_wanted(layer):
    """clx_conv_first_dgrad for the input-image gradient of `layer` (the first convolution)?  1-4 input channels, unless
    CLX_FIRST_DGRAD=0 asks for the generic data-gradient convolution (A/B runs, tests)."""
    return layer.cin <= 4 and os.environ.get("CLX_FIRST_DGRAD", "1") != "0"


from .dual import DualPlan, dual_stream_wanted  # noqa: E402,F401  (dual.py imports UNetPlan from this module)
