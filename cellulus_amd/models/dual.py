"""A training batch as two half batches on two HIP streams."""

import os

import torch

from .. import _clx
from .plan import UNetPlan          # (plan.py re-exports DualPlan below its class: it is imported first)
from .topology import forward_flops


class _Rows:
    """Read-only view of a per-tensor buffer dict of the two halves as full-batch tensors (rows are pixels,
    batch-major: the halves concatenate)."""

    def __init__(self, parts, attr):
        self._parts, self._attr = parts, attr

    def __getitem__(self, name):
        return torch.cat([getattr(p, self._attr)[name] for p in self._parts], dim=0)

    def __contains__(self, name):
        return name in getattr(self._parts[0], self._attr)

    def __bool__(self):
        return bool(getattr(self._parts[0], self._attr))

    def get(self, name, default=None):
        return self[name] if name in self else default

    def keys(self):
        return getattr(self._parts[0], self._attr).keys()


def dual_stream_wanted(topo, batch, keep_activations):
    """Two half batches on two streams (DualPlan)?  Training plans with an even batch whose halves are big enough
    to fill the device (CLX_STREAMS_MIN_GFLOP per half-batch forward pass, default 100: below that the step is
    launch-bound and twice the launches cost more than the overlap returns); never in reproducible mode.
    CLX_STREAMS=1 switches it off."""
    if not keep_activations or batch < 2 or batch % 2 or os.environ.get("CLX_STREAMS", "2") == "1":
        return False
    if os.environ.get("CLX_DETERMINISTIC", "0") == "1":
        return False
    return forward_flops(topo, batch // 2) >= float(os.environ.get("CLX_STREAMS_MIN_GFLOP", "100")) * 1e9


class DualPlan:
    """A training batch as two half batches on two HIP streams.

    A step is a strict chain of launches, each either bound by the matrix cores (the GEMMs) or by HBM (Winograd
    transforms, pooling, fills, the first layer): on one stream the two kinds never overlap.  Two independent half
    batches do — the transforms of one half run under the GEMMs of the other, and the partial last round of one
    half's tiles is filled by the other's.  Both halves use ONE set of packed weights and add their weight and bias
    gradients into ONE set of accumulators (the kernels add with atomics anyway); a layer's packed gradient is
    unpacked on the caller's stream once both halves have passed that layer, which is also when on_layer_done
    fires — the data-parallel buckets leave exactly as they do with one stream.
    Same interface as UNetPlan (pack_weights / forward / backward); CLX_STREAMS=1 keeps one stream."""

    def __init__(self, topo, batch, device, keep_activations):
        assert batch % 2 == 0 and keep_activations
        self.topo, self.B, self.device, self.keep = topo, int(batch), device, True
        self.parts = [UNetPlan(topo, batch // 2, device, True) for _ in range(2)]
        self.streams = [torch.cuda.Stream(device=device) for _ in range(2)]
        self._events = [[], [], []]
        self._shared = False
        self.buf = _Rows(self.parts, "buf")

    def __getattr__(self, name):            # algo, chains, subpixel, gate, ... : the halves agree
        if name in ("parts", "streams"):
            raise AttributeError(name)
        if name == "gbuf":
            return _Rows(self.parts, "gbuf")
        return getattr(self.parts[0], name)

    def pack_weights(self, params, version, need_dgrad):
        a, b = self.parts
        a.pack_weights(params, version, need_dgrad)
        if need_dgrad and not self._shared:
            b._alloc_backward()
            b.share_from(a)
            self._shared = True
        b._packed_version = a._packed_version

    def _fork(self):
        main = torch.cuda.current_stream(self.device)
        for s in self.streams:
            s.wait_stream(main)
        return main

    def _join(self, main):
        for s in self.streams:
            main.wait_stream(s)

    def forward(self, raw, params, out=None):
        t = self.topo
        assert self._shared, "pack_weights(need_dgrad=True) must run before forward"
        raw = raw.contiguous()
        if out is None:
            out = torch.empty((self.B, t.out_channels) + tuple(t.out_shape[3 - t.nd:]), dtype=torch.float32,
                              device=self.device)
        h = self.B // 2
        main = self._fork()
        for i, (p, s) in enumerate(zip(self.parts, self.streams)):
            with torch.cuda.stream(s):
                p.forward(raw[i * h:(i + 1) * h], params, out=out[i * h:(i + 1) * h])
        self._join(main)
        return out

    def _event(self, i, k):
        ev = self._events[i]
        while len(ev) <= k:
            ev.append(torch.cuda.Event())
        return ev[k]

    def backward(self, dout, params, grads, on_layer_done=None, flat_grad=None, dx=None):
        dout = dout.contiguous()
        h = self.B // 2
        self.parts[0].zero_gradients(grads, flat_grad)           # the one set of accumulators, on the caller's stream
        main = self._fork()
        # (dx is allocated on the caller's stream before the fork; each half writes its slice on its own stream and the
        #  join orders both behind the caller)
        dxs = [dx[:h], dx[h:]] if dx is not None else [None, None]
        self._backward_halves([dout[:h], dout[h:]], params, grads, on_layer_done, main, dxs=dxs)
        self._join(main)

    def train_pass(self, raw, params, grads, flat_grad, loss_fn, after_loss=None, on_layer_done=None):
        """UNetPlan.train_pass with each half's loss on its own stream (no join between the forward and the backward
        pass); the accumulators are zeroed on the caller's stream while the halves run their forward passes."""
        t = self.topo
        assert self._shared, "pack_weights(need_dgrad=True) must run before train_pass"
        raw = raw.contiguous()
        out = torch.empty((self.B, t.out_channels) + tuple(t.out_shape[3 - t.nd:]), dtype=torch.float32,
                          device=self.device)
        h = self.B // 2
        main = self._fork()
        douts = []
        # (starting the second half behind operation 0 .. 8 of the first — which gains 1.5-3 % on the inference chunks,
        #  models/unet.py — LOSES 0.3-3 % here, round 4: the step ends at a join and the delay is not recovered)
        for i, (p, s) in enumerate(zip(self.parts, self.streams)):
            with torch.cuda.stream(s):
                o = p.forward(raw[i * h:(i + 1) * h], params, out=out[i * h:(i + 1) * h])
                douts.append(loss_fn(o, i * h, (i + 1) * h))
                self._event(i, 0).record(s)
        self.parts[0].zero_gradients(grads, flat_grad)
        zeroed = self._event(2, 0)
        zeroed.record(main)
        for i, s in enumerate(self.streams):
            main.wait_event(self._event(i, 0))
            s.wait_event(zeroed)
        if after_loss is not None:
            after_loss()
        self._backward_halves(douts, params, grads, on_layer_done, main)
        self._join(main)
        return out

    def _backward_halves(self, douts, params, grads, on_layer_done, main, dxs=(None, None)):
        st_main = _clx.stream_ptr(self.device)
        gens = []
        for p, s, d, dx in zip(self.parts, self.streams, douts, dxs):
            with torch.cuda.stream(s):
                gens.append(p.backward_steps(d, params, grads, dx=dx))
        k = 1
        while True:
            items = []
            for i, (g, s) in enumerate(zip(gens, self.streams)):
                with torch.cuda.stream(s):
                    item = next(g, None)
                    if item is not None:
                        self._event(i, k).record(s)
                items.append(item)
            if items[0] is None:
                assert items[1] is None
                break
            assert items[1] is not None and items[0][0] == items[1][0]
            for i in range(2):
                main.wait_event(self._event(i, k))
            done, unpack = items[0]                  # (the halves share the accumulators: either closure does)
            unpack(st_main)
            if on_layer_done is not None:
                for idx in done:
                    on_layer_done(idx)
            k += 1
