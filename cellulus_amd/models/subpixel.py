"""Sub-pixel form of a convolution over cat(skip, nearest-upsample(low)): when it applies, the records a
plan keeps of it, and the algebra of its weights in torch ops."""

import os
from dataclasses import dataclass
from typing import Tuple

import torch

from .topology import pad4


@dataclass(eq=False)
class SubpixelHalf:
    """One of the two convolutions a sub-pixel layer runs as — 3x3 over the skip tensor, 2x2 over the low-resolution
    tensor — as allocation, packing, the weight gradient and the sharing between plans see it: weights (rows, C, taps),
    packed as (rows_pad, packed_taps, Cp)."""

    rows: int                        # output channels of the weights ...
    rows_pad: int                    # ... and of their packed form
    C: int                           # input channels, and padded
    Cp: int
    kernel: Tuple[int, int, int]
    wino: int = 0                    # algorithm code of the forward pass and the weight gradient ...
    wino_dgrad: int = 0              # ... and of the data gradient
    fused: bool = False              # forward pass in the one-launch form (wino_fused.hip)
    planes_fwd: bool = False         # the split-precision products read P3 planes of wp_fwd / of wp_dgrad
    planes_dgrad: bool = False
    vcache_bytes: int = 0            # size of vcache (0: the forward pass keeps no transformed input)
    w: torch.Tensor = None           # weights (written by clx_subpixel_split_weights)
    wp_fwd: torch.Tensor = None      # packed for the forward pass / for the data gradient
    wp_dgrad: torch.Tensor = None
    dw: torch.Tensor = None          # packed weight gradient: a slice of the plan's dwpack
    g: torch.Tensor = None           # weight gradient, unpacked (read by clx_subpixel_fold_grads)
    vcache: torch.Tensor = None      # transformed input, kept by the forward pass for the weight gradient ...
    v_fresh: bool = False            # ... and written by the last forward pass

    @property
    def taps(self):
        return self.kernel[0] * self.kernel[1] * self.kernel[2]


@dataclass(eq=False)
class Subpixel:
    """Geometry of the sub-pixel form of a convolution over cat(skip, nearest-upsample(low)) (subpixel_geometry)."""

    fac: Tuple[int, int, int]        # upsampling factor, P = its product: the phases
    P: int
    N: int                           # padded output channels of the layer; the low half computes P * N
    zshape: Tuple[int, int, int]     # extent of the low half's output Z, stored in buf[zname]
    zname: str
    level: int
    skip: SubpixelHalf
    low: SubpixelHalf

    @property
    def halves(self):
        return self.skip, self.low


def subpixel_geometry(topo, layer):
    """A convolution over cat(skip, nearest-upsample(low)) equals, exactly,
         conv(skip) + depth_to_space( conv_{2^d taps}(low, phase-summed weights) )
    because the k=3 taps of an output pixel with parity a fall on only two low-res rows.
    Returns the geometry of that rewrite or None when it does not apply (odd crop, odd
    output extent, cropped low-res grid, CLX_SUBPIXEL=0)."""
    if os.environ.get("CLX_SUBPIXEL", "1") == "0" or len(layer.sources) != 2:
        return None
    skip_s, up_s = layer.sources
    f, k, o = up_s.factor, layer.kernel, up_s.crop
    if max(f) != 2 or min(f) < 1 or skip_s.factor != (1, 1, 1):
        return None
    low_shape, low_c = topo.shapes[up_s.tensor]
    zshape, zk, zcrop = [], [], []
    for d in range(3):
        if f[d] == 2:
            if k[d] != 3 or o[d] % 2 != 0 or layer.out_shape[d] % 2 != 0:
                return None
            zshape.append(layer.out_shape[d] // 2)
            zk.append(2)
            zcrop.append(o[d] // 2)
        else:
            zshape.append(layer.out_shape[d])
            zk.append(k[d])
            zcrop.append(o[d])
        # the Z convolution must read the WHOLE low-res grid (its dgrad writes all of it)
        if zcrop[d] != 0 or zshape[d] + zk[d] - 1 != low_shape[d]:
            return None
    level = [i["level"] for i in topo.r_info if i["conv0"] is layer][0]
    P, N = f[0] * f[1] * f[2], pad4(layer.cout)
    return Subpixel(fac=f, P=P, N=N, zshape=tuple(zshape), zname="Z%d" % level, level=level,
                    skip=SubpixelHalf(rows=layer.cout, rows_pad=N, C=skip_s.channels, Cp=pad4(skip_s.channels),
                                      kernel=tuple(layer.kernel)),
                    low=SubpixelHalf(rows=P * N, rows_pad=P * N, C=up_s.channels, Cp=pad4(up_s.channels),
                                     kernel=tuple(zk)))


def phase_sum(w, axis, a):
    """3 taps -> 2 taps along `axis` for output parity `a`: the taps that land on the same
    low-res row are summed (a = 0: {0,1},{2};  a = 1: {0},{1,2}).  Elementwise torch ops."""
    t0, t1, t2 = w.select(axis, 0), w.select(axis, 1), w.select(axis, 2)
    pair = (t0 + t1, t2) if a == 0 else (t0, t1 + t2)
    return torch.stack(pair, dim=axis)


def phase_spread(g, axis, a):
    """adjoint of phase_sum: 2 taps -> 3 taps."""
    g0, g1 = g.select(axis, 0), g.select(axis, 1)
    trip = (g0, g0, g1) if a == 0 else (g0, g1, g1)
    return torch.stack(trip, dim=axis)


def phase_weights(layer, sp, w_up):
    """w_up (cout, C1, kd, kh, kw) -> phase-summed (P*N, C1, zkd, zkh, zkw); rows of padded
    output channels are zero.  Tiny tensors: plain elementwise torch ops.  (The statement of the algebra the tests
    check clx_subpixel_split_weights against, not a launch path: `sp` is any mapping with fac, P, N, C1 and zk.)"""
    f, N, cout = sp["fac"], sp["N"], layer.cout
    out = w_up.new_zeros((sp["P"], N, sp["C1"]) + sp["zk"])
    for a in range(f[0]):
        for b in range(f[1]):
            for c in range(f[2]):
                v = w_up
                for axis, (ff, par) in enumerate(zip(f, (a, b, c))):
                    if ff == 2:
                        v = phase_sum(v, 2 + axis, par)
                out[(a * f[1] + b) * f[2] + c, :cout] = v
    return out.reshape((sp["P"] * N, sp["C1"]) + sp["zk"])


def fold_phase_grads(layer, sp, dweff):
    """adjoint of phase_weights: (P*N, C1, zk...) -> (cout, C1, kd, kh, kw)."""
    f, N, cout = sp["fac"], sp["N"], layer.cout
    g = dweff.reshape((sp["P"], N, sp["C1"]) + sp["zk"])
    out = dweff.new_zeros((cout, sp["C1"]) + tuple(layer.kernel))
    for a in range(f[0]):
        for b in range(f[1]):
            for c in range(f[2]):
                v = g[(a * f[1] + b) * f[2] + c, :cout]
                for axis, (ff, par) in enumerate(zip(f, (a, b, c))):
                    if ff == 2:
                        v = phase_spread(v, 2 + axis, par)
                out += v
    return out
