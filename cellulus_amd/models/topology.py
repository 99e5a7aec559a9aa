"""Topology of the U-Net + head for one input crop shape: pure Python on shapes (no device, no library, no switch).

The topology is the one ``cellulus/models/unet.py:24-63`` requests from
``funlib.learn.torch.models.UNet`` (valid convolutions ``[3,1,1,3]`` + ReLU per
level, max-pool down, nearest ``constant_upsample`` up, centre-cropped skip
concatenated *before* the upsampled tensor) followed by the 1x1 head.  funlib
is not vendored in the reference; the restated rules (``crop_to_factor``,
channel counts, module names) are documented in SURVEY.md §3.4.
"""

import math
from dataclasses import dataclass, field
from typing import List, Tuple


def pad4(c: int) -> int:
    return (c + 3) // 4 * 4


@dataclass
class Source:
    """One input of a convolution: a stored tensor seen through crop/upsample."""

    tensor: str                      # buffer name
    channels: int                    # real channels
    crop: Tuple[int, int, int] = (0, 0, 0)
    factor: Tuple[int, int, int] = (1, 1, 1)


@dataclass
class ConvLayer:
    name: str                        # state_dict prefix, e.g. backbone.l_conv.0.conv_pass.0
    sources: List[Source]
    cout: int
    kernel: Tuple[int, int, int]     # (kd, kh, kw), kd = 1 for 2-D
    in_shape: Tuple[int, int, int]   # logical input extent (D, H, W)
    out: str                         # output buffer name
    relu: bool = True
    param_index: int = -1            # index into the flat (weight, bias) list

    @property
    def cin(self):
        return sum(s.channels for s in self.sources)

    @property
    def cin_pad(self):
        return sum(pad4(s.channels) for s in self.sources)

    @property
    def taps(self):
        return self.kernel[0] * self.kernel[1] * self.kernel[2]

    @property
    def out_shape(self):
        return tuple(i - k + 1 for i, k in zip(self.in_shape, self.kernel))


@dataclass
class PoolOp:
    src: str
    out: str
    channels: int
    in_shape: Tuple[int, int, int]
    factor: Tuple[int, int, int]


@dataclass
class Topology:
    """Static description of the network for one input crop shape."""

    nd: int
    in_channels: int
    out_channels: int
    in_shape: Tuple[int, int, int]
    convs: List[ConvLayer] = field(default_factory=list)
    pools: List[PoolOp] = field(default_factory=list)
    fwd_order: list = field(default_factory=list)      # ConvLayer | PoolOp in execution order
    shapes: dict = field(default_factory=dict)         # buffer -> ((D,H,W), channels)
    levels: int = 0
    # per r-level: (conv0 layer, skip tensor, up tensor)
    r_info: list = field(default_factory=list)
    out_shape: Tuple[int, int, int] = (1, 1, 1)


def build_topology(in_channels, out_channels, num_fmaps, fmap_inc_factor, features_in_last_layer,
                   downsampling_factors, num_spatial_dims, spatial):
    """Derives every layer's geometry for an input of spatial extent `spatial`."""
    nd = num_spatial_dims
    assert nd in (2, 3), "num_spatial_dims must be 2 or 3"
    assert len(spatial) == nd
    L = len(downsampling_factors)
    factors = []
    for f in downsampling_factors:
        f = tuple(int(a) for a in f)
        assert len(f) == nd, "downsampling factor rank must equal num_spatial_dims"
        factors.append((1,) + f if nd == 2 else f)
    shape = ((1,) + tuple(int(s) for s in spatial)) if nd == 2 else tuple(int(s) for s in spatial)
    k3 = (1, 3, 3) if nd == 2 else (3, 3, 3)
    k1 = (1, 1, 1)
    pass_kernels = [k3, k1, k1, k3]
    conv_crop = tuple(sum(k[d] - 1 for k in pass_kernels) for d in range(3))

    topo = Topology(nd=nd, in_channels=in_channels, out_channels=out_channels, in_shape=shape, levels=L)
    topo.shapes["raw"] = (shape, in_channels)

    def add_pass(prefix, first_sources, first_in_shape, cout, out_prefix):
        srcs, ishape = first_sources, first_in_shape
        layers = []
        for j, k in enumerate(pass_kernels):
            name = f"{prefix}.conv_pass.{2 * j}"
            out = f"{out_prefix}.{j}"
            layer = ConvLayer(name=name, sources=srcs, cout=cout, kernel=k, in_shape=ishape, out=out)
            for d in range(3):
                if layer.out_shape[d] <= 0:
                    raise ValueError(
                        f"input extent {spatial} is too small for the U-Net (layer {name} would be empty)")
            topo.convs.append(layer)
            topo.fwd_order.append(layer)
            topo.shapes[out] = (layer.out_shape, cout)
            layers.append(layer)
            srcs, ishape = [Source(out, cout)], layer.out_shape
        return layers

    # ---- left (contracting) path
    left_out = []
    cur, cur_c, cur_shape = "raw", in_channels, shape
    for i in range(L + 1):
        cout = num_fmaps * fmap_inc_factor ** i
        layers = add_pass(f"backbone.l_conv.{i}", [Source(cur, cur_c)], cur_shape, cout, f"l{i}")
        y, yshape = layers[-1].out, layers[-1].out_shape
        left_out.append((y, cout, yshape))
        if i < L:
            f = factors[i]
            for d in range(3):
                if yshape[d] % f[d] != 0:
                    raise RuntimeError(
                        f"Can not downsample shape {yshape[3 - nd:]} with factor {f[3 - nd:]}, "
                        f"mismatch in spatial dimension {d - (3 - nd)}")
            pshape = tuple(s // ff for s, ff in zip(yshape, f))
            pool = PoolOp(src=y, out=f"p{i}", channels=cout, in_shape=yshape, factor=f)
            topo.pools.append(pool)
            topo.fwd_order.append(pool)
            topo.shapes[pool.out] = (pshape, cout)
            cur, cur_c, cur_shape = pool.out, cout, pshape

    # ---- right (expanding) path, bottom-up
    crop_factors = []
    prod = None
    for f in factors[::-1]:
        prod = tuple(f) if prod is None else tuple(a * b for a, b in zip(f, prod))
        crop_factors.append(prod)
    crop_factors = crop_factors[::-1]

    below, below_c, below_shape = left_out[L]
    topo.r_info = [None] * L
    for i in range(L - 1, -1, -1):
        f = factors[i]
        up_shape = tuple(s * ff for s, ff in zip(below_shape, f))
        # crop_to_factor: keep (size - conv_crop) a multiple of the cumulative factor
        cf = crop_factors[i]
        target = tuple(int(math.floor((s - c) / ff)) * ff + c for s, c, ff in zip(up_shape, conv_crop, cf))
        for d in range(3):
            if target[d] <= conv_crop[d] and up_shape[d] != target[d]:
                raise RuntimeError(f"Feature map with shape {up_shape} is too small for cropping to factor")
        up_crop = tuple((s - t) // 2 for s, t in zip(up_shape, target))
        skip, skip_c, skip_shape = left_out[i]
        for d in range(3):
            if skip_shape[d] < target[d]:
                raise RuntimeError("skip connection smaller than the upsampled feature map")
        skip_crop = tuple((s - t) // 2 for s, t in zip(skip_shape, target))
        cout = features_in_last_layer if i == 0 else num_fmaps * fmap_inc_factor ** i
        srcs = [Source(skip, skip_c, crop=skip_crop),
                Source(below, below_c, crop=up_crop, factor=f)]
        layers = add_pass(f"backbone.r_conv.0.{i}", srcs, target, cout, f"r{i}")
        topo.r_info[i] = dict(conv0=layers[0], skip=skip, up=below, level=i)
        below, below_c, below_shape = layers[-1].out, cout, layers[-1].out_shape

    # ---- head: 1x1 conv + ReLU + 1x1 conv (unet.py:52-63)
    top, top_c, top_shape = below, below_c, below_shape
    if L > 0 and top_c != features_in_last_layer:
        raise AssertionError("internal: top level width mismatch")
    h0 = ConvLayer(name="head.0", sources=[Source(top, top_c)], cout=features_in_last_layer,
                   kernel=k1, in_shape=top_shape, out="h0", relu=True)
    h1 = ConvLayer(name="head.2", sources=[Source("h0", features_in_last_layer)], cout=out_channels,
                   kernel=k1, in_shape=top_shape, out="h1", relu=False)
    if L == 0 and top_c != features_in_last_layer:
        # funlib keeps num_fmaps at level 0 when there is no upsampling path; the
        # reference head then expects features_in_last_layer inputs (a config error).
        raise ValueError("with no downsampling, num_fmaps must equal features_in_last_layer")
    for layer in (h0, h1):
        topo.convs.append(layer)
        topo.fwd_order.append(layer)
        topo.shapes[layer.out] = (layer.out_shape, layer.cout)
    topo.out_shape = top_shape
    for idx, layer in enumerate(topo.convs):
        layer.param_index = idx
    return topo


def tensor_consumers(topo):
    """How many operations READ each stored tensor: every source of every convolution (skip connections and
    upsampled tensors are sources of a level's first convolution) and every pooling."""
    n = {}
    for layer in topo.convs:
        for src in layer.sources:
            n[src.tensor] = n.get(src.tensor, 0) + 1
    for pool in topo.pools:
        n[pool.src] = n.get(pool.src, 0) + 1
    return n


def find_chain_pairs(topo, algo_fwd, batch):
    """The (a, b) pairs of consecutive 64-channel 1x1 layers that may run as one launch each way.

    The fused backward pass OVERWRITES the gradient of the pair's input and never writes the gradient of the
    middle tensor (and neither tensor gets ReLU gate bits), so a pair qualifies only if the middle tensor is read
    by `b` alone and the pair's input by `a` alone: a tensor that is also a skip connection, pooled, or read by a
    second convolution keeps the layer-by-layer path, where gradients add up."""
    produced_by_conv = {layer.out: layer for layer in topo.convs}
    readers = tensor_consumers(topo)
    one = (1, 1, 1)
    plain = lambda s: tuple(s.crop) == (0, 0, 0) and tuple(s.factor) == (1, 1, 1)       # noqa: E731
    pairs = []
    i = 0
    while i + 1 < len(topo.convs):
        a, b = topo.convs[i], topo.convs[i + 1]
        ok = (tuple(a.kernel) == one and tuple(b.kernel) == one and len(a.sources) == 1 and len(b.sources) == 1
              and plain(a.sources[0]) and plain(b.sources[0]) and b.sources[0].tensor == a.out
              and a.sources[0].tensor in produced_by_conv and a.sources[0].channels == 64 and a.cout == 64
              and a.relu and (b.cout == 64 or b.cout <= 8)
              and readers.get(a.out, 0) == 1 and readers.get(a.sources[0].tensor, 0) == 1
              and not algo_fwd[a.name] and not algo_fwd[b.name]
              and batch * a.in_shape[0] * a.in_shape[1] * a.in_shape[2] < (1 << 31) - 256)
        if ok:
            pairs.append((a, b))
            i += 2
        else:
            i += 1
    return pairs


def forward_flops(topo, batch):
    """2 M N K over the convolutions of one forward pass (direct form)."""
    total = 0
    for layer in topo.convs:
        m = batch * layer.out_shape[0] * layer.out_shape[1] * layer.out_shape[2]
        total += 2 * m * layer.cout * layer.cin * layer.taps
    return total
