"""The convolutions over <= 4 input channels (csrc/conv_smallc.hip: the first layer of every network, raw image ->
num_fmaps, and its weight gradient) through clx_conv_fwd / clx_conv_wgrad with hand-filled descriptors, against float64
torch on the CPU: the generic family conv_smallc_fwd_kernel<4..64> / conv_smallc_wgrad_stream_kernel<4..64> and the
grey-scale family conv_grey_fwd_kernel<1|3> / conv_grey_wgrad_kernel<1|3>, plus the descriptors over 4 channels that the
small-channel kernels must leave to the implicit-GEMM kernel.

Primary comparison: EXACT.  Operands are small integers (image in {1..4} on the real channels, weights and bias in
{-8..8}; for the weight gradient dy in {-2..2} and the image in {0..3}), so every partial sum stays far below 2^24
(forward: <= 4 * 27 * 4 * 8 + 8 = 3464; weight gradient: <= 6 * M + prefill, asserted per case) and float32 FMAs and
float atomics are exact in any order: torch.equal with the float64 result.  Secondary: one real-valued case per kernel
family under bars derived from float32 rounding alone (stated where they are used).

Conventions of test_gpu_glue.py: outputs are prefilled with NaN and lanes [N, ld) must still be NaN; lanes [4, ld_x) of
the image, lanes [N, ld_dy) of dy and every stored pixel outside the cropped logical window hold NaN and must never reach
a result (the grey kernels clamp their dead loads into the window instead of predicating them: this pins that).

Which kernel ran: the profile counters count implicit-GEMM launches (kinds 0, 1: forward; 2: weight gradient) — 0 on
the small-channel routes, >= 1 on the fallback routes; grey versus generic is observed in
test_dispatch_between_grey_and_generic_kernels.

Replaces nn.Conv{2,3}d(in_channels -> num_fmaps, 3) of l_conv.0.conv_pass.0 (cellulus/models/unet.py:24-51) and its
autograd weight / bias gradient.  Not covered here: det_turns (the reproducible weight gradient is another kernel with
its own end-to-end test), clx_conv_first_dgrad and clx_grey_rows (own tests).
"""
import ctypes
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 2.0 ** -24


def _clx():
    from cellulus_amd import _clx

    return _clx


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).float()


def _nan(device, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=device)


def _pad4(n):
    return (n + 3) // 4 * 4


@contextmanager
def _igemm_launches():
    """launches of the implicit-GEMM kernels inside the block: {"fwd": kinds 0 + 1, "wgrad": kind 2}"""
    c = _clx()
    c.call("clx_profile_enable", 2)
    counts = {}
    try:
        yield counts
        got = []
        for k in (0, 1, 2):
            n, ms, fl = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            c.check(c.load().clx_profile_read(k, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)), "clx_profile_read")
            got.append(int(n.value))
        counts["fwd"], counts["wgrad"] = got[0] + got[1], got[2]
    finally:
        c.call("clx_profile_enable", 0)


def _case(B=2, I=(1, 13, 19), K=(1, 3, 3), P=(0, 0, 0), cin=3, N=4, c_real=0, stored=None, crop=(0, 0, 0), ld_x=4,
          extra=0, bias=True, relu=True, dbias=True, seed=0):
    """I: logical input extent; stored: extent of the stored grid (default: I) in which the logical window starts at
    crop; extra: lanes of out / dy past pad4(N)."""
    O = tuple(i + 2 * p - k + 1 for i, p, k in zip(I, P, K))
    return SimpleNamespace(B=B, I=I, K=K, P=P, cin=cin, N=N, c_real=c_real, stored=stored or I, crop=crop, ld_x=ld_x,
                           ld=_pad4(N) + extra, bias=bias, relu=relu, dbias=dbias, seed=seed, O=O,
                           M=B * O[0] * O[1] * O[2], taps=K[0] * K[1] * K[2])


def _id(c):
    s = "b%d_i%dx%dx%d_k%d%d%d_p%d%d%d_c%d_n%d_r%d" % ((c.B,) + c.I + c.K + c.P + (c.cin, c.N, c.c_real))
    if c.stored != c.I:
        s += "_crop"
    if c.ld != _pad4(c.N):
        s += "_ld%d" % c.ld
    if not c.bias:
        s += "_plain"
    if not c.dbias:
        s += "_nodb"
    return s + "_s%d" % c.seed


def _image(c, real):
    """real (B, ID, IH, IW, cin or 4) -> (stored grid (B, D, H, W, ld_x): NaN outside the logical window and in lanes
    [4, ld_x), zero in the channel slots past the real ones; the window's four slots in float64)."""
    win = torch.zeros(c.B, *c.I, 4)
    win[..., : real.shape[-1]] = real
    x = torch.full((c.B, *c.stored, c.ld_x), NAN)
    (oz, oy, ox), (d, h, w) = c.crop, c.I
    x[:, oz:oz + d, oy:oy + h, ox:ox + w, :4] = win
    return x, win.double()


def _desc(c, x_dev):
    C = _clx()
    d = C.ClxConvDesc()
    d.nsrc = 1
    s = d.src[0]
    s.ptr, s.C, s.ld = x_dev.data_ptr(), 4, c.ld_x
    s.D, s.H, s.W = c.stored
    s.oz, s.oy, s.ox = c.crop
    s.fz = s.fy = s.fx = 1
    d.B = c.B
    d.ID, d.IH, d.IW = c.I
    d.KD, d.KH, d.KW = c.K
    d.PD, d.PH, d.PW = c.P
    d.N = c.N
    d.c_real = c.c_real
    d.algo = 0
    d.precision = 0
    return d


def _pack(w, device):
    """w (N, cin, KD, KH, KW) -> wpack [N][taps][4] by clx_pack_weights(CLX_PACK_FWD, cin_pad = 4): N rows, all written"""
    C = _clx()
    N, cin = w.shape[:2]
    taps = w[0, 0].numel()
    w_d = w.reshape(N, cin, taps).contiguous().to(device)
    wp = _nan(device, N * taps * 4)
    C.call("clx_pack_weights", C.ptr(w_d), C.ptr(wp), N, cin, taps, 4, _pad4(N), 0, C.stream_ptr(device))
    return wp


def _conv_ref(c, win, w, b):
    """float64 convolution of the window's first w.shape[1] slots: (M, N)"""
    r = F.conv3d(win[..., : w.shape[1]].permute(0, 4, 1, 2, 3), w.double(), None if b is None else b.double(), padding=c.P)
    r = r.permute(0, 2, 3, 4, 1).reshape(c.M, c.N)
    return r.clamp_min(0) if c.relu else r


def _run_fwd(c, device, x, wp, b_dev, igemm=False, prefill=None, **fields):
    """clx_conv_fwd of case c: the (M, ld) output on the host.  fields: further descriptor fields (tensors by pointer)."""
    C = _clx()
    x_d = x.to(device)
    out = _nan(device, c.M, c.ld)
    if prefill is not None:
        out[:, : c.N] = prefill.to(device)
    d = _desc(c, x_d)
    d.wpack, d.out, d.ld_out, d.relu = wp.data_ptr(), out.data_ptr(), c.ld, int(c.relu)
    d.bias = b_dev if isinstance(b_dev, int) else (b_dev.data_ptr() if b_dev is not None else None)
    for k, v in fields.items():
        setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
    with _igemm_launches() as n:
        C.call("clx_conv_fwd", ctypes.byref(d), C.stream_ptr(device))
    if igemm:
        assert n["fwd"] >= 1 and n["wgrad"] == 0, n
    else:
        assert n == {"fwd": 0, "wgrad": 0}, n
    return out.cpu()


def _check_out(out, ref, N):
    assert torch.equal(out[:, :N].double(), ref)
    assert torch.isnan(out[:, N:]).all()


def _fwd_exact(c, device):
    assert c.M < 2 ** 31 and 4 * c.taps * 4 * 8 + 8 < 2 ** 24
    x, win = _image(c, _ints((c.B, *c.I, c.cin), 1, 4, c.seed))
    w = _ints((c.N, c.cin, *c.K), -8, 8, c.seed + 1)
    b = _ints((c.N,), -8, 8, c.seed + 2) if c.bias else None
    out = _run_fwd(c, device, x, _pack(w, device), None if b is None else b.to(device))
    _check_out(out, _conv_ref(c, win, w, b), c.N)


def _fwd_real(c, device):
    """|got - ref| <= (4 * taps + 1) * 2^-24 * (conv(|x|, |w|) + |b|) elementwise: a float32 sum of 4 * taps products and
    the bias, in any order and with or without fused multiply-adds, is within (terms) * 2^-24 of the exact value relative
    to the sum of the terms' magnitudes (each product rounds once or not at all, each of the 4 * taps additions once);
    ReLU does not widen a difference.  A dropped tap misses by a whole term: hundreds to ten thousands of times the bar."""
    x, win = _image(c, torch.rand((c.B, *c.I, c.cin), generator=_gen(c.seed)))
    w = torch.randn((c.N, c.cin, *c.K), generator=_gen(c.seed + 1))
    b = torch.randn((c.N,), generator=_gen(c.seed + 2))
    out = _run_fwd(c, device, x, _pack(w, device), b.to(device))
    ref = _conv_ref(c, win, w, b)
    plain = SimpleNamespace(**{**vars(c), "relu": False})
    bar = (4 * c.taps + 1) * EPS * _conv_ref(plain, win.abs(), w.abs(), b.abs())
    err = (out[:, : c.N].double() - ref).abs()
    print("forward %s: max err / bar = %.3g" % (_id(c), (err / bar).max().item()))
    assert (err <= bar).all()
    assert torch.isnan(out[:, c.N:]).all()


def _wgrad_ref(c, win, dy):
    """float64 einsum per tap over the shifted windows of the zero-padded image: ([taps][N][4], [N])"""
    pd, ph, pw = c.P
    xp = F.pad(win, (0, 0, pw, pw, ph, ph, pd, pd))
    dyv = dy.double().view(c.B, *c.O, c.N)
    od, oh, ow = c.O
    g = torch.stack([torch.einsum("bdhwc,bdhwn->nc", xp[:, tz:tz + od, ty:ty + oh, tx:tx + ow], dyv)
                     for tz in range(c.K[0]) for ty in range(c.K[1]) for tx in range(c.K[2])])
    return g, dyv.sum((0, 1, 2, 3))


def _run_wgrad(c, device, x, dy, dw0, db0, igemm=False):
    """clx_conv_wgrad of case c into dwpack / dbias prefilled with dw0 / db0: (dwpack [taps][N][4], dbias or None)"""
    C = _clx()
    x_d = x.to(device)
    dy_d = _nan(device, c.M, c.ld)
    dy_d[:, : c.N] = dy.to(device)
    dw = dw0.to(device).contiguous()
    db = db0.to(device).contiguous() if db0 is not None else None
    d = _desc(c, x_d)
    with _igemm_launches() as n:
        C.call("clx_conv_wgrad", ctypes.byref(d), C.ptr(dy_d), c.ld, C.ptr(dw), C.ptr(db), C.stream_ptr(device))
    if igemm:
        assert n["wgrad"] >= 1 and n["fwd"] == 0, n
    else:
        assert n == {"fwd": 0, "wgrad": 0}, n
    return dw.cpu(), None if db is None else db.cpu()


def _wgrad_exact(c, device, x_hi=3, dy_hi=2):
    """accumulation included: dwpack and dbias are prefilled with integers, the result is prefill + gradient, exactly.
    Slots [cin, 4) of the image are zero, so their gradient is zero and they keep their prefill — on the grey route
    because the kernel leaves them alone, on the generic one because it adds 0."""
    assert c.N % 4 == 0 and x_hi * dy_hi * c.M + 3 < 2 ** 24
    x, win = _image(c, _ints((c.B, *c.I, c.cin), 0, x_hi, c.seed))
    dy = _ints((c.M, c.N), -dy_hi, dy_hi, c.seed + 1)
    dw0 = _ints((c.taps, c.N, 4), -3, 3, c.seed + 2)
    db0 = _ints((c.N,), -3, 3, c.seed + 3) if c.dbias else None
    dw, db = _run_wgrad(c, device, x, dy, dw0, db0)
    g, gb = _wgrad_ref(c, win, dy)
    assert torch.equal(dw.double(), dw0.double() + g)
    assert torch.equal(dw[..., c.cin:], dw0[..., c.cin:])
    if c.dbias:
        assert torch.equal(db.double(), db0.double() + gb)


def _wgrad_real(c, device):
    """|got - ref| <= (M + 1) * 2^-24 * sum |dy * x| per element (bias: sum |dy|): M products, each rounded at most once,
    and M additions in ANY order or grouping (registers, LDS atomics, global atomics) — the standard bound
    gamma_(M + 1) of a float32 sum of M terms.  Only useful while M is small (M <= 400 here): at larger M a dropped
    pixel hides under it, which is what the integer cases are for."""
    assert c.M <= 400
    x, win = _image(c, torch.rand((c.B, *c.I, c.cin), generator=_gen(c.seed)))
    dy = torch.randn((c.M, c.N), generator=_gen(c.seed + 1))
    dw, db = _run_wgrad(c, device, x, dy, torch.zeros(c.taps, c.N, 4), torch.zeros(c.N))
    g, gb = _wgrad_ref(c, win, dy)
    ga, gba = _wgrad_ref(c, win.abs(), dy.abs())
    err, errb = (dw.double() - g).abs(), (db.double() - gb).abs()
    bar, barb = (c.M + 1) * EPS * ga, (c.M + 1) * EPS * gba
    print("weight gradient %s: max err / bar = %.3g, bias %.3g" % (_id(c), (err / bar.clamp_min(1e-300)).max().item(),
                                                                  (errb / barb).max().item()))
    assert (err <= bar).all() and (errb <= barb).all()
    assert torch.equal(dw[..., c.cin:], torch.zeros(c.taps, c.N, 4 - c.cin))


# ------------------------------------------------------------------------------------------------
# the generic family: conv_smallc_fwd_kernel<NG>, conv_smallc_wgrad_stream_kernel<G>
# ------------------------------------------------------------------------------------------------
CROP = dict(stored=(4, 11, 14), crop=(1, 2, 3), I=(3, 7, 9), ld_x=8)      # logical window strictly inside the stored grid

# every NG instance (N 4: NG 4; 6, 13, 16, 17: 4, 4, 4, 8; 36: 16; 72: 32; 136, 260: 64, 260 in two channel blocks) over
# M = 2 * 11 * 17 = 374 pixels (a ragged last tile of 64); N = 6, 13, 17 store a partial channel quad, 72 / 136 leave
# dead lanes in the channel tile; every other case has ld_out = pad4(N) + 4; with bias + ReLU and plain
GENERIC_FWD = [_case(N=N, c_real=(0, 3)[i % 2], extra=4 * (i % 2), bias=full, relu=full, seed=10 + i)
               for i, N in enumerate([4, 6, 13, 16, 17, 36, 72, 136, 260]) for full in (True, False)]
# kernel extents on a volume (ID = 5)
GENERIC_FWD += [_case(I=(5, 6, 7), K=K, cin=cin, c_real=cin % 4, N=20, seed=40 + i)
                for i, K in enumerate([(1, 2, 2), (2, 2, 2), (1, 1, 3), (3, 1, 1), (1, 3, 3), (3, 3, 3)]) for cin in (2, 4)]
# zero padding: P = K - 1 on every axis (the data-gradient geometry) and a mixed one, on inputs so small that most
# taps of most pixels fall outside, and once over several pixel tiles
PADDED = [dict(I=(1, 3, 4), K=(1, 3, 3), P=(0, 2, 2)), dict(I=(2, 3, 3), K=(3, 3, 3), P=(2, 2, 2)),
          dict(I=(1, 3, 4), K=(1, 3, 3), P=(0, 2, 1)), dict(I=(4, 3, 4), K=(3, 3, 3), P=(0, 2, 1)),
          dict(I=(1, 13, 19), K=(1, 3, 3), P=(0, 2, 2))]
GENERIC_FWD += [_case(cin=3, N=8, seed=60 + i, **g) for i, g in enumerate(PADDED)]
# crop and pixel stride
GENERIC_FWD += [_case(K=K, cin=3, c_real=3, N=8, seed=70 + i, **CROP) for i, K in enumerate([(3, 3, 3), (1, 3, 3)])]
# ... with zero padding at the window's border, where the stored neighbour holds NaN
GENERIC_FWD += [_case(K=(3, 3, 3), P=(2, 2, 2), cin=3, N=8, seed=75, **CROP)]
# more than 4096 pixel tiles: tiles_per_block = 4 (M = 513 * 513 = 263 169, ragged)
GENERIC_FWD += [_case(B=1, I=(1, 515, 515), cin=2, c_real=2, N=4, seed=80)]
# 3-D with NG = 32 / 64: 83 KB / 138 KB of dynamic LDS per workgroup
GENERIC_FWD += [_case(I=(5, 6, 7), K=(3, 3, 3), cin=3, N=N, seed=90 + N) for N in (72, 136)]


@pytest.mark.parametrize("c", GENERIC_FWD, ids=_id)
def test_generic_forward_exact(c, device):
    _fwd_exact(c, device)


def test_generic_forward_large_lds_request():
    """the two 3-D cases above ask for more than 64 KB of dynamic LDS ((4 * taps * NG * 4 + 64 * 4 * taps) * 4 bytes) —
    launches the HIP runtime accepts on gfx950 (160 KB per workgroup) without a function attribute: they pass"""
    for c in GENERIC_FWD[-2:]:
        ng = 4
        while ng < 64 and ng * 4 < c.N:
            ng *= 2
        assert (4 * c.taps * ng * 4 + 64 * 4 * c.taps) * 4 in (82944, 138240)


# lane groupings G = 4, 4, 8, 16, 32, 64, 64: the per-tap-load path (G < 16) and the lane-broadcast path (G >= 16);
# every other case has ld_dy = N + 4; a third has no dbias
GENERIC_WGRAD = [_case(N=N, cin=cin, c_real=cin % 4, extra=4 * ((i + cin) % 2), dbias=(i + cin) % 3 != 0, seed=100 + 3 * i + cin)
                 for i, N in enumerate([4, 8, 20, 36, 72, 136, 260]) for cin in (2, 3, 4)]
# tap groups on blockIdx.z (27 taps: three), 8 taps, 4 taps
GENERIC_WGRAD += [_case(I=(5, 6, 7), K=K, cin=3, N=N, seed=130 + i)
                  for i, (K, N) in enumerate([((3, 3, 3), 8), ((3, 3, 3), 72), ((2, 2, 2), 8), ((2, 2, 2), 36), ((1, 2, 2), 8)])]
GENERIC_WGRAD += [_case(cin=3, N=N, seed=140 + 2 * i + N // 36, **g) for i, g in enumerate(PADDED) for N in (8, 36)]
GENERIC_WGRAD += [_case(K=K, cin=3, c_real=3, N=N, extra=4, seed=160 + i, **CROP)
                  for i, (K, N) in enumerate([((3, 3, 3), 8), ((1, 3, 3), 8), ((1, 3, 3), 72)])]
GENERIC_WGRAD += [_case(K=(3, 3, 3), P=(2, 2, 2), cin=3, N=8, seed=165, **CROP)]
# M = 182 * 182 = 33 124 >= 32 768: 512 blocks of cdiv(M, 512) pixels instead of one block per 64
GENERIC_WGRAD += [_case(B=1, I=(1, 184, 184), cin=2, c_real=2, N=8, seed=170)]


@pytest.mark.parametrize("c", GENERIC_WGRAD, ids=_id)
def test_generic_weight_gradient_exact(c, device):
    _wgrad_exact(c, device)


# ------------------------------------------------------------------------------------------------
# the grey-scale family (c_real = 1, valid 3x3 / 3x3x3, N % 4 == 0): conv_grey_fwd_kernel, conv_grey_wgrad_kernel
# ------------------------------------------------------------------------------------------------
def _grey(**kw):
    return _case(cin=1, c_real=1, **kw)


WIDTHS = [3, 4, 5, 6, 7, 9, 10]          # OW = 1, 2, 3, 4, 5, 7, 8: every OW % 4, and OW < 4
VOLUMES = [dict(I=(3, 5, 7), K=(3, 3, 3)), dict(I=(6, 5, 7), K=(3, 3, 3)), dict(I=(4, 5, 7), K=(1, 3, 3))]
# runs of four pixels along x: every tail
GREY_FWD = [_grey(I=(1, 5, IW), N=N, extra=4 * (i % 2), seed=200 + 7 * i + j)
            for i, N in enumerate([4, 8, 64, 72, 136]) for j, IW in enumerate(WIDTHS)]
# one output plane / several (KD = 3), the (1, 3, 3) kernel of an anisotropic network on a volume
GREY_FWD += [_grey(N=N, seed=240 + 2 * i + N // 72, **g) for i, g in enumerate(VOLUMES) for N in (8, 72)]
# one item: three of the four waves have nothing to do, every prefetch is clamped to the last item
GREY_FWD += [_grey(B=1, I=(1, 3, 3), N=4, seed=250), _grey(B=1, I=(3, 3, 3), K=(3, 3, 3), N=4, seed=251)]
# the prefetch loop unrolled by three: 768 waves per block column over 960, 1920, 2400 runs: 1-2, 2-3, 3-4 trips
GREY_FWD += [_grey(B=1, I=(1, IH, 192), N=256, bias=IH != 42, relu=IH != 42, seed=260 + IH) for IH in (22, 42, 52)]
GREY_FWD += [_grey(K=K, N=8, seed=270 + i, **CROP) for i, K in enumerate([(3, 3, 3), (1, 3, 3)])]


@pytest.mark.parametrize("c", GREY_FWD, ids=_id)
def test_grey_forward_exact(c, device):
    _fwd_exact(c, device)


GREY_WGRAD = [_grey(I=(1, 5, IW), N=N, extra=4 * ((i + j) % 2), dbias=(i + j) % 3 != 0, seed=300 + 7 * i + j)
              for i, N in enumerate([4, 64, 72]) for j, IW in enumerate(WIDTHS)]
GREY_WGRAD += [_grey(N=N, seed=330 + 2 * i + N // 72, **g) for i, g in enumerate(VOLUMES) for N in (8, 72)]
GREY_WGRAD += [_grey(B=1, I=(1, 3, 3), N=4, seed=340), _grey(B=1, I=(3, 3, 3), K=(3, 3, 3), N=4, seed=341)]
GREY_WGRAD += [_grey(K=K, N=8, extra=4, seed=350 + i, **CROP) for i, K in enumerate([(3, 3, 3), (1, 3, 3)])]


@pytest.mark.parametrize("c", GREY_WGRAD, ids=_id)
def test_grey_weight_gradient_exact(c, device):
    _wgrad_exact(c, device)


def test_grey_weight_gradient_prefetch_rotation_exact(device):
    """2400 runs over 768 waves: 3-4 trips through the loop unrolled by three.  dy in {-1, 0, 1} and an image in {0, 1}:
    sums <= M = 9500."""
    _wgrad_exact(_grey(B=1, I=(1, 52, 192), N=256, seed=360), device, x_hi=1, dy_hi=1)


# ------------------------------------------------------------------------------------------------
# real-valued data under derived bars: one case per kernel family
# ------------------------------------------------------------------------------------------------
REAL_FWD = [_grey(I=(1, 13, 19), N=72, seed=400),                                          # grey, 2-D
            _case(I=(5, 6, 7), K=(3, 3, 3), cin=3, N=136, seed=401),                       # generic, 3-D, NG = 64
            _case(I=(2, 3, 3), K=(3, 3, 3), P=(2, 2, 2), cin=4, N=13, extra=4, seed=402),  # generic, 3-D padded
            _case(cin=2, c_real=2, N=260, seed=403),                                       # generic, two channel blocks
            _grey(I=(6, 5, 7), K=(3, 3, 3), N=8, seed=404)]                                # grey, 3-D


@pytest.mark.parametrize("c", REAL_FWD, ids=_id)
def test_forward_real_valued(c, device):
    _fwd_real(c, device)


REAL_WGRAD = [_case(cin=3, N=36, seed=410), _case(cin=2, c_real=2, N=8, seed=411),        # generic: G = 16 (broadcast), 4
              _case(I=(5, 6, 7), K=(3, 3, 3), cin=4, N=72, seed=412),                      # generic, three tap groups
              _grey(I=(1, 13, 19), N=72, seed=413), _grey(I=(6, 5, 7), K=(3, 3, 3), N=8, seed=414)]


@pytest.mark.parametrize("c", REAL_WGRAD, ids=_id)
def test_weight_gradient_real_valued(c, device):
    _wgrad_real(c, device)


# ------------------------------------------------------------------------------------------------
# which of the two families ran
# ------------------------------------------------------------------------------------------------
def test_dispatch_between_grey_and_generic_kernels(device):
    """c_real = 1 promises that only channel slot 0 of the image can be non-zero.  This test VIOLATES the hint on purpose,
    to observe the dispatch without touching product code: slots 1..3 of the image and of a hand-built wpack hold
    non-zero integers, so the grey kernels (which read slot 0 only) give the slot-0 convolution and the generic kernels
    the full 4-slot one.  Every other test keeps the slots >= c_real zero."""
    C = _clx()

    def setup(N=8, K=(1, 3, 3), P=(0, 0, 0), seed=500):
        c = _case(I=(1, 6, 7), K=K, P=P, cin=4, c_real=1, N=N, seed=seed)
        x, win = _image(c, _ints((c.B, *c.I, 4), 1, 4, seed))
        w = _ints((N, 4, *K), 1, 8, seed + 1) * (1 - 2 * _ints((N, 4, *K), 0, 1, seed + 2))      # non-zero, both signs
        b = _ints((N + 1,), -8, 8, seed + 3)
        wp = w.reshape(N, 4, c.taps).permute(0, 2, 1).contiguous().to(device)                    # [N][taps][4] by hand
        grey, full = _conv_ref(c, win, w[:, :1], b[:N]), _conv_ref(c, win, w, b[:N])
        assert not torch.equal(grey, full)
        return c, x, win, w, wp, b, grey, full

    # forward: aligned bias -> grey
    c, x, win, w, wp, b, grey, full = setup()
    b_d = b.to(device)
    assert b_d.data_ptr() % 16 == 0
    _check_out(_run_fwd(c, device, x, wp, b_d), grey, c.N)
    # the same call with the bias one float further (4-byte aligned only) -> generic
    b_off = torch.cat([b[:1], b[:c.N]]).to(device)
    _check_out(_run_fwd(c, device, x, wp, b_off.data_ptr() + 4), full, c.N)
    # no bias -> grey again
    _check_out(_run_fwd(c, device, x, wp, None), _conv_ref(c, win, w[:, :1], None), c.N)
    # N % 4 != 0, a 2 x 2 kernel, any padding -> generic
    for i, kw in enumerate((dict(N=6), dict(K=(1, 2, 2)), dict(P=(0, 1, 1)), dict(P=(0, 0, 1)))):
        c, x, win, w, wp, b, grey, full = setup(seed=510 + i, **kw)
        _check_out(_run_fwd(c, device, x, wp, b[:c.N].to(device)), full, c.N)

    # weight gradient: the grey route leaves slots 1..3 of dwpack untouched (7.0 stays 7.0), the generic route adds the
    # gradient of every slot
    for kw, is_grey in ((dict(), True), (dict(K=(1, 2, 2)), False), (dict(P=(0, 1, 1)), False)):
        c, x, win = setup(seed=530, **kw)[:3]
        dy = _ints((c.M, c.N), -2, 2, 531)
        dw, db = _run_wgrad(c, device, x, dy, torch.full((c.taps, c.N, 4), 7.0), torch.zeros(c.N))
        g, gb = _wgrad_ref(c, win, dy)
        assert (g[..., 1:] != 0).any()
        assert torch.equal(dw[..., 0].double(), 7.0 + g[..., 0])
        assert torch.equal(dw[..., 1:].double(), torch.full_like(g[..., 1:], 7.0) if is_grey else 7.0 + g[..., 1:])
        assert torch.equal(db.double(), gb)


# ------------------------------------------------------------------------------------------------
# the seam: 4-channel descriptors the small-channel kernels must leave to the implicit-GEMM kernel
# ------------------------------------------------------------------------------------------------
def _gate_words(t, words):
    """(M, n) booleans -> (M, words) int32 words, bit (n & 31) of word (n >> 5)"""
    M, n = t.shape
    bits = torch.zeros(M, words * 32, dtype=torch.int64)
    bits[:, :n] = t.long()
    v = (bits.view(M, words, 32) << torch.arange(32)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


@pytest.mark.parametrize("seam", ["accumulate", "mask", "gate_out", "mask_bits", "n2", "k1"])
@pytest.mark.parametrize("c_real", [1, 3])
def test_seam_to_the_implicit_gemm_kernel(seam, c_real, device):
    """accumulate, a float mask, gate_out, mask_bits, N < 4 and a 1x1 kernel: exact on integers, and the profile counters
    show the implicit-GEMM launch."""
    N = 2 if seam == "n2" else 8
    K = (1, 1, 1) if seam == "k1" else (1, 3, 3)
    c = _case(I=(1, 9, 11), K=K, cin=c_real, c_real=c_real, N=N, extra=24 if seam == "gate_out" else 4,
              seed=600 + c_real)
    x, win = _image(c, _ints((c.B, *c.I, c.cin), 1, 4, c.seed))
    w = _ints((c.N, c.cin, *c.K), -8, 8, c.seed + 1)
    b = _ints((c.N,), -8, 8, c.seed + 2)
    wp, b_d = _pack(w, device), b.to(device)
    ref = _conv_ref(c, win, w, b)
    if seam == "accumulate":
        prev = _ints((c.M, c.N), -9, 9, c.seed + 3)
        out = _run_fwd(c, device, x, wp, b_d, igemm=True, prefill=prev, accumulate=1)
        c.relu = False
        ref = (_conv_ref(c, win, w, b) + prev.double()).clamp_min(0)
    elif seam == "mask":
        mask = _nan(device, c.M, c.ld)
        m = _ints((c.M, c.N), -1, 1, c.seed + 3)
        mask[:, : c.N] = m.to(device)
        out = _run_fwd(c, device, x, wp, b_d, igemm=True, mask=mask, ld_mask=c.ld)
        ref = ref * (m > 0)
    elif seam == "mask_bits":
        m = _ints((c.M, c.N), 0, 1, c.seed + 3) > 0
        out = _run_fwd(c, device, x, wp, b_d, igemm=True, mask_bits=_gate_words(m, 1).to(device), ld_mask_bits=1)
        ref = ref * m
    elif seam == "gate_out":
        assert c.ld == 32
        gate = torch.full((c.M, 1), -1, dtype=torch.int32, device=device)
        out = _run_fwd(c, device, x, wp, b_d, igemm=True, gate_out=gate, ld_gate=1)
        assert (ref > 0).any() and (ref == 0).any()
        assert torch.equal(gate.cpu(), _gate_words(ref > 0, 1))
    else:
        out = _run_fwd(c, device, x, wp, b_d, igemm=True)
    _check_out(out, ref, c.N)
