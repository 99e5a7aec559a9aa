"""The streaming kernels between the convolutions (csrc/glue.hip, csrc/pack.hip) through the C ABI, each against a plain
restatement of what include/clx.h says it computes: max-pool forward / backward, nearest-upsample backward, the sub-pixel
re-indexing pair, planar <-> pixel-major, the plain weight packings, the inference statistics.

These kernels move, compare, gate and add in a fixed order, so every comparison is exact (torch.equal on values) except
the statistics, whose bars are derived where they are used.  Outputs are prefilled with NaN (every element that should be
written was written, no padding lane was), lanes an input's wider pixel stride leaves unused hold NaN (never read).

Replaces funlib Downsample / Upsample (nn.MaxPool{2,3}d, nearest upsample + crop: cellulus/models/unet.py:24-51) and
torch.std_mean of the noisy forwards (cellulus/models/unet.py:90-98).

Not pinned here: NaN / Inf inside pooled data (the kernels' `>` drops a NaN that is not first in its window, torch
propagates it).
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _clx():
    from cellulus_amd import _clx

    return _clx


def _call(name, device, *args):
    c = _clx()
    c.call(name, *[c.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], c.stream_ptr(device))


def _nan(device, *shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=device)


def _widen(t, ld, device):
    """t (..., C) on the host -> device tensor (..., ld) whose lanes [C, ld) hold NaN."""
    out = _nan(device, *t.shape[:-1], ld)
    out[..., : t.shape[-1]] = t.to(device)
    return out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


# ------------------------------------------------------------------------------------------------
# 1 / 2. clx_maxpool_fwd, clx_maxpool_bwd
# ------------------------------------------------------------------------------------------------
# (B, D, H, W, C, (fz, fy, fx)): the smallest; C/4 = 3; 3-D; pooled width 1 and a factor of 1; a prime width (the
# multiply-shift decode divides by 1031, 3, 5, 1); 364 * 364 * 16 = 2 119 936 work items — above the grid cap of
# 8192 * 256 = 2 097 152, so the grid-stride loop makes a second trip
POOL_CASES = [
    (2, 1, 6, 8, 4, (1, 2, 2)),
    (1, 1, 9, 4, 12, (1, 3, 2)),
    (3, 4, 6, 10, 8, (2, 2, 2)),
    (1, 6, 5, 2, 20, (3, 1, 2)),
    (1, 1, 4, 1031, 4, (1, 2, 1)),
    (1, 1, 728, 728, 64, (1, 2, 2)),
]
POOL_IDS = ["smallest", "c12_f32", "3d", "pooled_w1", "prime_w", "above_grid_cap"]
KINDS = ["randn", "ints"]          # continuous | integer-valued in {-2..3}: all-negative windows and many ties


def _windows(x, f):
    """(B, D, H, W, C) -> list of the window's members in scan order (dz, dy, dx), each (B, OD, OH, OW, C)."""
    B, D, H, W, C = x.shape
    fz, fy, fx = f
    v = x.view(B, D // fz, fz, H // fy, fy, W // fx, fx, C)
    return [v[:, :, dz, :, dy, :, dx] for dz in range(fz) for dy in range(fy) for dx in range(fx)]


def _pool_ref(x, f):
    m = None
    for s in _windows(x, f):
        m = s.clone() if m is None else torch.where(s > m, s, m)      # the running value is replaced on `>`
    return m.contiguous()


def _route_ref(x, dy, f):
    """The pooled gradient at the winner of each window: torch's float64 max_pool3d on the CPU."""
    xd = x.double().permute(0, 4, 1, 2, 3).requires_grad_()
    y, _ = F.max_pool3d(xd, f, f, return_indices=True)
    y.backward(dy.double().permute(0, 4, 1, 2, 3))
    return xd.grad.permute(0, 2, 3, 4, 1).float().contiguous()


@pytest.fixture(scope="module")
def pool_data():
    """Inputs and references of the pooling cases, made once per (case, kind) and shared by the forward and backward
    tests (never modified); released with the module."""
    cache = {}

    def get(case, kind):
        key = (case, kind)
        if key not in cache:
            B, D, H, W, C, f = case
            seed = POOL_CASES.index(case) * 2 + KINDS.index(kind)
            shape = (B, D, H, W, C)
            x = torch.randn(shape, generator=_gen(seed)) if kind == "randn" else _ints(shape, -2, 3, seed)
            if kind == "ints":
                x[0, ..., 0] = _ints(shape[1:4], -2, -1, seed)         # a channel whose every window is all negative
            pooled = _pool_ref(x, f)
            dy = torch.randn(pooled.shape, generator=_gen(100 + seed))
            cache[key] = dict(x=x, pooled=pooled, dy=dy, routed=None)
        return cache[key]

    yield get
    cache.clear()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_maxpool_fwd(case, kind, device, pool_data):
    B, D, H, W, C, f = case
    d = pool_data(case, kind)
    if kind == "ints":
        assert (d["pooled"] < 0).any()                  # all-negative windows: the result is not a clamped 0
    x = d["x"].to(device)
    y = _nan(device, *d["pooled"].shape)
    _call("clx_maxpool_fwd", device, x, y, B, D, H, W, C, *f)
    assert torch.equal(y.cpu(), d["pooled"])


def _skip_geometry(mode, dims):
    """Extent and crop offset of the skip tensor inside a grid of extent dims."""
    S, c = [], []
    for a in dims:
        if mode == "inner":           # one pixel in from the near side, one short of the far side
            c.append(min(1, a - 1))
            S.append(max(1, a - c[-1] - 1))
        elif mode == "corner":        # flush against the far corner
            S.append(max(1, a // 2))
            c.append(a - S[-1])
        else:                         # "origin": crop (0, 0, 0)
            c.append(0)
            S.append(max(1, a - 1))
    return tuple(S), tuple(c)


SKIPS = [None, ("inner", 0), ("inner", 4), ("corner", 4), ("origin", 0)]
SKIP_IDS = ["noskip", "inner_ldC", "inner_ldC4", "corner_ldC4", "origin_ldC"]


def _run_maxpool_bwd(device, case, x, pooled, dy, skip, seed):
    """-> (dx on the host, the skip gradient placed in a zero grid of x's extent)."""
    B, D, H, W, C, f = case
    placed = torch.zeros_like(x)
    sk_dev, ld, S, c = None, 0, (0, 0, 0), (0, 0, 0)
    if skip is not None:
        mode, pad = skip
        S, c = _skip_geometry(mode, (D, H, W))
        assert mode == "origin" or any(c)
        ld = C + pad
        sk = torch.randn((B, *S, C), generator=_gen(200 + seed))
        placed[:, c[0]:c[0] + S[0], c[1]:c[1] + S[1], c[2]:c[2] + S[2]] = sk
        sk_dev = _widen(sk, ld, device)
    dx = _nan(device, B, D, H, W, C)
    _call("clx_maxpool_bwd", device, x.to(device), pooled.to(device), dy.to(device), sk_dev, ld, *S, *c, dx,
          B, D, H, W, C, *f)
    return dx.cpu(), placed


@pytest.mark.parametrize("skip", SKIPS, ids=SKIP_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", POOL_CASES, ids=POOL_IDS)
def test_maxpool_bwd(case, kind, skip, device, pool_data):
    """Routing by torch's float64 max_pool3d (first maximum of the window), then the skip gradient added in float32,
    then the gate x > 0."""
    d = pool_data(case, kind)
    if d["routed"] is None:
        d["routed"] = _route_ref(d["x"], d["dy"], case[5])
    x = d["x"]
    dx, placed = _run_maxpool_bwd(device, case, x, d["pooled"], d["dy"], skip, POOL_CASES.index(case))
    ref = torch.where(x > 0, d["routed"] + placed, torch.zeros(()))
    assert not torch.isnan(dx).any()                    # every element of dx was overwritten
    assert torch.equal(dx, ref)


@pytest.mark.parametrize("case", POOL_CASES[:5], ids=POOL_IDS[:5])
def test_maxpool_bwd_gives_a_tied_window_to_its_first_maximum(case, device):
    """Integer-valued input: the gradient of a window whose positive maximum occurs more than once goes to the first
    occurrence in (dz, dy, dx) order; a later equal one gets only its skip term.  The reference here is a NumPy
    first-occurrence argmax, not torch."""
    B, D, H, W, C, f = case
    seed = 50 + POOL_CASES.index(case)
    x = _ints((B, D, H, W, C), -2, 3, seed)
    pooled = _pool_ref(x, f)
    dy = _ints(tuple(pooled.shape), 1, 4, seed + 1)                   # never 0: a routed gradient is visible
    win = np.stack([s.numpy() for s in _windows(x, f)])               # (K, B, OD, OH, OW, C)
    m = win.max(axis=0)
    is_max = win == m
    first = np.arange(len(win)).reshape(-1, 1, 1, 1, 1, 1) == win.argmax(axis=0)     # argmax: the first occurrence
    later = is_max & ~first
    # precondition on the input (not a measurement): some window has a positive maximum at two scan positions
    assert ((m > 0) & (is_max.sum(axis=0) >= 2)).any()
    assert (later & (win > 0)).any()

    def to_grid(a):                                                    # (K, B, OD, OH, OW, C) -> (B, D, H, W, C)
        fz, fy, fx = f
        a = a.reshape(fz, fy, fx, B, D // fz, H // fy, W // fx, C)
        return np.ascontiguousarray(a.transpose(3, 4, 0, 5, 1, 6, 2, 7)).reshape(B, D, H, W, C)

    dx, placed = _run_maxpool_bwd(device, case, x, pooled, dy, ("inner", 4), seed)
    dx, placed, xs = dx.numpy(), placed.numpy(), x.numpy()
    routed = to_grid(np.where(first, dy.numpy()[None], np.float32(0)))
    ref = np.where(xs > 0, routed + placed, np.float32(0))
    assert np.array_equal(dx, ref)
    sel = to_grid(later) & (xs > 0)
    assert np.array_equal(dx[sel], placed[sel])                        # the later equal maximum: its skip term alone
    sel = to_grid(first) & (xs > 0)
    assert np.array_equal(dx[sel], (to_grid(np.broadcast_to(dy.numpy()[None], win.shape)) + placed)[sel])


# ------------------------------------------------------------------------------------------------
# 3. clx_upsample_bwd
# ------------------------------------------------------------------------------------------------
def _crop(mode, lo_dims, f):
    """Crop offset o and extent L of dcat inside the up-sampled grid, per axis."""
    o, L = [], []
    for a, k in zip(lo_dims, f):
        ext = a * k
        if mode == "full" or ext < 3:
            o.append(0), L.append(ext)
        elif mode == "odd":          # boundary blocks are partly outside the crop
            o.append(1), L.append(ext - 2)
        else:                        # "empty": the first and last low-resolution rows / columns have no member at all
            o.append(k), L.append(ext - 2 * k)
    return tuple(o), tuple(L)


def _upsample_bwd_ref(dcat, coff, C, o, L, y, f):
    B, D, H, W, _ = y.shape
    fz, fy, fx = f
    grid = torch.zeros(B, D * fz, H * fy, W * fx, C)
    grid[:, o[0]:o[0] + L[0], o[1]:o[1] + L[1], o[2]:o[2] + L[2]] = dcat[..., coff:coff + C]
    g = torch.zeros(B, D, H, W, C)
    for s in _windows(grid, f):      # sequential float32 additions in (dz, dy, dx) order
        g = g + s
    return torch.where(y > 0, g, torch.zeros(()))


def _run_upsample_bwd(device, lo_dims, B, C, f, mode, coff, seed):
    D, H, W = lo_dims
    o, L = _crop(mode, lo_dims, f)
    for a, k, oo, ll in zip(lo_dims, f, o, L):
        assert oo >= 0 and ll >= 1 and oo + ll <= a * k
    ld = coff + C + 4
    dcat = torch.full((B, *L, ld), NAN)
    dcat[..., coff:coff + C] = torch.randn((B, *L, C), generator=_gen(seed))
    y = torch.randn((B, D, H, W, C), generator=_gen(seed + 1))
    flat = y.view(-1)
    flat[0::5] = 0.0
    flat[1::7] = -0.0
    assert (y == 0).any() and (y < 0).any() and (y > 0).any() and torch.signbit(y[y == 0]).any()
    dy = _nan(device, B, D, H, W, C)
    _call("clx_upsample_bwd", device, dcat.to(device), ld, coff, *L, *o, y.to(device), dy, B, D, H, W, C, *f)
    ref = _upsample_bwd_ref(dcat, coff, C, o, L, y, f)
    if mode == "empty":
        assert (ref[:, :, 0] == 0).all() and (ref[:, :, :, -1] == 0).all()
    return dy.cpu(), ref


@pytest.mark.parametrize("C,coff", list(itertools.product([4, 12, 64], [0, 4, 68])))
@pytest.mark.parametrize("mode", ["full", "odd", "empty"])
@pytest.mark.parametrize("f", [(1, 2, 2), (2, 2, 2), (1, 3, 3), (1, 1, 2)], ids=lambda f: "f%d%d%d" % f)
def test_upsample_bwd(f, mode, C, coff, device):
    lo_dims = (3 if f[0] > 1 else 1, 5, 7)
    dy, ref = _run_upsample_bwd(device, lo_dims, 2, C, f, mode, coff, seed=C + coff)
    assert torch.equal(dy, ref)


def test_upsample_bwd_above_the_grid_cap(device):
    dy, ref = _run_upsample_bwd(device, (1, 364, 364), 1, 64, (1, 2, 2), "odd", 4, seed=9)
    assert torch.equal(dy, ref)


# ------------------------------------------------------------------------------------------------
# 4. clx_depth_to_space, clx_space_to_depth
# ------------------------------------------------------------------------------------------------
def _d2s_ref(lo, N, f):
    """hi[(b, z fz + a, y fy + bb, x fx + c)][n] = lo[(b, z, y, x)][((a fy + bb) fx + c) N + n]"""
    B, D, H, W, _ = lo.shape
    fz, fy, fx = f
    v = lo[..., : fz * fy * fx * N].reshape(B, D, H, W, fz, fy, fx, N)
    return v.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, D * fz, H * fy, W * fx, N).contiguous()


def _subpixel_pair(device, dims, N, f, pad_lo, pad_hi, lo_vals, hi_vals):
    """-> (depth_to_space(lo_vals), space_to_depth(hi_vals)) as written by the kernels, padding lanes checked."""
    B, D, H, W = dims
    P = f[0] * f[1] * f[2]
    ld_lo, ld_hi = P * N + pad_lo, N + pad_hi
    hi = _nan(device, B, D * f[0], H * f[1], W * f[2], ld_hi)
    _call("clx_depth_to_space", device, _widen(lo_vals, ld_lo, device), ld_lo, hi, ld_hi, B, D, H, W, N, *f)
    lo = _nan(device, B, D, H, W, ld_lo)
    _call("clx_space_to_depth", device, _widen(hi_vals, ld_hi, device), ld_hi, lo, ld_lo, B, D, H, W, N, *f)
    assert torch.isnan(hi[..., N:]).all() and torch.isnan(lo[..., P * N:]).all()
    return hi[..., :N].cpu().contiguous(), lo[..., : P * N].cpu().contiguous()


@pytest.mark.parametrize("pad_lo,pad_hi", [(0, 0), (4, 0), (0, 4), (4, 4)])
@pytest.mark.parametrize("N", [4, 12])
@pytest.mark.parametrize("f", [(1, 2, 2), (2, 2, 2), (1, 1, 2), (2, 1, 2)], ids=lambda f: "f%d%d%d" % f)
def test_subpixel_pair(f, N, pad_lo, pad_hi, device):
    dims = (2, 3 if f[0] > 1 else 1, 3, 5)
    B, D, H, W = dims
    P = f[0] * f[1] * f[2]
    a = torch.randn((B, D, H, W, P * N), generator=_gen(N))
    b = torch.randn((B, D * f[0], H * f[1], W * f[2], N), generator=_gen(N + 1))
    hi, lo = _subpixel_pair(device, dims, N, f, pad_lo, pad_hi, a, b)
    assert torch.equal(hi, _d2s_ref(a, N, f))
    # space_to_depth is the inverse gather: the element depth_to_space(lo) takes FROM is where it puts b's element
    assert torch.equal(_d2s_ref(lo, N, f), b)
    # round trip through both kernels
    _, back = _subpixel_pair(device, dims, N, f, pad_lo, pad_hi, a, hi)
    assert torch.equal(back, a)
    # adjoint: the two are permutations of each other.  Small integers, so both float64 sums are exact whatever their
    # order (|term| <= 64, < 2^14 terms) and the identity holds to the bit
    ai, bi = _ints(tuple(a.shape), -8, 8, N + 2), _ints(tuple(b.shape), -8, 8, N + 3)
    hi, lo = _subpixel_pair(device, dims, N, f, pad_lo, pad_hi, ai, bi)
    assert (hi.double() * bi.double()).sum().item() == (ai.double() * lo.double()).sum().item()


def test_subpixel_pair_above_the_grid_cap(device):
    dims, N, f = (1, 1, 364, 364), 16, (1, 2, 2)            # 364 * 364 * 4 phases * 4 = 2 119 936 work items
    a = torch.randn((1, 1, 364, 364, 64), generator=_gen(0))
    b = torch.randn((1, 1, 728, 728, 16), generator=_gen(1))
    hi, lo = _subpixel_pair(device, dims, N, f, 4, 4, a, b)
    assert torch.equal(hi, _d2s_ref(a, N, f))
    assert torch.equal(_d2s_ref(lo, N, f), b)


# ------------------------------------------------------------------------------------------------
# 5. clx_planar_to_pixel, clx_pixel_to_planar
# ------------------------------------------------------------------------------------------------
GUARD = 64       # floats behind a buffer's logical end: NaN before, NaN after (not written), and never a value read


def _guarded(device, *shape):
    n = int(np.prod(shape))
    buf = _nan(device, n + GUARD)
    return buf, buf[:n].view(*shape)


def _run_planar_pixel(device, B, C, n, ld):
    planar = torch.randn((B, C, n), generator=_gen(C * 10 + B))
    # the planar source sits in front of one more plane of NaN: a channel loop that runs one too far would carry it into
    # the pad lanes
    src = _nan(device, B * C * n + n)[: B * C * n].view(B, C, n)
    src.copy_(planar)
    pix_buf, pix = _guarded(device, B, n, ld)
    _call("clx_planar_to_pixel", device, src, pix, B, C, n, ld)
    want = torch.zeros(B, n, ld)
    want[..., :C] = planar.permute(0, 2, 1)
    assert torch.equal(pix.cpu(), want)                  # lanes [C, ld) are written as 0
    assert torch.isnan(pix_buf[-GUARD:]).all()
    # back, from a pixel-major tensor whose lanes [C, ld) hold NaN
    pix[..., C:] = NAN
    back_buf, back = _guarded(device, B, C, n)
    _call("clx_pixel_to_planar", device, pix, back, B, C, n, ld)
    assert torch.equal(back.cpu(), planar)
    assert torch.isnan(back_buf[-GUARD:]).all()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 7, 4099])
@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5])
def test_planar_pixel(C, extra, n, B, device):
    _run_planar_pixel(device, B, C, n, (C + 3) // 4 * 4 + extra)


def test_planar_pixel_above_the_grid_cap(device):
    _run_planar_pixel(device, 2, 1, 600_000, 4)          # 1 200 000 pixels > 4096 * 256 = 1 048 576


# ------------------------------------------------------------------------------------------------
# 6. clx_pack_weights (CLX_PACK_FWD / CLX_PACK_DGRAD), clx_unpack_wgrad
# ------------------------------------------------------------------------------------------------
CLX_PACK_FWD, CLX_PACK_DGRAD = 0, 1
PACK_SHAPES = [(5, 3, 9), (8, 1, 27), (64, 12, 1), (7, 6, 4)]       # (cout, cin, taps)


@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("cout,cin,taps", PACK_SHAPES)
def test_pack_weights_fwd_and_dgrad(cout, cin, taps, extra, device):
    cin_pad, cout_pad = (cin + 3) // 4 * 4 + extra, (cout + 3) // 4 * 4 + extra
    w = torch.randn((cout, cin, taps), generator=_gen(cout))
    # FWD: wp[n][tap][c] = w[n][c][tap], c >= cin -> 0; the packed buffer is [cout][taps][cin_pad]
    buf, wp = _guarded(device, cout, taps, cin_pad)
    _call("clx_pack_weights", device, w.to(device), wp, cout, cin, taps, cin_pad, cout_pad, CLX_PACK_FWD)
    want = torch.zeros(cout, taps, cin_pad)
    want[:, :, :cin] = w.permute(0, 2, 1)
    assert torch.equal(wp.cpu(), want)
    assert torch.isnan(buf[-GUARD:]).all()
    # DGRAD: wp[c][tap][n] = w[n][c][taps - 1 - tap], n >= cout or c >= cin -> 0; [cin_pad][taps][cout_pad]
    buf, wp = _guarded(device, cin_pad, taps, cout_pad)
    _call("clx_pack_weights", device, w.to(device), wp, cout, cin, taps, cin_pad, cout_pad, CLX_PACK_DGRAD)
    want = torch.zeros(cin_pad, taps, cout_pad)
    want[:cin, :, :cout] = w.flip(2).permute(1, 2, 0)
    assert torch.equal(wp.cpu(), want)
    assert torch.isnan(buf[-GUARD:]).all()
    if taps > 1:
        assert not torch.equal(w.flip(2), w)             # the reversal of the taps is visible in this input


@pytest.mark.parametrize("cout,cin,taps", PACK_SHAPES)
def test_unpack_wgrad(cout, cin, taps, device):
    rows, cin_pad = cout + 3, (cin + 3) // 4 * 4 + 4
    dw_ref = torch.randn((cout, cin, taps), generator=_gen(cin))
    dwp = torch.full((taps, rows, cin_pad), NAN)         # NaN in every padded row and lane
    dwp[:, :cout, :cin] = dw_ref.permute(2, 0, 1)
    buf, dw = _guarded(device, cout, cin, taps)
    _call("clx_unpack_wgrad", device, dwp.to(device), dw, cout, cin, taps, rows, cin_pad)
    assert not torch.isnan(dw).any()
    assert torch.equal(dw.cpu(), dw_ref)
    assert torch.isnan(buf[-GUARD:]).all()


# ------------------------------------------------------------------------------------------------
# 7. clx_noise_stats, clx_noise_stats_minmax
# ------------------------------------------------------------------------------------------------
def _noise_stats_f32(p):
    """The kernels' arithmetic restated in float32 NumPy: sequential sum over t, mean = s / T, sequential sum of the
    squared deviations, sqrt(v / T), the channels' standard deviations added in order (no fused multiply-add)."""
    T, C, n = p.shape
    s = np.zeros((C, n), np.float32)
    for t in range(T):
        s = s + p[t]
    mean = s / np.float32(T)
    v = np.zeros((C, n), np.float32)
    for t in range(T):
        dlt = p[t] - mean
        v = v + dlt * dlt
    std = np.sqrt(v / np.float32(T))
    tot = np.zeros(n, np.float32)
    for c in range(C):
        tot = tot + std[c]
    return mean, tot


@pytest.mark.parametrize("n", [1, 255, 4099])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 6, 31, 32, 33, 64, 65, 70])
def test_noise_stats(T, C, n, device):
    """The three code paths of the launcher (registers for T <= 32, for T <= 64, the generic kernel above) against
    torch.std_mean(unbiased=False) in float64.

    Bars, with m = max|preds|: a mean is a sequential float32 sum of T terms (error <= (T - 1) 2^-24 T m) divided by T,
    one more rounding: (T + 2) 2^-24 m.  A standard deviation computed around a mean that is off by e is off by at most
    e, plus the roundings of the T squares, T - 1 additions, the division and the root, each relative 2^-24 of at most m
    and halved by the root: (T + 4) 2^-23 m per channel, C channels summed.  Both hold whether or not the compiler
    contracts d * d + v into a fused multiply-add (one rounding less).  Checked on the CPU before they are used: the
    float32 restatement above stays inside both on this test's own inputs — the worst case over all parameters is
    0.16 of the mean bar and 0.052 of the std bar, so neither bar was widened.
    """
    c = _clx()
    variants = [(1.0, True), (50.0, True)] if n > 1 else [(1.0, False), (50.0, False), (1.0, True)]
    for s, const in variants:
        preds = torch.randn((T, C, n), generator=_gen(T * 100 + C)) * s
        if const:
            preds[:, :, n // 2] = 0.25                   # a pixel whose standard deviation is exactly 0
        m = preds.abs().max().item()
        std64, mean64 = torch.std_mean(preds.double(), dim=0, unbiased=False)
        tot64 = std64.sum(0)
        mean_bar = (T + 2) * 2.0 ** -24 * m
        std_bar = C * (T + 4) * 2.0 ** -23 * m
        mean32, tot32 = _noise_stats_f32(preds.numpy())
        assert np.abs(mean32 - mean64.numpy()).max() <= mean_bar
        assert np.abs(tot32 - tot64.numpy()).max() <= std_bar

        dev_preds = preds.to(device)
        out = _nan(device, C + 1, n)
        _call("clx_noise_stats", device, dev_preds, out, T, C, n)
        got = out.cpu().double()
        mean_err = (got[:C] - mean64).abs().max().item()
        std_err = (got[C] - tot64).abs().max().item()
        print(f"T={T} C={C} n={n} s={s}: mean err {mean_err:.3e} (bar {mean_bar:.3e}), std err {std_err:.3e} (bar {std_bar:.3e})")
        assert mean_err <= mean_bar
        assert std_err <= std_bar
        if const:
            assert got[C, n // 2].item() == 0.0
            assert torch.equal(got[:C, n // 2], torch.full((C,), 0.25, dtype=torch.float64))

        mm = _nan(device, c.NOISE_MINMAX_FLOATS)
        out2 = _nan(device, C + 1, n)
        if T <= 64:
            _call("clx_noise_stats_minmax", device, dev_preds, out2, T, C, n, mm, 1)
            assert torch.equal(out2, out)
            assert mm[:2].cpu().tolist() == [out[C].min().item(), out[C].max().item()]
        else:
            with pytest.raises(c.ClxError):
                _call("clx_noise_stats_minmax", device, dev_preds, out2, T, C, n, mm, 1)
            assert torch.isnan(out2).all()


# ------------------------------------------------------------------------------------------------
# 8. argument checks: a rejected call returns an error (and launches nothing) instead of ending the process.  Every
# buffer is as large as the nearest valid shape that covers the rejected one.
# ------------------------------------------------------------------------------------------------
def _pool_bufs(device):
    """x / dx (1, 2, 6, 8, 8); y / dy_pool of the same size (covers every pooled extent); a skip tensor with stride 12."""
    big = lambda: torch.zeros(1, 2, 6, 8, 12, device=device)
    return big(), big(), big(), big(), big()


def _rejected(fn):
    with pytest.raises(_clx().ClxError):
        fn()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("entry", ["clx_maxpool_fwd", "clx_maxpool_bwd", "clx_upsample_bwd"])
def test_rejects_a_factor_of_zero(entry, axis, device):
    x, y, dy, sk, dx = _pool_bufs(device)
    f = [2, 2, 2]
    f[axis] = 0
    if entry == "clx_maxpool_fwd":
        _rejected(lambda: _call(entry, device, x, y, 1, 2, 6, 8, 8, *f))
    elif entry == "clx_maxpool_bwd":
        _rejected(lambda: _call(entry, device, x, y, dy, None, 0, 0, 0, 0, 0, 0, 0, dx, 1, 2, 6, 8, 8, *f))
        _rejected(lambda: _call(entry, device, x, y, dy, sk, 8, 1, 1, 1, 0, 0, 0, dx, 1, 2, 6, 8, 8, *f))
    else:
        _rejected(lambda: _call(entry, device, sk, 12, 0, 2, 6, 8, 0, 0, 0, y, dx, 1, 1, 3, 4, 8, *f))


def test_rejects_an_extent_the_factor_does_not_divide(device):
    x, y, dy, sk, dx = _pool_bufs(device)
    for D, H, W, f in ((2, 5, 8, (1, 2, 2)), (2, 6, 7, (1, 2, 2)), (1, 6, 8, (2, 2, 2)), (2, 6, 8, (1, 4, 2))):
        _rejected(lambda: _call("clx_maxpool_fwd", device, x, y, 1, D, H, W, 8, *f))
        _rejected(lambda: _call("clx_maxpool_bwd", device, x, y, dy, None, 0, 0, 0, 0, 0, 0, 0, dx, 1, D, H, W, 8, *f))


def test_rejects_channel_counts_and_strides_it_cannot_vectorise(device):
    x, y, dy, sk, dx = _pool_bufs(device)
    f = (1, 2, 2)
    # C % 4 != 0
    _rejected(lambda: _call("clx_maxpool_fwd", device, x, y, 1, 2, 6, 8, 6, *f))
    _rejected(lambda: _call("clx_maxpool_bwd", device, x, y, dy, None, 0, 0, 0, 0, 0, 0, 0, dx, 1, 2, 6, 8, 6, *f))
    _rejected(lambda: _call("clx_upsample_bwd", device, sk, 12, 0, 2, 6, 8, 0, 0, 0, y, dx, 1, 2, 3, 4, 6, *f))
    # ld_skip < C
    _rejected(lambda: _call("clx_maxpool_bwd", device, x, y, dy, sk, 4, 1, 2, 2, 0, 1, 1, dx, 1, 2, 6, 8, 8, *f))
    # coff + C > ld_cat; coff % 4 != 0
    _rejected(lambda: _call("clx_upsample_bwd", device, sk, 8, 4, 2, 6, 8, 0, 0, 0, y, dx, 1, 2, 3, 4, 8, *f))
    _rejected(lambda: _call("clx_upsample_bwd", device, sk, 12, 2, 2, 6, 8, 0, 0, 0, y, dx, 1, 2, 3, 4, 8, *f))
    # the accepted neighbours of the calls above go through (the rejections are not an accident of these buffers)
    _call("clx_maxpool_bwd", device, x, y, dy, sk, 8, 1, 2, 2, 0, 1, 1, dx, 1, 2, 6, 8, 8, *f)
    _call("clx_upsample_bwd", device, sk, 12, 4, 2, 6, 8, 0, 0, 0, y, dx, 1, 2, 3, 4, 8, *f)


@pytest.mark.parametrize("entry", ["clx_depth_to_space", "clx_space_to_depth"])
def test_subpixel_pair_rejects_bad_channel_counts_and_strides(entry, device):
    lo = torch.zeros(1, 1, 3, 5, 36, device=device)          # P = 4 phases of up to 8 channels, and 4 spare lanes
    hi = torch.zeros(1, 1, 6, 10, 12, device=device)
    a, b = (lo, hi) if entry == "clx_depth_to_space" else (hi, lo)
    lds = (lambda ld_lo, ld_hi: (ld_lo, ld_hi)) if entry == "clx_depth_to_space" else (lambda ld_lo, ld_hi: (ld_hi, ld_lo))

    def run(ld_lo, ld_hi, N, f=(1, 2, 2)):
        l0, l1 = lds(ld_lo, ld_hi)
        _call(entry, device, a, l0, b, l1, 1, 1, 3, 5, N, *f)

    _rejected(lambda: run(36, 12, 6))                         # N % 4 != 0
    _rejected(lambda: run(12, 12, 4))                         # ld_lo < P N
    _rejected(lambda: run(28, 12, 8))
    _rejected(lambda: run(32, 4, 8))                          # ld_hi < N
    _rejected(lambda: run(32, 12, 8, (1, 0, 2)))              # a factor of 0
    run(32, 12, 8)
