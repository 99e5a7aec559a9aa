"""The train-step tail (csrc/loss.hip) through the C ABI, each entry point against a plain NumPy float64 restatement of
what include/clx.h says it computes: clx_gather_add_fwd / _bwd, clx_oce_loss_fwd_bwd, clx_oce_pairs_fused and its
reproducible form clx_oce_pairs_fused_det, clx_adam_step / clx_adam_step_guarded, clx_sample_pairs.

Two regimes of input.

EXACT: the embedding at a pixel is one of the 2 ND axis vectors +-8 e_c (chosen by a hash of the pixel index), T = 0.5,
w = 2^-10.  Then |a| = 8, w / |a| = 2^-13, reg = 2^-7 per pair, d^2 is 0, 128 or 256, exp(-d^2 / T) is exactly 1 or
underflows to exactly 0, the gradient is +-2^-10 on the class axis and 0 elsewhere: every float32 intermediate is exact
(asserted on the NumPy float32 restatement below before the kernel is looked at), so sums and gradients are compared
with `==` whatever order the atomics arrive in.  sums[1] is the integer count of pairs whose classes differ: one pair
dropped or doubled by a grid-stride loop changes it by 1.  Every pair-taking entry point runs this regime at B P = 1,
255, 256, 257, 3000 and 600 000 (above the cap of 1024 blocks x 256 threads: 2.3 trips per thread).

GENERAL: continuous inputs against float64 under ABSOLUTE bars derived by first-order error propagation, written where
they are used (_pair_bars, _adam_bars), with u = 2^-24, 1 ulp = 2 u allowed per add / multiply / divide / sqrt, 2 ulp
= 4 u for expf, u for a host scalar converted to float32, and a fused multiply-add only removing roundings.  No bar is
taken from what the kernels give.  Each test also asserts that the NumPy float32 restatement stays below HALF of the
bar on its own inputs, and prints the largest fraction of the bar that the kernel and the restatement use.  Largest
fractions observed on an MI355X (kernel / float32 restatement) are recorded next to each bar.

Conventions of tests/test_gpu_glue.py: outputs that are overwritten start as NaN, outputs that are added to start as
zero, every float buffer a call may write sits between NaN canary lanes that are checked afterwards, Adam is also handed
pointers at odd float offsets into larger buffers.  Rejected calls get real device buffers large enough for the extents
they name.

Not pinned here: NaN / Inf embeddings, a negative temperature (accepted by clx_oce_loss_fwd_bwd and
clx_oce_pairs_fused, rejected by the reproducible form), and |coordinate| > 2^24, where (float)coord rounds.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -24            # unit roundoff of float32
FLUSH = 2.0 ** -126       # smallest normal float32: what an expf that flushes a subnormal result to zero loses
TINY = 2.0 ** -149        # smallest subnormal float32: the absolute error of one rounding below the normal range
GUARD = 64                # canary lanes in front of and behind every guarded buffer


def _clx():
    from cellulus_amd import _clx

    return _clx


def _call(name, device, *args):
    c = _clx()
    c.call(name, *[c.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], c.stream_ptr(device))


def _rejected(fn):
    with pytest.raises(_clx().ClxError):
        fn()


def _guard(host, device, odd=0):
    """host array -> (buf, view): a device buffer of NaN with `host` at float offset GUARD + odd inside it."""
    t = torch.from_numpy(np.ascontiguousarray(host))
    n = t.numel()
    buf = torch.full((GUARD + odd + n + GUARD,), NAN, dtype=t.dtype, device=device)
    view = buf[GUARD + odd: GUARD + odd + n].view(t.shape)
    view.copy_(t)
    return buf, view


def _intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool(torch.isnan(buf[:lo]).all() and torch.isnan(buf[lo + view.numel():]).all())


def _frac(err, bar):
    """Largest fraction of the bar that err uses (inf where the bar is 0 and the error is not)."""
    err, bar = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bar, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    assert not np.isnan(f).any()
    return float(f.max()) if f.size else 0.0


def _check(what, got, ref, bar, restated):
    """|got - ref| <= bar everywhere, |restated - ref| <= bar / 2 everywhere; -> the two fractions, printed."""
    fk, fr = _frac(np.abs(got - ref), bar), _frac(np.abs(restated - ref), bar)
    print(f"{what}: kernel {fk:.3f} of the bar, float32 restatement {fr:.3f}")
    assert fr <= 0.5, (what, fr)
    assert fk <= 1.0, (what, fk)
    return fk, fr


# ------------------------------------------------------------------------------------------------
# shapes, coordinates
# ------------------------------------------------------------------------------------------------
# (B, P): one pair; the block edge (255 with more than one batch row); heavy duplication per pixel; above the grid cap
SHAPES = [(1, 1), (3, 85), (1, 256), (1, 257), (3, 1000), (3, 200_000)]
SHAPE_IDS = ["1", "255", "256", "257", "3x1000", "above_cap"]
ABOVE_CAP = SHAPES[-1]
TW = [(10.0, 1e-5), (0.5, 1e-5), (1e4, 1e-2), (10.0, 0.0)]
BIG = 2 ** 40


def _dims(nd, shape):
    if shape == ABOVE_CAP:
        return (1, 24, 28) if nd == 2 else (6, 8, 10)
    return (1, 9, 11) if nd == 2 else (5, 6, 7)


def _sizes(nd, dims):
    """Extent indexed by coordinate column c: column 0 is the LAST spatial axis."""
    return np.array([dims[2], dims[1], dims[0]][:nd], dtype=np.int64)


def _pixel(co, nd, dims):
    """(…, ND) coordinates -> linear pixel index with the reference's index rules; -1 where it raises IndexError."""
    size = _sizes(nd, dims)
    with np.errstate(over="ignore"):
        c = np.where(co < 0, co + size, co)
    ok = ((c >= 0) & (c < size)).all(-1)
    c = np.where(ok[..., None], c, 0)
    idx = c[..., 0] + dims[2] * c[..., 1]
    if nd == 3:
        idx = idx + dims[2] * dims[1] * c[..., 2]
    return np.where(ok, idx, -1)


def _pixel_coords(nd, dims):
    """(npix, ND): the non-negative coordinate row of every pixel."""
    pix = np.arange(dims[0] * dims[1] * dims[2], dtype=np.int64)
    cols = [pix % dims[2], (pix // dims[2]) % dims[1], pix // (dims[2] * dims[1])]
    return np.stack(cols[:nd], axis=-1)


def _pairs(rng, B, P, nd, dims):
    """Anchors repeated 8 times in a row (as np.repeat of the sampled anchors gives), references within +-3."""
    size = _sizes(nd, dims)
    base = rng.integers(0, size, size=(B, -(-P // 8), nd))
    a = np.repeat(base, 8, axis=1)[:, :P]
    r = np.clip(a + rng.integers(-3, 4, size=a.shape), 0, size - 1)
    return np.ascontiguousarray(a, dtype=np.int64), np.ascontiguousarray(r, dtype=np.int64)


def _wrap(rng, co, nd, dims):
    """The same pixels, about a third of the coordinates written as -n..-1."""
    return np.where(rng.random(co.shape) < 0.3, co - _sizes(nd, dims), co)


def _bad_values(n):
    return [n, -n - 1, BIG, -BIG, -2 ** 63, 2 ** 63 - 1]


def _plant_bad(co, nd, dims, rows, shift=0):
    """Writes one out-of-range value into each of the given flat rows, rotating over values and columns."""
    flat = co.reshape(-1, nd)
    assert np.shares_memory(flat, co)
    size = _sizes(nd, dims)
    for k, row in enumerate(rows):
        c = (k + shift) % nd
        flat[row, c] = _bad_values(int(size[c]))[(k + 3 * shift) % 6]


def _dev_i64(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------------------------------------
# the pair formula (include/clx.h, clx_oce_loss_fwd_bwd): float64 reference, float32 restatement, bars
# ------------------------------------------------------------------------------------------------
def _pair_f64(a, r, T, w):
    """d = |a - r|, oce = 1 - exp(-d^2 / T), reg = w |a|, da = (2 / T) exp(-d^2 / T) (a - r) + w a / |a| (0 at norm 0)"""
    diff = a - r
    e = np.exp(-(diff * diff).sum(1) / T)
    nrm = np.sqrt((a * a).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = np.where(nrm[:, None] > 0, a / nrm[:, None], 0.0)
    return 1.0 - e, w * nrm, (2.0 / T) * e[:, None] * diff + w * unit


def _pair_f32(a, r, T, w):
    """The same in float32, one rounding per operation, in the order the formulas are written."""
    a, r, T, w = a.astype(np.float32), r.astype(np.float32), np.float32(T), np.float32(w)
    diff = a - r
    s, na = np.zeros(len(a), np.float32), np.zeros(len(a), np.float32)
    for c in range(a.shape[1]):
        s = s + diff[:, c] * diff[:, c]
        na = na + a[:, c] * a[:, c]
    d = np.sqrt(s)
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        e = np.exp(-(d * d) / T)
        nrm = np.sqrt(na)
        k = np.float32(2) * e / T
        inv = np.where(nrm > 0, w / nrm, np.float32(0)).astype(np.float32)
        g = k[:, None] * diff + inv[:, None] * a
    assert g.dtype == np.float32 and e.dtype == np.float32
    return np.float32(1) - e, w * nrm, g


def _pair_bars(a, r, T, w, alpha=0.0, rho=0.0):
    """Absolute bars on (oce, reg, da) of one pair, first order, from the float64 values.  alpha, rho: absolute errors
    the components of a and r arrive with (0 when they are the kernel's inputs, 2 u |a_c| when the kernel first adds
    the coordinate to the offset).  With x = d^2 / T, e = exp(-x), k = 2 e / T:

      diff_c = a_c - r_c                 D_c = alpha_c + rho_c + 2u |diff_c|
      s = sum diff_c^2                   ND squares and ND - 1 additions of positive terms: 2u ND s + sum 2 |diff_c| D_c
      d = sqrt(s); d d; / T              relative ds / s + (2 + 2 + 2 + 2) u, so with I = sum 2 |diff_c| (alpha_c + rho_c) / T
                                         dx = I + (2 ND + 12) u x
      e = expf(-x)                       de = e dx + 4u e + FLUSH
      oce = 1 - e                        d oce = de + 2u oce                         = u (4 e + 2 oce + (2 ND + 12) x e) + e I
      |a| = sqrt(sum a_c^2), reg = w |a| d reg = w |a| ((ND + 4) u + J),  J = sum |a_c| alpha_c / |a|^2
      k = 2 e / T                        dk = k (dx + 6u) + 2 FLUSH / T
      k diff_c                           k |diff_c| (dx + 10u) + k (alpha_c + rho_c) + 2 FLUSH |diff_c| / T
      (w / |a|) a_c                      w (|a_c| / |a|) ((ND + 6) u + J) + w alpha_c / |a|
      their sum                          2u (k |diff_c| + w |a_c| / |a|)
      da_c                               u [((2 ND + 12) x + 12) k |diff_c| + (ND + 8) w |a_c| / |a|] + the alpha / rho / FLUSH terms

    T and w are the float32 values the kernel receives, so they carry no error.
    Largest fractions observed, kernel / float32 restatement -- clx_oce_loss_fwd_bwd: summed oce 0.146 / 0.146,
    summed reg 0.011 / 0.009, da 0.328 / 0.328 (the kernel and the restatement differ in the fourth digit at most).
    """
    nd = a.shape[1]
    alpha, rho = np.broadcast_to(alpha, a.shape), np.broadcast_to(rho, a.shape)
    diff = a - r
    ad = np.abs(diff)
    x = (diff * diff).sum(1) / T
    e = np.exp(-x)
    oce = 1.0 - e
    inflow = (2.0 * ad * (alpha + rho)).sum(1) / T
    dx = inflow + (2 * nd + 12) * U * x
    bar_oce = e * dx + U * (4.0 * e + 2.0 * oce) + FLUSH
    na = (a * a).sum(1)
    nrm = np.sqrt(na)
    with np.errstate(divide="ignore", invalid="ignore"):
        J = np.where(na > 0, (np.abs(a) * alpha).sum(1) / na, 0.0)
        unit = np.where(nrm[:, None] > 0, np.abs(a) / nrm[:, None], 0.0)
        a_in = np.where(nrm[:, None] > 0, alpha / nrm[:, None], 0.0)
    bar_reg = w * nrm * ((nd + 4) * U + J)
    k = 2.0 * e / T
    bar_g = (k[:, None] * ad * (dx + 12.0 * U)[:, None] + k[:, None] * (alpha + rho) + 2.0 * FLUSH * ad / T
             + w * unit * ((nd + 8) * U + J)[:, None] + w * a_in)
    return bar_oce, bar_reg, bar_g


def _classes(B, npix, nd):
    """Class 0 .. 2 ND - 1 of every pixel: a multiplicative hash of its index."""
    i = np.arange(B * npix, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    return (h % np.uint64(2 * nd)).astype(np.int64).reshape(B, npix)


def _axis_vectors(cls, nd):
    """class -> +-8 e_c as float32 (..., ND)"""
    E = np.zeros(cls.shape + (nd,), np.float32)
    np.put_along_axis(E, (cls // 2)[..., None], (8.0 * (1 - 2 * (cls % 2)))[..., None].astype(np.float32), axis=-1)
    return E


EXACT_T, EXACT_W = 0.5, 2.0 ** -10


def _exact_pair_values(ca, cr, nd):
    """(oce, reg, da) of pairs with anchor class ca and reference class cr; asserts that the float32 restatement
    reproduces them exactly, that is, that no float32 intermediate of the formula rounds for these constants."""
    oce = (ca != cr).astype(np.float64)
    reg = np.full(len(ca), 2.0 ** -7)
    g = _axis_vectors(ca, nd).astype(np.float64) * 2.0 ** -13
    o32, r32, g32 = _pair_f32(_axis_vectors(ca, nd), _axis_vectors(cr, nd), EXACT_T, EXACT_W)
    assert np.array_equal(o32, oce) and np.array_equal(r32, reg) and np.array_equal(g32, g)
    return oce, reg, g


# ------------------------------------------------------------------------------------------------
# 1. clx_gather_add_fwd, clx_gather_add_bwd
# ------------------------------------------------------------------------------------------------
def _gather_case(nd, shape, seed):
    B, P = shape
    dims = _dims(nd, shape)
    rng = np.random.default_rng(seed)
    npix = dims[0] * dims[1] * dims[2]
    co, _ = _pairs(rng, B, P, nd, dims)
    co = _wrap(rng, co, nd, dims)
    if B * P >= 255:
        # every value of -n..-1 and of 0..n-1 on every axis
        size = _sizes(nd, dims)
        flat = co.reshape(-1, nd)
        for c in range(nd):
            vals = np.arange(-size[c], size[c])
            flat[10 + 30 * c: 10 + 30 * c + len(vals), c] = vals
    bad_rows = []
    if B * P >= 255:
        bad_rows = [0, 100, 101, B * P - 1, 128, 200, 64, 65, 253, 130, 131, 132]
        _plant_bad(co, nd, dims, bad_rows)
    idx = _pixel(co, nd, dims)
    assert ((idx < 0).reshape(-1).nonzero()[0].tolist() == sorted(bad_rows))
    offsets = rng.standard_normal((B, nd, npix)).astype(np.float32)
    return B, P, dims, npix, co, idx, offsets, len(bad_rows)


@pytest.mark.parametrize("count", [True, False], ids=["oob_count", "oob_null"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("nd", [2, 3])
def test_gather_add_fwd(nd, shape, count, device):
    """sel = offsets[pixel] + (float)coord, one float32 addition: exact against NumPy float32.  The RAW coordinate is
    what is added (negative where it wrapped).  A bad row is NaN, counted, and nothing else changes."""
    B, P, dims, npix, co, idx, offsets, nbad = _gather_case(nd, shape, 10 + nd)
    good = idx >= 0
    ref = np.full((B, P, nd), np.nan, np.float32)
    bsel = np.broadcast_to(np.arange(B)[:, None], (B, P))
    for c in range(nd):
        ref[..., c][good] = offsets[bsel[good], c, idx[good]] + co[..., c][good].astype(np.float32)
    obuf, off = _guard(offsets, device)
    sbuf, sel = _guard(np.full((B, P, nd), np.nan, np.float32), device)
    oob = torch.zeros(3, dtype=torch.int32, device=device)
    _call("clx_gather_add_fwd", device, off, _dev_i64(co, device), sel, B, P, nd, *dims, oob[1:] if count else None)
    got = sel.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isnan(got).all(-1), ~good) and np.array_equal(np.isnan(got).any(-1), ~good)
    assert np.array_equal(got[good], ref[good])
    assert oob.cpu().tolist() == [0, nbad if count else 0, 0]
    assert _intact(sbuf, sel) and _intact(obuf, off)
    if B * P >= 255:
        assert (co < 0).any() and nbad == 12


@pytest.mark.parametrize("count", [True, False], ids=["oob_count", "oob_null"])
@pytest.mark.parametrize("kind", ["ints", "randn"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("nd", [2, 3])
def test_gather_add_bwd(nd, shape, kind, count, device):
    """doffsets[pixel] += dsel.  Integer-valued dsel in {-3..3}: every partial sum is a small integer, so the float
    atomics are exact in any order.  Continuous dsel: m float32 additions in an unknown order, each off by at most
    u |partial sum| <= u sum |dsel_i|: |got - ref64| <= u m sum |dsel_i| per pixel (the last, m-th, u covers the
    conversion of the float64 reference's own value to what a float32 can hold).
    Largest fraction observed, kernel / sequential float32 restatement: 0.469 / 0.469."""
    B, P, dims, npix, co, idx, _, nbad = _gather_case(nd, shape, 20 + nd)
    rng = np.random.default_rng(5)
    if kind == "ints":
        dsel = rng.integers(-3, 4, size=(B, P, nd)).astype(np.float32)
    else:
        dsel = rng.standard_normal((B, P, nd)).astype(np.float32)
    good = (idx >= 0).reshape(-1)
    bsel = np.repeat(np.arange(B), P)
    n = B * nd * npix
    ref, mass, m, seq = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.float32)
    for c in range(nd):
        lin = (bsel * nd + c) * npix + idx.reshape(-1)
        val = dsel[..., c].reshape(-1)
        ref += np.bincount(lin[good], weights=val[good].astype(np.float64), minlength=n)
        mass += np.bincount(lin[good], weights=np.abs(val[good]).astype(np.float64), minlength=n)
        m += np.bincount(lin[good], minlength=n)
        np.add.at(seq, lin[good], val[good])
    dbuf, doff = _guard(np.zeros((B, nd, npix), np.float32), device)
    oob = torch.zeros(3, dtype=torch.int32, device=device)
    _call("clx_gather_add_bwd", device, torch.from_numpy(dsel).to(device), _dev_i64(co, device),
          doff, B, P, nd, *dims, oob[1:] if count else None)
    got = doff.cpu().numpy().reshape(-1).astype(np.float64)
    if kind == "ints":
        assert np.array_equal(got, ref) and np.array_equal(seq, ref)
    else:
        _check(f"gather_add_bwd nd={nd} {shape}", got, ref, U * m * mass, seq.astype(np.float64))
    assert oob.cpu().tolist() == [0, nbad if count else 0, 0]
    assert _intact(dbuf, doff)


@pytest.mark.parametrize("nd", [2, 3])
def test_gather_add_with_no_pairs_touches_nothing(nd, device):
    dims = _dims(nd, (1, 1))
    npix = dims[0] * dims[1] * dims[2]
    buf, t = _guard(np.full((2, nd, npix), np.nan, np.float32), device)
    sbuf, sel = _guard(np.full((2, 4, nd), np.nan, np.float32), device)
    co = torch.zeros(2, 4, nd, dtype=torch.int64, device=device)
    oob = torch.zeros(1, dtype=torch.int32, device=device)
    _call("clx_gather_add_fwd", device, t, co, sel, 2, 0, nd, *dims, oob)
    _call("clx_gather_add_bwd", device, sel, co, t, 2, 0, nd, *dims, oob)
    assert torch.isnan(buf).all() and torch.isnan(sbuf).all() and oob.item() == 0


# ------------------------------------------------------------------------------------------------
# 2. clx_oce_loss_fwd_bwd
# ------------------------------------------------------------------------------------------------
def _run_loss(device, a, r, nd, T, w, gs, with_da=True, sums0=None):
    """-> (sums[0:3], da or None); sums[3] and the lanes around every buffer are canaries."""
    n = len(a)
    abuf, ad = _guard(a, device)
    rbuf, rd = _guard(r, device)
    dbuf, da = _guard(np.full((max(n, 1), nd), np.nan, np.float32), device)
    init = np.array([0.0, 0.0, 0.0, np.nan]) if sums0 is None else np.append(sums0, np.nan)
    sbuf, sums = _guard(init, device)
    _call("clx_oce_loss_fwd_bwd", device, ad, rd, da if with_da else None, sums, n, nd, T, w, gs)
    s = sums.cpu().numpy()
    assert np.isnan(s[3]) and _intact(sbuf, sums) and _intact(dbuf, da) and _intact(abuf, ad) and _intact(rbuf, rd)
    if not with_da:
        assert torch.isnan(da).all()
    return s[:3], (da.cpu().numpy()[:n] if with_da else None)


@pytest.mark.parametrize("npairs", [1, 255, 256, 257, 3000, 600_000])
@pytest.mark.parametrize("nd", [2, 3])
def test_oce_loss_counts_every_pair_once(nd, npairs, device):
    """The exact regime: sums[1] is the number of pairs whose classes differ, sums[2] = n 2^-7, every da row is
    grad_scale times +-2^-10 on the anchor's axis."""
    rng = np.random.default_rng(30 + nd)
    ca, cr = rng.integers(0, 2 * nd, npairs), rng.integers(0, 2 * nd, npairs)
    cr[::3] = ca[::3]
    oce, reg, g = _exact_pair_values(ca, cr, nd)
    a, r = _axis_vectors(ca, nd), _axis_vectors(cr, nd)
    want = np.array([oce.sum() + reg.sum(), oce.sum(), reg.sum()])
    assert want[1] == (ca != cr).sum() and want[2] == npairs * 2.0 ** -7
    for gs in (1.0, 0.25):
        s, da = _run_loss(device, a, r, nd, EXACT_T, EXACT_W, gs)
        assert np.array_equal(s, want)
        assert not np.isnan(da).any()                      # every row of da was written
        assert np.array_equal(da, gs * g)
    s_fwd, _ = _run_loss(device, a, r, nd, EXACT_T, EXACT_W, 1.0, with_da=False)
    assert s_fwd.tobytes() == want.tobytes()               # da == NULL: the same sums, bit for bit
    s2, _ = _run_loss(device, a, r, nd, EXACT_T, EXACT_W, 1.0, sums0=want)
    assert np.array_equal(s2, 2 * want)                    # sums is ADDED to


def _general_pairs(rng, n, nd):
    """Embeddings randn 4, references anchor + randn 3; planted: a zero-norm anchor, anchor == reference, a pair so far
    apart that the exponential underflows."""
    a = (rng.standard_normal((n, nd)) * 4).astype(np.float32)
    r = (a + rng.standard_normal((n, nd)) * 3).astype(np.float32)
    a[0] = 0.0
    if n > 1:
        r[1] = a[1]
    if n > 2:
        r[2] = a[2] + np.float32(1000.0)
    return a, r


@pytest.mark.parametrize("npairs", [1, 255, 256, 257, 3000, 600_000])
@pytest.mark.parametrize("nd", [2, 3])
def test_oce_loss_general(nd, npairs, device):
    """Every row of every case against float64 under _pair_bars; the bar of a sum is the sum of its pairs' bars (the
    float64 accumulation of n terms adds n 2^-53 of the sum of magnitudes).  grad_scale multiplies da only: one more
    multiplication, 2u |gs da|, on the bar scaled by |gs|.  The case above the grid cap runs once."""
    rng = np.random.default_rng(40 + nd)
    a, r = _general_pairs(rng, npairs, nd)
    a64, r64 = a.astype(np.float64), r.astype(np.float64)
    cases = [(TW[0], 1.0)] if npairs == 600_000 else [(tw, gs) for tw in TW for gs in (1.0, 0.25)]
    for (T, w), gs in cases:
        T32, w32 = float(np.float32(T)), float(np.float32(w))
        oce, reg, g = _pair_f64(a64, r64, T32, w32)
        b_oce, b_reg, b_g = _pair_bars(a64, r64, T32, w32)
        o32, r32, g32 = _pair_f32(a, r, T, w)
        assert not np.isnan(g).any() and (a64[0] == 0).all()               # zero norm: no regulariser gradient, no NaN
        if npairs > 2:
            assert oce[1] == 0.0 and oce[2] == 1.0
        # the per-pair bars on the restatement (the kernel returns no per-pair loss terms)
        assert _frac(np.abs(o32 - oce), b_oce) <= 0.5 and _frac(np.abs(r32 - reg), b_reg) <= 0.5
        s, da = _run_loss(device, a, r, nd, T, w, gs)
        tag = f"oce_loss nd={nd} n={npairs} T={T} w={w} gs={gs}"
        acc = npairs * 2.0 ** -53
        _check(tag + " oce", s[1], oce.sum(), b_oce.sum() + acc * oce.sum(), o32.astype(np.float64).sum())
        _check(tag + " reg", s[2], reg.sum(), b_reg.sum() + acc * reg.sum(), r32.astype(np.float64).sum())
        _check(tag + " loss", s[0], oce.sum() + reg.sum(), (b_oce + b_reg).sum() + acc * (oce + reg).sum(),
               o32.astype(np.float64).sum() + r32.astype(np.float64).sum())
        assert not np.isnan(da).any()
        _check(tag + " da", da.astype(np.float64), gs * g, abs(gs) * b_g + 2 * U * np.abs(gs * g),
               (np.float32(gs) * g32).astype(np.float64))
        s_fwd, _ = _run_loss(device, a, r, nd, T, w, gs, with_da=False)
        _check(tag + " loss, forward only", s_fwd[0], oce.sum() + reg.sum(),
               (b_oce + b_reg).sum() + acc * (oce + reg).sum(), o32.astype(np.float64).sum() + r32.astype(np.float64).sum())


def test_oce_loss_edge_arguments(device):
    a, r = _general_pairs(np.random.default_rng(0), 8, 2)
    abuf, ad = _guard(a, device)
    rbuf, rd = _guard(r, device)
    dbuf, da = _guard(np.full((8, 2), np.nan, np.float32), device)
    sbuf, sums = _guard(np.full(4, np.nan), device)
    _call("clx_oce_loss_fwd_bwd", device, ad, rd, da, sums, 0, 2, 10.0, 1e-5, 1.0)       # no pairs: OK, nothing touched
    assert torch.isnan(dbuf).all() and torch.isnan(sbuf).all()
    _rejected(lambda: _call("clx_oce_loss_fwd_bwd", device, ad, rd, da, sums, 8, 2, 0.0, 1e-5, 1.0))
    _rejected(lambda: _call("clx_oce_loss_fwd_bwd", device, ad, rd, da, sums, 4, 4, 10.0, 1e-5, 1.0))
    _rejected(lambda: _call("clx_oce_loss_fwd_bwd", device, ad, rd, da, sums, -1, 2, 10.0, 1e-5, 1.0))
    assert torch.isnan(dbuf).all() and torch.isnan(sbuf).all()


# ------------------------------------------------------------------------------------------------
# 3. clx_oce_pairs_fused, clx_oce_pairs_fused_det
# ------------------------------------------------------------------------------------------------
FUSED = ["clx_oce_pairs_fused", "clx_oce_pairs_fused_det"]


class _FusedRun:
    """Device buffers of one fused call: offsets and doffsets between canaries, four sums, the scratch of the
    reproducible form filled with 0xFF bytes (the header: it need not be zeroed)."""

    def __init__(self, device, entry, offsets, anchor, reference, nd, dims):
        self.device, self.entry, self.nd, self.dims = device, entry, nd, dims
        self.det = entry.endswith("_det")
        self.B, self.P = anchor.shape[:2]
        self.npix = dims[0] * dims[1] * dims[2]
        self.obuf, self.off = _guard(offsets, device)
        self.a, self.r = _dev_i64(anchor, device), _dev_i64(reference, device)
        fill = np.nan if self.det else 0.0                 # overwritten | added to
        self.dbuf, self.doff = _guard(np.full(offsets.shape, fill, np.float32), device)
        self.sbuf, self.sums = _guard(np.zeros(4), device)
        nbytes = int(_clx().load().clx_oce_pairs_det_scratch_bytes(self.B, nd, self.npix))
        self.scratch = torch.full((nbytes + 8,), 0xFF, dtype=torch.uint8, device=device) if self.det else None

    def call(self, T, w, rows=None, scratch_offset=0):
        lo, hi = rows or (0, self.B)
        tail = (self.scratch[scratch_offset:],) if self.det else ()
        _call(self.entry, self.device, self.off[lo:hi], self.a[lo:hi], self.r[lo:hi], self.doff[lo:hi], self.sums,
              hi - lo, self.P, self.nd, *self.dims, T, w, *tail)
        return self

    def result(self):
        assert _intact(self.obuf, self.off) and _intact(self.dbuf, self.doff) and _intact(self.sbuf, self.sums)
        return self.doff.cpu().numpy().reshape(-1).astype(np.float64), self.sums.cpu().numpy()


def _plant_bad_pairs(anchor, reference, nd, dims):
    """Anchor only, reference only, both: 4 + 4 + 4 rows, each ONE bad pair.  -> their number"""
    n = anchor.shape[0] * anchor.shape[1]
    if n < 255:
        return 0
    _plant_bad(anchor, nd, dims, [3, 60, 129, n - 1])
    _plant_bad(reference, nd, dims, [5, 61, 127, n - 2])
    both = [7, 62, 128, n - 3]
    _plant_bad(anchor, nd, dims, both)
    _plant_bad(reference, nd, dims, both, shift=1)
    return 12


def _scatter(n, lin, val, good):
    """Float64 sum of val into n bins at lin, over the good rows."""
    return np.bincount(lin[good], weights=val[good], minlength=n)


def _lin(B, P, nd, npix, ia, c):
    return (np.repeat(np.arange(B), P) * nd + c) * npix + ia.reshape(-1)


def _exact_case(nd, B, P, dims):
    npix = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(50 + nd)
    anchor, reference = _pairs(rng, B, P, nd, dims)
    nbad = _plant_bad_pairs(anchor, reference, nd, dims)
    cls = _classes(B, npix, nd)
    # offsets[b, c, pix] = E_c(pix) - coord_c(pix): small integers, so offsets + (float)coord is exact
    offsets = (_axis_vectors(cls, nd) - _pixel_coords(nd, dims)[None].astype(np.float32)).transpose(0, 2, 1)
    ia, ir = _pixel(anchor, nd, dims), _pixel(reference, nd, dims)
    good = ((ia >= 0) & (ir >= 0))
    assert (~good).sum() == nbad
    rowb = np.broadcast_to(np.arange(B)[:, None], (B, P))
    ca = np.where(good, cls[rowb, np.maximum(ia, 0)], 0)
    cr = np.where(good, cls[rowb, np.maximum(ir, 0)], 0)
    oce, reg, g = _exact_pair_values(ca.reshape(-1), cr.reshape(-1), nd)
    gf = good.reshape(-1)
    per_row = np.stack([(oce + reg) * gf, oce * gf, reg * gf, (~gf).astype(np.float64)], 1).reshape(B, P, 4).sum(1)
    n = B * nd * npix
    doff = np.zeros(n)
    for c in range(nd):
        doff += _scatter(n, _lin(B, P, nd, npix, ia, c), g[:, c], gf)
    assert np.bincount((rowb * npix + ia)[good], minlength=B * npix).max() < 2 ** 14
    return dict(dims=dims, offsets=np.ascontiguousarray(offsets), anchor=anchor, reference=reference,
                per_row=per_row, doff=doff, nbad=nbad)


@pytest.fixture(scope="module")
def exact_data():
    """Exact-regime inputs and expected results per (nd, shape), shared by the two fused entry points."""
    cache = {}

    def get(nd, shape):
        if (nd, shape) not in cache:
            cache[(nd, shape)] = _exact_case(nd, shape[0], shape[1], _dims(nd, shape))
        return cache[(nd, shape)]

    yield get
    cache.clear()


@pytest.mark.parametrize("entry", FUSED)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("nd", [2, 3])
def test_fused_counts_every_pair_once(nd, shape, entry, device, exact_data):
    """The exact regime through gather, gather, loss, scatter: sums[1] counts the pairs whose classes differ, sums[3] the
    bad pairs (one each, whether the anchor, the reference or both are out of range), doffsets is 2^-10 times the signed
    number of good pairs anchored at the pixel.  Half batches through sliced pointers add up to the same sums exactly."""
    d = exact_data(nd, shape)
    B = shape[0]
    want = d["per_row"].sum(0)
    doff, sums = _FusedRun(device, entry, d["offsets"], d["anchor"], d["reference"], nd, d["dims"]).call(EXACT_T, EXACT_W).result()
    assert sums.tolist() == want.tolist()
    assert sums[3] == d["nbad"]
    assert np.array_equal(doff, d["doff"])
    if B == 3:
        run = _FusedRun(device, entry, d["offsets"], d["anchor"], d["reference"], nd, d["dims"])
        run.call(EXACT_T, EXACT_W, rows=(0, 1))
        _, first = run.result()
        assert first.tolist() == d["per_row"][0].tolist()
        doff2, sums2 = run.call(EXACT_T, EXACT_W, rows=(1, 3)).result()
        assert sums2.tolist() == want.tolist()
        assert np.array_equal(doff2, d["doff"])            # each half wrote (det) / added into (atomic) its own rows
        # ... and a second whole call ADDS to sums; doffsets doubles (atomic form) or is overwritten (reproducible form)
        doff3, sums3 = run.call(EXACT_T, EXACT_W).result()
        assert sums3.tolist() == (2 * want).tolist()
        assert np.array_equal(doff3, d["doff"] if run.det else 2 * d["doff"])


def test_fused_det_converts_every_pixel_of_a_large_grid(device):
    """The conversion pass of the reproducible form runs over B ND Z Y X elements with its own grid cap (2048 blocks of
    256): 2 x 520 x 512 = 532 480 elements take a second trip.  Every element of the NaN-prefilled doffsets is written."""
    d = _exact_case(2, 1, 20_000, (1, 520, 512))
    run = _FusedRun(device, "clx_oce_pairs_fused_det", d["offsets"], d["anchor"], d["reference"], 2, d["dims"])
    doff, sums = run.call(EXACT_T, EXACT_W).result()
    assert sums.tolist() == d["per_row"].sum(0).tolist()
    assert np.array_equal(doff, d["doff"])
    assert d["doff"][-1] == 0 and np.count_nonzero(d["doff"][2048 * 256:]) > 0


@pytest.fixture(scope="module")
def general_data():
    """General-regime inputs per (nd, shape): offsets randn 3 around the pixel's own coordinate (as a trained network's
    are), wrapped coordinates, bad pairs; planted pixels: an embedding of norm zero (offsets = -coord), an anchor that is
    its own reference, a pixel 1000 away from everything."""
    cache = {}

    def get(nd, shape):
        if (nd, shape) not in cache:
            B, P = shape
            dims = _dims(nd, shape)
            npix = dims[0] * dims[1] * dims[2]
            rng = np.random.default_rng(60 + nd)
            anchor, reference = _pairs(rng, B, P, nd, dims)
            pc = _pixel_coords(nd, dims)
            offsets = (rng.standard_normal((B, nd, npix)) * 3).astype(np.float32)
            zero_pix, far_pix = npix // 2, npix // 3
            offsets[:, :, zero_pix] = -pc[zero_pix].astype(np.float32)
            offsets[:, :, far_pix] = 1000.0
            # wrapping happens before anything is planted: it would move a planted embedding and could repair a bad pair
            anchor, reference = _wrap(rng, anchor, nd, dims), _wrap(rng, reference, nd, dims)
            anchor, reference = np.ascontiguousarray(anchor), np.ascontiguousarray(reference)
            flat_a, flat_r = anchor.reshape(-1, nd), reference.reshape(-1, nd)
            flat_a[0] = pc[zero_pix]                        # (with one pair, this is the pair)
            if B * P > 3:
                flat_r[1] = flat_a[1]
                flat_r[2] = pc[far_pix]
            nbad = _plant_bad_pairs(anchor, reference, nd, dims)
            cache[(nd, shape)] = dict(dims=dims, offsets=offsets, anchor=anchor, reference=reference, nbad=nbad)
        return cache[(nd, shape)]

    yield get
    cache.clear()


def _fused_reference(d, nd, T, w, rows=None):
    """Gather, gather, loss, scatter composed from the float64 restatement, with the bars of _pair_bars: the kernel's
    first operation, offsets + (float)coord, is one float32 addition, so a and r arrive with alpha = 2u |a|, rho = 2u |r|.

    doffsets, atomic form: the summed per-pair bars plus u m sum |g_i| for m float additions in an unknown order.
    Reproducible form: the summed per-pair bars, m 2^-41 for the m roundings to 2^-40 fixed point, and half an ulp of
    the result (u |result|) for the final conversion to float32.
    Largest fractions observed, kernel / float32 restatement -- clx_oce_pairs_fused: sums 0.101 / 0.336, doffsets
    0.267 / 0.266; clx_oce_pairs_fused_det: sums 0.101 / 0.336, doffsets 0.870 / 0.477 (a pixel with one tiny
    contribution: the rounding to 2^-40 fixed point may use all of its 2^-41; the restatement adds floats and has none).
    """
    anchor, reference, offsets, dims = d["anchor"], d["reference"], d["offsets"], d["dims"]
    if rows is not None:
        anchor, reference, offsets = anchor[rows[0]:rows[1]], reference[rows[0]:rows[1]], offsets[rows[0]:rows[1]]
    B, P = anchor.shape[:2]
    npix = dims[0] * dims[1] * dims[2]
    T32, w32 = float(np.float32(T)), float(np.float32(w))
    ia, ir = _pixel(anchor, nd, dims), _pixel(reference, nd, dims)
    good = ((ia >= 0) & (ir >= 0)).reshape(-1)
    rowb = np.repeat(np.arange(B), P)
    ja, jr = np.maximum(ia, 0).reshape(-1), np.maximum(ir, 0).reshape(-1)
    ca = np.where(good[:, None], anchor.reshape(-1, nd), 0)
    cr = np.where(good[:, None], reference.reshape(-1, nd), 0)
    oa = offsets[rowb[:, None], np.arange(nd)[None], ja[:, None]]
    orr = offsets[rowb[:, None], np.arange(nd)[None], jr[:, None]]
    a64, r64 = oa.astype(np.float64) + ca, orr.astype(np.float64) + cr
    a32, r32 = oa + ca.astype(np.float32), orr + cr.astype(np.float32)
    oce, reg, g = _pair_f64(a64, r64, T32, w32)
    b_oce, b_reg, b_g = _pair_bars(a64, r64, T32, w32, 2 * U * np.abs(a64), 2 * U * np.abs(r64))
    o32, g32r, g32 = _pair_f32(a32, r32, T, w)
    assert _frac(np.abs(o32 - oce), b_oce) <= 0.5 and _frac(np.abs(g32r - reg), b_reg) <= 0.5
    assert _frac(np.abs(g32 - g), b_g) <= 0.5
    n = B * nd * npix
    doff, bar_pairs, mass, m, seq = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.float32)
    for c in range(nd):
        lin = _lin(B, P, nd, npix, ja, c)
        doff += _scatter(n, lin, g[:, c], good)
        bar_pairs += _scatter(n, lin, b_g[:, c], good)
        mass += _scatter(n, lin, np.abs(g[:, c]), good)
        m += np.bincount(lin[good], minlength=n)
        np.add.at(seq, lin[good], g32[good, c])
    acc = good.sum() * 2.0 ** -53
    so, sr = oce[good].sum(), reg[good].sum()
    sums = np.array([so + sr, so, sr, (~good).sum()])
    sums_bar = np.array([(b_oce + b_reg)[good].sum() + acc * (so + sr), b_oce[good].sum() + acc * so,
                         b_reg[good].sum() + acc * sr, 0.0])
    s32 = np.array([o32[good].astype(np.float64).sum() + g32r[good].astype(np.float64).sum(),
                    o32[good].astype(np.float64).sum(), g32r[good].astype(np.float64).sum(), (~good).sum()])
    return dict(sums=sums, sums_bar=sums_bar, sums32=s32, doff=doff, seq=seq.astype(np.float64),
                bar_atomic=bar_pairs + U * m * mass, bar_det=bar_pairs + m * 2.0 ** -41 + U * np.abs(doff),
                g=g, a64=a64, good=good)


@pytest.mark.parametrize("entry", FUSED)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("nd", [2, 3])
def test_fused_general(nd, shape, entry, device, general_data):
    """Every (T, w) case (the one above the grid cap: the first) against the composed float64 restatement; the planted
    pixels; half batches; a random permutation of the pairs within each batch row -- bit-identical doffsets for the
    reproducible form (the point of the fixed-point scatter), inside the same bar for the atomic form."""
    d = general_data(nd, shape)
    B, P = shape
    det = entry.endswith("_det")
    for T, w in (TW[:1] if shape == ABOVE_CAP else TW):
        ref = _fused_reference(d, nd, T, w)
        assert not np.isnan(ref["g"]).any() and (ref["a64"][0] == 0).all()     # the planted zero-norm embedding
        bar = ref["bar_det"] if det else ref["bar_atomic"]
        tag = f"{entry} nd={nd} {shape} T={T} w={w}"
        doff, sums = _FusedRun(device, entry, d["offsets"], d["anchor"], d["reference"], nd, d["dims"]).call(T, w).result()
        assert sums[3] == d["nbad"] == ref["sums"][3]
        _check(tag + " sums", sums, ref["sums"], ref["sums_bar"], ref["sums32"])
        _check(tag + " doffsets", doff, ref["doff"], bar, ref["seq"])
        if shape == ABOVE_CAP or shape == (3, 1000) and (T, w) == TW[0]:
            # the pairs of each batch row in another order
            perm = np.stack([np.random.default_rng(7 + b).permutation(P) for b in range(B)])
            pa = np.take_along_axis(d["anchor"], perm[..., None], axis=1)
            pr = np.take_along_axis(d["reference"], perm[..., None], axis=1)
            doff_p, sums_p = _FusedRun(device, entry, d["offsets"], pa, pr, nd, d["dims"]).call(T, w).result()
            assert sums_p[3] == d["nbad"]
            _check(tag + " sums, permuted", sums_p, ref["sums"], ref["sums_bar"], ref["sums32"])
            _check(tag + " doffsets, permuted", doff_p, ref["doff"], bar, ref["seq"])
            if det:
                assert doff_p.tobytes() == doff.tobytes()
        if B == 3 and (T, w) == TW[0]:
            run = _FusedRun(device, entry, d["offsets"], d["anchor"], d["reference"], nd, d["dims"])
            run.call(T, w, rows=(0, 1))
            _, first = run.result()
            half = _fused_reference(d, nd, T, w, rows=(0, 1))
            _check(tag + " sums, rows [0:1]", first, half["sums"], half["sums_bar"], half["sums32"])
            doff2, sums2 = run.call(T, w, rows=(1, 3)).result()
            _check(tag + " sums, half batches", sums2, ref["sums"], ref["sums_bar"], ref["sums32"])
            _check(tag + " doffsets, half batches", doff2, ref["doff"], bar, ref["seq"])
            if det:
                assert doff2.tobytes() == doff.tobytes()


@pytest.mark.parametrize("nd", [2, 3])
def test_fused_edge_arguments(nd, device, general_data):
    d = general_data(nd, (3, 85))
    dims = d["dims"]
    # no pairs: the atomic form touches nothing; the reproducible form overwrites doffsets with zeros, sums unchanged
    for entry in FUSED:
        run = _FusedRun(device, entry, d["offsets"], d["anchor"], d["reference"], nd, dims)
        run.sums.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5], dtype=torch.float64))
        run.P = 0
        run.doff.fill_(NAN)
        doff, sums = run.call(10.0, 1e-5).result()
        assert sums.tolist() == [1.5, 2.5, 3.5, 4.5]
        assert (doff == 0).all() if run.det else np.isnan(doff).all()
    # rejected: T = 0 by both, T < 0 and a misaligned scratch by the reproducible form, bad extents by both
    for entry in FUSED:
        run = _FusedRun(device, entry, d["offsets"], d["anchor"], d["reference"], nd, dims)
        before = run.dbuf.clone()
        _rejected(lambda: run.call(0.0, 1e-5))
        if run.det:
            _rejected(lambda: run.call(-10.0, 1e-5))
            _rejected(lambda: run.call(10.0, 1e-5, scratch_offset=4))
        run.nd = 4
        _rejected(lambda: run.call(10.0, 1e-5))
        run.nd = nd
        run.dims = (dims[0], 0, dims[2])
        _rejected(lambda: run.call(10.0, 1e-5))
        run.dims = dims
        assert run.dbuf.view(torch.int32).equal(before.view(torch.int32)) and (run.sums == 0).all()
        run.call(10.0, 1e-5, scratch_offset=8 if run.det else 0)         # the accepted neighbour goes through
        assert run.result()[1][3] == d["nbad"]


def test_two_dimensional_calls_require_a_single_plane(device):
    """ND == 2 with Z != 1 is rejected by all four entry points that take a grid (with a plane stride of Z Y X and
    plane 0 alone indexed, such a call has no meaning).  The buffers cover Z Y X pixels, as the call claims."""
    B, P, Z, Y, X = 2, 16, 3, 5, 6
    off = torch.zeros(B, 2, Z * Y * X, device=device)
    doff = torch.zeros(B, 2, Z * Y * X, device=device)
    sel = torch.zeros(B, P, 2, device=device)
    co = torch.zeros(B, P, 2, dtype=torch.int64, device=device)
    sums = torch.zeros(4, dtype=torch.float64, device=device)
    oob = torch.zeros(1, dtype=torch.int32, device=device)
    nbytes = int(_clx().load().clx_oce_pairs_det_scratch_bytes(B, 2, Z * Y * X))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def calls(z):
        return [lambda: _call("clx_gather_add_fwd", device, off, co, sel, B, P, 2, z, Y, X, oob),
                lambda: _call("clx_gather_add_bwd", device, sel, co, doff, B, P, 2, z, Y, X, oob),
                lambda: _call("clx_oce_pairs_fused", device, off, co, co, doff, sums, B, P, 2, z, Y, X, 10.0, 1e-5),
                lambda: _call("clx_oce_pairs_fused_det", device, off, co, co, doff, sums, B, P, 2, z, Y, X, 10.0, 1e-5,
                              scratch)]

    for fn in calls(Z):
        _rejected(fn)
    assert (sums == 0).all() and (doff == 0).all() and (sel == 0).all()
    for fn in calls(1):
        fn()
    for fn in calls(0):
        _rejected(fn)


# ------------------------------------------------------------------------------------------------
# 4. clx_adam_step, clx_adam_step_guarded
# ------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _adam_f64(p, g, m, v, step, wd):
    """include/clx.h / csrc/loss.hip: g += wd p; m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g g;
    denom = sqrt(v) / sqrt(bc2) + eps; p -= (lr / bc1) m / denom, with bc_i = 1 - b_i^step."""
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    gv = g + wd * p
    m2 = m + (1.0 - B1) * (gv - m)
    v2 = B2 * v + (1.0 - B2) * gv * gv
    den = np.sqrt(v2) / np.sqrt(bc2) + EPS
    return p - (LR / bc1) * (m2 / den), m2, v2


def _adam_f32(p, g, m, v, step, wd):
    f = np.float32
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    c1, b2, c2, eps, wd, ss, sq = f(1.0 - B1), f(B2), f(1.0 - B2), f(EPS), f(wd), f(LR / bc1), f(np.sqrt(bc2))
    gv = g + wd * p
    m2 = m + c1 * (gv - m)
    v2 = b2 * v + c2 * gv * gv
    den = np.sqrt(v2) / sq + eps
    p2 = p - ss * (m2 / den)
    assert p2.dtype == np.float32 and v2.dtype == np.float32
    return p2, m2, v2


def _adam_bars(p, g, m, v, step, wd, u=U, tiny=TINY, dp0=0.0, dm0=0.0, dv0=0.0):
    """Absolute bars (dp, dm, dv) of one step from the float64 values; dp0, dm0, dv0: the errors the state arrives with
    (a trajectory).  op = 2u per operation, u per host scalar converted to float32 (1 - b1, b2, 1 - b2, lr / bc1,
    sqrt(bc2), eps, wd), `tiny` per operation on v (g g of a gradient of 1e-20 is subnormal in float32):

      gv = g + wd p              dgv = 3u wd |p| + 2u (|g| + wd |p|) + wd dp0       -- ABSOLUTE: gv may cancel to nothing
      m' = m + c1 (gv - m)       dm  = (1 - c1) dm0 + c1 dgv + (2 + 3) u c1 |gv - m| + 2u |m'|
      v' = b2 v + c2 gv gv       dv  = b2 dv0 + 2 c2 |gv| dgv + c2 dgv^2 + 5u c2 gv^2 + 3u b2 v + 2u v' + 4 tiny
      r  = sqrt(v')              dr  = min(dv / r, sqrt(dv)) + 2u r          (|sqrt(x) - sqrt(y)| = |x - y| / (sqrt(x) + sqrt(y)))
      den = r / sq + eps         dden = dr / sq + 3u r / sq + u eps + 2u den
      q  = m' / den              dq  = dm / den + |m'| dden / den^2 + 2u |q|
      p' = p - ss q              dp  = dp0 + ss dq + 3u ss |q| + 2u |p'|

    Largest fractions observed, kernel / float32 restatement: p 0.498 / 0.498, m 0.480 / 0.480, v 0.473 / 0.473
    (the final rounding of p alone may use u |p'| of the 2u |p'| allowed for it).
    """
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    c1, c2, ss, sq = 1.0 - B1, 1.0 - B2, LR / bc1, np.sqrt(bc2)
    p2, m2, v2 = _adam_f64(p, g, m, v, step, wd)
    gv = g + wd * p
    dgv = 3 * u * wd * np.abs(p) + 2 * u * (np.abs(g) + wd * np.abs(p)) + wd * dp0
    dm = (1 - c1) * dm0 + c1 * dgv + 5 * u * c1 * np.abs(gv - m) + 2 * u * np.abs(m2)
    dv = B2 * dv0 + 2 * c2 * np.abs(gv) * dgv + c2 * dgv ** 2 + 5 * u * c2 * gv * gv + 3 * u * B2 * v + 2 * u * v2 + 4 * tiny
    r = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
        dr = np.where(r > 0, np.minimum(dv / r, np.sqrt(dv)), np.sqrt(dv)) + 2 * u * r
    den = r / sq + EPS
    dden = dr / sq + 3 * u * r / sq + u * EPS + 2 * u * den
    q = m2 / den
    dq = dm / den + np.abs(m2) * dden / den ** 2 + 2 * u * np.abs(q)
    dp = dp0 + ss * dq + 3 * u * ss * np.abs(q) + 2 * u * np.abs(p2)
    return dp, dm, dv


def _adam_inputs(n, scale, wd, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * scale).astype(np.float32)
    m = (rng.standard_normal(n) * scale * 0.3).astype(np.float32)
    v = ((rng.standard_normal(n) * scale) ** 2 * rng.random(n)).astype(np.float32)
    if n > 1:
        g[-1], v[-1] = 0.0, 0.0                            # g = 0 with v = 0: the denominator is eps alone
    if n > 2 and wd > 0:
        g[1] = np.float32(-np.float32(wd) * p[1])          # g + wd p cancels to rounding noise
    return p, g, m, v


class _AdamRun:
    """p, g, m, v at odd float offsets 1, 3, 5, 7 inside larger NaN buffers, as slices of one flat buffer are."""

    def __init__(self, device, p, g, m, v):
        self.device, self.n = device, len(p)
        self.bufs = [_guard(x, device, odd=o) for x, o in zip((p, g, m, v), (1, 3, 5, 7))]
        assert all(view.data_ptr() % 8 == 4 for _, view in self.bufs)
        self.g_host = g

    def step(self, step, wd, guard=False):
        views = [v for _, v in self.bufs]
        if guard is False:
            _call("clx_adam_step", self.device, *views, self.n, LR, B1, B2, EPS, wd, step)
        else:
            _call("clx_adam_step_guarded", self.device, *views, self.n, LR, B1, B2, EPS, wd, step, guard)
        return self

    def result(self):
        assert all(_intact(b, v) for b, v in self.bufs)
        p, g, m, v = [v.cpu().numpy() for _, v in self.bufs]
        assert g.tobytes() == self.g_host.tobytes()        # the gradient is read only
        return p, m, v


ADAM_N = [1, 255, 256, 257, 262_143, 262_145, 600_001]     # the block edge, the grid cap +- 1, 2.3 trips


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step(n, device):
    """One step from arbitrary (p, g, m, v) against the float64 formula under _adam_bars: the full cross of step, weight
    decay and gradient scale up to 257 elements, one combination per value of each above."""
    grid = [(s, wd, sc) for s in (1, 7, 1000) for wd in (0.0, 0.01) for sc in (1.0, 1e-3, 1e-20)]
    combos = grid if n <= 257 else [(1, 0.01, 1.0), (7, 0.01, 1e-3), (1000, 0.0, 1e-20)]
    for step, wd, scale in combos:
        p, g, m, v = _adam_inputs(n, scale, wd, seed=step + n)
        ref = _adam_f64(*[x.astype(np.float64) for x in (p, g, m, v)], step, wd)
        bars = _adam_bars(*[x.astype(np.float64) for x in (p, g, m, v)], step, wd)
        with np.errstate(under="ignore"):
            rest = _adam_f32(p, g, m, v, step, wd)
        got = _AdamRun(device, p, g, m, v).step(step, wd).result()
        for name, gk, rk, bk, sk in zip("pmv", got, ref, bars, rest):
            assert not np.isnan(gk).any()
            _check(f"adam n={n} step={step} wd={wd} scale={scale} {name}", gk.astype(np.float64), rk, bk, sk.astype(np.float64))
        if scale == 1e-20 and wd == 0:
            assert ref[2].max() < EPS ** 2 * 1e-20             # v is far below eps^2 (weight decay would couple p in)


def test_adam_five_steps_follow_torch_adam(device):
    """Five steps with fresh gradients from a zero state against torch.optim.Adam on float64 copies.  The bar of step t
    is _adam_bars fed with the bars of step t - 1 (dp0, dm0, dv0): the state's error is carried through the same
    first-order propagation.  The float64 formula used for the bars is itself held to torch's result under the same
    function with u = 2^-53.  Largest fractions observed, kernel / float32 restatement: p 0.435 / 0.435, m 0.326 / 0.326,
    v 0.400 / 0.400."""
    n, wd = 4099, 0.01
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * (0.1 + t)).astype(np.float32) for t in range(5)]
    tp = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([tp], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    zero = np.zeros(n, np.float32)
    run = _AdamRun(device, p0, grads[0], zero, zero)
    state64 = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    state32 = (p0, zero, zero)
    bars, bars64 = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    for t, g in enumerate(grads, start=1):
        tp.grad = torch.from_numpy(g).double()
        opt.step()
        run.bufs[1][1].copy_(torch.from_numpy(g))
        run.g_host = g
        got = run.step(t, wd).result()
        g64 = g.astype(np.float64)
        bars = _adam_bars(state64[0], g64, state64[1], state64[2], t, wd, dp0=bars[0], dm0=bars[1], dv0=bars[2])
        bars64 = _adam_bars(state64[0], g64, state64[1], state64[2], t, wd, u=2.0 ** -53, tiny=0.0,
                            dp0=bars64[0], dm0=bars64[1], dv0=bars64[2])
        state64 = _adam_f64(state64[0], g64, state64[1], state64[2], t, wd)
        state32 = _adam_f32(state32[0], g, state32[1], state32[2], t, wd)
        st = opt.state[tp]
        torch_state = (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
        for name, gk, tk, fk, bk, b64, sk in zip("pmv", got, torch_state, state64, bars, bars64, state32):
            assert _frac(np.abs(fk - tk), b64) <= 1.0
            _check(f"adam trajectory step {t} {name}", gk.astype(np.float64), tk, bk, sk.astype(np.float64))
    assert np.abs(state64[0] - p0).max() > 3 * LR                # the parameters moved


def test_adam_guard(device):
    """skip_if_positive: NULL and a device 0.0 give identical bits, a negative value runs, a positive value leaves p, m
    and v untouched at 600 001 elements (every trip of every block returns)."""
    n, step, wd = 600_001, 7, 0.01
    p, g, m, v = _adam_inputs(n, 1.0, wd, seed=1)
    gbuf, guard = _guard(np.array([0.0, -1.0, 2.0 ** -1074, 3.0]), device)
    plain = _AdamRun(device, p, g, m, v).step(step, wd).result()
    assert not np.array_equal(plain[0], p)
    for k, runs in ((0, True), (1, True), (2, False), (3, False)):
        got = _AdamRun(device, p, g, m, v).step(step, wd, guard=guard[k:]).result()
        want = plain if runs else (p, m, v)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), k
    got = _AdamRun(device, p, g, m, v).step(step, wd, guard=None).result()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain))
    assert _intact(gbuf, guard)


def test_adam_edge_arguments(device):
    p, g, m, v = _adam_inputs(16, 1.0, 0.0, seed=2)
    run = _AdamRun(device, p, g, m, v)
    run.n = 0
    run.step(1, 0.0)                                        # no elements: OK, nothing touched
    run.n = 16
    _rejected(lambda: run.step(0, 0.0))
    _rejected(lambda: run.step(-1, 0.0))
    run.n = -1
    _rejected(lambda: run.step(1, 0.0))
    got = run.result()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (p, m, v)))


# ------------------------------------------------------------------------------------------------
# 5. clx_sample_pairs
# ------------------------------------------------------------------------------------------------
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _u64(x):
    return np.asarray(x).astype(np.uint64) if not isinstance(x, int) else np.array(x & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _below(r, n):
    """Multiply-shift range reduction of the upper 32 bits of r to [0, n)."""
    return ((r >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def _sample_pairs_ref(table, B, num_anchors, num_refs, nd, lo, hi, seed, stream):
    """The documented generator on uint64 arrays (wrap-around is silent): per batch row b
         key = mix(seed ^ mix(stream * 0x100000001b3 + b))
       per anchor a: ra = mix(key ^ (0xa5a5a5a5 + 2 a)), rb = mix(ra); column 0 takes the upper half of ra, column 1 its
       lower half, column 2 the upper half of rb, each reduced to [lo, hi[d]]
       per pair p of the row: the offset row is the upper half of mix(key ^ (0x5a5a5a5a00000000 + p)) reduced to
       [0, noffsets)."""
    P = num_anchors * num_refs
    with np.errstate(over="ignore"):
        b = np.arange(B, dtype=np.uint64)[:, None]
        p = np.arange(P, dtype=np.uint64)[None, :]
        a = p // np.uint64(num_refs)
        key = _splitmix64(_u64(seed) ^ _splitmix64(_u64(stream) * np.uint64(0x100000001B3) + b))
        ra = _splitmix64(key ^ (np.uint64(0xA5A5A5A5) + np.uint64(2) * a))
        rb = _splitmix64(ra)
        ro = _splitmix64(key ^ (np.uint64(0x5A5A5A5A00000000) + p))
        bits = [ra, ra << np.uint64(32), rb]
    o = _below(ro, len(table)).astype(np.int64)
    anchor = np.stack([lo + _below(bits[d], hi[d] - lo + 1).astype(np.int64) for d in range(nd)], axis=-1)
    return anchor, anchor + table[o].astype(np.int64)


# (nd, B, num_anchors, num_refs, lo, hi, noffsets, seed, stream id)
SAMPLE_CASES = [
    (2, 2, 10_000, 17, 4, (40, 52), 28, 0, 0),                              # 340 000 pairs: above the grid cap
    (3, 2, 10_000, 17, 4, (20, 30, 9), 122, 2 ** 64 - 1, 2 ** 63),
    (3, 3, 50, 3, 5, (5, 12, 5), 7, 12345, 1),                              # lo == hi[d]
    (2, 1, 255, 1, -3, (3, -3), 1, 2 ** 64 - 1, 0),                         # one offset; a negative lower end
    (2, 3, 1, 257, 0, (1000, 1000), 3, 0, 2 ** 63),                         # one anchor; equal ranges in both columns
    (3, 1, 1, 1, 0, (2 ** 31 - 2, 1, 2 ** 30), 2, 1, 1),                    # the widest range
]


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: "nd%d_B%d_%dx%d" % c[:4])
def test_sample_pairs_is_the_documented_stream(case, device):
    """Bit-exact against the NumPy uint64 restatement: the same (seed, stream_id) gives the same pairs, on any build."""
    nd, B, na, nr, lo, hi, noff, seed, stream = case
    table = np.random.default_rng(noff).integers(-6, 7, size=(noff, nd)).astype(np.int32)
    P = na * nr
    SENT = -7777
    out = [torch.full((B * P * nd + GUARD,), SENT, dtype=torch.int64, device=device) for _ in range(2)]
    hi_c = (ctypes.c_int * nd)(*hi)
    _call("clx_sample_pairs", device, out[0], out[1], torch.from_numpy(table).to(device), noff, B, na, nr, nd, lo, hi_c,
          seed, stream)
    want = _sample_pairs_ref(table, B, na, nr, nd, lo, hi, seed, stream)
    for got, ref in zip(out, want):
        g = got.cpu().numpy()
        assert (g[B * P * nd:] == SENT).all()
        assert np.array_equal(g[: B * P * nd].reshape(B, P, nd), ref)
    for d in range(nd):
        assert want[0][..., d].min() >= lo and want[0][..., d].max() <= hi[d]
    if na >= 10_000:
        # the input can tell the columns, the rows and the streams apart
        assert not np.array_equal(want[0][..., 0], want[0][..., 1]) and not np.array_equal(want[0][0], want[0][1])
        other = _sample_pairs_ref(table, B, na, nr, nd, lo, hi, seed, (stream + 1) % 2 ** 64)
        assert not np.array_equal(other[0], want[0])


def test_sample_pairs_rejects_empty_ranges_and_zero_counts(device):
    nd, B, na, nr, noff = 3, 2, 8, 4, 5
    out = [torch.full((B * na * nr * nd,), -7777, dtype=torch.int64, device=device) for _ in range(2)]
    table = torch.zeros(noff, nd, dtype=torch.int32, device=device)

    def run(noff=noff, B=B, na=na, nr=nr, nd=nd, lo=2, hi=(9, 9, 9)):
        _call("clx_sample_pairs", device, out[0], out[1], table, noff, B, na, nr, nd, lo, (ctypes.c_int * 3)(*hi), 1, 1)

    _rejected(lambda: run(hi=(1, 9, 9)))
    _rejected(lambda: run(hi=(9, 1, 9)))
    _rejected(lambda: run(hi=(9, 9, 1)))
    for zero in ("noff", "B", "na", "nr"):
        _rejected(lambda: run(**{zero: 0}))
    _rejected(lambda: run(nd=4))
    assert all((t == -7777).all() for t in out)
    run(nd=2, hi=(9, 9, 1))                                 # a 2-D call does not look at hi[2]
    run()
    assert all((t != -7777).all() for t in out)
