"""The split precision (clx_conv_desc.precision = CLX_PREC_F32X3BF16, csrc/gemm_sp.hip) through clx_conv_fwd and
clx_conv_wgrad, the way the network runs it: 1x1 layers and the transform-domain products of the 2-D Winograd layers,
every epilogue of the split kernels, the plane hand-overs between calls (aplanes_valid, dyplanes_valid, vcache_valid,
dy_vcache), the planes the transforms and the product epilogue write, against float64 and against the same descriptor
in float32.

Every call reads the launch profile: a 1x1 launch without its planes runs in float32 and would meet every float64 bar,
so each test also proves that the split kernels ran (one split product of the kind the K rule picks, a split pass only
where no planes were handed over, no float32 GEMM).  Scratch, caches and planes start as 0xFF bytes (NaN); outputs
carry sentinels past N and past M.

Replaces the same reference arithmetic as the default kernels: nn.Conv{2,3}d in float32 and its autograd backward
(cellulus/models/unet.py:24-63, cellulus/train.py:178).
"""
import ctypes
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from cellulus_amd import _clx
from cellulus_amd._clx import ClxConvDesc, ClxSrc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -7.25                        # output sentinel
KINDS = {"IGEMM_WIDE": 0, "IGEMM_NARROW": 1, "WGRAD": 2, "GEMM_SP": 3, "WGRAD_SP": 4, "SPLIT_PLANES": 5, "GEMM_SP2": 16}


def _st():
    return _clx.stream_ptr(DEV)


def _padded_rows(rows):             # sp::padded_rows (csrc/sp_planes.h)
    return 128 if rows <= 128 else (rows + 63) // 64 * 64


def _ff(nbytes):
    """scratch that reads as NaN until written: 0xFF bytes"""
    return torch.full((int(nbytes) + 16,), 255, dtype=torch.uint8, device=DEV)


def _split(x):
    """clx_split_planes of a [rows][K] view (row stride x.stride(0))"""
    rows, K = x.shape
    buf = _ff(_clx.load().clx_planes_bytes(rows, K))
    _clx.call("clx_split_planes", _clx.ptr(x), x.stride(0), rows, K, _clx.ptr(buf), _st())
    return buf


def _join(buf, rows, K, offset=0):
    x = torch.full((rows, K), float("nan"), device=DEV)
    _clx.call("clx_join_planes", ctypes.c_void_p(buf.data_ptr() + offset), rows, K, _clx.ptr(x), K, _st())
    return x


def _tail(buf, rows, K, offset=0):
    """the 16-bit words of the padding rows [rows, padded_rows(rows)) of the planes at buf[offset:], all pieces"""
    prows = _padded_rows(rows)
    nb = prows // 32 * (K // 16) * 3072
    h = buf[offset:offset + nb].view(torch.int16).view(prows // 32, K // 16, 3, 2, 32, 8)
    return h.permute(0, 4, 1, 2, 3, 5).reshape(prows, -1)[rows:]


def _same_bits(a, b):
    """bit-identical float32 tensors (-0.0 taken as +0.0: the planes give it back as +0.0)"""
    return torch.equal((a + 0.0).view(torch.int32), (b + 0.0).view(torch.int32))


def _kind(kernel, K):
    """the profile kind of the split product clx_sp_launch picks (CLX_SP_TILE / CLX_SP_MFMA, else K <= 1024)"""
    if kernel == "tile128":
        return "GEMM_SP2"
    if kernel in ("tile256", "mfma16"):
        return "GEMM_SP"
    return "GEMM_SP2" if K <= 1024 else "GEMM_SP"


def _select(monkeypatch, kernel):
    monkeypatch.delenv("CLX_SP_TILE", raising=False)
    monkeypatch.delenv("CLX_SP_MFMA", raising=False)
    monkeypatch.delenv("CLX_SP_TILE_MAXK", raising=False)
    if kernel == "mfma16":
        monkeypatch.setenv("CLX_SP_MFMA", "16")
    elif kernel != "default":
        monkeypatch.setenv("CLX_SP_TILE", kernel[4:])


@contextmanager
def _launches():
    """launch counts per profile kind of what runs inside the block"""
    _clx.call("clx_profile_enable", 2)
    counts = {}
    try:
        yield counts
        lib = _clx.load()
        for name, k in KINDS.items():
            n, ms, fl = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            _clx.check(lib.clx_profile_read(k, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)), "clx_profile_read")
            counts[name] = int(n.value)
    finally:
        _clx.call("clx_profile_enable", 0)


def _expect(counts, **want):
    full = {k: 0 for k in KINDS}
    full.update(want)
    assert counts == full, (counts, full)


def _bars(got, ref, what=""):
    """the bars of test_gpu_sp.py::test_product_from_planes_against_float64"""
    d = got.double() - ref
    rms = ref.pow(2).mean().sqrt().item()
    rel = (d.pow(2).mean().sqrt() / rms).item()
    err = d.abs().max().item()
    bias_err = abs((d.mean() / rms).item())
    assert rel < 3e-7, (what, rel, err)
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), (what, err)
    assert bias_err < 2e-8, (what, bias_err)


def _colsum_ok(got, vals, what=""):
    """column sums added in float32 (partial sums, then float atomics in any order) against the float64 sums of the same
    values: within (2 sqrt(rows) + 8) float32 roundings of the column's sum of magnitudes (a random walk of roundings;
    measured 1.05e-6 of it on 70 000 rows, where the bar is 3.2e-5 — a partial sum left out costs ~1e-3 or more)"""
    want = vals.double().sum(0)
    scale = (vals.double().abs().sum(0) + 1.0) * (2 * vals.shape[0] ** 0.5 + 8) * 2.0 ** -24
    assert ((got.double() - want).abs() / scale).max().item() < 1.0, what


def _words(bits):
    """(rows, 32 w) bool -> (rows, w) int32 gate words (bit n & 31 of word n >> 5)"""
    b = bits.reshape(bits.shape[0], -1, 32).to(torch.int64)
    w = (b << torch.arange(32, device=bits.device)).sum(-1)
    return (w - (w >= 2 ** 31).to(torch.int64) * 2 ** 32).to(torch.int32)


def _unbits(words, C):
    w = words.to(torch.int64) & 0xFFFFFFFF
    return ((w[:, :, None] >> torch.arange(32, device=words.device)) & 1).bool().reshape(words.shape[0], -1)[:, :C]


def _src(ptr, C, ld, D, H, W):
    s = ClxSrc()
    s.ptr, s.C, s.ld = ptr, C, ld
    s.D, s.H, s.W = D, H, W
    s.oz = s.oy = s.ox = 0
    s.fz = s.fy = s.fx = 1
    return s


def _pack(w, cout, cin, taps, mode):
    """clx_pack_weights of w (cout, cin, taps) with cin_pad = cin, cout_pad = cout"""
    a2 = {0: 1, 2: 16, 3: 16, 4: 36 if taps == 9 else 25, 5: 36 if taps == 9 else 25, 6: 36}[mode]
    wp = torch.full((a2 * cout * cin * (taps if mode == 0 else 1),), float("nan"), device=DEV)
    wd = w.reshape(cout, cin, taps).to(DEV).contiguous()
    _clx.call("clx_pack_weights", _clx.ptr(wd), _clx.ptr(wp), cout, cin, taps, cin, cout, mode, _st())
    return wp


# ------------------------------------------------------------------------------------------------ 1x1 layers, forward
def _pw_desc(x, grid, C, N, wp, wplanes, aplanes, out, ld_out):
    B, D, H, W = grid
    d = ClxConvDesc()
    d.nsrc = 1
    d.src[0] = _src(x.data_ptr(), C, x.stride(0), D, H, W)
    d.B, d.ID, d.IH, d.IW = B, D, H, W
    d.KD = d.KH = d.KW = 1
    d.N = N
    d.wpack = wp.data_ptr()
    d.out, d.ld_out = out.data_ptr(), ld_out
    d.precision = 1
    d.wplanes = wplanes.data_ptr()
    d.aplanes = aplanes.data_ptr()
    return d


# (kernel, (B, D, H, W), C, N): every kernel sees every epilogue on a ragged M with an odd number of 64-wide K periods
# (C = 192, 320, 1088: 3, 5, 17); M from 5 to 70 000, below one tile and above; one 3-D 1x1x1 layer
FWD_CASES = [
    ("tile128", (1, 1, 1, 1000), 192, 128),
    ("tile128", (1, 1, 1, 5), 1088, 384),
    ("tile256", (1, 1, 1, 129), 320, 384),
    ("tile256", (1, 1, 1, 70000), 192, 128),
    ("mfma16", (1, 1, 1, 100), 320, 128),
    ("mfma16", (1, 1, 1, 1000), 1088, 384),
    ("default", (2, 3, 5, 7), 128, 128),
]


@pytest.mark.parametrize("kernel,grid,C,N", FWD_CASES)
def test_pointwise_forward_every_epilogue(kernel, grid, C, N, monkeypatch):
    """A 1x1 layer through clx_conv_fwd in the split precision on each of the three product kernels: plain (the fast
    path of whole tiles), bias + ReLU + gate bits out, float mask, gate bits in, accumulate, the data-gradient hand-over
    form (gate bits in + the output's own planes + its column sums), and aplanes_valid — against float64 with the bars
    of the plane-level test.  The planes the epilogue writes are the exact split of the stored output: joined, they give
    it back bit for bit, they equal clx_split_planes(out) byte for byte, and their padding rows are zero."""
    _select(monkeypatch, kernel)
    kind = _kind(kernel, C)
    lib = _clx.load()
    B, D, H, W = grid
    M = B * D * H * W
    torch.manual_seed(M + C + N)
    x = torch.relu(torch.randn(M, C + 4, device=DEV))[:, :C]          # (a padded leading dimension)
    w = torch.randn(N, C, device=DEV) / C ** 0.5
    bias = torch.randn(N, device=DEV)
    wp = _pack(w, N, C, 1, 0)
    wplanes = _split(wp.view(N, C))
    ref = x.double() @ w.double().t()
    ldo = N + 32
    aplanes = _ff(lib.clx_planes_bytes(M, C))

    def run(setup, ld_out=ldo, valid=False):
        out = torch.full((M + 3, ld_out), SENT, device=DEV)
        if not valid:
            aplanes.fill_(255)
        d = _pw_desc(x, grid, C, N, wp, wplanes, aplanes, out, ld_out)
        keep = setup(d, out)
        assert lib.clx_conv_sp_covers(ctypes.byref(d), 0) == 1
        with _launches() as n:
            _clx.call("clx_conv_fwd", ctypes.byref(d), _st())
        _expect(n, **{kind: 1, "SPLIT_PLANES": 0 if valid else 1})
        assert (out[M:] == SENT).all() and (out[:M, N:] == SENT).all()       # nothing past M, nothing past N
        return out[:M, :N], keep

    out, _ = run(lambda d, o: None)
    _bars(out, ref, "plain")

    gate = torch.full((M + 3, ldo // 32), 0x5A5A5A5A, dtype=torch.int32, device=DEV)

    def bias_relu(d, o):
        d.bias, d.relu = bias.data_ptr(), 1
        d.gate_out, d.ld_gate = gate.data_ptr(), ldo // 32
    out, _ = run(bias_relu)
    _bars(out, torch.relu(ref + bias.double()), "bias_relu")
    bits = _unbits(gate[:M], N)
    assert torch.equal(bits, out > 0)
    assert (gate[M:] == 0x5A5A5A5A).all()

    mask = torch.randn(M, ldo, device=DEV)

    def float_mask(d, o):
        d.mask, d.ld_mask = mask.data_ptr(), ldo
    out, _ = run(float_mask)
    _bars(out, ref * (mask[:, :N] > 0), "mask")

    def bit_mask(d, o):                                # the gates written above, read back as the mask
        d.mask_bits, d.ld_mask_bits = gate.data_ptr(), ldo // 32
    out, _ = run(bit_mask)
    _bars(out, ref * bits, "mask_bits")

    prev = torch.randn(M, ldo, device=DEV)

    def accumulate(d, o):
        o[:M, :N].copy_(prev[:, :N])
        d.accumulate, d.bias, d.relu = 1, bias.data_ptr(), 1
    out, _ = run(accumulate)
    _bars(out, torch.relu(ref + bias.double() + prev[:, :N].double()), "accumulate")

    # the data-gradient hand-over form: gate bits in, the output's planes and column sums out (dense output)
    out_planes = _ff(lib.clx_planes_bytes(M, N))
    colsum = torch.full((N,), 0.5, device=DEV)

    def hand_over(d, o):
        d.mask_bits, d.ld_mask_bits = gate.data_ptr(), ldo // 32
        d.out_planes, d.out_colsum = out_planes.data_ptr(), colsum.data_ptr()
    out, _ = run(hand_over, ld_out=N)
    _bars(out, ref * bits, "hand_over")
    _colsum_ok(colsum - 0.5, out, "out_colsum")
    assert _same_bits(_join(out_planes, M, N), out)
    assert not _tail(out_planes, M, N).any()
    assert torch.equal(out_planes, _split(out))

    # aplanes_valid: the product reads the planes it is handed (those of another x), not src[0]
    x2 = torch.relu(torch.randn(M, C, device=DEV)) - 0.25
    aplanes.copy_(_split(x2))
    out, _ = run(lambda d, o: setattr(d, "aplanes_valid", 1), valid=True)
    _bars(out, x2.double() @ w.double().t(), "aplanes_valid")


# --------------------------------------------------------------------------------------- 1x1 layers, weight gradient
@pytest.mark.parametrize("rows,N,C,case", [(5, 128, 128, "fresh"), (129, 256, 768, "dyplanes_valid"),
                                           (1000, 768, 256, "aplanes_valid"), (33001, 128, 768, "fresh"),
                                           (33000, 256, 128, "dyplanes_valid")])
def test_pointwise_weight_gradient(rows, N, C, case, monkeypatch):
    """A 1x1 layer's weight gradient through clx_conv_wgrad in the split precision: fresh planes (the bias gradient is
    the split pass's column sums); dyplanes_valid on the planes a data-gradient epilogue wrote (gate bits in, out_planes,
    out_colsum — no dbias, as the planner runs it); aplanes_valid on planes of another x.  The bars of
    test_weight_gradient_from_planes_against_float64."""
    _select(monkeypatch, "default")
    lib = _clx.load()
    torch.manual_seed(rows + N + C)
    x = torch.relu(torch.randn(rows, C, device=DEV))
    dwp = torch.full((N, C), 1.0, device=DEV)                        # += into what is there
    dbias = torch.full((N,), 0.25, device=DEV)
    aplanes, dyplanes = _ff(lib.clx_planes_bytes(rows, C)), _ff(lib.clx_planes_bytes(rows, N))
    splits = 2
    xr = x
    if case == "dyplanes_valid":
        # dY = (z w2^T) * gate, made by the split 1x1 product whose epilogue writes dY's planes and column sums
        K2 = 192
        z = torch.randn(rows, K2, device=DEV)
        w2 = torch.randn(N, K2, device=DEV) / K2 ** 0.5
        wp2 = _pack(w2, N, K2, 1, 0)
        wpl2 = _split(wp2.view(N, K2))
        gate = _words(torch.rand(rows, N, device=DEV) < 0.5)
        dy_buf = torch.full((rows + 3, N), SENT, device=DEV)
        zpl = _ff(lib.clx_planes_bytes(rows, K2))
        d2 = _pw_desc(z, (1, 1, 1, rows), K2, N, wp2, wpl2, zpl, dy_buf, N)
        d2.mask_bits, d2.ld_mask_bits = gate.data_ptr(), N // 32
        d2.out_planes, d2.out_colsum = dyplanes.data_ptr(), dbias.data_ptr()
        with _launches() as n:
            _clx.call("clx_conv_fwd", ctypes.byref(d2), _st())
        _expect(n, GEMM_SP2=1, SPLIT_PLANES=1)
        dy = dy_buf[:rows]
        splits = 1
    else:
        dy = torch.randn(rows, N, device=DEV) * (torch.rand(rows, N, device=DEV) < 0.5)    # a gated gradient
    if case == "aplanes_valid":
        xr = torch.relu(torch.randn(rows, C, device=DEV)) + 0.125
        aplanes.copy_(_split(xr))
        splits = 1
    d = ClxConvDesc()
    d.nsrc = 1
    d.src[0] = _src(x.data_ptr(), C, C, 1, 1, rows)
    d.B, d.ID, d.IH, d.IW = 1, 1, 1, rows
    d.KD = d.KH = d.KW = 1
    d.N = N
    d.precision = 1
    d.aplanes, d.aplanes_valid = aplanes.data_ptr(), int(case == "aplanes_valid")
    d.dyplanes, d.dyplanes_valid = dyplanes.data_ptr(), int(case == "dyplanes_valid")
    assert lib.clx_conv_sp_covers(ctypes.byref(d), 1) == 1
    with _launches() as n:
        _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy), N, _clx.ptr(dwp),
                  None if case == "dyplanes_valid" else _clx.ptr(dbias), _st())
    _expect(n, WGRAD_SP=1, SPLIT_PLANES=splits)
    ref = dy.double().t() @ xr.double()
    got = dwp.double() - 1.0
    rms = ref.pow(2).mean().sqrt().item()
    rel = ((got - ref).pow(2).mean().sqrt() / rms).item()
    assert rel < 3e-7, rel
    assert abs(((got - ref).mean() / rms).item()) < 3e-8
    # the bias gradient: from the split pass of dY, or from the epilogue that made dY
    _colsum_ok(dbias - 0.25, dy, "dbias")


# ----------------------------------------------------------------------------------------------- 2-D Winograd layers
# (algo, k, C, N, H, W), B = 2: output extents that are not multiples of the tile, tile counts 96 / 220 / 84 (below and
# above 128, not multiples of 64), C != N both ways; the two F(4x4) layers have even output extents (pool_out)
WINO = [(1, 3, 128, 256, 14, 17), (2, 3, 256, 128, 44, 40), (2, 2, 128, 128, 27, 23)]
B_W = 2
# from measurements on the MI355X (the docstrings give them): the split result's rel-L2 error against float64 at most
# RATIO x the float32 result's (measured 0.48 .. 0.91), and the two results at most SPLIT_VS_F32 rel-L2 of the float64
# result apart (measured up to 1.9e-6: mostly the float32 result's own error)
RATIO = 1.0
SPLIT_VS_F32 = 3e-6


def _wino_a(algo, k):
    return (2 if algo == 1 else 4) + k - 1


def _wino_desc(x, shape, algo, k, C, N, pad):
    B, H, W = shape
    d = ClxConvDesc()
    d.nsrc = 1
    d.src[0] = _src(x.data_ptr(), C, C, 1, H, W)
    d.B, d.ID, d.IH, d.IW = B, 1, H, W
    d.KD, d.KH, d.KW = 1, k, k
    d.PH = d.PW = pad
    d.N = N
    d.algo = algo
    return d


def _compare(got, want, what, errs):
    """rel-L2 of both precisions against float64, and of their difference; the split's error at most RATIO x the
    float32 one's"""
    g1, g0 = got[1].double().cpu(), got[0].double().cpu()
    rms = want.pow(2).mean().sqrt().item()
    e1 = ((g1 - want).pow(2).mean().sqrt() / rms).item()
    e0 = ((g0 - want).pow(2).mean().sqrt() / rms).item()
    dd = ((g1 - g0).pow(2).mean().sqrt() / rms).item()
    errs.append((what, e1, e0, dd))
    tol = 2e-5 * max(1.0, want.abs().max().item())            # the float32 test's bar, for both
    assert (g0 - want).abs().max().item() < tol, (what, "f32")
    assert (g1 - want).abs().max().item() < tol, (what, "split")
    assert e1 <= RATIO * e0, (what, e1, e0)
    assert dd < SPLIT_VS_F32, (what, dd)


@pytest.mark.parametrize("algo,k,C,N,H,W", WINO)
def test_winograd_forward_split_vs_float32_and_float64(algo, k, C, N, H, W, monkeypatch):
    """clx_conv_fwd of a 2-D Winograd layer in the split precision and in float32 (the same descriptor otherwise):
    plain, bias + ReLU + gate bits, float mask, gate bits in, accumulate with the V cache, 2 x 2 pooling, the padded
    (data-gradient) form, and tile lists of one tile and of a sparse subset, which give the dense result's bits on
    their tiles and leave every other pixel alone.  Both against float64 (F.conv2d once per shape).

    The V cache the split forward writes is the exact split of the float32 forward's: per transform point, joined, it
    equals the float32 V bit for bit, and its padding rows are zero.  (The plane-writing and the float32 instances of
    the input transform, wino_input_kernel<.., PL>, do the same float32 arithmetic: measured, not one bit differs, so
    the check is exact rather than one ulp.)

    Measured on the MI355X (these shapes and seeds): the split result's rel-L2 error against float64 is 0.85 .. 0.89 x
    the float32 result's on every epilogue — the transforms are float32 in both, the split products are the more
    accurate —, and the two results lie at most 1.3e-6 rel-L2 apart (F(4x4, 3x3), C = 256).  Bars: RATIO, SPLIT_VS_F32."""
    _select(monkeypatch, "default")
    lib = _clx.load()
    torch.manual_seed(algo * 100 + k * 10 + C + H)
    mt, a = (2 if algo == 1 else 4), _wino_a(algo, k)
    OH, OW = H - k + 1, W - k + 1
    th, tw = -(-OH // mt), -(-OW // mt)
    T = B_W * th * tw
    x = torch.randn(B_W, H, W, C)
    w = torch.randn(N, C, k, k) * (2.0 / (C * k * k)) ** 0.5
    bias = torch.randn(N)
    xc = x.permute(0, 3, 1, 2).double()
    ref = F.conv2d(xc, w.double()).permute(0, 2, 3, 1)                               # (B, OH, OW, N)
    ref_pad = F.conv2d(xc, w.double(), padding=k - 1).permute(0, 2, 3, 1)
    x_d = x.to(DEV).contiguous()
    wp = _pack(w, N, C, k * k, 2 if algo == 1 else 4)
    wplanes = _split(wp.view(a * a * N, C))
    ldo = N + 32
    Mo = B_W * OH * OW
    prev = torch.randn(Mo, ldo, device=DEV)
    mask = torch.randn(Mo, ldo, device=DEV)
    gbits = torch.rand(Mo, N, device=DEV) < 0.5
    gwords = _words(gbits)
    errs = []
    vcaches = {}

    def run(prec, mode, pad=0, tiles=None):
        d = _wino_desc(x_d, (B_W, H, W), algo, k, C, N, pad)
        d.precision = prec
        oh, ow = OH + 2 * pad, OW + 2 * pad
        mo = B_W * oh * ow
        out = torch.full((mo + 3, ldo), SENT, device=DEV)
        d.out, d.ld_out = out.data_ptr(), ldo
        d.wpack = wp.data_ptr()
        if prec:
            d.wplanes = wplanes.data_ptr()
        assert lib.clx_conv_sp_covers(ctypes.byref(d), 0) == prec
        ws = _ff(lib.clx_conv_workspace_bytes(ctypes.byref(d), 0))
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        keep = {}
        if mode == "bias_relu":
            keep["gate"] = torch.full((mo, ldo // 32), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            keep["b"] = bias.to(DEV)
            d.bias, d.relu = keep["b"].data_ptr(), 1
            d.gate_out, d.ld_gate = keep["gate"].data_ptr(), ldo // 32
        elif mode == "mask":
            d.mask, d.ld_mask = mask.data_ptr(), ldo
        elif mode == "mask_bits":
            d.mask_bits, d.ld_mask_bits = gwords.data_ptr(), N // 32
        elif mode == "accumulate":
            out[:mo, :N].copy_(prev[:, :N])
            d.accumulate = 1
            keep["v"] = _ff(lib.clx_conv_vcache_bytes(ctypes.byref(d), 0))
            d.vcache = keep["v"].data_ptr()
        elif mode == "pool":
            keep["b"] = bias.to(DEV)
            d.bias, d.relu = keep["b"].data_ptr(), 1
            keep["pool"] = torch.full((mo // 4 + 3, N), SENT, device=DEV)
            d.pool_out, d.ld_pool = keep["pool"].data_ptr(), N
        if tiles is not None:
            keep["list"] = torch.tensor(tiles, dtype=torch.int32, device=DEV)
            d.tile_list, d.tile_count = keep["list"].data_ptr(), len(tiles)
        with _launches() as n:
            _clx.call("clx_conv_fwd", ctypes.byref(d), _st())
        if prec:
            _expect(n, **{_kind("default", C): 1})
        else:
            assert n["IGEMM_WIDE"] + n["IGEMM_NARROW"] >= 1 and n["GEMM_SP"] + n["GEMM_SP2"] + n["SPLIT_PLANES"] == 0, n
        assert (out[mo:] == SENT).all() and (out[:mo, N:] == SENT).all()
        if mode == "accumulate":
            vcaches[prec] = keep["v"]
        return out[:mo, :N].view(B_W, oh, ow, N), keep

    got = {p: run(p, "plain")[0] for p in (0, 1)}
    _compare(got, ref, "plain", errs)
    dense = got

    rr = {p: run(p, "bias_relu") for p in (0, 1)}
    _compare({p: rr[p][0] for p in rr}, torch.relu(ref + bias.double()), "bias_relu", errs)
    for p in rr:
        g = rr[p][1]["gate"]
        assert torch.equal(_unbits(g, N), (rr[p][0] > 0).reshape(Mo, N)), p

    got = {p: run(p, "mask")[0] for p in (0, 1)}
    _compare(got, ref * (mask[:, :N] > 0).cpu().view(B_W, OH, OW, N), "mask", errs)
    got = {p: run(p, "mask_bits")[0] for p in (0, 1)}
    _compare(got, ref * gbits.cpu().view(B_W, OH, OW, N), "mask_bits", errs)
    got = {p: run(p, "accumulate")[0] for p in (0, 1)}
    _compare(got, ref + prev[:, :N].double().cpu().view(B_W, OH, OW, N), "accumulate", errs)
    got = {p: run(p, "plain", pad=k - 1)[0] for p in (0, 1)}
    _compare(got, ref_pad, "padded", errs)

    # the V cache: per transform point the joined planes are the float32 V, bit for bit; padding rows zero
    pb = lib.clx_planes_bytes(T, C)
    v32 = vcaches[0][:a * a * T * C * 4].view(torch.float32).view(a * a, T, C)
    for xi in range(a * a):
        assert _same_bits(_join(vcaches[1], T, C, xi * pb), v32[xi]), xi
        assert not _tail(vcaches[1], T, C, xi * pb).any(), xi

    if OH % 2 == 0 and OW % 2 == 0:
        pr = {p: run(p, "pool") for p in (0, 1)}
        _compare({p: pr[p][0] for p in pr}, torch.relu(ref + bias.double()), "pool_out", errs)
        for p, (o, keep) in pr.items():
            pooled = o.reshape(B_W, OH // 2, 2, OW // 2, 2, N).amax((2, 4)).reshape(-1, N)
            assert torch.equal(keep["pool"][:Mo // 4], pooled), p
            assert (keep["pool"][Mo // 4:] == SENT).all()

    # tile lists: one tile, and a sparse subset — the dense result's bits there, the sentinel everywhere else
    ty = torch.arange(OH, device=DEV) // mt
    tx = torch.arange(OW, device=DEV) // mt
    tile_of = ((torch.arange(B_W, device=DEV)[:, None, None] * th + ty[None, :, None]) * tw + tx[None, None, :])
    for tiles in ([T // 2 + 1], list(range(3, T, 7)) + [T - 1]):
        for p in (0, 1):
            o, _ = run(p, "plain", tiles=tiles)
            sel = torch.isin(tile_of, torch.tensor(tiles, device=DEV))
            assert _same_bits(o[sel], dense[p][sel]), (p, len(tiles))
            assert (o[~sel] == SENT).all(), (p, len(tiles))
    # (pytest -s shows the rel-L2 errors (split, float32, split - float32) the bars were set from)
    print("\nwinograd forward", (algo, k, C, N), ["%s %.3g %.3g %.3g" % e for e in errs])


@pytest.mark.parametrize("algo,k,C,N,H,W", WINO)
def test_winograd_gradients_split_vs_float32_and_float64(algo, k, C, N, H, W, monkeypatch):
    """clx_conv_wgrad of a 2-D Winograd layer in the split precision and in float32: with the input transform of its
    own (and dy_vcache + dbias), and with the V cache of the forward (vcache_valid); then the data gradient that reads
    dy_vcache, which equals the same call without it bit for bit; for F(4x4, 3x3) also the adjoint data gradient
    (planes of the mode-6 pack) with a float mask and with gate bits.  Against float64 autograd.

    The dY transform the split weight gradient leaves in dy_vcache (wino_dy_dual_kernel<.., PL>) is the exact split of
    the float32 one: joined, bit for bit per transform point (measured: no ulp apart), padding rows zero.

    Measured on the MI355X (these shapes and seeds): the split weight gradient's rel-L2 error is 0.48 .. 0.69 x the
    float32 one's, the data gradients' (two-transform and adjoint) 0.88 .. 0.91 x; the two precisions lie at most 1.9e-6
    rel-L2 apart (the F(4x4, 3x3) weight gradient, C = 256, N = 128).  Bars: RATIO, SPLIT_VS_F32."""
    _select(monkeypatch, "default")
    lib = _clx.load()
    torch.manual_seed(algo * 1000 + k * 10 + N + W)
    mt, a = (2 if algo == 1 else 4), _wino_a(algo, k)
    OH, OW = H - k + 1, W - k + 1
    x = torch.randn(B_W, H, W, C)
    w = torch.randn(N, C, k, k) * (2.0 / (C * k * k)) ** 0.5
    dy = torch.randn(B_W, OH, OW, N) * (torch.rand(B_W, OH, OW, N) < 0.5)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    (F.conv2d(xr, wr) * dy.permute(0, 3, 1, 2).double()).sum().backward()
    ref_dw, ref_dx = wr.grad, xr.grad.permute(0, 2, 3, 1)
    ref_db = dy.double().sum((0, 1, 2))
    x_d, dy_d = x.to(DEV).contiguous(), dy.to(DEV).contiguous()
    wp = _pack(w, N, C, k * k, 2 if algo == 1 else 4)
    wpl = _split(wp.view(a * a * N, C))
    wpd = _pack(w, N, C, k * k, 3 if algo == 1 else 5)               # flipped filter: U[a^2][C][N]
    wpld = _split(wpd.view(a * a * C, N))
    gm = torch.randn(B_W * H * W, C, device=DEV)                   # the adjoint's ReLU gate, float and bits
    gw = _words(gm > 0)
    errs = []
    dw_got, db_got, dx_got, dyv = {}, {}, {}, {}
    adj = {}
    for prec in (0, 1):
        # the forward leaves V in the cache
        d = _wino_desc(x_d, (B_W, H, W), algo, k, C, N, 0)
        d.precision = prec
        out = torch.empty(B_W * OH * OW, N, device=DEV)
        d.out, d.ld_out, d.wpack = out.data_ptr(), N, wp.data_ptr()
        d.wplanes = wpl.data_ptr() if prec else None
        vc = _ff(lib.clx_conv_vcache_bytes(ctypes.byref(d), 0))
        d.vcache = vc.data_ptr()
        ws = _ff(lib.clx_conv_workspace_bytes(ctypes.byref(d), 0))
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        _clx.call("clx_conv_fwd", ctypes.byref(d), _st())
        for cached in (False, True):
            d = _wino_desc(x_d, (B_W, H, W), algo, k, C, N, 0)
            d.precision = prec
            assert lib.clx_conv_sp_covers(ctypes.byref(d), 1) == prec
            ws = _ff(lib.clx_conv_workspace_bytes(ctypes.byref(d), 1))
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
            if cached:
                d.vcache, d.vcache_valid = vc.data_ptr(), 1
            else:
                dyv[prec] = _ff(lib.clx_conv_vcache_bytes(ctypes.byref(d), 1))
                d.dy_vcache = dyv[prec].data_ptr()
            dwp = torch.zeros(a * a * N * C, device=DEV)
            db = torch.full((N,), 0.25, device=DEV)
            with _launches() as n:
                _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy_d), N, _clx.ptr(dwp), _clx.ptr(db), _st())
            if prec:
                _expect(n, WGRAD_SP=1)
            else:
                assert n["WGRAD"] >= 1 and n["WGRAD_SP"] + n["SPLIT_PLANES"] == 0, n
            dw = torch.empty(N, C, k * k, device=DEV)
            _clx.call("clx_unpack_wgrad_wino", _clx.ptr(dwp), _clx.ptr(dw), N, C, N, C, mt, k, 1, _st())
            dw_got[prec, cached] = dw.view(N, C, k, k)
            db_got[prec, cached] = db - 0.25
            adj_ws = ws
        if algo == 2 and k == 3:
            # the adjoint data gradient: A dY A^T from the weight gradient's workspace (the last call above)
            wpa = _pack(w, N, C, 9, 6)
            wpla = _split(wpa.view(36 * C, N))
            for mk in ("float", "bits"):
                dd = _wino_desc(dy_d, (B_W, OH, OW), 2, 3, N, C, 2)
                dd.adjoint, dd.precision = 1, prec
                dd.wpack = wpa.data_ptr()
                dd.wplanes = wpla.data_ptr() if prec else None
                dd.workspace, dd.workspace_bytes = adj_ws.data_ptr(), adj_ws.numel()
                o = torch.full((B_W * H * W + 3, C), SENT, device=DEV)
                dd.out, dd.ld_out = o.data_ptr(), C
                if mk == "float":
                    dd.mask, dd.ld_mask = gm.data_ptr(), C
                else:
                    dd.mask_bits, dd.ld_mask_bits = gw.data_ptr(), C // 32
                with _launches() as n:
                    _clx.call("clx_conv_fwd", ctypes.byref(dd), _st())
                if prec:
                    _expect(n, **{_kind("default", N): 1})
                assert (o[B_W * H * W:] == SENT).all()
                adj[prec, mk] = (o[:B_W * H * W].view(B_W, H, W, C), (gm > 0).view(B_W, H, W, C).cpu())
        # the data gradient, with dY's transform from dy_vcache and without it
        for cached in (True, False):
            dd = _wino_desc(dy_d, (B_W, OH, OW), algo, k, N, C, k - 1)
            dd.precision = prec
            dd.wpack = wpd.data_ptr()
            dd.wplanes = wpld.data_ptr() if prec else None
            assert lib.clx_conv_sp_covers(ctypes.byref(dd), 0) == prec
            ws = _ff(lib.clx_conv_workspace_bytes(ctypes.byref(dd), 0))
            dd.workspace, dd.workspace_bytes = ws.data_ptr(), ws.numel()
            if cached:
                dd.vcache, dd.vcache_valid = dyv[prec].data_ptr(), 1
            o = torch.full((B_W * H * W + 3, C), SENT, device=DEV)
            dd.out, dd.ld_out = o.data_ptr(), C
            with _launches() as n:
                _clx.call("clx_conv_fwd", ctypes.byref(dd), _st())
            if prec:
                _expect(n, **{_kind("default", N): 1})
            assert (o[B_W * H * W:] == SENT).all()
            dx_got[prec, cached] = o[:B_W * H * W].view(B_W, H, W, C)
        assert _same_bits(dx_got[prec, True], dx_got[prec, False]), prec

    for cached in (False, True):
        _compare({p: dw_got[p, cached] for p in (0, 1)}, ref_dw, "dw cached=%d" % cached, errs)
        for p in (0, 1):
            _colsum_ok(db_got[p, cached].cpu(), dy.reshape(-1, N), "dbias")
    _compare({p: dx_got[p, True] for p in (0, 1)}, ref_dx, "dx", errs)
    for mk in ("float", "bits"):
        if (0, mk) in adj:
            _compare({p: adj[p, mk][0] for p in (0, 1)}, ref_dx * adj[0, mk][1], "adjoint " + mk, errs)

    # dy_vcache: the split weight gradient's dY transform is the exact split of the float32 one
    gd_h, gd_w = -(-(OH + k - 1) // mt), -(-(OW + k - 1) // mt)
    Td = B_W * gd_h * gd_w
    pb = lib.clx_planes_bytes(Td, N)
    v32 = dyv[0][:a * a * Td * N * 4].view(torch.float32).view(a * a, Td, N)
    for xi in range(a * a):
        assert _same_bits(_join(dyv[1], Td, N, xi * pb), v32[xi]), xi
        assert not _tail(dyv[1], Td, N, xi * pb).any(), xi
    # (pytest -s shows the rel-L2 errors (split, float32, split - float32) the bars were set from)
    print("\nwinograd gradients", (algo, k, C, N), ["%s %.3g %.3g %.3g" % e for e in errs])
