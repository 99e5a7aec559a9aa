"""The split precision for channel counts that are multiples of 64 (csrc/gemm_sp.hip: the 128 x 64 tile of gemm_sp2_kernel,
the clamped B side of gemm_sp_kernel<0> and of the weight gradient) and the opt-in precision value that reaches them,
clx_conv_desc.precision = CLX_PREC_F32X3BF16_G64 = 2 / CLX_PRECISION=f32x3bf16g64: the bare products from planes against
float64, bit-equality with the 128-wide form, 1x1 layers with every epilogue and a 2-D Winograd layer through the C ABI,
and the 64 x 3 networks against the oracle.  The bars are those of test_gpu_sp.py / test_gpu_sp_conv.py, unchanged; the
harness is theirs: 0xFF scratch, sentinels past N and past M, launch-profile counts that prove which kernel ran.

Replaces the same reference arithmetic as the default kernels: nn.Conv{2,3}d in float32 and its autograd backward
(cellulus/models/unet.py:24-63, cellulus/train.py:178).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_gpu_sp_conv as S
from cellulus_amd import _clx
from cellulus_amd._clx import ClxConvDesc

pytestmark = pytest.mark.gpu

DEV = S.DEV
SENT = S.SENT
G64 = 2                              # CLX_PREC_F32X3BF16_G64


# ------------------------------------------------------------------------------------------- the products from planes
# N below one tile (64), 128 q + 64 (192, 320, 576); M below and above a tile; odd numbers of 64-wide periods (K = 192,
# 320, 1088); both sides of the K = 1024 rule
@pytest.mark.parametrize("tile", ["default", "tile128", "tile256"])
@pytest.mark.parametrize("M,N,K,relu", [(256, 64, 128, 0), (5, 64, 192, 1), (1000, 192, 256, 1), (100, 320, 320, 0),
                                        (70000, 64, 768, 1), (1000, 64, 1088, 1), (257, 576, 2304, 0)])
def test_product_from_planes_against_float64(M, N, K, relu, tile, monkeypatch):
    """clx_gemm_planes at N % 128 == 64 on the kernel the K rule picks and on each of the two forced ones (gemm_sp2_kernel on
    128 x 64 tiles; gemm_sp_kernel<0> with a half-dead last tile column), against float64 with the bars of
    test_gpu_sp.py::test_product_from_planes_against_float64; nothing written past column N or past row M."""
    S._select(monkeypatch, tile)
    torch.manual_seed(M + K)
    x = torch.relu(torch.randn(M, K, device=DEV))
    w = torch.randn(N, K, device=DEV) / K ** 0.5
    bias = torch.randn(N, device=DEV)
    out = torch.full((M + 3, N + 4), float("nan"), device=DEV)
    pa, pb = S._split(x), S._split(w)
    with S._launches() as n:
        _clx.call("clx_gemm_planes", _clx.ptr(pa), _clx.ptr(pb), M, N, K, _clx.ptr(bias), relu, _clx.ptr(out), N + 4, S._st())
    S._expect(n, **{S._kind(tile, K): 1})
    ref = x.double() @ w.double().t() + bias.double()
    if relu:
        ref = torch.relu(ref)
    assert torch.isnan(out[:, N:]).all() and torch.isnan(out[M:]).all()
    got = out[:M, :N].double()
    rms = ref.pow(2).mean().sqrt().item()
    err = (got - ref).abs().max().item()
    rel = ((got - ref).pow(2).mean().sqrt() / rms).item()
    bias_err = abs(((got - ref).mean() / rms).item())
    print("\nproduct", (M, N, K, relu, tile), "rel %.3g err %.3g bias %.3g" % (rel, err, bias_err))
    assert rel < 3e-7, (rel, err)
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err
    assert bias_err < 2e-8, bias_err


@pytest.mark.parametrize("M,K", [(1000, 256), (333, 192)])
def test_narrow_products_equal_the_128_wide_form_bit_for_bit(M, K, monkeypatch):
    """Per output element the arithmetic does not depend on N or on the tile: with CLX_SP_TILE=128, N = 64 on the first 64
    rows of a weight matrix gives the bits of columns [0, 64) of the N = 128 product on its first 128 rows (B's planes are
    row-block major: the narrow operand's planes are a prefix of the wide one's), and N = 192 those of [0, 192) of N = 256.
    The 256 x 128 kernel with its half-dead tile column gives the same bits again."""
    S._select(monkeypatch, "tile128")
    torch.manual_seed(M * K)
    x = torch.relu(torch.randn(M, K, device=DEV))
    w = torch.randn(256, K, device=DEV) / K ** 0.5
    bias = torch.randn(256, device=DEV)
    pa = S._split(x)

    def product(N, relu):
        pb = S._split(w[:N])
        out = torch.full((M, N), float("nan"), device=DEV)
        _clx.call("clx_gemm_planes", _clx.ptr(pa), _clx.ptr(pb), M, N, K, _clx.ptr(bias), relu, _clx.ptr(out), N, S._st())
        torch.cuda.synchronize()
        return out

    for relu in (0, 1):                  # (relu = 0 without bias would be the store straight from the accumulators; both go
        for narrow, wide in ((64, 128), (192, 256)):        # through the LDS epilogue here, the plain store below)
            a, b = product(narrow, relu), product(wide, relu)
            assert not torch.isnan(a).any()
            assert torch.equal(a, b[:, :narrow]), (narrow, wide, relu)
    # the plain store of whole tiles (no bias): M = 1000 has whole and ragged row tiles
    for narrow, wide in ((64, 128), (192, 256)):
        outs = []
        for N in (narrow, wide):
            pb = S._split(w[:N])
            out = torch.full((M, N), float("nan"), device=DEV)
            _clx.call("clx_gemm_planes", _clx.ptr(pa), _clx.ptr(pb), M, N, K, None, 0, _clx.ptr(out), N, S._st())
            outs.append(out)
        assert torch.equal(outs[0], outs[1][:, :narrow]), (narrow, wide)
        monkeypatch.setenv("CLX_SP_TILE", "256")
        pb = S._split(w[:narrow])
        out = torch.full((M, narrow), float("nan"), device=DEV)
        _clx.call("clx_gemm_planes", _clx.ptr(pa), _clx.ptr(pb), M, narrow, K, None, 0, _clx.ptr(out), narrow, S._st())
        assert torch.equal(out, outs[0]), narrow
        monkeypatch.setenv("CLX_SP_TILE", "128")


@pytest.mark.parametrize("rows,N,C", [(128, 64, 128), (5, 64, 128), (1000, 192, 192), (1000, 128, 192), (33000, 320, 192),
                                      (70001, 64, 768)])
def test_weight_gradient_from_planes_against_float64(rows, N, C):
    """clx_wgrad_planes with a partial last tile on either side (N below the 256 rows of a tile, C = 128 q + 64): += into
    ones, the sentinel columns past C untouched; the bars of test_gpu_sp.py's weight-gradient test."""
    torch.manual_seed(rows + N)
    x = torch.relu(torch.randn(rows, C, device=DEV))
    dy = torch.randn(rows, N, device=DEV) * (torch.rand(rows, N, device=DEV) < 0.5)          # a gated gradient
    dw = torch.full((N + 3, C + 4), 1.0, device=DEV)                                          # += into what is there
    pdy, px = S._split(dy), S._split(x)
    with S._launches() as n:
        _clx.call("clx_wgrad_planes", _clx.ptr(pdy), _clx.ptr(px), rows, N, C, _clx.ptr(dw), C + 4, S._st())
    S._expect(n, WGRAD_SP=1)
    ref = dy.double().t() @ x.double() + 1.0
    got = dw[:N, :C].double()
    assert torch.equal(dw[:, C:], torch.ones(N + 3, 4, device=DEV)) and torch.equal(dw[N:], torch.ones(3, C + 4, device=DEV))
    rms = (ref - 1.0).pow(2).mean().sqrt().item()
    rel = ((got - ref).pow(2).mean().sqrt() / rms).item()
    mean = abs(((got - ref).mean() / rms).item())
    print("\nweight gradient", (rows, N, C), "rel %.3g mean %.3g" % (rel, mean))
    assert rel < 3e-7, rel
    assert mean < 3e-8, mean


# ------------------------------------------------------------------------------------------------ 1x1 layers, forward
FWD_CASES = [
    ("default", (1, 1, 1, 1000), 192, 192),
    ("default", (1, 1, 1, 129), 320, 192),
    ("tile256", (1, 1, 1, 129), 320, 192),
    ("default", (2, 3, 5, 7), 192, 192),
]


def test_pointwise_320_to_64_stays_float32():
    """N = 64 is excluded from the precision-2 rule (it measured no faster than float32 MFMA: tests/test_cpu_sp64.py gives the
    figures): the 320 -> 64 layer on the (1, 1, 1, 129) grid runs one float32 GEMM and no split kernel under precision = 2,
    planes supplied or not, and refuses the plane hand-overs."""
    lib = _clx.load()
    grid, C, N = (1, 1, 1, 129), 320, 64
    M = 129
    torch.manual_seed(M + C + N)
    x = torch.relu(torch.randn(M, C, device=DEV))
    w = torch.randn(N, C, device=DEV) / C ** 0.5
    wp = S._pack(w, N, C, 1, 0)
    wplanes = S._split(wp.view(N, C))
    aplanes = S._ff(lib.clx_planes_bytes(M, C))
    out = torch.full((M + 3, N + 32), SENT, device=DEV)
    d = S._pw_desc(x, grid, C, N, wp, wplanes, aplanes, out, N + 32)
    d.precision = G64
    assert lib.clx_conv_sp_covers(ctypes.byref(d), 0) == 0 and lib.clx_conv_sp_covers(ctypes.byref(d), 1) == 0
    with S._launches() as n:
        _clx.call("clx_conv_fwd", ctypes.byref(d), S._st())
    assert n["IGEMM_WIDE"] + n["IGEMM_NARROW"] == 1 and n["GEMM_SP"] + n["GEMM_SP2"] + n["SPLIT_PLANES"] == 0, n
    ref = x.double() @ w.double().t()
    assert (out[:M, :N].double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    assert (out[M:] == SENT).all() and (out[:M, N:] == SENT).all()
    d.out_planes = S._ff(lib.clx_planes_bytes(M, N)).data_ptr()
    with pytest.raises(_clx.ClxError, match="out_planes"):
        _clx.call("clx_conv_fwd", ctypes.byref(d), S._st())


@pytest.mark.parametrize("kernel,grid,C,N", FWD_CASES)
def test_pointwise_forward_every_epilogue(kernel, grid, C, N, monkeypatch):
    """test_gpu_sp_conv.py::test_pointwise_forward_every_epilogue for precision = 2 at N = 192 (three 64-wide tile columns, or
    one and a half 128-wide ones; N = 64 is excluded from the rule: the test above): plain, bias + ReLU
    + gate bits out, float mask, gate bits in, accumulate, the data-gradient hand-over form (gate bits in, the output's own
    planes, its column sums) and aplanes_valid, against float64; the planes the epilogue writes equal clx_split_planes(out)
    byte for byte with zero padding rows; one split product and no float32 GEMM per call.  The same descriptor with
    precision = 1 is not covered and runs a float32 GEMM."""
    S._select(monkeypatch, kernel)
    kind = S._kind(kernel, C)
    lib = _clx.load()
    B, D, H, W = grid
    M = B * D * H * W
    torch.manual_seed(M + C + N)
    x = torch.relu(torch.randn(M, C + 4, device=DEV))[:, :C]          # (a padded leading dimension)
    w = torch.randn(N, C, device=DEV) / C ** 0.5
    bias = torch.randn(N, device=DEV)
    wp = S._pack(w, N, C, 1, 0)
    wplanes = S._split(wp.view(N, C))
    ref = x.double() @ w.double().t()
    ldo = N + 32
    aplanes = S._ff(lib.clx_planes_bytes(M, C))

    def run(setup, ld_out=ldo, valid=False, precision=G64):
        out = torch.full((M + 3, ld_out), SENT, device=DEV)
        if not valid:
            aplanes.fill_(255)
        d = S._pw_desc(x, grid, C, N, wp, wplanes, aplanes, out, ld_out)
        d.precision = precision
        setup(d, out)
        if precision == G64:
            assert lib.clx_conv_sp_covers(ctypes.byref(d), 0) == 1
            with S._launches() as n:
                _clx.call("clx_conv_fwd", ctypes.byref(d), S._st())
            S._expect(n, **{kind: 1, "SPLIT_PLANES": 0 if valid else 1})
        else:
            assert lib.clx_conv_sp_covers(ctypes.byref(d), 0) == 0
            with S._launches() as n:
                _clx.call("clx_conv_fwd", ctypes.byref(d), S._st())
            assert n["IGEMM_WIDE"] + n["IGEMM_NARROW"] == 1 and n["GEMM_SP"] + n["GEMM_SP2"] + n["SPLIT_PLANES"] == 0, n
        assert (out[M:] == SENT).all() and (out[:M, N:] == SENT).all()       # nothing past M, nothing past N
        return out[:M, :N]

    out = run(lambda d, o: None)
    S._bars(out, ref, "plain")
    out1 = run(lambda d, o: None, precision=1)                         # float32 MFMA: close, and not the split kernels
    assert (out1.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())

    gate = torch.full((M + 3, ldo // 32), 0x5A5A5A5A, dtype=torch.int32, device=DEV)

    def bias_relu(d, o):
        d.bias, d.relu = bias.data_ptr(), 1
        d.gate_out, d.ld_gate = gate.data_ptr(), ldo // 32
    out = run(bias_relu)
    S._bars(out, torch.relu(ref + bias.double()), "bias_relu")
    bits = S._unbits(gate[:M], N)
    assert torch.equal(bits, out > 0)
    assert (gate[M:] == 0x5A5A5A5A).all() and (gate[:, N // 32:] == 0x5A5A5A5A).all()      # no word past M or past N

    mask = torch.randn(M, ldo, device=DEV)

    def float_mask(d, o):
        d.mask, d.ld_mask = mask.data_ptr(), ldo
    out = run(float_mask)
    S._bars(out, ref * (mask[:, :N] > 0), "mask")

    def bit_mask(d, o):                                # the gates written above, read back as the mask
        d.mask_bits, d.ld_mask_bits = gate.data_ptr(), ldo // 32
    out = run(bit_mask)
    S._bars(out, ref * bits, "mask_bits")

    prev = torch.randn(M, ldo, device=DEV)

    def accumulate(d, o):
        o[:M, :N].copy_(prev[:, :N])
        d.accumulate, d.bias, d.relu = 1, bias.data_ptr(), 1
    out = run(accumulate)
    S._bars(out, torch.relu(ref + bias.double() + prev[:, :N].double()), "accumulate")

    # the data-gradient hand-over form: gate bits in, the output's planes and column sums out (dense output)
    out_planes = S._ff(lib.clx_planes_bytes(M, N))
    colsum = torch.full((N + 4,), 0.5, device=DEV)

    def hand_over(d, o):
        d.mask_bits, d.ld_mask_bits = gate.data_ptr(), ldo // 32
        d.out_planes, d.out_colsum = out_planes.data_ptr(), colsum.data_ptr()
    out = run(hand_over, ld_out=N)
    S._bars(out, ref * bits, "hand_over")
    S._colsum_ok(colsum[:N] - 0.5, out, "out_colsum")
    assert (colsum[N:] == 0.5).all()
    assert S._same_bits(S._join(out_planes, M, N), out)
    assert not S._tail(out_planes, M, N).any()
    assert torch.equal(out_planes, S._split(out))

    # aplanes_valid: the product reads the planes it is handed (those of another x), not src[0]
    x2 = torch.relu(torch.randn(M, C, device=DEV)) - 0.25
    aplanes.copy_(S._split(x2))
    out = run(lambda d, o: setattr(d, "aplanes_valid", 1), valid=True)
    S._bars(out, x2.double() @ w.double().t(), "aplanes_valid")


@pytest.mark.parametrize("grid,N,C,case", [((1, 1, 1, 1000), 192, 192, "fresh"), ((1, 1, 1, 129), 192, 320, "dyplanes_valid"),
                                           ((2, 3, 5, 7), 192, 192, "aplanes_valid"), ((1, 1, 1, 33001), 320, 192, "fresh")])
def test_pointwise_weight_gradient(grid, N, C, case, monkeypatch):
    """A 1x1 layer's weight gradient through clx_conv_wgrad with precision = 2 (test_gpu_sp_conv.py's test at 64-granular
    counts): fresh planes, dyplanes_valid on planes a product's epilogue wrote at N = 192, aplanes_valid; one split weight
    gradient and no float32 one.  precision = 1 on the same descriptor runs the float32 weight gradient."""
    S._select(monkeypatch, "default")
    lib = _clx.load()
    B, D, H, W = grid
    rows = B * D * H * W
    torch.manual_seed(rows + N + C)
    x = torch.relu(torch.randn(rows, C, device=DEV))
    dwp = torch.full((N, C), 1.0, device=DEV)                        # += into what is there
    dbias = torch.full((N,), 0.25, device=DEV)
    aplanes, dyplanes = S._ff(lib.clx_planes_bytes(rows, C)), S._ff(lib.clx_planes_bytes(rows, N))
    splits = 2
    xr = x
    if case == "dyplanes_valid":
        K2 = 192
        z = torch.randn(rows, K2, device=DEV)
        w2 = torch.randn(N, K2, device=DEV) / K2 ** 0.5
        wp2 = S._pack(w2, N, K2, 1, 0)
        wpl2 = S._split(wp2.view(N, K2))
        gate = S._words(torch.rand(rows, N, device=DEV) < 0.5)
        dy_buf = torch.full((rows + 3, N), SENT, device=DEV)
        zpl = S._ff(lib.clx_planes_bytes(rows, K2))
        d2 = S._pw_desc(z, grid, K2, N, wp2, wpl2, zpl, dy_buf, N)
        d2.precision = G64
        d2.mask_bits, d2.ld_mask_bits = gate.data_ptr(), N // 32
        d2.out_planes, d2.out_colsum = dyplanes.data_ptr(), dbias.data_ptr()
        with S._launches() as n:
            _clx.call("clx_conv_fwd", ctypes.byref(d2), S._st())
        S._expect(n, GEMM_SP2=1, SPLIT_PLANES=1)
        assert (dy_buf[rows:] == SENT).all()
        dy = dy_buf[:rows]
        splits = 1
    else:
        dy = torch.randn(rows, N, device=DEV) * (torch.rand(rows, N, device=DEV) < 0.5)    # a gated gradient
    if case == "aplanes_valid":
        xr = torch.relu(torch.randn(rows, C, device=DEV)) + 0.125
        aplanes.copy_(S._split(xr))
        splits = 1
    d = ClxConvDesc()
    d.nsrc = 1
    d.src[0] = S._src(x.data_ptr(), C, C, D, H, W)
    d.B, d.ID, d.IH, d.IW = B, D, H, W
    d.KD = d.KH = d.KW = 1
    d.N = N
    d.precision = G64
    d.aplanes, d.aplanes_valid = aplanes.data_ptr(), int(case == "aplanes_valid")
    d.dyplanes, d.dyplanes_valid = dyplanes.data_ptr(), int(case == "dyplanes_valid")
    assert lib.clx_conv_sp_covers(ctypes.byref(d), 1) == 1
    with S._launches() as n:
        _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy), N, _clx.ptr(dwp),
                  None if case == "dyplanes_valid" else _clx.ptr(dbias), S._st())
    S._expect(n, WGRAD_SP=1, SPLIT_PLANES=splits)
    ref = dy.double().t() @ xr.double()
    got = dwp.double() - 1.0
    rms = ref.pow(2).mean().sqrt().item()
    rel = ((got - ref).pow(2).mean().sqrt() / rms).item()
    assert rel < 3e-7, rel
    assert abs(((got - ref).mean() / rms).item()) < 3e-8
    S._colsum_ok(dbias - 0.25, dy, "dbias")
    if case == "fresh":
        d.precision = 1
        assert lib.clx_conv_sp_covers(ctypes.byref(d), 1) == 0
        with S._launches() as n:
            _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy), N, _clx.ptr(dwp), _clx.ptr(dbias), S._st())
        assert n["WGRAD"] >= 1 and n["WGRAD_SP"] + n["SPLIT_PLANES"] == 0, n


# ----------------------------------------------------------------------------------------------- a 2-D Winograd layer
@pytest.mark.parametrize("algo", [1, 2])
def test_winograd_layer_192_to_192(algo, monkeypatch):
    """Forward, weight gradient (which leaves dy_vcache) and the data gradient that reads it, of a 3x3 layer 192 -> 192 as
    F(2x2) and F(4x4) with precision = 2, B = 2 at 30 x 26 (28 x 24 outputs: 336 / 84 tiles, above and below 128 and no multiple
    of 64), against float64 and against the same calls in float32 with the bars of test_gpu_sp_conv.py (_compare: RATIO,
    SPLIT_VS_F32); precision = 1 does not cover the layer."""
    S._select(monkeypatch, "default")
    lib = _clx.load()
    k, C, N, H, W, Bw = 3, 192, 192, 30, 26, S.B_W
    torch.manual_seed(algo * 7 + 3)
    mt, a = (2 if algo == 1 else 4), S._wino_a(algo, k)
    OH, OW = H - k + 1, W - k + 1
    x = torch.randn(Bw, H, W, C)
    w = torch.randn(N, C, k, k) * (2.0 / (C * k * k)) ** 0.5
    dy = torch.randn(Bw, OH, OW, N) * (torch.rand(Bw, OH, OW, N) < 0.5)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    ref_out = F.conv2d(xr, wr)
    (ref_out * dy.permute(0, 3, 1, 2).double()).sum().backward()
    ref_out = ref_out.detach().permute(0, 2, 3, 1)
    ref_dw, ref_dx = wr.grad, xr.grad.permute(0, 2, 3, 1)
    x_d, dy_d = x.to(DEV).contiguous(), dy.to(DEV).contiguous()
    wp = S._pack(w, N, C, k * k, 2 if algo == 1 else 4)
    wpl = S._split(wp.view(a * a * N, C))
    wpd = S._pack(w, N, C, k * k, 3 if algo == 1 else 5)               # flipped filter: U[a^2][C][N]
    wpld = S._split(wpd.view(a * a * C, N))
    d1 = S._wino_desc(x_d, (Bw, H, W), algo, k, C, N, 0)
    d1.precision = 1
    assert lib.clx_conv_sp_covers(ctypes.byref(d1), 0) == 0 and lib.clx_conv_sp_covers(ctypes.byref(d1), 1) == 0
    fwd, dwg, dxg, errs = {}, {}, {}, []
    for prec in (0, G64):
        sp = int(prec == G64)
        d = S._wino_desc(x_d, (Bw, H, W), algo, k, C, N, 0)
        d.precision = prec
        assert lib.clx_conv_sp_covers(ctypes.byref(d), 0) == sp
        out = torch.full((Bw * OH * OW + 3, N + 4), SENT, device=DEV)
        d.out, d.ld_out, d.wpack = out.data_ptr(), N + 4, wp.data_ptr()
        d.wplanes = wpl.data_ptr() if sp else None
        vc = S._ff(lib.clx_conv_vcache_bytes(ctypes.byref(d), 0))
        d.vcache = vc.data_ptr()
        ws = S._ff(lib.clx_conv_workspace_bytes(ctypes.byref(d), 0))
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        with S._launches() as n:
            _clx.call("clx_conv_fwd", ctypes.byref(d), S._st())
        if sp:
            S._expect(n, GEMM_SP2=1)
        else:
            assert n["IGEMM_WIDE"] + n["IGEMM_NARROW"] >= 1 and n["GEMM_SP"] + n["GEMM_SP2"] == 0, n
        assert (out[Bw * OH * OW:] == SENT).all() and (out[:, N:] == SENT).all()
        fwd[sp] = out[:Bw * OH * OW, :N].reshape(Bw, OH, OW, N)
        # the weight gradient on the forward's V, leaving dY's padded transform for the data gradient
        d = S._wino_desc(x_d, (Bw, H, W), algo, k, C, N, 0)
        d.precision = prec
        assert lib.clx_conv_sp_covers(ctypes.byref(d), 1) == sp
        ws = S._ff(lib.clx_conv_workspace_bytes(ctypes.byref(d), 1))
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        d.vcache, d.vcache_valid = vc.data_ptr(), 1
        dyv = S._ff(lib.clx_conv_vcache_bytes(ctypes.byref(d), 1))
        d.dy_vcache = dyv.data_ptr()
        dwp = torch.zeros(a * a * N * C, device=DEV)
        db = torch.full((N,), 0.25, device=DEV)
        with S._launches() as n:
            _clx.call("clx_conv_wgrad", ctypes.byref(d), _clx.ptr(dy_d), N, _clx.ptr(dwp), _clx.ptr(db), S._st())
        if sp:
            S._expect(n, WGRAD_SP=1)
        else:
            assert n["WGRAD"] >= 1 and n["WGRAD_SP"] == 0, n
        dw = torch.empty(N, C, k * k, device=DEV)
        _clx.call("clx_unpack_wgrad_wino", _clx.ptr(dwp), _clx.ptr(dw), N, C, N, C, mt, k, 1, S._st())
        dwg[sp] = dw.view(N, C, k, k)
        S._colsum_ok((db - 0.25).cpu(), dy.reshape(-1, N), "dbias")
        # the data gradient from dy_vcache
        dd = S._wino_desc(dy_d, (Bw, OH, OW), algo, k, N, C, k - 1)
        dd.precision = prec
        dd.wpack = wpd.data_ptr()
        dd.wplanes = wpld.data_ptr() if sp else None
        assert lib.clx_conv_sp_covers(ctypes.byref(dd), 0) == sp
        ws2 = S._ff(lib.clx_conv_workspace_bytes(ctypes.byref(dd), 0))
        dd.workspace, dd.workspace_bytes = ws2.data_ptr(), ws2.numel()
        dd.vcache, dd.vcache_valid = dyv.data_ptr(), 1
        o = torch.full((Bw * H * W + 3, C), SENT, device=DEV)
        dd.out, dd.ld_out = o.data_ptr(), C
        with S._launches() as n:
            _clx.call("clx_conv_fwd", ctypes.byref(dd), S._st())
        if sp:
            S._expect(n, GEMM_SP2=1)
        assert (o[Bw * H * W:] == SENT).all()
        dxg[sp] = o[:Bw * H * W].view(Bw, H, W, C)
    S._compare(fwd, ref_out, "forward", errs)
    S._compare(dwg, ref_dw, "dw", errs)
    S._compare(dxg, ref_dx, "dx", errs)
    print("\nwinograd 192 -> 192", algo, ["%s %.3g %.3g %.3g" % e for e in errs])


# --------------------------------------------------------------------------------------------------------- networks
NETS = {
    "2d_sp64x3": dict(cfg=dict(in_channels=1, out_channels=2, num_fmaps=64, fmap_inc_factor=3, features_in_last_layer=64,
                               downsampling_factors=[[2, 2]], num_spatial_dims=2), spatial=(76, 84), batch=2),
    "3d_sp64x3": dict(cfg=dict(in_channels=1, out_channels=3, num_fmaps=64, fmap_inc_factor=3, features_in_last_layer=64,
                               downsampling_factors=[[2, 2, 2]], num_spatial_dims=3), spatial=(24, 20, 20), batch=1),
}
ALL = (True, True, True)
NONE = (False, False, False)
# plan.sp_pass[layer] = (forward, data gradient, weight gradient) under CLX_PRECISION=f32x3bf16g64: the 192 -> 192 layers of
# level 1 — the two 1x1 layers, and in 2-D the 3x3 Winograd layer.  Float32: every layer with a 64-channel side (a
# contraction of 64 in one of its three products; 1 -> 64 and 64 -> 192 among them), the 3-D Winograd layers, the
# sub-pixel layer of the right path (its own descriptors) and the head.
L1 = "backbone.l_conv.1.conv_pass."
SPLIT_LAYERS = {"2d_sp64x3": {L1 + "2": ALL, L1 + "4": ALL, L1 + "6": ALL}, "3d_sp64x3": {L1 + "2": ALL, L1 + "4": ALL}}


def _nets(monkeypatch, name):
    import test_gpu_unet as T

    monkeypatch.setitem(T.CONFIGS, name, NETS[name])
    monkeypatch.setenv("CLX_PRECISION", "f32x3bf16g64")
    return T


@pytest.mark.parametrize("name", list(NETS))
def test_networks_match_the_oracle_and_run_the_expected_layers_split(name, device, monkeypatch):
    T = _nets(monkeypatch, name)
    T.test_forward_matches_oracle(name, device)
    T.test_backward_matches_oracle(name, device)
    _o, model, raw = T._make(name, device, seed=1)
    model(raw.to(device)).sum().backward()
    plan = next(iter(model._plans.values()))
    assert plan.precision == 2
    want = {layer.name: SPLIT_LAYERS[name].get(layer.name, NONE) for layer in plan.topo.convs}
    assert plan.sp_pass == want, {k: v for k, v in plan.sp_pass.items() if v != want[k]}
    assert plan._wplanes


def test_two_stream_half_batches_under_g64(device, monkeypatch):
    T = _nets(monkeypatch, "2d_sp64x3")
    T.test_two_stream_half_batches_equal_the_one_stream_step("2d_sp64x3", device, monkeypatch)


def test_noisy_copies_through_changed_rows_under_g64(device, monkeypatch):
    """The reused test knows its own configurations by name: it expects a changed-rows prefix of every one but 2d_chain64
    and a tile list of 2d_96 / 2d_sp128 only.  At 64 feature maps the 1x1 layers of level 0 are fused pairs (no prefix), so
    CLX_CHAIN64=0 runs them one by one here, and CLX_SPARSE_TILES=0 keeps the Winograd layer behind them dense: the
    changed-rows path against the dense forward, bit for bit, under the new precision name."""
    T = _nets(monkeypatch, "2d_sp64x3")
    monkeypatch.setenv("CLX_CHAIN64", "0")
    monkeypatch.setenv("CLX_SPARSE_TILES", "0")
    T.test_noisy_copies_through_changed_rows_equal_the_dense_forward_bit_for_bit("2d_sp64x3", device, monkeypatch)


def test_default_precision_leaves_the_64x3_network_in_float32(device, monkeypatch):
    """the default name covers nothing of the same network (restated from test_gpu_unet.py, which pins it): no split pass, the
    arena bytes of CLX_PRECISION=f32; the new name takes planes — more bytes — and a split pass"""
    from cellulus_amd.models import get_model

    c = NETS["2d_sp64x3"]
    arena, split = {}, {}
    for precision in ("f32x3bf16", "f32", "f32x3bf16g64"):
        monkeypatch.setenv("CLX_PRECISION", precision)
        torch.manual_seed(7)
        model = get_model(**c["cfg"]).to(device)
        model(torch.rand(c["batch"], 1, *c["spatial"], device=device)).sum().backward()
        plan = next(iter(model._plans.values()))
        arena[precision] = plan.arena_bytes()
        split[precision] = any(any(s) for s in plan.sp_pass.values())
    assert arena["f32x3bf16"] == arena["f32"] and not split["f32x3bf16"] and not split["f32"]
    assert split["f32x3bf16g64"] and arena["f32x3bf16g64"] > arena["f32"]
