"""What a launch plan tells libclx about a convolution: the descriptor builders (clx_src, clx_conv_desc) and the codes and
rules behind their algorithm and precision fields.  FUSED_MAX_CHANNELS is read from the environment at import, every
other switch at the call that asks.  (The channel thresholds of the Winograd forms are the plan's: plan.py.)"""

import os

from .._clx import ClxConvDesc, ClxSrc

# address in the descriptors of the library's geometry-only queries (workspace and cache sizes, applicability, split-precision
# coverage), which never dereference: a plan decides with them before it owns a buffer
QUERY_PTR = 16

# per-layer algorithm code = clx_conv_algo: 0 direct, 1 Winograd F(2x2), 2 Winograd F(4x4)
# (3 = F(4x4) with the transforms inside the product kernel, forward only: clx_conv_algo CLX_ALGO_WINOGRAD4_FUSED)
WINO_PACK_FWD = {1: 2, 2: 4, 3: 7}  # clx_pack_mode
WINO_PACK_DGRAD = {1: 3, 2: 5}
WINO_TILE = {1: 2, 2: 4, 3: 4}


def winograd_code() -> int:
    return 2 if os.environ.get("CLX_WINOGRAD_TILE", "4") == "4" else 1


def wino_taps(code, kernel):
    """packed-weight / weight-gradient planes of a Winograd layer: a^2 transform points x z taps, a = tile + k - 1
    (F(2x2, 3x3): 16, F(4x4, 3x3): 36, the F(4x4, 2x2) of a sub-pixel layer's low-resolution half: 25)."""
    return (WINO_TILE[code] + kernel[1] - 1) ** 2 * kernel[0]


def packed_taps(code, kernel):
    """planes of the packed weights (or of the packed weight gradient) of a layer that runs with algorithm `code`"""
    return wino_taps(code, kernel) if code else kernel[0] * kernel[1] * kernel[2]


def pack_job_elements(cout, cin, taps, cin_pad, cout_pad, mode):
    """elements one packing writes (the arguments of clx_pack_weights behind the two pointers): clx_pack_weights_batch
    sizes its grid by the biggest job of the table"""
    if mode in (0, 1):
        return (cout if mode == 0 else cin_pad) * taps * (cin_pad if mode == 0 else cout_pad)
    if mode == 7:
        return cout_pad * cin_pad
    rows, cols = (cin_pad, cout_pad) if mode in (3, 5, 6) else (cout_pad, cin_pad)
    return rows * (3 if taps == 27 else 2 if taps == 8 else 1) * cols


# The arithmetic of the plain products (1x1 layers, the transform-domain products of the 2-D Winograd layers; forward, data
# gradient and weight gradient), clx_conv_precision:
#   "f32x3bf16" (default since round 6): every float32 operand split EXACTLY into three bfloat16 pieces, six exact products
#       per float32 product accumulated in float32 on the bf16 matrix cores (csrc/gemm_sp.hip).  Results
#       are float32; distance from the float64 oracle at a trained network's output scale 7.2e-5 (float32 MFMA: 7.3e-5).
#   "f32": float32 MFMA everywhere (v_mfma_f32_32x32x2_f32), the only arithmetic of rounds 1-5; CLX_PRECISION=f32.
#   "f32x3bf16g64" (opt-in, CLX_PRECISION=f32x3bf16g64): the arithmetic of "f32x3bf16" for channel counts that are multiples
#       of 64 instead of 128, from 128 channels on (the 192 / 576-channel layers of the 64-feature-map networks).  Which layers that reaches is the library's answer
#       (clx_conv_sp_covers; include/clx.h), as for the default: this module holds no copy of either rule.
DEFAULT_PRECISION = "f32x3bf16"
PRECISION_CODES = {"f32": 0, "f32x3bf16": 1, "f32x3bf16g64": 2}


def precision_name() -> str:
    name = os.environ.get("CLX_PRECISION", "") or DEFAULT_PRECISION
    if name not in PRECISION_CODES:
        raise ValueError(f"CLX_PRECISION must be 'f32', 'f32x3bf16' or 'f32x3bf16g64', got {name!r}")
    return name


def precision_code() -> int:
    """clx_conv_precision: 0 = float32 MFMA, 1 = the three-way bfloat16 split (CLX_PREC_F32X3BF16), 2 = the same split
    with the 64-channel granule (CLX_PREC_F32X3BF16_G64).  The run-to-run reproducible mode (CLX_DETERMINISTIC=1) exists
    in float32 only and selects it."""
    if os.environ.get("CLX_DETERMINISTIC", "0") == "1":
        return 0
    return PRECISION_CODES[precision_name()]


def winograd_enabled() -> bool:
    return os.environ.get("CLX_WINOGRAD", "1") != "0"


# The fused forms keep the products' results on chip: 36 x 32 x 64 accumulators per workgroup, i.e. 10.7 FLOP per
# byte of operands from L2 where the 128 x 128 tiles of the batched GEMMs have 32 — they top out near 110 TFLOP/s.  That
# beats the three-launch form where ITS GEMMs are short (K = C <= 256: 78-90 TFLOP/s with the transforms) or narrow
# (N = 64: HBM-bound on V and M), and loses at C = 768 (113 TFLOP/s with the transforms; tools/exp/fused_bench.py,
# DESIGN.md 3.1g).
FUSED_MAX_CHANNELS = int(os.environ.get("CLX_WINO_FUSED_MAX_CHANNELS", "256"))


def fused_pays(cin_pad: int, cout: int) -> bool:
    return cout <= 64 or cin_pad <= FUSED_MAX_CHANNELS


def fused_wanted(keep_activations: bool) -> bool:
    """2-D F(4x4) forward layers as ONE launch each (csrc/wino_fused.hip: the transformed tensors never reach HBM).
    CLX_WINO_FUSED=0 keeps the three-launch form everywhere; the training plans (which keep the transformed input for
    the weight gradient) take it with CLX_WINO_FUSED_TRAIN=1 only."""
    if os.environ.get("CLX_WINO_FUSED", "1") == "0":
        return False
    return (not keep_activations) or os.environ.get("CLX_WINO_FUSED_TRAIN", "0") == "1"


def conv_src(ptr, C, ld, shape, crop=(0, 0, 0), factor=(1, 1, 1)):
    """clx_src: a stored tensor (C of its ld channels, extent `shape`) seen through crop and nearest upsampling"""
    s = ClxSrc()
    s.ptr, s.C, s.ld = ptr, C, ld
    s.D, s.H, s.W = shape
    s.oz, s.oy, s.ox = crop
    s.fz, s.fy, s.fx = factor
    return s


def conv_desc(sources, B, in_shape, kernel, pad, N, precision, c_real=0):
    """clx_conv_desc of a convolution over `sources`.  What is not named here is what a fresh structure holds, zero and
    NULL: no bias, ReLU, mask or accumulation, the direct algorithm, no workspace — the caller sets what it uses."""
    d = ClxConvDesc()
    d.nsrc = len(sources)
    for i, s in enumerate(sources):
        d.src[i] = s
    d.B = B
    d.ID, d.IH, d.IW = in_shape
    d.KD, d.KH, d.KW = kernel
    d.PD, d.PH, d.PW = pad
    d.N = N
    d.precision = precision
    d.c_real = c_real
    return d
