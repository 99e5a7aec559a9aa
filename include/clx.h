/*
 * clx.h — C ABI of libclx.so, the MI355X (gfx950) kernel library behind
 * cellulus_amd.  Plain C: caller-owned DEVICE pointers, explicit extents, a HIP
 * stream handle.  No allocation and no ownership transfer inside the library.
 * Every entry point is asynchronous on `stream` and returns 0 on success or a
 * negative clx_status; clx_last_error() returns the message of the last
 * failure on the calling thread.
 *
 * The reference (funkelab/cellulus) is pure Python and has no FFI; what each
 * entry point replaces is the *library call* the reference makes on the hot
 * path.  The replaced call site is cited per function as
 * `cellulus/<file>:<line>` (paths relative to the reference checkout).
 *
 * Tensor layout used by all kernels: channels-last ("pixel-major"):
 *   element (b, z, y, x, c) of a (B, D, H, W) grid with C channels sits at
 *   ptr[(((b*D + z)*H + y)*W + x) * ld + c],  ld >= C, ld % 4 == 0, C % 4 == 0
 * (2-D data uses D == 1).  The reference's NCHW tensors are converted at the
 * model boundary with clx_planar_to_pixel / clx_pixel_to_planar.
 */
#ifndef CLX_H
#define CLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* clx_stream; /* hipStream_t */

enum clx_status {
  CLX_OK = 0,
  CLX_ERR_ARG = -1,    /* invalid argument / unsupported shape */
  CLX_ERR_LAUNCH = -2, /* HIP launch or runtime failure */
  CLX_ERR_WORKSPACE = -3
};

const char* clx_last_error(void);
/* Library/ABI version (bumped when a signature changes). */
int clx_abi_version(void);
/* Number of HIP devices visible to the library (0 = none; not an error). */
int clx_device_count(void);

/* Kernel timing for roofline reports: while enabled (on = 1; on = 2 also clears the
 * records, 0 disables and clears) every launch of an MFMA kernel — and of the HBM-bound kernels of
 * detect / segment listed below — carries a HIP event pair stamped with the kernel's own start and end on its stream.  clx_profile_read sums launches / milliseconds / executed FLOPs
 * (2*M*N*K per GEMM of the launch, real extents) of one kernel kind; it synchronises. */
enum clx_profile_kind {
  CLX_PROF_IGEMM_WIDE = 0,   /* conv_igemm_kernel<128,128> */
  CLX_PROF_IGEMM_NARROW = 1, /* conv_igemm_kernel<128,64>  */
  CLX_PROF_WGRAD = 2,        /* conv_wgrad_kernel<...>     */
  CLX_PROF_GEMM_SP = 3,      /* gemm_sp_kernel (and gemm_sp16_kernel, CLX_SP_MFMA=16): split-precision products
                                (clx_conv_desc.precision = CLX_PREC_F32X3BF16; FLOPs = the f32-equivalent 2*M*N*K) */
  CLX_PROF_WGRAD_SP = 4,     /* wgrad_sp_kernel: the weight gradient of the same precision */
  CLX_PROF_SPLIT_PLANES = 5, /* sp_split_kernel (HBM-bound: no FLOPs) */
  CLX_PROF_CHAIN64 = 6,      /* chain64_fwd / _bwd kernels (fused pairs of 64-channel 1x1 layers) */
  /* the HBM-bound kernels of detect / segment (no FLOPs: total_flops of these kinds is 0; the caller prices them by bytes) */
  CLX_PROF_MS_PREPARE = 7,   /* ms_flags_kernel + ms_scatter_kernel (the two launches of clx_ms_prepare / _f32) */
  CLX_PROF_MS_ASSIGN = 8,    /* ms_assign_dense / ms_assign_cells2d / ms_assign_grid / ms_assign kernels */
  CLX_PROF_CC = 9,           /* every kernel of clx_label_filter (connected components + size filter + relabel) */
  CLX_PROF_GROW_SHRINK = 10, /* every kernel of clx_grow_shrink */
  CLX_PROF_MINMAX = 11,      /* minmax_init + minmax_kernel */
  CLX_PROF_HISTOGRAM = 12,   /* histogram_kernel */
  CLX_PROF_NOISE_STATS = 13, /* noise_stats kernels */
  CLX_PROF_WINO_FUSED = 14,  /* wino_fused_kernel (CLX_ALGO_WINOGRAD4_FUSED; FLOPs = 2 * a^2 * tiles * N * C executed) */
  CLX_PROF_WINO_TRANSFORM = 15, /* the HBM-bound transform kernels of CLX_ALGO_WINOGRAD / _WINOGRAD4 (no FLOPs) */
  CLX_PROF_GEMM_SP2 = 16     /* gemm_sp2_kernel: the split-precision product on 128 x 128 (N % 128 == 64: 128 x 64) tiles, two workgroups per CU (K <= 1024) */
};
int clx_profile_enable(int on);
int clx_profile_read(int kind, double* launches, double* total_ms, double* total_flops);
/* Shader clock the MFMA kernels actually ran at: the middle block of every clx_conv_fwd GEMM launch adds the shader-clock
 * ticks and the 100-MHz wall-clock ticks of its own life to two device counters; this reads (and optionally resets)
 * them: MHz = 100 * shader_ticks / wall_ticks.  Synchronises the device.  (Measurement only: no reference counterpart.) */
int clx_profile_clock(double* shader_ticks, double* wall_ticks_100mhz, int reset);

/* ------------------------------------------------------------------------ */
/* Convolution (valid, stride 1, kernel extent 1 or 3 per dim)              */
/* replaces: nn.Conv{2,3}d + nn.ReLU inside funlib ConvPass and the 1x1     */
/* head (cellulus/models/unet.py:24-63), their autograd backward            */
/* (cellulus/train.py:178), nn.Upsample(nearest) + centre-crop + torch.cat  */
/* of the U-Net's right path (fused into the A-operand gather).             */
/* ------------------------------------------------------------------------ */

/* One input source of a convolution.  The convolution reads a *logical* input
 * grid of extent (ID, IH, IW); logical voxel l of source s is stored at grid
 * position ((l + o) / f) of the source's (D, H, W) array — `o` is a crop
 * offset, `f` a nearest-neighbour upsampling factor (1 = none). */
typedef struct clx_src {
  const float* ptr;
  int C;          /* channels taken from this source (multiple of 4) */
  int ld;         /* floats between consecutive pixels */
  int D, H, W;    /* stored grid extent */
  int oz, oy, ox; /* crop offset (in logical = upsampled coordinates) */
  int fz, fy, fx; /* nearest upsample factor per dim, >= 1 */
} clx_src;

typedef struct clx_conv_desc {
  int nsrc;       /* 1 or 2; channels of src[0] come first (torch.cat order) */
  clx_src src[2];
  int B;
  int ID, IH, IW; /* logical input extent */
  int KD, KH, KW; /* kernel extent, each 1, 2 or 3 */
  int PD, PH, PW; /* zero padding per side (0 for the valid forward conv) */
  int N;          /* output channels actually computed (<= ld_out) */
  const float* wpack; /* [N][KD*KH*KW][Ctot] packed weights (clx_pack_weights) */
  const float* bias;  /* [N] or NULL */
  int relu;           /* epilogue: max(0, .) */
  const float* mask;  /* optional [M][ld_mask]: out *= (mask > 0) (ReLU backward) */
  int ld_mask;
  float* out;         /* [M][ld_out], M = B*OD*OH*OW, O = I + 2P - K + 1 */
  int ld_out;
  int accumulate;     /* epilogue: out = act(conv + bias + out) (residual already in `out`) */
  int algo;           /* clx_conv_algo: 0 = direct implicit GEMM */
  void* workspace;    /* CLX_ALGO_WINOGRAD*: clx_conv_workspace_bytes() bytes of scratch */
  size_t workspace_bytes;
  /* Winograd only, optional: a^2 * T * C floats (the head of the workspace layout) that hold the
   * transformed input V = B^T d B instead of the workspace.  clx_conv_fwd writes it; a later
   * clx_conv_wgrad of the same layer with vcache_valid = 1 reads it and skips its own input
   * transform (the forward and the weight gradient transform the same tensor); clx_conv_fwd with
   * vcache_valid = 1 takes V from it instead of transforming (see dy_vcache). */
  void* vcache;
  int vcache_valid;
  /* Hint, 0 = unknown: only the first c_real channels of src[0] can be non-zero (the rest is the
   * padding of a 1-, 2- or 3-channel raw image up to 4).  Kernels may skip the padding; the weight
   * gradient then leaves the padded channels of dwpack untouched (clx_unpack_wgrad drops them). */
  int c_real;
  /* Winograd, optional: clx_conv_wgrad also writes the input transform of dY that the data gradient
   * of the same layer needs (zero padding K - 1) into this buffer — a^2 * T_d * N floats, T_d = B *
   * output planes * ceil((OH + K - 1) / tile) * ceil((OW + K - 1) / tile) — reading dY once for both
   * transforms; the following clx_conv_fwd (data-gradient form) then sets vcache = this buffer and
   * vcache_valid = 1 and skips its own input transform.  dY must be dense (ld_dy == N). */
  void* dy_vcache;
  /* ReLU gates as bits (optional, both may be NULL).  gate_out: with relu = 1, also write
   * bit (n & 31) of word gate_out[m * ld_gate + (n >> 5)] = (out[m][n] > 0); requires ld_out % 32 == 0
   * (whole words per pixel; bits of channels >= N are written as 0).  mask_bits: the same layout
   * read INSTEAD of `mask` in the epilogue (out *= gate): 1/32 of the bytes of the float mask, which
   * is what the data-gradient of a 1x1 layer — HBM-bound at 64 channels — otherwise reads in full. */
  unsigned int* gate_out;
  int ld_gate;
  const unsigned int* mask_bits;
  int ld_mask_bits;
  /* clx_conv_wgrad only, optional: run-to-run REPRODUCIBLE weight gradients (the reference's CPU
   * autograd, cellulus/train.py:177-179, is deterministic; the default split-K combine is not:
   * float atomics arrive in any order).  With det_turns != NULL (clx_conv_wgrad_turns_bytes(d)
   * bytes of device scratch) the pixel slices of an output tile add their partial sums in slice
   * order — each block waits for its predecessor's turn counter — and the first-layer kernels
   * (whose block sums meet in LDS atomics) are not used.  Pass dbias = NULL with it and take the
   * bias gradient from clx_colsum_ordered. */
  int* det_turns;
  /* clx_conv_fwd in its data-gradient form, CLX_ALGO_WINOGRAD4 with a 3x3 (2-D) or 3x3x3 kernel only: ADJOINT
   * form.  The call must directly follow the clx_conv_wgrad of the same layer with the same workspace: the
   * weight gradient's A dY A^T (left in the workspace) is the operand — dX = sum over tiles of
   * B [U^T (A dY A^T)] B^T — so dY is not transformed a second time (src[0].ptr is not read).  wpack must come
   * from clx_pack_weights(CLX_PACK_WINO4_ADJOINT).  Epilogues: mask / mask_bits (no bias, ReLU, accumulate). */
  int adjoint;
  /* clx_conv_fwd, Winograd algorithms on 2-D layers (KD = 1) only, optional: ALSO write the 2 x 2 max-pooled output
   * (funlib's Downsample after a level's last convolution, cellulus/models/unet.py:24-51: nn.MaxPool2d(2) of this very
   * tensor) — pool_out[(b, y / 2, x / 2)][n] = max over the 2 x 2 window of out, after bias / ReLU / mask —, whose four
   * pixels lie inside one output tile of the transform: the separate pooling pass (a full read of `out`) disappears.
   * Output height and width must be even; ld_pool % 4 == 0; the same values clx_maxpool_fwd(out, 1, 2, 2) writes. */
  float* pool_out;
  int ld_pool;
  /* clx_conv_fwd, Winograd algorithms on 2-D layers (KD = 1) only, optional: compute ONLY the output tiles listed —
   * tile_list[i] = (b * th + ty) * tw + tx with th x tw = ceil(OH / tile) x ceil(OW / tile) tiles per image — and leave
   * every other element of `out` (and `pool_out`) untouched: the noisy copies of one image differ from it in some
   * tiles only (the caller has put the clean image's output under every copy).  The transforms and the
   * batched products see tile_count tiles; each listed tile gets the bits the full computation gives it.  No
   * vcache / accumulate with a list. */
  const int* tile_list;
  int tile_count;
  /* clx_conv_precision.  CLX_PREC_F32 (0): float32 MFMA — the reference's arithmetic.
   * The default at each layer: this C ABI — CLX_PREC_F32, the value of a zeroed descriptor; the Python layer
   * (models/plan.py, DEFAULT_PRECISION) — CLX_PREC_F32X3BF16 ("f32x3bf16"; CLX_PRECISION=f32 selects float32 and
   * CLX_PRECISION=f32x3bf16g64 the wider rules below; CLX_DETERMINISTIC=1 forces float32); bench.py — whatever the Python
   * layer resolves, unless --precision names one.
   * CLX_PREC_F32X3BF16: where the convolution is a plain matrix product — 1x1 layers, the transform-domain products of the 2-D Winograd layers,
   * forward, data gradient and weight gradient; N % 128 == 0, contraction length % 64 == 0 and >= 128 — the operands
   * are split exactly into three bfloat16 pieces (each rounded to nearest) and six exact products per float32 product are
   * accumulated in float32 on the bf16 matrix cores ("P3 planes" above; csrc/gemm_sp.hip).  Everything else stays on the
   * float32 kernels.
   * CLX_PREC_F32X3BF16_G64 (opt-in): the same arithmetic, kernels and plane hand-overs under the channel granule of the
   * planes, 64, instead of the 128 of the first kernels' tiles — the 192 / 320 / 576-channel layers of the 64-feature-map
   * networks (both channel counts at least 128: N = 64 does not pay and stays float32).  Rules:
   * clx_conv_sp_covers below.  What CLX_PREC_F32X3BF16 covers, this value covers with the same launches and bits.
   * The planes of the weights come from the caller (wplanes: clx_split_planes of `wpack` seen as [rows][K], K = the
   * product's contraction length — Ctot for a 1x1 layer, KD * C per transform point for a Winograd layer — refreshed
   * whenever wpack is); those of the activations are made by the library: by the Winograd transforms themselves inside
   * `workspace` / `vcache` (clx_conv_workspace_bytes and clx_conv_vcache_bytes grow accordingly), by a split pass into
   * `aplanes` (clx_planes_bytes(M, C) bytes of scratch) for a 1x1 layer.  A layer without wplanes (or a 1x1 layer
   * without aplanes) runs in float32.  clx_conv_sp_covers(d, pass) says, from geometry and precision alone, which calls run
   * in this precision once the planes are supplied.
   * aplanes_valid = 1: `aplanes` already holds the planes of src[0] (an earlier call of the same layer left them: the
   * forward pass for the weight gradient, the weight gradient's dyplanes for the data gradient) — no split pass.
   * dyplanes (clx_conv_wgrad of a 1x1 layer only): clx_planes_bytes(M, N) bytes that receive the planes of dY; the bias
   * gradient comes out of that split pass.
   * out_planes / out_colsum (clx_conv_fwd of a 1x1 layer that runs in this precision, dense output ld_out == N): the
   * epilogue ALSO writes the P3 planes of `out` (clx_planes_bytes(M, N) bytes: the operand planes of the layer that reads
   * `out` next — its aplanes with aplanes_valid = 1, or a weight gradient's dyplanes with dyplanes_valid = 1) and adds the
   * column sums of `out` into out_colsum[N] (the bias gradient of the layer whose dY this data-gradient call produces).
   * Only the split 1x1 product honours out_planes / out_colsum / aplanes_valid: clx_conv_fwd refuses them (an error before
   * any launch) on every other path — Winograd, fused, small-channel, float32, or planes missing.  Likewise
   * clx_conv_wgrad refuses aplanes_valid / dyplanes_valid on a call that will not read the planes. */
  int precision;
  const void* wplanes;
  void* aplanes;
  int aplanes_valid;
  void* dyplanes;
  int dyplanes_valid;   /* clx_conv_wgrad: dyplanes already hold the planes of dY (and dbias has been taken care of) */
  void* out_planes;
  float* out_colsum;
} clx_conv_desc;

enum clx_conv_precision { CLX_PREC_F32 = 0, CLX_PREC_F32X3BF16 = 1, CLX_PREC_F32X3BF16_G64 = 2 };

enum clx_conv_algo {
  CLX_ALGO_DIRECT = 0,
  /* Winograd F(2x2, 3x3) for 2-D 3x3 convolutions (KD = 1, one source, no upsampling):
   * input transform -> 16 batched f32-MFMA GEMMs over C -> output transform; 2.25x fewer
   * multiplications than the direct form, f32 throughout (error ~7e-7 of the output range on a
   * 768-channel layer, the direct kernel ~4e-7).
   * wpack must come from clx_pack_weights(CLX_PACK_WINO_FWD / _WINO_DGRAD). */
  CLX_ALGO_WINOGRAD = 1,
  /* Winograd F(4x4, 3x3), interpolation points {0, 1, -1, 1/2, -2}: 36 batched GEMMs per 4x4
   * outputs, 4x fewer multiplications than the direct form; f32 throughout, error ~5e-6 of the
   * output range on a 768-channel layer (F(2x2): ~7e-7, direct: ~4e-7).
   * wpack must come from clx_pack_weights(CLX_PACK_WINO4_FWD / _WINO4_DGRAD).
   * Also accepts 2x2 kernels (F(4x4, 2x2), points {0, 1, -1, 1/2}: 25 GEMMs per 4x4 outputs
   * instead of 64 multiplications) — the low-resolution half of the sub-pixel upsample conv —
   * and 3-D layers with cubic kernels (3x3x3, 2x2x2; PD = PH): the transform is applied in
   * (y, x) per z plane and the z taps stay a contraction inside the batched GEMMs
   * (K = KD * C), i.e. 4x / 2.56x fewer multiplications in 3-D as well. */
  CLX_ALGO_WINOGRAD4 = 2,
  /* The same F(4x4, 3x3) / F(4x4, 2x2) arithmetic for 2-D valid layers in ONE launch and without workspace: a
   * workgroup owns 32 output tiles x 64 output channels and ALL 36 (25) transform-domain products of them — the input
   * transform of 8 channels at a time goes through LDS into the MFMA A operand, the 36 x 32 x 64 accumulators live
   * in the registers of 8 waves, the weights arrive as ready-made B fragments (CLX_PACK_WINO4_FUSED), the output
   * transform + bias / ReLU / accumulate / gate bits / 2 x 2 pooling runs on the accumulators through LDS.  The
   * transformed tensors V and M (2.25x the activation each, written and read once by CLX_ALGO_WINOGRAD4) never
   * exist in HBM.  Layers with N > 64 given clx_conv_fused_workspace_bytes(d) of workspace run as TWO launches instead
   * (input transform once, then products + output transform: only M stays on chip).  Requires
   * clx_conv_fused_applicable(d); honours tile_list / pool_out / gate_out / accumulate, knows neither mask / mask_bits
   * nor vcache (forward form only). */
  CLX_ALGO_WINOGRAD4_FUSED = 3
};
/* 1 if clx_conv_fwd accepts `d` with algo = CLX_ALGO_WINOGRAD4_FUSED (2-D valid 3x3 or 2x2 layer, one plain source with
 * C % 8 == 0 and a tensor below 4 GB, N % 64 == 0), else 0. */
int clx_conv_fused_applicable(const clx_conv_desc* d);
/* Scratch bytes CLX_ALGO_WINOGRAD4_FUSED wants in clx_conv_desc.workspace (0 = none: N = 64, everything in one launch).
 * With it (N > 64) the input is transformed ONCE by a launch of its own into the workspace, in the MFMA-fragment order
 * the product kernel loads straight into registers, and only the products' results M stay on chip; without it the
 * one-launch form runs (every block of 64 output channels transforms its input again). */
size_t clx_conv_fused_workspace_bytes(const clx_conv_desc* d);
enum clx_conv_pass { CLX_PASS_FWD = 0, CLX_PASS_WGRAD = 1 };
/* Scratch bytes clx_conv_fwd (pass FWD; also the dgrad form) / clx_conv_wgrad (pass WGRAD)
 * need for descriptor `d` with algo = CLX_ALGO_WINOGRAD / _WINOGRAD4; 0 if Winograd does not apply to
 * the geometry (the caller must then use CLX_ALGO_DIRECT). */
size_t clx_conv_workspace_bytes(const clx_conv_desc* d, int pass);
/* Bytes of the buffers a caller may hand to a Winograd layer to carry transformed tensors from one call to the next:
 * which = 0: clx_conv_desc.vcache (V = B^T d B of the layer's input: written by clx_conv_fwd, reused by clx_conv_wgrad);
 * which = 1: clx_conv_desc.dy_vcache (the data gradient's input transform of dY, written by clx_conv_wgrad).  Float32
 * tensors, or P3 planes — 1.5x the bytes — where the layer runs in the split precision (clx_conv_sp_covers).  0 if
 * Winograd does not apply. */
size_t clx_conv_vcache_bytes(const clx_conv_desc* d, int which);

/* ---- Split-precision operands ("P3 planes", round 6) ----
 * The precision CLX_PREC_F32X3BF16 of clx_conv_desc computes float32 products on the bf16 matrix cores: every operand
 * element is split EXACTLY into three bfloat16 pieces x = h0 + h1 + h2 (round to nearest: h0 = rn(x), h1 = rn(x - h0),
 * h2 = x - h0 - h1; csrc/sp_planes.h) and the six products a_i b_j, i + j <= 2, are accumulated in float32
 * (v_mfma_f32_32x32x16_bf16) — the dropped terms are <= 2^-25 relative, below one float32 rounding.  The pieces are
 * made ONCE where a tensor is produced, in the layout the matrix core consumes ("P3"): an [R][K] operand (K % 16 == 0) as 1-KB fragments, fragment (rb, ks, p) = piece p of
 * rows 32 rb .. 32 rb + 31, k = 16 ks .. 16 ks + 15 at byte ((rb * K/16 + ks) * 3 + p) * 1024; inside a fragment the 16 bytes
 * at 512 h + 16 r hold x_p[32 rb + r][16 ks + 8 h .. + 7].  Rows up to the next multiple of 64 (at least 128 rows) exist and are ZERO.  6 bytes
 * per element.  (No reference counterpart: the reference's torch.nn.Conv{2,3}d keep float32 operands,
 * cellulus/models/unet.py:24-63.) */
/* bytes of the P3 planes of an [rows][K] operand (0 if K % 16 != 0) */
size_t clx_planes_bytes(long long rows, int K);
/* planes <- split(x[rows][ld], columns [0, K)).  x and planes 16-byte aligned, ld % 4 == 0, K % 16 == 0. */
int clx_split_planes(const float* x, long long ld, long long rows, int K, void* planes, clx_stream stream);
/* x[rows][ld] <- h0 + h1 + h2 of the planes (exact; tests and diagnostics) */
int clx_join_planes(const void* planes, long long rows, int K, float* x, long long ld, clx_stream stream);
/* out[m][n] = act(sum_k A[m][k] B[n][k] + bias[n]) from the P3 planes of A ([M][K]) and B ([N][K]): N % 64 == 0,
 * K % 64 == 0, K >= 128, ld_out % 4 == 0.  The plain-product form of clx_conv_fwd with precision = CLX_PREC_F32X3BF16 /
 * _G64 (which splits / reuses planes by itself); exported for tests and for callers that keep planes of their own.
 * Per output element the arithmetic does not depend on N or on the tile: with the same operand rows the N = 64 result equals
 * columns [0, 64) of the N = 128 one bit for bit.
 * Environment, read per launch: CLX_SP_TILE=128 — the two-workgroups-per-CU kernel always (128 x 128 tiles; 128 x 64 tiles
 * throughout where N % 128 == 64), =256 — the 256 x 128 kernel always (N % 128 == 64: its last tile column half dead),
 * unset — the former up to K = CLX_SP_TILE_MAXK (default 1024), the latter beyond, whatever N;
 * CLX_SP_MFMA=16 — the 16 x 16 x 32 form of the 256 x 128 kernel for N % 128 == 0 (other N fall back to the 32 x 32 x 16 kernels
 * above). */
int clx_gemm_planes(const void* a_planes, const void* b_planes, int M, int N, int K, const float* bias, int relu,
                    float* out, int ld_out, clx_stream stream);
/* dw[n][c] += sum over rows of dY[row][n] * x[row][c] from the P3 planes of dY ([rows][N]) and x ([rows][C]), N % 64 == 0,
 * C % 64 == 0, C >= 128: float atomics into the caller's (zeroed or accumulating) dw[N][ld_dw] (256 x 128 tiles of dW; rows
 * and columns of a last partial tile are computed and not added).  The plain-product form of clx_conv_wgrad with
 * precision = CLX_PREC_F32X3BF16 / _G64 (replaces the autograd weight gradient of nn.Conv{2,3}d, cellulus/train.py:178). */
int clx_wgrad_planes(const void* dy_planes, const void* x_planes, long long rows, int N, int C, float* dw, int ld_dw,
                     clx_stream stream);

/* 1 if a call of pass `pass` (CLX_PASS_FWD: clx_conv_fwd, the data-gradient form included — ask with the data-gradient
 * descriptor; CLX_PASS_WGRAD: clx_conv_wgrad) with descriptor `d` runs its products in the split precision once the planes
 * buffers are supplied, else 0.  Judges `algo`, geometry and `precision` only — no pointer field is read, so a caller can
 * ask before it allocates:
 *   CLX_ALGO_DIRECT, FWD:   1x1 layer over one plain source (no padding, crop or upsampling), N % 128 == 0, C % 64 == 0,
 *                           C >= 128 — the form that honours out_planes / out_colsum / aplanes_valid;
 *   CLX_ALGO_DIRECT, WGRAD: the same layer with N % 128 == 0, C % 128 == 0 and the operand planes below 4 GB;
 *   CLX_ALGO_WINOGRAD / _WINOGRAD4, either pass: 2-D layer, N % 128 == 0, C % 128 == 0, one transform point's planes below
 *                           4 GB (forward, data gradient and weight gradient of a layer share V / A dY A^T as planes);
 *   CLX_ALGO_WINOGRAD4_FUSED: 0 (float32 throughout).
 * precision = CLX_PREC_F32X3BF16_G64 answers by the 64-channel granule instead:
 *   CLX_ALGO_DIRECT, FWD:   N % 64 == 0, C % 64 == 0, both >= 128 (a data-gradient descriptor has N and C swapped; passes are
 *                           judged one by one, and with both counts >= 128 a layer's three passes get the same answer);
 *   CLX_ALGO_DIRECT, WGRAD: N % 64 == 0, C % 64 == 0, both >= 128 and the operand planes below 4 GB;
 *                           (N = 64 is excluded although the kernels cover it — clx_gemm_planes / clx_wgrad_planes take it —:
 *                           one 64-wide tile column reads 6-byte planes once for 128 FLOPs per element, HBM-bound at the
 *                           ~105 TFLOP/s float32 MFMA reaches there, and the weight gradient fills a quarter of its tile
 *                           rows: measured x0.92 .. x1.03 and x0.55 .. x0.62 of float32 MFMA, profiles/sp64.txt)
 *   CLX_ALGO_WINOGRAD / _WINOGRAD4, either pass: 2-D layer, both counts % 64 == 0 and >= 128 (each is the contraction
 *                           length of one of the layer's three products), one transform point's planes below 4 GB;
 *   3-D Winograd and CLX_ALGO_WINOGRAD4_FUSED: 0.
 * clx_conv_vcache_bytes, clx_conv_workspace_bytes and the out_planes / aplanes_valid / dyplanes_valid refusals follow the
 * same answers.  precision = CLX_PREC_F32X3BF16 answers as it always has.
 * The launches still run in float32 where wplanes (or, for a 1x1 layer, aplanes / dyplanes) are missing. */
int clx_conv_sp_covers(const clx_conv_desc* d, int pass);

/* out = act(conv(in) + bias).  f32 MFMA implicit GEMM (M = output pixels,
 * N = output channels, K = taps x channels). Also used for the data gradient
 * (PD = K-1, weights packed with CLX_PACK_DGRAD). */
int clx_conv_fwd(const clx_conv_desc* d, clx_stream stream);

/* Bytes of device scratch clx_conv_desc.det_turns needs for this layer (0 if d is NULL). */
size_t clx_conv_wgrad_turns_bytes(const clx_conv_desc* d);
/* out[n] += sum_m x[m][n] (ADDS into out, like the bias path of clx_conv_wgrad: zero it once per step) in a FIXED order (block partials over contiguous row ranges, then one pass
 * over the partials in block order): the reproducible bias gradient, db = column sums of dY
 * (autograd of nn.ConvNd's bias, cellulus/train.py:178).  scratch: clx_colsum_scratch_bytes(N). */
size_t clx_colsum_scratch_bytes(int N);
int clx_colsum_ordered(const float* x, int ld, long long M, int N, float* out, void* scratch, clx_stream stream);

/* Two consecutive 1x1 convolutions over 64 channels in one pass over the pixels — the
 * `conv_pass.2 -> conv_pass.4` pair of every funlib ConvPass the reference builds
 * (cellulus/models/unet.py:24-51: kernel sizes [3, 1, 1, 3]) and the head
 * `head.0 -> head.2` (unet.py:52-63), where the level is 64 channels wide (HBM-bound layers):
 *   y1 = relu(x w1^T + b1)           [M][ld_y1]  (y1 may be NULL: inference keeps nothing)
 *   y2 = act(y1 w2^T + b2)           [M][ld_y2], N2 = 64 or <= 32 channels, act = ReLU if relu2
 * w1 / w2: forward packs of clx_pack_weights (CLX_PACK_FWD, one tap): [64][64] and [pad4(N2)][64].
 * gate1 / gate2: optional ReLU gates as bits (layout of clx_conv_desc.gate_out).
 * Same arithmetic as two clx_conv_fwd calls (f32 MFMA, f32 accumulation over the 64 channels). */
int clx_chain64_fwd(const float* x, int ld_x, long long M, const float* w1, const float* b1, float* y1,
                    int ld_y1, unsigned int* gate1, int ld_gate1, const float* w2, const float* b2, int N2,
                    int relu2, float* y2, int ld_y2, unsigned int* gate2, int ld_gate2, clx_stream stream);
/* Backward of that pair in one pass (autograd of the two convolutions in cellulus/train.py:178):
 *   dP1 = (dp2 w2) * (y1 > 0)   — never written —   dp0 = (dP1 w1) * (x > 0 if gate_x)
 *   dw2[n][c] += sum_p dp2[p][n] y1[p][c],  db2[n] += sum_p dp2[p][n]      ([pad4(N2)][64], [N2])
 *   dw1[n][c] += sum_p dP1[p][n] x[p][c],   db1[n] += sum_p dP1[p][n]      ([64][64], [64])
 * dp2: gradient w.r.t. layer 2's PRE-activation, [M][ld_dp2], N2 = 64 or <= 8 channels;
 * w2t / w1t: data-gradient packs (CLX_PACK_DGRAD, one tap): [64][pad4(N2)] and [64][64];
 * dw*: the dwpack layout of clx_conv_wgrad (one tap), accumulated with float atomics;
 * dp0 may be NULL (no data gradient wanted), db* may be NULL. */
int clx_chain64_bwd(const float* dp2, int ld_dp2, int N2, const float* y1, int ld_y1, const float* x,
                    int ld_x, int gate_x, long long M, const float* w2t, const float* w1t, float* dp0,
                    int ld_dp0, float* dw2, float* db2, float* dw1, float* db1, clx_stream stream);

/* Weight gradient of the convolution described by `d` (d->out/bias/relu/mask/
 * wpack ignored): dwpack[tap][n][c] += sum_p dy[p][n] * in[p (+) tap][c],
 * dbias[n] += sum_p dy[p][n]  (dbias may be NULL).  Both outputs are
 * ACCUMULATED with float atomics (split-K): zero them first.
 * dy: [M][ld_dy] gradient w.r.t. the pre-activation output.
 * Validates the descriptor like clx_conv_fwd (extents, kernel 1..3, padding < kernel, input >= kernel, every
 * source's channels / ld / alignment / factors / crop and that it covers the logical input, M < 2^31) before any
 * dispatch, whatever the algo: a descriptor clx_conv_fwd refuses is refused here with the same message. */
int clx_conv_wgrad(const clx_conv_desc* d, const float* dy, int ld_dy,
                   float* dwpack, float* dbias, clx_stream stream);

enum clx_pack_mode {
  CLX_PACK_FWD = 0,        /* w[n][c][tap] -> wp[n][tap][cpad]               */
  CLX_PACK_DGRAD = 1,      /* w[n][c][tap] -> wp[c][flip(tap)][npad] (rows c < cpad) */
  CLX_PACK_WINO_FWD = 2,   /* 3x3 only: U[16][cout_pad][cin_pad] = G g G^T             */
  CLX_PACK_WINO_DGRAD = 3, /* 3x3 only: U[16][cin_pad][cout_pad] of the flipped filter */
  CLX_PACK_WINO4_FWD = 4,  /* F(4x4): taps 9 -> U[36][cout_pad][cin_pad], taps 4 (2x2) -> U[25][..],
                            * taps 27 / 8 (3-D) -> U[36 | 25][cout_pad][kd][cin_pad]            */
  CLX_PACK_WINO4_DGRAD = 5, /* the same for the flipped filter: U[a*a][cin_pad][kd][cout_pad]    */
  CLX_PACK_WINO4_ADJOINT = 6, /* F(4x4, 3x3[x3]): the FORWARD filter transform stored transposed (z taps reversed),
                               * U[36][cin_pad][kd][cout_pad] (clx_conv_desc.adjoint) */
  CLX_PACK_WINO4_FUSED = 7    /* 2-D F(4x4, 3x3) / F(4x4, 2x2) for CLX_ALGO_WINOGRAD4_FUSED: the values of _WINO4_FWD in the
                               * MFMA-fragment order the fused kernel's waves load straight into registers,
                               * [cout_pad / 64][cin_pad / 8][36 | 25][2][64 lanes][4]; cout_pad % 64 == 0, cin_pad % 8 == 0 */
};
/* Repack torch-layout conv weights w (Cout, Cin, taps) for clx_conv_fwd.
 * cin_pad/cout_pad >= real extents (multiples of 4), padding is zero-filled.
 * FWD:   wp is [Cout][taps][cin_pad].
 * DGRAD: wp is [cin_pad][taps][cout_pad] with the taps reversed. */
int clx_pack_weights(const float* w, float* wp, int cout, int cin, int taps,
                     int cin_pad, int cout_pad, int mode, clx_stream stream);
/* All the weight packings of a step in ONE launch (a step packs ~20 small layers, forward and data-gradient
 * form each: as separate launches they are latency-bound).  `jobs`: DEVICE array of njobs descriptors, each
 * exactly the arguments of one clx_pack_weights call; max_total: the largest element count of a job's packed
 * output (sizes the grid).  Same results as the single calls. */
typedef struct clx_pack_job {
  const float* w;
  float* wp;
  int cout, cin, taps, cin_pad, cout_pad, mode;
} clx_pack_job;
int clx_pack_weights_batch(const clx_pack_job* jobs, int njobs, long long max_total, clx_stream stream);
/* dw[n][c][tap] = dwpack[tap][n][c] for n < cout, c < cin  (wgrad output ->
 * torch layout). dwpack is [taps][rows][cin_pad], rows >= cout. */
int clx_unpack_wgrad(const float* dwpack, float* dw, int cout, int cin, int taps,
                     int rows, int cin_pad, clx_stream stream);
/* Winograd wgrad output dU[a*a][rows][cin_pad] (a = tile + ksize - 1; (tile, ksize) = (2, 3),
 * (4, 3) or (4, 2)) -> dw[n][c][kd][ksize x ksize] = G^T dU G per z tap (torch layout);
 * kd = 1 for 2-D layers, kd = ksize for the 3-D form of CLX_ALGO_WINOGRAD4. */
int clx_unpack_wgrad_wino(const float* du, float* dw, int cout, int cin, int rows,
                          int cin_pad, int tile, int ksize, int kd, clx_stream stream);

/* (B, C, n) planar <-> (B, n, ld) pixel-major; channels c >= C of the
 * pixel-major side are written as zero / ignored. */
int clx_planar_to_pixel(const float* planar, float* pixel, int B, int C,
                        long long n, int ld, clx_stream stream);
int clx_pixel_to_planar(const float* pixel, float* planar, int B, int C,
                        long long n, int ld, clx_stream stream);

/* Sub-pixel re-indexing used to run the convolution over a nearest-upsampled tensor on
 * the LOW-resolution grid: with P = fz*fy*fx phases,
 *   depth_to_space: hi[(b, z*fz+a, y*fy+bb, x*fx+c)][n] = lo[(b,z,y,x)][((a*fy+bb)*fx+c)*N + n]
 *   space_to_depth: the inverse gather.
 * lo: (B, D, H, W) grid, P*N channels (pixel stride ld_lo); hi: (B, D*fz, H*fy, W*fx) grid,
 * N channels (pixel stride ld_hi). N % 4 == 0. */
int clx_depth_to_space(const float* lo, int ld_lo, float* hi, int ld_hi, int B, int D, int H,
                       int W, int N, int fz, int fy, int fx, clx_stream stream);
int clx_space_to_depth(const float* hi, int ld_hi, float* lo, int ld_lo, int B, int D, int H,
                       int W, int N, int fz, int fy, int fx, clx_stream stream);

/* Weights of the sub-pixel form: w (cout, cin, kd, kh, kw) with cin = C0 (skip half) + C1
 * (upsampled half) -> w_skip (cout, C0, taps) and weff (P*N, C1, ztaps), P = fz*fy*fx phases, N >=
 * cout rows per phase (padding rows zero), low-res kernel 2 along axes with factor 2 (taps {0,1} |
 * {2} for even, {0} | {1,2} for odd output positions summed), unchanged along axes with factor 1.
 * clx_subpixel_fold_grads is the adjoint: gradients of w_skip / weff -> gradient of w. */
int clx_subpixel_split_weights(const float* w, float* w_skip, float* weff, int cout, int cin,
                               int C0, int N, int kd, int kh, int kw, int fz, int fy, int fx,
                               clx_stream stream);
int clx_subpixel_fold_grads(const float* g_skip, const float* g_eff, float* gw, int cout, int cin,
                            int C0, int N, int kd, int kh, int kw, int fz, int fy, int fx,
                            clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Max pooling / upsample backward (funlib Downsample / Upsample,           */
/* cellulus/models/unet.py:24-51)                                           */
/* ------------------------------------------------------------------------ */
/* y = maxpool(x), window = stride = (fz, fy, fx); extents must divide. */
int clx_maxpool_fwd(const float* x, float* y, int B, int D, int H, int W, int C,
                    int fz, int fy, int fx, clx_stream stream);
/* Gradient w.r.t. the PRE-activation of the tensor x that feeds both the
 * max-pool and the cropped skip connection:
 *   g[p][c]  = (x[p][c] is the first maximum of its window ? dy_pool[win][c] : 0)
 *            + (p inside the crop ? dskip[p - crop][c] : 0)
 *   dx[p][c] = g * (x[p][c] > 0)
 * dskip may be NULL. dskip has extent (SD, SH, SW), pixel stride ld_skip and
 * sits at offset (cz, cy, cx) inside x's grid. */
int clx_maxpool_bwd(const float* x, const float* y, const float* dy_pool,
                    const float* dskip, int ld_skip, int SD, int SH, int SW,
                    int cz, int cy, int cx, float* dx, int B, int D, int H,
                    int W, int C, int fz, int fy, int fx, clx_stream stream);
/* Backward of nearest upsample (+ crop) into the PRE-activation gradient of the
 * low-resolution tensor y (extent D,H,W; C channels):
 *   dy[q][c] = (sum over the f-block of dcat[(q*f + r) - o][coff + c]) * (y > 0)
 * dcat: gradient of the concatenated tensor, logical extent (LD, LH, LW),
 * pixel stride ld_cat, channel offset coff; o = crop offset. */
int clx_upsample_bwd(const float* dcat, int ld_cat, int coff, int LD, int LH,
                     int LW, int oz, int oy, int ox, const float* y, float* dy,
                     int B, int D, int H, int W, int C, int fz, int fy, int fx,
                     clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Embedding gather, OCE loss, Adam                                         */
/* ------------------------------------------------------------------------ */
/* sel[b][p][c] = offsets[b][c][coord...] + coord[b][p][c]
 * replaces UNetModel.select_and_add_coordinates (cellulus/models/unet.py:108-124).
 * offsets: planar (B, ND, [Z,] Y, X) f32; coords: (B, P, ND) int64, column 0
 * indexes the LAST spatial axis.  Index rules of the reference's advanced indexing: -n..-1
 * wrap around, anything else outside [0, n) is an IndexError there; here such a row is never
 * dereferenced, its selection is NaN and *oob_count (device int, zeroed by the caller, may be
 * NULL) counts it so that the host can raise.  Z must be 1 when ND == 2. */
int clx_gather_add_fwd(const float* offsets, const long long* coords, float* sel,
                       int B, int P, int ND, int Z, int Y, int X, int* oob_count,
                       clx_stream stream);
/* doffsets[b][c][coord] += dsel[b][p][c]  (float atomics; zero doffsets first); out-of-range
 * rows are skipped and counted as above.  As for the forward call, Z must be 1 when ND == 2. */
int clx_gather_add_bwd(const float* dsel, const long long* coords, float* doffsets,
                       int B, int P, int ND, int Z, int Y, int X, int* oob_count,
                       clx_stream stream);
/* OCE loss forward + gradient, replaces OCELoss.forward
 * (cellulus/criterions/oce_loss.py:45-63) and its autograd backward:
 *   d = |a - r|, oce = sum(1 - exp(-d^2/T)), reg = w * sum |a|
 *   da = (2/T) exp(-d^2/T) (a - r) + w a/|a|      (0 where the norm is 0)
 * a, r: (npairs, ND) f32. sums[0..2] += (loss, oce, reg) in f64 (zero first).
 * da may be NULL (forward only); grad_scale multiplies da. */
int clx_oce_loss_fwd_bwd(const float* a, const float* r, float* da, double* sums,
                         long long npairs, int ND, float temperature,
                         float reg_weight, float grad_scale, clx_stream stream);
/* Fused train-step tail: gather(anchor), gather(reference), OCE loss, and the
 * scatter-add of the anchor gradient straight into doffsets (planar, zeroed by
 * the caller). Equivalent to the three calls above composed as in
 * cellulus/train.py:170-178.  sums: FOUR doubles, zeroed by the caller: (loss, oce, reg) and
 * the number of pairs with an out-of-range coordinate (skipped, never dereferenced; the
 * reference raises IndexError there, so must the caller when sums[3] != 0).  A pair counts once, whether
 * one of its coordinates is out of range or both.  Z must be 1 when ND == 2. */
int clx_oce_pairs_fused(const float* offsets, const long long* anchor,
                        const long long* reference, float* doffsets, double* sums,
                        int B, int P, int ND, int Z, int Y, int X,
                        float temperature, float reg_weight, clx_stream stream);
/* The same with REPRODUCIBLE results: the scatter-add of the anchor gradients (every anchor pixel occurs
 * ~31 times) accumulates 2^-40 fixed-point integers — integer addition is associative, so the sum
 * does not depend on the order the atomics arrive in — and the loss sums are block partials reduced in
 * block order.  `sums` is ADDED to, as by clx_oce_pairs_fused; doffsets is overwritten.
 * scratch: clx_oce_pairs_det_scratch_bytes(B, ND, Z * Y * X), need not be zeroed. */
size_t clx_oce_pairs_det_scratch_bytes(int B, int ND, long long npix);
int clx_oce_pairs_fused_det(const float* offsets, const long long* anchor, const long long* reference,
                            float* doffsets, double* sums, int B, int P, int ND, int Z, int Y, int X,
                            float temperature, float reg_weight, void* scratch, clx_stream stream);

/* Optional on-device pair sampler with the distribution of ZarrDataset.sample_coordinates
 * (cellulus/datasets/zarr_dataset.py:177-242) — NOT its random stream: anchor column d uniform on
 * the integers [lo, hi[d]] (hi: HOST array of ND ints), each anchor repeated num_refs times,
 * reference = anchor + a uniformly chosen row of `offsets` (DEVICE, noffsets x ND int32: the
 * admissible offsets |o|^2 < kappa^2, o != 0).  anchor / reference: (B, num_anchors*num_refs, ND)
 * int64 out.  Counter-based: the same (seed, stream_id) gives the same pairs. */
int clx_sample_pairs(long long* anchor, long long* reference, const int* offsets, int noffsets,
                     int B, int num_anchors, int num_refs, int ND, int lo, const int* hi,
                     unsigned long long seed, unsigned long long stream_id, clx_stream stream);
/* torch.optim.Adam(lr, betas, eps, weight_decay) single step with coupled L2
 * (cellulus/train.py:80-82,179) over flat buffers of n floats.
 * step = 1-based step count AFTER increment. */
int clx_adam_step(float* param, const float* grad, float* exp_avg,
                  float* exp_avg_sq, long long n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step,
                  clx_stream stream);
/* The same step, enqueued BEFORE the host has read the loss kernel's bad-coordinate count: the kernel does
 * nothing when the device double *skip_if_positive is > 0 (NULL = unconditional).  cellulus/train.py:171-179
 * raises IndexError from the coordinate indexing before optimizer.step(); here the step is already in the
 * stream when the host looks, and is a no-op exactly in that case. */
int clx_adam_step_guarded(float* param, const float* grad, float* exp_avg,
                          float* exp_avg_sq, long long n, double lr, double beta1,
                          double beta2, double eps, double weight_decay, int step,
                          const double* skip_if_positive, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Inference statistics (cellulus/models/unet.py:90-98)                     */
/* ------------------------------------------------------------------------ */
/* preds: (T, C, n) planar predictions of T noisy forwards of one sample.
 * out: (C+1, n): out[c] = mean_t preds[t][c], out[C] = sum_c std_t (population
 * std, torch.std_mean(unbiased=False)). */
int clx_noise_stats(const float* preds, float* out, int T, int C, long long n,
                    clx_stream stream);
/* The same, ALSO keeping the running minimum and maximum of the std plane out[C] in std_minmax[0..1] (float32):
 * the range numpy.histogram needs for the Otsu threshold of that plane (cellulus/detect.py:88-91 ->
 * skimage.filters.threshold_otsu), so the fused predict -> detect path reads the plane once (histogram) instead
 * of twice.  init != 0 starts a new image; with init == 0 the call folds into what earlier calls (the other tiles
 * of the sample) left.  std_minmax: CLX_NOISE_MINMAX_FLOATS floats — the two results followed by scratch for the
 * per-block partials.  T <= 64. */
#define CLX_NOISE_MINMAX_FLOATS (2 + 2 * 1024)
int clx_noise_stats_minmax(const float* preds, float* out, int T, int C, long long n, float* std_minmax,
                           int init, clx_stream stream);

/* Salt / pepper noise of the infer-mode forward (cellulus/models/unet.py:75-88: `noisy[rnd <= p] = 0.5`, then 1.0):
 * rnd (T, n) uniform randoms, raw (n) the clean tile, out (T, n): out[t][i] = rnd[t][i] <= p ? (t < n_half ? 0.5 : 1.0)
 * : raw[i], the comparison in float32 as torch compares a float32 tensor with a Python scalar.  One launch in place
 * of torch's compare + where. */
int clx_noise_inject(const float* rnd, const float* raw, float* out, int T, int n_half, long long n, float p,
                     clx_stream stream);
/* Per-column minimum and maximum of a (n, width) float64 array, width 2 or 3: extent[0..width) = minima,
 * extent[width..2 width) = maxima — the bounding box the uniform grid of the mean-shift fit points is laid over
 * (sklearn builds a KD-tree there; cellulus/utils/mean_shift.py:62-74).  extent: CLX_ROWS_EXTENT_DOUBLES doubles (the
 * results + room for the block partials).  One launch up to 256 rows x 256, two above. */
#define CLX_ROWS_EXTENT_DOUBLES (6 * (1 + 256))
int clx_rows_extent_f64(const double* src, long long n, int width, double* extent, clx_stream stream);
/* Zero fills of `count` device buffers (16-byte aligned, sizes multiples of 4 bytes) in one launch per eight: the
 * accumulators a training step adds into (packed weight gradients, bias gradients, the scatter target of the loss). */
int clx_zero_many(void* const* buffers, const long long* nbytes, int count, clx_stream stream);
/* dst[i][:] = src[rows[i]][:] for float64 rows of `width` values: the random subsample MeanShift is fitted on
 * (cellulus/utils/mean_shift.py:69-70, `X[np.random.rand(len(X)) < p]`; the host draws the mask and sends the row
 * numbers, so the device-side size is known without a synchronising masked select). */
int clx_gather_rows_f64(const double* src, const int* rows, long long n, int width, double* dst, clx_stream stream);

/* The noisy copies of one tile (cellulus/models/unet.py:75-88: 2 * num_infer_iterations forwards of the same image
 * with salt / pepper noise in p_salt_pepper of its pixels) differ from the clean image only around those pixels.  Behind
 * the first k x k convolution the changed output pixels are the window-dilated set, and 1 x 1 layers keep it; a row of a
 * 1 x 1 layer depends on the same row of its input alone, so those layers are computed once on the clean image and
 * again on the CHANGED rows of each copy — the same bits as the dense computation.  The four calls below move the rows.
 *
 * clx_changed_rows: clean (C, ID, IH, IW) and noisy (T, C, ID, IH, IW), planar float32.  An output pixel of a
 * (KD, KH, KW) valid convolution of copy t is CHANGED if any input value in its window differs from the clean image's.
 * The copies are taken in chunks of `chunk`; chunk c's changed rows are written to rows[c * cap ...] as
 * (t - c * chunk) * npix_out + output pixel (any order), their number to counts[c] (which may exceed cap: rows beyond
 * cap are not written — the caller then takes the dense path).  counts: ceil(T / chunk) ints.
 * workspace: clx_changed_rows_workspace(T, ID, IH, IW) bytes of scratch (a bit per input pixel and per output row of
 * every copy), 8-byte aligned.  KW < 64. */
size_t clx_changed_rows_workspace(int T, int ID, int IH, int IW);
int clx_changed_rows(const float* clean, const float* noisy, int T, int C, int ID, int IH, int IW, int KD, int KH,
                     int KW, int chunk, int* rows, int* counts, long long cap, void* workspace, clx_stream stream);
/* After clx_changed_rows (same T, extents and window; 2-D: one output plane), from the row bits it left in `workspace`:
 * the output TILES (tile x tile) of a (WH, WW) valid convolution over those rows that see a changed row in their
 * (tile + WH - 1) x (tile + WW - 1) window — what clx_conv_desc.tile_list takes for the Winograd layer behind the 1 x 1
 * layers.  Chunk c's tiles go to tiles[c * cap ...] as ((t - c * chunk) * th + ty) * tw + tx (any order), their number to
 * counts[c] (may exceed cap; tiles beyond cap are not written).  tile + WW - 1 <= 64. */
int clx_changed_tiles(const void* workspace, int T, int ID, int IH, int IW, int KD, int KH, int KW, int WH, int WW,
                      int tile, int chunk, int* tiles, int* counts, long long cap, clx_stream stream);
/* The first layer of a ONE-channel image (3 x 3 or 3 x 3 x 3, valid; what clx_conv_fwd runs for c_real == 1) for a LIST of
 * output pixels: x planar (B, ID, IH, IW), rows[r] = b * (output pixels per image) + output pixel, wpack / bias as for
 * clx_conv_fwd of that layer; out[r][0..N) — the same fused multiply-adds in the same order as the dense kernel, so the
 * same bits (the changed rows of noisy copies never pass through a dense first-layer tensor). */
int clx_grey_rows(const float* x, int B, int ID, int IH, int IW, int KD, const int* rows, long long n, const float* wpack,
                  const float* bias, int relu, int N, float* out, int ld_out, clx_stream stream);
/* Data gradient of the first convolution with respect to the raw image: the input gradient of l_conv.0.conv_pass.0,
 * nn.Conv{2,3}d(in_channels -> num_fmaps, 3) with valid padding (cellulus/models/unet.py:24-51), which autograd leaves in
 * raw.grad there.  For 1-4 input channels and a 3x3 (KD = 1) or 3x3x3 (KD = 3) kernel:
 *   dx[b][c][z][y][x] = sum over kz < KD, ky < 3, kx < 3, n < N of w[n][c][kz][ky][kx] * dy[(b, z-kz, y-ky, x-kx)][n]
 * with the taps outside [0, OD) x [0, OH) x [0, OW) dropped; dx extent D = OD + KD - 1, H = OH + 2, W = OW + 2.
 * dy: pixel-major [B * OD * OH * OW][ld_dy] (16-byte aligned, ld_dy >= N, ld_dy % 4 == 0; lanes n >= N are not read);
 * w: the torch parameter (N, cin, KD, 3, 3) as it stands; dx: planar (B, cin, D, H, W), overwritten.  Float32 products and
 * sums whatever the precision switch; no atomics: the same inputs give the same bits. */
int clx_conv_first_dgrad(const float* dy, int ld_dy, const float* w, int N, int cin, int B, int OD, int OH, int OW, int KD,
                         float* dx, clx_stream stream);
/* dst[r][0..width) = src[rows[r]][0..width) for r < n (row strides ld_src / ld_dst floats; width, strides % 4 == 0,
 * 16-byte aligned bases). */
int clx_gather_rows(const float* src, int ld_src, const int* rows, long long n, int width, float* dst, int ld_dst,
                    clx_stream stream);
/* dst[rows[r]][0..width) = src[r][0..width) for r < n. */
int clx_scatter_rows(const float* src, int ld_src, const int* rows, long long n, int width, float* dst, int ld_dst,
                     clx_stream stream);
/* dst[k][0..nfloats) = src[0..nfloats) for k < copies (nfloats % 4 == 0, 16-byte aligned): the clean image's rows
 * under every copy, before clx_scatter_rows overwrites the changed ones. */
int clx_broadcast_rows(const float* src, long long nfloats, float* dst, int copies, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Mean-shift clustering (cellulus/utils/mean_shift.py:6-121 ->             */
/* sklearn.cluster.MeanShift.fit/predict), float64                          */
/* ------------------------------------------------------------------------ */
/* Adds pixel coordinates to the embedding IN PLACE (the reference mutates its
 * argument, mean_shift.py:15-32), builds the foreground mask std < threshold
 * and compacts foreground pixels in raster order:
 *   emb:  (ND, [Z,] Y, X) f64, channel 0 += x, 1 += y, 2 += z
 *   X:    (nfg, ND) f64 out,  index: (nfg) int32 raster index of each fg pixel
 *   nfg_out: device int32, number of foreground pixels
 * workspace: clx_ms_prepare_workspace(npix) bytes of scratch (16-byte aligned; no contents are expected; what the call
 * leaves — the foreground flags as one bit per pixel, the counts per tile and per chunk of tiles, the points in front of
 * every tile — is what clx_ms_assign_dense reads back).  Two launches: flags + counts from the std plane; the scatter
 * pass, which sums the counts in front of each tile itself.  index may be NULL (clx_ms_assign_dense does not need it). */
size_t clx_ms_prepare_workspace(long long npix);
int clx_ms_prepare(double* emb, const double* std, double threshold, int ND,
                   int Z, int Y, int X, double* Xout, int* index, int* nfg_out,
                   void* workspace, clx_stream stream);
/* The same compaction for the fused predict -> detect hand-off of infer() (cellulus/infer.py:69-73 without the
 * round trip through the float64 `embeddings` dataset, cellulus/predict.py:104-112 -> cellulus/detect.py:83): emb
 * and std are the network's float32 output, widened to float64 in registers — the values the staged path reads
 * back — so X and index are bit-identical to clx_ms_prepare's on the widened tensors.  emb is NOT modified (the
 * caller of this form discards the coordinate-added copy, as cellulus/detect.py:155-160 does).  Same workspace. */
int clx_ms_prepare_f32(const float* emb, const float* std, double threshold, int ND,
                       int Z, int Y, int X, double* Xout, int* index, int* nfg_out,
                       void* workspace, clx_stream stream);
/* Flat-kernel mean-shift of every seed over the fit points until
 * |shift| <= 1e-3*bandwidth or max_iter (sklearn _mean_shift_single_seed).
 * fit: (nfit, ND) f64; seeds: (nseeds, ND) f64; outputs centers (nseeds, ND)
 * f64, counts (nseeds) int32 = members within bandwidth of the final query,
 * iters (nseeds) int32. */
int clx_ms_iterate(const double* fit, int nfit, const double* seeds, int nseeds,
                   int ND, double bandwidth, int max_iter, double* centers,
                   int* counts, int* iters, clx_stream stream);
/* Same as clx_ms_iterate with the fit points bucketed in a uniform grid (for large
 * nfit): fit_sorted is sorted by cell id ((z*ny + y)*nx + x, cell coordinate =
 * floor((p - origin) / cell) per dim, cell >= bandwidth), cell_start (nx*ny*nz + 1)
 * holds each cell's first row.  `origin` is a HOST pointer to ND doubles.  A seed may lie
 * outside the grid, at any distance (beyond `bandwidth` of every point: count 0, centre = seed). */
int clx_ms_iterate_grid(const double* fit_sorted, int nfit, const int* cell_start,
                        const double* origin, double cell, int nx, int ny, int nz,
                        const double* seeds, int nseeds, int ND, double bandwidth,
                        int max_iter, double* centers, int* counts, int* iters,
                        clx_stream stream);
/* Bucketing for clx_ms_iterate_grid: counting sort of the fit points by uniform-grid cell
 * (cell id = x + nx * (y + ny * z), cell index = clamp(floor((p - origin) / cell))), the points of
 * one cell in their original order (what a stable sort by cell id gives).  fit_sorted: (n, ND) f64
 * out; cell_start: (nx*ny*nz + 1) int32 out; `origin` is a HOST pointer to ND doubles;
 * workspace: clx_ms_bucket_workspace(n, nx*ny*nz) bytes. */
size_t clx_ms_bucket_workspace(int n, long long ncells);
int clx_ms_bucket(const double* fit, int n, int ND, const double* origin, double cell, int nx,
                  int ny, int nz, double* fit_sorted, int* cell_start, void* workspace,
                  clx_stream stream);
/* A batch of random crops with the elastic augmentation from a data set held on the device: gunpowder's RandomLocation +
 * Normalize + ElasticAugment(control_point_spacing, jitter_sigma, rotation [0, pi/2], scale [0.9, 1.1]) as the
 * reference's datasets/zarr_dataset.py:84-131 chains them, with the arithmetic of ZarrDataset._random_crop /
 * _elastic_crop (the numpy / scipy restatement that runs in the loader processes).  The random numbers are drawn on the
 * host (ZarrDataset.elastic_params) and arrive in `params`; the deformation field, the placement, the resampling and
 * the maximum of every crop (the empty-crop rule) are computed here.
 * data: DEVICE (S, C, *spatial) contiguous, element type `dtype` (enum below); spatial, crop, cp_shape: HOST arrays of nd
 * ints (cp_shape, mats, workspace may be NULL when elastic = 0); factor: the float32 normalisation factor.
 * params: DEVICE float64, one record per crop —
 *   elastic:  [sample index, A = rot * scale (nd x nd, row-major), u_0..u_{nd-1} in [0, 1), nd control-point grids of
 *              prod(cp_shape) values each]                      (1 + nd * nd + nd + nd * prod(cp_shape) doubles)
 *   plain:    [sample index, offset_0..offset_{nd-1}]          (1 + nd doubles)
 * (sample indices and offsets outside the data set are clamped into it, never followed.)
 * mats: DEVICE float64, axis after axis the (crop_d x cp_shape_d) row-major matrix that up-samples a control-point grid
 * along axis d.  workspace: DEVICE, clx_elastic_crop_workspace(nd, crop, B) bytes, need not be initialised.
 * Per voxel, float64:  rel = A . (index - (crop - 1) / 2) + sum_ijk M_0[z][i] M_1[y][j] M_2[x][k] grid_d[i][j][k];
 * lo / hi = min / max of rel over the crop; room = spatial - 1 - (hi - lo); all room >= 0: mode `constant` (cval 0), else
 * scipy's `reflect`; coordinate = rel + u * max(room, 0) - lo; value = multilinear interpolation (float64 weights and sums)
 * of float32(data) * factor, rounded once to float32.  elastic = 0: raw = float32(data[window]) * factor, bit for bit.
 * raw: (B, C, *crop) float32 out, 16-byte aligned; maxima: B floats out, max(raw[b]).  Two launches (one when
 * elastic = 0) and one 4 * B byte fill on `stream`; no allocation, no float atomic adds: the same inputs give the same bits. */
enum clx_aug_dtype { CLX_AUG_U8 = 0, CLX_AUG_U16 = 1, CLX_AUG_F32 = 2 };
size_t clx_elastic_crop_workspace(int nd, const int* crop, int B);
int clx_elastic_crop(const void* data, int dtype, int S, int C, int nd, const int* spatial, const int* crop,
                     const int* cp_shape, float factor, int elastic, int B, const double* params, const double* mats,
                     void* workspace, float* raw, float* maxima, clx_stream stream);
/* HOST function: the offsets of the reference's pair sampler (cellulus/datasets/zarr_dataset.py:185-198,
 * sample_offsets_within_radius) drawn from numpy's LEGACY global generator — MT19937, 32-bit outputs, masked rejection,
 * i.e. what `np.random.randint(-radius, radius + 1, size = ND * number_offsets)` called ND times produces — filtered
 * (0 < |o|^2 < radius^2) and cut to number_offsets rows, redrawn like the reference when too few survive.  key[624],
 * *pos: the generator's state (np.random.get_state()[1:3]), advanced exactly as numpy would have; offsets:
 * (number_offsets, ND) int64 out; *rounds (may be NULL): how many times everything was drawn.  Same values, same
 * final state as the numpy form (tests/test_cpu_host.py), a fifth of its time. */
int clx_sample_offsets_mt19937(unsigned int* key, int* pos, int radius, int ND, long long number_offsets,
                               long long* offsets, int* rounds);
/* HOST function (host pointers, no stream): sklearn MeanShift.fit's post-processing of the converged seeds —
 * identical centre tuples collapse (the last count wins), sort by (count, centre) descending, greedy removal of every
 * centre within `bandwidth` (squared distance <= bandwidth^2) of a kept one
 * [cellulus/utils/mean_shift.py:62-74 -> sklearn/cluster/_mean_shift.py MeanShift.fit].  centers (n, ND) and counts (n)
 * are what clx_ms_iterate* produced, copied to the host; out: room for n centres; *n_out: the kept ones, in sklearn's
 * order (0 when no seed had a neighbour — sklearn raises there, and so does the Python caller). */
int clx_ms_dedup_centers(const double* centers, const int* counts, int n, int ND, double bandwidth,
                         double* out, int* n_out);
/* labels[index[i]] = 1 + argmin_k |X[i] - centers[k]|  (first minimum);
 * labels (npix) int32 must be zero-filled by the caller (background = 0). */
int clx_ms_assign(const double* X, const int* index, int nfg,
                  const double* centers, int ncenters, int ND, int* labels,
                  clx_stream stream);
/* The same result with the centres bucketed into a uniform grid (order: centre ids sorted by
 * cell, cell_start: (nx*ny*nz + 1) offsets into it, cell index = clamp(floor((c - origin) /
 * cell))): a pixel examines the 3^ND cells around it and falls back to all centres only when
 * no candidate is closer than `cell`.  `origin` is a HOST pointer to ND doubles. */
int clx_ms_assign_grid(const double* X, const int* index, int nfg, const double* centers,
                       int ncenters, int ND, const int* order, const int* cell_start,
                       const double* origin, double cell, int nx, int ny, int nz, int* labels,
                       clx_stream stream);
/* The grid search with the centres handed over IN CELL ORDER (centers_sorted[j] = centre order[j]; 16-byte aligned
 * in 2-D): a candidate is one load from a contiguous range instead of two dependent ones, the ranges of the
 * neighbouring rows are fetched together — the same labels (same arithmetic, same tie rule) in about half the time
 * (replaces the nearest-centre `predict` of sklearn MeanShift, cellulus/utils/mean_shift.py:93-104). */
int clx_ms_assign_cells(const double* X, const int* index, int nfg, const double* centers_sorted,
                        int ncenters, int ND, const int* order, const int* cell_start,
                        const double* origin, double cell, int nx, int ny, int nz, int* labels,
                        clx_stream stream);
/* The same assignment writing the WHOLE label map — every pixel once, in full lines, background as 0 — instead of
 * scattering one label per foreground pixel into a map the caller zeroed.  It reads the compaction's flag words and
 * per-tile point counts back from `prepare_workspace`: the workspace the clx_ms_prepare (prepared_from_f32 = 0) or
 * clx_ms_prepare_f32 (= 1) call that produced X for this (Z, Y, X) image left behind, untouched since (the ONE piece of
 * state between two calls of this library; the raster index is not read and may have been left out of that call).
 * labels: (Z, Y, X) int32, no initial contents expected.  Same labels as clx_ms_assign_cells + a zero fill
 * (cellulus/utils/mean_shift.py:93-104 with the `-1 -> 0` of :29-32). */
int clx_ms_assign_dense(const double* X, const double* centers_sorted, int ncenters, int ND, const int* order,
                        const int* cell_start, const double* origin, double cell, int nx, int ny, int nz,
                        const void* prepare_workspace, int prepared_from_f32, int Z, int Y, int Xdim, int* labels,
                        clx_stream stream);

/* Seeds for use_seeds = true (cellulus/detect.py:128-132), float64, the libraries' operation order:
 *   clx_offset_magnitude    np.linalg.norm(emb[:ND], axis=0): emb (ND, npix) -> out (npix)
 *   clx_gaussian_filter_f64 scipy.ndimage.gaussian_filter(in, sigma) with mode "reflect": `weights`
 *                           (DEVICE, radius + 1 doubles: centre first) are the normalised kernel scipy
 *                           builds (the caller computes them as scipy does); axes in scipy's order;
 *                           in / out / tmp: three distinct npix-buffers
 *   clx_negate_f64          out = -in
 *   clx_peak_local_max      skimage.feature.peak_local_max(img) defaults: pixels equal to the maximum
 *                           of their 3^ND neighbourhood, > min(img) (minmax[0], DEVICE, e.g. from
 *                           clx_minmax_f64), not on the image border; raster indices appended to
 *                           `peaks` in arrival order, *npeaks = how many (may exceed capacity:
 *                           only the first `capacity` are stored) */
int clx_offset_magnitude(const double* emb, double* out, int ND, long long npix, clx_stream stream);
int clx_gaussian_filter_f64(const double* in, double* out, double* tmp, int Z, int Y, int X,
                            const double* weights, int radius, clx_stream stream);
int clx_negate_f64(const double* in, double* out, long long n, clx_stream stream);
int clx_peak_local_max(const double* img, int Z, int Y, int X, const double* minmax, int* peaks,
                       int capacity, int* npeaks, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Greedy clustering (cellulus/utils/greedy_cluster.py:46-120,176-253)      */
/* ------------------------------------------------------------------------ */
/* emb: (ND, n) embeddings + coordinates of the n foreground pixels (raster order);
 * seedmap: (n) normalised seediness; both float32 (is_f64 = 0, the reference's 2-D
 * class) or float64 (is_f64 = 1, its 3-D class).  Runs the reference's whole
 * seed loop on the device: pick the unclustered pixel of highest seediness (stop
 * below seed_thresh), propose exp(-|e - c|^2 / (2 bw^2)) > 0.5, accept the
 * proposal as instance `count` if it has more than min_object_size pixels of
 * which more than half were unclustered, clear it, repeat while more than
 * min_unclustered_sum pixels remain.  instance: (n) int32 ids (0 = none);
 * result[0] = instances, result[1] = seeds tried.  workspace: 2*(n+16) bytes. */
int clx_greedy_cluster(const void* emb, const void* seedmap, int n, int ND, int is_f64,
                       double bandwidth, int min_object_size, double seed_thresh,
                       int min_unclustered_sum, void* workspace, int* instance, int* result,
                       clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Connected components + size filter (cellulus/utils/misc.py:11-25 ->      */
/* skimage.measure.label, full connectivity, background 0)                  */
/* ------------------------------------------------------------------------ */
size_t clx_cc_workspace(long long npix);
/* out[p] = raster-order component id (1..ncomp) of the maximal equal-value
 * 8-/26-connected region containing p, 0 for seg[p]==0. Components with fewer
 * than min_size pixels are removed first (min_size <= 0: keep all — and, as in
 * the reference, min_size == 0 means "return seg unchanged": the caller
 * handles that case). ncomp_out: device int32. */
int clx_cc_label_filter(const int* seg, int* out, int Z, int Y, int X,
                        int min_size, int* ncomp_out, void* workspace,
                        clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Exact squared Euclidean distance transform (scipy distance_transform_edt */
/* as used by cellulus/segment.py:41-51)                                    */
/* ------------------------------------------------------------------------ */
size_t clx_edt_workspace(long long npix);
/* out[p] = min over q with in[q]==0 of |p-q|^2 (int32).  cap > 0 limits every
 * axis search to `cap` steps: values < cap^2 are exact, larger ones are only
 * guaranteed to be >= cap^2 (enough for "distance < cap" tests); cap <= 0 is the
 * full transform.  An image without any zero reproduces scipy's phantom zero at
 * index -1 of the first axis. */
int clx_edt_sq(const unsigned char* in, int* out, int Z, int Y, int X, int cap,
               void* workspace, clx_stream stream);
/* segment "cell" post-processing in one call (segment.py:41-51):
 *   d1 = edt(seg==0); grown = d1 < grow; d2 = edt(grown); seg[d2 < shrink] = 0 */
int clx_grow_shrink(int* seg, int Z, int Y, int X, int grow, int shrink,
                    void* workspace /* 2*clx_edt_workspace(npix) + npix bytes */,
                    clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Otsu histogram (skimage.filters.threshold_otsu, cellulus/detect.py:88-91) */
/* ------------------------------------------------------------------------ */
/* minmax[0..1] = min, max of x (f64, n elements).  minmax: CLX_MINMAX_DOUBLES doubles — the two results followed by
 * scratch for the per-block partials (no two blocks meet on an address: same-address float64 atomics are served one after
 * the other at the memory side, which made the kernel's time proportional to its grid). */
#define CLX_MINMAX_DOUBLES (2 + 2 * 512)
int clx_minmax_f64(const double* x, long long n, double* minmax, clx_stream stream);
/* numpy.histogram(x, bins=nbins, range=(edges[0], edges[nbins])) with the
 * caller-supplied edges (np.linspace) — counts (nbins) int64, zeroed by caller. */
int clx_histogram_f64(const double* x, long long n, const double* edges,
                      int nbins, long long* counts, clx_stream stream);
/* The same two primitives for a float32 image whose values are to be read as float64 (the network's std plane handed
 * over in device memory; the staged path reads exactly these values widened from the `embeddings` dataset):
 * minmax and counts are bit-identical to the float64 entry points on the widened image. */
int clx_minmax_f32(const float* x, long long n, double* minmax, clx_stream stream);
int clx_histogram_f32(const float* x, long long n, const double* edges, int nbins,
                      long long* counts, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "nucleus" post-processing (cellulus/segment.py:52-101): per-instance Otsu */
/* of the raw intensities + scipy.ndimage.binary_fill_holes in the bbox      */
/* ------------------------------------------------------------------------ */
typedef enum { CLX_RAW_F32 = 0, CLX_RAW_F64 = 1, CLX_RAW_I32 = 2 } clx_raw_type;
/* For every id in [1, nid): bbox[id] = {zmin,ymin,xmin,zmax,ymax,xmax} (max < 0:
 * id absent) and vkey[id] = {min,max} of raw over seg==id as order-preserving
 * keys (f32: u32 bits, sign-flipped, in the low word; f64: same on 64 bits;
 * i32: v ^ 0x80000000).  Replaces np.unique/np.where/min/max, segment.py:58-79. */
int clx_inst_stats(const int32_t* seg, const void* raw, int raw_type, int Z, int Y,
                   int X, int nid, int32_t* bbox, unsigned long long* vkey,
                   clx_stream stream);
/* All instance histograms of skimage.filters.threshold_otsu(raw[seg==id])
 * (segment.py:80-81) in one pass.  slot[id] = row of `counts` (or -1: skip).
 * Float raw: edges_or_min = [rows][nbins+1] np.linspace edges in the raw dtype,
 * numpy.histogram's index arithmetic is followed in that dtype.  Integer raw:
 * edges_or_min = int32[rows] minimum per row, one bin per value.
 * counts: u32 [rows][nbins], zeroed by the caller. */
int clx_inst_histogram(const int32_t* seg, const void* raw, int raw_type,
                       long long npix, const int32_t* slot, int nid,
                       const void* edges_or_min, int nbins, uint32_t* counts,
                       clx_stream stream);
/* For instance k (id ids[k], ascending): mask = (seg==id) & (raw > thr[k]);
 * binary_fill_holes inside bbox[id] (face connectivity, background connected to
 * the box border stays background; ndim 2 or 3 says whether the z faces of the
 * box are borders); out[p] = max(out[p], id) on the filled mask — `out` zeroed
 * by the caller (segment.py:82-101).  scratch: one byte per bounding-box voxel,
 * instance k at scratch_off[k]. */
int clx_inst_refine(const int32_t* seg, const void* raw, int raw_type, int ndim,
                    int Z, int Y, int X, const int32_t* ids, const int32_t* bbox,
                    const double* thr, const long long* scratch_off,
                    unsigned char* scratch, int n, int32_t* out, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* evaluation (cellulus/evaluate.py:72-100): compute_pairwise_IoU's          */
/* #pred x #gt full-image mask passes as ONE joint histogram of id pairs     */
/* ------------------------------------------------------------------------ */
/* present[id] = 1 for every id in `labels` (np.unique, evaluate.py:73-76);
 * *bad = 1 if an id lies outside [0, nid).  present / bad zeroed by the caller. */
int clx_label_presence(const int32_t* labels, long long n, int nid,
                       int32_t* present, int32_t* bad, clx_stream stream);
/* joint[pred_row[pred[i]]][gt_col[gt[i]]] += 1 for all i: intersections
 * (evaluate.py:84-86) directly, object sizes and unions (:87-94) from its row /
 * column sums.  pred_row / gt_col: id -> row / column tables (every id present in
 * the maps must have an entry); joint: u64 [rows][ncol], zeroed by the caller. */
int clx_joint_histogram(const int32_t* pred, const int32_t* gt, long long n,
                        const int32_t* pred_row, const int32_t* gt_col, int ncol,
                        unsigned long long* joint, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* measure stage: the per-object table of skimage.measure.regionprops (area, */
/* bbox, centroid, second moments, mean / min / max intensity) as integer    */
/* sums taken in one pass over the label map — no host copy of the map       */
/* ------------------------------------------------------------------------ */
/* Geometry of every id in [1, nid) of a label map [Z][Y][X] (2-D: Z = 1); replaces the coordinate lists behind
 * regionprops' area / bbox / centroid / inertia_tensor.  The entry point initialises ALL outputs itself (nothing
 * depends on what the buffers held); row 0 (background) of every output is unspecified.
 *   area [nid]     pixel count (0: id absent)
 *   bbox [nid][6]  zmin,ymin,xmin,zmax,ymax,xmax, inclusive; max < 0: id absent (clx_inst_stats' convention)
 *   sum1 [nid][3]  Σz, Σy, Σx          sum2 [nid][6]  Σzz, Σyy, Σxx, Σzy, Σzx, Σyx
 *   bad  [1]       1: a label outside [0, nid) — never followed as an index, that pixel is skipped
 * Integer accumulators only: the same map gives the same bits in every run.  Refused (CLX_ERR_ARG) before any launch:
 * null pointers, nid outside [1, 2^24], Z*Y*X >= 2^32, (max(Z,Y,X) - 1)^2 * Z*Y*X >= 2^63 (the second moments would
 * not fit in 64 bits). */
int clx_region_moments(const int32_t* labels, int Z, int Y, int X, int nid,
                       unsigned long long* area, int32_t* bbox, unsigned long long* sum1,
                       unsigned long long* sum2, int32_t* bad, clx_stream stream);
/* One raw channel (npix values of `raw_type`) over the same labels; replaces regionprops' mean / min / max_intensity.
 * Outputs are initialised by the entry point, row 0 is unspecified.
 *   isum [nid]     Σ q over the id's pixels.  CLX_RAW_I32: q = v, exact, `shift` ignored.  CLX_RAW_F32 / _F64:
 *                  q = (long long) rint(ldexp((double) v, shift)); the caller picks `shift` so that the sum fits
 *                  (cellulus_amd.measure.intensity_shift) and divides Σ q by 2^shift
 *   vkey [nid][2]  min, max as clx_inst_stats' order-preserving keys ({~0, 0}: id absent)
 *   bad  [1]       bit 0: a label outside [0, nid); bit 1: a value under an object id that is NaN, ±Inf or has
 *                  |q| > 2^62 >> bit_length(npix) (a wrong `shift` cannot overflow silently).  Such pixels are skipped.
 * Refused before any launch: null pointers, unknown raw_type, nid outside [1, 2^24], npix outside [1, 2^32). */
int clx_region_intensity(const int32_t* labels, const void* raw, int raw_type, long long npix,
                         int nid, int shift, long long* isum, unsigned long long* vkey,
                         int32_t* bad, clx_stream stream);
/* Contacts: the faces between pixels of different ids, per id pair — the region adjacency / cell-contact graph, the
 * boundary size of every object and its contact with the image edge, which no moment gives.  Label map [Z][Y][X].
 *   face      between two pixels that are neighbours along one counted axis (connectivity 1): y and x for nd == 2
 *             (Z must be 1), z, y and x for nd == 3 (Z == 1 allowed: its two z faces per pixel then go to id 0)
 *   outside   the outside of the image is id 0 on both ends of every counted axis: a pixel in the first or last row,
 *             column (or slice) has a face to id 0
 *   pair      every face whose two ids differ counts once for (lo, hi), lo < hi; lo may be 0 (background or outside)
 *   labels    a label outside [0, nid) is treated as 0, is never followed as an index and sets bit 0 of info[0]
 * Output: an open-addressing table of `capacity` slots (a power of two in [1024, 2^28]).
 *   keys   [capacity]  (lo << 32) | hi; 0: empty slot (hi >= 1, so no key is 0)
 *   counts [capacity]  faces of that pair
 *   info   [2]         [0] bit 0: a label outside [0, nid); bit 2: a pair could not be placed — the table is to be
 *                      discarded and the call repeated with a larger capacity.  [1] occupied slots (<= capacity)
 * The entry point initialises keys, counts and info itself.  Which slot a pair gets depends on which block claims first,
 * so the slot order is unspecified; the SET of (key, count) is determined by the map: integer adds only.  Either the
 * set is exact or bit 2 is set, nothing in between.  An insertion probes at most min(capacity, 4096) consecutive slots
 * (modulo capacity) and then gives up with bit 2: it never spins, always terminates and writes only keys[0, capacity)
 * and counts[0, capacity).  With a table a few times larger than the number of pairs bit 2 means "more pairs than
 * slots" in practice, but a caller must not rely on that: repeat while it is set.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent,
 * Z*Y*X >= 2^32, nid outside [1, 2^24], capacity not a power of two in [1024, 2^28]. */
int clx_region_contacts(const int32_t* labels, int nd, int Z, int Y, int X, int nid, int capacity,
                        unsigned long long* keys, unsigned long long* counts, int32_t* info,
                        clx_stream stream);
/* Perimeter, 2-D label map [Y][X]: scikit-image's perimeter(mask, neighbourhood=4) of every object's mask, restated on
 * the full map (the formula is restated here, not compared with scikit-image by a fixture).  The outside of the image,
 * the background and other objects all count as "not the object".
 *   border pixel of i   a pixel of i with a 4-neighbour that is not i
 *   code                1 + 2 n4 + 10 nd; n4 / nd: the border pixels of i among its 4 edge / 4 diagonal neighbours
 *   classes [nid][4]    [0] border pixels; [1] codes 5 7 15 17 25 27 (weight 1); [2] codes 21 33 (weight sqrt 2);
 *                       [3] codes 13 23 (weight (1 + sqrt 2) / 2).  perimeter = c1 + c2 sqrt 2 + c3 (1 + sqrt 2) / 2, formed
 *                       by the caller; a one-pixel object has code 1 and perimeter 0
 *   bad [1]             1: a label outside [0, nid) — never followed as an index, treated as background
 * Outputs are initialised by the entry point; row 0 is unspecified.  Integer adds only: the same bits in every run.
 * Refused before any launch: null pointers, a non-positive extent, nid outside [1, 2^24], Y*X >= 2^32. */
int clx_region_perimeter(const int32_t* labels, int Y, int X, int nid, unsigned long long* classes,
                         int32_t* bad, clx_stream stream);
/* Topology: per object the sums over all 2 x 2 (nd == 2) / 2 x 2 x 2 (nd == 3) windows of the label map [Z][Y][X], from
 * which the caller forms the Euler numbers, the Crofton perimeter (2-D) and the surface area (3-D) of every object
 * (cellulus_amd.measure.topology_columns).  The map is padded with id 0 on both ends of every counted axis: y and x for
 * nd == 2 (Z must be 1), z, y and x for nd == 3 (Z == 1 allowed).
 *   window    the 2^nd voxels of the padded map around one lattice vertex: (Y+1)(X+1) resp. (Z+1)(Y+1)(X+1) of them
 *   bits      for an id i > 0: bit b_v = [voxel v of the window == i]; other objects, background and outside are "not i".
 *             A window with no bit or with every bit set adds nothing to i
 *   d-cell    through the vertex: a choice of d of the nd axes and a side along each (C(nd,d) 2^d of them); its voxels
 *             are the 2^(nd-d) window voxels on the chosen sides
 *   counts [nid][5], summed over all windows:
 *     [0] T1    voxel pairs of the window that differ in exactly one coordinate and have different bits
 *     [1] T2    the same for pairs that differ in exactly two coordinates
 *     [2] T3    the same for pairs that differ in three coordinates (0 for nd == 2)
 *     [3] E_hi  sum over d of (-1)^d 2^(nd-d) #{d-cells that touch at least one set voxel}
 *     [4] E_lo  sum over d of (-1)^(nd-d) 2^(nd-d) #{d-cells all of whose voxels are set}
 *   so that T1 = 2^(nd-1) (faces between i and not-i), T2 = 2^(nd-2) (face-diagonal neighbour pairs i / not-i), T3 = space-
 *   diagonal pairs, E_hi = 2^nd (Euler number under 8- / 26-connectivity), E_lo = 2^nd (Euler number under 4- / 6-
 *   connectivity); in 2-D E_hi / E_lo = Q1 - Q3 -/+ 2 QD, Gray's bit quads.  E_hi and E_lo may be negative.
 *   bad [1]   1: a label outside [0, nid) -- never followed as an index, treated as 0
 * Outputs are initialised by the entry point; row 0 is unspecified.  Integer adds only: the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent,
 * Z*Y*X >= 2^32, nid outside [1, 2^24]. */
int clx_region_topology(const int32_t* labels, int nd, int Z, int Y, int X, int nid,
                        long long* counts, int32_t* bad, clx_stream stream);
/* Convex hull: per object the integers behind area_convex, solidity and the maximum / minimum Feret diameter
 * (cellulus_amd.measure.hull_columns forms the columns).  Label map [Z][Y][X]; nd == 2 needs Z == 1.
 * Definitions -- NOT scikit-image's, which counts the pixels of the rasterised convex_hull_image and takes the Feret
 * diameter from a contour; no fixture compares with it:
 *   object    the union of its pixels as closed unit squares (3-D: unit cubes): pixel (y, x) has the corners
 *             (y .. y+1, x .. x+1), and the hull of the object is the hull of its pixels' corner lattice points.  Everything
 *             stays an integer and solidity = area / area_convex <= 1.  One pixel: area_convex 1, Feret max sqrt 2, min 1
 *   hull [nid][5], nd == 2:
 *     [0] A2  twice the area of the hull polygon (shoelace formula)
 *     [1] NV  its strict vertices (no collinear point counts)
 *     [2] F2  the largest squared distance between two vertices: feret_diameter_max = sqrt(F2)
 *     [3] C, [4] L2  the minimum caliper width as an exact rational, C / sqrt(L2): for every hull edge e = b - a,
 *             c_e = max over the vertices v of |cross(e, v - a)| and l_e = |e|^2; the edge with the smallest c_e^2 / l_e
 *             is reported (compared exactly, c_a^2 l_b against c_b^2 l_a as 128-bit products), ties towards the smaller l_e
 *   hull [nid][5], nd == 3: F2 only, the largest squared distance between two corner points of the object's voxels;
 *             A2 = NV = C = L2 = 0.  Convex volume and solidity in 3-D are not computed.
 *   bbox      [nid][6] clx_region_moments' output, left on the device
 *   row_base  [nid] exclusive prefix sum over the ids of (zmax - zmin + 1) (ymax - ymin + 1), 0 rows for an absent id; `rows`
 *             is the total.  Row (z, y) of object i is row_base[i] + (z - zmin) (ymax - ymin + 1) + (y - ymin)
 *   workspace at least clx_region_hull_workspace(rows) bytes (a host-only function; 0: rows out of range), 8-byte aligned
 *   bad [1]   bit 0: a label outside [0, nid) -- never followed as an index, treated as background
 *             bit 1: a pixel that the bbox / row_base of its id does not contain (a stale or wrong box); it is skipped.
 *             Boxes and row_base are checked against the image and `rows` before use: no index outside the workspace
 *             is ever formed, whatever they hold; an id whose box fails that check gets a row of zeros
 * The entry point initialises hull, bad and the workspace itself.  Row 0 and the rows of absent ids are zero.  Integer
 * operations only: the same map gives the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent, an
 * extent >= 2^30, Z*Y*X >= 2^32, nid outside [1, 2^24], nd == 2 with (Y+1)(X+1) > 2^31 (C^2 must fit 64 bits), rows outside
 * [0, (nid - 1) Z Y], workspace_bytes below clx_region_hull_workspace(rows), a workspace that is not 8-byte aligned. */
size_t clx_region_hull_workspace(long long rows);
int clx_region_hull(const int32_t* labels, int nd, int Z, int Y, int X, int nid, const int32_t* bbox,
                    const long long* row_base, long long rows, void* workspace, size_t workspace_bytes,
                    long long* hull, int32_t* bad, clx_stream stream);
/* Label-aware distance map: for every object pixel the squared distance to the nearest pixel that carries ANOTHER value,
 * another object or the background alike -- what distance_transform_edt(labels == i) gives inside object i, for every i in
 * one call.  (clx_edt_sq is binary: in a tissue whose objects touch it measures the distance to the background instead.)
 * Label map [Z][Y][X] of int32; nd == 2 needs Z == 1.
 *   labels    0 is background, every other value (a negative one too) an object.  Values are only compared with each
 *             other, never followed as an index
 *   d2(p)     for labels[p] != 0: the smallest |p - q|^2 over the pixels q with labels[q] != labels[p], between pixel centres
 *             at unit spacing; 0 for labels[p] == 0
 *   edge      0: only pixels of the map are candidates (scipy's convention).  1: the map counts as padded with one layer of
 *             0 on both ends of every counted axis: y and x for nd == 2, z, y and x for nd == 3 (Z == 1 allowed: every object
 *             pixel is then at distance 1 from the padding)
 *   CLX_DIST_INF  the value of a pixel without any candidate: only with edge == 0, on a map that carries one non-zero value
 *             everywhere.  Every other distance is below it
 *   dist_sq   [Z][Y][X] int32, every element is written
 *   workspace at least clx_label_distance_workspace(Z*Y*X) bytes (a host-only function; 0: npix outside [1, 2^32)), 4-byte
 *             aligned: one more map, the other side of the passes' ping-pong
 * Separable and exact: a pass along x, then min-plus passes along y (and z) in which a pixel of another value counts as
 * distance 0 and a pixel of the same value with what the pass before left there.  Integers only: the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent, edge not
 * 0 or 1, Z*Y*X >= 2^32, (Z-1)^2 + (Y-1)^2 + (X-1)^2 >= 2^30 (a finite distance must stay below CLX_DIST_INF),
 * workspace_bytes below clx_label_distance_workspace(Z*Y*X), a workspace that is not 4-byte aligned. */
#define CLX_DIST_INF (1 << 30)
size_t clx_label_distance_workspace(long long npix);
int clx_label_distance_sq(const int32_t* labels, int nd, int Z, int Y, int X, int edge, int32_t* dist_sq,
                          void* workspace, size_t workspace_bytes, clx_stream stream);
/* Largest inscribed circle / ball: per id the maximum of a distance map over the id's pixels, where it is attained, and
 * the map's sum (cellulus_amd.measure.inscribed_columns forms the columns).  labels and dist_sq: npix values each.
 *   out [nid][3]  [0] D2   the largest dist_sq over the id's pixels: inscribed radius = sqrt(D2)
 *                 [1]      the smallest linear index (z Y + y) X + x among the pixels that attain it
 *                 [2]      the sum of dist_sq over the id's pixels (at most 2^32 2^30)
 *   bad [1]       bit 0: a label outside [0, nid) -- never followed as an index, that pixel is skipped
 *                 bit 1: a dist_sq outside [0, CLX_DIST_INF] under an id in [1, nid); that pixel is skipped
 * The entry point initialises out and bad itself.  Row 0 and the rows of absent ids are zero.  Integer maxima and adds
 * only: the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nid outside [1, 2^24], npix outside [1, 2^32). */
int clx_region_inscribed(const int32_t* labels, const int32_t* dist_sq, long long npix, int nid,
                         unsigned long long* out, int32_t* bad, clx_stream stream);
/* Order statistics: per id the keys of given ranks among the keys of the id's pixels in one raw channel -- what np.quantile /
 * np.median over an object's pixels sort for, for every object in one call (cellulus_amd.measure.quantile_columns forms the
 * columns).  labels and raw: npix values each.  A key is the order-preserving 64-bit key of clx_inst_stats /
 * clx_region_intensity; for CLX_RAW_F32 and CLX_RAW_I32 it lies in the low 32 bits.
 *   area      [nid] clx_region_moments' output, left on the device
 *   seg_base  [nid] exclusive prefix sum of area over the ids 1 .., an absent id taking 0 pixels; `total` is the sum.  The
 *             keys of object i are gathered in positions [seg_base[i], seg_base[i] + area[i]) of a buffer in the workspace
 *   centre    NULL: the key of a pixel is that of its value, in the raw type.  [nid] float64: the key is that of
 *             fabs((double) v - centre[id]), one IEEE subtraction in float64, and decodes as float64 whatever raw_type is
 *             (the median absolute deviation: centre = the medians of a first call)
 *   rank      [nid][nq] 0-based ranks, 0 the smallest key
 *   out       [nid][nq] the key of that rank among the id's keys.  An order statistic is one of the values: exact, the
 *             same bits in every run although the order inside a segment is not.  ~0 in every column of an absent id
 *   workspace at least clx_region_order_workspace(total, nid) bytes (a host-only function; 0: an argument out of range),
 *             8-byte aligned: the key buffer, a cursor per id, and the histograms of the segments too long for one block
 *   bad [1]   bit 0: a label outside [0, nid) -- never followed as an index, that pixel is skipped
 *             bit 1: a NaN or +-Inf under an id in [1, nid).  Its key is still written, so the segment stays full; that
 *                    object's row is unspecified, every other row is right.  Non-finite values on background are ignored
 *             bit 2: the map disagrees with area / seg_base: a cursor went past area[id] (that key is dropped: nothing is
 *                    ever written outside the segment) or ended below it (the row is unspecified), or a segment does not
 *                    lie inside [0, total) (nothing of it is read or written, the row stays ~0)
 *             bit 3: a rank >= area[id] for a present id; that element is ~0, nothing out of bounds is read
 * The entry point initialises out, bad and the workspace itself; row 0 is unspecified.  The number of launches does not
 * depend on the number of objects or ranks.
 * Refused (CLX_ERR_ARG) before any launch, the outputs untouched: null pointers (centre may be null), an unknown raw_type,
 * nid outside [1, 2^24], npix outside [1, 2^32), nq outside [1, 32], total outside [0, npix], workspace_bytes below
 * clx_region_order_workspace(total, nid), a workspace that is not 8-byte aligned.  total == 0 launches the initialisation
 * only. */
size_t clx_region_order_workspace(long long total, int nid);
int clx_region_order_stats(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid,
                           const unsigned long long* area, const unsigned long long* seg_base, long long total,
                           const double* centre, const unsigned long long* rank, int nq, unsigned long long* out,
                           void* workspace, size_t workspace_bytes, int32_t* bad, clx_stream stream);
/* One phase of clx_region_order_stats alone, for timing (tools/bench_order_stats.py): the same arguments and refusals;
 * phase 1 initialises the outputs and gathers the keys, phase 2 selects from a workspace that phase 1 has filled with the
 * same arguments and leaves bad as it is.  Any other phase is refused. */
int clx_region_order_phase(const int32_t* labels, const void* raw, int raw_type, long long npix, int nid,
                           const unsigned long long* area, const unsigned long long* seg_base, long long total,
                           const double* centre, const unsigned long long* rank, int nq, unsigned long long* out,
                           void* workspace, size_t workspace_bytes, int32_t* bad, int phase, clx_stream stream);
/* Texture: per object the grey-level co-occurrence matrices of one raw channel, from which the caller forms Haralick's
 * features (cellulus_amd.measure.texture_columns).  Label map and raw [Z][Y][X]; nd == 2 needs Z == 1.
 *   level(v)    min(levels - 1, max(0, (int) floor(((double) v - lo) / (hi - lo) * levels))): IEEE float64 in that order
 *               of operations (the floor is clamped as a double, so no cast is out of range; a NaN quotient, which only
 *               an infinite hi - lo gives, is level 0).  hi == lo: every pixel is at level 0.  Values outside [lo, hi]
 *               clamp to level 0 / levels - 1
 *   direction k the k-th offset of {-1, 0, 1}^nd that is lexicographically greater than zero, ascending: (dy, dx) = (0,1),
 *               (1,-1), (1,0), (1,1) for nd == 2 (ndir = 4); 13 for nd == 3, (0,0,1) first, (1,1,1) last.  Each is multiplied
 *               by `distance`
 *   counts [nrows][ndir][levels][levels] int32.  counts[r][k][a][b]: the pixels p of id ids[r] at level a whose partner
 *               q = p + distance * offset_k lies inside the map (no wrap across row, slice or map ends), carries the same id
 *               and is at level b.  Ordered pairs, not symmetrised.  A partner in another object, on background or outside
 *               the map gives no pair
 *   ids [nrows] the objects this call takes, any order.  An id outside [1, nid), an absent id, and an id whose box fails the
 *               check below get a row of zeros and seen 0.  Rows are independent of each other: an id that appears twice
 *               gets two equal rows
 *   bbox        [nid][6] clx_region_moments' output, left on the device.  A box is checked against the map before use
 *               (0 <= min <= max < extent on every axis), so no index outside labels, raw or counts is ever formed whatever
 *               bbox and ids hold; only pixels p inside the box of their id are visited (their partners q may lie outside it)
 *   seen [nrows] the pixels of ids[r] that the call visited: equal to the id's area unless the box is stale
 *   bad [1]     over the WHOLE map, whatever ids holds: bit 0 a label outside [0, nid) -- never followed as an index, it
 *               matches no id; bit 1 a NaN or +-Inf under a label in [1, nid): that pixel takes part in no pair, neither
 *               as p nor as q.  Non-finite values on background are ignored
 *   workspace   at least clx_region_cooccurrence_workspace(Z*Y*X, nrows) bytes (a host-only function; 0: an argument out of
 *               range), 8-byte aligned: the list of work items (below) and the levels staged as one byte per pixel
 * Three kernels ahead of the main one: a pass over the map stages the levels (one float64 division per object pixel, not
 * one per pair) and sets bad; one block turns the boxes of ids into the exclusive prefix sum of their slab counts -- a slab
 * is a run of box rows (z, y) of about 8192 pixels, so an object that fills the map is cut into thousands of work items and a
 * small one is a single item; the third zeroes seen and the rows that more than one item adds into.  The main kernel's
 * blocks take the items in turn (the grid does not grow with nrows), find the row by bisection, keep the ndir x levels^2
 * matrices in LDS (at most 13 x 32 x 32 x 4 = 52 KiB) and write them out once: plain stores for a single-item object, atomic
 * adds for a shared one.  p owns its pair whichever slab q lies in.
 * The entry point initialises counts, seen, bad and the workspace itself.  Integer adds only: the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch, the outputs untouched: null pointers, an unknown raw_type, nd not 2 or 3, nd == 2
 * with Z != 1, a non-positive extent, Z*Y*X >= 2^31 (counts are int32), nid outside [1, 2^24], nrows outside [0, nid),
 * levels outside [2, 32], distance outside [1, 64], lo or hi not finite, hi < lo, a byte size of counts that does not fit
 * size_t (with a 64-bit size_t the bounds above already exclude it), workspace_bytes below
 * clx_region_cooccurrence_workspace(Z*Y*X, nrows), a workspace that is not 8-byte aligned. */
size_t clx_region_cooccurrence_workspace(long long npix, int nrows);
int clx_region_cooccurrence(const int32_t* labels, const void* raw, int raw_type, int nd, int Z, int Y, int X, int nid,
                            const int32_t* bbox, const int32_t* ids, int nrows, double lo, double hi, int levels,
                            int distance, int32_t* counts, long long* seen, int32_t* bad, void* workspace,
                            size_t workspace_bytes, clx_stream stream);
/* Radial distribution: per object, ring and angular wedge the pixel count and the sum of one raw channel -- where inside the
 * object the signal sits: rim against core (a membrane against a cytoplasm, a translocation), one side against the other (a
 * polarity); cellulus_amd.measure.radial_columns forms the columns (CellProfiler's FracAtD, MeanFrac, RadialCV).  Label map,
 * dist_sq and raw [Z][Y][X]; nd == 2 needs Z == 1.  The definitions are the project's own:
 *   d2(p)     dist_sq[p], clx_label_distance_sq's map of the same labels
 *   D2(i)     inscribed[i][0];  c(i): the pixel with linear index inscribed[i][1]  (clx_region_inscribed's out [nid][3], left on
 *             the device)
 *   ring      relative mode (width == 0): for a pixel of object i the smallest k in [0, rings) with
 *             d2 * rings^2 <= (k + 1)^2 * D2: ceil(rings * sqrt(d2 / D2)) - 1 decided in 64-bit integers (the products reach
 *             2^40), with no square root and no floating point; a pixel exactly on a ring's edge lies in the ring the inequality
 *             gives.  Ring 0 is the RIM, next to the boundary; ring rings - 1 the CORE, which holds c(i).
 *             absolute mode (width in [1, 32768]): the smallest k with d2 <= ((k + 1) * width)^2, clamped to rings - 1: bands
 *             of `width` pixels counted from the boundary, the last ring taking everything deeper
 *   wedge     wedges == 1: always 0.  wedges == 8 (nd == 2 only): (dy, dx) = p - c(i), theta = atan2(dy, dx) in [0, 2 pi); wedge
 *             o holds o * 45 deg <= theta < (o + 1) * 45 deg, decided by integer comparisons of dy, dx, |dy|, |dx|: a boundary
 *             ray belongs to the wedge that starts at it, (0, 0) is in wedge 0
 *   row [nid] the output row of an id; < 0: the id is not taken.  Ids that share a row are summed into it
 *   count [nrows][rings][wedges]  the pixels of the id with row[id] == r in ring k and wedge o
 *   isum  [nrows][rings][wedges]  Σ q over those pixels, q exactly clx_region_intensity's: CLX_RAW_I32: q = v, `shift` ignored;
 *             CLX_RAW_F32 / _F64: q = (long long) rint(ldexp((double) v, shift)) under the same per-pixel bound
 *             2^62 >> bit_length(Z*Y*X).  For every taken id the sum of isum over its rings and wedges is clx_region_intensity's
 *             isum for the same shift, bit for bit, and the sum of count is its area
 *   raw       may be NULL, and isum then too: counts only, raw_type and shift are ignored (an isum given all the same is zeroed)
 *   bad [1]   bit 0: a label outside [0, nid) -- never followed as an index, counts as background
 *             bit 1: a NaN, +-Inf or |q| above the bound under a taken id; that pixel is skipped in count and isum alike.
 *                    Such values on background and under ids that are not taken are ignored
 *             bit 2: the maps disagree: under a taken id a d2 outside [1, D2] (relative) or [1, CLX_DIST_INF] (absolute), or, with
 *                    wedges == 8, a centre index outside [0, Z*Y*X); the pixel is skipped.  No index outside count / isum is
 *                    ever formed, whatever inscribed, row and dist_sq hold (a D2 above 2^41 is cut there: every d2 is in ring 0
 *                    either way)
 *             bit 3: a row[id] >= nrows under a pixel of the map; the id is treated as not taken
 * The entry point initialises count, isum and bad itself.  Integer adds only: the same bits in every run.  Two launches,
 * whatever the number of objects: the initialisation, and one pass in which a block combines runs of pixels of one cell in a
 * table of 1024 cells in LDS that it adds to the outputs once.
 * Refused (CLX_ERR_ARG) before any launch, the outputs untouched: null pointers other than the raw / isum pair, an unknown
 * raw_type with a non-null raw, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent, Z*Y*X >= 2^32, nid outside
 * [1, 2^24], nrows outside [0, nid), rings outside [1, 32], width outside [0, 32768], wedges not 1 or 8, wedges == 8 with
 * nd == 3, nrows * rings * wedges >= 2^31. */
int clx_region_radial(const int32_t* labels, const int32_t* dist_sq, const void* raw, int raw_type, int nd, int Z, int Y,
                      int X, int nid, const unsigned long long* inscribed, const int32_t* row, int nrows, int rings,
                      int width, int wedges, int shift, unsigned long long* count, long long* isum, int32_t* bad,
                      clx_stream stream);
/* Sums of products of two raw channels per object: what the intensity standard deviation and the colocalization of two
 * channels inside every object need (cellulus_amd.measure.products_columns forms the columns: regionprops' intensity_std,
 * CellProfiler's MeasureColocalization).  labels, raw_a and raw_b hold npix values; both channels are of `raw_type`;
 * raw_a == raw_b is allowed.
 *   q_a, q_b  exactly clx_region_intensity's q of the two channels for shift_a and shift_b: CLX_RAW_I32: q = v, the shifts
 *             ignored; CLX_RAW_F32 / _F64: q = (long long) rint(ldexp((double) v, shift)) under the same per-pixel bound
 *             |q| <= 2^62 >> L, L = bit_length(npix).  A product is then at most 2^(124 - 2 L) in magnitude and a sum of fewer
 *             than 2^L of them is below 2^(124 - L): it fits a signed 128-bit integer, which is how the products are summed
 *   classes   a pixel of object i is "above a" when q_a >= thr_a[i], "above b" when q_b >= thr_b[i], "both" when it is above
 *             a and above b.  thr_a, thr_b [nid]: per-id thresholds in q units (any int64); both may be NULL together, and every
 *             pixel is then above both
 *   out [nid][20]  per id, as 64-bit words: [0] n, the pixels; [1] Σa, [2] Σb (signed, two's complement); [3] n_both;
 *             [4] Σa over the pixels above a, [5] Σb over those above b; [6] Σa, [7] Σb over `both`; then six signed 128-bit
 *             sums as (lo, hi) pairs of words, two's complement: [8,9] Σaa, [10,11] Σbb, [12,13] Σab over all the id's pixels,
 *             [14,15] Σaa, [16,17] Σbb, [18,19] Σab over `both`.  Σa and Σb equal clx_region_intensity's isum for the same
 *             shift bit for bit, and n is clx_region_moments' area.  Row 0 (background) is unspecified
 *   bad [1]   bit 0: a label outside [0, nid) -- never followed as an index, counts as background
 *             bit 1: under an object id a NaN, +-Inf or |q| above the bound in EITHER channel; that pixel is skipped in all
 *                    20 words.  Such values on the background are ignored
 * The entry point initialises out and bad itself.  Integer adds only; a 128-bit add, to LDS and to global memory alike, is
 * two 64-bit atomic adds (the low limbs, whose returned old value gives the carry exactly, then the high limbs plus carry),
 * and adds modulo 2^128 commute: the same map gives the same bits in every run.  Two launches, whatever the number of
 * objects: the initialisation, and one pass in which a block combines runs of pixels of one id in a table of 256 ids in LDS
 * (20 words an id with thresholds, 9 without, where the conditioned words are copies) that it adds to the output once.
 * Refused (CLX_ERR_ARG) before any launch, the outputs untouched: null pointers other than the threshold pair as a pair,
 * exactly one of thr_a / thr_b null, an unknown raw_type, nid outside [1, 2^24], npix outside [1, 2^32). */
int clx_region_products(const int32_t* labels, const void* raw_a, const void* raw_b, int raw_type, long long npix, int nid,
                        int shift_a, int shift_b, const long long* thr_a, const long long* thr_b,
                        unsigned long long* out /* [nid][20] */, int32_t* bad, clx_stream stream);
/* Intensity-weighted moments and the place of the peak per object: what the weighted centroid, the weighted covariance, the
 * mass displacement, the integrated intensity and the position of the brightest pixel need (cellulus_amd.measure.
 * weighted_columns forms the columns: regionprops' centroid_weighted, CellProfiler's Location_CenterMassIntensity,
 * MassDisplacement, Location_MaxIntensity, IntegratedIntensity).  labels and raw hold Z*Y*X values, x fastest; a 2-D map has Z = 1.
 *   counted   a pixel counts if its id lies in [1, nid) and its value quantises under clx_region_intensity's rule: CLX_RAW_I32:
 *             q = v, the shift ignored; CLX_RAW_F32 / _F64: q = (long long) rint(ldexp((double) v, shift)) with
 *             |q| <= 2^62 >> L, L = bit_length(Z*Y*X).  Every other pixel is skipped in all 21 words
 *   out [nid][21]  per id, as 64-bit words: [0] n, the counted pixels; [1] Σq modulo 2^64, two's complement (it equals
 *             clx_region_intensity's isum for the same shift bit for bit); [2] the smallest flat index p = (z*Y + y)*X + x among
 *             the counted pixels whose order key (clx_region_intensity's, of the raw value, not of q) equals peak_keys[id], ~0
 *             if there is none or peak_keys is NULL: with peak_keys[id] = vkey[2*id + 1] of clx_region_intensity the first pixel in
 *             raster order that attains the object's maximum; then nine signed 128-bit sums as (lo, hi) pairs of words, two's
 *             complement, in the order of clx_region_moments' sum1 and sum2: [3,4] Σq·z, [5,6] Σq·y, [7,8] Σq·x, [9,10] Σq·zz,
 *             [11,12] Σq·yy, [13,14] Σq·xx, [15,16] Σq·zy, [17,18] Σq·zx, [19,20] Σq·yx.  Every term is below 2^(62 - L) 2^(2 L) in
 *             magnitude and a sum of fewer than 2^L of them below 2^126: it fits.  Row 0 (background) is unspecified
 *   peak_keys [nid] or NULL
 *   bad [1]   bit 0: a label outside [0, nid) -- never followed as an index, counts as background
 *             bit 1: under an object id a NaN, +-Inf or |q| above the bound; that pixel is skipped.  Such values on the
 *                    background are ignored
 * The entry point initialises out and bad itself.  Integer adds and an integer minimum only; a 128-bit add is two 64-bit
 * atomic adds as in clx_region_products: the same map gives the same bits in every run.  Two launches, whatever the number of
 * objects: the initialisation, and one pass in which a block combines runs of pixels of one id and one image row in a table
 * of 256 ids in LDS that it adds to the output once.
 * Refused (CLX_ERR_ARG) before any launch, the outputs untouched: null pointers other than peak_keys, an unknown raw_type,
 * nid outside [1, 2^24], a non-positive extent, Z*Y*X >= 2^32. */
int clx_region_weighted(const int32_t* labels, const void* raw, int raw_type, int Z, int Y, int X, int nid, int shift,
                        const unsigned long long* peak_keys, unsigned long long* out /* [nid][21] */, int32_t* bad,
                        clx_stream stream);
/* Intensity on every object's rim (cellulus_amd.measure.border_intensity_columns forms the columns: CellProfiler's
 * IntegratedIntensityEdge, Mean- / Std- / Min- / MaxIntensityEdge).  A pixel of object i is a BORDER PIXEL if any of its
 * 2*nd face neighbours is not i: another object, background, an id outside [0, nid) or the outside of the image --
 * clx_region_perimeter's definition, in 3-D too.  nd 2 (Z must be 1; there are no z neighbours) or 3 (with Z == 1 every
 * object pixel is a border pixel).  Labels alone decide which pixels are border pixels; only their raw values are read.
 *   out [nid][7]  per id, as 64-bit words: [0] the border pixels (for nd == 2 clx_region_perimeter's class 0); over the
 *             border pixels whose value quantises under clx_region_intensity's rule for `shift` (as in clx_region_weighted):
 *             [1] their number, [2] Σq modulo 2^64, two's complement, [3] the smallest and [4] the largest order key
 *             (clx_region_intensity's; ~0 and 0 where word 1 is 0), [5,6] Σq² as a signed 128-bit (lo, hi) pair.  Row 0
 *             (background) is unspecified
 *   bad [1]   bit 0: a label outside [0, nid) -- counts as background, and makes border pixels of its neighbours
 *             bit 1: a border pixel whose value is a NaN, +-Inf or has |q| above the bound: it stays in word 0 and drops out of
 *                    words 1 - 6.  Such values anywhere else are not looked at
 * The entry point initialises out and bad itself; integer adds, minima and maxima only: the same map gives the same bits in
 * every run.  Two launches: the initialisation, and one pass over the label map with a stencil of 2*nd neighbours in which a
 * wave of 256 consecutive pixels without a border pixel reads no raw value at all.
 * Refused (CLX_ERR_ARG) before any launch, the outputs untouched: null pointers, an unknown raw_type, nd not 2 or 3, nd == 2
 * with Z != 1, a non-positive extent, Z*Y*X >= 2^32, nid outside [1, 2^24]. */
int clx_region_border_intensity(const int32_t* labels, const void* raw, int raw_type, int nd, int Z, int Y, int X, int nid,
                                int shift, unsigned long long* out /* [nid][7] */, int32_t* bad, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "relate" stage: two label maps of one image (label_overlap.hip)           */
/* ------------------------------------------------------------------------ */
/* Overlaps: the sparse joint histogram of two label maps a and b of npix pixels each -- which object of b every object of a
 * lies in and with how many pixels, where clx_joint_histogram fills a dense #a x #b table and needs ids below 2^16.
 *   pair      every pixel p with (a[p], b[p]) != (0, 0) counts once for the key ((u64) a[p] << 32) | b[p]; no key is 0.
 *             (i, 0): pixels of i over b's background; (0, j): pixels of j over a's.  The pixel counts |A_i| and |B_j| are the
 *             row and column sums of the table
 *   labels    a label outside [0, nid_a) resp. [0, nid_b) counts as 0, is never followed as an index and sets bit 0 (map a)
 *             resp. bit 1 (map b) of info[0]
 * Output: clx_region_contacts' open-addressing table of `capacity` slots (a power of two in [1024, 2^28]), under the same
 * contract.
 *   keys   [capacity]  (a << 32) | b; 0: empty slot
 *   counts [capacity]  pixels of that pair
 *   info   [2]         [0] bit 0 / bit 1: a label of a / b out of range; bit 2: a pair could not be placed -- the table is to be
 *                      discarded and the call repeated with a larger capacity.  [1] occupied slots (<= capacity)
 * The entry point initialises keys, counts and info itself.  The slot order is unspecified; the SET of (key, count) is
 * determined by the maps: integer adds only.  Either the set is exact or bit 2 is set.  An insertion probes at most
 * min(capacity, 4096) consecutive slots (modulo capacity) and then gives up with bit 2: it never spins and writes only
 * keys[0, capacity) and counts[0, capacity).  A caller repeats while bit 2 is set.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, npix outside [1, 2^32), nid_a or nid_b outside [1, 2^24], capacity
 * not a power of two in [1024, 2^28]. */
int clx_label_overlaps(const int32_t* a, const int32_t* b, long long npix, int nid_a, int nid_b, int capacity,
                       unsigned long long* keys, unsigned long long* counts, int32_t* info, clx_stream stream);
/* Clearance: how near every object of a comes to the boundary of the object of b it was assigned to (a nucleus to its cell's
 * membrane).  a, b and dist_sq: npix values each; dist_sq is clx_label_distance_sq's map of b.
 *   parent [nid_a]  for every id of a the id of b it belongs to, or 0 (cellulus_amd.relate.assign_parents); parent[0] is not read
 *   counted   a pixel p with i = a[p] in [1, nid_a), parent[i] > 0 and b[p] == parent[i].  Values of b and parent are only
 *             compared, never followed as an index
 *   out [nid_a][3], over the counted pixels of i:
 *             [0] their number
 *             [1] the smallest ((u64) dist_sq[p] << 32) | p: the smallest distance and the first pixel in raster order that
 *                 attains it; all ones if there is none.  sqrt(out[i][1] >> 32) is the clearance; 1: i touches the boundary
 *             [2] the sum of dist_sq
 *   bad [1]   bit 0: a label of a outside [0, nid_a) -- never followed as an index, that pixel is skipped
 *             bit 1: a dist_sq outside [0, CLX_DIST_INF] under a counted pixel; that pixel is skipped
 * The entry point initialises out and bad itself.  Integer minima and adds only: the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, npix outside [1, 2^32), nid_a outside [1, 2^24]. */
int clx_region_clearance(const int32_t* a, const int32_t* b, const int32_t* dist_sq, const int32_t* parent,
                         long long npix, int nid_a, unsigned long long* out, int32_t* bad, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "expand" stage: which object is nearest (label_nearest.hip)               */
/* ------------------------------------------------------------------------ */
/* Nearest object: the exact Euclidean feature transform of a label map [Z][Y][X] of int32 -- for every pixel which object is
 * nearest and how far it is: scipy's distance_transform_edt(labels == 0, return_indices=True) with a stated choice among
 * equidistant objects, skimage's expand_labels, the Voronoi zones of the objects.  nd == 2 needs Z == 1.
 *   object pixel  q with 0 < labels[q] < nid.  A label outside [0, nid) counts as background, is never followed as an index
 *             and sets bit 0 of bad[0] (value 1, as in the measure kernels)
 *   dist_sq   [Z][Y][X] int32: the smallest |p - q|^2 over the object pixels q, between pixel centres at unit spacing
 *   nearest   [Z][Y][X] int32: the SMALLEST label among the object pixels at that distance.  An object pixel gets its own
 *             label and 0.  The result is a function of the map alone: transposing the map transposes it
 *   limit_sq  -1: no limit.  >= 0: a pixel whose smallest squared distance exceeds limit_sq gets nearest 0 and dist_sq
 *             CLX_DIST_INF, as every pixel of a map without object pixels does
 *   bad [1]   cleared by the call
 *   workspace at least clx_label_nearest_workspace(Z*Y*X) bytes (a host-only function; 0: npix outside [1, 2^32)), 4-byte
 *             aligned: two more int32 maps, the other side of the passes' ping-pong
 * Every element of nearest and dist_sq is written.  Separable and exact: a pixel carries the key (d2 << 32) | id, a scan
 * along x and min-plus passes along y (and z) take the unsigned minimum.  Integers only: the same bits in every run.
 * The passes along y and z search outwards: their cost grows with the distance to the nearest object (at most
 * sqrt(limit_sq)); a map with one small object and no limit is the slow case.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent, nid
 * outside [1, 2^24], limit_sq outside [-1, 2^30), Z*Y*X >= 2^32, (Z-1)^2 + (Y-1)^2 + (X-1)^2 >= 2^30, workspace_bytes below
 * clx_label_nearest_workspace(Z*Y*X), a workspace that is not 4-byte aligned. */
size_t clx_label_nearest_workspace(long long npix);
int clx_label_nearest(const int32_t* labels, int nd, int Z, int Y, int X, int nid, int limit_sq,
                      int32_t* nearest, int32_t* dist_sq, int32_t* bad,
                      void* workspace, size_t workspace_bytes, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "split" stage: basins of the distance map (label_basins.hip)              */
/* ------------------------------------------------------------------------ */
/* Basins: a watershed of a label map [Z][Y][X] of int32 on its distance map dist_sq (clx_label_distance_sq's, or any int32 map
 * in [0, CLX_DIST_INF]) without a flood queue -- the declumping of touching objects by shape.  nd == 2 needs Z == 1.
 *   object pixel  p with labels[p] != 0 (negative values are objects, as in clx_label_distance_sq) and dist_sq[p] in
 *             [0, CLX_DIST_INF].  An object pixel with another dist_sq counts as background and sets bit 1 of info[0].  Labels
 *             are only compared with each other, never followed as an index
 *   neighbours  the 8 (nd == 2) or 26 pixels around p that lie inside the map and are object pixels of p's label; the ends of
 *             rows and slices never wrap
 *   key(p)    ((u64) dist_sq[p] << 32) | (2^32 - 1 - p), p the raster index: the larger distance is higher, among equal ones
 *             the smaller index.  No two pixels share a key
 *   up(p)     the neighbour with the largest key if that exceeds key(p), else p: a summit
 *   root      [Z][Y][X]: the raster index (as uint32) of the summit the chain p, up(p), up(up(p)), ... ends at;
 *             CLX_BASIN_NONE on pixels that are no object pixels.  Every element is written
 *   summits   [capacity]: the raster indices of the summits, in NO stated order (the caller sorts); capacity in [1, 2^30]
 *   info [2]  cleared by the call.  [0] bit 1: a dist_sq out of range under a label; bit 2: more summits than capacity -- the
 *             list holds `capacity` of them, root and the count are right.  [1] the exact number of summits (uint32)
 *   workspace at least clx_label_basins_workspace(Z*Y*X) bytes (a host-only function; 0: npix outside [1, 2^32)), 4-byte
 *             aligned: 16 status words and one more int32 map
 * One stencil launch and seven root launches, all queued on the stream: a root launch follows at most 64 links per pixel
 * between two buffers (no launch reads a word it writes), which multiplies the resolved length of every chain by 65, and
 * 65^7 > 2^32; a status word lets the launches after the last needed one return at once.  Integers only: the same bits in
 * every run, the order of the summit list aside.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent,
 * Z*Y*X >= 2^32, capacity outside [1, 2^30], workspace_bytes below clx_label_basins_workspace(Z*Y*X), a workspace that is not
 * 4-byte aligned. */
#define CLX_BASIN_NONE (-1)
size_t clx_label_basins_workspace(long long npix);
int clx_label_basins(const int32_t* labels, const int32_t* dist_sq, int nd, int Z, int Y, int X, int capacity,
                     int32_t* root, int32_t* summits, int32_t* info,
                     void* workspace, size_t workspace_bytes, clx_stream stream);
/* Passes: for every two basins of one label that have neighbouring pixels the height of the pass between them.
 *   pair      neighbouring pixels p, q (8 / 26, inside the map) with labels[p] == labels[q], root[p] != root[q] and neither root
 *             CLX_BASIN_NONE; every such pair is visited once, through the 4 / 13 forward offsets
 *   key       ((u64) min(root[p], root[q]) << 32) | max(root[p], root[q]); never 0, as the larger root is >= 1
 *   value     the maximum over the pair's pixel pairs of min(dist_sq[p], dist_sq[q])
 * Output: clx_region_contacts' open-addressing table of `capacity` slots (a power of two in [1024, 2^28]) under the same
 * contract, with the maximum in place of the count: keys [capacity] (0: empty slot), values [capacity], info [2] ([0] bit 2: a
 * pair could not be placed -- discard the table and repeat with a larger capacity; [1] occupied slots).  The entry point
 * initialises all three.  root is clx_label_basins' of the same labels and dist_sq; its values are compared and never
 * followed.  The set of (key, value) is determined by the maps: integer maxima only.
 * Refused (CLX_ERR_ARG) before any launch: null pointers, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent,
 * Z*Y*X >= 2^32, capacity not a power of two in [1024, 2^28]. */
int clx_basin_passes(const int32_t* labels, const int32_t* dist_sq, const int32_t* root, int nd, int Z, int Y, int X,
                     int capacity, unsigned long long* keys, unsigned long long* values, int32_t* info, clx_stream stream);
/* Relabel: out[p] = ids[i] where root[p] == summits[i], 0 where root[p] is CLX_BASIN_NONE.  (summits, ids, n): per summit the
 * id (>= 1) the caller gave it, n in [0, 2^30]; the list is scattered into a map of npix int32 in the workspace first.
 *   bad [1]   cleared by the call.  bit 0: a summit outside [0, npix), not followed; bit 1: a root that is no summit of the list
 *             or lies outside the map; that pixel gets 0
 *   workspace at least clx_label_basins_workspace(npix) bytes, 4-byte aligned
 * Every element of out is written.
 * Refused (CLX_ERR_ARG) before any launch: null pointers (summits and ids may be null with n == 0), npix outside [1, 2^32), n
 * outside [0, 2^30], workspace_bytes below clx_label_basins_workspace(npix), a workspace that is not 4-byte aligned. */
int clx_basin_relabel(const int32_t* root, long long npix, const int32_t* summits, const int32_t* ids, int n,
                      int32_t* out, int32_t* bad, void* workspace, size_t workspace_bytes, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "propagate" stage: seeds grown inside a mask, guided by an image          */
/* (label_propagate.hip)                                                     */
/* ------------------------------------------------------------------------ */
/* Propagation: for every pixel of three maps [Z][Y][X] the seed that reaches it on the cheapest path and that path's cost --
 * CellProfiler's IdentifySecondaryObjects "Propagation", skimage's watershed(image, markers, mask=...), without a flood queue
 * and with a stated choice among equal costs.  nd == 2 needs Z == 1.
 *   seeds     int32.  A pixel with 0 < seeds[p] < nid is a SEED pixel.  An id outside [0, nid) counts as a non-seed pixel of
 *             label 0, is never followed as an index and sets bit 0 of info[0] (value 1)
 *   mask      uint8, or NULL (all allowed).  A non-seed pixel is ALLOWED iff mask[p] != 0.  Seed pixels are always sources and
 *             keep their label, in or out of the mask
 *   weight    int32 in [0, 65535], or NULL (flat): the image in grey levels.  A weight outside that range under an allowed or
 *             seed pixel makes the pixel impassable -- no source and not allowed -- and sets bit 1 of info[0] (value 2)
 *   neighbours  the 8 (nd == 2) or 26 pixels around p inside the map; the ends of rows and slices never wrap
 *   step      from p to a neighbour q that is an allowed non-seed pixel: reg * a(p, q) + |weight[p] - weight[q]|, a = 3 for a
 *             face neighbour, 4 for an edge neighbour, 5 for a corner neighbour (the <3, 4, 5> chamfer); reg in [0, 65535]
 *   path      starts at a seed pixel and makes steps; its cost is their sum.  Paths costlier than `limit` do not exist; limit in
 *             [0, 2^30), -1: 2^30 - 1
 *   key       every pixel holds the key (cost, id) of its best path: the smaller cost wins, among equal costs the smaller seed
 *             id.  A seed pixel has (0, its label); a pixel that no path reaches has owner 0 and cost CLX_COST_INF.  Zero-cost
 *             steps are legal.  The keys are the least fixed point of key[q] = min(key[q], key[p] + step(p, q)): a function of
 *             the inputs alone; transposing the inputs transposes them
 *   owner, cost  [Z][Y][X] int32: the key.  While info[1] != 0 they hold an intermediate state
 *   rounds    1 .. 64: the relaxation rounds this call queues on the stream at most, without any host synchronisation
 *   resume    0: the call initialises owner, cost and the workspace from the seeds.  1: it continues from the state a call
 *             with the same other arguments left in owner, cost and workspace, and initialises nothing but info
 *   info [3]  cleared by the call.  [0] the two bits above (resume == 0 only).  [1] the tiles that changed in the last round of
 *             the call: 0 means the fixed point is reached and owner / cost hold the result.  [2] the rounds of this call in
 *             which some tile changed; summed over the calls it is the same in every run, whatever `rounds` each call was given
 *   workspace at least clx_label_propagate_workspace(nd, Z, Y, X) bytes (a host-only function; 0: a shape the call would
 *             refuse), 4-byte aligned: 16 head words, 64 round counters, two more int32 maps and two flag bytes per tile
 * A round is one launch: a block takes a tile of 1024 pixels (64 x 16, or 16 x 8 x 8) with a halo of one pixel, relaxes it in
 * LDS on whole 64-bit keys, at most 32 sweeps, and writes its interior to the other pair of planes (owner / cost and the
 * workspace's alternate: no launch reads a word it writes).  A tile works only if it or a neighbour tile changed in the round
 * before; the rounds after the fixed point return at once.  No block waits for another.  Integer minima only: the same bits
 * and the same rounds in every run.  cost <= 2^30 and a step < 2^19: a candidate fits 32 bits.
 * Refused (CLX_ERR_ARG) before any launch: null seeds, owner, cost, info or workspace, nd not 2 or 3, nd == 2 with Z != 1, a
 * non-positive extent, nid outside [1, 2^24], reg outside [0, 65535], limit outside [-1, 2^30), rounds outside [1, 64], resume
 * not 0 or 1, Z*Y*X >= 2^32, workspace_bytes below clx_label_propagate_workspace(nd, Z, Y, X), a workspace that is not 4-byte
 * aligned. */
#define CLX_COST_INF CLX_DIST_INF
size_t clx_label_propagate_workspace(int nd, int Z, int Y, int X);
int clx_label_propagate(const int32_t* seeds, const uint8_t* mask, const int32_t* weight,
                        int nd, int Z, int Y, int X, int nid, int reg, int limit, int rounds, int resume,
                        int32_t* owner, int32_t* cost, int32_t* info,
                        void* workspace, size_t workspace_bytes, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "fill" stage: holes inside the objects of a label map, closed             */
/* (label_holes.hip)                                                         */
/* ------------------------------------------------------------------------ */
/* Holes: CellProfiler's FillObjects / centrosome's fill_labeled_holes ("surrounded by a single object") on a stored label map,
 * for all objects in one call, with a census of the holes.
 *   input     one int32 map [Z][Y][X], 2-D (nd == 2, Z == 1) or 3-D.  Every non-zero value is an OBJECT pixel; the value is
 *             compared and never used as an index, so no nid argument is needed.  Value 0 is BACKGROUND
 *   neighbours and components  background pixels are FACE neighbours (4 in 2-D, 6 in 3-D): the complement of the 8 /
 *             26-connectivity the objects have in clx_cc_label_filter.  The ends of rows and slices never wrap.  A COMPONENT
 *             is a maximal face-connected set of background pixels
 *   planewise  with planewise == 1 (3-D only) z neighbours do not exist, and every slice is a 2-D map of its own
 *             (CellProfiler's planewise fill): the useful mode for stacks whose cavities are open along z
 *   reaching the border  a component REACHES THE BORDER iff one of its pixels has x in {0, X-1} or y in {0, Y-1}; in 3-D
 *             without planewise, z in {0, Z-1} counts as well
 *   hole      a component is a HOLE of label L iff it does not reach the border and every object pixel that is a face neighbour
 *             of one of its pixels carries the same value L.  Edge and corner neighbours do not count (centrosome's
 *             fill_labeled_holes rule: "surrounded by a single object")
 *   not a hole  a gap that touches two labels is not a hole and stays background; so does a ring between an object and a
 *             different object nested inside it.  A hole's FIRST pixel is its smallest raster index, its AREA its pixel count
 *   out       [Z][Y][X] int32, every element written: out[p] = labels[p] on object pixels; on a background pixel L if the
 *             pixel's component is a hole of L with area <= max_size (max_size == -1: no cap), otherwise 0.  With
 *             max_size == 0 nothing changes and the call is a census of the holes
 *   holes     [capacity][4] int32: for every hole, capped or not, one row (first, owner, area, kept); kept = 1: the hole
 *             exceeded max_size and was left open.  The order of the rows is unspecified; the host sorts them by first
 *   info [4]  cleared by the call.  [0] the number of holes found: it may exceed capacity -- rows beyond capacity are dropped,
 *             out is complete regardless.  [1] the number of pixels filled.  [2] the number of background components.
 *             [3] reserved, 0
 *   workspace at least clx_label_holes_workspace(nd, Z, Y, X) bytes (a host-only function; 0: a shape the call refuses), 4-byte
 *             aligned: 16 bytes per pixel -- the parent plane of a union-find over the background's horizontal runs, and at
 *             a component's root its area with the border bit, and the smallest and largest value among its face neighbours
 * Five plain launches on the stream and no host synchronisation: runs, link (lock-free atomicMin unions; only overlap in x
 * links, never a diagonal), flatten (with the border bits), reduce (the attributes of the components off the border), fill.  No
 * block waits for another; integers only; ids are 32-bit raster indices.  out, info and the set of rows are a function of the
 * input alone.
 * Refused (CLX_ERR_ARG) before any launch: null labels, out, info or workspace, null holes with capacity > 0, nd not 2 or 3,
 * nd == 2 with Z != 1, planewise not 0 or 1 or set with nd == 2, a non-positive extent, Z*Y*X >= 2^31, max_size < -1,
 * capacity < 0, workspace_bytes below clx_label_holes_workspace(nd, Z, Y, X), a workspace that is not 4-byte aligned,
 * out == labels. */
size_t clx_label_holes_workspace(int nd, int Z, int Y, int X);
int clx_label_holes(const int32_t* labels, int nd, int Z, int Y, int X, int planewise, long long max_size,
                    int capacity, int32_t* out, int32_t* holes, int32_t* info,
                    void* workspace, size_t workspace_bytes, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "skeleton" stage: every object thinned to its centre lines, and measured  */
/* (label_thin.hip)                                                          */
/* ------------------------------------------------------------------------ */
/* Thinning: CellProfiler's MorphologicalSkeleton, MATLAB's bwmorph('thin'), skimage.morphology.thin -- Guo & Hall 1989,
 * algorithm A1, two alternating sub-iterations -- on a stored label map, for all objects in one call, label-aware.
 *   input     one int32 map [Z][Y][X], 2-D (nd == 2, Z == 1) or 3-D.  Every non-zero value is an OBJECT pixel; the value is
 *             compared and never used as an index.  With nd == 3 every slice is a 2-D map of its own: z neighbours do not
 *             exist (3-D curve skeletons are not done).  The ends of rows and slices never wrap
 *   neighbours of p  P2 .. P9 = N, NE, E, SE, S, SW, W, NW, N at y - 1.  Pk = 1 iff that pixel lies inside the slice, is still
 *             alive and carries p's label.  A pixel of another label counts as background: touching objects thin independently
 *   counts    C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
 *             N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
 *   sub-iteration  every alive pixel with C == 1, 2 <= N <= 3 and m == 0 is deleted, all at once from the state before the
 *             sub-iteration.  Odd sub-iterations (the 1st, 3rd, ...): m = (P2 | P3 | !P5) & P4; even ones: m = (P6 | P7 | !P9) & P8
 *   iteration an odd, then an even sub-iteration over the whole map
 *   skeleton  the state after the first iteration that deletes nothing.  The rule is not transpose-equivariant
 *   out       [Z][Y][X] int32, every element written by every call: labels[p] where p is alive after the iterations run so
 *             far (over all calls since resume == 0), else 0
 *   iterations  1 .. 64: the whole iterations this call queues on the stream at most, without any host synchronisation
 *   resume    0: the call initialises the workspace from the labels.  1: it continues from the state a call with the same other
 *             arguments left in the workspace, and initialises nothing but info
 *   info [3]  cleared by the call.  [0] reserved, 0.  [1] the pixels deleted in the last iteration this call ran: 0 means the
 *             fixed point is reached and out holds the skeleton.  [2] the pixels deleted by this call; summed over the calls it
 *             is object pixels minus skeleton pixels, whatever `iterations` each call was given
 *   workspace at least clx_label_thin_workspace(nd, Z, Y, X) bytes (a host-only function; 0: a shape the call refuses), 8-byte
 *             aligned: 16 head words, 16 counters, ten bit planes of one 64-bit word per 64 pixels of a row (rows are padded
 *             to whole words) and two flag bytes per tile
 * The labels are read once, into bit planes: alive (two copies), and per neighbour "lies in my slice and has my label".  A
 * launch runs up to 8 iterations: a block loads 8 words x 128 rows of the alive plane -- a tile of 384 x 96 pixels and a halo of
 * 64 pixels / 16 rows -- into LDS, keeps the eight neighbour words of its words in registers, makes up to 16 bit-sliced
 * sub-iterations on chip (one 64-bit operation serves 64 pixels) and writes its tile to the other alive plane: no launch reads
 * a word it writes.  Every tile advances by the same sub-iterations a launch.  A tile works only if it or a neighbour tile
 * deleted a pixel in the launch before; the launches after the fixed point return at once.  No block waits for another.
 * Bits only: the same result in every run.
 * Refused (CLX_ERR_ARG) before any launch: null labels, out, info or workspace, nd not 2 or 3, nd == 2 with Z != 1, a
 * non-positive extent, Z*Y*X >= 2^31, iterations outside [1, 64], resume not 0 or 1, workspace_bytes below
 * clx_label_thin_workspace(nd, Z, Y, X), a workspace that is not 8-byte aligned, out == labels. */
size_t clx_label_thin_workspace(int nd, int Z, int Y, int X);
int clx_label_thin(const int32_t* labels, int nd, int Z, int Y, int X, int iterations, int resume,
                   int32_t* out, int32_t* info, void* workspace, size_t workspace_bytes, clx_stream stream);

/* Census of a thinned map (of any map: the definitions need no thinning), per label, slice by slice as above.
 *   face link      two face neighbours of one label
 *   diagonal link  two diagonal neighbours of one label, neither of whose two common face neighbours carries that label
 *   block          a 2 x 2 window in which all four pixels carry one label
 *   degree         of a pixel: the number of its links.  END: degree 1, JUNCTION pixel: degree >= 3, ISOLATED: degree 0
 *   words [nid][10] int64, initialised by the call: pixels, face_links, diag_links, blocks, ends, junctions, isolated, d2_sum,
 *             d2_min, d2_max.  Every link and block is counted once.  The last three are the sum and extremes of dist_sq over
 *             the label's pixels; with dist_sq == NULL, and for a label without pixels, 0, CLX_DIST_INF and -1.
 *             pixels - face_links - diag_links + blocks is the label's Euler number with 8-connectivity, on any map
 *   bad [1]   initialised by the call.  Bit 0: a label outside [0, nid): it counts as background, for its neighbours too, and
 *             is never an index.  Bit 1: a dist_sq outside [0, CLX_DIST_INF) under a counted pixel; that pixel's value is left
 *             out of the three d2 words
 * Runs of a label inside 64 pixels of a row are summed in the wave, a block combines them in a table in LDS keyed by label
 * (then straight to global memory) which it adds to the words once.  Integer atomics only: the same bits in every run.
 * Refused (CLX_ERR_ARG) before any launch: null skeleton, words or bad, nd not 2 or 3, nd == 2 with Z != 1, a non-positive
 * extent, Z*Y*X >= 2^31, nid outside [1, 2^24]. */
int clx_skeleton_census(const int32_t* skeleton, const int32_t* dist_sq, int nd, int Z, int Y, int X, int nid,
                        long long* words, int32_t* bad, clx_stream stream);

/* Branch graph of a thinned map (of any map: the definitions need no thinning), slice by slice as above (skeleton_graph.hip):
 * skan's summarize, CellProfiler's MeasureObjectSkeleton, ImageJ's AnalyzeSkeleton -- the census's pixel graph contracted to
 * nodes and branches, one row each, and one round of spur pruning.
 *   input     one int32 map [Z][Y][X], 2-D (nd == 2, Z == 1) or 3-D.  Every non-zero value is an OBJECT pixel; the value is
 *             compared and never used as an index, so no nid argument is needed.  With nd == 3 every slice is a 2-D map of its
 *             own.  The ends of rows and slices never wrap
 *   links and degree  exactly the census's: a face link joins two face neighbours of one label, a diagonal link two diagonal
 *             neighbours of one label neither of whose two common face neighbours carries it; a pixel's degree is the number
 *             of its links
 *   pixel kinds  a PATH pixel has degree 2, an END pixel degree 1, a JUNCTION pixel degree >= 3, an ISOLATED pixel degree 0
 *   node      a maximal set of junction pixels connected by links between two junction pixels (kind 3); an end pixel alone
 *             (kind 1); an isolated pixel alone (kind 0).  A node's ID is its smallest raster index
 *   branch    (a) a maximal set of path pixels connected by links between two path pixels, together with every link from one of
 *             them to a pixel that is no path pixel (a TERMINAL link); its FIRST is its smallest path pixel.  (b) a DIRECT
 *             branch: a single link between an end pixel and a junction pixel or between two end pixels; it has 0 path pixels
 *             and its first is the end pixel, the smaller one of two.  Links between two junction pixels belong to their node
 *             and are no branches
 *   terminals a path pixel has two links, so a branch of kind (a) has two terminal links or none; with none it is a CYCLE.  A
 *             full 2 x 2 block of one label on its own is a cycle of 4 pixels: each of its pixels has two face links and no
 *             diagonal one
 *   branch kind  0 end-end, 1 end-junction (a SPUR), 2 junction-junction (both terminals on one node included), 3 cycle
 *   branches  [capacity_b][13] int64: first, label, kind, path_pixels, face_links, diag_links (the terminal links included),
 *             pixel_a, pixel_b (the two pixels beyond the terminal links as raster indices, a <= b; -1, -1 for a cycle),
 *             node_a, node_b (the ids of the nodes these pixels belong to; -1, -1 for a cycle), d2_sum, d2_min, d2_max (the sum
 *             and extremes of dist_sq over the path pixels; with dist_sq == NULL, and for a branch without path pixels, 0,
 *             CLX_DIST_INF and -1)
 *   nodes     [capacity_n][7] int64: first (the id), label, kind, pixels, links_out (the branch terminals attached to the node;
 *             a branch with both ends on the node counts twice), inner_face, inner_diag (the links between two of its junction
 *             pixels, each counted once)
 *             Every link of the map lies in exactly one branch or inside exactly one node; every object pixel is a path pixel
 *             of one branch or a pixel of one node.  The order of the rows is unspecified; the host sorts them by first
 *   pruning   limit_q10 is a length in units of 1/1024 pixel.  A spur is PRUNED iff face_links + sqrt(2) diag_links <
 *             limit_q10 / 1024, decided in integers: with F = 1024 face_links, D = 1024 diag_links, T = limit_q10 it is not
 *             pruned if F >= T or D >= T, otherwise iff 2 D^2 < (T - F)^2 (no tie is possible but with diag_links == 0, where
 *             the test is F < T; T < 2^30 keeps the squares in 64 bits).  End-end branches, junction-junction branches and
 *             cycles are never pruned.  One call is one round: the junction a spur left may have become a path or an end pixel,
 *             so a second round is a second call on out
 *   branch_map  [Z][Y][X] int32 or NULL, every element written: first + 1 of its branch on a path pixel, -(node id + 1) on a
 *             node pixel, 0 on background
 *   out       [Z][Y][X] int32, every element written: labels with the path pixels and the end pixel of every pruned spur set
 *             to 0; the junction stays.  With limit_q10 == 0 out equals labels.  NULL is allowed with limit_q10 == 0
 *   info [6]  cleared by the call.  [0] the branches found, [1] the nodes found: they may exceed the capacities -- rows beyond
 *             capacity are dropped; branch_map, out and info are complete regardless.  [2] the pixels pruned.  [3] the spurs
 *             pruned.  [4] bad bits; bit 1: a dist_sq outside [0, CLX_DIST_INF) under a path pixel; that pixel's value is left
 *             out of the three d2 words.  [5] reserved, 0
 *   workspace at least clx_skeleton_graph_workspace(nd, Z, Y, X) = 40 * Z * Y * X bytes (a host-only function; 0: a shape the
 *             call refuses), 8-byte aligned: over raster indices the parent plane of a union-find, and at a root seven 32-bit
 *             words and one 64-bit word -- of a branch its path pixels, face links, diagonal links, smallest and largest
 *             terminal pixel and the three d2 words; of a node, in the first four of these planes, its pixels, links out, inner
 *             face links and inner diagonal links
 * Six plain launches on the stream and no host synchronisation: classify, link (lock-free atomicMin unions of path pixels with
 * path pixels and of junction pixels with junction pixels, each link taken once by the pixel that has it towards E, S, SE or
 * SW), flatten, reduce (the attributes at the roots), emit (the rows; a wave reserves those of 8 segments of 64 pixels with one
 * add to each counter), write.  No block waits for another; integer atomics only; ids are 32-bit raster indices.  Everything
 * written is a function of the input alone but the order of the rows.
 * Refused (CLX_ERR_ARG) before any launch: null labels, info or workspace, null branches with capacity_b > 0, null nodes with
 * capacity_n > 0, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent, Z*Y*X >= 2^31, a negative capacity, limit_q10
 * outside [0, 2^30), limit_q10 > 0 with a null out, workspace_bytes below clx_skeleton_graph_workspace(nd, Z, Y, X), a workspace
 * that is not 8-byte aligned, out == labels, branch_map == labels, out == branch_map. */
size_t clx_skeleton_graph_workspace(int nd, int Z, int Y, int X);
int clx_skeleton_graph(const int32_t* labels, const int32_t* dist_sq, int nd, int Z, int Y, int X, long long limit_q10,
                       int capacity_b, int capacity_n, int32_t* branch_map, int32_t* out, long long* branches,
                       long long* nodes, int32_t* info, void* workspace, size_t workspace_bytes, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* "granularity" stage: grey-scale morphology on a map of grey levels        */
/* (grey_morph.hip)                                                          */
/* ------------------------------------------------------------------------ */
/* Erosion, dilation and reconstruction by dilation -- the building blocks of CellProfiler's MeasureGranularity, of opening by
 * reconstruction, top-hat, h-maxima and regional maxima -- on int32 maps [Z][Y][X], 2-D (nd == 2, Z == 1) or 3-D.
 *   values    grey levels in [0, 65535]
 *   mask      uint8, or NULL (all inside).  A pixel with mask[p] == 0 is OUTSIDE, and so is everything beyond the map; the ends
 *             of rows and slices never wrap.  Outside pixels get 0 and conduct nothing
 *   neighbours  the 4 (nd == 2) or 6 FACE neighbours: CellProfiler's footprint, the disc of radius 1
 *   bad values  a value outside [0, 65535] under an inside pixel counts as 0 and sets a bad bit
 *
 * clx_grey_morph: op 0 erodes, op 1 dilates.  One step: out[p] = the min / max of in over p and its inside face neighbours;
 * `steps` = k steps are the step applied k times: the min / max over the inside pixels reachable from p by at most k face steps
 * through inside pixels -- without a mask the L1 ball of radius k.
 *   steps     1 .. 16 (nd == 3: 1 .. 4): all of them are made on chip in one launch; callers chain calls for more
 *   out       [Z][Y][X] int32, every element written; must not alias in
 *   bad [1]   initialised by the call.  Bit 0: a value of `in` out of range under an inside pixel
 * A block takes a tile (64 x 32, or 32 x 8 x 8) and a halo of `steps` pixels, as 16-bit values and inside bits in LDS, applies
 * the step `steps` times between two LDS buffers, each on the region it is still exact on, and writes the tile.
 * Refused (CLX_ERR_ARG) before any launch: null in, out or bad, nd not 2 or 3, nd == 2 with Z != 1, a non-positive extent,
 * Z*Y*X >= 2^32, op not 0 or 1, steps outside [1, 16] (nd == 3: [1, 4]), out == in or out == mask.
 *
 * clx_grey_reconstruct: reconstruction by dilation of `marker` under `image`.  With m = min(marker, image) pointwise, out is
 * the least map r >= m with r[p] = min(image[p], max(r[p], max over the inside face neighbours q of r[q])): out[p] is the
 * maximum, over the face-connected paths of inside pixels from some q to p, of min(m[q], the smallest image value on the path).
 * So m <= out <= image, reconstructing out again changes nothing, out is monotone in marker, and transposing the inputs
 * transposes out.  The value only rises from m and every value it takes is that of a real path: the fixed point reached from
 * below is the least one whatever the order of the updates, a function of the inputs alone.
 *   out       [Z][Y][X] int32.  While info[1] != 0 it holds an intermediate state; must not alias marker, image or mask
 *   rounds    1 .. 64: the rounds this call queues on the stream at most, without any host synchronisation
 *   resume    0: the call initialises out and the workspace from marker, image and mask.  1: it continues from the state a call
 *             with the same other arguments left in out and workspace, and initialises nothing but info
 *   info [3]  cleared by the call.  [0] (resume == 0 only) bit 0: a marker value out of range under an inside pixel, bit 1: an
 *             image value.  [1] the tiles that changed in the last round of the call: 0 means the fixed point is reached and
 *             out holds the result.  [2] the rounds of this call in which some tile changed; summed over the calls it is the
 *             same in every run, whatever `rounds` each call was given
 *   workspace at least clx_grey_reconstruct_workspace(nd, Z, Y, X) bytes (a host-only function; 0: a shape the call refuses),
 *             4-byte aligned: 16 head words, 64 round counters, one more int32 map, two flag bytes per tile and the image as
 *             16-bit words
 * A round is one launch: a block takes a tile (256 x 32, or 64 x 8 x 8) with a halo of one pixel, 16-bit values in LDS, and
 * makes sweeps of directional scans -- +x, -x, +y, -y (+z, -z) -- until a sweep changes nothing, at most 16 of them (a tile cut
 * short counts as changed), then writes its interior to the other plane (out and the workspace's alternate: no launch reads a
 * word it writes).  Along a row 64 pixels are one wave scan over clamps x -> min(hi, max(lo, x)), whose composition is again
 * a clamp.  A tile works only if it or a face-, edge- or corner-adjacent tile changed in the round before; the rounds after the
 * fixed point return at once.  No block waits for another.  Integer minima and maxima only: the same bits and the same rounds
 * in every run.  Because the fixed point is unique only info[2] depends on the inner loop.
 * Refused (CLX_ERR_ARG) before any launch: null marker, image, out, info or workspace, nd not 2 or 3, nd == 2 with Z != 1, a
 * non-positive extent, Z*Y*X >= 2^32, rounds outside [1, 64], resume not 0 or 1, workspace_bytes below
 * clx_grey_reconstruct_workspace(nd, Z, Y, X), a workspace that is not 4-byte aligned, out == marker, image or mask. */
int clx_grey_morph(const int32_t* in, const uint8_t* mask, int nd, int Z, int Y, int X, int op, int steps,
                   int32_t* out, int32_t* bad, clx_stream stream);
size_t clx_grey_reconstruct_workspace(int nd, int Z, int Y, int X);
int clx_grey_reconstruct(const int32_t* marker, const int32_t* image, const uint8_t* mask,
                         int nd, int Z, int Y, int X, int rounds, int resume, int32_t* out, int32_t* info,
                         void* workspace, size_t workspace_bytes, clx_stream stream);

/* ------------------------------------------------------------------------ */
/* Input decoding (host side): the Blosc/LZ4 chunks zarr writes by default    */
/* (docs/examples/2d/01-data.py:35-50, read by zarr_dataset.py:104-121)       */
/* ------------------------------------------------------------------------ */
/* LZ4 block decoder on HOST buffers; returns the bytes written (<= dst_capacity) or < 0. */
long long clx_lz4_decompress(const unsigned char* src, long long src_bytes, unsigned char* dst,
                             long long dst_capacity);
/* BloscLZ stream decoder (codec 0 of a Blosc chunk) on HOST buffers; same return convention. */
long long clx_blosclz_decompress(const unsigned char* src, long long src_bytes, unsigned char* dst,
                                 long long dst_capacity);
/* Writer side (HOST buffers): one Blosc chunk, LZ4 inside, byte shuffle on / off — what zarr-python writes with
 * its default compressor (zarr outputs of predict / detect / segment, cellulus/predict.py:103-110 etc.).
 * dst must hold clx_blosc_compress_bound(nbytes) bytes; returns the chunk size or < 0. */
long long clx_blosc_compress_bound(long long nbytes);
long long clx_blosc_compress_lz4(const unsigned char* src, long long nbytes, int typesize, int shuffle,
                                 unsigned char* dst, long long dst_capacity);
/* inverse of Blosc's byte shuffle for n bytes of elements of `typesize` bytes (HOST buffers) */
int clx_unshuffle_bytes(const unsigned char* src, unsigned char* dst, long long n, int typesize);

#ifdef __cplusplus
}
#endif
#endif /* CLX_H */
