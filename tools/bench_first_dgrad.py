"""Times the input-image gradient of the first convolution: clx_conv_first_dgrad against the generic route (data-gradient
convolution through clx_conv_fwd into pixel-major scratch + clx_pixel_to_planar) on the benchmark shapes, with a float64
check on one image; then one model(raw) + backward at the 2-D benchmark config with and without raw.requires_grad."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cellulus_amd import _clx  # noqa: E402
from cellulus_amd._clx import ClxConvDesc, ClxSrc  # noqa: E402
from cellulus_amd.models import get_model  # noqa: E402
from cellulus_amd.models.plan import precision_code  # noqa: E402

dev = torch.device("cuda:0")
PEAK_TBS = 8.0
REPS = 20


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def case(label, B, N, KD, O):
    OD = O if KD == 3 else 1
    OH = OW = O
    D, H, W = OD + KD - 1, OH + 2, OW + 2
    M = B * OD * OH * OW
    taps = KD * 9
    torch.manual_seed(0)
    dy = torch.randn(M, N, device=dev)
    w = torch.randn(N, 1, KD, 3, 3, device=dev) * 0.05
    dx = torch.empty(B, 1, D, H, W, device=dev)
    st = _clx.stream_ptr(dev)

    def kernel():
        _clx.call("clx_conv_first_dgrad", _clx.ptr(dy), N, _clx.ptr(w), N, 1, B, OD, OH, OW, KD, _clx.ptr(dx), st)

    # the generic route (plan.UNetPlan.first_dgrad with CLX_FIRST_DGRAD=0)
    wp = torch.empty(4 * taps * N, device=dev)
    px = torch.empty(B * D * H * W, 4, device=dev)
    dx2 = torch.empty_like(dx)
    d = ClxConvDesc()
    d.nsrc = 1
    s = ClxSrc()
    s.ptr = dy.data_ptr(); s.C = N; s.ld = N; s.D, s.H, s.W = OD, OH, OW
    s.oz = s.oy = s.ox = 0; s.fz = s.fy = s.fx = 1
    d.src[0] = s
    d.B = B; d.ID, d.IH, d.IW = OD, OH, OW; d.KD, d.KH, d.KW = KD, 3, 3; d.PD, d.PH, d.PW = KD - 1, 2, 2
    d.N = 4; d.wpack = wp.data_ptr(); d.out = px.data_ptr(); d.ld_out = 4; d.precision = precision_code()

    def generic():
        _clx.call("clx_pack_weights", _clx.ptr(w), _clx.ptr(wp), N, 1, taps, 4, N, 1, st)
        _clx.call("clx_conv_fwd", ctypes.byref(d), st)
        _clx.call("clx_pixel_to_planar", _clx.ptr(px), _clx.ptr(dx2), B, 1, D * H * W, 4, st)

    t_k = timed(kernel)
    t_g = timed(generic)
    # float64 check on image 0
    npix = OD * OH * OW
    dy0 = dy[:npix].double().cpu().view(OD, OH, OW, N).permute(3, 0, 1, 2).unsqueeze(0)
    w64 = w.double().cpu()
    if KD == 1:
        ref = torch.nn.grad.conv2d_input((1, 1, H, W), w64[:, :, 0], dy0[:, :, 0]).unsqueeze(2)
    else:
        ref = torch.nn.grad.conv3d_input((1, 1, D, H, W), w64, dy0)
    scale = ref.abs().max().item()
    err_k = (dx[:1].double().cpu() - ref).abs().max().item() / scale
    err_g = (dx2[:1].double().cpu() - ref).abs().max().item() / scale
    nbytes = M * N * 4 + dx.numel() * 4 + w.numel() * 4
    flops = 2.0 * M * N * taps
    for name, t, err in (("clx_conv_first_dgrad", t_k, err_k), ("generic route", t_g, err_g)):
        tbs = nbytes / (t * 1e-3) / 1e12
        print(f"{label:34s} {name:22s} {t:8.3f} ms  {nbytes / 1e6:7.1f} MB  {flops / 1e9:5.2f} GFLOP  {tbs:5.2f} TB/s "
              f"({100 * tbs / PEAK_TBS:4.1f} % of {PEAK_TBS:.0f})  max err / max |ref| {err:.1e}")
    print(f"{label:34s} kernel / generic: {t_g / t_k:.2f}x faster")
    del dy, px


def end_to_end():
    cfg = dict(in_channels=1, out_channels=2, num_fmaps=256, fmap_inc_factor=3, features_in_last_layer=64,
               downsampling_factors=[[2, 2]], num_spatial_dims=2)
    torch.manual_seed(0)
    model = get_model(**cfg).to(dev)
    raw = torch.rand(8, 1, 256, 256, device=dev)
    out = model(raw)
    dout = torch.randn(out.shape, device=dev)
    del out

    def step(want_dx):
        x = raw.detach().requires_grad_(want_dx)
        model(x).backward(dout)

    res = {False: [], True: []}
    for want in (False, True):
        for _ in range(2):
            step(want)
    torch.cuda.synchronize()
    for _ in range(5):                      # alternating, device events around each forward + backward
        for want in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(want)
            e1.record()
            torch.cuda.synchronize()
            res[want].append(e0.elapsed_time(e1))
    a, b = sorted(res[False]), sorted(res[True])
    ma, mb = a[len(a) // 2], b[len(b) // 2]
    print(f"model(raw) + backward, 2-D benchmark config (B=8, 256^2, 256 fmaps), median of 5: "
          f"{ma:.2f} ms without raw.grad, {mb:.2f} ms with  (+{100 * (mb - ma) / ma:.2f} %)")
    print(f"  runs without: {' '.join(f'{v:.2f}' for v in res[False])}")
    print(f"  runs with:    {' '.join(f'{v:.2f}' for v in res[True])}")


if __name__ == "__main__":
    print(f"device: {torch.cuda.get_device_name(0)}; CLX_PRECISION code {precision_code()}")
    case("2-D first layer, B=8, dY [8*254^2, 256]", 8, 256, 1, 254)
    case("2-D first layer, B=4, dY [4*254^2, 256]", 4, 256, 1, 254)
    case("3-D first layer, B=8, dY [8*62^3, 64]", 8, 64, 3, 62)
    torch.cuda.empty_cache()
    if "--no-e2e" not in sys.argv:
        end_to_end()
