"""GPU: the gradient of UNetModel's output with respect to the input image (raw.grad) — the first convolution's data
gradient (clx_conv_first_dgrad for 1-4 channels, the generic data-gradient convolution above that or with
CLX_FIRST_DGRAD=0) behind the data gradients of every other layer.  Judged like the parameter gradients of
tests/test_gpu_unet.py: against the float64 oracle evaluated on the HIP forward pass's own ReLU gates and pooling
winners, with a sanity bound against the free-running oracle."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

from cellulus_amd import _clx
from cellulus_amd.models import get_model
from cellulus_amd.models.plan import DualPlan, pad4
from oracle.unet_oracle import OracleUNetModel, forced_decisions

pytestmark = pytest.mark.gpu

CONFIGS = {
    "2d_grey": dict(cfg=dict(in_channels=1, out_channels=2, num_fmaps=8, fmap_inc_factor=3, features_in_last_layer=16,
                             downsampling_factors=[[2, 2]], num_spatial_dims=2), spatial=(44, 52), batch=3),
    "2d_two_channels": dict(cfg=dict(in_channels=2, out_channels=2, num_fmaps=6, fmap_inc_factor=2,
                                     features_in_last_layer=10, downsampling_factors=[[2, 2]], num_spatial_dims=2),
                            spatial=(36, 40), batch=2),
    "3d_grey": dict(cfg=dict(in_channels=1, out_channels=3, num_fmaps=4, fmap_inc_factor=2, features_in_last_layer=8,
                             downsampling_factors=[[2, 2, 2]], num_spatial_dims=3), spatial=(20, 20, 24), batch=2),
    # 128 feature maps: the layers above the first run their products in the split precision (csrc/gemm_sp.hip)
    "2d_sp128": dict(cfg=dict(in_channels=1, out_channels=2, num_fmaps=128, fmap_inc_factor=2, features_in_last_layer=64,
                              downsampling_factors=[[2, 2]], num_spatial_dims=2), spatial=(52, 44), batch=2),
    # more than four channels: the generic data-gradient convolution
    "2d_five_channels": dict(cfg=dict(in_channels=5, out_channels=2, num_fmaps=8, fmap_inc_factor=2,
                                      features_in_last_layer=8, downsampling_factors=[[2, 2]], num_spatial_dims=2),
                             spatial=(36, 40), batch=2),
}


def _make(name, device, seed=0, batch=None):
    c = CONFIGS[name]
    torch.manual_seed(seed)
    oracle = OracleUNetModel(**c["cfg"])
    for _n, layer in oracle.named_modules():
        if isinstance(layer, torch.nn.modules.conv._ConvNd):
            torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
            torch.nn.init.uniform_(layer.bias, -0.1, 0.1)
    model = get_model(**c["cfg"])
    model.load_state_dict(oracle.state_dict(), strict=True)
    model = model.to(device)
    raw = torch.rand(batch or c["batch"], c["cfg"]["in_channels"], *c["spatial"])
    return oracle, model, raw


def _train_plan(model):
    plans = [p for k, p in model._plans.items() if k[2]]
    assert len(plans) == 1
    return plans[0]


def _decisions(plan):
    """the ReLU gates and pooling winners of the plan's last forward pass, in the oracle's call order"""
    nd = plan.topo.nd

    def planar(tensor_name):
        shape, c = plan.topo.shapes[tensor_name]
        t = plan.buf[tensor_name].view((plan.B,) + tuple(shape) + (-1,))[..., :c].permute(0, 4, 1, 2, 3).contiguous().cpu()
        return t[:, :, 0] if nd == 2 else t

    masks = [planar(layer.out) > 0 for layer in plan.topo.convs if layer.relu]
    pool = F.max_pool2d if nd == 2 else F.max_pool3d
    winners = [pool(planar(p.src), p.factor[3 - nd:], stride=p.factor[3 - nd:], return_indices=True)[1]
               for p in plan.topo.pools]
    return masks, winners


def _oracle_input_grad(oracle64, raw, dout, decisions=None):
    x = raw.double().clone().requires_grad_(True)
    if decisions is None:
        oracle64(x).backward(dout.double())
    else:
        with forced_decisions(oracle64, *decisions):
            oracle64(x).backward(dout.double())
    return x.grad


def _check(got, ref, free, what):
    got = got.detach().cpu().double()
    l2 = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    err = ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()
    assert l2 < 1e-4, f"{what}: rel L2 {l2}"
    assert err < 1e-3, f"{what}: max err / max |ref| {err}"
    fl2 = ((got - free).norm() / (free.norm() + 1e-30)).item()
    assert fl2 < 1e-1, f"{what}: rel L2 {fl2} against the free-running float64 oracle"


def _run_and_check(name, model, oracle, raw, device, seed=2):
    x = raw.to(device).requires_grad_(True)
    out = model(x)
    torch.manual_seed(seed)
    dout = torch.randn(out.shape)
    out.backward(dout.to(device))
    assert x.grad is not None and x.grad.shape == raw.shape
    plan = _train_plan(model)
    oracle64 = oracle.double()
    ref = _oracle_input_grad(oracle64, raw, dout, _decisions(plan))
    free = _oracle_input_grad(oracle64, raw, dout)
    _check(x.grad, ref, free, name)
    return x.grad, plan


@pytest.mark.parametrize("name", list(CONFIGS))
def test_input_grad_matches_float64_oracle(name, device):
    oracle, model, raw = _make(name, device, seed=1)
    _run_and_check(name, model, oracle, raw, device)


def test_input_grad_two_streams(device, monkeypatch):
    monkeypatch.setenv("CLX_STREAMS_MIN_GFLOP", "0")
    oracle, model, raw = _make("2d_grey", device, seed=3, batch=4)
    _g, plan = _run_and_check("2d_grey/two streams", model, oracle, raw, device)
    assert isinstance(plan, DualPlan)


def test_input_grad_with_frozen_parameters(device):
    oracle, model, raw = _make("3d_grey", device, seed=4)
    torch.manual_seed(5)
    x = raw.to(device).requires_grad_(True)
    out = model(x)
    dout = torch.randn(out.shape).to(device)
    out.backward(dout)
    trainable = x.grad.clone()
    frozen = get_model(**CONFIGS["3d_grey"]["cfg"])
    frozen.load_state_dict(oracle.state_dict(), strict=True)
    frozen = frozen.to(device).requires_grad_(False)
    x2 = raw.to(device).requires_grad_(True)
    out2 = frozen(x2)
    assert out2.requires_grad
    (g,) = torch.autograd.grad(out2, x2, dout)
    assert all(p.grad is None for p in frozen.parameters())
    l2 = ((g - trainable).norm() / trainable.norm()).item()
    assert l2 < 1e-6, l2
    # backward() on the frozen network: the gradient reaches raw, no parameter gets one
    frozen(x2).backward(dout)
    assert x2.grad is not None and all(p.grad is None for p in frozen.parameters())


def test_input_grad_composes_with_autograd(device):
    oracle, model, raw = _make("2d_grey", device, seed=6)
    a = torch.tensor(1.3, device=device, requires_grad=True)
    b = torch.tensor(-0.2, device=device, requires_grad=True)
    out = model(raw.to(device) * a + b)
    torch.manual_seed(7)
    dout = torch.randn(out.shape)
    out.backward(dout.to(device))
    plan = _train_plan(model)
    decisions = _decisions(plan)
    o64 = oracle.double()
    a64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    b64 = torch.tensor(-0.2, dtype=torch.float64, requires_grad=True)
    with forced_decisions(o64, *decisions):
        o64(raw.double() * a64 + b64).backward(dout.double())
    x = raw.double().clone().requires_grad_(True)
    with forced_decisions(o64, *decisions):
        o64(x * 1.3 - 0.2).backward(dout.double())
    dxr = x.grad / 1.3                     # d loss / d (raw * a + b)
    # bounds scaled by the sums of magnitudes: a.grad and b.grad are sums of terms of either sign
    assert abs(a.grad.item() - a64.grad.item()) < 1e-4 * (raw.double() * dxr).abs().sum().item()
    assert abs(b.grad.item() - b64.grad.item()) < 1e-4 * dxr.abs().sum().item()
    # a second backward accumulates into raw.grad, as torch does
    xr = raw.to(device).requires_grad_(True)
    model(xr).backward(dout.to(device))
    first = xr.grad.clone()
    model(xr).backward(dout.to(device))
    assert torch.allclose(xr.grad, 2 * first, rtol=1e-6, atol=1e-7 * first.abs().max().item())


def _first_dgrad_ref(dy, w, B, cin, OD, OH, OW, KD, N):
    """float64 torch reference of clx_conv_first_dgrad"""
    dyp = dy[:, :N].double().view(B, OD, OH, OW, N).permute(0, 4, 1, 2, 3)
    if KD == 1:
        return torch.nn.grad.conv2d_input((B, cin, OH + 2, OW + 2), w.double()[:, :, 0], dyp[:, :, 0]).unsqueeze(2)
    return torch.nn.grad.conv3d_input((B, cin, OD + 2, OH + 2, OW + 2), w.double(), dyp)


@pytest.mark.parametrize("cin, KD, N, B, OD, OH, OW", [
    (1, 1, 6, 2, 1, 7, 9),
    (2, 1, 64, 3, 1, 13, 17),
    (3, 1, 256, 1, 1, 11, 5),
    (4, 1, 64, 2, 1, 9, 12),
    (1, 3, 6, 2, 5, 7, 9),
    (2, 3, 64, 1, 4, 6, 11),
    (3, 3, 6, 1, 3, 5, 5),
    (4, 3, 256, 1, 4, 10, 12),
    (1, 3, 64, 1, 32, 10, 12),       # a deep, narrow volume: runs of z planes per workgroup
    (1, 1, 256, 2, 1, 40, 150),      # several workgroups along each image row
    (1, 3, 64, 2, 9, 30, 131),
])
def test_first_dgrad_kernel_matches_float64(cin, KD, N, B, OD, OH, OW, device):
    torch.manual_seed(cin * 100 + KD * 10 + N)
    M = B * OD * OH * OW
    ld = pad4(N)
    dy = torch.randn(M, ld)
    if ld > N:
        dy[:, N:] = float("nan")           # pad lanes hold garbage: they must not be read
    w = torch.randn(N, cin, KD, 3, 3)
    ref = _first_dgrad_ref(dy, w, B, cin, OD, OH, OW, KD, N)
    dyd, wd = dy.to(device), w.to(device)
    outs = []
    for _ in range(2):
        dx = torch.full(ref.shape, float("nan"), dtype=torch.float32, device=device)
        _clx.call("clx_conv_first_dgrad", _clx.ptr(dyd), ld, _clx.ptr(wd), N, cin, B, OD, OH, OW, KD, _clx.ptr(dx),
                  _clx.stream_ptr(device))
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    got = outs[0].double()
    assert torch.isfinite(got).all()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    l2 = ((got - ref).norm() / ref.norm()).item()
    assert err < 2e-5 and l2 < 5e-6, (err, l2)


@pytest.mark.parametrize("name", ["2d_grey", "3d_grey"])
def test_kernel_and_generic_route_agree(name, device, monkeypatch):
    _oracle, model, raw = _make(name, device, seed=8)
    torch.manual_seed(9)
    grads = []
    for route in ("1", "0"):
        monkeypatch.setenv("CLX_FIRST_DGRAD", route)
        x = raw.to(device).requires_grad_(True)
        out = model(x)
        out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(device))
        grads.append(x.grad.double())
        assert bool(_train_plan(model).dx_bufs) == (route == "0")
    l2 = ((grads[0] - grads[1]).norm() / grads[1].norm()).item()
    err = ((grads[0] - grads[1]).abs().max() / grads[1].abs().max()).item()
    assert l2 < 1e-6 and err < 1e-5, (l2, err)


@pytest.mark.parametrize("name", ["2d_grey", "3d_grey"])
def test_input_grad_reproducible(name, device, monkeypatch):
    monkeypatch.setenv("CLX_DETERMINISTIC", "1")
    _oracle, model, raw = _make(name, device, seed=10)
    runs = []
    for _ in range(2):
        x = raw.to(device).requires_grad_(True)
        out = model(x)
        out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(11)).to(device))
        runs.append(x.grad.cpu())
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("name, route", [("2d_grey", "0"), ("2d_five_channels", "1")])
def test_no_input_grad_buffers_without_raw_requires_grad(name, route, device, monkeypatch):
    monkeypatch.setenv("CLX_FIRST_DGRAD", route)
    _oracle, model, raw = _make(name, device, seed=12)
    x = raw.to(device)
    out = model(x)
    out.backward(torch.ones_like(out))
    assert x.grad is None
    plan = _train_plan(model)
    assert not plan.dx_bufs
    assert all(p.grad is not None for p in model.parameters())
    # (the same plan makes them once raw asks for its gradient)
    xg = raw.to(device).requires_grad_(True)
    model(xg).backward(torch.ones_like(out))
    assert xg.grad is not None and plan.dx_bufs
