"""GPU: the changed-rows path of infer mode (UNetModel._sparse_prepare, UNetPlan._pointwise_on_rows) at a channel count
that is no multiple of 4, after the device's caching allocator has been handed memory full of NaN.  The compact row
buffers of that path are 8 lanes wide for 6 channels; the 1x1 kernels write the 6 real ones, the next layer reads all 8
(the pad lanes times zero weights) and the scatter copies all 8 into the dense tensor.  Pad lanes left as the allocator's
memory turn a NaN into NaN * 0 = NaN and, behind a ReLU, into 0: finite, wrong embeddings."""

import pytest
import torch

from cellulus_amd.models import get_model

pytestmark = pytest.mark.gpu

CFG = dict(in_channels=2, out_channels=2, num_fmaps=6, fmap_inc_factor=2, features_in_last_layer=10,
           downsampling_factors=[[2, 2]], num_spatial_dims=2)


def _poison(device):
    """return blocks of many sizes, filled with NaN, to the caching allocator"""
    held = [torch.full((n,), float("nan"), device=device) for n in (1 << k for k in range(6, 22)) for _ in range(6)]
    torch.cuda.synchronize()
    del held


@pytest.mark.parametrize("streams", ["2", "1"])
def test_changed_rows_equal_dense_forward_after_nan_memory(streams, device, monkeypatch):
    torch.manual_seed(6)
    model = get_model(**CFG)
    for _n, layer in model.named_modules():
        if isinstance(layer, torch.nn.modules.conv._ConvNd):
            torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
            torch.nn.init.uniform_(layer.bias, -0.1, 0.1)
    model = model.to(device)
    raw = torch.rand(2, 2, 36, 40)
    noise = torch.rand(2, 8, 2, 36, 40, generator=torch.Generator().manual_seed(2))
    x = raw.to(device)
    monkeypatch.setenv("CLX_STREAMS_MIN_GFLOP", "0")
    monkeypatch.setenv("CLX_INFER_STREAMS", streams)
    model.max_infer_batch = 4
    model.set_infer(p_salt_pepper=0.008, num_infer_iterations=4, device=device)
    monkeypatch.setenv("CLX_SPARSE_NOISE", "0")
    dense = model.infer_on_device(x, noise=noise).clone()
    monkeypatch.delenv("CLX_SPARSE_NOISE")
    _poison(device)
    sparse = model.infer_on_device(x, noise=noise)
    assert model._last_changed_rows["used"], "the changed-rows path was expected at 0.8 % noise"
    assert torch.equal(dense, sparse)
    plan = next(p for k, p in model._plans.items() if not k[2])
    for buf in plan._compact_bufs.values():
        assert torch.isfinite(buf).all()
    first, tail = plan.pointwise_prefix()
    last = plan.buf[tail[-1].out]
    assert not last[:, tail[-1].cout:].any(), "pad lanes of the dense tensor behind the changed rows are not zero"
