"""The opt-in precision value CLX_PREC_F32X3BF16_G64 (clx_conv_desc.precision = 2, CLX_PRECISION=f32x3bf16g64): the split
precision of csrc/gemm_sp.hip under the 64-channel granule of the P3 planes instead of the 128 of the first kernels' tiles.
Without a GPU: what clx_conv_sp_covers answers for the three precision values, the cache sizes that follow it, the
refusals in front of any launch (fake pointers), and the switch of the Python layer.

Replaces the same reference arithmetic as the default kernels: nn.Conv{2,3}d in float32 (cellulus/models/unet.py:24-63).
"""
import ctypes

import pytest

from test_cpu_host import _sp_desc


def _covers(lib, d):
    return lib.clx_conv_sp_covers(ctypes.byref(d), 0), lib.clx_conv_sp_covers(ctypes.byref(d), 1)


# (arguments of _sp_desc, forward / data gradient, weight gradient) for precision = 2
G64_TABLE = [
    # EXCLUDED after measurement (profiles/sp64.txt): N = 64 — the benchmark network's 256 -> 64 and
    # 768 -> 64 layers among them.  One 64-wide tile column reads its A planes (6 bytes per element, float32 MFMA: 4) once
    # for 128 FLOPs per element: HBM-bound where float32 MFMA already runs (x1.03 / x0.92 / x0.98 of it at K = 256 / 768 /
    # 1024, inside the spread between rounds); the weight gradient with a quarter of its tile rows live: x0.55 .. x0.62.
    # The bare products (clx_gemm_planes / clx_wgrad_planes) keep N = 64.
    (dict(C=256, N=64, B=8, hw=(254, 254)), 0, 0),
    (dict(C=768, N=64, B=8, hw=(254, 254)), 0, 0),
    (dict(C=1024, N=64, B=8, hw=(254, 254)), 0, 0),
    (dict(C=192, N=64), 0, 0),
    (dict(C=192, N=64, D=16, hw=(16, 16)), 0, 0),
    (dict(C=256, N=128), 1, 1),                              # ... from N = 128 on
    (dict(C=320, N=320), 1, 1),
    (dict(C=192, N=192), 1, 1),                              # the 64 x 3 network
    (dict(C=192, N=256), 1, 1),
    (dict(C=256, N=192), 1, 1),
    (dict(C=576, N=576), 1, 1),
    (dict(C=256, N=256), 1, 1),                              # what precision = 1 covers stays covered
    (dict(C=64, N=128), 0, 0),                               # C < 128: a contraction of 64 (the chain64 pairs' ground)
    (dict(C=96, N=256), 0, 0),                               # C % 64
    (dict(C=256, N=96), 0, 0),                               # N % 64
    (dict(C=256, N=32), 0, 0),
    (dict(C=192, N=192, D=16, hw=(16, 16)), 1, 1),           # a 3-D 1x1 layer
    (dict(C=192, N=192, k=3, algo=2), 1, 1),                 # 2-D Winograd, F(4x4) and F(2x2)
    (dict(C=192, N=192, k=3, algo=1), 1, 1),
    (dict(C=576, N=192, k=3, algo=2), 1, 1),
    (dict(C=256, N=64, k=3, algo=2), 0, 0),                  # a 64-channel side: the contraction of one of the three products
    (dict(C=64, N=192, k=3, algo=2), 0, 0),
    (dict(C=192, N=192, k=3, algo=2, D=10), 0, 0),           # 3-D Winograd
    (dict(C=192, N=192, k=3, algo=3), 0, 0),                 # fused Winograd: float32 throughout
    (dict(C=192, N=192, crop=4), 0, 0),                      # cropped source
    (dict(C=192, N=192, factor=2), 0, 0),                    # upsampled source
    (dict(C=192, N=192, k=3), 0, 0),                         # 3x3, direct
    (dict(C=768, N=768, B=8, hw=(512, 512)), 1, 0),          # the weight gradient's planes would pass 4 GB
]


def test_sp_covers_by_the_64_channel_granule_for_precision_2_only():
    """clx_conv_sp_covers under precision = 2; the same descriptors under precision = 1 answer as they always have (the
    rule of the 128-wide tiles), under precision = 0 nothing is covered.  One shape class is excluded from the precision-2
    rule after measurement, N = 64: G64_TABLE gives the reason."""
    from cellulus_amd import _clx

    lib = _clx.load()
    for i, (kw, fwd, wgrad) in enumerate(G64_TABLE):
        d = _sp_desc(precision=2, **kw)
        assert _covers(lib, d) == (fwd, wgrad), (i, kw)
        d.wplanes = d.aplanes = d.dyplanes = None            # pointers are not part of the answer
        assert _covers(lib, d) == (fwd, wgrad), (i, kw)
        assert _covers(lib, _sp_desc(precision=0, **kw)) == (0, 0), (i, kw)
        assert _covers(lib, _sp_desc(precision=3, **kw)) == (0, 0), (i, kw)          # no such value
    # passes are judged one by one — a 128 -> 192 layer: forward, weight gradient and (the descriptor is 192 -> 128) data
    # gradient; a 64 -> 192 layer: none (contractions of 64; its data-gradient descriptor 192 -> 64 has N = 64)
    assert _covers(lib, _sp_desc(128, 192, precision=2)) == (1, 1) and _covers(lib, _sp_desc(192, 128, precision=2))[0] == 1
    assert _covers(lib, _sp_desc(64, 192, precision=2)) == (0, 0) and _covers(lib, _sp_desc(192, 64, precision=2))[0] == 0
    # precision = 1: today's answers on the same descriptors
    today = [
        (dict(C=256, N=64, B=8, hw=(254, 254)), 0, 0),
        (dict(C=768, N=64, B=8, hw=(254, 254)), 0, 0),
        (dict(C=192, N=192), 0, 0),
        (dict(C=192, N=256), 1, 0),
        (dict(C=256, N=192), 0, 0),
        (dict(C=256, N=256), 1, 1),
        (dict(C=192, N=192, D=16, hw=(16, 16)), 0, 0),
        (dict(C=192, N=192, k=3, algo=2), 0, 0),
        (dict(C=192, N=256, k=3, algo=2), 0, 0),
        (dict(C=576, N=192, k=3, algo=2), 0, 0),
        (dict(C=256, N=256, k=3, algo=2), 1, 1),
    ]
    for i, (kw, fwd, wgrad) in enumerate(today):
        assert _covers(lib, _sp_desc(precision=1, **kw)) == (fwd, wgrad), (i, kw)


def test_transform_caches_follow_the_rule():
    """clx_conv_vcache_bytes of a 192 -> 192 Winograd layer: P3 planes under precision = 2, float32 under 1 and 0.
    66 x 66 -> 64 x 64 outputs, 16 x 16 tiles of 4 x 4; the data gradient's (K - 1)-padded grid has 17 x 17."""
    from cellulus_amd import _clx

    lib = _clx.load()
    tiles, dy_tiles = 2 * 16 * 16, 2 * 17 * 17

    def vcache(d, which):
        return int(lib.clx_conv_vcache_bytes(ctypes.byref(d), which))

    d = _sp_desc(192, 192, hw=(66, 66), k=3, algo=2, precision=2)
    assert vcache(d, 0) == 36 * lib.clx_planes_bytes(tiles, 192)
    assert vcache(d, 1) == 36 * lib.clx_planes_bytes(dy_tiles, 192)
    d = _sp_desc(576, 192, hw=(66, 66), k=3, algo=2, precision=2)
    assert vcache(d, 0) == 36 * lib.clx_planes_bytes(tiles, 576)
    assert vcache(d, 1) == 36 * lib.clx_planes_bytes(dy_tiles, 192)
    for prec in (1, 0):
        d = _sp_desc(192, 192, hw=(66, 66), k=3, algo=2, precision=prec)
        assert vcache(d, 0) == 36 * tiles * 192 * 4
        assert vcache(d, 1) == 36 * dy_tiles * 192 * 4
    d = _sp_desc(256, 64, hw=(66, 66), k=3, algo=2, precision=2)                 # a 64-channel side: float32
    assert vcache(d, 0) == 36 * tiles * 256 * 4 and vcache(d, 1) == 36 * dy_tiles * 64 * 4
    # the workspace of a covered layer holds V as planes and the products' results in float32
    d = _sp_desc(192, 192, hw=(66, 66), k=3, algo=2, precision=2)
    assert int(lib.clx_conv_workspace_bytes(ctypes.byref(d), 0)) == 36 * (lib.clx_planes_bytes(tiles, 192) + tiles * 192 * 4)
    assert int(lib.clx_conv_workspace_bytes(ctypes.byref(d), 1)) == 36 * 2 * lib.clx_planes_bytes(tiles, 192)


def test_refusals_in_front_of_any_launch():
    """What the kernels do not cover is an argument error (fake pointers: a launch would fault): the bare products at
    N = 96 / 32, K = 64 / 48, weight-gradient C = 64 / 96 and N = 96; plane hand-overs on a precision-2 call the rule does
    not cover.  The covered forms pass the same checks: they are the GPU tests' ground."""
    from cellulus_amd import _clx

    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)
    for N, K in ((96, 128), (32, 128), (64, 64), (64, 48), (192, 64), (0, 128)):
        with pytest.raises(_clx.ClxError, match="clx_gemm_planes"):
            _clx.call("clx_gemm_planes", p, p, 64, N, K, null, 0, p, 256, null)
    # the message names the granule that holds now, and still the one of the whole 128-wide tiles (earlier tests look for it)
    with pytest.raises(_clx.ClxError, match="N % 64 == 0.*N % 128"):
        _clx.call("clx_gemm_planes", p, p, 64, 96, 128, null, 0, p, 96, null)
    with pytest.raises(_clx.ClxError, match="N % 64 == 0, C % 64 == 0 and C >= 128"):
        _clx.call("clx_wgrad_planes", p, p, 1000, 128, 64, p, 64, null)
    with pytest.raises(_clx.ClxError, match="ld_out"):
        _clx.call("clx_gemm_planes", p, p, 64, 64, 128, null, 0, p, 66, null)
    for N, C in ((128, 64), (128, 96), (96, 128), (64, 64), (32, 128)):
        with pytest.raises(_clx.ClxError, match="128"):
            _clx.call("clx_wgrad_planes", p, p, 1000, N, C, p, 256, null)
    # out_planes / out_colsum / aplanes_valid on precision-2 calls that do not take the split 1x1 product
    for d in (_sp_desc(64, 128, precision=2), _sp_desc(256, 96, precision=2), _sp_desc(192, 192, k=3, algo=2, precision=2),
              _sp_desc(192, 192, crop=4, precision=2), _sp_desc(256, 64, precision=2)):
        d.out_planes = 4096
        with pytest.raises(_clx.ClxError, match="out_planes"):
            _clx.call("clx_conv_fwd", ctypes.byref(d), null)
    d = _sp_desc(64, 192, precision=2)
    d.out_colsum = 4096
    with pytest.raises(_clx.ClxError, match="out_planes"):
        _clx.call("clx_conv_fwd", ctypes.byref(d), null)
    d = _sp_desc(192, 192, precision=2)
    d.aplanes_valid = 1
    d.wplanes = None                                         # (no weight planes: the float32 product)
    with pytest.raises(_clx.ClxError, match="aplanes_valid"):
        _clx.call("clx_conv_fwd", ctypes.byref(d), null)
    # the weight gradient: planes marked valid on a call that will not read them
    for d in (_sp_desc(64, 192, precision=2), _sp_desc(192, 96, precision=2), _sp_desc(192, 192, k=3, algo=2, precision=2),
              _sp_desc(320, 64, precision=2)):
        d.dyplanes_valid = 1
        with pytest.raises(_clx.ClxError, match="dyplanes_valid"):
            _clx.call("clx_conv_wgrad", ctypes.byref(d), ctypes.c_void_p(4096), 192, ctypes.c_void_p(4096), null, null)
    # ... which precision = 1 still refuses on a shape only the wider rule covers
    d = _sp_desc(192, 192, precision=1)
    d.dyplanes_valid = 1
    with pytest.raises(_clx.ClxError, match="dyplanes_valid"):
        _clx.call("clx_conv_wgrad", ctypes.byref(d), ctypes.c_void_p(4096), 192, ctypes.c_void_p(4096), null, null)
    d = _sp_desc(256, 64, precision=1)
    d.out_planes = 4096
    with pytest.raises(_clx.ClxError, match="out_planes"):
        _clx.call("clx_conv_fwd", ctypes.byref(d), null)


def test_python_switch(monkeypatch):
    from cellulus_amd.models import plan as P

    monkeypatch.delenv("CLX_DETERMINISTIC", raising=False)
    monkeypatch.delenv("CLX_PRECISION", raising=False)
    assert P.DEFAULT_PRECISION == "f32x3bf16" and P.precision_name() == "f32x3bf16" and P.precision_code() == 1
    for name, code in (("f32", 0), ("f32x3bf16", 1), ("f32x3bf16g64", 2)):
        monkeypatch.setenv("CLX_PRECISION", name)
        assert P.precision_name() == name and P.precision_code() == code
    for name in ("bf16", "f32x3bf16g32", "F32X3BF16G64", "2"):
        monkeypatch.setenv("CLX_PRECISION", name)
        with pytest.raises(ValueError):
            P.precision_name()
        with pytest.raises(ValueError):
            P.precision_code()
    monkeypatch.setenv("CLX_PRECISION", "f32x3bf16g64")
    monkeypatch.setenv("CLX_DETERMINISTIC", "1")
    assert P.precision_code() == 0
    # the enum value in the header is the one the Python layer hands over
    import os

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clx.h")).read()
    assert "CLX_PREC_F32X3BF16_G64 = 2" in hdr
