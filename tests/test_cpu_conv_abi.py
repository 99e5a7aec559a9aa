"""CPU tier: the descriptor checks of clx_conv_fwd and clx_conv_wgrad.  Both entry points validate the geometry of a
clx_conv_desc with one function before any dispatch, so a descriptor the forward pass refuses is refused by the weight
gradient with the same words — whatever kernel family (small-channel, grey-scale, implicit GEMM) it would have reached.

Every call below must be refused BEFORE a launch: the pointers are placeholders (aligned, never dereferenced), so the
return code is -1 (CLX_ERR_ARG), never -2 (CLX_ERR_LAUNCH: a launch was attempted), and no call may end the process
(the weight-gradient grid of an input smaller than its kernel was once sized with a division by zero)."""

import ctypes

import pytest

from cellulus_amd import _build, _clx
from cellulus_amd._clx import ClxConvDesc


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _clx.load()


P = 4096                            # aligned, never dereferenced
NULL = ctypes.c_void_p(0)
LD_DY = 8

# (channels of the source, c_real): the grey-scale and the generic small-channel route, the implicit-GEMM route
ROUTES = [(4, 1), (4, 3), (32, 0)]
ROUTE_IDS = ["c4_grey", "c4_generic", "c32_igemm"]


def _good(C, c_real):
    """A 2-D valid 3x3 layer over a (10, 10) image that both entry points would accept (never called as it stands)."""
    d = ClxConvDesc()
    d.nsrc = 1
    s = d.src[0]
    s.ptr, s.C, s.ld = P, C, C
    s.D, s.H, s.W = 1, 10, 10
    s.oz = s.oy = s.ox = 0
    s.fz = s.fy = s.fx = 1
    d.B = 2
    d.ID, d.IH, d.IW = 1, 10, 10
    d.KD, d.KH, d.KW = 1, 3, 3
    d.PD = d.PH = d.PW = 0
    d.N = 8
    d.wpack, d.out, d.ld_out = P, P, 8
    d.c_real = c_real
    return d


def _set(d, change):
    for name, v in change.items():
        if name.startswith("src."):
            setattr(d.src[0], name[4:], v)
        else:
            setattr(d, name, v)
    return d


def _fwd(lib, d):
    rc = lib.clx_conv_fwd(ctypes.byref(d), NULL)
    return rc, lib.clx_last_error().decode()


def _wgrad(lib, d, dy=P, ld_dy=LD_DY, dwp=P, db=P):
    rc = lib.clx_conv_wgrad(ctypes.byref(d), ctypes.c_void_p(dy), ld_dy, ctypes.c_void_p(dwp), ctypes.c_void_p(db), NULL)
    return rc, lib.clx_last_error().decode()


GEOMETRY = [
    ({"src.W": 6}, "source 0 smaller than the logical input"),          # stored grid narrower than the logical input
    ({"src.ox": 3}, "source 0 smaller than the logical input"),         # the crop pushes the window out of the source
    ({"PW": 3}, "padding must be < kernel extent"),
    ({"KW": 4}, "kernel extent must be 1, 2 or 3"),
    ({"B": 0}, "bad extent"),
    ({"IW": 2}, "input smaller than kernel"),                           # (the weight gradient once died here: SIGFPE)
    ({"src.H": 9}, "source 0 smaller than the logical input"),
    ({"src.oy": -1}, "negative crop"),
    ({"src.fx": 0}, "upsample factors >= 1"),
    ({"src.ld": 2}, "source channels/ld must be multiples of 4"),
    ({"src.ptr": P + 4}, "source pointer must be 16-byte aligned"),
    ({"src.ptr": 0}, "null source 0"),
    ({"nsrc": 3}, "nsrc must be 1 or 2"),
    ({"KH": 0}, "kernel extent must be 1, 2 or 3"),
    ({"PH": -1}, "padding must be < kernel extent"),
    ({"ID": 0}, "bad extent"),
    ({"B": 1 << 24, "src.H": 1 << 12, "IH": 1 << 12}, "too many output pixels"),     # M = 2^24 * 4094 * 8 >= 2^31
]
GEOMETRY_IDS = ["narrow_source", "crop_outside", "pad_ge_kernel", "kernel_4", "batch_0", "input_lt_kernel", "short_source",
                "negative_crop", "factor_0", "ld_lt_c", "misaligned_source", "null_source", "nsrc_3", "kernel_0",
                "negative_pad", "depth_0", "too_many_pixels"]


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("change, message", GEOMETRY, ids=GEOMETRY_IDS)
def test_both_entry_points_refuse_bad_geometry_alike(lib, route, change, message):
    d = _set(_good(*route), change)
    rc_f, msg_f = _fwd(lib, d)
    rc_w, msg_w = _wgrad(lib, d)
    assert rc_f == -1, (rc_f, msg_f)
    assert rc_w == -1, (rc_w, msg_w)                # -2 would mean that a launch was attempted
    assert msg_f.startswith("clx_conv_fwd: ") and msg_w.startswith("clx_conv_wgrad: "), (msg_f, msg_w)
    assert message in msg_f
    assert msg_f[len("clx_conv_fwd: "):] == msg_w[len("clx_conv_wgrad: "):]
    with pytest.raises(_clx.ClxError, match="clx_conv_fwd"):
        _clx.call("clx_conv_fwd", ctypes.byref(d), NULL)
    with pytest.raises(_clx.ClxError, match="clx_conv_wgrad"):
        _clx.call("clx_conv_wgrad", ctypes.byref(d), ctypes.c_void_p(P), LD_DY, ctypes.c_void_p(P), ctypes.c_void_p(P), NULL)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("algo", [1, 2])
def test_wgrad_checks_geometry_for_every_algo(lib, route, algo):
    """the Winograd weight gradients sit behind the same checks"""
    d = _set(_good(*route), {"algo": algo, "IW": 2})
    rc, msg = _wgrad(lib, d)
    assert rc == -1 and "input smaller than kernel" in msg, (rc, msg)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("change, message", [
    ({"ld_out": 4}, "bad N/ld_out"),                                     # ld_out < N
    ({"N": 0}, "bad N/ld_out"),
    ({"ld_out": 10}, "out must be 16-byte aligned with ld_out % 4 == 0"),
    ({"out": P + 4}, "out must be 16-byte aligned with ld_out % 4 == 0"),
    ({"wpack": P + 8}, "wpack must be 16-byte aligned"),
    ({"wpack": 0}, "null wpack/out"),
    ({"out": 0}, "null wpack/out"),
    ({"gate_out": P, "ld_gate": 1, "ld_out": 32}, "gate_out needs relu"),            # relu = 0
    ({"gate_out": P, "ld_gate": 1, "relu": 1}, "gate_out needs relu, ld_out % 32 == 0"),     # ld_out = 8
    ({"mask_bits": P, "ld_mask_bits": 1, "mask": P, "ld_mask": 8}, "mask_bits replaces mask"),
    ({"mask": P + 4, "ld_mask": 8}, "mask must be 16-byte aligned"),
    ({"pool_out": P, "ld_pool": 8}, "need a Winograd algorithm"),
    ({"tile_list": P, "tile_count": 1}, "need a Winograd algorithm"),
    ({"adjoint": 1}, "need a Winograd algorithm"),
    ({"algo": 7}, "bad algo"),
], ids=["ld_out_lt_n", "n_0", "ld_out_mod_4", "misaligned_out", "misaligned_wpack", "null_wpack", "null_out",
        "gate_out_no_relu", "gate_out_ld_out", "mask_bits_and_mask", "misaligned_mask", "pool_out_direct",
        "tile_list_direct", "adjoint_direct", "bad_algo"])
def test_forward_only_refusals(lib, route, change, message):
    d = _set(_good(*route), change)
    rc, msg = _fwd(lib, d)
    assert rc == -1, (rc, msg)
    assert msg.startswith("clx_conv_fwd: ") and message in msg, msg
    with pytest.raises(_clx.ClxError, match="clx_conv_fwd"):
        _clx.call("clx_conv_fwd", ctypes.byref(d), NULL)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("change, args, message", [
    ({"N": 6}, {}, "N and ld_dy must be multiples of 4 (N=6 ld_dy=8)"),
    ({}, {"ld_dy": 4}, "N and ld_dy must be multiples of 4 (N=8 ld_dy=4)"),       # ld_dy < N
    ({}, {"ld_dy": 10}, "N and ld_dy must be multiples of 4 (N=8 ld_dy=10)"),
    ({}, {"dy": P + 4}, "dy must be 16-byte aligned"),
    ({}, {"dy": 0}, "null pointer"),
    ({}, {"dwp": 0}, "null pointer"),
    ({"algo": 3}, {}, "bad algo"),                                                   # the fused form has no weight gradient
    ({"aplanes_valid": 1}, {}, "aplanes_valid / dyplanes_valid"),
], ids=["n_mod_4", "ld_dy_lt_n", "ld_dy_mod_4", "misaligned_dy", "null_dy", "null_dwpack", "bad_algo", "stale_planes"])
def test_wgrad_only_refusals(lib, route, change, args, message):
    d = _set(_good(*route), change)
    rc, msg = _wgrad(lib, d, **args)
    assert rc == -1, (rc, msg)
    assert msg.startswith("clx_conv_wgrad: ") and message in msg, msg
    a = dict(dy=P, ld_dy=LD_DY, dwp=P)
    a.update(args)
    with pytest.raises(_clx.ClxError, match="clx_conv_wgrad"):
        _clx.call("clx_conv_wgrad", ctypes.byref(d), ctypes.c_void_p(a["dy"]), a["ld_dy"], ctypes.c_void_p(a["dwp"]),
                  ctypes.c_void_p(P), NULL)


def test_null_descriptor(lib):
    assert lib.clx_conv_fwd(None, NULL) == -1
    assert "null descriptor" in lib.clx_last_error().decode()
    assert lib.clx_conv_wgrad(None, ctypes.c_void_p(P), LD_DY, ctypes.c_void_p(P), NULL, NULL) == -1
    assert "null pointer" in lib.clx_last_error().decode()
    assert lib.clx_abi_version() == 13
