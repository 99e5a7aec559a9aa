"""CPU tier: the C ABI of clx_conv_first_dgrad (the input-image gradient of the first convolution).  Its arguments are
checked before any launch, so the refusals are testable without a HIP device."""

import ctypes

import pytest

from cellulus_amd import _build, _clx


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _clx.load()


def test_first_dgrad_is_exported_and_declared(lib):
    raw = ctypes.CDLL(_clx.LIB_PATH)
    assert hasattr(raw, "clx_conv_first_dgrad")
    assert "clx_conv_first_dgrad" in _clx.PROTOTYPES
    assert lib.clx_abi_version() == 13


P = ctypes.c_void_p(4096)          # aligned, never dereferenced: every call below is refused before a launch
NULL = ctypes.c_void_p(0)
# dy, ld_dy, w, N, cin, B, OD, OH, OW, KD, dx, stream
GOOD = [P, 8, P, 6, 1, 2, 5, 7, 9, 1, P, NULL]


@pytest.mark.parametrize("change, message", [
    ({4: 5}, "1 to 4 input channels"),
    ({4: 0}, "1 to 4 input channels"),
    ({9: 2}, "3x3 or 3x3x3"),
    ({1: 4}, "ld_dy >= N"),                       # ld_dy < N
    ({1: 10}, "ld_dy % 4 == 0"),
    ({3: 0}, "N >= 1"),
    ({0: NULL}, "null pointer"),
    ({2: NULL}, "null pointer"),
    ({10: NULL}, "null pointer"),
    ({0: ctypes.c_void_p(4100)}, "16-byte aligned"),
    ({10: ctypes.c_void_p(4098)}, "4-byte aligned"),
    ({5: 0}, "bad extents"),
    ({7: 0}, "bad extents"),
    ({6: -1}, "bad extents"),
])
def test_first_dgrad_refuses_bad_arguments(lib, change, message):
    args = list(GOOD)
    for i, v in change.items():
        args[i] = v
    assert lib.clx_conv_first_dgrad(*args) == -1
    assert message in lib.clx_last_error().decode()
    with pytest.raises(_clx.ClxError, match="clx_conv_first_dgrad"):
        _clx.call("clx_conv_first_dgrad", *args)
