"""The narrow-Y entry points (include/ternary_spgemm.h, tcsc_hip_gemm_dev_xy /
tcsc_hip_gemm_prelu_dev_xy) without a GPU: the library exports them, a null
handle is an argument error for every ytype and touches no buffer, the header
declares enum tsg_ytype with its three values, mirrored by the Python
constants, and the ABI version is still 2 (the change is additive)."""
import ctypes as C
import re

import pytest

NAMES = ("tcsc_hip_gemm_dev_xy", "tcsc_hip_gemm_prelu_dev_xy")


def _header(tsg):
    return open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


@pytest.mark.parametrize("name", NAMES)
def test_xy_symbols_exported(tsg, name):
    assert name in tsg.EXPORTED_SYMBOLS
    assert hasattr(tsg.lib(), name)
    assert f"int {name}(" in _header(tsg)


def test_header_declares_the_ytype_enum(tsg):
    m = re.search(r"enum\s+tsg_ytype\s*\{([^}]*)\}", _header(tsg))
    assert m, "enum tsg_ytype is not declared"
    values = {k: int(v) for k, v in re.findall(r"(TSG_Y_\w+)\s*=\s*(\d+)", m.group(1))}
    assert values == {"TSG_Y_F32": 0, "TSG_Y_F16": 1, "TSG_Y_BF16": 2}
    assert (tsg.TSG_Y_F32, tsg.TSG_Y_F16, tsg.TSG_Y_BF16) == (0, 1, 2)


def test_abi_version_is_still_2(tsg):
    assert "#define TSG_ABI_VERSION 2" in _header(tsg)


@pytest.mark.parametrize("ytype", [0, 1, 2, 3, -1])
def test_xy_null_handle_is_an_argument_error(tsg, ytype):
    L = tsg.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert L.tcsc_hip_gemm_dev_xy(None, p, 0, p, p, ytype, 4, 1, 4, 4, None) == 1  # TSG_ERR_ARG
    assert b"null handle" in L.tcsc_hip_last_error()
    assert L.tcsc_hip_gemm_prelu_dev_xy(None, p, 0, p, p, p, ytype, 4, 1, 4, 4, None) == 1
    assert b"null handle" in L.tcsc_hip_last_error()
    assert all(v == 0.0 for v in buf)
