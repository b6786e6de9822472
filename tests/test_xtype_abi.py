"""The narrow-X entry points (include/ternary_spgemm.h, tcsc_hip_gemm_dev_x /
tcsc_hip_gemm_prelu_dev_x) without a GPU: the library exports them, a null
handle is an argument error, not a crash, the header declares enum tsg_xtype
with its four values, and the ABI version is still 2 (the change is additive)."""
import ctypes as C
import re

import pytest

NAMES = ("tcsc_hip_gemm_dev_x", "tcsc_hip_gemm_prelu_dev_x")


def _header(tsg):
    return open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


@pytest.mark.parametrize("name", NAMES)
def test_x_symbols_exported(tsg, name):
    assert name in tsg.EXPORTED_SYMBOLS
    assert hasattr(tsg.lib(), name)
    assert f"int {name}(" in _header(tsg)


def test_header_declares_the_xtype_enum(tsg):
    m = re.search(r"enum\s+tsg_xtype\s*\{([^}]*)\}", _header(tsg))
    assert m, "enum tsg_xtype is not declared"
    values = {k: int(v) for k, v in re.findall(r"(TSG_X_\w+)\s*=\s*(\d+)", m.group(1))}
    assert values == {"TSG_X_F32": 0, "TSG_X_F16": 1, "TSG_X_BF16": 2, "TSG_X_I8": 3}
    assert (tsg.TSG_X_F32, tsg.TSG_X_F16, tsg.TSG_X_BF16, tsg.TSG_X_I8) == (0, 1, 2, 3)


def test_abi_version_is_still_2(tsg):
    assert "#define TSG_ABI_VERSION 2" in _header(tsg)


@pytest.mark.parametrize("xtype", [0, 1, 2, 3, 4, -1])
def test_x_null_handle_is_an_argument_error(tsg, xtype):
    L = tsg.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert L.tcsc_hip_gemm_dev_x(None, p, xtype, p, p, 4, 1, 4, 4, None) == 1  # TSG_ERR_ARG
    assert b"null handle" in L.tcsc_hip_last_error()
    assert L.tcsc_hip_gemm_prelu_dev_x(None, p, xtype, p, p, p, 4, 1, 4, 4, None) == 1
    assert b"null handle" in L.tcsc_hip_last_error()
    assert all(v == 0.0 for v in buf)
