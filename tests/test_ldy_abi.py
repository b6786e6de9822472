"""The output-row-stride entry points (include/ternary_spgemm.h,
tcsc_hip_gemm_dev_ld / tcsc_hip_gemm_prelu_dev_ld) without a GPU: the library
exports them, and a null handle is an argument error, not a crash."""
import ctypes as C

import pytest

NAMES = ("tcsc_hip_gemm_dev_ld", "tcsc_hip_gemm_prelu_dev_ld")


@pytest.mark.parametrize("name", NAMES)
def test_ld_symbols_exported(tsg, name):
    assert name in tsg.EXPORTED_SYMBOLS
    assert hasattr(tsg.lib(), name)
    assert f"int {name}(" in open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


def test_abi_version_is_2(tsg):
    assert "#define TSG_ABI_VERSION 2" in open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


def test_ld_null_handle_is_an_argument_error(tsg):
    L = tsg.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert L.tcsc_hip_gemm_dev_ld(None, p, p, p, 4, 1, 4, 4, None) == 1  # TSG_ERR_ARG
    assert b"null handle" in L.tcsc_hip_last_error()
    assert L.tcsc_hip_gemm_prelu_dev_ld(None, p, p, p, p, 4, 1, 4, 4, None) == 1
    assert b"null handle" in L.tcsc_hip_last_error()
    assert all(v == 0.0 for v in buf)
