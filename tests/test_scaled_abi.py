"""The scaled entry points (include/ternary_spgemm.h, tcsc_hip_gemm_dev_scaled /
tcsc_hip_gemm_prelu_dev_scaled) without a GPU: the library exports them and the
header declares them, a null handle is an argument error that touches no
buffer, the ABI version is still 2 (the change is additive), and the Python
wrappers exist with the documented signatures."""
import ctypes as C
import inspect

import pytest

NAMES = ("tcsc_hip_gemm_dev_scaled", "tcsc_hip_gemm_prelu_dev_scaled")


def _header(tsg):
    return open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


@pytest.mark.parametrize("name", NAMES)
def test_scaled_symbols_exported(tsg, name):
    assert name in tsg.EXPORTED_SYMBOLS
    assert hasattr(tsg.lib(), name)
    assert f"int {name}(" in _header(tsg)


def test_abi_version_is_still_2(tsg):
    assert "#define TSG_ABI_VERSION 2" in _header(tsg)


@pytest.mark.parametrize("scales", ["both", "row", "col", "none"])
def test_scaled_null_handle_is_an_argument_error(tsg, scales):
    L = tsg.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    rs = p if scales in ("both", "row") else None
    cs = p if scales in ("both", "col") else None
    for ytype in (0, 1, 2, 3, -1):
        assert L.tcsc_hip_gemm_dev_scaled(None, p, 0, rs, cs, p, p, ytype, 4, 1, 4, 4, None) == 1  # TSG_ERR_ARG
        assert b"null handle" in L.tcsc_hip_last_error()
        assert L.tcsc_hip_gemm_prelu_dev_scaled(None, p, 0, rs, cs, p, p, p, ytype, 4, 1, 4, 4, None) == 1
        assert b"null handle" in L.tcsc_hip_last_error()
    assert all(v == 0.0 for v in buf)


def test_python_wrappers_have_the_documented_signatures(tsg):
    dev = inspect.signature(tsg.TCSCDevice.gemm_dev_scaled)
    assert list(dev.parameters) == ["self", "dX", "xtype", "db", "dY", "ytype", "M", "stream", "dalpha", "ldY",
                                    "drow_scale", "dcol_scale"]
    assert dev.parameters["stream"].default == 0
    assert all(dev.parameters[k].default is None for k in ("dalpha", "ldY", "drow_scale", "dcol_scale"))
    tor = inspect.signature(tsg.TCSCDevice.gemm_torch_scaled)
    assert list(tor.parameters) == ["self", "X", "b", "Y", "alpha", "out_dtype", "row_scale", "col_scale"]
    assert all(tor.parameters[k].default is None for k in ("Y", "alpha", "out_dtype", "row_scale", "col_scale"))


def test_sharded_forward_takes_the_scales(tsg):
    import tsg_dist
    for fn in (tsg_dist.ShardedTCSC.forward, tsg_dist.ShardedTCSC.forward_into):
        p = inspect.signature(fn).parameters
        assert p["row_scale"].default is None and p["col_scale_full"].default is None
