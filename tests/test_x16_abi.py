"""The 16-bit matrix-core setting's two entry points (tcsc_hip_set_x16_mfma,
tcsc_hip_call_x16_mfma) without a GPU: listed, exported, declared, and a null
handle is TSG_ERR_ARG from both."""
import ctypes
import os
import re

NAMES = ("tcsc_hip_set_x16_mfma", "tcsc_hip_call_x16_mfma")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ternary_spgemm.h")


def test_names_and_null_handle(tsg):
    header = open(HEADER).read()
    L = ctypes.CDLL(tsg.LIB_PATH)
    for name in NAMES:
        assert name in tsg.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert L.tcsc_hip_set_x16_mfma(None, 1) == 1  # TSG_ERR_ARG
    assert L.tcsc_hip_call_x16_mfma(None, 64, tsg.TSG_X_BF16) == 1
