"""The fused gate/up call's ABI without a GPU: the three entry points are
exported and declared, and tsg_gemm_glu_check accepts a valid descriptor and
refuses every handle-free error of the header with a message naming the field:
the descriptor call's own errors, a NULL db_up, and activations that are not int8."""
import ctypes as C
import re

import pytest

from test_epilogue_abi import HEADER, N, P
from test_gpu_epilogue import error_mutations


def _valid(tsg, in_mode=0):
    d = tsg.tsg_gemm_ex(in_mode=in_mode, act=tsg.TSG_ACT_RELU2, dX=P, ytype=tsg.TSG_Y_BF16, dcol_scale=P, db=P,
                        dalpha=P, dmul=P, ldmul=N + 5, multype=tsg.TSG_Y_F16, dadd=P, ldadd=N, addtype=tsg.TSG_Y_F32,
                        dY=P, ldY=N + 3)
    d.xtype = tsg.TSG_X_I8 if in_mode == tsg.TSG_IN_PLAIN else tsg.TSG_X_BF16
    if in_mode != tsg.TSG_IN_PLAIN:
        d.drow_scale_out = P
    if in_mode == tsg.TSG_IN_NORMQUANT:
        d.dgamma, d.eps = P, 1e-5
    return d


def test_symbols_are_exported_and_declared(tsg):
    text = open(HEADER).read()
    for name in ("tcsc_hip_gemm_dev_glu", "tsg_gemm_glu_check", "tcsc_hip_reserve_glu"):
        assert name in tsg.EXPORTED_SYMBOLS
        assert getattr(tsg.lib(), name) is not None
        assert re.search(r"\bint %s\(" % name, text), name


@pytest.mark.parametrize("in_mode", [0, 1, 2])
def test_a_valid_descriptor_per_in_mode(tsg, in_mode):
    tsg.gemm_glu_check(_valid(tsg, in_mode), P, 16, N, 193)
    d = _valid(tsg, in_mode)
    d.dmul = d.dadd = d.dcol_scale = None  # u alone multiplies
    tsg.gemm_glu_check(d, P, 16, N, 193)


# (field, mutation, db_up, the xtype of the valid PLAIN descriptor it starts from): the descriptor call's
# own errors from its bf16 descriptor -- tsg_gemm_ex_check's refusal comes first -- then this call's from int8
MUTATIONS = [(field, m, P, 2) for field, m in error_mutations(N)] + [
    ("db_up", lambda d: None, None, 3),
    ("xtype", lambda d: setattr(d, "xtype", 0), P, 3), ("xtype", lambda d: setattr(d, "xtype", 1), P, 3),
    ("xtype", lambda d: setattr(d, "xtype", 2), P, 3),
]


@pytest.mark.parametrize("i", range(len(MUTATIONS)), ids=lambda i: f"{i}-{MUTATIONS[i][0]}")
def test_every_error_names_its_field(tsg, i):
    field, mutate, db_up, xtype = MUTATIONS[i]
    d = _valid(tsg)
    tsg.gemm_glu_check(d, P, 16, N, 193)
    d.xtype = xtype
    tsg.gemm_ex_check(d, 16, N, 193)
    mutate(d)
    L = tsg.lib()
    assert L.tsg_gemm_glu_check(C.byref(d), db_up, 16, N, 193) == 1, field
    msg = L.tcsc_hip_last_error().decode()
    assert field in msg, (field, msg)
    with pytest.raises(tsg.TSGError, match=field) as e:
        tsg.gemm_glu_check(d, db_up, 16, N, 193)
    assert e.value.code == 1


def test_null_handles_and_pick(tsg):
    """A NULL handle is named before the descriptor is read; the split-K choice is host arithmetic."""
    L = tsg.lib()
    d = _valid(tsg)
    assert L.tcsc_hip_gemm_dev_glu(None, None, C.byref(d), P, None, 16, N, 193, None) == 1
    assert b"h_gate" in L.tcsc_hip_last_error()
    assert L.tcsc_hip_reserve_glu(None, None, 16) == 1
    assert [tsg.i8glu_pick(K, N) for K in (0, 1, 64, 65, 200, 512, 576, 131072)] == \
        [(32, S) for S in (1, 1, 1, 2, 4, 8, 8, 8)]
