"""The descriptor call's ABI without a GPU: the symbols and their declarations,
the struct's size, tsg_gemm_ex_check on one valid descriptor per in_mode and on
every error of the header's Errors paragraph, and the Python signatures."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_gpu_epilogue import error_mutations

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ternary_spgemm.h")
P = 0x1000  # a non-NULL pointer: tsg_gemm_ex_check never reads through one
N = 301


def _valid(tsg, in_mode=0):
    d = tsg.tsg_gemm_ex(in_mode=in_mode, act=tsg.TSG_ACT_RELU2, dX=P, xtype=tsg.TSG_X_BF16, ytype=tsg.TSG_Y_BF16,
                        dcol_scale=P, db=P, dalpha=P, dmul=P, ldmul=N + 5, multype=tsg.TSG_Y_F16, dadd=P, ldadd=N,
                        addtype=tsg.TSG_Y_F32, dY=P, ldY=N + 3)
    if in_mode == tsg.TSG_IN_PLAIN:
        d.drow_scale = P
    else:
        d.drow_scale_out = P
    if in_mode == tsg.TSG_IN_NORMQUANT:
        d.dgamma, d.eps = P, 1e-5
    return d


def test_symbols_are_exported_and_declared(tsg):
    L = tsg.lib()
    text = open(HEADER).read()
    for name in ("tcsc_hip_gemm_dev_ex", "tsg_gemm_ex_check"):
        assert name in tsg.EXPORTED_SYMBOLS
        assert getattr(L, name) is not None
        assert re.search(r"\bint %s\(" % name, text), name
    for word in ("typedef struct tsg_gemm_ex", "enum tsg_act", "enum tsg_in_mode", "TSG_ACT_RELU2 = 3",
                 "TSG_IN_NORMQUANT = 2", "SiLU", "ShardedTCSC"):
        assert word in text, word
    assert re.search(r"#define TSG_ABI_VERSION 2\b", text)
    assert (tsg.TSG_ACT_NONE, tsg.TSG_ACT_PRELU, tsg.TSG_ACT_RELU, tsg.TSG_ACT_RELU2) == (0, 1, 2, 3)
    assert (tsg.TSG_IN_PLAIN, tsg.TSG_IN_ACTQUANT, tsg.TSG_IN_NORMQUANT) == (0, 1, 2)


def test_struct_layout_is_the_headers(tsg):
    """The offsets the header spells out, and the size the library accepts."""
    text = open(HEADER).read()
    body = text[text.index("typedef struct tsg_gemm_ex {"):text.index("} tsg_gemm_ex;")]
    declared = [(m.group(2), int(m.group(3))) for m in
                re.finditer(r"^\s+([\w ]+?[ *])(\w+);\s+/\*\s+(\d+) ", body, re.M)]
    fields = [(n, getattr(tsg.tsg_gemm_ex, n).offset) for n, _ in tsg.tsg_gemm_ex._fields_]
    assert declared == fields, (declared, fields)
    assert C.sizeof(tsg.tsg_gemm_ex) == 144
    d = _valid(tsg)
    assert d.struct_size == 144 and tsg.lib().tsg_gemm_ex_check(C.byref(d), 16, N, 193) == tsg.TSG_OK
    for size in (143, 145, 136, 0):
        d.struct_size = size
        assert tsg.lib().tsg_gemm_ex_check(C.byref(d), 16, N, 193) == 1
        assert b"struct_size" in tsg.lib().tcsc_hip_last_error()


def test_null_handle_and_null_descriptor(tsg):
    """TSG_ERR_ARG before anything is read: the pointers of the descriptor are not mapped."""
    L = tsg.lib()
    d = _valid(tsg)
    assert L.tcsc_hip_gemm_dev_ex(None, C.byref(d), 16, N, 193, None) == 1
    assert b"null handle" in L.tcsc_hip_last_error()
    assert L.tcsc_hip_gemm_dev_ex(None, None, 16, N, 193, None) == 1
    assert L.tsg_gemm_ex_check(None, 16, N, 193) == 1
    assert b"null descriptor" in L.tcsc_hip_last_error()
    with pytest.raises(tsg.TSGError) as e:
        tsg.gemm_ex_check(None, 16, N, 193)
    assert e.value.code == 1


@pytest.mark.parametrize("in_mode", [0, 1, 2])
def test_a_valid_descriptor_per_in_mode(tsg, in_mode):
    tsg.gemm_ex_check(_valid(tsg, in_mode), 16, N, 193)
    d = _valid(tsg, in_mode)
    d.dmul = d.dadd = None  # no operands: their ld and type are not looked at beyond the enum
    d.ldmul = d.ldadd = 0
    d.act = tsg.TSG_ACT_NONE
    d.dalpha = None
    tsg.gemm_ex_check(d, 16, N, 193)
    d.dalpha = P  # read for PRELU only, ignored otherwise
    tsg.gemm_ex_check(d, 16, N, 193)


MUTATIONS = error_mutations(N)


@pytest.mark.parametrize("i", range(len(MUTATIONS)), ids=lambda i: f"{i}-{MUTATIONS[i][0]}")
def test_every_error_names_its_field(tsg, i):
    field, mutate = MUTATIONS[i]
    d = _valid(tsg)
    d.drow_scale = None  # (the mutations start from a PLAIN descriptor without a row scale)
    tsg.gemm_ex_check(d, 16, N, 193)
    mutate(d)
    L = tsg.lib()
    assert L.tsg_gemm_ex_check(C.byref(d), 16, N, 193) == 1, field
    msg = L.tcsc_hip_last_error().decode()
    assert field in msg, (field, msg)
    with pytest.raises(tsg.TSGError, match=field) as e:
        tsg.gemm_ex_check(d, 16, N, 193)
    assert e.value.code == 1


def test_python_signatures(tsg):
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(tsg.TCSCDevice.gemm_dev_ex) == [("self", E), ("desc", E), ("M", E), ("stream", 0)]
    assert params(tsg.TCSCDevice.gemm_torch_ex) == [
        ("self", E), ("X", E), ("b", E), ("Y", None), ("act", "none"), ("alpha", None), ("mul", None), ("add", None),
        ("out_dtype", None), ("row_scale", None), ("col_scale", None), ("quant", None), ("gamma", None), ("eps", None),
        ("row_scale_out", None)]
    assert params(tsg.epilogue_ref) == [("y32", E), ("act", E), ("alpha", None), ("mul", None), ("add", None)]
    assert params(tsg.gemm_ex_check) == [("desc", E), ("M", E), ("N", E), ("K", E)]
    assert issubclass(tsg.tsg_gemm_ex, C.Structure)
