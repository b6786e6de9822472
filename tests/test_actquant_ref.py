"""The actquant entry points (include/ternary_spgemm.h, tcsc_hip_gemm_dev_actquant
/ tcsc_hip_gemm_prelu_dev_actquant) without a GPU: tspgemm.act_quant_ref is the
torch-CPU formula of the contract, the input conditions of the GPU file's case
builder (test_gpu_actquant's module docstring) hold on every shape it uses, the
library exports the symbols and the header declares them, a null handle is an
argument error that touches no buffer, the ABI version is still 2 and the
Python wrappers have the documented signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest

import test_gpu_actquant as G

NAMES = ("tcsc_hip_gemm_dev_actquant", "tcsc_hip_gemm_prelu_dev_actquant")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The case builder imports the oracle itself: it is built first."""


def _torch_formula(Xw):
    import torch
    x = torch.from_numpy(np.array(Xw))
    a = x.abs().amax(dim=1, keepdim=True).clamp_min(1e-5)
    # (a tensor over a tensor: torch evaluates `127.0 / a` as a.reciprocal() *
    # 127.0, two roundings -- one of the variants the near-ties tell apart)
    inv = torch.full_like(a, 127.0) / a
    q = torch.round(x * inv).clamp(-127.0, 127.0)
    assert a.dtype == inv.dtype == q.dtype == torch.float32
    return q.to(torch.int8).numpy(), (a / 127.0).reshape(-1).numpy()


# every (M, K) the GPU file builds an X for: fp32 on all of them, the 16-bit types on the type shapes
TYPE_SHAPES = G.TYPE_SHAPES + [(16, 388, 301), (130, 388, 700), (130, 193, 301)]
X_CASES = sorted({(M, K, "float32") for M, K, N, B in G.FAMILY_SHAPES} |
                 {(M, K, x) for M, K, N in TYPE_SHAPES for x in G.XDTYPES})


@pytest.mark.parametrize("M,K,xdtype", X_CASES)
def test_act_quant_ref_is_the_torch_formula(tsg, M, K, xdtype):
    """amax, clamp_min(1e-5), 127 / a, round (half to even), clamp -- on the
    near-tie X of every shape, and on a Gaussian one."""
    Xt, Xw, q, deq, tie_rows = G._xq(M, K, xdtype)
    for X in (Xw, np.random.default_rng(M + K).standard_normal((M, K)).astype(np.float32)):
        q1, d1 = tsg.act_quant_ref(X)
        q2, d2 = _torch_formula(X)
        assert q1.dtype == np.int8 and d1.dtype == np.float32 and q1.shape == X.shape and d1.shape == (M,)
        assert np.array_equal(q1, q2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal(q, tsg.act_quant_ref(Xw)[0])


def test_act_quant_ref_edge_cases(tsg):
    q, d = tsg.act_quant_ref(np.zeros((3, 0), np.float32))
    assert q.shape == (3, 0) and np.array_equal(d, np.full(3, np.float32(1e-5) / np.float32(127.0), np.float32))
    X = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 127.0, -0.0]], np.float32)  # inv = 1: ties go to even
    q, d = tsg.act_quant_ref(X)
    assert q.tolist() == [[0, 2, 2, 0, -2, -2, 127, 0]] and d[0] == np.float32(1.0)
    with pytest.raises(tsg.TSGError):
        tsg.act_quant_ref(np.zeros((2, 2), np.float64))


def test_a_gaussian_x_cannot_tell_the_variants_apart(tsg):
    """Why the builder makes near-ties: on a random X every wrong neighbour of
    the contract gives (almost) the contract's q."""
    X = np.random.default_rng(0).standard_normal((130, 388)).astype(np.float32)
    q, _ = tsg.act_quant_ref(X)
    for name, v in G.variants(X).items():
        assert float(np.mean(v != q)) < 0.001, name


@pytest.mark.parametrize("M,K,N,B", G.FAMILY_SHAPES)
def test_builder_conditions_hold_on_the_family_shapes(tsg, M, K, N, B):
    """_acase asserts them: each variant told apart (>= 3 % on an fp32 X, half
    away >= 30 % on the exact-tie rows), the row maximum exactly a[m], a
    finite expected Y."""
    arrays, Xt, Xw, b, alpha, cs, deq, want = G._acase(M, K, N, "float32", "float32", B)
    assert Xw.shape == (M, K) and deq.shape == (M,) and len(want) == 4
    assert all(w.shape == (M, N) for w in want.values())


@pytest.mark.parametrize("ydtype", G.YDTYPES)
@pytest.mark.parametrize("xdtype", G.XDTYPES)
@pytest.mark.parametrize("M,K,N", TYPE_SHAPES)
def test_builder_conditions_hold_on_the_type_shapes(tsg, M, K, N, xdtype, ydtype):
    """The type product's cases, the misaligned-X cases and the capture cases."""
    arrays, Xt, Xw, b, alpha, cs, deq, want = G._acase(M, K, N, xdtype, ydtype)
    assert str(Xt.dtype) == "torch." + xdtype and want[(True, "plain")].dtype == (
        np.uint32 if ydtype == "float32" else np.uint16)


@pytest.mark.parametrize("name", NAMES)
def test_actquant_symbols_exported(tsg, name):
    assert name in tsg.EXPORTED_SYMBOLS
    assert hasattr(tsg.lib(), name)
    assert f"int {name}(" in open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()
    assert "act_quant_ref" in dir(tsg)


def test_abi_version_is_still_2(tsg):
    assert "#define TSG_ABI_VERSION 2" in open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


@pytest.mark.parametrize("out", ["scale out", "none"])
def test_actquant_null_handle_is_an_argument_error(tsg, out):
    L = tsg.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    rs = p if out == "scale out" else None
    for xtype in (0, 1, 2, 3, 4, -1):
        for ytype in (0, 1, 2, 3, -1):
            assert L.tcsc_hip_gemm_dev_actquant(None, p, xtype, rs, p, p, p, ytype, 4, 1, 4, 4, None) == 1  # TSG_ERR_ARG
            assert b"null handle" in L.tcsc_hip_last_error()
            assert L.tcsc_hip_gemm_prelu_dev_actquant(None, p, xtype, rs, p, p, p, p, ytype, 4, 1, 4, 4, None) == 1
            assert b"null handle" in L.tcsc_hip_last_error()
    assert all(v == 0.0 for v in buf)


def test_python_wrappers_have_the_documented_signatures(tsg):
    dev = inspect.signature(tsg.TCSCDevice.gemm_dev_actquant)
    assert list(dev.parameters) == ["self", "dX", "xtype", "db", "dY", "ytype", "M", "stream", "dalpha", "ldY",
                                    "drow_scale_out", "dcol_scale"]
    assert dev.parameters["stream"].default == 0
    assert all(dev.parameters[k].default is None for k in ("dalpha", "ldY", "drow_scale_out", "dcol_scale"))
    tor = inspect.signature(tsg.TCSCDevice.gemm_torch_actquant)
    assert list(tor.parameters) == ["self", "X", "b", "Y", "alpha", "out_dtype", "col_scale", "row_scale_out"]
    assert all(tor.parameters[k].default is None for k in ("Y", "alpha", "out_dtype", "col_scale", "row_scale_out"))
    assert list(inspect.signature(tsg.act_quant_ref).parameters) == ["Xw"]
