"""The normquant entry points (include/ternary_spgemm.h, tcsc_hip_gemm_dev_normquant
/ tcsc_hip_gemm_prelu_dev_normquant) without a GPU: tspgemm.rms_norm_ref is a
plain per-row loop of the contract, its edge cases, the input conditions of the
GPU file's case builder (test_gpu_normquant's module docstring) hold on every
shape it uses, the library exports the symbols and the header declares them, a
null handle is an argument error that touches no buffer, the ABI version is
still 2 and the Python wrappers have the documented signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest

import test_gpu_normquant as G

NAMES = ("tcsc_hip_gemm_dev_normquant", "tcsc_hip_gemm_prelu_dev_normquant")
F = np.float32


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The case builder imports the oracle itself: it is built first."""


def _loop(Xw, gamma, eps):
    """The contract, one row and one operation at a time."""
    M, K = Xw.shape
    xn, rn = np.zeros((M, K), F), np.zeros(M, F)
    for m in range(M):
        s = [F(0.0)] * 256
        for k in range(K):
            sq = F(Xw[m, k] * Xw[m, k])
            s[k % 256] = F(s[k % 256] + sq)
        while len(s) > 1:
            s = [F(s[2 * p] + s[2 * p + 1]) for p in range(len(s) // 2)]
        ms = F(s[0] / F(K))
        rn[m] = F(F(1.0) / F(np.sqrt(F(ms + F(eps)))))
        for k in range(K):
            t = F(Xw[m, k] * rn[m])
            xn[m, k] = t if gamma is None else F(t * gamma[k])
    return xn, rn


@pytest.mark.parametrize("M,K", [(3, 7), (2, 256), (2, 257), (3, 700)])
@pytest.mark.parametrize("with_gamma", [True, False])
def test_rms_norm_ref_is_the_plain_loop(tsg, M, K, with_gamma):
    rng = np.random.default_rng(M * K)
    X = (rng.standard_normal((M, K)) * 3).astype(F)
    g = rng.uniform(0.5, 1.5, size=K).astype(F) if with_gamma else None
    for eps in (1e-5, 1e-6):
        xn, rn = tsg.rms_norm_ref(X, g, eps)
        xl, rl = _loop(X, g, eps)
        assert xn.dtype == F and rn.dtype == F and xn.shape == (M, K) and rn.shape == (M,)
        assert np.array_equal(xn.view(np.uint32), xl.view(np.uint32))
        assert np.array_equal(rn.view(np.uint32), rl.view(np.uint32))


def test_rms_norm_ref_edge_cases(tsg):
    xn, rn = tsg.rms_norm_ref(np.zeros((3, 0), F), None, 1e-5)  # K = 0: no sum, no division
    assert xn.shape == (3, 0) and rn.shape == (3,) and np.isfinite(rn).all()
    q, d = tsg.act_quant_ref(xn)
    assert q.shape == (3, 0) and np.array_equal(d, np.full(3, F(1e-5) / F(127.0), F))
    X = np.zeros((2, 5), F)  # a zero row: rn = 1 / sqrt(eps), xn = +0
    X[1] = [3.0, -4.0, 0.0, 0.0, 0.0]
    g = np.array([1.0, 0.5, 2.0, 1.0, 1.0], F)
    xn, rn = tsg.rms_norm_ref(X, g, 1e-5)
    assert rn[0] == F(1.0) / np.sqrt(F(1e-5)) and not xn[0].any() and not np.signbit(xn[0]).any()
    # ss = 25, ms = 5, rn = 1 / sqrt(5 + eps)
    r1 = F(1.0) / np.sqrt(F(F(5.0) + F(1e-5)))
    assert rn[1] == r1 and xn[1, 0] == F(F(3.0) * r1) and xn[1, 1] == F(F(F(-4.0) * r1) * F(0.5))
    x0, r0 = tsg.rms_norm_ref(X, None, 1e-5)  # gamma None: one multiply
    assert np.array_equal(r0, rn) and x0[1, 1] == F(F(-4.0) * r1)
    for bad in (np.zeros((2, 2), np.float64), np.zeros(4, F)):
        with pytest.raises(tsg.TSGError):
            tsg.rms_norm_ref(bad, None, 1e-5)
    for bad_g in (np.ones(4, F), np.ones(5, np.float64)):
        with pytest.raises(tsg.TSGError):
            tsg.rms_norm_ref(X, bad_g, 1e-5)


def test_a_gaussian_x_tells_little(tsg):
    """Why the builder makes near-ties and picks rows from a pool: on a random
    X a wrong multiplication order changes (almost) no q and a wrong sum shape
    changes deq in a minority of rows."""
    K = 388
    X = np.random.default_rng(0).standard_normal((130, K)).astype(F)
    g = G._gamma(K)
    xn, rn = tsg.rms_norm_ref(X, g, G.EPS)
    q, deq = tsg.act_quant_ref(xn)
    for name, v in G.elem_variants(X, g, G.EPS).items():
        assert float(np.mean(v != q)) < 0.001, name
    for name, d in G.row_variants(X, g, G.EPS).items():
        if name != "serial sum":
            assert float(np.mean(d.view(np.uint32) != deq.view(np.uint32))) < 0.35, name


# every (M, K) the GPU file builds an X for: fp32 on all of them, the 16-bit types on the type shapes
TYPE_SHAPES = G.TYPE_SHAPES + [(16, 388, 301), (130, 193, 301)]
X_CASES = sorted({(M, K, "float32") for M, K, N, B in G.FAMILY_SHAPES} |
                 {(M, K, x) for M, K, N in TYPE_SHAPES for x in G.XDTYPES})


@pytest.mark.parametrize("M,K,xdtype", X_CASES)
def test_builder_input_conditions(tsg, M, K, xdtype):
    """_xn asserts them, with the shares in its messages: every tellable
    row-level variant is told apart by a row (M = 1: by the one row, all at
    once), each element-level variant by >= 5 % of an fp32 case's elements, the
    zero row and the tiny row are what the docstring says."""
    Xt, Xw, g, xn = G._xn(M, K, xdtype)
    assert str(Xt.dtype) == "torch." + xdtype and Xw.shape == xn.shape == (M, K) and g.shape == (K,)
    names = G.row_variant_names(K, xdtype)
    assert ("fma" in names) == (K > 256 and xdtype == "float32")
    deq = tsg.act_quant_ref(xn)[1]
    rv = G.row_variants(Xw, g, G.EPS)
    told = np.stack([rv[n].view(np.uint32) != deq.view(np.uint32) for n in names], axis=1)
    if M == 1:
        assert told[0].all(), dict(zip(names, told[0]))
    else:
        assert told.any(axis=0).all(), dict(zip(names, told.mean(axis=0)))


@pytest.mark.parametrize("M,K,N,B", G.FAMILY_SHAPES)
def test_builder_cases_on_the_family_shapes(tsg, M, K, N, B):
    case = G._ncase(M, K, N, "float32", "float32", B)
    want = case[9]
    assert len(want) == 4 and all(w.shape == (M, N) for w in want.values()) and case[8].shape == (M,)


@pytest.mark.parametrize("ydtype", G.YDTYPES)
@pytest.mark.parametrize("xdtype", G.XDTYPES)
@pytest.mark.parametrize("M,K,N", G.TYPE_SHAPES)
def test_builder_cases_on_the_type_shapes(tsg, M, K, N, xdtype, ydtype):
    case = G._ncase(M, K, N, xdtype, ydtype)
    assert case[9][(True, "plain")].dtype == (np.uint32 if ydtype == "float32" else np.uint16)


@pytest.mark.parametrize("M,K,N", G.TYPE_SHAPES)
def test_builder_cases_without_gamma_and_with_another_eps(tsg, M, K, N):
    base = G._ncase(M, K, N)[9][(True, "plain")]
    for kw in (dict(gamma=False), dict(eps=1e-6)):
        assert not np.array_equal(G._ncase(M, K, N, **kw)[9][(True, "plain")], base), kw


@pytest.mark.parametrize("name", NAMES)
def test_normquant_symbols_exported(tsg, name):
    assert name in tsg.EXPORTED_SYMBOLS
    assert hasattr(tsg.lib(), name)
    assert f"int {name}(" in open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()
    assert "rms_norm_ref" in dir(tsg)


def test_abi_version_is_still_2(tsg):
    assert "#define TSG_ABI_VERSION 2" in open(tsg.PKG_DIR + "/../include/ternary_spgemm.h").read()


@pytest.mark.parametrize("out", ["scale out", "none"])
def test_normquant_null_handle_is_an_argument_error(tsg, out):
    L = tsg.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    rs = p if out == "scale out" else None
    for xtype in (0, 1, 2, 3, 4, -1):
        for ytype in (0, 1, 2, 3, -1):
            for eps in (1e-5, 0.0, float("nan")):
                for g in (p, None):
                    assert L.tcsc_hip_gemm_dev_normquant(None, p, xtype, g, eps, rs, p, p, p, ytype, 4, 1, 4, 4,
                                                         None) == 1  # TSG_ERR_ARG
                    assert b"null handle" in L.tcsc_hip_last_error()
                    assert L.tcsc_hip_gemm_prelu_dev_normquant(None, p, xtype, g, eps, rs, p, p, p, p, ytype, 4, 1, 4,
                                                               4, None) == 1
                    assert b"null handle" in L.tcsc_hip_last_error()
    assert all(v == 0.0 for v in buf)


def test_python_wrappers_have_the_documented_signatures(tsg):
    dev = inspect.signature(tsg.TCSCDevice.gemm_dev_normquant)
    assert list(dev.parameters) == ["self", "dX", "xtype", "dgamma", "eps", "db", "dY", "ytype", "M", "stream",
                                    "dalpha", "ldY", "drow_scale_out", "dcol_scale"]
    assert dev.parameters["stream"].default == 0
    assert all(dev.parameters[k].default is None for k in ("dalpha", "ldY", "drow_scale_out", "dcol_scale"))
    tor = inspect.signature(tsg.TCSCDevice.gemm_torch_normquant)
    assert list(tor.parameters) == ["self", "X", "b", "gamma", "eps", "Y", "alpha", "out_dtype", "col_scale",
                                    "row_scale_out"]
    assert all(tor.parameters[k].default is None for k in ("Y", "alpha", "out_dtype", "col_scale", "row_scale_out"))
    assert list(inspect.signature(tsg.rms_norm_ref).parameters) == ["Xw", "gamma", "eps"]
