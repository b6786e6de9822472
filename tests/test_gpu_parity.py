"""GPU parity: the HIP path (through the C-ABI) against the reference's golden
vectors and the CPU oracle, bit for bit (integer AND non-integer X, so the
accumulation order of BaseTCSC, cpp_impl/comp.h:37-63, is pinned).

All cases call libternary_spgemm.so; nothing here falls back to the CPU.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden_small

pytestmark = pytest.mark.gpu


def _sha(*arrays) -> str:
    return hashlib.sha256(np.concatenate([np.ascontiguousarray(a).ravel() for a in arrays]).tobytes()).hexdigest()


def _bits_eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def small():
    return load_golden_small()


def _case_prefixes(z):
    return sorted({k.split("_")[0] + "_" for k in z.files})


def test_kat_4x4(tsg):
    kat = json.load(open(os.path.join(GOLDEN, "kat_tcsc_4x4.json")))
    h = tsg.TCSCDevice(kat["col_start_pos"], kat["col_start_neg"], kat["row_index_pos"],
                       kat["row_index_neg"], 4, 4)
    Y = h.gemm(np.array(kat["X"], np.float32), np.array(kat["b"], np.float32))
    assert _bits_eq(Y, kat["Y_base_tcsc_oracle"])
    assert np.array_equal(h.to_dense(), np.array(kat["W"]))


def test_golden_small(tsg, small):
    z = small
    for p in _case_prefixes(z):
        M, K, N, s, seed = (int(v) for v in z[p + "shape"])
        pos = np.unpackbits(z[p + "Wpos_bits"])[: K * N].reshape(K, N).astype(np.int32)
        neg = np.unpackbits(z[p + "Wneg_bits"])[: K * N].reshape(K, N).astype(np.int32)
        W = pos - neg
        if p + "csp" in z.files:
            h = tsg.TCSCDevice(z[p + "csp"], z[p + "csn"], z[p + "rip"], z[p + "rin"], K, N)
        else:
            h = tsg.TCSCDevice.from_dense(W)
        assert np.array_equal(h.to_dense(), W)
        b, alpha = z[p + "b"], z[p + "alpha"]
        assert _bits_eq(h.gemm(z[p + "X"], b), z[p + "Y_ref_gemm"]), p
        assert _bits_eq(h.gemm(z[p + "Xfrac"], b), z[p + "Yfrac_oracle"]), p
        assert _bits_eq(h.gemm_prelu(z[p + "X"], b, alpha), z[p + "Y_ref_gemm_prelu"]), p
        assert _bits_eq(h.gemm_prelu(z[p + "Xfrac"], b, alpha), z[p + "Yfrac_prelu_oracle"]), p
        h.close()


EDGE = [
    # (M, K, N, s): ragged tiles (128-row M tile, 128-col N tile, 128-row K chunk)
    (1, 1, 1, 1), (1, 64, 96, 2), (2, 127, 3, 1), (127, 129, 63, 4), (128, 128, 64, 2),
    (129, 257, 65, 4), (300, 1000, 129, 16), (64, 513, 1000, 8), (5, 4096, 17, 4),
    (200, 96, 2048, 4),
]


@pytest.mark.parametrize("small_m", [0, 1], ids=["auto", "jit-only"])
@pytest.mark.parametrize("M,K,N,s", EDGE)
def test_edges_vs_oracle(tsg, oracle_mod, M, K, N, s, small_m):
    """Ragged shapes, automatic kernel choice (the small-M kernel for M <= 16)
    and the weight-compiled kernel forced for every M."""
    O = oracle_mod
    W = O.gen_ternary(K, N, s, M * 7 + K)
    t = O.tcsc_encode(W)
    h = tsg.TCSCDevice(*t.arrays, K, N)
    h.set_small_m(small_m)
    b = (np.arange(N, dtype=np.float32) - N / 2) * 0.37
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    for X in (O.init_x_int(M, K, 5), O.init_x_frac(M, K, 6)):
        assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, t, b))
        assert _bits_eq(h.gemm_prelu(X, b, alpha), O.base_tcsc_prelu(X, t, b, alpha))


@pytest.mark.parametrize("width", [64, 32, 16, 8])
def test_every_stream_width_vs_oracle(tsg, oracle_mod, width):
    """Each jit stream width (tcsc_hip_set_jit_width) pinned, on ragged shapes,
    bit for bit against the oracle (integer and order-sensitive X, PReLU)."""
    O = oracle_mod
    for M, K, N, s in ((1, 64, 96, 2), (129, 257, 65, 4), (300, 1000, 129, 16), (200, 96, 700, 4)):
        W = O.gen_ternary(K, N, s, M + K + width)
        t = O.tcsc_encode(W)
        h = tsg.TCSCDevice(*t.arrays, K, N)
        h.set_small_m(1)  # the weight-compiled kernel for every M (M = 1 would take the small-M kernel)
        h.set_tile_rows(128)  # the 128-row image (the 64-row one: tests/test_gpu_rows64.py)
        h.set_jit_width(width)
        assert h.jit_width(M) == width and h.call_kernel(M) == "tsg_jit_kernel"
        b = (np.arange(N, dtype=np.float32) - N / 2) * 0.37
        alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
        for X in (O.init_x_int(M, K, 5), O.init_x_frac(M, K, 6)):
            assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, t, b)), (M, K, N, s, width)
            assert _bits_eq(h.gemm_prelu(X, b, alpha), O.base_tcsc_prelu(X, t, b, alpha))
        h.close()


def test_far_image_vs_oracle(tsg, oracle_mod):
    """The far-X^T image (tcsc_hip_set_far: no code touches, non-temporal X^T
    staging) on ragged shapes, bit for bit against the oracle and the default
    image; the automatic rule keeps small calls on the default image."""
    O = oracle_mod
    for M, K, N, s in ((129, 257, 600, 4), (300, 1000, 1100, 16), (5, 96, 520, 2)):
        W = O.gen_ternary(K, N, s, 3 * M + K)
        t = O.tcsc_encode(W)
        h = tsg.TCSCDevice(*t.arrays, K, N)
        h.set_small_m(1)
        h.set_tile_rows(128)
        h.set_jit_width(64)
        assert not h.call_far(M)  # X^T far below the Infinity Cache: the default image
        b = (np.arange(N, dtype=np.float32) - N / 3) * 0.21
        alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
        Xs = (O.init_x_int(M, K, 15), O.init_x_frac(M, K, 16))
        base = [h.gemm(X, b) for X in Xs]
        h.set_far(2)
        assert h.call_far(M) and h.call_kernel(M) == "tsg_jit_kernel"
        for X, Yb in zip(Xs, base):
            Y = h.gemm(X, b)
            assert _bits_eq(Y, Yb) and _bits_eq(Y, O.base_tcsc(X, t, b)), (M, K, N, s)
            assert _bits_eq(h.gemm_prelu(X, b, alpha), O.base_tcsc_prelu(X, t, b, alpha))
        h.set_far(1)
        assert not h.call_far(M)
        with pytest.raises(tsg.TSGError):
            h.set_far(3)
        h.close()


def test_auto_width_small_m(tsg, oracle_mod):
    """Automatic width: narrow streams for small M, 128 columns per wave (the
    64-row image) at config 3's M; one handle switching widths and images
    call by call stays bit-exact."""
    O = oracle_mod
    K, N = 1024, 4096
    t = O.tcsc_encode(O.gen_ternary(K, N, 4, 77))
    h = tsg.TCSCDevice(*t.arrays, K, N)
    h.set_small_m(1)
    assert h.jit_width(32) < 64 and h.jit_width(8192) == 128 and h.call_kernel(8192) == "tsg_jit64_kernel"
    b = np.full(N, 2.0, np.float32)
    for M in (32, 8192, 7):
        X = O.init_x_frac(M, K, M)
        Y = h.gemm(X, b)
        rows = slice(0, 64)
        assert _bits_eq(Y[rows], O.base_tcsc(X[rows], t, b)), M
    with pytest.raises(tsg.TSGError):
        h.set_jit_width(24)
    h.close()


@pytest.mark.parametrize("M,K,N,shape", [(512, 4096, 4096, (16, 4)), (256, 2048, 16384, (32, 4)),
                                         (1024, 1024, 4096, (32, 4)), (4096, 1024, 16384, (64, 8)),
                                         (300, 1000, 700, None)])
def test_auto_shape_mid_m(tsg, oracle_mod, M, K, N, shape):
    """The automatic (width, waves) shape of the 128-row image at mid M (pinned:
    the automatic choice runs the 64-row image up to M = 512): 4-wave
    workgroups where they double the workgroups of a wider stream (configs[1]
    on this image takes 16 x 4); every launched shape bit for bit on sampled
    rows, and one handle switching shapes call by call."""
    import torch
    O = oracle_mod
    arrs = tsg.gen_tcsc(K, N, 4, 5)
    h = tsg.TCSCDevice(*arrs, K, N)
    h.set_small_m(1)
    h.set_tile_rows(128)
    if shape is not None:
        assert (h.jit_width(M), h.jit_waves(M)) == shape
    b = torch.linspace(-2, 2, N, device="cuda")
    for m in (M, 128 * 12 + 3, M // 2 + 1):
        Xn = O.init_x_frac(m, K, m)
        Y = h.gemm_torch(torch.from_numpy(Xn).cuda(), b).cpu().numpy()
        rows = np.unique(np.r_[0, 1, 127, m // 2, m - 1].clip(0, m - 1))
        ref = O.base_tcsc(np.ascontiguousarray(Xn[rows]), O.TCSC(*arrs, K, N), b.cpu().numpy())
        assert _bits_eq(Y[rows], ref), (m, h.jit_width(m), h.jit_waves(m))
    h.close()


def test_structural_edges(tsg, oracle_mod):
    """All-zero W, fully dense ternary W, empty and full columns, K=0."""
    O = oracle_mod
    rng = np.random.default_rng(3)
    for W in (np.zeros((300, 70), np.int32),
              rng.integers(-1, 2, size=(260, 150)).astype(np.int32),
              np.ones((129, 5), np.int32), -np.ones((129, 5), np.int32)):
        K, N = W.shape
        W[:, 0] = 0  # an empty column
        t = O.tcsc_encode(W)
        h = tsg.TCSCDevice(*t.arrays, K, N)
        b = rng.standard_normal(N).astype(np.float32)
        for M in (131, 7):  # the weight-compiled and the small-M kernel
            X = O.init_x_frac(M, K, 9)
            assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, t, b))
    # K = 0: the chain is the +0.0 start, Y = 0 + b
    h = tsg.TCSCDevice(np.zeros(4, np.int32), np.zeros(4, np.int32), [], [], 0, 3)
    Y = h.gemm(np.zeros((5, 0), np.float32), np.array([1.5, -2.0, 0.0], np.float32))
    assert _bits_eq(Y, np.tile(np.array([1.5, -2.0, 0.0], np.float32), (5, 1)))


def test_config2_golden_hash(tsg):
    """BASELINE.json configs[1]: M=512 K=4096 N=4096 s=4; Y hash from the
    reference's dense GEMM (tests/golden/ref_hashes.json)."""
    g = json.load(open(os.path.join(GOLDEN, "ref_hashes.json")))["config2"]
    M, K, N, s = g["M"], g["K"], g["N"], g["s"]
    arrs = tsg.gen_tcsc(K, N, s, g["seed_w"])
    assert _sha(*arrs) == g["sha256_tcsc"]
    h = tsg.TCSCDevice(*arrs, K, N)
    X = tsg.gen_x(M, K, g["seed_x"])
    Y = h.gemm(X, np.full(N, 2.0, np.float32))
    assert Y[0, 0] == g["Y_0_0"] and Y[-1, -1] == g["Y_last"]
    assert _sha(Y) == g["sha256_Y"]


def test_config3_full_size(tsg, oracle_mod):
    """BASELINE.json configs[2] at full size (M=4096 K=4096 N=16384 s=4):
    sampled rows equal the reference GEMM (hash) for integer X, and the
    oracle bit for bit for non-integer X (order at full size)."""
    import torch
    O = oracle_mod
    g = json.load(open(os.path.join(GOLDEN, "ref_hashes.json")))["config3_rows"]
    M, K, N, s = g["M"], g["K"], g["N"], g["s"]
    arrs = tsg.gen_tcsc(K, N, s, g["seed_w"])
    assert _sha(*arrs) == g["sha256_tcsc"]
    h = tsg.TCSCDevice(*arrs, K, N)
    rows = np.array(g["rows"])
    b = np.full(N, 2.0, np.float32)
    dev = torch.device("cuda:0")
    bt = torch.from_numpy(b).to(dev)
    X = torch.from_numpy(tsg.gen_x(M, K, g["seed_x"])).to(dev)
    Y = h.gemm_torch(X, bt)
    torch.cuda.synchronize()
    assert _sha(Y[torch.from_numpy(rows).to(dev)].cpu().numpy()) == g["sha256_Y_rows"]
    # non-integer X, order pinned against the oracle on sampled rows
    Xf = O.init_x_frac(M, K, 77)
    Yf = h.gemm_torch(torch.from_numpy(Xf).to(dev), bt).cpu().numpy()
    t = O.TCSC(*arrs, K, N)
    sub = rows[:8]
    assert _bits_eq(Yf[sub], O.base_tcsc(np.ascontiguousarray(Xf[sub]), t, b))
    # size-independent property: Y is fully overwritten (no stale values)
    Y2 = torch.full((M, N), float("nan"), device=dev)
    h.gemm_torch(X, bt, Y=Y2)
    torch.cuda.synchronize()
    assert torch.equal(Y2, Y)


def test_device_path_streams_and_timing(tsg, oracle_mod):
    import torch
    O = oracle_mod
    K, N, M = 700, 513, 333
    t = O.tcsc_encode(O.gen_ternary(K, N, 4, 1))
    h = tsg.TCSCDevice(*t.arrays, K, N)
    h.reserve(M)
    X = O.init_x_frac(M, K, 2)
    b = np.linspace(-1, 1, N).astype(np.float32)
    ref = O.base_tcsc(X, t, b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        Xd, bd = torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()
        h.set_timing(True)
        for _ in range(3):
            Y = h.gemm_torch(Xd, bd)
    s.synchronize()
    ms, n = h.kernel_time(reset=True)
    assert n == 3 and ms > 0
    assert _bits_eq(Y.cpu().numpy(), ref)
    info = h.info()
    assert info["K"] == K and info["N"] == N and info["nnz_pos"] == len(t.row_index_pos)
    assert info["tcsc_bytes"] == t.size_bytes()


def test_errors_are_loud(tsg, oracle_mod):
    O = oracle_mod
    t = O.tcsc_encode(O.gen_ternary(64, 32, 4, 1))
    h = tsg.TCSCDevice(*t.arrays, 64, 32)
    X = np.zeros((4, 64), np.float32)
    Y = np.zeros((4, 32), np.float32)
    b = np.zeros(32, np.float32)
    with pytest.raises(tsg.TSGError) as e:
        h(X, b, Y, 4, 31, 64)  # N mismatch
    assert e.value.code == 1
    with pytest.raises(tsg.TSGError):
        tsg.TCSCDevice(t.col_start_pos, t.col_start_neg, t.row_index_pos[::-1].copy(),
                       t.row_index_neg, 64, 32)
    h(X, b, Y, 0, 32, 64)  # M = 0 is a no-op, as the reference's empty loop


def test_csc_packed_input(tsg, oracle_mod):
    """readme.md:111 format in, identical BaseTCSC chains out."""
    O = oracle_mod
    for s in (2, 4, 8, 16):
        K, N, M = 900, 700, 130
        W = O.gen_ternary(K, N, s, s)
        t = O.tcsc_encode(W)
        h = tsg.TCSCDevice.from_csc_packed(*O.csc_packed_encode(W), K, N)
        X = O.init_x_frac(M, K, s)
        b = np.linspace(-1, 1, N).astype(np.float32)
        assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, t, b))


def test_default_is_weight_compiled(tsg, oracle_mod):
    O = oracle_mod
    t = O.tcsc_encode(O.gen_ternary(200, 70, 4, 3))
    h = tsg.TCSCDevice(*t.arrays, 200, 70)
    assert h.kernel_name() == "tsg_jit_kernel"


def test_rx_kernel_family(tsg, oracle_mod, monkeypatch):
    """The register-X kernel (TSG_KERNEL=rx at registration; also the fallback
    for W too large for one compiled image) stays bit-exact too."""
    monkeypatch.setenv("TSG_KERNEL", "rx")
    O = oracle_mod
    for M, K, N, s in [(129, 257, 65, 4), (300, 1000, 129, 16), (5, 1100, 300, 2)]:
        t = O.tcsc_encode(O.gen_ternary(K, N, s, M + K))
        h = tsg.TCSCDevice(*t.arrays, K, N)
        assert h.kernel_name() == "tsg_tcsc_rx_kernel"
        b = np.linspace(-1, 1, N).astype(np.float32)
        alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
        X = O.init_x_frac(M, K, 3)
        assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, t, b))
        assert _bits_eq(h.gemm_prelu(X, b, alpha), O.base_tcsc_prelu(X, t, b, alpha))
        h.close()


def test_failed_image_load_falls_back_to_rx(tsg, oracle_mod, monkeypatch, capfd):
    """A weight-compiled image the loader cannot build (here: its dispatcher
    template is missing) registers on the rx kernel with a logged warning,
    instead of failing the registration; asking for jit explicitly still fails."""
    O = oracle_mod
    monkeypatch.setenv("TSG_JIT_DIR", "/nonexistent-tsg-jit-dir")
    K, N, M = 300, 200, 70
    t = O.tcsc_encode(O.gen_ternary(K, N, 4, 5))
    h = tsg.TCSCDevice(*t.arrays, K, N)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel"
    assert "falling back to the rx kernel" in capfd.readouterr().err
    X = O.init_x_frac(M, K, 4)
    b = np.linspace(-1, 1, N).astype(np.float32)
    assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, t, b))
    h.close()
    monkeypatch.setenv("TSG_KERNEL", "jit")
    with pytest.raises(tsg.TSGError, match="cannot open jit template"):
        tsg.TCSCDevice(*t.arrays, K, N)


def test_missing_64row_dispatcher_falls_back_to_128row(tsg, oracle_mod, monkeypatch, capfd, tmp_path):
    """VERDICT r04 "next" 5 / ADVICE r04: with a dispatcher directory that
    holds only the 128-row template (an older install), a configs[2]-shaped
    call -- the 64-row 128 x 8 image by default -- runs the 128-row image
    registered at tcsc_hip_create, with a warning on stderr, and is still
    bit-exact; later calls and the plan queries report the image that runs.
    A pinned 64-row image fails loudly instead."""
    import shutil
    import torch
    O = oracle_mod
    libdir = os.path.join(os.path.dirname(tsg.LIB_PATH))
    shutil.copy(os.path.join(libdir, "tsg_jit.co"), tmp_path / "tsg_jit.co")
    monkeypatch.setenv("TSG_JIT_DIR", str(tmp_path))
    M, K, N, s = 4096, 4096, 2048, 4
    csp, csn, rip, rin = tsg.gen_tcsc(K, N, s, 42)
    t = O.TCSC(csp, csn, rip, rin, K, N)
    h = tsg.TCSCDevice(csp, csn, rip, rin, K, N)
    assert h.kernel_name() == "tsg_jit_kernel"          # registration: the 128-row image loaded
    assert h.call_kernel(M) == "tsg_jit64_kernel"       # the automatic plan picks the 64-row image
    X = O.init_x_frac(M, K, 31)
    b = (np.arange(N, dtype=np.float32) % 13 - 6) * np.float32(0.37)
    Y = h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    assert "running the 128-row 64 x 8 image instead" in capfd.readouterr().err
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    ref = O.base_tcsc(X, t, b, threads=16)
    assert _bits_eq(Y, ref)
    Y2 = h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
    assert _bits_eq(Y2, ref) and "warning" not in capfd.readouterr().err  # no retry per call
    h.set_tile_rows(64)  # pinned: no fallback
    with pytest.raises(tsg.TSGError, match="cannot open jit template"):
        h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda())
    h.close()


def test_gpu_encoder_matches_host_ctor(tsg, oracle_mod):
    """GPU-side TCSC encoder == the TCSC ctor (TCSC.h:13-41)
    array for array, incl. the 4x4 KAT, values other than +-1 (zeros there),
    empty columns and a registration through it."""
    import torch
    O = oracle_mod
    kat = json.load(open(os.path.join(GOLDEN, "kat_tcsc_4x4.json")))
    cases = [np.array(kat["W"], np.int32), O.gen_ternary(300, 70, 4, 1), O.gen_ternary(1000, 513, 2, 2),
             O.gen_ternary(129, 1, 16, 3), np.zeros((5, 7), np.int32)]
    odd = O.gen_ternary(64, 33, 4, 4)
    odd[::7, ::3] = 2
    odd[3::11, 1::5] = -5
    cases.append(odd)
    for W in cases:
        t = O.tcsc_encode(np.where(np.abs(W) == 1, W, 0).astype(np.int32))
        g = tsg.encode_dense_torch(torch.from_numpy(np.ascontiguousarray(W)).cuda())
        for a, b in zip(t.arrays, g):
            assert np.array_equal(np.asarray(a, np.int32), b.cpu().numpy())
    W = O.gen_ternary(700, 300, 4, 9)
    h = tsg.TCSCDevice.from_dense_torch(torch.from_numpy(W).cuda())
    X = O.init_x_frac(77, 700, 1)
    b = np.linspace(-1, 1, 300).astype(np.float32)
    assert _bits_eq(h.gemm(X, b), O.base_tcsc(X, O.tcsc_encode(W), b))


@pytest.mark.parametrize("M,K,N,s,B", [(5, 70, 33, 2, 16), (130, 1000, 520, 4, 64), (17, 300, 64, 8, 100),
                                       (131, 1100, 700, 4, 512), (9, 96, 70, 2, 1), (4, 10, 5, 2, 32),
                                       (256, 4096, 1024, 4, 512)])
def test_blocked_tcsc_vs_oracle(tsg, oracle_mod, M, K, N, s, B):
    """BlockedTCSC<B> (BlockedTCSC.h:15-41) registered as is, BaseBlockedTCSC
    (comp.h:607-658) order bit for bit: integer X (== BaseTCSC / the dense GEMM,
    SURVEY 8f rank 2's pin) and order-sensitive X.  B = 512 is the reference's
    BLOCK_SIZE (main.cpp:7); K % B != 0 drops the tail rows as the ctor does."""
    O = oracle_mod
    W = O.gen_ternary(K, N, s, M + K + B)
    blk = O.blocked_tcsc_encode(W, B)
    h = tsg.TCSCDevice.from_blocked(*blk, K, N, B)
    assert h.kernel_name() == "tsg_jit_kernel"
    Wt = W.copy()
    Wt[(K // B) * B:] = 0
    assert np.array_equal(h.to_dense(), Wt)
    assert h.info()["tcsc_bytes"] == 4 * (len(blk[0]) + len(blk[1]) + len(blk[2]) + len(blk[3]))
    b = np.linspace(-2, 2, N).astype(np.float32)
    Xi, Xf = O.init_x_int(M, K, 5), O.init_x_frac(M, K, 6)
    assert _bits_eq(h.gemm(Xi, b), O.base_blocked_tcsc(Xi, blk, b, K, N, B))
    assert _bits_eq(h.gemm(Xi, b), O.base_tcsc(Xi, O.tcsc_encode(Wt), b))
    assert _bits_eq(h.gemm(Xf, b), O.base_blocked_tcsc(Xf, blk, b, K, N, B))
    h.close()


def test_blocked_tcsc_kat(tsg, oracle_mod):
    """plots/data_example_image/blocked.py:12-30 (4x4, B = 2)."""
    O = oracle_mod
    kat = json.load(open(os.path.join(GOLDEN, "kat_blocked_4x4_B2.json")))
    W = np.array(kat["W"], np.int32)
    blk = O.blocked_tcsc_encode(W, 2)
    h = tsg.TCSCDevice.from_blocked(*blk, 4, 4, 2)
    X = np.array(kat["X"], np.float32)
    b = np.zeros(4, np.float32)
    assert _bits_eq(h.gemm(X, b), O.base_blocked_tcsc(X, blk, b, 4, 4, 2))


def test_blocked_tcsc_errors(tsg, oracle_mod, monkeypatch):
    O = oracle_mod
    blk = O.blocked_tcsc_encode(O.gen_ternary(64, 8, 2, 1), 16)
    with pytest.raises(tsg.TSGError):
        tsg.TCSCDevice.from_blocked(*blk, 64, 8, 0)
    with pytest.raises(tsg.TSGError, match="malformed BlockedTCSC"):
        tsg.TCSCDevice.from_blocked(*blk, 64, 8, 32)  # arrays are for B = 16
    monkeypatch.setenv("TSG_KERNEL", "rx")
    with pytest.raises(tsg.TSGError, match="jit kernel only"):
        tsg.TCSCDevice.from_blocked(*blk, 64, 8, 16)


def test_plugin_against_reference_headers():
    """oracle/_ref/plugin_ref_check (built in the build container from the
    reference's own common.h / DataStructureInterface.hpp / sparseUtils.h,
    tests/test_integration_ref.py): the reference's generateSparseMatrix, TCSC
    and BlockedTCSC<512> ctors, dense GEMM / GEMM_PreLU and compare_results
    around the registered HIP comp_funcs, as main.cpp:192-247 runs them."""
    import subprocess
    from conftest import REPO
    exe = os.path.join(REPO, "oracle", "_ref", "plugin_ref_check")
    if not os.path.exists(exe):
        pytest.skip("plugin_ref_check not built (needs the reference headers in the build container)")
    # main.cpp:49-52 argv; the last two are BASELINE configs[0] (M=32 K=1024
    # N=4096 s=4, "./sparseGEMM.out -correctness") and configs[1] (M=512
    # K=4096 N=4096 s=4): the reference's own generator, ctors, serial dense
    # GEMM and compare_results (main.cpp:192-247) around the HIP comp_funcs
    # "-perf" (configs[0] and configs[1]) then runs the reference's own
    # benchmark loop (main.cpp:253-293) with its perf_test (perf.cpp compiled
    # unmodified, -DCALIBRATE rdtsc path): "Running: / cycles / Speedup is:"
    # per comp_func, the speedup relative to "BaseTCSC" (main.cpp:10)
    import re
    for argv in ([], ["-M", "130", "-K", "1100", "-N", "300", "-s", "2"],
                 ["-M", "32", "-K", "1024", "-N", "4096", "-s", "4", "-perf"],
                 ["-M", "512", "-K", "4096", "-N", "4096", "-s", "4", "-perf"]):
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stdout + r.stderr
        for name in ("BaseTCSC", "HipBaseTCSC", "HipBaseBlockedTCSC", "BaseTCSC_PreLU", "HipBaseTCSC_PreLU"):
            assert f"Test case {name} passed!" in r.stdout, r.stdout
        assert "DataStructureInterface round trip passed!" in r.stdout
        if "-perf" not in argv:
            continue
        # main.cpp:257-263's three lines per function, as run_benchmark.py:63-67 scrapes them
        runs = re.findall(r"Running: \x1b\[31m(\w+)\x1b\[0m\n([0-9.e+]+) cycles\nSpeedup is: \x1b\[32m([0-9.e+]+)\x1b\[0m",
                          r.stdout)
        got = {name: (float(cyc), float(sp)) for name, cyc, sp in runs}
        assert sorted(got) == sorted(["BaseTCSC", "HipBaseTCSC", "HipBaseBlockedTCSC", "BaseTCSC_PreLU",
                                      "HipBaseTCSC_PreLU"]), r.stdout
        assert got["BaseTCSC"][1] == 1.0 and got["BaseTCSC_PreLU"][1] == 1.0
        for name in ("HipBaseTCSC", "HipBaseBlockedTCSC", "HipBaseTCSC_PreLU"):
            assert got[name][0] > 0 and got[name][1] > 1.0, (name, got[name])  # the GPU beats one CPU core
        out = os.environ.get("TSG_REF_PERF_OUT")  # keep the report (profiles/r05_ref_perf_test.txt)
        if out:
            with open(out, "a") as f:
                f.write(f"$ oracle/_ref/plugin_ref_check {' '.join(argv)}\n{r.stdout}\n")
