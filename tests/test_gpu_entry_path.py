"""The four kernels on one small handle, as the round-end smoke check runs
them (M = 600 pinned to the 128-row image, M = 96 on the 64-row image, M = 5
on the walk, M = 1 on the producer/consumer walk), each bit for bit against
the BaseTCSC oracle (comp.h:25-69) with integer and order-sensitive X.  Since
round 5 registration compiles the 64-row image, so the 128-row one is built
by the pinned call itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_four_kernels_on_one_handle(tsg, oracle_mod):
    import torch
    O = oracle_mod
    K, N, s = 700, 300, 4
    t = O.tcsc_encode(O.gen_ternary(K, N, s, 1234))
    h = tsg.TCSCDevice(*t.arrays, K, N, device=0)
    info = h.info()  # the registration image: the 64-row image's 128 x 8
    assert (info["tile_rows"], info["tile_cols"], info["chunk_rows"]) == (64, 1024, 188)
    b = np.linspace(-3, 3, N).astype(np.float32)
    ran = []
    for M in (600, 96, 5, 1):
        h.set_small_m(1 if M >= 96 else 0)
        h.set_tile_rows(128 if M == 600 else 0)
        for X in (O.init_x_int(M, K, 1), O.init_x_frac(M, K, 2)):
            Y = h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
            assert np.array_equal(Y.view(np.uint32), O.base_tcsc(X, t, b).view(np.uint32)), h.call_kernel(M)
        ran.append(h.call_kernel(M))
    assert ran == ["tsg_jit_kernel", "tsg_jit64_kernel", "tsg_tcsc_ell_kernel", "tsg_tcsc_ell_pc_kernel"], ran
    h.close()


def test_handle_queries_are_the_host_plan(tsg, oracle_mod):
    """A handle's per-call queries and the host-only plan (tsg_call_plan) are
    one function (tsg_plan.cpp plan_call): an unpinned plain-TCSC handle
    answers what call_plan answers for its K, N, nnz.  At K = 256, N = 1024,
    s = 4 the M list reaches the producer/consumer walk (M = 1, 4), the walk
    (5, 16) and the 64-row image on 8 x 4 (33, 64, 65, 300) and on 16 x 8
    (1100); one M of each family runs, every row bit for bit against the
    oracle."""
    import torch
    O = oracle_mod
    K, N, s = 256, 1024, 4
    arrs = tsg.gen_tcsc(K, N, s, 7)
    nnz = len(arrs[2]) + len(arrs[3])
    h = tsg.TCSCDevice(*arrs, K, N, device=0)
    info = h.info()
    assert info["nnz_pos"] + info["nnz_neg"] == nnz
    t = O.TCSC(*arrs, K, N)
    b = np.linspace(-3, 3, N).astype(np.float32)
    ran = {}
    for M in (1, 4, 5, 16, 33, 64, 65, 300, 1100):
        p = tsg.call_plan(K, N, nnz, M)
        assert h.call_kernel(M) == p["kernel"], M
        assert h.call_far(M) == p["far"], M
        if p["kernel"] in ("tsg_jit_kernel", "tsg_jit64_kernel"):
            assert (h.jit_width(M), h.jit_waves(M)) == (p["width"], p["waves"]), M
            assert h.call_tile_rows(M) == (64 if p["kernel"] == "tsg_jit64_kernel" else 128), M
        else:
            assert h.call_tile_rows(M) == 0, M
        ran.setdefault((p["kernel"], p["width"], p["waves"]), M)
    walks = [k for k in ran if k[0].startswith("tsg_tcsc_ell")]
    images = [k for k in ran if k[0].startswith("tsg_jit")]
    assert walks and len(images) >= 2 and any(k[0] == "tsg_jit64_kernel" for k in images), ran
    for M in ran.values():
        X = O.init_x_frac(M, K, M)
        Y = h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        assert np.array_equal(Y.view(np.uint32), O.base_tcsc(X, t, b).view(np.uint32)), (M, h.call_kernel(M))
    h.close()
